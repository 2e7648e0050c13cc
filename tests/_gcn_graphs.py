"""The graphs and inputs shared by the tests of ctgcn_gcn.hip's gather (test_gpu_gcn_layer.py, test_gpu_gcn_conv.py)."""
import numpy as np
import scipy.sparse as sp

DEV = "cuda:0"
N = 67                                   # not a multiple of the rows per block of any lane-group width (64, 32, 16, 8, 4)
WIDTHS = (4, 8, 16, 32, 64)              # lanes per row: ceil(d / 4) (float4) or d (scalar) rounded up to one of these; the graphs' row lengths
# the kernel's lane-group width follows from d.  float4 (d % 4 == 0): 12 -> 4 lanes, 24 -> 8 (partial group), 48 -> 16, 128 -> 32 (full
# group), 132 -> 64 (partial).  scalar: 1 -> 4, 6 -> 8, 10 -> 16, 27 -> 32, 130 -> 64 and three passes.
DIMS = (1, 6, 10, 12, 24, 27, 48, 128, 130, 132)
_graphs = {}


def havel_hakimi(deg):
    """edges of a simple graph with the given degree sequence, or None when there is none"""
    left = [[d, i] for i, d in enumerate(deg)]
    edges = []
    while True:
        left.sort(key=lambda p: (-p[0], p[1]))
        d, i = left[0]
        if d == 0:
            return edges
        if d > len(left) - 1:
            return None
        left[0][0] = 0
        for other in left[1:d + 1]:
            if other[0] == 0:
                return None
            other[0] -= 1
            edges.append((i, other[1]))


def symmetric_graph(width, float32_values=False):
    """float64 symmetric CSR [N, N] with values of both signs whose rows hold 0, 1, width - 1, width, width + 1, 8 and 9 entries
    (rows 0..6) among others; stored entries = neighbours + an optional diagonal entry.  float32_values: the values rounded to float32,
    for a matrix that goes to the device as it is."""
    if (width, float32_values) in _graphs:
        return _graphs[width, float32_values]
    want = [0, 1, width - 1, width, width + 1, 8, 9]
    for seed in range(100):
        rng = np.random.default_rng(1000 * width + seed)
        length = np.array(want + list(rng.integers(2, 14, N - len(want))))
        diag = (length > 0) & (rng.random(N) < 0.5)
        diag[1] = True                                      # the row of one entry is its diagonal
        deg = length - diag
        if deg.sum() % 2:
            deg[-1] += 1
            length[-1] += 1
        edges = havel_hakimi(list(deg))
        if edges is not None:
            break
    else:
        raise AssertionError("no graph with the wanted row lengths")
    u, v = np.array(edges).T
    w = rng.uniform(0.2, 1.0, len(u)) * rng.choice([-1.0, 1.0], len(u))
    dg = np.nonzero(diag)[0]
    m = sp.coo_matrix((np.concatenate([w, w, rng.uniform(-1.0, 1.0, len(dg))]), (np.concatenate([u, v, dg]), np.concatenate([v, u, dg]))),
                      shape=(N, N)).tocsr()
    m.sort_indices()
    if float32_values:
        m.data = m.data.astype(np.float32).astype(np.float64)
    assert abs(m - m.T).sum() == 0 and list(np.diff(m.indptr)[:7]) == want
    _graphs[width, float32_values] = m
    return m


def gcn_adj(m, long_threshold=None):
    from ctgcn_amd import ops
    return ops.GcnAdj.from_scipy(m, DEV, long_threshold=long_threshold)


def dense(shape, seed):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)
