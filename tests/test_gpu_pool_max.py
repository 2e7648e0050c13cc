"""ops.pool_max (ctgcn_pool.hip) against numpy: the maximum over each row's stored entries and the index that holds it, at every
dispatch boundary (scalar and float4 rows, every lane-group width, long rows in pieces), empty and all-negative rows, ties (the lower
column index wins, also across two pieces of a long row, and takes the whole gradient), and the backward's pull over the transposed
CSR against a host loop over arg.  A maximum is one of its inputs, so the forward is compared exactly; the backward adds fp32 values
in another order than the host loop's float64 and is held to conftest.close_scaled's tolerance.  Every output is repeated and compared
bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

from _gcn_graphs import DEV, DIMS, N, WIDTHS, dense, gcn_adj
from conftest import close_scaled
from test_gpu_gcn_conv import directed_graph, f64, graph, tolerance

pytestmark = pytest.mark.gpu


def reference(m, S):
    """(Y, arg) by a host loop: the first (lowest) column among equal maxima; 0 and -1 for an empty row"""
    S = np.asarray(S)
    n, d = S.shape
    Y, arg = np.zeros((n, d), dtype=S.dtype), np.full((n, d), -1, dtype=np.int32)
    for i in range(n):
        cols = m.indices[m.indptr[i]:m.indptr[i + 1]]
        if len(cols):
            g = S[cols]
            pick = g.argmax(axis=0)                                # numpy's argmax: the first among equals; cols are ascending
            Y[i], arg[i] = g[pick, np.arange(d)], cols[pick]
    return Y, arg


def pull_reference(arg, dY):
    """dS[j, c] = sum_i [arg[i, c] == j] dY[i, c] in float64"""
    n, d = dY.shape
    dS = np.zeros((n, d))
    for c in range(d):
        hit = arg[:, c] >= 0
        np.add.at(dS[:, c], arg[hit, c], dY[hit, c].astype(np.float64))
    return dS


def check(m, adj, S, what):
    from ctgcn_amd import ops
    Y, arg = ops._pool_max_fwd(adj, S)
    ref, ref_arg = reference(m, S.cpu().numpy())
    assert arg.dtype == torch.int32 and np.array_equal(Y.cpu().numpy(), ref) and np.array_equal(arg.cpu().numpy(), ref_arg), what
    Y2, arg2 = ops._pool_max_fwd(adj, S)
    assert torch.equal(Y, Y2) and torch.equal(arg, arg2)
    dY = torch.from_numpy(dense(tuple(S.shape), S.shape[1] + 2)).to(DEV)
    dS = ops._pool_max_bwd(adj.transposed(), dY, arg)
    want = pull_reference(ref_arg, dY.cpu().numpy())
    print("  [tol] %-40s %.3f of the tolerance" % (what + " dS", float((np.abs(f64(dS) - want) / tolerance(want)).max())))
    close_scaled(f64(dS), want)
    assert torch.equal(dS, ops._pool_max_bwd(adj.transposed(), dY, arg))
    return Y, arg, dS


@pytest.mark.parametrize("d", DIMS)
def test_forward_and_backward_at_every_lane_group_width(d):
    for width in WIDTHS:
        m = graph(width)
        adj = gcn_adj(m)
        assert adj.long_rows is None and m.indptr[1] == 0
        s = dense((N, d), d)
        neg = int(np.argmax(np.diff(m.indptr) >= 3))              # a row of three entries or more: all of its neighbours negative
        s[m.indices[m.indptr[neg]:m.indptr[neg + 1]]] = -np.abs(s[m.indices[m.indptr[neg]:m.indptr[neg + 1]]]) - 0.5
        Y, arg, dS = check(m, adj, torch.from_numpy(s).to(DEV), "d %d width %d" % (d, width))
        assert not Y[0].any() and bool((arg[0] == -1).all())      # the empty row
        assert bool((Y[neg] < 0).all())                           # stays negative: no zero is mixed in


@pytest.mark.parametrize("d", DIMS)
def test_long_rows_of_a_directed_matrix_and_of_its_transpose(d):
    from ctgcn_amd import ops
    m = directed_graph()
    adj, plain = gcn_adj(m, long_threshold=8), gcn_adj(m)
    assert adj.long_rows is not None and adj.transposed().long_rows is not None and adj.pieces > 1
    S = torch.from_numpy(dense((N, d), d)).to(DEV)
    Y, arg, dS = check(m, adj, S, "pieces d %d" % d)
    Y0, arg0 = ops._pool_max_fwd(plain, S)
    assert torch.equal(Y, Y0) and torch.equal(arg, arg0)


@pytest.mark.parametrize("long_threshold", [None, 2], ids=["rows", "pieces"])
@pytest.mark.parametrize("d", [6, 24])
def test_ties_go_to_the_lower_index_and_take_the_whole_gradient(d, long_threshold):
    """row 0 reads nodes 1 .. 20, row 2 reads 5 and 9.  Nodes 3 and 17 hold the same maximum in the even columns (long_threshold 2:
    pieces of 7 entries, so the two lie in the first and the last piece); 5 and 9 tie everywhere."""
    from ctgcn_amd import ops
    n = 24
    rows = [0] * 20 + [2, 2] + [5]
    cols = list(range(1, 21)) + [5, 9] + [0]
    m = sp.csr_matrix((np.ones(len(rows)), (rows, cols)), shape=(n, n))
    m.sort_indices()
    s = dense((n, d), 31)
    s[3, 0::2] = 7.0
    s[17, 0::2] = 7.0
    s[17, 1::2] = 8.0
    s[9] = s[5]
    adj = ops.GcnAdj.from_scipy(m, DEV, long_threshold=long_threshold)
    assert (adj.long_rows is not None) == bool(long_threshold) and (not long_threshold or adj.pieces == 3)
    S = torch.from_numpy(s).to(DEV).requires_grad_()
    Y = ops.pool_max(S, adj)
    _, arg = ops._pool_max_fwd(adj, S.detach())
    ref, ref_arg = reference(m, s)
    assert np.array_equal(Y.detach().cpu().numpy(), ref) and np.array_equal(arg.cpu().numpy(), ref_arg)
    assert bool((arg[0, 0::2] == 3).all()) and bool((arg[0, 1::2] == 17).all()) and bool((arg[2] == 5).all())
    C = torch.from_numpy(dense((n, d), 32)).to(DEV)
    (Y * C).sum().backward()
    g = S.grad
    assert torch.equal(g[3, 0::2], C[0, 0::2]) and not g[17, 0::2].any() and torch.equal(g[17, 1::2], C[0, 1::2]) and not g[3, 1::2].any()
    assert torch.equal(g[5], C[2]) and not g[9].any() and torch.equal(g[0], C[5])
    close_scaled(f64(g), pull_reference(ref_arg, C.cpu().numpy()))
    S2 = S.detach().clone().requires_grad_()
    (ops.pool_max(S2, adj) * C).sum().backward()
    assert torch.equal(S2.grad, g)


def test_padded_rows_at_an_unaligned_base_take_the_scalar_path_and_argument_checks():
    from ctgcn_amd import ops
    d, ld = 24, 27
    buf = torch.zeros(N * ld + 1, device=DEV)
    S = buf[1:].as_strided((N, d), (ld, 1))
    S.copy_(torch.from_numpy(dense((N, d), 5)))
    assert S.data_ptr() % 16 == 4
    m = directed_graph()
    for long_threshold in (None, 8):
        adj = gcn_adj(m, long_threshold)
        Y, arg, _ = check(m, adj, S, "unaligned")
        Y0, arg0 = ops._pool_max_fwd(adj, S.contiguous())
        assert torch.equal(Y, Y0) and torch.equal(arg, arg0)
    with pytest.raises(ValueError):
        ops.pool_max(S[:-1], adj)
    with pytest.raises(TypeError):
        ops.pool_max(S.double(), adj)
