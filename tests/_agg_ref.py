"""Float64 model of the CoreDiffusion aggregation (ctgcn_hip.hip: agg_fwd_kernel, agg_bwd_kernel, agg_bwd_prep_kernel, the hub kernels and
agg_hub_final_kernel), written from the INPUT matrix list and the flags — never from CoreAdj's arrays.

The operation (reference layers.py:41-48 and the [N, K, d] layout of :58), for the list A_0 .. A_{K-1} (A_0 + I with the self loop):

    pre_j = sum_{i <= j} A_i x          H_j = relu?(pre_j)                                  forward
    G_j = dH_j [pre_j > 0]?   S_j = sum_{i >= j} G_i   dX = sum_j A_j^T S_j                 backward
    Z_j = S_j (general storage)  or  sum_{i >= j} S_i (nested storage: an entry tagged s is stored once for matrices s .. K-1);  S0 = S_0

Every result comes with its term mass T = sum |terms| (a term counts as often as the cumulative sums count it: an entry of A_i enters
pre_j once for every i <= j ... and H_j only once, so T is per element [n, K, d]) and the term count m.

Two tiers of inputs
  exact    x, dH multiples of 1/4, matrix values multiples of 1/2: every product is a multiple of the granule 1/8, every partial sum
           of any subset of an element's terms is an integer multiple of the granule of magnitude <= T.  While T / granule < 2^24 that
           integer fits fp32's significand: every partial sum in ANY order is exact, and a correct kernel equals the model bit for bit.
           check_exact() asserts the condition for every intermediate the model has (P, R = pre, S, Z, dX).
  rounded  arbitrary fp32 inputs.  Bound per element: |got - model| <= gamma_k T, gamma_k = k u / (1 - k u), u = 2^-24, k = m + K + 2.
           Derivation.  A sum of m products evaluated in any order (lane-group chains, group partials in LDS, pieces) passes each product
           through at most m roundings (its own, an FMA has one, and at most m - 1 additions: adding an exact zero of an empty group or
           slot rounds nothing), so by the standard summation bound (Higham, Accuracy and Stability, §4.2) its error is at most
           gamma_m sum |terms|.  On top of that a term meets at most K roundings of the slot recurrences (R += P over the K slots; the
           nested Pc += sk chain of the hub kernels only rounds at non-empty slots, which the m above already pays for; S and Z of the
           prep kernel: a dH entry reaches Z_j through at most i - j + 1 <= K additions) and one for the self-loop row.  The model itself
           is computed in float64 from the same fp32 inputs: its own error, gamma'_{m+K} T with u' = 2^-53, is covered by the last unit
           of k = m + K + 2.  Nothing is measured, no floor is added: an element with T = 0 must be exactly 0.
"""
import numpy as np
import scipy.sparse as sp

U = 2.0 ** -24
GRANULE = 0.125


class Result(object):
    """value (float64), T (term mass, same shape) and m (term count, broadcastable to value)"""

    def __init__(self, value, T, m):
        self.value, self.T, self.m = value, T, m

    def bound(self, K):
        k = np.asarray(self.m, dtype=np.float64) + K + 2
        g = k * U / (1.0 - k * U)
        while g.ndim < self.T.ndim:
            g = g[..., None]
        return g * self.T

    def used(self, got, K):
        """worst |got - value| / bound over the elements (0 where both are 0; inf where the bound is 0 and the error is not)"""
        err = np.abs(np.asarray(got, dtype=np.float64) - self.value)
        b = self.bound(K)
        with np.errstate(divide="ignore", invalid="ignore"):
            frac = np.where(err == 0, 0.0, err / b)
        return float(frac.max(initial=0.0))


def _mats64(mats, self_loop):
    out = []
    for j, m in enumerate(mats):
        m = sp.csr_matrix(m).astype(np.float64)
        m.sum_duplicates()
        if j == 0 and self_loop:
            m = (m + sp.identity(m.shape[0], dtype=np.float64, format="csr")).tocsr()
        out.append(m)
    return out


def is_nested(mats):
    """every entry of A_i is an entry of A_{i+1} with the same value (the k-core lists; what CoreAdj stores once per entry)"""
    ms = _mats64(mats, False)
    for a, b in zip(ms[:-1], ms[1:]):
        a, b = a.copy(), b.copy()
        a.eliminate_zeros()
        b.eliminate_zeros()
        diff = (b - a).tocsr()
        diff.eliminate_zeros()
        if diff.nnz != b.nnz - a.nnz:
            return False
    return True


def _row_counts(mats, transpose=False):
    """stored terms of each row: the rows of the largest matrix of a nested list (one product per entry), else every matrix's entries"""
    ms = _mats64(mats, False)
    axis = 0 if transpose else 1
    cnt = [np.asarray((m != 0).sum(axis=axis)).reshape(-1) for m in ms]
    return cnt[-1] if is_nested(mats) else np.sum(cnt, axis=0)


def forward(mats, x, self_loop, relu):
    """(H, pre): Results [n, K, d].  H.T = pre.T, m [n, 1]."""
    x = np.asarray(x, dtype=np.float64)
    ms = _mats64(mats, self_loop)
    n, d = x.shape
    K = len(ms)
    pre, T = np.empty((n, K, d)), np.empty((n, K, d))
    P, TP = np.zeros((n, d)), np.zeros((n, d))
    ax = np.abs(x)
    for j, m in enumerate(ms):
        P = P + m @ x                          # R_j = R_{j-1} + A_j x: the kernels' R += P with P running over the slots (nested) or per slot
        TP = TP + abs(m) @ ax
        pre[:, j], T[:, j] = P, TP
    cnt = (_row_counts(mats) + (1 if self_loop else 0))[:, None]
    H = np.maximum(pre, 0.0) if relu else pre
    return Result(H, T, cnt), Result(pre, T, cnt)


def backward_prep(H, dH, nested, relu):
    """(Z [n, K, d], S0 [n, d]) as Results from H (its sign pattern is the mask: H > 0) and dH; m = 0 (no gathered products: the K
    additions are the K of k)."""
    H, dH = np.asarray(H, dtype=np.float64), np.asarray(dH, dtype=np.float64)
    G = np.where(H > 0, dH, 0.0) if relu else dH
    S = np.cumsum(G[:, ::-1], axis=1)[:, ::-1]
    TS = np.cumsum(np.abs(G)[:, ::-1], axis=1)[:, ::-1]
    if nested:
        Z, TZ = np.cumsum(S[:, ::-1], axis=1)[:, ::-1], np.cumsum(TS[:, ::-1], axis=1)[:, ::-1]
    else:
        Z, TZ = S, TS
    return Result(np.ascontiguousarray(Z), np.ascontiguousarray(TZ), 0), Result(S[:, 0].copy(), TS[:, 0].copy(), 0)


def backward(mats, x, dH, self_loop, relu, H=None):
    """dX [n, d] = d sum(H dH) / dx as a Result.  The mask comes from the model's own float64 pre-activations (or from H when given)."""
    dH = np.asarray(dH, dtype=np.float64)
    ms = _mats64(mats, self_loop)
    if H is None:
        H = forward(mats, x, self_loop, relu)[1].value
    prep = backward_prep(H, dH, False, relu)[0]
    S, TS = prep.value, prep.T
    n, K, d = dH.shape
    dX, T = np.zeros((n, d)), np.zeros((n, d))
    for j, m in enumerate(ms):
        mt = m.T.tocsr()
        dX += mt @ S[:, j]
        T += abs(mt) @ TS[:, j]
    cnt = (_row_counts(mats, transpose=True) + (1 if self_loop else 0))[:, None]
    return Result(dX, T, cnt)


def check_exact(*results):
    """the exact tier's condition: every term mass below 2^24 granules (see the module docstring); returns the worst T / granule"""
    worst = max(float(r.T.max(initial=0.0)) for r in results) / GRANULE
    assert worst < 2.0 ** 24, "term mass %.3g granules: partial sums are not exact in fp32, shrink the value ranges" % worst
    for r in results:
        assert np.array_equal(r.value, np.round(r.value / GRANULE) * GRANULE)
    return worst


def model_all(mats, x, dH, self_loop, relu):
    """everything a GPU case compares: H, pre, Z, S0, dX (Results), for the storage CoreAdj chooses (nested when the list is)"""
    H, pre = forward(mats, x, self_loop, relu)
    nested = is_nested(mats)
    Z, S0 = backward_prep(H.value, dH, nested, relu)
    dX = backward(mats, x, dH, self_loop, relu, H=H.value)
    return dict(H=H, pre=pre, Z=Z, S0=S0, dX=dX, nested=nested)


def exact_model(mats, x, dH, self_loop, relu):
    """model_all + the 2^24 check on every intermediate: P and R (pre.T bounds both), S and Z (Z.T >= S.T), dX"""
    out = model_all(mats, x, dH, self_loop, relu)
    out["granules"] = check_exact(out["pre"], out["Z"], out["S0"], out["dX"])
    return out
