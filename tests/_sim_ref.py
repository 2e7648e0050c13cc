"""Shared by the similarity-prediction tests: a numpy/scipy statement of the reference's ground truth (the adjacency it builds and
the Leicht–Holme–Newman series with its finish steps), written from the algorithm, for small graphs."""
import numpy as np
import scipy.sparse as sp


def adjacency(src, dst, w, n):
    """The reference's matrix of snapshot rows: a lil matrix where every row sets A[u, v] = A[v, u] = w in file order (assigning 0
    removes the entry), self loops skipped, then CSR."""
    A = sp.lil_matrix((n, n))
    for u, v, x in zip(np.asarray(src).tolist(), np.asarray(dst).tolist(), np.asarray(w, np.float64).tolist()):
        if u == v:
            continue
        A[u, v] = x
        A[v, u] = x
    return A.tocoo().tocsr()


def similarity(A, lam, alpha=0.5, iter_num=100):
    """The n x n similarity as scipy COO: iter_num steps of S = c·(A·S) + I from S = 0 with c = alpha / lam (scipy's CSR x dense
    product), then (S + Sᵀ)/2, minus I, min-max over all entries, entries below 1e-6 set to 0."""
    A = sp.csr_matrix(A)
    n = A.shape[0]
    c = alpha / lam
    eye = np.eye(n)
    S = np.zeros((n, n))
    for _ in range(iter_num):
        S = c * A.dot(S) + eye
    S = (S + S.T) / 2
    S = S - eye
    S = (S - S.min()) / (S.max() - S.min())
    S[S < 1e-6] = 0
    return sp.coo_matrix(S)


# ------------------------------------------------------------------------------------------------ the finish, stated on the block
def finish(S, pad_zero, eps):
    """(S, (min, max), row_nnz) of the finish over an m x m block: (S + Sᵀ)/2 - I, min and max over all entries (and over 0 when
    pad_zero: the zero rows of the isolated vertices of the n x n matrix), (S - min)/(max - min), entries below eps set to 0, and
    the non-zeros left per row (a NaN counts, as it does for np.nonzero)."""
    S = np.asarray(S, np.float64)
    S = (S + S.T) / 2
    S = S - np.eye(len(S))
    mn, mx = S.min(), S.max()
    if pad_zero:
        mn, mx = min(mn, 0.0), max(mx, 0.0)
    with np.errstate(divide='ignore', invalid='ignore'):
        S = (S - mn) / (mx - mn)
        S[S < eps] = 0
    return S, (mn, mx), np.count_nonzero(S, axis=1).astype(np.int64)


# ------------------------------------------------------------------------------------------------ numpy's float64 sum, in Python
NP_BUF = 8192        # elements the add.reduce loop is handed at a time
NP_BLOCK = 128       # the pairwise recursion stops at blocks of at most this many elements


def _np_block(a):
    """A block of at most 128 float64: below 8 elements a running sum from 0.0; otherwise 8 running sums r[j] over a[j], a[8 + j], ...,
    combined as ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the n % 8 trailing elements added in order.  Python floats
    are IEEE doubles, so every + here is the one numpy's loop performs."""
    n = len(a)
    if n < 8:
        res = 0.0
        for v in a:
            res = res + v
        return res
    r = a[:8]
    i = 8
    while i < n - n % 8:
        r = [r[j] + a[i + j] for j in range(8)]
        i += 8
    res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
    for v in a[i:]:
        res = res + v
    return res


def _np_pairwise(a):
    n = len(a)
    if n <= NP_BLOCK:
        return _np_block(a)
    h = n // 2
    h -= h % 8
    return _np_pairwise(a[:h]) + _np_pairwise(a[h:])


def np_sum_model(x):
    """numpy's sum of a contiguous float64 array, operation for operation: chunks of 8192 elements in memory order, each summed
    pairwise (halves cut at multiples of 8 down to blocks of at most 128), the chunk sums added in order from 0.0."""
    a = np.ascontiguousarray(x, np.float64).ravel().tolist()
    total = 0.0
    for lo in range(0, len(a), NP_BUF):
        total = total + _np_pairwise(a[lo:lo + NP_BUF])
    return total


def normalize(x):
    """The predictor's two normalisations with numpy itself: ((x - min)/(max - min)) / sum.  Returns (result, (min, max, sum))."""
    x = np.asarray(x, np.float64)
    mn, mx = x.min(), x.max()
    y = (x - mn) / (mx - mn)
    s = y.sum()
    return y / s, (mn, mx, s)


# ------------------------------------------------------------------------------------------------ Spearman sums, exactly
def spearman_sums(x, y):
    """(Σ (rx-μ)(ry-μ), Σ (rx-μ)², Σ (ry-μ)²) with average 1-based ranks and μ = (N+1)/2, in integer arithmetic: twice a rank and
    twice μ are integers, so each sum is an integer over 4.  The float64 results are exact while 4·Σ stays below 2^53."""
    out = []
    N = len(x)
    doubled = []
    for v in (x, y):
        v = np.asarray(v, np.float64).ravel()
        vals, inv, cnt = np.unique(v, return_inverse=True, return_counts=True)
        first = np.cumsum(cnt) - cnt                                   # 0-based position of each tie run in sorted order
        twice_rank = 2 * first + cnt + 1                               # 2 * mean(first + 1 .. first + cnt)
        doubled.append([int(t) - (N + 1) for t in twice_rank[inv]])
    dx, dy = doubled
    for a, b in ((dx, dy), (dx, dx), (dy, dy)):
        total = sum(p * q for p, q in zip(a, b))
        assert total < 2 ** 53
        out.append(total / 4.0)
    return tuple(out)
