"""Float64 host model of ops.topk_scores and of evaluation/graph_reconstruction.py: scores, admissibility, the total order, padding,
the three metrics, MAP, the global pair ranking and its certificate.  numpy only; dense [m, n] matrices, so for small cases."""
import numpy as np


def csr_from_pairs(n, pairs):
    """(row_ptr int32 [n + 1], col int32) of the set of (row, col) pairs, columns ascending within a row"""
    keys = np.unique(np.array([r * n + c for r, c in pairs], dtype=np.int64)) if len(pairs) else np.zeros(0, np.int64)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(np.bincount(keys // n, minlength=n))
    return row_ptr.astype(np.int32), (keys % n).astype(np.int32)


def csr_dense(n, row_ptr, col):
    M = np.zeros((n, n), dtype=bool)
    for r in range(n):
        M[r, col[row_ptr[r]:row_ptr[r + 1]]] = True
    return M


def scores(E, rows=None, row_bias=None, col_bias=None):
    """float64 [m, n]: E[q] · E[j] + col_bias[j] + row_bias[i]"""
    E = np.asarray(E, dtype=np.float64)
    q = np.arange(E.shape[0]) if rows is None else np.asarray(rows, dtype=np.int64)
    S = E[q] @ E.T
    if col_bias is not None:
        S = S + np.asarray(col_bias, dtype=np.float64)[None, :]
    if row_bias is not None:
        S = S + np.asarray(row_bias, dtype=np.float64)[:, None]
    return S


def abs_scores(E, rows=None, row_bias=None, col_bias=None):
    """float64 [m, n]: Σ_t |E[q, t] E[j, t]| + |col_bias[j]| + |row_bias[i]|, the magnitude the rounding bound scales with"""
    return scores(np.abs(np.asarray(E, dtype=np.float64)), rows, None if row_bias is None else np.abs(row_bias),
                  None if col_bias is None else np.abs(col_bias))


def admissible(n, rows=None, exclude_self=False, upper_only=False, exclude=None):
    """bool [m, n]; exclude = (row_ptr, col) indexed by node id"""
    q = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    j = np.arange(n)[None, :]
    ok = np.ones((len(q), n), dtype=bool)
    if exclude_self:
        ok &= j != q[:, None]
    if upper_only:
        ok &= j > q[:, None]
    if exclude is not None:
        ok &= ~csr_dense(n, *exclude)[q]
    return ok


def select(S, ok, k):
    """(score float64 [m, k], index int32 [m, k]): per row the k best admissible columns, score descending, the lower column among
    equal scores; -inf / -1 in unused slots"""
    m, n = S.shape
    score = np.full((m, k), -np.inf)
    index = np.full((m, k), -1, dtype=np.int32)
    for i in range(m):
        cols = np.nonzero(ok[i])[0]
        order = cols[np.lexsort((cols, -S[i, cols]))][:k]
        score[i, :len(order)] = S[i, order]
        index[i, :len(order)] = order
    return score, index


def topk(E, k, rows=None, row_bias=None, col_bias=None, exclude_self=False, upper_only=False, exclude=None):
    n = np.asarray(E).shape[0]
    return select(scores(E, rows, row_bias, col_bias), admissible(n, rows, exclude_self, upper_only, exclude), k)


def score_inputs(E, metric):
    """(X, row_bias, col_bias) in float64"""
    E = np.asarray(E, dtype=np.float64)
    if metric == 'dot':
        return E, None, None
    sq = (E ** 2).sum(1)
    if metric == 'cosine':
        norm = np.sqrt(sq)
        return E / np.where(norm > 0, norm, 1.0)[:, None], None, None
    assert metric == 'l2'
    return E, -0.5 * sq, -0.5 * sq


def average_precision(hits, n_rel, K):
    """(MAP, rows counted) by the definition, one row and one rank at a time"""
    aps = []
    for h, nr in zip(np.asarray(hits, dtype=bool), n_rel):
        if nr <= 0:
            continue
        total, found = 0.0, 0
        for r in range(K):
            if h[r]:
                found += 1
                total += found / (r + 1.0)
        aps.append(total / min(int(nr), K))
    return (float(np.mean(aps)) if aps else float("nan")), len(aps)


def targets(n, target, known=None):
    """bool [n, n]: target's positions minus the diagonal, minus known's"""
    T = csr_dense(n, *target)
    np.fill_diagonal(T, False)
    if known is not None:
        T &= ~csr_dense(n, *known)
    return T


def global_pairs(S, ok_upper):
    """every admissible pair i < j as rows (i, j), ordered by (score descending, i ascending, j ascending)"""
    i, j = np.nonzero(ok_upper)
    order = np.lexsort((j, i, -S[i, j]))
    return i[order], j[order]


def evaluate(E, target, k_list, max_k, metric='dot', known=None, X=None):
    """The whole evaluation from dense matrices: {'MAP', 'rows', 'precision' {k}, 'pairs' {k}}.  X overrides the metric's operands
    (the float32 values the device ranks by, so that both sides order the same numbers)."""
    n = np.asarray(E).shape[0]
    Xm, rb, cb = score_inputs(E, metric) if X is None else X
    S = scores(Xm, None, rb, cb)
    T = targets(n, target, known)
    _, index = select(S, admissible(n, None, True, False, known), max_k)
    hits = np.zeros(index.shape, dtype=bool)
    for i in range(n):
        valid = index[i] >= 0
        hits[i, valid] = T[i, index[i, valid]]
    mean_ap, rows = average_precision(hits, T.sum(1), max_k)
    gi, gj = global_pairs(S, admissible(n, None, False, True, known))
    cum = np.cumsum(T[gi, gj])
    precision, pairs = {}, {}
    for k in k_list:
        den = min(k, len(gi))
        pairs[k] = den
        precision[k] = float(cum[den - 1]) / den if den else float("nan")
    return {'MAP': mean_ap, 'rows': rows, 'precision': precision, 'pairs': pairs}


def certified(S, ok_upper, width, k):
    """Whether upper-triangle lists of `width` entries a row certify the first k global pairs: no row with at least `width`
    admissible pairs has its width-th pair at or before the k-th pair of the global order (fewer than k listed: no full row)."""
    n = S.shape[0]
    _, index = select(S, ok_upper, width)
    full = index[:, width - 1] >= 0
    if not full.any():
        return True
    li, lj = np.nonzero(index >= 0)
    lj = index[li, lj]
    order = np.lexsort((lj, li, -S[li, lj]))
    if len(order) < k:
        return False
    ki, kj = li[order[k - 1]], lj[order[k - 1]]
    kth = (-S[ki, kj], ki, kj)
    for i in np.nonzero(full)[0]:
        j = index[i, width - 1]
        if (-S[i, j], i, j) <= kth:
            return False
    return True
