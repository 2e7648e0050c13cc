"""The TIMERS fixture's recipe and a numpy mirror of the TIMERS passes (Obj, Obj_SimChange, TRIP, the bound operator, a block subspace
solver), shared by tests/golden/make_golden_timers.py and the TIMERS tests.  The mirror is written from the method's formulas, in
fp64, with dense or scipy operands; it is the reference the kernels are compared with at sizes the golden file does not cover."""
import numpy as np
import scipy.sparse as sp

# the main fixture and the tiny one (host tests): nodes, rank, snapshots after the first, restart threshold
N, K, STEPS, THETA = 300, 16, 5, 0.17
TINY_N, TINY_K = 96, 4
PAIRS_PER_NODE = 4              # 4 n random pairs with weights 1 + randint(3)
CHANGE_DIV = 16                 # steps 1, 2, 4, 5 set n / 16 random pairs to weight randint(4) (0 deletes)
COMMUNITY_STEP, COMMUNITY_NODES, COMMUNITY_DENSITY, COMMUNITY_WEIGHT = 3, 12, 0.7, 2.0
PICKS = 256                     # stored entries of U_cur V_curᵀ per step
RATIO_MARGIN = 0.005            # every Loss_store / Loss_bound is at least this far from 1 + Theta
GAP_MIN = 5e-4                  # smallest relative gap among the K + 1 leading |λ| of every decomposed matrix
SPREAD_MAX = 1e-10             # the reference's losses agree with themselves to this, relative, across svds start vectors
TOL = 1e-12                     # the solver tolerance of the tests
U53 = 2.0 ** -53


def _random_pairs(rng, n, count):
    i = rng.randint(n, size=count)
    j = (i + 1 + rng.randint(n - 1, size=count)) % n          # never a self pair
    return i, j


def make_snapshots(seed, n):
    """The STEPS + 1 cumulative symmetric weighted snapshots of the recipe, as scipy CSR"""
    rng = np.random.RandomState(seed)
    A = np.zeros((n, n))
    i, j = _random_pairs(rng, n, PAIRS_PER_NODE * n)
    w = 1.0 + rng.randint(3, size=len(i))
    for a, b, v in zip(i, j, w):
        A[a, b] = A[b, a] = v
    snaps = [A.copy()]
    for step in range(1, STEPS + 1):
        if step == COMMUNITY_STEP:
            nodes = rng.choice(n, COMMUNITY_NODES, replace=False)
            for x in range(COMMUNITY_NODES):
                for y in range(x + 1, COMMUNITY_NODES):
                    if rng.rand() <= COMMUNITY_DENSITY:
                        A[nodes[x], nodes[y]] = A[nodes[y], nodes[x]] = COMMUNITY_WEIGHT
        else:
            i, j = _random_pairs(rng, n, n // CHANGE_DIV)
            w = rng.randint(4, size=len(i)).astype(np.float64)
            for a, b, v in zip(i, j, w):
                A[a, b] = A[b, a] = v
        snaps.append(A.copy())
    return [sp.csr_matrix(s) for s in snaps]


def delta(prev, cur):
    d = (sp.csr_matrix(cur) - sp.csr_matrix(prev)).tocsr()
    d.eliminate_zeros()
    return d


def put_csr(out, key, m):
    m = sp.csr_matrix(m, dtype=np.float64)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    out[key + "_indptr"], out[key + "_indices"], out[key + "_data"] = m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data


def get_csr(g, key):
    indptr = g[key + "_indptr"]
    n = len(indptr) - 1
    return sp.csr_matrix((g[key + "_data"], g[key + "_indices"], indptr), shape=(n, n))


# ------------------------------------------------------------------------------------------------ the mirror
def entries(S):
    S = sp.csr_matrix(S)
    rows = np.repeat(np.arange(S.shape[0]), np.diff(S.indptr))
    return rows, S.indices, S.data


def obj_sums(S, U, V, s_old=None, as_float=True):
    """(Σ s², Σ s d) or with s_old (Σ (s_old + s − d)² − (s_old − d)², Σ s d), d = ⟨U_r, V_c⟩, over the stored entries of S"""
    r, c, s = entries(S)
    d = (U[r] * V[c]).sum(axis=1)
    a = (s * s).sum() if s_old is None else ((s_old + s - d) ** 2 - (s_old - d) ** 2).sum()
    b = (s * d).sum()
    return (float(a), float(b)) if as_float else (a, b)       # (as they are: extended-precision operands)


def obj_bound(S, U, V, s_old=None):
    """Worst-case rounding bound of obj_sums in any summation order: m·2⁻⁵³·Σ|terms| with every product of the expanded sums a term
    (m = entries · (k + 4)), for each of the two outputs"""
    r, c, s = entries(S)
    k = U.shape[1]
    D = (np.abs(U[r]) * np.abs(V[c])).sum(axis=1)
    m = (len(s) * (k + 4) + 4) * U53
    if s_old is None:
        return m * float((s * s).sum()), m * float((np.abs(s) * D).sum())
    so = np.abs(s_old)
    return m * float(((so + np.abs(s) + D) ** 2 + (so + D) ** 2).sum()), m * float((np.abs(s) * D).sum())


def Obj(S, U, V):
    a, b = obj_sums(S, U, V)
    return a - 2.0 * b + float(((U.T @ U) * (V.T @ V)).sum())


def Obj_SimChange(S_ori, S_add, U, V, loss_ori):
    r, c, _ = entries(S_add)
    old = np.asarray(sp.csr_matrix(S_ori)[r, c]).ravel() if len(r) else np.zeros(0)
    return loss_ori + obj_sums(S_add, U, V, s_old=old)[0]


def trip_parts(Old_U, Old_S, Old_V, Delta):
    """TRIP's intermediates: X (signs unified), Old_L, temp_sum = Xᵀ Δ X, ΔL, alpha [K, K]"""
    K = Old_U.shape[1]
    s = np.diag(Old_S) if np.ndim(Old_S) == 2 else np.asarray(Old_S)
    cols = np.arange(K)
    X = Old_U.copy()
    lead = X[np.abs(X).argmax(axis=0), cols]
    X = X * np.where(lead < 0, -1.0, 1.0)
    Old_L = s * np.sign(Old_U.max(axis=0) * Old_V[Old_U.argmax(axis=0), cols])
    temp_sum = X.T @ (sp.csr_matrix(Delta) @ X)
    Delta_L = np.diag(temp_sum).copy()
    alpha = np.zeros((K, K))
    for i in range(K):
        D = np.diag(np.ones(K) * (Old_L[i] + Delta_L[i]) - Old_L)
        alpha[:, i] = np.linalg.pinv(D - temp_sum) @ temp_sum[:, i]
    return X, Old_L, temp_sum, Delta_L, alpha


def TRIP(Old_U, Old_S, Old_V, Delta):
    X, Old_L, _, Delta_L, alpha = trip_parts(Old_U, Old_S, Old_V, Delta)
    New_U = X + X @ alpha
    New_U = New_U / np.sqrt((New_U * New_U).sum(axis=0))
    New_L = Old_L + Delta_L
    return New_U, np.diag(np.abs(New_L)), New_U * np.sign(New_L)


def bound_operator(S_ori, S_add):
    """(apply, trace_change) of RefineBound: x ↦ S_ori (S_add x) + S_add ((S_ori + S_add) x), ‖S_ori + S_add‖²_F − ‖S_ori‖²_F"""
    ori, add = sp.csr_matrix(S_ori), sp.csr_matrix(S_add)
    tot = (ori + add).tocsr()
    return (lambda x: ori @ (add @ x) + add @ (tot @ x)), float((tot.data ** 2).sum() - (ori.data ** 2).sum())


def bound_dense(S_ori, S_add):
    ori, add = sp.csr_matrix(S_ori).toarray(), sp.csr_matrix(S_add).toarray()
    M = ori @ add
    return M + M.T + add @ add


def topk_dense(M, k):
    """The k eigenvalues of largest magnitude of a dense symmetric matrix, |w| descending (LAPACK)"""
    w = np.linalg.eigvalsh((M + M.T) / 2)
    return w[np.argsort(-np.abs(w), kind="stable")[:k]]


def eigen_sum(w, K):
    kept = np.sort(w[w >= 0])[::-1]
    if len(kept) >= K:
        return float(kept[:K].sum()), kept
    return float(kept.sum() + kept[-1] * (K - len(kept))), kept


def sym_topk(apply, n, k, tol=TOL, max_iter=5000, seed=0):
    """Block subspace iteration with Rayleigh–Ritz, width min(n, 2 k + 8), Householder QR; stops when every wanted pair has
    ‖A x − w x‖₂ <= tol·|w₁|.  Returns (w, X, iterations)."""
    b = min(n, 2 * k + 8)
    Q = np.linalg.qr(np.random.RandomState(seed).randn(n, b))[0]
    for it in range(1, max_iter + 1):
        Z = apply(Q)
        theta, S = np.linalg.eigh(Q.T @ Z)
        order = np.argsort(-np.abs(theta), kind="stable")[:k]
        theta, S = theta[order], S[:, order]
        res = np.linalg.norm(Z @ S - (Q @ S) * theta, axis=0).max()
        if res <= tol * abs(theta[0]):
            return theta, Q @ S, it
        Q = np.linalg.qr(Z)[0]
    raise RuntimeError("residual %.3e after %d iterations" % (res, max_iter))


def gap_min(mats, K):
    """Smallest relative gap between consecutive magnitudes among the K + 1 leading |λ| of the matrices"""
    g = np.inf
    for M in mats:
        a = np.sort(np.abs(np.linalg.eigvalsh(sp.csr_matrix(M).toarray())))[::-1][:K + 1]
        g = min(g, float(((a[:-1] - a[1:]) / a[0]).min()))
    return g


def obj_total_bound(S, U, V):
    """Worst-case rounding bound of Obj = Σs² − 2 Σ s d + ⟨UᵀU, VᵀV⟩ in any summation order (the third term: n + K² + 2 operations deep
    over the products |U_ri U_rj| |V_si V_sj|)"""
    b0, b1 = obj_bound(S, U, V)
    k = U.shape[1]
    third = (U.shape[0] + V.shape[0] + k * k + 2) * U53 * float(((np.abs(U).T @ np.abs(U)) * (np.abs(V).T @ np.abs(V))).sum())
    return b0 + 2.0 * b1 + third + 4 * U53 * abs(Obj(S, U, V))


def trip_bound(Old_U, Old_S, Old_V, Delta):
    """How far two fp64 evaluations of TRIP that differ in summation order can lie apart, to first order, from the inputs alone:
    (tolerance per column of New_U and New_V in the 2-norm (so per entry too), tolerance of diag(New_S)).
    temp_sum = Xᵀ Δ X carries dT <= (n + r) 2⁻⁵³ |X|ᵀ|Δ||X| per entry (r: the longest row of Δ).  alpha_i = pinv(M_i) t_i with
    M_i = D_i − temp_sum moves by at most ‖pinv(M_i)‖₂ (‖dT‖_F + ‖dM_i‖_F ‖alpha_i‖₂), ‖dM_i‖_F <= ‖dT‖_F + 4 K 2⁻⁵³ max|L| (a change
    of M_i that crosses pinv's cut-off is not first order and is not covered).  New_U's column i is X (e_i + alpha_i) over its norm, and
    that norm is at least 1/2 for an orthonormal X, so its error is at most 4 (‖d alpha_i‖₂ + (n + K) 2⁻⁵³ (1 + ‖alpha_i‖₁))."""
    X, Old_L, temp_sum, Delta_L, alpha = trip_parts(Old_U, Old_S, Old_V, Delta)
    n, K = X.shape
    D = abs(sp.csr_matrix(Delta))
    r = int(np.diff(D.indptr).max(initial=0))
    dT = (n + r + 2) * U53 * (np.abs(X).T @ (D @ np.abs(X)))
    dTF = float(np.linalg.norm(dT))
    cols = np.zeros(K)
    for i in range(K):
        M = np.diag(np.ones(K) * (Old_L[i] + Delta_L[i]) - Old_L) - temp_sum
        pn = float(np.linalg.norm(np.linalg.pinv(M), 2))
        dM = dTF + 4 * K * U53 * float(np.abs(Old_L).max())
        da = pn * (dTF + dM * float(np.linalg.norm(alpha[:, i])))
        cols[i] = 4.0 * (da + (n + K) * U53 * (1.0 + float(np.abs(alpha[:, i]).sum())))
    return cols, np.diag(dT) + 2 * U53 * np.abs(Old_L + Delta_L)


def run_mirror(snaps, K, theta, update, tol=TOL, decompose=None):
    """The TIMERS loop on the mirror: dict of loss, bound, tested_loss, tested_bound, restart, sigma [steps, K], cur (U_cur, V_cur per
    step).  decompose(A) -> (w, X) defaults to the mirror's subspace solver."""
    n = snaps[0].shape[0]
    if decompose is None:
        decompose = lambda A: sym_topk(lambda x: A @ x, n, K, tol=tol)[:2]      # noqa: E731

    def factors(A):
        w, X = decompose(sp.csr_matrix(A))
        w, X = w[::-1], X[:, ::-1]
        return X, np.abs(w), X * np.sign(w)

    steps = len(snaps)
    rec = dict(loss=np.zeros(steps), bound=np.zeros(steps), tested_loss=np.zeros(steps), tested_bound=np.zeros(steps),
               restart=np.zeros(steps, dtype=bool), sigma=np.zeros((steps, K)), cur=[])
    Sim = S_cum = sp.csr_matrix(snaps[0])
    S_perturb = sp.csr_matrix((n, n))
    U, s, V = factors(Sim)
    U_cur, V_cur = U * np.sqrt(s), V * np.sqrt(s)
    loss_rerun = Obj(Sim, U_cur, V_cur)
    rec["loss"][0] = rec["bound"][0] = rec["tested_loss"][0] = rec["tested_bound"][0] = loss_rerun
    rec["sigma"][0] = s
    rec["cur"].append((U_cur, V_cur))
    for i in range(1, steps):
        S_add = delta(S_cum, snaps[i])
        S_perturb = S_perturb + S_add
        if update:
            U, S_mat, V = TRIP(U, s, V, S_add)
            s = np.diag(S_mat)
            U_cur, V_cur = U * np.sqrt(s), V * np.sqrt(s)
            loss = Obj(S_cum + S_add, U_cur, V_cur)
        else:
            loss = Obj_SimChange(S_cum, S_add, U_cur, V_cur, rec["loss"][i - 1])
        apply, trace_change = bound_operator(Sim, S_perturb)
        w = sym_topk(apply, n, min(2 * K, n), tol=tol)[0]
        bound = loss_rerun + trace_change - eigen_sum(w, K)[0]
        S_cum = S_cum + S_add
        rec["tested_loss"][i], rec["tested_bound"][i] = loss, bound
        if loss >= (1 + theta) * bound:
            rec["restart"][i] = True
            Sim, S_perturb = S_cum, sp.csr_matrix((n, n))
            U, s, V = factors(Sim)
            U_cur, V_cur = U * np.sqrt(s), V * np.sqrt(s)
            loss_rerun = loss = bound = Obj(Sim, U_cur, V_cur)
        rec["loss"][i], rec["bound"][i], rec["sigma"][i] = loss, bound, s
        rec["cur"].append((U_cur, V_cur))
    return rec
