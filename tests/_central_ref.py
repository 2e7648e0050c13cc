"""Float64 centralities in numpy + scipy, written for the tests: networkx's closeness, exact betweenness (Brandes) and eigenvector
definitions, vectorised over a batch of sources (one sparse product per BFS level) instead of networkx's per-vertex Python loops."""
import numpy as np
import scipy.sparse as sp


def adjacency(indptr, indices, n):
    return sp.csr_matrix((np.ones(len(indices)), np.asarray(indices), np.asarray(indptr)), shape=(n, n))


def brandes(indptr, indices, n, sources=None, batch=256):
    """(bc, r, D): unscaled Brandes dependency sums over `sources` (default: all), vertices reached and distance sums per source."""
    A = adjacency(indptr, indices, n)
    sources = np.arange(n) if sources is None else np.asarray(sources)
    bc = np.zeros(n)
    r, D = [], []
    for b0 in range(0, len(sources), batch):
        S = sources[b0:b0 + batch]
        rows = np.arange(len(S))
        dist = np.full((len(S), n), -1, np.int64)
        sigma = np.zeros((len(S), n))
        dist[rows, S] = 0
        sigma[rows, S] = 1.0
        front = sigma.copy()
        L = 0
        while True:
            nxt = (A @ front.T).T                 # Σ sigma over the neighbours on level L
            new = (nxt > 0) & (dist < 0)
            if not new.any():
                break
            dist[new] = L + 1
            front = np.where(new, nxt, 0.0)
            sigma += front
            L += 1
        delta = np.zeros_like(sigma)
        for k in range(L - 1, 0, -1):
            coef = np.where(dist == k + 1, (1.0 + delta) / np.where(sigma > 0, sigma, 1.0), 0.0)
            delta = np.where(dist == k, sigma * (A @ coef.T).T, delta)
        bc += delta.sum(0)
        r.append((dist >= 0).sum(1))
        D.append(np.clip(dist, 0, None).sum(1))
    return bc, np.concatenate(r).astype(np.int64), np.concatenate(D).astype(np.int64)


def closeness(r, D, n):
    out = np.zeros(len(r))
    ok = (D > 0) & (n > 1)
    out[ok] = ((r[ok] - 1.0) / D[ok]) * ((r[ok] - 1.0) / (n - 1))
    return out


def betweenness(indptr, indices, n):
    bc = brandes(indptr, indices, n)[0]
    return bc * (1 / ((n - 1) * (n - 2))) if n > 2 else bc


def eigenvector(indptr, indices, n, max_iter=100, tol=1e-6):
    """(x, stop step) of x <- (A + I) x / ||(A + I) x|| from 1/n; (None, None) when no step passes Σ|x - x_last| < n tol."""
    A = adjacency(indptr, indices, n)
    x = np.full(n, 1.0 / n)
    for it in range(max_iter):
        y = x + A @ x
        norm = np.linalg.norm(y) or 1.0
        xn = y / norm
        if np.abs(xn - x).sum() < n * tol:
            return xn, it + 1
        x = xn
    return None, None


def kfold_bounds(n, k):
    sizes = np.full(k, n // k)
    sizes[:n % k] += 1
    return np.concatenate([[0], np.cumsum(sizes)])


def ridge_cv_errors(X, Y, alpha_list, k=5):
    """[|alpha|, T]: mean_squared_error(y, cross_val_predict(Ridge(alpha), X, y, cv=k)) / mean(y), from per-fold augmented Grams."""
    X, Y = np.asarray(X, np.float64), np.asarray(Y, np.float64).reshape(len(X), -1)
    n, d = X.shape
    Z = np.hstack([X, np.ones((n, 1)), Y])
    b = kfold_bounds(n, k)
    grams = np.stack([Z[b[f]:b[f + 1], :d + 1].T @ Z[b[f]:b[f + 1]] for f in range(k)])
    total = grams.sum(0)
    pred = np.zeros((len(alpha_list), n, Y.shape[1]))
    for f in range(k):
        tr = total - grams[f]
        m = tr[d, d]
        sx, sy = tr[:d, d], tr[d, d + 1:]
        xtx = tr[:d, :d] - np.outer(sx, sx) / m
        xty = tr[:d, d + 1:] - np.outer(sx, sy) / m
        for a, alpha in enumerate(alpha_list):
            w = np.linalg.solve(xtx + alpha * np.eye(d), xty)
            pred[a, b[f]:b[f + 1]] = X[b[f]:b[f + 1]] @ w + (sy / m - (sx / m) @ w)
    with np.errstate(divide='ignore', invalid='ignore'):
        return ((pred - Y[None]) ** 2).mean(1) / Y.mean(0)[None]


# ------------------------------------------------------------------------------------------------ test graphs (symmetric CSR)
def csr(n, edges):
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    m = sp.coo_matrix((np.ones(2 * len(e)), (np.concatenate([e[:, 0], e[:, 1]]), np.concatenate([e[:, 1], e[:, 0]]))), shape=(n, n)).tocsr()
    m.sum_duplicates()
    m.sort_indices()
    return m.indptr.astype(np.int32), m.indices.astype(np.int32)


def path(n):
    return csr(n, [(i, i + 1) for i in range(n - 1)])


def star(n):
    return csr(n, [(0, i) for i in range(1, n)])


def cliques(sizes, isolated=0):
    edges, base = [], 0
    for s in sizes:
        edges += [(base + i, base + j) for i in range(s) for j in range(i + 1, s)]
        base += s
    return base + isolated, csr(base + isolated, edges)


def diamonds(k):
    """k diamonds in series: 3k + 1 vertices, 2^k shortest paths end to end."""
    edges = []
    for i in range(k):
        a, t, b, c = 3 * i, 3 * i + 3, 3 * i + 1, 3 * i + 2
        edges += [(a, b), (a, c), (b, t), (c, t)]
    return 3 * k + 1, csr(3 * k + 1, edges)


def power_law(n, m, seed, hub_frac=0.25):
    """Preferential attachment (m edges per new vertex) plus a hub (vertex 0) joined to a random n * hub_frac of the vertices,
    and a few isolated vertices at the end."""
    rng = np.random.default_rng(seed)
    targets = list(range(m))
    pool = []
    edges = []
    for v in range(m, n - 8):
        for t in set(targets):
            edges.append((v, t))
        pool += targets + [v] * m
        targets = [pool[i] for i in rng.integers(0, len(pool), m)]
    hub = rng.choice(np.arange(1, n - 8), int(n * hub_frac), replace=False)
    edges += [(0, int(h)) for h in hub]
    return csr(n, edges)


LAYER_SIZES = (1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 300)


def layered(sizes=LAYER_SIZES, isolated=0, p=0.5, seed=0):
    """(n, (indptr, indices), levels): vertices numbered layer by layer from vertex 0 (sizes[0] must be 1), edges between
    consecutive layers only: every vertex gets one random parent in the layer before it, and every other pair of consecutive layers
    is joined with probability p.  So the BFS levels from vertex 0 are the layers (levels[v] = layer of v; -1 for the `isolated`
    vertices appended at the end) and row lengths run from 1 to most of two layers."""
    rng = np.random.default_rng(seed)
    assert sizes[0] == 1
    starts = np.concatenate([[0], np.cumsum(sizes)])
    edges = []
    for k in range(1, len(sizes)):
        prev = np.arange(starts[k - 1], starts[k])
        for v in range(starts[k], starts[k + 1]):
            edges.append((int(rng.choice(prev)), v))
            edges += [(int(u), v) for u in prev[rng.random(len(prev)) < p]]
    n = int(starts[-1]) + isolated
    levels = np.full(n, -1, np.int64)
    for k in range(len(sizes)):
        levels[starts[k]:starts[k + 1]] = k
    return n, csr(n, edges), levels


# ------------------------------------------------------------------------------------------------ ridge passes in long double
U = 2.0 ** -53       # unit roundoff of float64


def gamma(k):
    """Higham's γ_k = k u / (1 - k u): the relative error bound of k chained float64 roundings."""
    return k * U / (1.0 - k * U)


def fold_grams(X, Y, k):
    """Per fold f of the unshuffled k-fold split: (Z_fᵀ Z_f restricted to [d+1, d+1+T], |Z_f|ᵀ|Z_f| likewise, rows of f), with
    Z = [X 1 Y], in np.longdouble."""
    X = np.asarray(X).astype(np.longdouble)
    Y = np.asarray(Y).astype(np.longdouble).reshape(len(X), -1)
    n, d = X.shape
    Z = np.hstack([X, np.ones((n, 1), np.longdouble), Y])
    b = kfold_bounds(n, k)
    out = []
    for f in range(k):
        Zf = Z[b[f]:b[f + 1]]
        out.append((Zf[:, :d + 1].T @ Zf, np.abs(Zf[:, :d + 1]).T @ np.abs(Zf), int(b[f + 1] - b[f])))
    return out


def fold_sse(X, Y, W, target_of, k, chain):
    """(sse, bound), each [k, P]: sse[f, p] = Σ_{rows r of fold f} (Y[r, target_of[p]] - (X[r]·W[f, p, :d] + W[f, p, d]))² in
    np.longdouble, and the running-error bound of a float64 evaluation that forms the dot in any order, adds the intercept,
    subtracts from y, squares, and sums the squares with every term passing through at most `chain` additions (u = 2^-53):
        e_dot = γ_d Σ_j |x_j w_j|;  e_pred = e_dot + u |pred|;  e_res = e_pred + u |res|;
        bound = Σ_r (2 |res| e_res + e_res²) + γ_chain Σ_r (|res| + e_res)²."""
    X = np.asarray(X).astype(np.longdouble)
    Y = np.asarray(Y).astype(np.longdouble).reshape(len(X), -1)
    W = np.asarray(W).astype(np.longdouble)
    n, d = X.shape
    b = kfold_bounds(n, k)
    P = W.shape[1]
    sse, bound = np.zeros((k, P), np.longdouble), np.zeros((k, P), np.longdouble)
    for f in range(k):
        Xf, Yf = X[b[f]:b[f + 1]], Y[b[f]:b[f + 1]]
        w, c = W[f, :, :d], W[f, :, d]
        dot = Xf @ w.T                                              # [rows, P]
        pred = dot + c[None, :]
        res = Yf[:, np.asarray(target_of)] - pred
        e_dot = gamma(d) * (np.abs(Xf) @ np.abs(w).T)
        e_pred = e_dot + U * np.abs(pred)
        e_res = e_pred + U * np.abs(res)
        sse[f] = (res ** 2).sum(0)
        bound[f] = (2 * np.abs(res) * e_res + e_res ** 2).sum(0) + gamma(chain) * ((np.abs(res) + e_res) ** 2).sum(0)
    return sse, bound
