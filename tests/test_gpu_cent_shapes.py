"""The centrality kernels (ctgcn_cent.hip) at the sizes where their code takes another path: every lane-group width of the Brandes
passes on a graph whose BFS level sizes are chosen, source ranges of every kind, the memory cap on the number of Brandes blocks, the
block cap of the eigenvector passes, and the two ridge passes called directly at their tile, fold and chunk edges.  References:
_central_ref.py (numpy / scipy, pinned against networkx and sklearn by test_centrality_host.py), closed forms, and np.longdouble
mirrors of the ridge passes.

Derived bounds (u = 2^-53; nothing here is tuned to pass):
  ridge Gram  every entry of a fold's Gram is a sum of rows_f products, formed by FMA chains of at most ceil(rows_f / 16) terms
              and a sum of 16 partials.  Any such order is within γ_{rows_f} Σ|z_i z_j| of the exact sum, and the long-double mirror
              adds 2^-64-sized errors, so the bound is rows_f · 2^-52 · (|Z_f|ᵀ|Z_f|) per entry, twice the first-order term.
  ridge SSE   the running-error bound of _central_ref.fold_sse: e_dot = γ_d Σ|x_j w_j|, e_pred = e_dot + u|pred|,
              e_res = e_pred + u|res|, bound = Σ_r (2|res| e_res + e_res²) + γ_K Σ_r (|res| + e_res)², where K counts the additions
              a square passes through: its FMA, the rows a wave takes of a chunk share (ceil(ceil(rows_f / 16) / 32)), the 4 waves
              of a block and the 128 block partials of a fold.
Worst fractions of these bounds measured on an MI355X: ridge Gram f32 0.485, f64 0.494 (both at n = F = 5, d = 62: one row per fold, so
one rounding against a bound of two); ridge SSE f32 0.260 (n = F = 5, d = 1, P = 63), f64 0.420 (n = F = 2, d = 1, P = 64).  Brandes
used at most 1.2e-5 of its 1e-10 · max|bc| (all 560 sources), the eigenvector at most 1.7e-15 of its 1e-12 (n = 262 358), and the
ridge wrapper 1.3e-15 of its 1e-8.
"""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _central_ref as R
from ctgcn_amd import _lib
from ctgcn_amd._lib import check, ptr

CP = importlib.import_module("ctgcn_amd.evaluation.centrality_prediction")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
ISOLATED = 6


def _dev(indptr, indices):
    return torch.from_numpy(np.asarray(indptr, np.int32)).to(DEV), torch.from_numpy(np.asarray(indices, np.int32)).to(DEV)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ================================================================================================ Brandes on chosen level sizes
_LAYERED = {}


def _layered():
    """The layered graph (level sizes 1, 4, 5, 8, 9, 16, 17, 32, 33, 64, 65, 300 from vertex 0, then 6 isolated vertices) and the
    reference's result for every source, computed once."""
    if not _LAYERED:
        n, (indptr, indices), levels = R.layered(isolated=ISOLATED)
        bc, r, D = R.brandes(indptr, indices, n)
        per_source = {}
        _LAYERED.update(n=n, indptr=indptr, indices=indices, levels=levels, r=r, D=D, bc=bc, per_source=per_source)
    return _LAYERED


def _ref_range(g, s0, s1):
    key = (s0, s1)
    if key not in g["per_source"]:
        g["per_source"][key] = R.brandes(g["indptr"], g["indices"], g["n"], sources=np.arange(s0, s1))[0] if s1 > s0 else np.zeros(g["n"])
    return g["per_source"][key], g["r"][s0:s1], g["D"][s0:s1]


def _check_range(g, s0, s1, what):
    rp, col = _dev(g["indptr"], g["indices"])
    bc, r, D = CP.brandes(rp, col, s0, s1)
    bc2, r2, D2 = CP.brandes(rp, col, s0, s1)
    assert torch.equal(bc, bc2) and torch.equal(r, r2) and torch.equal(D, D2), what + ": a repeated call differs"
    ref_bc, ref_r, ref_D = _ref_range(g, s0, s1)
    assert r.shape == (s1 - s0,) and D.shape == (s1 - s0,)
    assert np.array_equal(r.cpu().numpy(), ref_r) and np.array_equal(D.cpu().numpy(), ref_D), what
    err = np.abs(bc.cpu().numpy() - ref_bc).max()
    tol = 1e-10 * np.abs(ref_bc).max()
    print("  [tol] brandes %-40s max |err| %.3e of %.3e allowed" % (what, err, tol))
    assert err <= tol, what
    return bc.cpu().numpy()


def test_brandes_every_group_width_from_three_sources():
    """Level sizes 1 and 4 give 64 lanes per vertex, 5 and 8 give 32, 9 and 16 give 16, 17 and 32 give 8, 33 and more give 4, in the
    discover, sigma and backward passes alike.  From vertex 0 the levels are the layers; from a vertex of the 65-layer the first
    frontier is one vertex with a row of more than 64 entries; from the last vertex of the 300-layer the sizes come the other way."""
    g = _layered()
    n_conn = g["n"] - ISOLATED
    mid = int(np.flatnonzero(g["levels"] == 10)[0])
    assert g["indptr"][mid + 1] - g["indptr"][mid] > 64
    for s, what in ((0, "source 0"), (mid, "a source in the 65-layer"), (n_conn - 1, "the last connected vertex")):
        bc = _check_range(g, s, s + 1, what)
        assert bc[s] == 0.0 and not bc[n_conn:].any()
    assert g["r"][0] == n_conn and g["D"][0] == int((np.arange(len(R.LAYER_SIZES)) * R.LAYER_SIZES).sum())


def test_brandes_source_ranges():
    """On the layered graph: a range that starts past 0, all 560 sources (more than the 512 blocks, so blocks take a second source),
    a range of isolated sources only (r = 1, D = 0, no dependency) and an empty range (all zeros)."""
    g = _layered()
    n = g["n"]
    _check_range(g, 100, 140, "s0 > 0")
    _check_range(g, 0, n, "all %d sources: more than the 512 blocks" % n)
    assert n > 512
    bc = _check_range(g, n - ISOLATED, n, "isolated sources only")
    assert not bc.any()
    rp, col = _dev(g["indptr"], g["indices"])
    _, r, D = CP.brandes(rp, col, n - ISOLATED, n)
    assert r.tolist() == [1] * ISOLATED and D.tolist() == [0] * ISOLATED
    bc, r, D = CP.brandes(rp, col, 7, 7)                            # an empty range: all zeros, nothing launched
    assert bc.shape == (n,) and not bc.any() and r.numel() == 0 and D.numel() == 0


def test_brandes_block_count_capped_by_memory():
    """A star on n = 120 001 vertices (hub 0) from the sources 0..599.  A slab takes 36 n + 8 bytes rounded up to 256 = 4 320 256, so
    the 2 GiB budget holds 497 of them: fewer blocks than the 512 of the grid cap, and than the sources, so blocks loop.
    Closed form: from the hub every leaf is at distance 1 and is nobody's predecessor, so r = n, D = n - 1 and no dependency.  From
    a leaf the hub is at distance 1 and the other n - 2 leaves at distance 2, each with the hub as its only predecessor and one path:
    delta[hub] = sigma[hub] Σ (1 + 0) / 1 = n - 2, every other delta is 0, r = n, D = 1 + 2 (n - 2).  Over the hub and 599 leaves
    bc[hub] = 599 (n - 2), an integer below 2^53, and every other entry is 0: exact."""
    n, k = 120_001, 600
    lib = _lib.load()
    slab = (36 * n + 8 + 255) // 256 * 256
    assert lib.ctgcn_cent_brandes_workspace_bytes(n, 0, k) == (2 ** 31 // slab) * slab and 2 ** 31 // slab == 497
    rp, col = _dev(*R.star(n))
    bc, r, D = CP.brandes(rp, col, 0, k)
    want = np.zeros(n)
    want[0] = (k - 1) * (n - 2)
    assert np.array_equal(bc.cpu().numpy(), want)
    assert np.array_equal(r.cpu().numpy(), np.full(k, n))
    assert np.array_equal(D.cpu().numpy(), np.array([n - 1] + [1 + 2 * (n - 2)] * (k - 1)))


# ================================================================================================ eigenvector
def _eig_raw(rp, col, max_iter, tol):
    """ctgcn_cent_eigenvector itself: (x, stop step), stop 0 when no step passed the test (the wrapper raises there)."""
    lib = _lib.load()
    n = rp.numel() - 1
    rp, col = CP._csr(rp, col)
    x = torch.empty(n, dtype=torch.float64, device=DEV)
    stop = ctypes.c_int32(-1)
    nb = lib.ctgcn_cent_eigenvector_workspace_bytes(n)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(lib.ctgcn_cent_eigenvector(n, ptr(rp), ptr(col), max_iter, tol, ptr(x), ctypes.byref(stop), ptr(ws), nb, _stream()),
              "ctgcn_cent_eigenvector")
    return x.cpu().numpy(), stop.value


def _eig_graph(n):
    if n == 1:
        return 1, R.csr(1, np.zeros((0, 2), np.int64))
    if n <= 257:
        return R.cliques([40, 17] + [3] * 60, isolated=n - 237)
    return R.cliques([40, 17] + [3] * 60000 + [2] * 41000, isolated=301)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 262_358])
def test_eigenvector_block_edges_and_past_the_block_cap(n):
    """One block short of full, full, one vertex into the next block, and n = 262 358: 1025 blocks of 256 would be needed, 1024 are
    launched, so the products' and the scaling's loops wrap, and n is no multiple of 256."""
    nn, (indptr, indices) = _eig_graph(n)
    assert nn == n
    rp, col = _dev(indptr, indices)
    ref_x, ref_stop = R.eigenvector(indptr, indices, n)
    x, stop = CP.eigenvector(rp, col)
    err = np.abs(x.cpu().numpy() - ref_x).max()
    print("  [tol] eigenvector n %-7d stop %d  max |err| %.3e = %.4f of 1e-12" % (n, stop, err, err / 1e-12))
    assert stop == ref_stop and err <= 1e-12
    # no step at all: the start vector and "not converged"
    x0, stop0 = _eig_raw(rp, col, 0, 1e-6)
    assert stop0 == 0 and np.array_equal(x0, np.full(n, 1.0 / n))
    with pytest.raises(CP.PowerIterationFailedConvergence):
        CP.eigenvector(rp, col, max_iter=0)
    # a tolerance the first step passes
    ref_x1, ref_stop1 = R.eigenvector(indptr, indices, n, tol=10.0)
    x1, stop1 = CP.eigenvector(rp, col, tol=10.0)
    assert stop1 == ref_stop1 == 1 and np.abs(x1.cpu().numpy() - ref_x1).max() <= 1e-12
    assert _eig_raw(rp, col, 100, 10.0)[1] == 1


# ================================================================================================ ridge passes, called directly
# (n, F, d, T): every (n, F) and every d and T of the list, d = 512 with T = 8 and d = 63 with T = 1 among them.  n == F gives folds of
# one row, (7, 3) folds of 3, 2, 2 rows and (33, 2) folds of 17 and 16: all shorter than or about the 16 row chunks of a fold;
# d + 1 = 64 and d + 1 + T = 64 or 65 sit on the 64-wide tile edge.
RIDGE_CASES = [(2, 2, 1, 1), (5, 5, 62, 1), (5, 5, 1, 8), (7, 3, 63, 1), (7, 3, 512, 8), (33, 2, 63, 4), (33, 2, 512, 8), (33, 2, 64, 8),
               (100, 5, 64, 4), (100, 5, 127, 1), (2003, 5, 65, 8), (2003, 5, 128, 4), (2003, 5, 63, 1)]


def _ridge_inputs(n, F, d, T, dtype, pad):
    rng = np.random.default_rng(10000 * n + 10 * d + T + pad)
    base = torch.from_numpy(rng.standard_normal((n, d + pad)) * 0.5 + 0.1).to(dtype).to(DEV)
    X = base[:, pad - 2:pad - 2 + d] if pad else base               # ldx = d + 5 and a first column 3 elements in
    assert X.stride(0) == d + pad and X.stride(1) == 1 and X.shape == (n, d)
    Y = torch.from_numpy(rng.standard_normal((n, T)) + 0.5).to(DEV)
    return X, Y


def _ridge_gram(X, Y, F):
    lib = _lib.load()
    n, d = X.shape
    T = Y.shape[1]
    suffix = "f32" if X.dtype == torch.float32 else "f64"
    gram = torch.full((F, d + 1, d + 1 + T), float("nan"), dtype=torch.float64, device=DEV)
    nb = lib.ctgcn_ridge_gram_workspace_bytes(d, T, F)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(getattr(lib, "ctgcn_ridge_gram_" + suffix)(n, d, T, F, ptr(X), X.stride(0), ptr(Y), ptr(gram), ptr(ws), nb, _stream()),
              "ctgcn_ridge_gram_" + suffix)
    return gram.cpu().numpy()


def _ridge_sse(X, Y, W, tgt, F):
    lib = _lib.load()
    n, d = X.shape
    T, P = Y.shape[1], W.shape[1]
    suffix = "f32" if X.dtype == torch.float32 else "f64"
    sse = torch.full((F, P), float("nan"), dtype=torch.float64, device=DEV)
    nb = lib.ctgcn_ridge_sse_workspace_bytes(P, F)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(getattr(lib, "ctgcn_ridge_sse_" + suffix)(n, d, T, F, P, ptr(X), X.stride(0), ptr(Y), ptr(W), ptr(tgt), ptr(sse), ptr(ws), nb,
                                                       _stream()), "ctgcn_ridge_sse_" + suffix)
    return sse.cpu().numpy()


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,F,d,T", RIDGE_CASES)
def test_ridge_gram_against_long_double(n, F, d, T, dtype):
    """Each fold's [d+1, d+1+T] block of [X 1]ᵀ[X 1 Y] against the long-double product of the fold's own rows, with ldx = d and with
    ldx = d + 5: within rows_f · 2^-52 · (|Z_f|ᵀ|Z_f|) per entry (module docstring).  A row dropped, doubled or given to the wrong
    fold moves an entry by a whole product."""
    for pad in (0, 5):
        X, Y = _ridge_inputs(n, F, d, T, dtype, pad)
        got = _ridge_gram(X, Y, F)
        worst = 0.0
        for f, (want, absg, rows) in enumerate(R.fold_grams(X.cpu().numpy(), Y.cpu().numpy(), F)):
            bound = rows * 2.0 ** -52 * absg
            assert got[f, d, d] == rows
            frac = float((np.abs(got[f] - want) / bound).max())
            assert frac <= 1.0, "ridge_gram (n %d F %d d %d T %d ldx %d) fold %d: %.3f of the bound" % (n, F, d, T, d + pad, f, frac)
            worst = max(worst, frac)
        print("  [bound] ridge_gram n %d F %d d %d T %d ldx %d %s: %.3f of rows·2^-52·|Z|ᵀ|Z|" % (n, F, d, T, d + pad, dtype, worst))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("n,F,d,T", RIDGE_CASES)
def test_ridge_sse_against_long_double(n, F, d, T, dtype):
    """Held-out squared errors of P in {1, 63, 64} models with random weights (no solve, so conditioning plays no part) and a target
    map that is not arange % T, with ldx = d and ldx = d + 5, against the long-double mirror within its running-error bound."""
    for pad, P in ((0, 1), (5, 63), (0, 64)):
        X, Y = _ridge_inputs(n, F, d, T, dtype, pad)
        rng = np.random.default_rng(P + d)
        W = torch.from_numpy(rng.standard_normal((F, P, d + 1)) * (0.5 / np.sqrt(d))).to(DEV)
        tgt = (T - 1 - (5 * np.arange(P) + 3) % T).astype(np.int32)
        assert P == 1 or T == 1 or not np.array_equal(tgt, np.arange(P) % T)
        got = _ridge_sse(X, Y, W, torch.from_numpy(tgt).to(DEV), F)
        rows_max = -(-n // F)
        chain = 1 + -(-(-(-rows_max // 16)) // 32) + 4 + 128
        want, bound = R.fold_sse(X.cpu().numpy(), Y.cpu().numpy(), W.cpu().numpy(), tgt, F, chain)
        frac = float((np.abs(got - want) / bound).max())
        print("  [bound] ridge_sse n %d F %d d %d T %d P %d ldx %d %s: %.3f of the running-error bound (bound / sse at most %.1e)"
              % (n, F, d, T, P, d + pad, dtype, frac, float((bound / want).max())))
        assert frac <= 1.0, "ridge_sse (n %d F %d d %d T %d P %d ldx %d): %.3f of the bound" % (n, F, d, T, P, d + pad, frac)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_ridge_wrapper_tiny_folds_and_strided_rows(dtype):
    """ridge_cv_errors end to end where the folds are 3, 2 and 2 rows, and on an embedding whose rows are d + 5 apart, against the
    numpy Gram form within the 1e-8 of test_gpu_centrality.py.  alpha >= 1 keeps the 4-row training systems well conditioned."""
    alphas = [1.0, 10.0]
    for n, F, d, T, pad in ((7, 3, 3, 2, 0), (203, 5, 37, 4, 5)):
        X, Y = _ridge_inputs(n, F, d, T, dtype, pad)
        Y = Y.abs() + 0.1                                           # the error is divided by mean(y)
        ours = CP.ridge_cv_errors(X, Y, alphas, F)
        ref = R.ridge_cv_errors(X.cpu().numpy().astype(np.float64), Y.cpu().numpy(), alphas, F)
        used = np.abs(ours / ref - 1).max()
        print("  [tol] ridge_cv_errors n %d F %d d %d ldx %d %s: %.3e = %.4f of 1e-8" % (n, F, d, d + pad, dtype, used, used / 1e-8))
        assert used <= 1e-8
