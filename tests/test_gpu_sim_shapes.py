"""The similarity kernels (ctgcn_sim.hip) one at a time, at the sizes where their code takes another path: the tile edges of the 32 x 32
finish and Gram tiles, the 256-column strips of the normalise and COO passes, the column ranges and panels of the series, every
boundary of numpy's pairwise sum tree, and block counts past the 1024-block cap of the grid-stride reductions.  Each kernel is held
to numpy, scipy or an exact integer mirror (_sim_ref.py, pinned on the CPU by test_sim_host.py), never to another run of itself.

Everything but the Gram is compared bit for bit.  The Gram's bound is derived: an fp64 dot of d products, chained by FMA in one
order here and summed by numpy in another, each within γ_d ≈ d·2^-53 of the exact value relative to Σ|a||b|, so the two differ by
at most d·2^-52·(|E||E|ᵀ) per entry.  Worst fraction of that bound measured on an MI355X: f32 0.052 (m = 1, d = 32), f64 0.060
(m = 31, d = 32); d = 1 is exact.  The Spearman correlation at 2049² values differed from scipy's by 1.7e-16, of the 1e-12 allowed.
"""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.stats
import torch

import _sim_ref as R
from ctgcn_amd import _lib
from ctgcn_amd._lib import check, ptr

SIM = importlib.import_module("ctgcn_amd.evaluation.similarity_prediction")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
SENTINEL = -7.25


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same_bits(got, want):
    return np.array_equal(_bits(got), _bits(want))


def _to(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV)


def _stream():
    return torch.cuda.current_stream(DEV).cuda_stream


# ================================================================================================ 1. series
def _series_graph(m, seed):
    """scipy CSR m x m float64: row i holds min(i % 10, m - 1) entries (so 0..9, every remainder of the 4-way unrolled gather and
    empty rows), sorted columns, no self loops, weights uniform in (0.1, 1): not dyadic, so a fused multiply-add changes bits."""
    rng = np.random.default_rng(seed)
    indptr, indices = [0], []
    for i in range(m):
        k = min(i % 10, m - 1)
        others = np.delete(np.arange(m), i)
        indices += sorted(rng.choice(others, k, replace=False).tolist())
        indptr.append(len(indices))
    data = rng.uniform(0.1, 1.0, len(indices))
    return sp.csr_matrix((data, np.asarray(indices, np.int32), np.asarray(indptr, np.int32)), shape=(m, m))


def _series(A, c, iters, panel, col0, col1):
    m = A.shape[0]
    lib = _lib.load()
    rp, col, val = _to(A.indptr.astype(np.int32)), _to(A.indices.astype(np.int32)), _to(A.data.astype(np.float64))
    if col.numel() == 0:                                           # no kernel argument is a null pointer
        col, val = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.float64, device=DEV)
    S = torch.full((m, m), SENTINEL, dtype=torch.float64, device=DEV)
    nb = lib.ctgcn_sim_series_workspace_bytes(m, panel)
    ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(lib.ctgcn_sim_series(m, ptr(rp), ptr(col), ptr(val), c, iters, panel, col0, col1, ptr(S), ptr(ws), nb, _stream()),
              "ctgcn_sim_series")
    return S.cpu().numpy()


@pytest.mark.parametrize("m", [1, 2, 33, 257])
def test_series_ranges_panels_and_steps(m):
    """S_k = c·A·S_{k-1} + I from S_0 = 0, restricted to the columns [col0, col1): scipy's bits inside the range (iter_num = 1 writes
    the identity), the sentinel outside it, for every panel width (1, 37, m, m + 5: one column, a width that does not divide the
    range, one panel, a panel wider than the block) and an empty range."""
    A = _series_graph(m, 100 + m)
    assert m < 33 or sorted(set(np.diff(A.indptr).tolist())) == list(range(10))
    c = 0.37 / 1.9
    eye = np.eye(m)
    ranges = [(0, m), (min(5, m), min(5, m))] + ([(3, m - 2)] if m >= 5 else [])
    S = np.zeros((m, m))
    calls = 0
    for it in range(1, 9):
        S = c * A.dot(S) + eye
        if it not in (1, 2, 3, 8):
            continue
        assert it > 1 or np.array_equal(S, eye)
        for panel in (1, 37, m, m + 5):
            for col0, col1 in ranges:
                got = _series(A, c, it, panel, col0, col1)
                inside = np.zeros(m, bool)
                inside[col0:col1] = True
                where = "m %d iter %d panel %d cols [%d, %d)" % (m, it, panel, col0, col1)
                assert _same_bits(got[:, inside], S[:, inside]), where
                assert np.all(got[:, ~inside] == SENTINEL), where + ": wrote outside the range"
                calls += 1
    assert calls == 4 * 4 * len(ranges)


# ================================================================================================ 2. finish
EPS = 1e-6


def _finish(S, pad_zero, eps=EPS):
    m = len(S)
    lib = _lib.load()
    St = _to(S)
    stats = torch.empty(2, dtype=torch.float64, device=DEV)
    nnz = torch.empty(m, dtype=torch.int64, device=DEV)
    nb = lib.ctgcn_sim_finish_workspace_bytes(m)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(lib.ctgcn_sim_finish(m, pad_zero, eps, ptr(St), ptr(stats), ptr(nnz), ptr(ws), nb, _stream()), "ctgcn_sim_finish")
    return St.cpu().numpy(), stats.cpu().numpy(), nnz.cpu().numpy()


def _check_finish(S, pad_zero, where):
    got, stats, nnz = _finish(S, pad_zero)
    want, (mn, mx), want_nnz = R.finish(S, pad_zero, EPS)
    assert _same_bits(stats, [mn, mx]), (where, stats, mn, mx)
    assert np.array_equal(_bits(got), _bits(want)) or (np.isnan(want).any() and np.array_equal(got, want, equal_nan=True)), where
    assert np.array_equal(nnz, want_nnz), where
    return want, (mn, mx), want_nnz


def _extreme_spots(m):
    """(name, i, j) of the places an extreme is put: the last partial (or last) tile off its diagonal, the diagonal, and strictly
    below the diagonal of the lower tile of an off-diagonal tile pair."""
    spots = [("diagonal", m // 2, m // 2)]
    if m >= 2:
        spots.append(("last tile", m - 1, m - 2))
    if m >= 38:
        spots.append(("below the diagonal of tile (1, 0)", 32 + 5, 2))
    return spots


@pytest.mark.parametrize("m", [31, 32, 33, 64, 65, 257])
@pytest.mark.parametrize("pad_zero", [0, 1])
def test_finish_extremes_in_every_tile_kind(m, pad_zero):
    """(S + Sᵀ)/2 - I, min-max, threshold on an asymmetric random block, with the global minimum and then the global maximum placed in
    turn in each kind of tile: stats, the block and the per-row counts are the numpy mirror's bits."""
    rng = np.random.default_rng(m)
    base = rng.uniform(-1.0, 1.0, (m, m))
    assert not np.array_equal(base, base.T)
    _check_finish(base, pad_zero, "m %d random" % m)
    for name, i, j in _extreme_spots(m):
        for sign in (-1.0, 1.0):
            S = base.copy()
            S[i, j], S[j, i] = (sign * 7.5, sign * 2.5) if i != j else (sign * 5.0 + 1.0,) * 2       # symmetrised: ±5 at (i, j)
            want, (mn, mx), _ = _check_finish(S, pad_zero, "m %d %s %+g" % (m, name, sign))
            assert (mn if sign < 0 else mx) == sign * 5.0
            assert want[i, j] == (0.0 if sign < 0 else 1.0)


@pytest.mark.parametrize("m", [1, 33, 65])
def test_finish_all_negative_block_pads_with_zero(m):
    """Every entry negative and pad_zero = 1: the maximum is the 0 of the isolated vertices' rows, not an entry of the block."""
    S = np.random.default_rng(m).uniform(-3.0, -1.0, (m, m))
    _, (mn, mx), _ = _check_finish(S, 1, "m %d all negative" % m)
    assert mx == 0.0 and mn < -1.0
    got, stats, _ = _finish(S, 1)
    assert stats[1] == 0.0 and not np.signbit(stats[1]) and got.max() < 1.0


@pytest.mark.parametrize("m", [33, 257])
def test_finish_threshold_at_eps(m):
    """Extremes exactly 0 and 1, so an entry scales to itself: eps stays, the double below it becomes 0, the double above stays."""
    rng = np.random.default_rng(m)
    S = rng.uniform(0.1, 0.9, (m, m))
    S[np.diag_indices(m)] += 1.0
    below, above = np.nextafter(EPS, 0.0), np.nextafter(EPS, 1.0)
    spots = {(1, 0): 0.0, (2, 0): 1.0, (m - 1, 3): EPS, (m - 2, 4): below, (m - 1, m - 3): above}
    for (i, j), v in spots.items():
        S[i, j] = S[j, i] = v
    want, (mn, mx), nnz = _check_finish(S, 0, "m %d eps" % m)
    assert (mn, mx) == (0.0, 1.0)
    assert want[m - 1, 3] == EPS and want[m - 2, 4] == 0.0 and want[m - 1, m - 3] == above
    assert nnz[m - 2] == m - 1 and nnz[m - 1] == m


def test_finish_single_vertex_is_nan_and_counted():
    """m = 1: min == max, so the scaling is 0/0.  numpy gives NaN, np.nonzero counts it, and so must the kernel."""
    want, (mn, mx), nnz = _check_finish(np.array([[1.75]]), 0, "m 1")
    assert mn == mx == 0.75 and np.isnan(want[0, 0]) and nnz.tolist() == [1]
    got, _, got_nnz = _finish(np.array([[1.75]]), 0)
    assert np.isnan(got[0, 0]) and got_nnz.tolist() == [1]
    want, _, nnz = _check_finish(np.array([[1.75]]), 1, "m 1 padded")                  # with the 0 of other rows: (0.75 - 0)/0.75
    assert want[0, 0] == 1.0 and nnz.tolist() == [1]


# ================================================================================================ 3. COO
@pytest.mark.parametrize("m", [1, 63, 64, 65, 256, 257, 600])
def test_coo_is_numpys_nonzero_in_row_major_order(m):
    rng = np.random.default_rng(m)
    S = np.where(rng.random((m, m)) < 0.3, rng.uniform(0.1, 1.0, (m, m)), 0.0)
    lone = [c for c in (0, 255, 256, m - 1) if c < m]
    for k, r in enumerate(range(0, m, 7)):                         # every 7th row in turn: empty, full, one entry at a strip edge
        S[r] = 0.0
        kind = k % (2 + len(lone))
        if kind == 1:
            S[r] = rng.uniform(0.1, 1.0, m)
        elif kind >= 2:
            S[r, lone[kind - 2]] = 0.5 + k
    if m == 1:
        S[0, 0] = 0.25
    ids = 3 * np.arange(m, dtype=np.int64) + 2                      # increasing, not the identity
    nnz = np.count_nonzero(S, axis=1).astype(np.int64)
    assert m < 63 or (nnz.min() == 0 and nnz.max() == m)
    off = np.cumsum(nnz) - nnz
    total = int(nnz.sum())
    row = torch.full((total + 1,), -1, dtype=torch.int32, device=DEV)
    col = torch.full((total + 1,), -1, dtype=torch.int32, device=DEV)
    data = torch.full((total + 1,), SENTINEL, dtype=torch.float64, device=DEV)
    St, offt, idst = _to(S), _to(off), _to(ids)
    with torch.cuda.device(DEV):
        check(_lib.load().ctgcn_sim_coo(m, ptr(St), ptr(offt), ptr(idst), ptr(row), ptr(col), ptr(data), _stream()), "ctgcn_sim_coo")
    r, c = np.nonzero(S)
    assert np.array_equal(row.cpu().numpy()[:total], ids[r].astype(np.int32))
    assert np.array_equal(col.cpu().numpy()[:total], ids[c].astype(np.int32))
    assert _same_bits(data.cpu().numpy()[:total], S[r, c])
    assert row[total].item() == -1 and col[total].item() == -1 and data[total].item() == SENTINEL      # nothing past the end


# ================================================================================================ 4. Gram
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_gram_tile_edges_views_and_repeated_rows(dtype):
    """E[rows] E[rows]ᵀ at the 32-edges of m and d, on a contiguous embedding (lde = d) and a column-sliced view (lde = d + 3), with
    unordered rows and a repeat: exactly symmetric, and within d·2^-52·(|E||E|ᵀ) of numpy's float64 product (module docstring)."""
    worst = (-1.0, None)
    for m in (1, 31, 32, 33, 65):
        for d in (1, 31, 32, 33, 100):
            for pad in (0, 3):
                rng = np.random.default_rng(1000 * m + 10 * d + pad)
                n = m + 7
                base = torch.from_numpy(rng.standard_normal((n, d + pad))).to(dtype).to(DEV)
                E = base[:, 1:d + 1] if pad else base
                assert E.stride(0) == d + pad and E.stride(1) == 1 and E.shape == (n, d)
                rows = rng.permutation(n)[:m]
                if m > 1:
                    rows[-1] = rows[0]
                assert m < 3 or (np.any(np.diff(rows) < 0) and len(set(rows.tolist())) == m - 1)
                out = SIM.gram(E, torch.from_numpy(rows))
                assert out.shape == (m, m) and torch.equal(out, out.T), (m, d, pad)
                E64 = E.cpu().numpy().astype(np.float64)[rows]
                ref = E64 @ E64.T
                bound = d * 2.0 ** -52 * (np.abs(E64) @ np.abs(E64).T)
                err = np.abs(out.cpu().numpy() - ref)
                frac = float((err / bound).max())
                assert frac <= 1.0, "gram m %d d %d lde %d: %.3f of the bound" % (m, d, d + pad, frac)
                if m > 1:
                    assert out[0, -1].item() == out[0, 0].item() == out[-1, -1].item()           # the repeated row
                if frac > worst[0]:
                    worst = (frac, (m, d, d + pad))
    print("  [bound] sim_gram %s: worst %.3f of d·2^-52·|E||E|ᵀ at (m, d, lde) = %s" % (dtype, worst[0], worst[1]))


# ================================================================================================ 5. normalise
@pytest.mark.parametrize("N", [2, 7, 8, 9, 127, 128, 129, 136, 137, 4097, 8191, 8192, 8193, 16385, 2049 * 2049])
def test_normalize_is_numpys_to_the_bit(N):
    """(x - min)/(max - min), then / sum: min, max, the sum and every value are numpy's own bits, at each boundary of numpy's sum tree
    (below 8, the 8 running sums, blocks of 128, halves cut at multiples of 8, chunks of 8192) and, at 2049² values, with more
    blocks of 4096 than the 1024 the reductions launch (a square 2-D block there, as the predictor's are)."""
    side = int(round(N ** 0.5))
    for draw in range(8 if N < 100_000 else 1):                     # one draw tells two summation orders apart only about half the time
        x = np.random.default_rng(1000 * draw + N).uniform(-2.0, 5.0, N)
        if side * side == N and N > 9:
            x = x.reshape(side, side)
        want, (mn, mx, s) = R.normalize(x)
        xt = _to(x)
        got = SIM._normalize(xt)
        assert _same_bits(got, [mn, mx, s]), (N, draw, got, (mn, mx, s))
        assert _same_bits(xt.cpu().numpy(), want), (N, draw)


# ================================================================================================ 6. Spearman
def _spearman_sums(x, y):
    lib = _lib.load()
    N = len(x)
    xs, xi = torch.sort(_to(x), stable=True)
    ys, yi = torch.sort(_to(y), stable=True)
    sums = torch.empty(3, dtype=torch.float64, device=DEV)
    nb = lib.ctgcn_sim_spearman_workspace_bytes(N)
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    with torch.cuda.device(DEV):
        check(lib.ctgcn_sim_spearman(N, ptr(xs), ptr(xi), ptr(ys), ptr(yi), ptr(sums), ptr(ws), nb, _stream()), "ctgcn_sim_spearman")
    return tuple(sums.cpu().numpy().tolist())


def _tie_patterns(N, rng):
    """x of three kinds: all distinct; one tie run that starts before sorted position 256 and ends after it (the whole array when
    N is shorter); everything equal except one value."""
    distinct = rng.permutation(N).astype(np.float64)
    run = distinct.copy()
    lo, hi = (250, 263) if N > 263 else (max(N - 2, 0), N)
    run[(run >= lo) & (run < hi)] = lo
    flat = np.full(N, 0.5)
    flat[N // 2] = 2.0
    return {"distinct": distinct, "tie run": run, "all but one equal": flat}


@pytest.mark.parametrize("N", [2, 3, 255, 256, 257, 4096, 4097, 8193])
def test_spearman_sums_are_exact(N):
    """Below 200 000 values the three sums are sums of multiples of 1/4 that stay under 2^53: exact in any order, so the kernel's must
    equal the integer mirror's bit for bit, for every tie pattern on either side."""
    rng = np.random.default_rng(N)
    xs = _tie_patterns(N, rng)
    ys = _tie_patterns(N, rng)
    ys["few values"] = rng.integers(0, 4, N).astype(np.float64)
    for xn, x in xs.items():
        for yn, y in ys.items():
            want = R.spearman_sums(x, y)
            assert _spearman_sums(x, y) == want, (N, xn, yn)
            rho = SIM.spearman(_to(x), _to(y))
            if want[1] == 0.0 or want[2] == 0.0:
                assert np.isnan(rho)
            else:
                assert rho == want[0] / np.sqrt(want[1] * want[2])
    const = np.full(N, 0.3)
    assert _spearman_sums(const, xs["distinct"])[1] == 0.0
    assert np.isnan(SIM.spearman(_to(const), _to(xs["distinct"])))
    assert np.isnan(SIM.spearman(_to(xs["distinct"]), _to(const)))


def test_spearman_past_the_block_cap_matches_scipy():
    """2049² values: 1025 blocks of 4096 would be needed, 1024 are launched, so the rank and correlation loops wrap.  Ties on both
    sides; the correlation is scipy's within the 1e-12 of test_gpu_similarity_prediction.py."""
    N = 2049 * 2049
    rng = np.random.default_rng(9)
    x = rng.integers(0, 50_000, N).astype(np.float64) * 0.1
    y = np.where(rng.random(N) < 0.5, 0.0, rng.random(N))
    y[: N // 3] = x[: N // 3] * 2 + 0.5
    want = scipy.stats.spearmanr(x, y)[0]
    got = SIM.spearman(_to(x), _to(y))
    print("  [tol] spearman at 2049^2: |ours - scipy| = %.3e = %.6f of 1e-12" % (abs(got - want), abs(got - want) / 1e-12))
    assert abs(got - want) <= 1e-12, (got, want)
