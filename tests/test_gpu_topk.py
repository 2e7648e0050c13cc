"""ops.topk_scores (ctgcn_topk.hip) against the float64 host model of tests/_topk_ref.py.

Exact cases: embeddings are integers in [-4, 4] and biases multiples of 0.5 in [-64, 64], so every score is exact in fp32 in any
order (|s| <= 16 * 512 + 128 < 2^24) and score and index must EQUAL the model entry for entry, padding included."""
import numpy as np
import pytest
import torch

import _topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ints(n, d, seed):
    return np.random.default_rng(seed).integers(-4, 5, size=(n, d)).astype(np.float32)


def _halves(n, seed):
    return (np.random.default_rng(seed).integers(-128, 129, size=n) * 0.5).astype(np.float32)


def _device_E(E, layout):
    """E on the device: 'dense'; 'padded' (lde = d + 4: 16-byte rows whenever d % 4 == 0); 'offset' (lde = d + 3 and the base one
    float past an aligned address: the element-by-element path)"""
    n, d = E.shape
    t = torch.from_numpy(E)
    if layout == "dense":
        return t.to(DEV)
    lde, off = (d + 4, 0) if layout == "padded" else (d + 3, 1)
    buf = torch.full((n * lde + off + 8,), 7.0, dtype=torch.float32, device=DEV)       # a 7 read from the padding breaks a score
    view = buf[off:off + n * lde].view(n, lde)[:, :d]
    view.copy_(t)
    assert view.data_ptr() % 16 == 4 * off and view.stride(0) == lde
    return view


def _adj(n, pairs):
    from ctgcn_amd import ops
    row_ptr, col = R.csr_from_pairs(n, pairs)
    t = lambda a: torch.from_numpy(a).to(DEV)
    return ops.GcnAdj(t(row_ptr), t(col), torch.ones(len(col), dtype=torch.float32, device=DEV)), (row_ptr, col)


def _check_exact(E, k, layout="dense", rows=None, row_bias=None, col_bias=None, exclude_self=False, upper_only=False, pairs=None,
                 col_chunks=None):
    from ctgcn_amd import ops
    n = E.shape[0]
    adj, csr = _adj(n, pairs) if pairs is not None else (None, None)
    dev = lambda a: None if a is None else torch.from_numpy(np.asarray(a)).to(DEV)
    score, index = ops.topk_scores(_device_E(E, layout), k, rows=dev(rows), row_bias=dev(row_bias), col_bias=dev(col_bias),
                                   exclude_self=exclude_self, upper_only=upper_only, exclude=adj, col_chunks=col_chunks)
    ref_s, ref_i = R.topk(E, k, rows, row_bias, col_bias, exclude_self, upper_only, csr)
    assert score.dtype == torch.float32 and index.dtype == torch.int32 and tuple(score.shape) == tuple(index.shape) == ref_s.shape
    got_s, got_i = score.cpu().numpy().astype(np.float64), index.cpu().numpy()
    assert np.array_equal(got_i, ref_i), "index differs in %d entries" % int((got_i != ref_i).sum())
    assert np.array_equal(got_s, ref_s), "score differs in %d entries" % int((got_s != ref_s).sum())
    return score, index


@pytest.mark.parametrize("n", [1, 31, 32, 33, 63, 64, 65, 1000])
def test_exact_every_n(n):
    E = _ints(n, 33, n)
    _check_exact(E, 33, "padded", row_bias=_halves(n, 1), col_bias=_halves(n, 2), exclude_self=True, col_chunks=2)
    _check_exact(E, 33, "offset", col_chunks=1)


@pytest.mark.parametrize("k", [1, 2, 31, 32, 33, 128])
def test_exact_every_k(k):
    _check_exact(_ints(100, 5, k), k, exclude_self=True, col_bias=_halves(100, 3))        # k = 128 > 99 admissible: padding
    _check_exact(_ints(1000, 8, k + 1), k, col_chunks=3)


@pytest.mark.parametrize("d", [1, 2, 3, 5, 31, 32, 33, 127, 128, 129, 512])
def test_exact_every_d_and_layout(d):
    E = _ints(65, d, d)
    for layout in ("dense", "padded", "offset"):
        _check_exact(E, 32, layout, row_bias=_halves(65, 4), col_bias=_halves(65, 5), col_chunks=2)


def test_exact_rows_a_permuted_subset_with_repeats():
    n = 200
    E = _ints(n, 17, 9)
    rows = np.random.default_rng(5).permutation(n)[:70].astype(np.int64)
    rows = np.concatenate([rows, rows[:9], rows[3:4]])
    for flags in ((True, False), (False, True)):
        _check_exact(E, 20, rows=rows, row_bias=_halves(len(rows), 6), col_bias=_halves(n, 7), exclude_self=flags[0], upper_only=flags[1])
    _check_exact(E, 20, rows=rows.astype(np.int32), col_chunks=7)


@pytest.mark.parametrize("col_chunks", [1, 2, 7, 40])
def test_exact_every_col_chunks(col_chunks):
    """n = 1000 is 32 column tiles: 40 chunks leave some of them empty"""
    _check_exact(_ints(1000, 31, 11), 128, "offset", col_bias=_halves(1000, 8), exclude_self=True, col_chunks=col_chunks)


def test_chunk_identity_and_repeatability():
    from ctgcn_amd import ops
    g = torch.Generator().manual_seed(3)
    E = torch.randn(1000, 128, generator=g).to(DEV)
    bias = torch.randn(1000, generator=g).to(DEV)
    runs = [ops.topk_scores(E, 50, row_bias=bias, col_bias=bias, exclude_self=True, col_chunks=c) for c in (1, 2, 7, 7, None)]
    for s, i in runs[1:]:
        assert torch.equal(s.view(torch.int32), runs[0][0].view(torch.int32)) and torch.equal(i, runs[0][1])


def test_exact_ties_duplicated_rows_and_all_equal_scores():
    E = _ints(40, 6, 13)
    E = np.concatenate([E, E, E[:17]])                                   # every score occurs at least twice
    _check_exact(E, 33, exclude_self=True, col_chunks=2)
    _check_exact(np.zeros((130, 4), dtype=np.float32), 64, upper_only=True, col_chunks=3)       # E = 0: the order is the index


def test_exact_ascending_scores_insert_every_candidate():
    n = 257
    _check_exact(np.zeros((n, 3), dtype=np.float32), 32, col_bias=(-64 + 0.5 * np.arange(n)).astype(np.float32), col_chunks=1)
    _check_exact(np.zeros((n, 3), dtype=np.float32), 128, col_bias=(-64 + 0.5 * np.arange(n)).astype(np.float32), col_chunks=2)


@pytest.mark.parametrize("exclude_self, upper_only", [(True, False), (False, True), (True, True)])
def test_exact_flags(exclude_self, upper_only):
    _check_exact(_ints(131, 12, 17), 40, col_bias=_halves(131, 18), exclude_self=exclude_self, upper_only=upper_only, col_chunks=2)


def test_exact_exclusion_patterns():
    n = 131
    rng = np.random.default_rng(21)
    pairs = [(int(r), int(c)) for r, c in rng.integers(0, n, size=(900, 2))]
    pairs = [p for p in pairs if p[0] not in (5, 6, 7)]                  # row 5: empty
    pairs += [(6, c) for c in range(n)]                                  # row 6: every candidate excluded
    pairs += [(7, c) for c in range(32, 64)]                             # row 7: a whole column tile excluded
    E = _ints(n, 9, 22)
    for chunks in (1, 3):
        s, i = _check_exact(E, 50, col_bias=_halves(n, 23), pairs=pairs, col_chunks=chunks)
        assert int(i[6].max()) == -1 and bool(torch.isinf(s[6]).all())
    _check_exact(E, 128, pairs=pairs, exclude_self=True, upper_only=True, col_chunks=2)


def test_real_valued_scores_within_the_chain_bound_and_nothing_better_left_out():
    """B(i, j) = (d + 2) 2^-24 (Σ_t |E[q, t] E[j, t]| + |col_bias[j]| + |row_bias[i]|) bounds the rounding of d fused multiply-adds
    and two adds in any order.  Every returned score lies within B of the float64 score of its index; no admissible column that was
    left out beats the returned k-th one by more than their two B; every row is in the total order."""
    from ctgcn_amd import ops
    n, d, k = 1000, 128, 50
    g = torch.Generator().manual_seed(7)
    E, rb, cb = torch.randn(n, d, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    score, index = ops.topk_scores(E.to(DEV), k, row_bias=rb.to(DEV), col_bias=cb.to(DEV), exclude_self=True)
    score, index = score.cpu().numpy(), index.cpu().numpy().astype(np.int64)
    S = R.scores(E.numpy(), None, rb.numpy(), cb.numpy())
    B = (d + 2) * 2.0 ** -24 * R.abs_scores(E.numpy(), None, rb.numpy(), cb.numpy())
    assert (index >= 0).all() and all(len(set(r)) == k for r in index) and (index != np.arange(n)[:, None]).all()
    ri = np.arange(n)[:, None]
    err = np.abs(score.astype(np.float64) - S[ri, index])
    print("  worst |score - fp64| / B = %.3f" % float((err / B[ri, index]).max()))
    assert (err <= B[ri, index]).all()
    ds, di = np.diff(score, axis=1), np.diff(index, axis=1)
    assert (ds <= 0).all() and (di[ds == 0] > 0).all()
    left = np.ones((n, n), dtype=bool)
    left[ri, index] = False
    left[np.arange(n), np.arange(n)] = False
    last = index[:, -1]
    slack = S[np.arange(n), last][:, None] + B[np.arange(n), last][:, None] + B
    assert not (left & (S > slack)).any()


def test_refusals_before_any_launch():
    from ctgcn_amd import _lib, ops
    E = torch.zeros(40, 8, device=DEV)
    with pytest.raises(ValueError):
        ops.topk_scores(E, 0)
    with pytest.raises(ValueError, match="ctgcn_topk_max_k"):
        ops.topk_scores(E, ops.topk_max_k() + 1)
    with pytest.raises(ValueError, match="ctgcn_topk_max_d"):
        ops.topk_scores(torch.zeros(4, ops.topk_max_d() + 1, device=DEV), 2)
    with pytest.raises(_lib.CtgcnHipError):
        ops.topk_scores(E.cpu(), 2)
    with pytest.raises(TypeError):
        ops.topk_scores(E.double(), 2)
    with pytest.raises(ValueError):
        ops.topk_scores(E, 2, col_bias=torch.zeros(39, device=DEV))
    with pytest.raises(ValueError):
        ops.topk_scores(E, 2, rows=torch.arange(5, device=DEV), row_bias=torch.zeros(40, device=DEV))
    t = lambda a: torch.tensor(a, dtype=torch.int32, device=DEV)
    unsorted = ops.GcnAdj(t([0, 2] + [2] * 39), t([5, 3]), torch.ones(2, device=DEV))
    with pytest.raises(ValueError, match="ascend"):
        ops.topk_scores(E, 2, exclude=unsorted)
    # the C entry refuses the same limits itself
    lib = _lib.load()
    assert lib.ctgcn_topk_max_k() >= 128 and lib.ctgcn_topk_max_d() >= 512
    out_s, out_i = torch.empty(40, 200, device=DEV), torch.empty(40, 200, dtype=torch.int32, device=DEV)
    args = lambda d, k, chunks: (40, 40, d, k, E.data_ptr(), 8, None, None, None, None, None, 0, chunks, out_s.data_ptr(), out_i.data_ptr(),
                                 None, 0, None)
    assert lib.ctgcn_topk_scores_f32(*args(8, 0, 1)) == -1
    assert lib.ctgcn_topk_scores_f32(*args(8, lib.ctgcn_topk_max_k() + 1, 1)) == -4
    assert lib.ctgcn_topk_scores_f32(*args(lib.ctgcn_topk_max_d() + 1, 4, 1)) == -4
    assert lib.ctgcn_topk_scores_f32(*args(8, 4, 0)) == -1
    assert lib.ctgcn_topk_scores_f32(*args(8, 4, 2)) == -3          # two chunks need a workspace
    assert b"topk_scores" in lib.ctgcn_last_error()


def test_no_dense_matrix_at_20000_nodes():
    from ctgcn_amd import ops
    n, k = 20000, 100
    E = torch.from_numpy(_ints(n, 16, 31)).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    score, index = ops.topk_scores(E, k, exclude_self=True)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base - score.numel() * 4 - index.numel() * 4
    print("  peak above inputs and outputs: %.1f MiB (n^2 bytes = %.1f MiB)" % (extra / 2 ** 20, n * n / 2 ** 20))
    assert extra < n * n
    # spot check against the model on a few rows
    rows = np.array([0, 1, 9999, 19999])
    ref_s, ref_i = R.topk(E.cpu().numpy(), k, rows, exclude_self=True)
    assert np.array_equal(index.cpu().numpy()[rows], ref_i) and np.array_equal(score.cpu().numpy()[rows].astype(np.float64), ref_s)


def test_offsets_past_2_31_elements():
    """n * lde above 2^31 elements: a strided view of an 8.6 GB buffer whose pages outside the rows are never touched"""
    from ctgcn_amd import ops
    n, d, k = 4100, 16, 8
    lde = (1 << 19) + 4
    assert n * lde > 2 ** 31
    need = 4 * n * lde
    if torch.cuda.get_device_properties(0).total_memory < 2 * need:
        pytest.skip("the strided view needs a device with at least %.0f GiB" % (2 * need / 2 ** 30))
    buf = torch.empty(n * lde, dtype=torch.float32, device=DEV)
    view = buf.as_strided((n, d), (lde, 1))
    E = _ints(n, d, 41)
    view.copy_(torch.from_numpy(E).to(DEV))
    rows = np.array([0, 1, 4095, 4096, 4099], dtype=np.int64)
    score, index = ops.topk_scores(view, k, rows=torch.from_numpy(rows).to(DEV), exclude_self=True, col_chunks=3)
    ref_s, ref_i = R.topk(E, k, rows, exclude_self=True)
    assert np.array_equal(index.cpu().numpy(), ref_i) and np.array_equal(score.cpu().numpy().astype(np.float64), ref_s)
    del view, buf
    torch.cuda.empty_cache()
