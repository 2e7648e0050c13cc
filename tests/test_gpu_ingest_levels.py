"""ops.edge_levels and ops.slot_reorder on synthetic inputs against the numpy models of tests/_kcore_ref.py, and the whole device
ingest (CoreAdj.from_graph) against the matrix route on a graph with known core numbers.

edge_level_kernel takes any `core` array, so no peel is needed to reach its branches: the block's LDS histogram (hist_len <= EL_HIST =
2 048) | global atomics (2 049, 3 001), the clamp min(level, hist_len - 1) (1, 5, 2 048 with cores up to 3 000), the second lap of the
grid-stride loop (4 096 blocks x 16 rows: n = 65 536 + 17), 16 lanes a row (lengths 0, 1, 15, 16, 17, 300), null histograms.
Integer-valued weights make every partial sum an exact fp64 integer, so wsum must be EQUAL in any atomic order; with random weights it
may differ from the extended-precision sum by count[b] * 2^-53 * sum|w| per bin: count[b] - 1 roundings of partial sums that never
exceed sum|w| in magnitude, the worst case of any summation order.  Nothing is measured.

slot_reorder_kernel keeps a row of up to 64 entries in registers (lengths 0, 1, 63, 64) and walks longer ones once per slot (65, 128,
129, 300), four rows a block (n = 1, 3, 4, 5, 1 000), K up to CTGCN_MAX_SLOTS = 255, levels past the table clamped to its last entry.
Equal slots inside a row carry distinct values, so an unstable partition shows.  No entry here maps to a slot >= K: from_graph cannot
produce one (slot_table gives such levels a slot only when their count is zero), and the two paths differ on them — the register path
writes them, the per-slot loop skips them and leaves the tail of the row unwritten.  The kernel is left as it is."""
import functools

import numpy as np
import pytest
import torch

import _kcore_ref as R

pytestmark = pytest.mark.gpu

E_INVALID = -1


def _dev():
    return torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(_dev())


# ------------------------------------------------------------------------------------------ edge levels
EL_LENGTHS = [0, 1, 15, 16, 17, 300]
EL_N = [1, 15, 16, 17, 1000, 65536 + 17]
EL_HIST_LEN = [1, 5, 2048, 2049, 3001]


@functools.lru_cache(maxsize=None)
def _el_case(n):
    rng = np.random.default_rng(7000 + n)
    ln = rng.choice(EL_LENGTHS, n, p=[.15, .2, .2, .2, .2, .05])
    ln[:min(n, 6)] = EL_LENGTHS[::-1][:n]                       # every length occurs (n = 1: the 300-entry row)
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    rows = np.repeat(np.arange(n), ln)
    col = rng.integers(0, n, len(rows))
    col = col[np.lexsort((col, rows))].astype(np.int32)         # sorted inside each row
    core = rng.integers(1, 3001, n).astype(np.int32)
    core[:min(n, 2)] = [3000, 1][:n]
    w_int = rng.integers(-8, 9, len(rows)).astype(np.float32)
    w_rnd = rng.standard_normal(len(rows)).astype(np.float32)
    host = dict(indptr=indptr, col=col, core=core, w_int=w_int, w_rnd=w_rnd)
    return host, {k: _t(v) for k, v in host.items()}


@functools.lru_cache(maxsize=None)
def _el_ref(n, hist_len, weights):
    h = _el_case(n)[0]
    w = {"w_int": h["w_int"], "w_rnd": h["w_rnd"], "abs": np.abs(h["w_rnd"])}[weights]
    return R.edge_levels_ref(h["indptr"], h["col"], w, h["core"], hist_len)


@pytest.mark.parametrize("hist_len", EL_HIST_LEN)
@pytest.mark.parametrize("n", EL_N)
def test_edge_levels_match_the_model(n, hist_len):
    from ctgcn_amd import ops
    h, d = _el_case(n)
    want_level, want_count, want_sum = _el_ref(n, hist_len, "w_int")
    assert want_count.sum() == len(h["col"]) and (hist_len > 5 or n < 15 or want_count[-1] > len(h["col"]) // 2)
    level, count, wsum = ops.edge_levels(d["indptr"], d["col"], d["w_int"], d["core"], hist_len)
    assert level.dtype == torch.int32 and count.dtype == torch.int64 and wsum.dtype == torch.float64
    assert np.array_equal(level.cpu().numpy(), want_level)
    assert np.array_equal(count.cpu().numpy(), want_count)
    assert np.array_equal(wsum.cpu().numpy(), want_sum.astype(np.float64))              # integers below 2^53: exact in any order
    # random weights: the summation-order bound
    _, _, ref = _el_ref(n, hist_len, "w_rnd")
    _, _, sum_abs = _el_ref(n, hist_len, "abs")
    level, count, wsum = ops.edge_levels(d["indptr"], d["col"], d["w_rnd"], d["core"], hist_len)
    assert np.array_equal(level.cpu().numpy(), want_level) and np.array_equal(count.cpu().numpy(), want_count)
    err = np.abs(wsum.cpu().numpy().astype(np.longdouble) - ref)
    bound = want_count.astype(np.longdouble) * np.longdouble(2.0) ** -53 * sum_abs
    worst = int(np.argmax(err - bound))
    print("  n=%d hist_len=%d: max wsum error %.3e, at bin %d %.3e of bound %.3e" % (n, hist_len, float(err.max()), worst, float(err[worst]),
                                                                                     float(bound[worst])))
    assert (err <= bound).all(), (worst, float(err[worst]), float(bound[worst]))


@pytest.mark.parametrize("hist_len", [7, 2049])
def test_edge_levels_weights_that_cancel_give_exact_zero(hist_len):
    """slot_table tests wsum[k] with ==: entries of one level whose weights cancel must leave exactly 0.0 beside a non-zero count"""
    from ctgcn_amd import ops
    # rows 0 - 1 at level 2 with weights +3 | -3 (and +0.5 | -0.5 in a second block of rows), rows 40 - 41 at level 5
    n = 42
    core = np.full(n, 6, dtype=np.int32)
    core[[0, 1, 20, 21]] = 2
    core[[40, 41]] = 5
    pairs = [(0, 1, 3.0), (1, 0, -3.0), (20, 21, 0.5), (21, 20, -0.5), (40, 41, 2.0), (41, 40, 2.0)]
    indptr = np.zeros(n + 1, dtype=np.int32)
    for r, _, _ in pairs:
        indptr[r + 1:] += 1
    col = np.array([c for _, c, _ in pairs], dtype=np.int32)
    val = np.array([w for _, _, w in pairs], dtype=np.float32)
    level, count, wsum = ops.edge_levels(_t(indptr), _t(col), _t(val), _t(core), hist_len)
    want_level, want_count, want_sum = R.edge_levels_ref(indptr, col, val, core, hist_len)
    assert want_count[2] == 4 and want_sum[2] == 0 and want_count[5] == 2 and want_sum[5] == 4
    assert np.array_equal(level.cpu().numpy(), want_level) and np.array_equal(count.cpu().numpy(), want_count)
    got = wsum.cpu().numpy()
    assert got[2] == 0.0 and np.array_equal(got, want_sum.astype(np.float64))


@pytest.mark.parametrize("hist_len", [2048, 2049])
@pytest.mark.parametrize("give", ["count", "wsum", "neither"])
def test_edge_levels_null_histograms(give, hist_len):
    """through the C ABI: a null histogram is skipped, the level array is still complete, and what is given accumulates"""
    from ctgcn_amd import _lib
    from ctgcn_amd._lib import ptr
    lib = _lib.load()
    n = 1000
    h, d = _el_case(n)
    want_level, want_count, want_sum = _el_ref(n, hist_len, "w_int")
    level = torch.full((len(h["col"]),), -7, dtype=torch.int32, device=_dev())
    count = torch.full((hist_len,), 11, dtype=torch.int64, device=_dev())
    wsum = torch.full((hist_len,), 0.5, dtype=torch.float64, device=_dev())
    rc = lib.ctgcn_edge_levels_i32(n, ptr(d["indptr"]), ptr(d["col"]), ptr(d["w_int"]), ptr(d["core"]), ptr(level),
                                   ptr(count) if give == "count" else None, ptr(wsum) if give == "wsum" else None, hist_len, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(level.cpu().numpy(), want_level)
    assert np.array_equal(count.cpu().numpy(), 11 + (want_count if give == "count" else np.zeros(hist_len, dtype=np.int64)))
    assert np.array_equal(wsum.cpu().numpy(), 0.5 + (want_sum.astype(np.float64) if give == "wsum" else np.zeros(hist_len)))


def test_edge_levels_count_only_needs_no_weights_and_wsum_needs_them():
    from ctgcn_amd import _lib
    from ctgcn_amd._lib import ptr
    lib = _lib.load()
    n, hist_len = 17, 5
    h, d = _el_case(n)
    want_level, want_count, _ = _el_ref(n, hist_len, "w_int")
    level = torch.full((len(h["col"]),), -7, dtype=torch.int32, device=_dev())
    count = torch.zeros(hist_len, dtype=torch.int64, device=_dev())
    wsum = torch.full((hist_len,), 0.5, dtype=torch.float64, device=_dev())
    rc = lib.ctgcn_edge_levels_i32(n, ptr(d["indptr"]), ptr(d["col"]), None, ptr(d["core"]), ptr(level), ptr(count), ptr(wsum), hist_len, None)
    torch.cuda.synchronize()
    assert rc == E_INVALID and b"val required" in lib.ctgcn_last_error()
    assert bool((level == -7).all()) and not bool(count.any()) and bool((wsum == 0.5).all())        # nothing was launched
    rc = lib.ctgcn_edge_levels_i32(n, ptr(d["indptr"]), ptr(d["col"]), None, ptr(d["core"]), ptr(level), ptr(count), None, hist_len, None)
    torch.cuda.synchronize()
    assert rc == 0
    assert np.array_equal(level.cpu().numpy(), want_level) and np.array_equal(count.cpu().numpy(), want_count)


# ------------------------------------------------------------------------------------------ slot reorder
SR_LENGTHS = [65, 64, 300, 63, 129, 128, 1, 0]
SR_TABLE_LEN, SR_MAX_LEVEL = 300, 400


@functools.lru_cache(maxsize=None)
def _sr_case(n):
    rng = np.random.default_rng(9000 + n)
    ln = rng.choice(SR_LENGTHS, n)
    ln[:min(n, 8)] = SR_LENGTHS[:n]                             # n = 1: a 65-entry row, n = 3: 65, 64, 300, ...
    indptr = np.concatenate([[0], np.cumsum(ln)]).astype(np.int32)
    nnz = int(indptr[-1])
    col = rng.integers(0, 1 << 20, nnz).astype(np.int32)
    val = (rng.permutation(nnz) - nnz // 2).astype(np.float32) * np.float32(0.25)       # distinct: tells equal-slot entries apart
    level = rng.integers(0, SR_MAX_LEVEL + 1, nnz).astype(np.int32)                    # a quarter lies past the table
    return indptr, col, val, level


@pytest.mark.parametrize("K", [1, 2, 7, 255])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 1000])
def test_slot_reorder_matches_the_model(n, K):
    from ctgcn_amd import ops
    indptr, col, val, level = _sr_case(n)
    assert len(set(val.tolist())) == len(val) and level.max() > SR_TABLE_LEN
    rng = np.random.default_rng(K)
    table = rng.integers(0, K, SR_TABLE_LEN).astype(np.uint8)
    table[-1] = K // 2                                          # the clamp decides: every level >= 299 lands in the middle slot
    table[:2] = [K - 1, 0]
    want = R.slot_reorder_ref(indptr, col, val, level, table)
    assert int(want[2].max()) < K
    got = ops.slot_reorder(_t(indptr), _t(col), _t(val), _t(level), _t(table), K)
    assert got[0].dtype == torch.int32 and got[1].dtype == torch.float32 and got[2].dtype == torch.uint8
    assert torch.equal(got[2].cpu(), torch.from_numpy(want[2]))
    assert torch.equal(got[0].cpu(), torch.from_numpy(want[0]))
    assert torch.equal(got[1].cpu(), torch.from_numpy(want[1]))
    assert torch.equal(got[1].cpu().view(torch.int32), torch.from_numpy(want[1]).view(torch.int32))


def test_slot_reorder_rejects_outputs_that_alias_inputs():
    from ctgcn_amd import _lib
    from ctgcn_amd._lib import ptr
    lib = _lib.load()
    indptr, col, val, level = (_t(a) for a in _sr_case(5))
    table = torch.zeros(SR_TABLE_LEN, dtype=torch.uint8, device=_dev())
    col0, val0 = col.clone(), val.clone()
    col2, val2 = torch.empty_like(col), torch.empty_like(val)
    slot2 = torch.full((col.numel(),), 9, dtype=torch.uint8, device=_dev())
    for co, vo in ((col, val2), (col2, val), (col, val)):
        rc = lib.ctgcn_slot_reorder(5, 1, ptr(indptr), ptr(col), ptr(val), ptr(level), ptr(table), SR_TABLE_LEN, ptr(co), ptr(vo), ptr(slot2), None)
        torch.cuda.synchronize()
        assert rc == E_INVALID and b"alias" in lib.ctgcn_last_error()
    assert torch.equal(col, col0) and torch.equal(val, val0) and bool((slot2 == 9).all())           # nothing was launched


# ------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("max_core", [-1, 16, 17, 45])
def test_ingest_of_the_caps_graph_equals_the_matrix_route(max_core):
    """kcore (peel at 16, capped sweeps at 17 and 45, sweeps at -1) -> edge_levels -> slot_table -> slot_reorder on the graph of the
    cap tests: cores 1, 20 and 39 only (levels 2..19 and 21..38 are empty and get no slot), rows of 1 030 and 39 entries"""
    from ctgcn_amd import CoreAdj
    from ctgcn_amd.helper import core_adj_from_scipy
    from oracle import oracle as O
    structure, want_core = R.caps_graph()
    csr = R.with_weights(structure)
    adj, core, files = core_adj_from_scipy(csr, max_core, _dev())
    assert files == (39 if max_core < 0 else min(39, max_core))
    assert np.array_equal(core.cpu().numpy(), want_core if max_core < 0 else np.minimum(want_core, max_core))
    mats = O.kcore_matrices(csr, core=want_core)
    assert len(mats) == 39
    ref = CoreAdj.from_matrices(O.core_adj_list([mats], 0, 1, 1, max_core=max_core)[0], device="cpu")
    assert ref.K == {-1: 3, 16: 2, 17: 2, 45: 3}[max_core]
    assert (adj.K, adj.nested, adj.self_loop, adj.symmetric) == (ref.K, True, True, True)
    assert adj.nnz_per_slot == ref.nnz_per_slot
    for a, b in ((adj.row_ptr, ref.row_ptr), (adj.col, ref.col), (adj.val, ref.val), (adj.slot, ref.slot)):
        assert torch.equal(a.cpu(), b)
