"""Gathered-row bias of the forward aggregation kernels (ctgcn_core_aggregate_bias_f32 / ctgcn_core_aggregate_split_bias_f32):
aggregate(Wt, gather_bias=b) against aggregate(Wt + b) on the materialised matrix, torch.equal — fp32 rows, both fp16 planes and the row
scales — at the smallest shapes that reach each kernel: the d = 128 two-rows-per-wave kernels, the one-wave-per-row kernels (d = 256), the
two-chunks-per-lane / multi-pass ones (d = 500), scalar lanes (d = 30), wide step masks (K = 33), hub rows and hub rows cut into pieces."""
import ctypes

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda:0")


def _hub_split_entries():
    from ctgcn_amd import _lib
    return int(_lib.load().ctgcn_hub_split_entries())


def _adj(n, K, nested, self_loop, seed, hub=0):
    """K matrices over n nodes from tagged random entries (nested: an entry tagged s is in A_s .. A_{K-1}; else in A_s alone); every
    fifth row has no entry at all; hub > 0: row 0 holds `hub` entries (distinct columns, every tag)"""
    from ctgcn_amd import CoreAdj
    rng = np.random.default_rng(seed)
    m = 6 * n
    rows, cols = rng.integers(0, n, m), rng.integers(0, n, m)
    keep = (rows != cols) & (rows % 5 != 3) & (rows != 0 if hub else np.ones(m, bool))
    rows, cols = rows[keep], cols[keep]
    if hub:
        assert hub < n
        rows = np.concatenate([np.zeros(hub, np.int64), rows])
        cols = np.concatenate([1 + rng.permutation(n - 1)[:hub], cols])
    key, first = np.unique(rows * n + cols, return_index=True)
    rows, cols = rows[first], cols[first]
    vals = (rng.integers(1, 9, len(rows)) * 0.25).astype(np.float32)
    tags = rng.integers(0, K, len(rows))
    mats = []
    for j in range(K):
        sel = (tags <= j) if nested else (tags == j)
        mats.append(sp.csr_matrix((vals[sel], (rows[sel], cols[sel])), shape=(n, n)))
    adj = CoreAdj.from_matrices(mats, self_loop=self_loop, device=_dev())
    assert adj.nested == nested and adj.self_loop == self_loop and adj.K == K
    assert int((adj.row_ptr[1:] - adj.row_ptr[:-1]).min()) == 0          # rows of degree 0
    return adj


def _operands(n, d, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    wt = (torch.randn(n, d, generator=g) * torch.rand(n, 1, generator=g).mul(3).exp()).to(_dev())
    b = torch.randn(d, generator=g).to(_dev())
    return wt, b


def _planes(adj, x, plan, n_out, bias):
    """the whole workspace (plane 1 | plane 2 | row scales | ...), zero-filled first: the rows a plan skips are never written"""
    from ctgcn_amd import _lib, ops
    lr = adj.long_rows()
    nbytes = int(_lib.load().ctgcn_core_aggregate_split_workspace_bytes(adj.n, x.shape[1], adj.K, n_out, 0 if lr is None else lr.numel()))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=x.device)
    ops.aggregate_split_planes(x, adj, n_out, plan, ws=ws, gather_bias=bias)
    return ws


def _check(adj, d, seed, relu_off=True):
    from ctgcn_amd import ops
    wt, b = _operands(adj.n, d, seed)
    ref_x = wt + b                                         # what ctgcn_transpose_bias_f32 writes: one fp32 add per element
    for relu in ((True, False) if relu_off else (True,)):
        want = ops._aggregate_fwd(adj, ref_x, relu)
        got = ops._aggregate_fwd(adj, wt, relu, b)
        assert torch.isfinite(want).all() and float(want.abs().max()) > 0
        assert torch.equal(got, want), "fp32 rows differ (relu=%s)" % relu
    if d % 4 or d < 32 or d > 512:
        return
    n_out, tile = (1, adj.PLAN_TILE) if d == 128 else (384, adj.PLAN_TILE_GEMM)
    kp = -(-d // 64) * 64
    for plan in (None, adj.row_plan(tile)):
        want, got = _planes(adj, ref_x, plan, n_out, None), _planes(adj, wt, plan, n_out, b)
        rows = adj.n * adj.K if (plan is None or d == 128) else plan["operand_rows"]
        p1, p2, sc = rows * kp * 2, 2 * rows * kp * 2, 2 * rows * kp * 2 + rows * 4
        assert int(want[:p1].count_nonzero()) > 0 and int(want[p2:sc].count_nonzero()) > 0
        what = "with" if plan is not None else "without"
        assert torch.equal(got[:p1], want[:p1]), "plane 1 differs %s the row plan" % what
        assert torch.equal(got[p1:p2], want[p1:p2]), "plane 2 differs %s the row plan" % what
        assert torch.equal(got[p2:sc], want[p2:sc]), "row scales differ %s the row plan" % what
        assert torch.equal(got, want)


SHAPES = {
    "n37_d128_K3": dict(n=37, d=128, K=3),       # not a multiple of 16 rows; two rows per wave
    "n33_d500_K3": dict(n=33, d=500, K=3),       # generic kernel in two passes; split kernel with two chunks per lane
    "n37_d64_K3": dict(n=37, d=64, K=3),
    "n37_d256_K2": dict(n=37, d=256, K=2),       # one wave per row, one chunk per lane
    "n37_d30_K3": dict(n=37, d=30, K=3),         # d % 4 != 0: scalar lanes (fp32 rows only)
    "n37_d20_K1": dict(n=37, d=20, K=1),         # eight lanes per row, a single matrix
    "n70_d128_K33": dict(n=70, d=128, K=33),     # wide step masks: two words per tile
    "n70_d256_K33": dict(n=70, d=256, K=33),
    "n70_d500_K33": dict(n=70, d=500, K=33),
}


@pytest.mark.parametrize("self_loop", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("nested", [True, False], ids=["nested", "list"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_gathered_bias_equals_the_materialised_operand(shape, nested, self_loop):
    s = SHAPES[shape]
    nested = nested or s["K"] == 1                   # a single matrix is a nested list
    adj = _adj(s["n"], s["K"], nested, self_loop, seed=len(shape) + 2 * nested + self_loop)
    assert adj.long_rows() is None
    _check(adj, s["d"], seed=7)


@pytest.mark.parametrize("self_loop", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("nested", [True, False], ids=["nested", "list"])
@pytest.mark.parametrize("d", [128, 500, 30])
def test_gathered_bias_on_a_hub_row(d, nested, self_loop):
    """one row of CoreAdj.LONG_ROW + 1 entries: the block-per-row kernel (row 0 is its own self-loop row, too)"""
    from ctgcn_amd import CoreAdj
    adj = _adj(CoreAdj.LONG_ROW + 40, 3, nested, self_loop, seed=d, hub=CoreAdj.LONG_ROW + 1)
    assert adj.long_rows().tolist() == [0] and adj.hub_split() == 1
    assert int(adj.row_ptr[1]) == CoreAdj.LONG_ROW + 1
    _check(adj, d, seed=11, relu_off=False)


@pytest.mark.parametrize("self_loop", [True, False], ids=["self", "noself"])
@pytest.mark.parametrize("nested", [True, False], ids=["nested", "list"])
@pytest.mark.parametrize("d", [128, 500])
def test_gathered_bias_on_a_hub_row_cut_into_pieces(d, nested, self_loop):
    """one row of ctgcn_hub_split_entries() + 1 entries (the library's constant, read from it): two blocks leave partial sums, the
    second pass adds the row's own row + bias"""
    entries = _hub_split_entries() + 1
    adj = _adj(entries + 40, 3, nested, self_loop, seed=d + 1, hub=entries)
    assert adj.long_rows().tolist() == [0] and adj.hub_split() == 2
    _check(adj, d, seed=13, relu_off=False)


def _call(lib, name, adj, x, bias, H):
    """the C entry point itself: `name` with the dense operand x (and, for the bias entry, the bias pointer, NULL allowed)"""
    from ctgcn_amd import _lib
    p = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
    n, d = x.shape
    head = (n, d, adj.K, p(adj.row_ptr), p(adj.col), p(adj.val), p(adj.slot), p(x))
    mid = (p(bias),) if name.endswith("_bias_f32") else (d,)
    rc = getattr(lib, name)(*head, *mid, p(H), adj.flags | _lib.F_RELU, None, 0, 0, 1, None, 0, None)
    torch.cuda.synchronize()
    assert rc == 0, lib.ctgcn_last_error().decode()


@pytest.mark.parametrize("d", [128, 500, 30])
def test_a_null_bias_is_the_call_without_one(d):
    from ctgcn_amd import _lib
    lib = _lib.load()
    adj = _adj(37, 3, True, True, seed=5)
    wt, _ = _operands(37, d, 3)
    want, got = torch.zeros(37, 3, d, device=_dev()), torch.zeros(37, 3, d, device=_dev())
    _call(lib, "ctgcn_core_aggregate_f32", adj, wt, None, want)
    _call(lib, "ctgcn_core_aggregate_bias_f32", adj, wt, None, got)
    assert float(want.abs().max()) > 0 and torch.equal(got, want)
    if d % 4 == 0:
        from ctgcn_amd import ops
        assert torch.equal(_planes(adj, wt, None, 1 if d == 128 else 384, None), _planes(adj, wt, None, 1 if d == 128 else 384, torch.zeros(d, device=_dev())))
        assert torch.equal(ops._aggregate_fwd(adj, wt, True), want)


def test_the_bias_entry_points_refuse_what_they_cannot_read():
    from ctgcn_amd import ops
    adj = _adj(37, 3, True, True, seed=5)
    wt, b = _operands(37, 128, 3)
    wide = torch.zeros(37, 256, device=_dev())[:, :128]
    with pytest.raises(ValueError, match="dense"):
        ops._aggregate_fwd(adj, wide, True, b)
    with pytest.raises(ValueError, match="gather_bias"):
        ops._aggregate_fwd(adj, wt, True, b[:64])
    with pytest.raises(ValueError, match="gather_bias"):
        ops.aggregate_split_planes(wt, adj, 1, None, gather_bias=b.double())
