"""ops.pgnn_conv (ctgcn_pgnn.hip) against a float64 mirror in the reference's materialising form and its autograd: the forward and the
gradients of PS, the table, w_p and b_p, for position output alone, structure output alone and both; a table with zero and negative
entries; every node choosing one node (a single pull list of N A items, cut into pieces) and a permutation (lists of one item); the
L2-normalised position output; the dropout epilogue against the mirror fed the mask that the host model of the draw gives for the
key; forward + backward twice, bit-identical; and the memory bound of the fused path.

Shapes (N, A, out): each of N in {1, 63, 257}, A in {1, 5, 100} and out in {1, 32, 33, 128, 500} at least once (every lane layout of the
kernels: 8, 16 .. 64 lanes across the channels and 2, 4, 8 channels per lane; N below, at and above a block's rows), and UCI's
(1899, 100, 32).

Tolerance per tensor (the project's rule): the largest error over the tensor's largest magnitude may reach the larger of 4 x the
mirror's own float32-vs-float64 error and a floor of 2e-6 (outputs) or 1e-5 (gradients).  A gradient the mirror has as exactly zero
must be exactly zero."""
import numpy as np
import pytest
import torch

import _gcrn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(1, 1, 1), (63, 5, 32), (257, 100, 33), (63, 1, 128), (257, 5, 500), (63, 100, 8), (257, 5, 200), (1899, 100, 32)]
VALUES = np.asarray([0.0, 0.125, 1.0 / 3.0, 0.5, 1.0], dtype=np.float32)          # ascending, as torch.unique orders them
TABLE = np.asarray([-0.7, 0.0, 0.4, -0.2, 1.3], dtype=np.float32)                # zero and negative entries


def share(what, got, ref, yard, floor):
    got, ref = got.detach().double().cpu().reshape(-1), ref.detach().double().cpu().reshape(-1)
    top = float(ref.abs().max()) if ref.numel() else 0.0
    if top == 0.0:
        print("  [tol] %-46s the mirror is exactly zero; largest |got| %.3e" % (what, float(got.abs().max()) if got.numel() else 0.0))
        return 0.0 if not bool(got.any()) else float("inf")
    err = float((got - ref).abs().max()) / top
    used = err / max(4 * yard, floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (what, err, used, yard, floor))
    return used


def inputs(n, A, d, kind="random"):
    rng = np.random.default_rng(n * 1000 + A * 10 + d)
    U = min(len(VALUES), n * A)
    lvl = rng.integers(0, U, (n, A))
    lvl.reshape(-1)[:U] = np.arange(U)                            # every value occurs: the table has U entries
    if kind == "equal":
        idx = np.full((n, A), n // 2, dtype=np.int64)
    elif kind == "permutation":
        idx = np.stack([rng.permutation(n) for _ in range(A)], axis=1)
    else:
        idx = rng.integers(0, n, (n, A))
        idx[rng.random((n, A)) < 0.4] = 0                          # a long list beside short ones
    return dict(PS=rng.standard_normal((n, 2 * d)).astype(np.float32), dm=VALUES[lvl], lvl=lvl, idx=idx.astype(np.int64),
                table=TABLE[:U].copy(), w=(rng.standard_normal(d) / np.sqrt(d)).astype(np.float32), b=np.asarray([0.3], dtype=np.float32),
                cp=rng.standard_normal((n, A)).astype(np.float32), cs=rng.standard_normal((n, d)).astype(np.float32))


def mirror(v, dtype, need_pos, need_struct, norm, keep=None, p=0.0):
    """(pos, struct, gradients by name) in the materialising form: [n, A, out] exists"""
    t = {k: torch.from_numpy(v[k]).to(dtype).requires_grad_(True) for k in ("PS", "table", "w", "b")}
    d = v["PS"].shape[1] // 2
    dprime = t["table"][torch.from_numpy(v["lvl"])]
    m = torch.relu(dprime.unsqueeze(-1) * t["PS"][:, :d][torch.from_numpy(v["idx"])] + t["PS"][:, None, d:])
    pos = strct = None
    loss = 0
    if need_pos:
        pos = m.matmul(t["w"]) + t["b"]
        if norm:
            pos = torch.nn.functional.normalize(pos, p=2, dim=-1)
        loss = loss + (pos * torch.from_numpy(v["cp"]).to(dtype)).sum()
    if need_struct:
        strct = m.mean(dim=1)
        if keep is not None:
            strct = strct * torch.from_numpy(keep).to(dtype) / (1.0 - p)
        loss = loss + (strct * torch.from_numpy(v["cs"]).to(dtype)).sum()
    loss.backward()
    return pos, strct, {k: (None if x.grad is None else x.grad) for k, x in t.items()}


def fused(v, need_pos, need_struct, norm, p=0.0, key=0, piece=None, table=True):
    from ctgcn_amd import ops
    t = {k: torch.from_numpy(v[k]).to(DEV).requires_grad_(True) for k in ("PS", "table", "w", "b")}
    dm, da = torch.from_numpy(v["dm"]).to(DEV), torch.from_numpy(v["idx"]).to(DEV)
    pos, strct = ops.pgnn_conv(t["PS"], dm, da, t["w"], t["b"], table=t["table"] if table else None, need_pos=need_pos, need_struct=need_struct,
                               epi=ops.PGNN_EPI_NORM if norm else ops.PGNN_EPI_NONE, p=p, key=key, piece=piece)
    loss = 0
    if need_pos:
        loss = loss + (pos * torch.from_numpy(v["cp"]).to(DEV)).sum()
    if need_struct:
        loss = loss + (strct * torch.from_numpy(v["cs"]).to(DEV)).sum()
    loss.backward()
    return pos, strct, {k: (None if x.grad is None else x.grad) for k, x in t.items()}


def compare(what, v, need_pos, need_struct, norm, keep=None, p=0.0, key=0, piece=None, table=True):
    pos64, st64, g64 = mirror(v, torch.float64, need_pos, need_struct, norm, keep, p)
    pos32, st32, g32 = mirror(v, torch.float32, need_pos, need_struct, norm, keep, p)
    pos, st, g = fused(v, need_pos, need_struct, norm, p, key, piece, table)
    pos2, st2, g2 = fused(v, need_pos, need_struct, norm, p, key, piece, table)

    def yard(a32, a64):
        top = float(a64.detach().abs().max()) if a64.numel() else 0.0
        return float((a32.detach().double() - a64.detach()).abs().max()) / top if top else 0.0

    used = {}
    assert (pos is None) == (not need_pos) and (st is None) == (not need_struct)
    if need_pos:
        assert torch.equal(pos, pos2)
        used["pos"] = share(what + " pos", pos, pos64, yard(pos32, pos64), 2e-6)
    if need_struct:
        assert torch.equal(st, st2)
        used["struct"] = share(what + " struct", st, st64, yard(st32, st64), 2e-6)
    for k in g64:
        if g64[k] is None or (not need_pos and k in ("w", "b")) or (not table and k == "table"):
            assert g[k] is None, k                                  # no position output: nothing reaches w_p and b_p, not even zeros
            continue
        assert torch.equal(g[k], g2[k]), k
        used["grad " + k] = share(what + " grad " + k, g[k], g64[k], yard(g32[k], g64[k]), 1e-5)
    over = {k: round(u, 3) for k, u in used.items() if not u <= 1.0}
    assert not over, "%s: share of the tolerance used %s" % (what, over)


@pytest.mark.parametrize("outputs", ["pos", "struct", "both"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_forward_and_gradients_match_the_float64_mirror(shape, outputs):
    n, A, d = shape
    v = inputs(n, A, d)
    compare("%s %s" % (shape, outputs), v, outputs != "struct", outputs != "pos", norm=False)


@pytest.mark.parametrize("shape", [(1, 5, 1), (63, 5, 32), (257, 100, 33), (257, 5, 500), (1899, 100, 32)], ids=lambda s: "%dx%dx%d" % s)
def test_the_normalised_position_output_and_its_backward(shape):
    n, A, d = shape
    compare("%s normalised" % (shape,), inputs(n, A, d), True, False, norm=True)
    compare("%s normalised, both" % (shape,), inputs(n, A, d), True, True, norm=True)


@pytest.mark.parametrize("kind", ["equal", "permutation"])
def test_one_pull_list_of_all_items_and_lists_of_one_item(kind):
    """idx all equal: one list of 257 x 100 = 25 700 items, 51 pieces of 512 (and 1 607 pieces of 16); a permutation per set: every node's
    list has exactly A items"""
    from ctgcn_amd import ops
    v = inputs(257, 100, 33, kind)
    for piece in (None, 16):
        prep = ops.pgnn_prepare(torch.from_numpy(v["dm"]).to(DEV), torch.from_numpy(v["idx"]).to(DEV), piece=piece)
        _, pieces, multi, multi_ptr, rows = prep.pull()
        if kind == "equal":
            assert pieces.shape[1] == -(-25700 // (piece or 512)) and multi.tolist() == [128] and rows == pieces.shape[1]
        else:
            assert pieces.shape[1] == (257 if piece is None else 257 * 7) and (rows == 0) == (piece is None)
        compare("%s piece %s" % (kind, piece), v, True, True, norm=True, piece=piece)


@pytest.mark.parametrize("shape", [(63, 5, 32), (257, 100, 33), (257, 5, 200)], ids=lambda s: "%dx%dx%d" % s)
def test_the_dropout_epilogue_matches_the_mirror_fed_the_host_model_s_mask(shape):
    n, A, d = shape
    key, p = 2 ** 61 + 12345, 0.5
    keep = R.keep_mask(key, n, d, p)
    assert 0.3 < keep.mean() < 0.7
    compare("%s dropout" % (shape,), inputs(n, A, d), False, True, norm=False, keep=keep, p=p, key=key)
    compare("%s dropout, both" % (shape,), inputs(n, A, d), True, True, norm=True, keep=keep, p=p, key=key)


def test_without_a_table_the_distances_themselves_scale_the_messages_and_many_values_take_the_composed_route():
    from ctgcn_amd import ops
    v = inputs(63, 5, 32)
    v["table"] = VALUES.copy()
    compare("no table", v, True, True, norm=False, table=False)
    # more distinct values than PGNN_MAX_TABLE: the composed torch formulation, same results as a mirror fed those values
    n, A, d = 257, 100, 8
    w = inputs(n, A, d)
    dm = np.linspace(0.0, 1.0, n * A, dtype=np.float32).reshape(n, A)
    assert np.unique(dm).size > ops.PGNN_MAX_TABLE
    w.update(dm=dm, lvl=np.arange(n * A).reshape(n, A), table=dm.reshape(-1).copy())
    key = 77
    keep = R.keep_mask(key, n, d, 0.5)
    assert ops.pgnn_prepare(torch.from_numpy(dm).to(DEV), torch.from_numpy(w["idx"]).to(DEV)).composed
    compare("composed", w, True, True, norm=True, keep=keep, p=0.5, key=key, table=False)
    with pytest.raises(ValueError, match="PGNN_MAX_TABLE"):
        ops.pgnn_conv(torch.zeros(n, 2 * d, device=DEV), torch.from_numpy(dm).to(DEV), torch.from_numpy(w["idx"]).to(DEV),
                      torch.zeros(d, device=DEV), None, table=torch.zeros(n * A, device=DEV))


def test_arguments_are_checked():
    from ctgcn_amd import _lib, ops
    PS, dm = torch.zeros(6, 8, device=DEV), torch.zeros(6, 3, device=DEV)
    da, w = torch.zeros(6, 3, dtype=torch.int64, device=DEV), torch.zeros(4, device=DEV)
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm, da, w, need_pos=False, need_struct=False)
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm, da + 6, w)                          # an index outside [0, n)
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm, da, w[:3])
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm[:, :2], da, w)
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm, da, w, p=1.0)
    with pytest.raises(ValueError):
        ops.pgnn_conv(PS, dm, da, w, table=torch.zeros(2, device=DEV))      # one distinct value: a table of one entry
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.pgnn_conv(PS.cpu(), dm, da, w)
    pos, st = ops.pgnn_conv(PS, dm, da, w)
    assert tuple(pos.shape) == (6, 3) and tuple(st.shape) == (6, 4) and not pos.any() and not st.any()


def test_forward_and_backward_stay_below_a_quarter_of_one_materialised_tensor():
    """N = 20 000, A = 196, out = 128.  One [N, A, out] fp32 tensor is N A out 4 = 2.0 GB, and the materialising form holds several
    (the gathered features, the products, the ReLU output, their gradients).  The fused path's arrays are [N, A] and [N, out] sized:
    the prepared index (lvl, idx, two sorted item lists, torch's sort and unique temporaries), pos, gd', gx: about N A 40 bytes =
    0.16 GB plus the sort's workspace.  The bound: the peak above the inputs stays below N A out 4 / 4 = 0.5 GB."""
    from ctgcn_amd import ops
    n, A, d = 20000, 196, 128
    gen = torch.Generator(device=DEV).manual_seed(5)
    PS = torch.randn(n, 2 * d, device=DEV, generator=gen).requires_grad_(True)
    dm = torch.from_numpy(VALUES).to(DEV)[torch.randint(0, len(VALUES), (n, A), device=DEV, generator=gen)]
    da = torch.randint(0, n, (n, A), device=DEV, generator=gen)
    da[torch.rand(n, A, device=DEV, generator=gen) < 0.5] = 0     # half of all items in one pull list
    table = torch.from_numpy(TABLE).to(DEV).requires_grad_(True)
    w, b = torch.randn(d, device=DEV, generator=gen).requires_grad_(True), torch.zeros(1, device=DEV, requires_grad=True)
    cp, cs = torch.randn(n, A, device=DEV, generator=gen), torch.randn(n, d, device=DEV, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    pos, st = ops.pgnn_conv(PS, dm, da, w, b, table=table, epi=ops.PGNN_EPI_NORM, p=0.5, key=9)
    ((pos * cp).sum() + (st * cs).sum()).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    bound = n * A * d * 4 // 4
    print("  [mem] peak above the inputs %.1f MB = %.3f of the bound %.1f MB (N A 40 bytes = %.1f MB)" % (peak / 1e6, peak / bound, bound / 1e6, n * A * 40 / 1e6))
    assert peak < bound
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (PS, table, w, b))


def test_the_prepared_index_is_cached_per_pair_and_lets_go_of_an_int32_index_tensor():
    """an int32, contiguous dists_argmax needs no conversion: the prepared index must still hold a copy, or the cache entry would keep
    alive the very tensor whose death is meant to end it"""
    import gc
    import weakref
    from ctgcn_amd import ops
    dm, da = torch.zeros(6, 3, device=DEV), torch.zeros(6, 3, dtype=torch.int32, device=DEV)
    prep = ops.pgnn_prepare(dm, da)
    assert ops.pgnn_prepare(dm, da) is prep and prep.idx is not da and prep.idx.data_ptr() != da.data_ptr()
    alive = weakref.ref(da)
    del da, prep
    gc.collect()
    assert alive() is None
    assert not any(e[0]() is dm and e[1]() is not None for e in ops._pgnn_cache)
