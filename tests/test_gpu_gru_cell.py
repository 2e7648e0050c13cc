"""ctgcn_grucell.hip and ops.gru_layer on the GPU, at the smallest shapes at which they can go wrong: widths around the float4 and the
wave boundaries, odd widths (the scalar form), more rows than a block, every optional operand present and absent, padded row strides,
bases one float off a 16-byte boundary, the running sum at its first and at a later step.

The reference is the float64 dense definition (tests/_gru_ref.py) and its autograd.  Rule of tests/test_gpu_lstm_cell.py: error <=
max(4 x yardstick, floor) max|ref|, floor 2e-6 for outputs and 1e-5 for gradients; the yardstick is the float32 evaluation of the same
dense definition against the float64 one.  CTGCN_PARITY_OUT=<dir> keeps the shares of the tolerance used."""
import numpy as np
import pytest
import torch

import _gru_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 129, 256, 300, 500)
ROWS = (1, 3, 64, 65, 257)
_used = {}


def placed(src, pad=0, off=0):
    """src [B, W] in memory of its own with row stride W + pad, starting off floats past an aligned base"""
    B, W = src.shape
    buf = torch.full((B * (W + pad) + off + 4,), float("nan"), dtype=torch.float32, device=src.device)
    t = buf[off:off + B * (W + pad)].view(B, W + pad)[:, :W]
    t.copy_(src)
    assert t.stride(0) == W + pad and (t.data_ptr() - buf.data_ptr()) == 4 * off
    return t


def rnd(gen, *shape, scale=1.0):
    return (torch.randn(*shape, generator=gen, dtype=torch.float32) * scale).to(DEV)


def run_fwd(gi, gh, b_hh, h_prev, pad=0, off=0, keep=True, acc=None, acc_init=False):
    """(h, gates, q, acc) of one kernel call on operands placed in memory of their own; acc: the running sum before the step, or None"""
    from ctgcn_amd import ops
    B, H = gi.shape[0], gi.shape[1] // 3
    p = lambda t: None if t is None else placed(t, pad, off)  # noqa: E731
    blank = lambda w: placed(torch.full((B, w), float("nan"), device=DEV), pad, off)  # noqa: E731
    h, gates, q = blank(H), (blank(3 * H) if keep else None), (blank(H) if keep else None)
    acc_io = None if acc is None else p(acc)
    ops._gru_cell_fwd(p(gi), p(gh), b_hh, p(h_prev), h, gates, q, acc_io, acc_init)
    return h, gates, q, acc_io


def run_bwd(gates, q, h_prev, dh_out, dh_rec, pad=0, off=0, want_dgh=True, want_dh_prev=True):
    from ctgcn_amd import ops
    B, H = q.shape
    p = lambda t: None if t is None else placed(t, pad, off)  # noqa: E731
    blank = lambda w: placed(torch.full((B, w), float("nan"), device=DEV), pad, off)  # noqa: E731
    dgi, dgh, dh_prev = blank(3 * H), (blank(3 * H) if want_dgh else None), (blank(H) if want_dh_prev else None)
    ops._gru_cell_bwd(p(gates), p(q), p(h_prev), p(dh_out), p(dh_rec), dgi, dgh, dh_prev)
    return dgi, dgh, dh_prev


def up(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("H", WIDTHS)
def test_cell_forward_and_backward_in_every_form(H):
    gen = torch.Generator().manual_seed(100 + H)
    worst = 0.0
    for B in ROWS:
        gi, gh, h_prev = rnd(gen, B, 3 * H, scale=1.5), rnd(gen, B, 3 * H), rnd(gen, B, H)
        b_hh, acc0 = rnd(gen, 3 * H, scale=0.3), rnd(gen, B, H, scale=2.0)
        nan = torch.full((B, H), float("nan"), device=DEV)                 # a first step must not read what acc held
        dh_out, dh_rec = rnd(gen, B, H), rnd(gen, B, H)
        # (gh, b_hh, h_prev, pad, off, gates and q kept, acc before the step, first step of the sum)
        for tag, a_gh, a_b, a_hp, pad, off, keep, a_acc, init in (
                ("full", gh, b_hh, h_prev, 0, 0, True, None, False), ("step0", None, b_hh, None, 0, 0, True, None, False),
                ("step0-nobias", None, None, None, 0, 0, True, None, False), ("nobias", gh, None, h_prev, 0, 0, True, None, False),
                ("padded", gh, b_hh, h_prev, 4, 0, True, acc0, False), ("odd-pad", gh, b_hh, h_prev, 3, 0, True, acc0, False),
                ("offset", gh, b_hh, h_prev, 0, 1, True, acc0, False), ("inference", gh, b_hh, h_prev, 0, 0, False, None, False),
                ("acc-first", None, b_hh, None, 0, 0, True, nan, True), ("acc-later", gh, b_hh, h_prev, 0, 0, True, acc0, False),
                ("acc-first-inference", None, b_hh, None, 0, 0, False, nan, True), ("acc-later-inference", gh, b_hh, h_prev, 0, 0, False, acc0, False)):
            h, gates, q, acc = run_fwd(gi, a_gh, a_b, a_hp, pad, off, keep, a_acc, init)
            h64, g64, q64 = G.cell_fwd(up(gi), up(a_gh), up(a_b), up(a_hp))
            h32, g32, q32 = G.cell_fwd(gi, a_gh, a_b, a_hp)
            what = "cell fwd H %d B %d %s" % (H, B, tag)
            worst = max(worst, G.dense_share(what + " h", h, h64, h32, 2e-6))
            if keep:
                worst = max(worst, G.dense_share(what + " gates", gates, g64, g32, 2e-6))
                if float(q64.abs().max()) > 0:
                    worst = max(worst, G.dense_share(what + " q", q, q64, q32, 2e-6))
                else:
                    assert float(q.abs().max()) == 0.0
            if a_acc is not None:
                worst = max(worst, G.dense_share(what + " acc", acc, h64 if init else a_acc.double() + h64, h32 if init else a_acc + h32, 2e-6))
        _, gates32, q32 = G.cell_fwd(gi, gh, b_hh, h_prev)
        # (h_prev, dh_out, dh_rec, pad, off, dgh wanted, dh_prev wanted): a middle step, the last step, a step without a gradient from
        # above, step 0, a step whose dgh nobody reads, padded strides, a base one float off
        for tag, a_hp, a_do, a_dr, pad, off, w_dgh, w_dp in (("full", h_prev, dh_out, dh_rec, 0, 0, True, True),
                                                          ("last", h_prev, dh_out, None, 0, 0, True, True),
                                                          ("no-dh-out", h_prev, None, dh_rec, 0, 0, True, True),
                                                          ("step0", None, dh_out, dh_rec, 0, 0, True, False),
                                                          ("no-dgh", None, dh_out, dh_rec, 0, 0, False, False),
                                                          ("padded", h_prev, dh_out, dh_rec, 4, 0, True, True),
                                                          ("odd-pad", h_prev, dh_out, dh_rec, 3, 0, True, True),
                                                          ("offset", h_prev, dh_out, dh_rec, 0, 1, True, True)):
            dgi, dgh, dh_prev = run_bwd(gates32, q32, a_hp, a_do, a_dr, pad, off, w_dgh, w_dp)
            r64 = G.cell_bwd(up(gates32), up(q32), up(a_hp), up(a_do), up(a_dr))
            r32 = G.cell_bwd(gates32, q32, a_hp, a_do, a_dr)
            what = "cell bwd H %d B %d %s" % (H, B, tag)
            worst = max(worst, G.dense_share(what + " dgi", dgi, r64[0], r32[0], 1e-5))
            if w_dgh:
                worst = max(worst, G.dense_share(what + " dgh", dgh, r64[1], r32[1], 1e-5))
            if w_dp:
                worst = max(worst, G.dense_share(what + " dh_prev", dh_prev, r64[2], r32[2], 1e-5))
    _used["H %d" % H] = worst
    G.record_parity("cell", _used)
    assert worst <= 1.0, "share of the tolerance used %.3f" % worst


def test_cell_backward_agrees_with_autograd_of_the_forward():
    """cell_bwd of the mirror is itself written out by hand: the kernel against float64 autograd of the forward definition"""
    gen = torch.Generator().manual_seed(7)
    B, H = 9, 12
    gi, gh, h_prev, b_hh = rnd(gen, B, 3 * H), rnd(gen, B, 3 * H), rnd(gen, B, H), rnd(gen, 3 * H)
    dh_out, dh_rec = rnd(gen, B, H), rnd(gen, B, H)
    h, gates, q, _ = run_fwd(gi, gh, b_hh, h_prev)
    dgi, dgh, dh_prev = run_bwd(gates.contiguous(), q.contiguous(), h_prev, dh_out, dh_rec)
    gi64, gh64, hp64 = (t.double().requires_grad_(True) for t in (gi, gh, h_prev))
    h64 = G.cell_fwd(gi64, gh64, b_hh.double(), hp64)[0]
    want = torch.autograd.grad((h64 * (dh_out + dh_rec).double()).sum(), (gi64, gh64, hp64))
    for name, got, ref in zip(("dgi", "dgh", "dh_prev"), (dgi, dgh, dh_prev), want):
        assert float((got.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), name


def test_saturated_pre_activations_stay_finite_and_exact():
    B, H = 3, 8
    worst = 0.0
    for z in (30.0, -30.0, 100.0, -100.0, 1e4, -1e4):
        gi = torch.full((B, 3 * H), z, device=DEV)
        h_prev, b_hh = torch.full((B, H), 0.5, device=DEV), torch.full((3 * H,), 0.5, device=DEV)
        b_hh[:2 * H] = 0.0                                                 # q = 0.5; r and z saturate with gi
        for form in (dict(), dict(off=1)):                             # float4 and scalar
            h, gates, q, _ = run_fwd(gi, None, b_hh, h_prev, **form)
            h64, g64, q64 = G.cell_fwd(gi.double(), None, b_hh.double(), h_prev.double())
            h32, g32, q32 = G.cell_fwd(gi, None, b_hh, h_prev)
            for name, got, r64, r32 in (("h", h, h64, h32), ("gates", gates, g64, g32), ("q", q, q64, q32)):
                assert bool(torch.isfinite(got).all()), (z, name)
                worst = max(worst, G.dense_share("saturation z %g %s" % (z, name), got, r64, r32, 2e-6))
            if abs(z) >= 100:
                want = 1.0 if z > 0 else 0.0
                r, u, n = gates.chunk(3, dim=1)
                assert bool((r == want).all() and (u == want).all() and (n == (1.0 if z > 0 else -1.0)).all()), z
            ones = torch.ones(B, H, device=DEV)
            dgi, dgh, dh_prev = run_bwd(gates.contiguous(), q.contiguous(), h_prev, ones, ones, **form)
            r64 = G.cell_bwd(g64, q64, h_prev.double(), ones.double(), ones.double())
            r32 = G.cell_bwd(g32, q32, h_prev, ones, ones)
            assert bool(torch.isfinite(dgi).all() and torch.isfinite(dgh).all() and torch.isfinite(dh_prev).all()), z
            worst = max(worst, G.dense_share("saturation z %g dh_prev" % z, dh_prev, r64[2], r32[2], 1e-5))
            if z <= -100:
                assert float(dh_prev.abs().max()) == 0.0                   # dh z with z exactly 0
            if abs(z) >= 100:                                              # every gate gradient is exactly zero
                assert float(dgi.abs().max()) == 0.0 and float(dgh.abs().max()) == 0.0
            else:
                worst = max(worst, G.dense_share("saturation z %g dgi" % z, dgi, r64[0], r32[0], 1e-5),
                            G.dense_share("saturation z %g dgh" % z, dgh, r64[1], r32[1], 1e-5))
    G.record_parity("saturation", {"worst": worst})
    assert worst <= 1.0, worst


def test_the_same_call_twice_gives_the_same_bits():
    gen = torch.Generator().manual_seed(11)
    for H, off in ((500, 0), (300, 1)):
        B = 65
        gi, gh, h_prev, b_hh, acc0 = rnd(gen, B, 3 * H), rnd(gen, B, 3 * H), rnd(gen, B, H), rnd(gen, 3 * H), rnd(gen, B, H)
        a, b = run_fwd(gi, gh, b_hh, h_prev, off=off, acc=acc0), run_fwd(gi, gh, b_hh, h_prev, off=off, acc=acc0)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        dh = rnd(gen, B, H)
        args = (a[1].contiguous(), a[2].contiguous(), h_prev, dh, dh)
        u, v = run_bwd(*args, off=off), run_bwd(*args, off=off)
        assert all(torch.equal(x, y) for x, y in zip(u, v))


def test_the_gates_may_take_the_memory_of_gi_and_dh_prev_that_of_dh_rec():
    """what ops.gru_layer relies on: each element is read once and written once by the same thread"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(13)
    for H in (500, 300, 7):
        B = 65
        gi, gh, h_prev, b_hh = rnd(gen, B, 3 * H), rnd(gen, B, 3 * H), rnd(gen, B, H), rnd(gen, 3 * H)
        h, gates, q, _ = run_fwd(gi, gh, b_hh, h_prev)
        h2, q2, inplace = torch.empty_like(h_prev), torch.empty_like(h_prev), gi.clone()
        ops._gru_cell_fwd(inplace, gh, b_hh, h_prev, h2, inplace, q2)
        assert torch.equal(inplace, gates) and torch.equal(h2, h) and torch.equal(q2, q)
        dh_out, dh_rec = rnd(gen, B, H), rnd(gen, B, H)
        dgi, dgh, dh_prev = run_bwd(inplace, q2, h_prev, dh_out, dh_rec)
        dgi2, dgh2, rec_io = torch.empty_like(inplace), torch.empty_like(inplace), dh_rec.clone()
        ops._gru_cell_bwd(inplace, q2, h_prev, dh_out, rec_io, dgi2, dgh2, rec_io)
        assert torch.equal(dgi2, dgi) and torch.equal(dgh2, dgh) and torch.equal(rec_io, dh_prev)
        # what the contract allows beyond that: h in the memory of h_prev, dgi in that of the saved gates
        h_io = h_prev.clone()
        ops._gru_cell_fwd(gi, gh, b_hh, h_io, h_io, None, None)
        assert torch.equal(h_io, h)
        gates_io = inplace.clone()
        ops._gru_cell_bwd(gates_io, q2, h_prev, dh_out, dh_rec, gates_io, dgh2, None)
        assert torch.equal(gates_io, dgi) and torch.equal(dgh2, dgh)


# ------------------------------------------------------------------------------------------------ ops.gru_layer
def layer_case(what, B, L, I, H, reduce_sum, bias, seed, precomputed=False, check_no_grad=True):
    """one ops.gru_layer call and its backward against float64 autograd of the dense definition; the share of the rule used"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(seed)
    bound = 1.0 / np.sqrt(H)
    params = {"w_ih": rnd(gen, 3 * H, I, scale=bound), "w_hh": rnd(gen, 3 * H, H, scale=bound)}
    if bias:
        params["b_ih"], params["b_hh"] = rnd(gen, 3 * H, scale=0.1), rnd(gen, 3 * H, scale=0.1)
    x = rnd(gen, B, L, I)
    dout = rnd(gen, B, H) if reduce_sum else rnd(gen, B, L, H)

    def dense(dtype):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in dict(params, x=x).items()}
        gi = None
        if precomputed:
            gi = leaves["x"] @ leaves["w_ih"].t() + (leaves["b_ih"] if bias else 0)
        out = G.gru_dense(leaves["x"], leaves["w_ih"], leaves["w_hh"], leaves.get("b_ih"), leaves.get("b_hh"), gi=gi, reduce_sum=reduce_sum)
        names = sorted(leaves)
        got = torch.autograd.grad((out * dout.to(dtype)).sum(), [leaves[k] for k in names], allow_unused=True)      # L = 1 does not use w_hh
        return out.detach(), {k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in zip(names, got)}

    leaves = {k: v.clone().requires_grad_(True) for k, v in dict(params, x=x).items()}
    if precomputed:                                                    # the input projection made by the caller, bias_ih folded in
        gi = leaves["x"] @ leaves["w_ih"].t() + (leaves["b_ih"] if bias else 0)
        out = ops.gru_layer(None, None, leaves["w_hh"], None, leaves.get("b_hh"), reduce_sum=reduce_sum, gi=gi)
    else:
        out = ops.gru_layer(leaves["x"], leaves["w_ih"], leaves["w_hh"], leaves.get("b_ih"), leaves.get("b_hh"), reduce_sum=reduce_sum)
    assert out.requires_grad and tuple(out.shape) == ((B, H) if reduce_sum else (B, L, H))
    names = sorted(leaves)
    grads = dict(zip(names, torch.autograd.grad((out * dout).sum(), [leaves[k] for k in names])))
    (o64, g64), (o32, g32) = dense(torch.float64), dense(torch.float32)
    used = G.dense_share(what + " out", out, o64, o32, 2e-6)
    for k in names:
        assert tuple(grads[k].shape) == tuple(leaves[k].shape)
        used = max(used, G.dense_share(what + " d" + k, grads[k], g64[k], g32[k], 1e-5))
    if check_no_grad:
        with torch.no_grad():                                          # without grad: nothing per step kept, h in two buffers; the same bits
            if precomputed:
                again = ops.gru_layer(None, None, params["w_hh"], None, params.get("b_hh"), reduce_sum=reduce_sum, gi=gi.detach())
            else:
                again = ops.gru_layer(x, params["w_ih"], params["w_hh"], params.get("b_ih"), params.get("b_hh"), reduce_sum=reduce_sum)
        assert not again.requires_grad and torch.equal(again, out.detach())
    return used


@pytest.mark.parametrize("reduce_sum", [False, True], ids=["sequence", "sum"])
@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_gru_layer_outputs_and_gradients(L, reduce_sum):
    used = {}
    for bias in (True, False):
        for H, I, B in ((6, 7, 5), (8, 5, 66)):                        # the scalar and the float4 form
            what = "layer L %d %s bias %d H %d" % (L, "sum" if reduce_sum else "seq", bias, H)
            used[what] = layer_case(what, B, L, I, H, reduce_sum, bias, seed=17 * L + H)
    used["precomputed gi L %d" % L] = layer_case("layer L %d gi" % L, 5, L, 7, 8, reduce_sum, True, seed=3 + L, precomputed=True)
    G.record_parity("layer_L%d_%s" % (L, "sum" if reduce_sum else "seq"), used)
    assert max(used.values()) <= 1.0, used


def test_gru_layer_256_wide_from_500_inputs():
    used = {"H 256 sequence": layer_case("layer H 256 seq", 3, 3, 500, 256, False, True, seed=29),
            "H 256 sum": layer_case("layer H 256 sum", 3, 3, 500, 256, True, True, seed=31)}
    G.record_parity("layer_H256", used)
    assert max(used.values()) <= 1.0, used


@pytest.mark.parametrize("reduce_sum", [False, True], ids=["sequence", "sum"])
def test_gru_layer_row_chunks(reduce_sum, monkeypatch):
    """more rows than a chunk: 66 rows in 4 chunks of 17 (ragged tail), forward and backward by the same rule as the unchunked call; the
    library may pick another GEMM kernel for another row count, so the two are compared through the reference and not bit for bit"""
    from ctgcn_amd import ops
    B, L, I, H = 66, 3, 5, 8
    seen = []
    monkeypatch.setattr(ops, "_GI_MAX_ELEMS", 20 * L * 3 * H)
    ops.set_launch_timer(lambda name, start, end, meta: seen.append((name, meta["n"])))
    try:
        used = layer_case("layer chunked %s" % ("sum" if reduce_sum else "seq"), B, L, I, H, reduce_sum, True, seed=41, check_no_grad=False)
    finally:
        ops.set_launch_timer(None)
    assert [n for name, n in seen if name == "gru_cell_fwd"] == [17] * (3 * L) + [15] * L
    assert sorted(n for name, n in seen if name == "gru_cell_bwd") == [15] * L + [17] * (3 * L)
    G.record_parity("layer_chunked_%s" % ("sum" if reduce_sum else "seq"), {"worst": used})
    assert used <= 1.0, used
    # inference through the same chunks: no buffer beyond the bound, the same rule
    gen = torch.Generator().manual_seed(43)
    x, w_ih, w_hh = rnd(gen, B, L, I), rnd(gen, 3 * H, I, scale=0.3), rnd(gen, 3 * H, H, scale=0.3)
    with torch.no_grad():
        got = ops.gru_layer(x, w_ih, w_hh, reduce_sum=reduce_sum)
        twice = ops.gru_layer(x, w_ih, w_hh, reduce_sum=reduce_sum)
    assert torch.equal(got, twice)
    r64 = G.gru_dense(x.double(), w_ih.double(), w_hh.double(), reduce_sum=reduce_sum)
    r32 = G.gru_dense(x, w_ih, w_hh, reduce_sum=reduce_sum)
    assert G.dense_share("layer chunked inference", got, r64, r32, 2e-6) <= 1.0


def test_gru_layer_takes_a_time_major_view_and_refuses_wrong_arguments():
    """the [B, L, H] output of an unchunked call is a view of time-major memory which a next layer reads as it is"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(23)
    B, L, I, H = 6, 3, 5, 8
    x, w_ih, w_hh = rnd(gen, B, L, I), rnd(gen, 3 * H, I, scale=0.3), rnd(gen, 3 * H, H, scale=0.3)
    with torch.no_grad():
        a = ops.gru_layer(x, w_ih, w_hh)
        b = ops.gru_layer(x.transpose(0, 1).contiguous().transpose(0, 1), w_ih, w_hh)
        s = ops.gru_layer(x, w_ih, w_hh, reduce_sum=True)
    assert a.transpose(0, 1).is_contiguous() and torch.equal(a, b)
    assert float((s - a.sum(1)).abs().max()) <= 2e-6 * float(s.abs().max())
    with pytest.raises(TypeError):
        ops.gru_layer(x.double(), w_ih.double(), w_hh.double())
    with pytest.raises(ValueError):
        ops.gru_layer(x, w_ih, w_hh[:, :4])
    with pytest.raises(ValueError):
        ops.gru_layer(x, w_ih[:, :4], w_hh)
    with pytest.raises(ValueError):
        ops.gru_layer(x, w_ih, w_hh, bias_hh=torch.zeros(2 * H, device=DEV))
    with pytest.raises(ValueError):
        ops.gru_layer(x, w_ih, w_hh, gi=torch.zeros(B, L, 3 * H, device=DEV))
    with pytest.raises(ValueError):
        ops.gru_layer(None, None, w_hh, gi=torch.zeros(B, L, 4 * H, device=DEV))
    with pytest.raises(ValueError):
        ops.gru_layer(x[0], w_ih, w_hh)
