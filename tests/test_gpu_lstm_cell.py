"""ctgcn_lstmcell.hip and ops.lstm_layer on the GPU, at the smallest shapes at which they can go wrong: widths around the float4 and
the wave boundaries, odd widths (the scalar form; 1899 is the shipped width of DynRNN's last layer), more rows than a block, every
optional operand present and absent, padded row strides, bases one float off a 16-byte boundary.

The reference is the float64 dense definition (tests/_dynrnn_ref.py) and its autograd.  Rule of tests/test_gpu_vgrnn.py: error <=
max(4 x yardstick, floor) max|ref|, floor 2e-6 for outputs and 1e-5 for gradients; the yardstick is the float32 evaluation of the same
dense definition against the float64 one.  CTGCN_PARITY_OUT=<dir> keeps the shares of the tolerance used."""
import numpy as np
import pytest
import torch

import _dyngem_ref as D
import _dynrnn_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = (1, 2, 3, 4, 5, 7, 8, 63, 64, 65, 127, 128, 129, 300, 500, 1899)
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


def run_fwd(gi, gh, bias, c_prev, pad=0, off=0, want_gates=True):
    from ctgcn_amd import ops
    B, H = gi.shape[0], gi.shape[1] // 4
    p = lambda t: None if t is None else placed(t, pad, off)  # noqa: E731
    blank = lambda w: placed(torch.full((B, w), float("nan"), device=DEV), pad, off)  # noqa: E731
    h, c, gates = blank(H), blank(H), (blank(4 * H) if want_gates else None)
    ops._lstm_cell_fwd(p(gi), p(gh), bias, p(c_prev), h, c, gates)
    return h, c, gates


def run_bwd(gates, c, c_prev, dh_out, dh_rec, dc_next, pad=0, off=0, want_dc_prev=True):
    from ctgcn_amd import ops
    B, H = c.shape
    p = lambda t: None if t is None else placed(t, pad, off)  # noqa: E731
    blank = lambda w: placed(torch.full((B, w), float("nan"), device=DEV), pad, off)  # noqa: E731
    dgates, dc_prev = blank(4 * H), (blank(H) if want_dc_prev else None)
    ops._lstm_cell_bwd(p(gates), p(c), p(c_prev), p(dh_out), p(dh_rec), p(dc_next), dgates, dc_prev)
    return dgates, dc_prev


def up(t):
    return None if t is None else t.double()


@pytest.mark.parametrize("H", WIDTHS)
def test_cell_forward_and_backward_in_every_form(H):
    gen = torch.Generator().manual_seed(100 + H)
    worst = 0.0
    for B in ROWS:
        gi, gh, c_prev = rnd(gen, B, 4 * H, scale=1.5), rnd(gen, B, 4 * H), rnd(gen, B, H)
        bias = rnd(gen, 4 * H, scale=0.3)
        dh_out, dh_rec, dc_next = rnd(gen, B, H), rnd(gen, B, H), rnd(gen, B, H)
        # (gh, bias, c_prev, pad, off, gates kept): the general step, step 0, padded strides, a base one float off, inference
        for tag, a_gh, a_bias, a_cp, pad, off, keep in (("full", gh, bias, c_prev, 0, 0, True), ("step0", None, None, None, 0, 0, True),
                                                        ("nobias", gh, None, c_prev, 0, 0, True), ("padded", gh, bias, c_prev, 4, 0, True),
                                                        ("odd-pad", gh, bias, c_prev, 3, 0, True), ("offset", gh, bias, c_prev, 0, 1, True),
                                                        ("inference", gh, bias, c_prev, 0, 0, False)):
            h, c, gates = run_fwd(gi, a_gh, a_bias, a_cp, pad, off, keep)
            h64, c64, g64 = R.cell_fwd(up(gi), up(a_gh), up(a_bias), up(a_cp))
            h32, c32, g32 = R.cell_fwd(gi, a_gh, a_bias, a_cp)
            what = "cell fwd H %d B %d %s" % (H, B, tag)
            worst = max(worst, R.dense_share(what + " h", h, h64, h32, 2e-6), R.dense_share(what + " c", c, c64, c32, 2e-6))
            if keep:
                worst = max(worst, R.dense_share(what + " gates", gates, g64, g32, 2e-6))
        gates32, c32 = R.cell_fwd(gi, gh, bias, c_prev)[2], R.cell_fwd(gi, gh, bias, c_prev)[1]
        # (c_prev, dh_out, dh_rec, dc_next, pad, off, dc_prev wanted): a middle step, the last step, a last-only layer's middle step,
        # step 0, padded strides, a base one float off
        for tag, a_cp, a_do, a_dr, a_dn, pad, off, keep in (("full", c_prev, dh_out, dh_rec, dc_next, 0, 0, True),
                                                            ("last", c_prev, dh_out, None, None, 0, 0, True),
                                                            ("no-dh-out", c_prev, None, dh_rec, dc_next, 0, 0, True),
                                                            ("step0", None, dh_out, dh_rec, dc_next, 0, 0, False),
                                                            ("padded", c_prev, dh_out, dh_rec, dc_next, 4, 0, True),
                                                            ("odd-pad", c_prev, dh_out, dh_rec, dc_next, 3, 0, True),
                                                            ("offset", c_prev, dh_out, dh_rec, dc_next, 0, 1, True)):
            dgates, dc_prev = run_bwd(gates32, c32, a_cp, a_do, a_dr, a_dn, pad, off, keep)
            dg64, dp64 = R.cell_bwd(up(gates32), up(c32), up(a_cp), up(a_do), up(a_dr), up(a_dn))
            dg32, dp32 = R.cell_bwd(gates32, c32, a_cp, a_do, a_dr, a_dn)
            what = "cell bwd H %d B %d %s" % (H, B, tag)
            worst = max(worst, R.dense_share(what + " dgates", dgates, dg64, dg32, 1e-5))
            if keep:
                worst = max(worst, R.dense_share(what + " dc_prev", dc_prev, dp64, dp32, 1e-5))
    _used["H %d" % H] = worst
    R.record_parity("cell", _used)
    assert worst <= 1.0, "share of the tolerance used %.3f" % worst


def test_cell_backward_agrees_with_autograd_of_the_forward():
    """cell_bwd of the mirror is itself written out by hand: the kernel against float64 autograd of the forward definition"""
    gen = torch.Generator().manual_seed(7)
    B, H = 9, 12
    gi, c_prev = rnd(gen, B, 4 * H), rnd(gen, B, H)
    dh, dc_next = rnd(gen, B, H), rnd(gen, B, H)
    h, c, gates = run_fwd(gi, None, None, c_prev)
    dgates, dc_prev = run_bwd(gates.contiguous(), c.contiguous(), c_prev, dh, None, dc_next)
    gi64, cp64 = gi.double().requires_grad_(True), c_prev.double().requires_grad_(True)
    h64, c64, _ = R.cell_fwd(gi64, None, None, cp64)
    dz, dcp = torch.autograd.grad((h64 * dh.double()).sum() + (c64 * dc_next.double()).sum(), (gi64, cp64))
    assert float((dgates.double() - dz).abs().max()) <= 1e-5 * float(dz.abs().max())
    assert float((dc_prev.double() - dcp).abs().max()) <= 1e-5 * float(dcp.abs().max())


def test_saturated_pre_activations_stay_finite_and_exact():
    B, H = 3, 8
    worst = 0.0
    for z in (30.0, -30.0, 100.0, -100.0, 1e4, -1e4):
        gi = torch.full((B, 4 * H), z, device=DEV)
        c_prev = torch.full((B, H), 0.5, device=DEV)
        for form in (dict(), dict(off=1)):                             # float4 and scalar
            h, c, gates = run_fwd(gi, None, None, c_prev, **form)
            h64, c64, g64 = R.cell_fwd(gi.double(), None, None, c_prev.double())
            h32, c32, g32 = R.cell_fwd(gi, None, None, c_prev)
            for name, got, r64, r32 in (("h", h, h64, h32), ("c", c, c64, c32), ("gates", gates, g64, g32)):
                assert bool(torch.isfinite(got).all()), (z, name)
                worst = max(worst, R.dense_share("saturation z %g %s" % (z, name), got, r64, r32, 2e-6))
            if abs(z) >= 100:
                want = 1.0 if z > 0 else 0.0
                i, f, g, o = gates.chunk(4, dim=1)
                assert bool((i == want).all() and (f == want).all() and (o == want).all() and (g == (1.0 if z > 0 else -1.0)).all()), z
            ones = torch.ones(B, H, device=DEV)
            dgates, dc_prev = run_bwd(gates.contiguous(), c.contiguous(), c_prev, ones, ones, ones, **form)
            dg64, dp64 = R.cell_bwd(g64, c64, c_prev.double(), ones.double(), ones.double(), ones.double())
            dg32, dp32 = R.cell_bwd(g32, c32, c_prev, ones, ones, ones)
            assert bool(torch.isfinite(dgates).all() and torch.isfinite(dc_prev).all()), z
            worst = max(worst, R.dense_share("saturation z %g dc_prev" % z, dc_prev, dp64, dp32, 1e-5))
            if float(dg64.abs().max()) > 1e-30:                        # at |z| >= 100 every gate gradient is exactly zero
                worst = max(worst, R.dense_share("saturation z %g dgates" % z, dgates, dg64, dg32, 1e-5))
            else:
                assert float(dgates.abs().max()) == 0.0
    R.record_parity("saturation", {"worst": worst})
    assert worst <= 1.0, worst


def test_the_same_call_twice_gives_the_same_bits():
    gen = torch.Generator().manual_seed(11)
    for H, off in ((1899, 0), (500, 0), (500, 1)):
        B = 65
        gi, gh, c_prev, bias = rnd(gen, B, 4 * H), rnd(gen, B, 4 * H), rnd(gen, B, H), rnd(gen, 4 * H)
        a, b = run_fwd(gi, gh, bias, c_prev, off=off), run_fwd(gi, gh, bias, c_prev, off=off)
        assert all(torch.equal(x, y) for x, y in zip(a, b))
        dh = rnd(gen, B, H)
        args = (a[2].contiguous(), a[1].contiguous(), c_prev, dh, dh, dh)
        u, v = run_bwd(*args, off=off), run_bwd(*args, off=off)
        assert all(torch.equal(x, y) for x, y in zip(u, v))


def test_the_gates_may_take_the_memory_of_gi_and_dc_prev_that_of_dc_next():
    """what ops.lstm_layer relies on: each element is read once and written once by the same thread"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(13)
    for H in (500, 1899):
        B = 65
        gi, c_prev = rnd(gen, B, 4 * H), rnd(gen, B, H)
        h, c, gates = run_fwd(gi, None, None, c_prev)
        h2, c2, inplace = torch.empty_like(c_prev), torch.empty_like(c_prev), gi.clone()
        ops._lstm_cell_fwd(inplace, None, None, c_prev, h2, c2, inplace)
        assert torch.equal(inplace, gates) and torch.equal(h2, h) and torch.equal(c2, c)
        dh, dc = rnd(gen, B, H), rnd(gen, B, H)
        dgates, dc_prev = run_bwd(inplace, c2, c_prev, dh, None, dc)
        dg2, dc_io = torch.empty_like(inplace), dc.clone()
        ops._lstm_cell_bwd(inplace, c2, c_prev, dh, None, dc_io, dg2, dc_io)
        assert torch.equal(dg2, dgates) and torch.equal(dc_io, dc_prev)


# ------------------------------------------------------------------------------------------------ ops.lstm_layer
def layer_case(what, B, L, I, H, last_only, bias, seed, precomputed=False):
    """one ops.lstm_layer call and its backward against float64 autograd of the dense definition; the share of the rule used"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(seed)
    bound = 1.0 / np.sqrt(H)
    params = {"w_ih": rnd(gen, 4 * H, I, scale=bound), "w_hh": rnd(gen, 4 * H, H, scale=bound)}
    if bias:
        params["b_ih"], params["b_hh"] = rnd(gen, 4 * H, scale=0.1), rnd(gen, 4 * H, scale=0.1)
    x = rnd(gen, B, L, I)
    dout = rnd(gen, B, H) if last_only else rnd(gen, B, L, H)

    def dense(dtype):
        leaves = {k: v.to(dtype).requires_grad_(True) for k, v in dict(params, x=x).items()}
        gi = None
        if precomputed:
            gi = leaves["x"] @ leaves["w_ih"].t() + (leaves["b_ih"] if bias else 0)
        out = R.lstm_dense(leaves["x"], leaves["w_ih"], leaves["w_hh"], leaves.get("b_ih"), leaves.get("b_hh"), gi=gi)
        out = out[:, -1] if last_only else out
        names = sorted(leaves)
        got = torch.autograd.grad((out * dout.to(dtype)).sum(), [leaves[k] for k in names], allow_unused=True)      # L = 1 does not use w_hh
        return out.detach(), {k: (torch.zeros_like(leaves[k]) if v is None else v) for k, v in zip(names, got)}

    leaves = {k: v.clone().requires_grad_(True) for k, v in dict(params, x=x).items()}
    if precomputed:                                                    # the input projection made by the caller, bias_ih folded in
        gi = leaves["x"] @ leaves["w_ih"].t() + (leaves["b_ih"] if bias else 0)
        out = ops.lstm_layer(None, None, leaves["w_hh"], None, leaves.get("b_hh"), last_only=last_only, gi=gi)
    else:
        out = ops.lstm_layer(leaves["x"], leaves["w_ih"], leaves["w_hh"], leaves.get("b_ih"), leaves.get("b_hh"), last_only=last_only)
    assert tuple(out.shape) == ((B, H) if last_only else (B, L, H))
    names = sorted(leaves)
    grads = dict(zip(names, torch.autograd.grad((out * dout).sum(), [leaves[k] for k in names])))
    (o64, g64), (o32, g32) = dense(torch.float64), dense(torch.float32)
    used = R.dense_share(what + " out", out, o64, o32, 2e-6)
    for k in names:
        assert tuple(grads[k].shape) == tuple(leaves[k].shape)
        used = max(used, R.dense_share(what + " d" + k, grads[k], g64[k], g32[k], 1e-5))
    if bias and not precomputed:
        assert torch.equal(grads["b_ih"], grads["b_hh"])               # equal, as in the reference
    with torch.no_grad():                                              # without grad: no gates kept, c in two buffers; the same bits
        if precomputed:
            again = ops.lstm_layer(None, None, params["w_hh"], None, params.get("b_hh"), last_only=last_only, gi=gi.detach())
        else:
            again = ops.lstm_layer(x, params["w_ih"], params["w_hh"], params.get("b_ih"), params.get("b_hh"), last_only=last_only)
    assert not again.requires_grad and torch.equal(again, out.detach())
    return used


@pytest.mark.parametrize("last_only", [False, True], ids=["sequence", "last-only"])
@pytest.mark.parametrize("L", [1, 2, 3, 5])
def test_lstm_layer_outputs_and_gradients(L, last_only):
    used = {}
    for bias in (True, False):
        for H, I, B in ((6, 7, 5), (8, 5, 66)):                        # the scalar and the float4 form
            what = "layer L %d %s bias %d H %d" % (L, "last" if last_only else "seq", bias, H)
            used[what] = layer_case(what, B, L, I, H, last_only, bias, seed=17 * L + H)
    used["precomputed gi L %d" % L] = layer_case("layer L %d gi" % L, 5, L, 7, 8, last_only, True, seed=3 + L, precomputed=True)
    R.record_parity("layer_L%d_%s" % (L, "last" if last_only else "seq"), used)
    assert max(used.values()) <= 1.0, used


def test_lstm_layer_stacks_without_copies_and_takes_batch_first_input():
    """the [B, L, H] output is a view of time-major memory which the next layer reads as it is; a batch-first input gives the same"""
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(23)
    B, L, I, H = 6, 3, 5, 8
    x, w_ih, w_hh = rnd(gen, B, L, I), rnd(gen, 4 * H, I, scale=0.3), rnd(gen, 4 * H, H, scale=0.3)
    with torch.no_grad():
        a = ops.lstm_layer(x, w_ih, w_hh)
        b = ops.lstm_layer(x.transpose(0, 1).contiguous().transpose(0, 1), w_ih, w_hh)
    assert a.transpose(0, 1).is_contiguous() and torch.equal(a, b)
    with pytest.raises(TypeError):
        ops.lstm_layer(x.double(), w_ih.double(), w_hh.double())
    with pytest.raises(ValueError):
        ops.lstm_layer(x, w_ih, w_hh[:, :4])
    with pytest.raises(ValueError):
        ops.lstm_layer(x, w_ih, w_hh, gi=torch.zeros(B, L, 4 * H, device=DEV))


def test_lstm_layer_at_the_width_of_dynrnn_s_last_layer():
    used = {"H 1899 sequence": layer_case("layer H 1899 seq", 3, 3, 24, 1899, False, True, seed=29),
            "H 1899 last-only": layer_case("layer H 1899 last", 3, 3, 24, 1899, True, True, seed=31)}
    R.record_parity("layer_H1899", used)
    assert max(used.values()) <= 1.0, used


def test_lstm_layer_fed_by_a_gather_2000_wide():
    """DynRNN's first layer at its shipped width: gi = rowsel_conv over the B L selected rows, d = 4 x 500"""
    import scipy.sparse as sp
    from ctgcn_amd import ops
    n, T, B, L, H = 70, 4, 9, 3, 500
    rng = np.random.default_rng(5)
    mats = [sp.random(n, n, density=0.08, random_state=int(rng.integers(1 << 30)), format="csr", dtype=np.float32).astype(np.float64) for _ in range(T)]
    rows = ops.SnapshotRows(mats, DEV)
    graph, node = rng.integers(0, T - L + 1, B), rng.integers(0, n, B)
    idx = np.stack([(graph + s) * n + node for s in range(L)], axis=1)
    idx[-1] = -1                                                       # a padded record
    gen = torch.Generator().manual_seed(37)
    w_ih, w_hh = rnd(gen, 4 * H, n, scale=0.1), rnd(gen, 4 * H, H, scale=1 / np.sqrt(H))
    b_ih, b_hh = rnd(gen, 4 * H, scale=0.1), rnd(gen, 4 * H, scale=0.1)
    dout = rnd(gen, B, L, H)
    xd = D.dense_rows(D.stacked(mats), idx, torch.float64, DEV)

    def dense(dtype):
        leaves = [t.to(dtype).requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh)]
        out = R.lstm_dense(xd.to(dtype), *leaves)
        return out.detach(), torch.autograd.grad((out * dout.to(dtype)).sum(), leaves)

    leaves = [t.clone().requires_grad_(True) for t in (w_ih, w_hh, b_ih, b_hh)]
    gi = ops.rowsel_conv(leaves[0].t().contiguous(), rows, idx.T.reshape(-1), leaves[2], relu=False, col_stride=0)
    assert tuple(gi.shape) == (L * B, 4 * H)
    out = ops.lstm_layer(None, None, leaves[1], None, leaves[3], gi=gi.view(L, B, 4 * H).transpose(0, 1))
    grads = torch.autograd.grad((out * dout).sum(), leaves)
    (o64, g64), (o32, g32) = dense(torch.float64), dense(torch.float32)
    used = {"out": R.dense_share("gather-fed layer out", out, o64, o32, 2e-6)}
    for k, got, r64, r32 in zip(("w_ih", "w_hh", "b_ih", "b_hh"), grads, g64, g32):
        used["d" + k] = R.dense_share("gather-fed layer d" + k, got, r64, r32, 1e-5)
    R.record_parity("layer_gather", used)
    assert max(used.values()) <= 1.0, used
