"""layers.rnn_reduce_norm and the models at embedding widths other than 128: the core-axis and the temporal RNN run as library GEMMs
plus the fused cell passes of ctgcn_grucell.hip / ctgcn_lstmcell.hip (ops.gru_layer / ops.lstm_layer), forward and backward.

References: float64 nn.GRU / nn.LSTM (+ sum, + LayerNorm) on the CPU for the layer, oracle/torch_path.py in float64 for the models.
Rule of tests/test_gpu_lstm_cell.py: error <= max(4 x yardstick, floor) max|ref|, floor 2e-6 for outputs and 1e-5 for gradients; the
yardstick is the float32 CPU evaluation of the same reference against the float64 one.  CTGCN_PARITY_OUT=<dir> keeps the shares."""
import copy

import pytest
import torch

import _gru_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CELL = {"GRU": ("gru_cell_fwd", "gru_cell_bwd"), "LSTM": ("lstm_cell_fwd", "lstm_cell_bwd")}
ALL_CELLS = set(CELL["GRU"] + CELL["LSTM"])
SHAPES = {16: (70, 4, 16), 64: (70, 4, 40), 256: (33, 3, 64)}       # hidden width: (rows, steps, d_in)


@pytest.fixture
def launches():
    """names of the timed HIP launches (ops.set_launch_timer) of the test"""
    from ctgcn_amd import ops
    seen = []
    ops.set_launch_timer(lambda name, start, end, meta: seen.append(name))
    try:
        yield seen
    finally:
        ops.set_launch_timer(None)


def module_run(rnn, norm, x, gsel, reduce_sum, dtype):
    """(output, gradients of sum(output gsel) by name) of norm(rnn(x)[0] (.sum(1))) through the torch modules on the CPU"""
    rnn, norm = copy.deepcopy(rnn).to(dtype), copy.deepcopy(norm).to(dtype)
    x = x.detach().clone().to(dtype).requires_grad_(True)
    out = rnn(x)[0]
    out = norm(out.sum(1) if reduce_sum else out)
    (out * gsel.to(dtype)).sum().backward()
    grads = {"rnn." + k: p.grad for k, p in rnn.named_parameters()}
    grads.update({"norm." + k: p.grad for k, p in norm.named_parameters()})
    grads["x"] = x.grad
    return out.detach(), grads


def layer_run(rnn, norm, x, gsel, reduce_sum):
    from ctgcn_amd import layers
    rnn.zero_grad()
    norm.zero_grad()
    x = x.detach().clone().requires_grad_(True)
    out = layers.rnn_reduce_norm(rnn, norm, x, reduce_sum)
    assert out.requires_grad
    (out * gsel).sum().backward()
    grads = {"rnn." + k: p.grad.clone() for k, p in rnn.named_parameters()}
    grads.update({"norm." + k: p.grad.clone() for k, p in norm.named_parameters()})
    grads["x"] = x.grad
    return out.detach().cpu(), {k: v.cpu() for k, v in grads.items()}


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
@pytest.mark.parametrize("hid", [16, 64, 256])
def test_rnn_reduce_norm_runs_the_cell_passes_and_matches_float64(hid, rnn_type, launches, monkeypatch):
    from ctgcn_amd import layers, ops
    rows, steps, d_in = SHAPES[hid]
    fwd, bwd = CELL[rnn_type]
    used = {}
    for reduce_sum in (True, False):
        for use_norm in (True, False):
            torch.manual_seed(1000 * hid + 10 * reduce_sum + use_norm)
            rnn = getattr(torch.nn, rnn_type)(d_in, hid, 1, batch_first=True)
            norm = torch.nn.LayerNorm(hid) if use_norm else torch.nn.Identity()
            x = torch.randn(rows, steps, d_in)
            gsel = torch.randn(rows, hid) if reduce_sum else torch.randn(rows, steps, hid)
            o64, g64 = module_run(rnn, norm, x, gsel, reduce_sum, torch.float64)
            o32, g32 = module_run(rnn, norm, x, gsel, reduce_sum, torch.float32)
            rnn_d, norm_d, xd, gd = copy.deepcopy(rnn).to(DEV), copy.deepcopy(norm).to(DEV), x.to(DEV), gsel.to(DEV)
            assert ops.rnn_cell_ok(rnn_d, xd) and not ops.gru_fused_ok(rnn_d, xd) and not ops.lstm_fused_ok(rnn_d, xd)
            what = "%s %d sum=%d ln=%d" % (rnn_type, hid, reduce_sum, use_norm)
            del launches[:]
            out, grads = layer_run(rnn_d, norm_d, xd, gd, reduce_sum)
            assert launches.count(fwd) == steps and launches.count(bwd) == steps, (what, launches)
            share = G.dense_share(what + " out", out, o64, o32, 2e-6)
            for k in sorted(g64):
                share = max(share, G.dense_share(what + " d" + k, grads[k], g64[k], g32[k], 1e-5))
            used[what] = share
            del launches[:]
            with torch.no_grad():
                again = layers.rnn_reduce_norm(rnn_d, norm_d, xd, reduce_sum)
                into = torch.full((rows, hid + 4), float("nan"), device=DEV)[:, :hid] if reduce_sum else None
                if into is not None:
                    assert layers.rnn_reduce_norm(rnn_d, norm_d, xd, reduce_sum, out=into) is into and torch.equal(into, again)
            assert launches.count(fwd) == steps * (2 if reduce_sum else 1) and bwd not in launches and not again.requires_grad
            assert torch.equal(again.cpu(), out), what + ": training forward != inference forward"
            # the switch: the PyTorch-ROCm modules, no cell launch, the same rule
            monkeypatch.setenv("CTGCN_RNN_CELL", "0")
            assert not ops.rnn_cell_ok(rnn_d, xd)
            del launches[:]
            out0, grads0 = layer_run(rnn_d, norm_d, xd, gd, reduce_sum)
            monkeypatch.delenv("CTGCN_RNN_CELL")
            assert not ALL_CELLS & set(launches), launches
            share0 = G.dense_share(what + " out (modules)", out0, o64, o32, 2e-6)
            for k in sorted(g64):
                share0 = max(share0, G.dense_share(what + " d" + k + " (modules)", grads0[k], g64[k], g32[k], 1e-5))
            used[what + " modules"] = share0
    G.record_parity("rnn_reduce_norm_%s_%d" % (rnn_type, hid), used)
    assert max(used.values()) <= 1.0, used


def test_what_the_cell_passes_do_not_cover_goes_to_the_modules(launches):
    """two layers, bidirectional, a projected LSTM: layers.rnn_over_rows, never a cell kernel; width 128 keeps its own kernels"""
    from ctgcn_amd import layers, ops
    torch.manual_seed(5)
    x = torch.randn(9, 3, 24, device=DEV)
    for rnn in (torch.nn.GRU(24, 32, 2, batch_first=True), torch.nn.LSTM(24, 32, 2, batch_first=True)):
        rnn = rnn.to(DEV)
        assert not ops.rnn_cell_ok(rnn, x)
        out = layers.rnn_reduce_norm(rnn, torch.nn.Identity(), x, True)
        assert out.requires_grad and tuple(out.shape) == (9, 32) and bool(torch.isfinite(out).all())
        out.sum().backward()
    assert not ALL_CELLS & set(launches), launches
    for rnn in (torch.nn.GRU(24, 32, 1, batch_first=True, bidirectional=True), torch.nn.LSTM(24, 32, 1, batch_first=True, proj_size=16),
                torch.nn.GRU(24, 32, 1)):
        assert not ops.rnn_cell_ok(rnn.to(DEV), x)
    wide = torch.nn.GRU(24, 128, 1, batch_first=True).to(DEV)
    assert ops.gru_fused_ok(wide, x) and not ops.rnn_cell_ok(wide, x)
    assert ops.rnn_cell_ok(torch.nn.GRU(24, 32, 1, batch_first=True).to(DEV), x) and not ops.rnn_cell_ok(torch.nn.GRU(24, 32, 1, batch_first=True).to(DEV), x.double())


# ------------------------------------------------------------------------------------------------ the models
_window = {}


def window():
    """3 snapshots of a 200-node graph with core lists of 2, 4 and 3 matrices: (CoreAdj list on the GPU, the oracle's lists, features)"""
    if not _window:
        from ctgcn_amd.helper import core_adj_from_scipy
        from ctgcn_amd.synth import dynamic_graph
        from oracle import oracle as O, torch_path as TP
        n, T = 200, 3
        adj, ref_adj = [], []
        for g, max_core, want in zip(dynamic_graph(n, 10, T, seed=4), (2, 4, 4), (2, 4, 3)):
            a, _, _ = core_adj_from_scipy(g, max_core, DEV)
            kept = O.core_adj_list([O.kcore_matrices(g)], 0, 1, 1, max_core)[0]
            assert len(kept) == want == a.K
            adj.append(a)
            ref_adj.append([TP.coo_like_reference(m) for m in kept])
        gen = torch.Generator().manual_seed(9)
        _window.update(n=n, T=T, adj=adj, ref_adj=ref_adj, x=[torch.randn(n, 20, generator=gen) for _ in range(T)])
    return _window


def build(kind, out_dim, rnn_type, seed=3):
    import ctgcn_amd
    torch.manual_seed(seed)
    if kind == "CGCN":
        return ctgcn_amd.CGCN(20, 48, out_dim, 1, 2, rnn_type=rnn_type).to(DEV)
    return ctgcn_amd.CTGCN(20, 48, out_dim, 1, 2, 3, rnn_type=rnn_type, model_type=kind, trans_activate_type="N" if kind == "S" else "L").to(DEV)


def flat(res):
    """the tensors of a model's result in a fixed order: CTGCN-C a tensor, CTGCN-S (tensor, list), CGCN a list"""
    if torch.is_tensor(res):
        return [res]
    out = []
    for r in res:
        out += flat(r)
    return out


def oracle_run(kind, sd, w, rnn_type, gsel, dtype):
    from oracle import torch_path as TP
    sdc = {k: v.to(dtype).requires_grad_(True) for k, v in sd.items()}
    x = [v.to(dtype) for v in w["x"]]
    adj = [[a.to(dtype).coalesce() for a in l] for l in w["ref_adj"]] if dtype == torch.float64 else w["ref_adj"]
    if kind == "CGCN":
        res = TP.cgcn_with_grad(sdc, x, adj, rnn_type, "C", "L")
    else:
        res = TP.ctgcn_with_grad(sdc, x, adj, rnn_type, kind, "N" if kind == "S" else "L")
    outs = flat(res)
    sum((o * g.to(dtype)).sum() for o, g in zip(outs, gsel)).backward()
    return [o.detach() for o in outs], {k: v.grad for k, v in sdc.items() if v.grad is not None}


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
@pytest.mark.parametrize("out_dim", [64, 40])
@pytest.mark.parametrize("kind", ["C", "S", "CGCN"])
def test_models_at_other_widths_match_the_float64_oracle(kind, out_dim, rnn_type, launches):
    w = window()
    model = build(kind, out_dim, rnn_type)
    xd = [v.to(DEV) for v in w["x"]]
    sd = {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}
    with torch.no_grad():
        inf = flat(model(xd, w["adj"]))
    fwd, bwd = CELL[rnn_type]
    steps = 2 * sum(a.K for a in w["adj"]) + (w["T"] if kind != "CGCN" else 0)       # two diffusion layers per snapshot, the temporal RNN
    assert launches.count(fwd) == steps and not (ALL_CELLS - {fwd}) & set(launches), launches
    gen = torch.Generator().manual_seed(11)
    gsel = [torch.randn(t.shape, generator=gen) for t in inf]
    o64, g64 = oracle_run(kind, sd, w, rnn_type, gsel, torch.float64)
    o32, g32 = oracle_run(kind, sd, w, rnn_type, gsel, torch.float32)
    del launches[:]
    outs = flat(model(xd, w["adj"]))
    sum((o * g.to(DEV)).sum() for o, g in zip(outs, gsel)).backward()
    assert launches.count(fwd) == steps and launches.count(bwd) == steps, launches
    what = "%s %s %d" % (kind, rnn_type, out_dim)
    used = {}
    for i, (a, b, r64, r32) in enumerate(zip(inf, outs, o64, o32)):
        assert torch.equal(a, b.detach())
        used["out %d" % i] = G.dense_share("%s out %d" % (what, i), b.cpu(), r64, r32, 2e-6)
    checked = 0
    for name, p in model.named_parameters():
        if name in g64:
            used["d" + name] = G.dense_share("%s d%s" % (what, name), p.grad.cpu(), g64[name], g32[name], 1e-5)
            checked += 1
    assert checked >= (20 if kind != "CGCN" else 10), checked
    G.record_parity("model_%s_%s_%d" % (kind, rnn_type, out_dim), used)
    assert max(used.values()) <= 1.0, used


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
def test_a_training_step_repeated_under_one_seed_is_bit_identical(rnn_type):
    w = window()
    xd = [v.to(DEV) for v in w["x"]]
    runs = []
    for _ in range(2):
        model = build("C", 64, rnn_type, seed=21)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        out = model(xd, w["adj"])
        out.square().mean().backward()
        opt.step()
        runs.append([out.detach().clone()] + [p.grad.clone() for p in model.parameters() if p.grad is not None]
                    + [p.detach().clone() for p in model.parameters()])
    assert len(runs[0]) == len(runs[1]) and all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("rnn_type", ["GRU", "LSTM"])
def test_gcrn_at_width_64_runs_inference_and_a_training_step_on_the_cell_passes(rnn_type, launches):
    import ctgcn_amd
    n, T = 50, 3
    gen = torch.Generator().manual_seed(17)
    adj = []
    for _ in range(T):
        a = (torch.rand(n, n, generator=gen) < 0.1).float()
        a = ((a + a.t()) > 0).float() + torch.eye(n)
        adj.append((a / a.sum(1, keepdim=True)).to_sparse().to(DEV))
    x = [torch.randn(n, 12, generator=gen).to(DEV) for _ in range(T)]
    torch.manual_seed(2)
    model = ctgcn_amd.GCRN(12, 0, 24, 64, duration=T, rnn_type=rnn_type).to(DEV)
    fwd, bwd = CELL[rnn_type]
    with torch.no_grad():
        out = model.eval()(x, adj)
    assert tuple(out.shape) == (T, n, 64) and bool(torch.isfinite(out).all())
    assert launches.count(fwd) == T and not (ALL_CELLS - {fwd}) & set(launches), launches
    del launches[:]
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()(x, adj).square().mean().backward()
    opt.step()
    assert launches.count(fwd) == T and launches.count(bwd) == T, launches
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.rnn.parameters())
