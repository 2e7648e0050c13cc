"""ctgcn_amd.baseline.GIN and SAGE on the GPU against the reference's recorded float64 results (tests/golden/gin_sage_uci.npz): outputs,
parameter gradients, the losses of 3 Adam steps and the BatchNorm running buffers for every fixture case, once more with the rows of
up to 199 entries cut into pieces; GIN sum / average with learn_eps (which the reference cannot run) against the float64 mirror; eval
mode; the dropout paths against the mirror fed the masks the host model regenerates from the run's base key; a list of snapshots
against the snapshots one by one.

Tolerance per tensor (tests/test_gpu_gat.py's rule): 4 x the reference's own float32-vs-float64 error (stored per tensor, over the
tensor's largest magnitude), with a floor of 2e-6 max|ref| for outputs, losses and buffers and 1e-5 max|ref| for gradients; the 3
losses are held like an output tensor of 3 entries.  A gradient the reference has as exactly zero (eps without learn_eps) must be
exactly zero here."""
import numpy as np
import pytest
import torch

import _egcn_ref as E
import _gcrn_ref as R
import _gin_sage_ref as G
from conftest import seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_runs = {}
_adj = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def prebuilt_adjacency(long_threshold=None):
    from ctgcn_amd import ops
    if long_threshold not in _adj:
        _adj[long_threshold] = [ops.GcnAdj.from_scipy(G.raw_csr(t, np.float32), DEV, long_threshold=long_threshold) for t in range(G.T)]
    return _adj[long_threshold]


def build(case, dropout=0.0, seed=None):
    import ctgcn_amd
    model = G.build(case, ctgcn_amd.GIN, ctgcn_amd.SAGE, dropout=dropout)
    seeded_parameters(model, int(G.fixture()["seed"]) if seed is None else seed)
    return model.to(DEV).train()


def gpu_run(case, long_threshold=None):
    if (case, long_threshold) not in _runs:
        model = build(case)
        x, adj = G.features(case, device=DEV), prebuilt_adjacency(long_threshold)
        losses, (outs, grads) = G.adam_losses(model, lambda: model(x, adj), G.surrogate_weights(device=DEV))
        _runs[case, long_threshold] = (losses, [o.cpu() for o in outs], {k: v.cpu() for k, v in grads.items()},
                                       {k: v.cpu() for k, v in G.buffers(model).items()})
    return _runs[case, long_threshold]


def share(what, got, ref, top, yard, floor):
    """the share of max(4 x yard, floor) that the largest error over the tensor's largest magnitude uses; printed, asserted by the caller"""
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if top == 0.0:
        print("  [tol] %-46s the reference is exactly zero; largest |got| %.3e" % (what, float(np.abs(got).max(initial=0.0))))
        return 0.0 if not got.any() else float("inf")
    err = float(np.abs(got - ref).max(initial=0.0) / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (what, err, used, float(yard), floor))
    return used


def measure(g, key, got, yard, floor):
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    return share(key, got if pick is None else got[pick], ref, top, yard, floor)


@pytest.mark.parametrize("long_threshold", [None, 16], ids=["rows", "pieces"])
@pytest.mark.parametrize("case", G.CASES)
def test_outputs_gradients_losses_and_buffers_match_the_reference(case, long_threshold):
    """long_threshold 16: UCI's rows of up to 198 entries go through up to four pieces of 64 entries.  That second run is held to the
    reference on everything the first step computes (outputs, gradients, the first loss) and on the buffers, but not on the two later
    losses: Adam's first step is lr g / (|g| + 1e-8), close to lr sign(g), so an entry of a gradient that lies below fp32's resolution
    of its sum takes its sign from the order of summation and moves its weight by +lr or -lr.  sage_average has one such entry
    (linear.weight, 4.5e-7 in rows and -2.2e-7 in pieces beside a largest entry of 17), which moves the third loss by 1e-5 of its
    value; the run in rows, whose order is the one the fixture's case describes, is held on all three."""
    g = G.fixture()
    adj = prebuilt_adjacency(long_threshold)
    if long_threshold:
        assert all(a.long_rows is not None for a in adj) and max(a.pieces for a in adj) == 4
    losses, outs, grads, bufs = gpu_run(case, long_threshold)
    used = {}
    for t in range(G.T):
        used["out_t%d" % t] = measure(g, "%s_out_t%d" % (case, t), outs[t], g[case + "_yard_out"][t], 2e-6)
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        used["grad_" + str(k)] = measure(g, "%s_grad_%s" % (case, k), grads[str(k)], yard, 1e-5)
    steps = 1 if long_threshold else len(losses)
    used["losses"] = share(case + "_losses", losses[:steps], g[case + "_losses"][:steps], float(np.abs(g[case + "_losses"]).max()),
                           g[case + "_yard_losses"], 2e-6)
    assert sorted(bufs) == [str(k) for k in g[case + "_buffer_keys"]]
    for k, yard in zip(g[case + "_buffer_keys"], g[case + "_yard_buffer"]):
        ref = g["%s_buffer_%s" % (case, k)]
        used["buffer_" + str(k)] = share("%s_buffer_%s" % (case, k), bufs[str(k)].double().numpy(), ref, float(np.abs(ref).max()), yard, 2e-6)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", G.EPS_CASES)
def test_learnt_eps_with_sum_and_average_matches_the_float64_mirror(case):
    """the reference raises UnboundLocalError here; the float32 mirror's error against the float64 mirror is the yardstick"""
    seed = int(G.fixture()["seed"])
    runs = {}
    for dtype in (torch.float64, torch.float32):
        mirror = G.build(case, G.GinMirror, G.SageMirror)
        seeded_parameters(mirror, seed)
        mirror = mirror.to(dtype).train()
        x, adj = G.features(case, dtype), G.adjacency(dtype)
        runs[dtype] = G.adam_losses(mirror, lambda: mirror(x, adj), G.surrogate_weights(dtype))
    (losses64, (outs64, grads64)), (losses32, (outs32, grads32)) = runs[torch.float64], runs[torch.float32]
    losses, outs, grads, _ = gpu_run(case)
    used = {}
    for t in range(G.T):
        top = float(outs64[t].abs().max())
        used["out_t%d" % t] = share("%s out t%d" % (case, t), outs[t], outs64[t], top, float((outs32[t].double() - outs64[t]).abs().max()) / top, 2e-6)
    for k in sorted(grads64):
        top = float(grads64[k].abs().max())
        assert top > 0 or k != "eps"
        yard = float((grads32[k].double() - grads64[k]).abs().max()) / top if top else 0.0
        used["grad_" + k] = share("%s grad %s" % (case, k), grads[k], grads64[k], top, yard, 1e-5)
    top = max(abs(v) for v in losses64)
    used["losses"] = share(case + " losses", losses, losses64, top, max(abs(a - c) for a, c in zip(losses32, losses64)) / top, 2e-6)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", ["gin_sum", "gin_max_eps", "gin_sum_mlp1", "sage_sum", "sage_max", "sage_sum_gcn"])
def test_state_dicts_move_between_the_module_and_the_mirror_and_eval_mode_uses_the_running_statistics(case):
    g = G.fixture()
    model = build(case, dropout=0.5)
    assert sorted(model.state_dict()) == [str(k) for k in g[case + "_state_keys"]]
    x, adj = G.features(case, device=DEV), prebuilt_adjacency()
    with torch.no_grad():
        torch.manual_seed(5)
        model(x, adj)                                            # one training-mode forward: the running buffers move
    mirror = G.build(case, G.GinMirror, G.SageMirror, dropout=0.5).to(DEV)
    mirror.load_state_dict(model.state_dict())
    other = build(case, dropout=0.0, seed=99)
    other.load_state_dict(mirror.state_dict())
    model.eval(), mirror.eval(), other.eval()
    with torch.no_grad():
        state = torch.random.get_rng_state()
        got = model(x, adj)
        assert torch.equal(state, torch.random.get_rng_state())   # no key is drawn in eval mode
        want = mirror(x, G.adjacency(device=DEV))
        same = other(x, adj)
    buffers = G.buffers(model)
    assert all(torch.equal(v, G.buffers(other)[k]) for k, v in buffers.items())            # eval mode leaves them alone
    if buffers:
        assert all(int(v) == G.T for k, v in buffers.items() if k.endswith("num_batches_tracked"))
    over = {}
    for t in range(G.T):
        assert torch.equal(got[t], same[t])                       # dropout is ignored; the checkpoint carries everything
        top = float(want[t].abs().max())
        used = share("%s eval t%d vs mirror" % (case, t), got[t].cpu(), want[t].cpu(), top, g[case + "_yard_out"][t], 2e-6)
        over.update({t: round(used, 3)} if not used <= 1.0 else {})
    assert not over, over


def keep_masks(case, base, p):
    """the masks of a training-mode forward under the base key `base`, as the mirrors take them"""
    kind, _, kwargs = G.spec(case)
    if kind == "SAGE":
        return [torch.from_numpy(R.keep_mask(base + t, G.N, G.HID, p)) for t in range(G.T)]
    return [[torch.from_numpy(R.keep_mask(base + 4096 * t + l, G.N, G.HID, p)) for l in range(kwargs["layer_num"] - 1)] for t in range(G.T)]


@pytest.mark.parametrize("case", ["gin_sum", "gin_max", "sage_sum", "sage_max"])
def test_training_mode_dropout_is_reproducible_and_differentiates_like_the_mirror(case):
    """dropout 0.5 in train() mode: bit-identical under the same torch seed, different under another; outputs and gradients match the
    float64 mirror fed the masks the host model gives for base + 4096 t + l (GIN) and base + t (SAGE), under the fixture cases' rule"""
    g = G.fixture()
    model = build(case, dropout=0.5)
    start = {k: v.clone() for k, v in model.state_dict().items()}
    x, adj = G.features(case, device=DEV), prebuilt_adjacency()
    weights = G.surrogate_weights(device=DEV)

    def run(seed):
        model.load_state_dict(start)
        model.zero_grad()
        torch.manual_seed(seed)
        outs = list(model(x, adj))
        E.surrogate(outs, weights).backward()
        return [o.detach().clone() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    outs, grads = run(77)
    outs2, grads2 = run(77)
    assert all(torch.equal(a, c) for a, c in zip(outs, outs2)) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    outs3, _ = run(78)
    assert not any(torch.equal(a, c) for a, c in zip(outs, outs3))
    torch.manual_seed(77)
    base = int(torch.randint(0, 2 ** 62, (1,)))
    keep = keep_masks(case, base, 0.5)
    mirror = G.build(case, G.GinMirror, G.SageMirror, dropout=0.5).double().train()
    mirror.load_state_dict({k: v.cpu().double() if v.is_floating_point() else v.cpu() for k, v in start.items()})
    want = list(mirror(G.features(case, torch.float64), G.adjacency(torch.float64), keep))
    E.surrogate(want, G.surrogate_weights(torch.float64)).backward()
    over = {}
    for t in range(G.T):
        used = share("%s dropout out t%d" % (case, t), outs[t].cpu(), want[t].detach(), float(want[t].detach().abs().max()),
                     g[case + "_yard_out"][t], 2e-6)
        over.update({"out_t%d" % t: round(used, 3)} if not used <= 1.0 else {})
    for (k, p), yard in zip(sorted(mirror.named_parameters()), g[case + "_yard_grad"]):
        if p.grad is None:
            assert k not in grads or not grads[k].any()
            continue
        used = share("%s dropout grad %s" % (case, k), grads[k].cpu(), p.grad, float(p.grad.abs().max()), yard, 1e-5)
        over.update({k: round(used, 3)} if not used <= 1.0 else {})
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", ["gin_average", "sage_average"])
def test_a_list_of_snapshots_equals_the_snapshots_one_by_one(case):
    """each snapshot is its own BatchNorm batch and the running buffers are carried in order; also with the loader-style sparse tensors"""
    x = G.features(case, device=DEV)
    adj = prebuilt_adjacency()
    tensors = G.adjacency(device=DEV)
    together, single, sparse = build(case), build(case), build(case)
    with torch.no_grad():
        outs = together(x, adj)
        ones = [single(x[t], adj[t]) for t in range(G.T)]
        loaded = sparse(x, tensors)
    for t in range(G.T):
        assert torch.equal(outs[t], ones[t]) and torch.equal(outs[t], loaded[t])
    for k, v in G.buffers(together).items():
        assert torch.equal(v, G.buffers(single)[k]) and torch.equal(v, G.buffers(sparse)[k])
        assert not k.endswith("num_batches_tracked") or int(v) == G.T
