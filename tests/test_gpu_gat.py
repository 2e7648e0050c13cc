"""ctgcn_amd.baseline.GAT on the GPU against the reference's recorded float64 results (tests/golden/gat_uci.npz): outputs, parameter
gradients and the losses of 3 Adam steps for every fixture case, once more with the rows of up to 199 entries cut into pieces, then
the dropout paths, which the reference cannot pin (its masks come from torch's generator), against the stock-torch mirror fed the
masks the host models regenerate from the run's base key.

Tolerance per tensor (tests/test_gpu_gcrn.py's rule): 4 x the reference's own float32-vs-float64 error (stored per tensor, over the
tensor's largest magnitude), with a floor of 2e-6 max|ref| for outputs and 1e-5 max|ref| for gradients; the 3 losses are held like an
output tensor of 3 entries."""
import os

import numpy as np
import pytest
import torch

import _egcn_ref as E
import _gat_ref as A
import _gcrn_ref as R
from conftest import check_close, load_golden, seeded_parameters

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
        _adj[long_threshold] = [ops.GcnAdj.from_scipy(R.row_normalized_csr(t, np.float32), DEV, long_threshold=long_threshold) for t in range(A.T)]
    return _adj[long_threshold]


def build(case, dropout=0.0, seed=None):
    import ctgcn_amd
    model = A.build(case, ctgcn_amd.GAT, dropout=dropout)
    seeded_parameters(model, int(A.fixture()["seed"]) if seed is None else seed)
    return model.to(DEV).train()


def gpu_run(case, long_threshold=None):
    if (case, long_threshold) not in _runs:
        model = build(case)
        x, adj = A.features(case, device=DEV), prebuilt_adjacency(long_threshold)
        losses, (outs, grads) = A.adam_losses(model, lambda: model(x, adj), A.surrogate_weights(case, device=DEV))
        _runs[case, long_threshold] = (losses, [o.cpu() for o in outs], {k: v.cpu() for k, v in grads.items()})
    return _runs[case, long_threshold]


def measure(g, key, got, yard, floor):
    """(largest error over the tensor's largest magnitude, the share of the tolerance it uses); printed, asserted by the caller"""
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    err = float(np.abs((got if pick is None else got[pick]) - ref).max() / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (key, err, used, float(yard), floor))
    return err, used


@pytest.mark.parametrize("long_threshold", [None, 16], ids=["rows", "pieces"])
@pytest.mark.parametrize("case", A.CASES)
def test_outputs_gradients_and_losses_match_the_reference(case, long_threshold):
    """long_threshold 16: UCI's rows of up to 199 entries go through up to four pieces of 64 entries."""
    g = A.fixture()
    adj = prebuilt_adjacency(long_threshold)
    if long_threshold:
        assert all(a.long_rows is not None for a in adj) and max(a.pieces for a in adj) == 4
    losses, outs, grads = gpu_run(case, long_threshold)
    seen, used = {}, {}
    for t in range(A.T):
        seen["out_t%d" % t], used["out_t%d" % t] = measure(g, "%s_out_t%d" % (case, t), outs[t], g[case + "_yard_out"][t], 2e-6)
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        seen["grad_" + str(k)], used["grad_" + str(k)] = measure(g, "%s_grad_%s" % (case, k), grads[str(k)], yard, 1e-5)
    scale = float(np.abs(g[case + "_losses"]).max())
    seen["losses"] = float(np.abs(np.asarray(losses) - g[case + "_losses"]).max() / scale)
    used["losses"] = seen["losses"] / max(4 * float(g[case + "_yard_losses"]), 2e-6)
    print("  [observed] %s: outputs %.3e, gradients %.3e (worst %s), losses %.3e" % (
        case, max(v for k, v in seen.items() if k.startswith("out")), max(v for k, v in seen.items() if k.startswith("grad")),
        max((k for k in seen if k.startswith("grad")), key=seen.get), seen["losses"]))
    out_dir = os.environ.get("CTGCN_PARITY_OUT")             # a measuring run keeps the observed errors
    if out_dir and not long_threshold:
        import json
        with open(os.path.join(out_dir, "gat_parity_%s.json" % case), "w") as fp:
            json.dump(seen, fp, indent=1, sort_keys=True)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", ["gat_uneg", "gat_dense"])
def test_eval_mode_ignores_dropout(case):
    x, adj = A.features(case, device=DEV), prebuilt_adjacency()
    dropping, plain = build(case, dropout=0.5).eval(), build(case, dropout=0.0).eval()
    with torch.no_grad():
        state = torch.random.get_rng_state()
        got = dropping(x, adj)
        assert torch.equal(state, torch.random.get_rng_state())          # no key is drawn
        want = plain(x, adj)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", ["gat_uneg", "gat_cfg"])
def test_training_mode_dropout_is_reproducible_and_differentiates_like_the_mirror(case):
    """dropout 0.5 in train() mode: bit-identical under the same torch seed; outputs and gradients match the float64 mirror fed the
    masks the host models give for base + 4096 t + 2048 l + h (attention) and base + 2^40 + t (features), under the fixture cases'
    tolerance rule.  Identity features: a dense input would first pass through stock F.dropout."""
    g = A.fixture()
    model = build(case, dropout=0.5)
    x, adj = A.features(case, device=DEV), prebuilt_adjacency()
    weights = A.surrogate_weights(case, device=DEV)

    def run():
        model.zero_grad()
        torch.manual_seed(77)
        outs = list(model(x, adj))
        E.surrogate(outs, weights).backward()
        return [o.detach().clone() for o in outs], {k: p.grad.detach().clone() for k, p in model.named_parameters()}

    outs, grads = run()
    outs2, grads2 = run()
    assert all(torch.equal(a, b) for a, b in zip(outs, outs2)) and all(torch.equal(grads[k], grads2[k]) for k in grads)
    torch.manual_seed(77)
    base = int(torch.randint(0, 2 ** 62, (1,)))
    _, heads, hid, _, _ = A.CASES[case]
    x64, adj64 = A.features(case, torch.float64), A.adjacency(torch.float64)
    keep = []
    for t in range(A.T):
        rows, cols = A.entries(adj64[t])
        keep.append(A.model_keep(base, t, rows.numpy(), cols.numpy(), heads, hid, 0.5))
        assert 0.45 < float(keep[t]["att0"].double().mean()) < 0.55 and 0.45 < float(keep[t]["feat"].double().mean()) < 0.55
    mirror = A.build(case, A.GatMirror, dropout=0.5).double()
    mirror.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
    want = list(mirror(x64, adj64, keep))
    E.surrogate(want, A.surrogate_weights(case, torch.float64)).backward()
    over = {}
    for t in range(A.T):
        top = float(want[t].detach().abs().max())
        err = float((outs[t].cpu().double() - want[t].detach()).abs().max()) / top
        used = err / max(4 * float(g[case + "_yard_out"][t]), 2e-6)
        print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of the tolerance" % ("%s dropout out t%d" % (case, t), err, used))
        over.update({"out_t%d" % t: round(used, 3)} if not used <= 1.0 else {})
    for (k, p), yard in zip(sorted(mirror.named_parameters()), g[case + "_yard_grad"]):
        err = float((grads[k].cpu().double() - p.grad).abs().max()) / float(p.grad.abs().max())
        used = err / max(4 * float(yard), 1e-5)
        print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of the tolerance" % ("%s dropout grad %s" % (case, k), err, used))
        over.update({k: round(used, 3)} if not used <= 1.0 else {})
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", A.CASES)
def test_state_dicts_move_between_the_module_and_the_mirror(case):
    g = A.fixture()
    model = build(case)
    mirror = A.build(case, A.GatMirror).to(DEV)
    mirror.load_state_dict(model.state_dict())
    x = A.features(case, device=DEV)
    with torch.no_grad():
        want = list(mirror(x, A.adjacency(device=DEV)))
        other = build(case, seed=99)
        other.load_state_dict(mirror.state_dict())
        got = list(other(x, prebuilt_adjacency()))
    for t in range(A.T):
        top = float(want[t].abs().max())
        check_close(got[t].cpu().numpy(), want[t].cpu().numpy(), 0.0, max(4 * float(g[case + "_yard_out"][t]), 2e-6) * top, "%s t%d vs mirror" % (case, t))


def _edge_files(folder):
    snaps = load_golden("uci_snapshots.npz")
    names = [str(s) for s in snaps["node_names"]]
    for t in range(A.T):
        with open(os.path.join(folder, "%d.csv" % t), "w") as fp:
            fp.write("from_id\tto_id\tweight\n")
            for s, o, w in zip(snaps["t%d_src" % t], snaps["t%d_dst" % t], snaps["t%d_w" % t]):
                fp.write("%s\t%s\t%s\n" % (names[s], names[o], repr(float(w))))
    return names


def test_reference_shaped_call_with_the_loader_s_sparse_tensors(tmp_path):
    from ctgcn_amd import DataLoader, SpGraphAttentionLayer
    names = _edge_files(str(tmp_path))
    loader = DataLoader(names, A.T, has_cuda=True)
    tensors = loader.get_date_adj_list(str(tmp_path), 0, A.T, normalize=True, row_norm=True, add_eye=True)
    adj = prebuilt_adjacency()
    for case in ("gat_uneg", "gat_dense"):
        model = build(case)
        x = A.features(case, device=DEV)
        with torch.no_grad():
            for got, want in zip(model(x, tensors), model(x, adj)):
                assert torch.equal(got, want)
            assert torch.equal(model(x[0], tensors[0]), model(x, tensors)[0])           # a single snapshot, as the reference's forward takes
    # one head on its own, as the reference's layer is called
    layer = SpGraphAttentionLayer(A.DENSE_IN, 8, 0.5, 0.2).to(DEV).eval()
    with torch.no_grad():
        assert torch.equal(layer(x[0], tensors[0]), layer(x[0], adj[0])) and tuple(layer(x[0], adj[0]).shape) == (A.N, 8)
