"""ctgcn_amd.baseline.VGRNN and ops.vae_nll on the GPU.

ops.vae_nll (the decoder loss without an [N, N] matrix) against the float64 mirror (tests/_vgrnn_ref.py) at every size at which the
dense kernel takes another path: N around its 32-row / 32-column tile (1, 31, 32, 33, 67: partial tiles, more than one wave, more
than one block needs 129), d around its accumulator widths (1, 3, 16, 128, 130: scalar and float4 loads, 1 / 4 accumulator tiles, the
chunked launch above 128).  The project has no yardstick for this loss, so the same dense expression in stock fp32 torch ops on the
same GPU is measured against the float64 mirror too, and the kernel may use 4 x that error (the project's margin for fp32 yardsticks)
with the fixture rule's floors: 2e-6 max|ref| for the loss, 1e-5 max|ref| for the gradient.

The model against the reference's recorded float64 results (tests/golden/vgrnn_uci.npz) by tests/test_gpu_gat.py's rule: error <=
max(4 x the stored yardstick, 2e-6) max|ref| for outputs and losses, 1e-5 for gradients."""
import os

import numpy as np
import pytest
import torch

import _vgrnn_ref as V
from conftest import seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TILE = 32
_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def make_case(n, d, seed=0, scale=1.0, empty_from=None):
    """z float32 [n, d] and a weighted, asymmetric target with duplicates summed, stored diagonal entries and rows without entries
    (every row from empty_from on, default the last third)"""
    gen = torch.Generator().manual_seed(1000 * n + d + seed)
    z = (torch.randn(n, d, generator=gen) * scale / np.sqrt(d)).float()
    top = max(1, (2 * n) // 3 if empty_from is None else empty_from)
    e = 3 * n
    rows, cols = torch.randint(0, top, (e,), generator=gen), torch.randint(0, n, (e,), generator=gen)
    k = min(4, top)
    rows, cols = torch.cat([rows, torch.arange(k)]), torch.cat([cols, torch.arange(k)])
    w = torch.rand(rows.numel(), generator=gen) * 0.5 + 0.25
    if n == 1:
        rows, cols, w = rows[:1], cols[:1], w[:1]                # S must stay below n² = 1
    return z, torch.sparse_coo_tensor(torch.stack((rows, cols)), w, (n, n)).coalesce()


def reference(z, target, dtype, device):
    """(loss, dZ) of the reference's dense expression in `dtype` on `device`"""
    zz = z.to(device=device, dtype=dtype).requires_grad_(True)
    loss = V.dense_nll(zz @ zz.t(), target.to_dense().to(device=device, dtype=dtype))
    grad, = torch.autograd.grad(loss, zz)
    return float(loss), grad.detach().double().cpu()


def kernel(z, target, long_threshold=None, view=False):
    from ctgcn_amd import ops
    adj = ops.GcnAdj.from_sparse_tensor(target, DEV, long_threshold=long_threshold, check_symmetric=False)
    if view:                                                     # rows of a wider buffer: a row stride above d
        zz = torch.zeros(z.shape[0], z.shape[1] + 5, device=DEV)[:, 2:2 + z.shape[1]]
        zz.copy_(z)
        zz = zz.detach().requires_grad_(True)
    else:
        zz = z.to(DEV).requires_grad_(True)
    loss = ops.vae_nll(zz, adj)
    grad, = torch.autograd.grad(loss, zz)
    return loss.detach(), grad.detach(), adj


def held(what, got_loss, got_grad, z, target):
    """the kernel's loss and gradient against the float64 mirror, next to stock fp32 torch on the same GPU"""
    ref_loss, ref_grad = reference(z, target, torch.float64, "cpu")
    dec = V.decomposed_nll(z.double(), target.double())
    assert abs(float(dec) - ref_loss) <= 1e-12 * abs(ref_loss)
    yard_loss, yard_grad = reference(z, target, torch.float32, DEV)
    top = float(ref_grad.abs().max())
    err_l, yl = abs(float(got_loss) - ref_loss) / abs(ref_loss), abs(yard_loss - ref_loss) / abs(ref_loss)
    print("  [tol] %-40s loss     kernel %.3e  stock fp32 %.3e  allowed %.3e" % (what, err_l, yl, max(4 * yl, 2e-6)))
    if top == 0.0:
        err_g, yg = float(got_grad.abs().max()), 0.0
        print("  [tol] %-40s gradient is zero: kernel max %.3e" % (what, err_g))
        assert err_g == 0.0
    else:
        err_g = float((got_grad.double().cpu() - ref_grad).abs().max()) / top
        yg = float((yard_grad - ref_grad).abs().max()) / top
        print("  [tol] %-40s gradient kernel %.3e  stock fp32 %.3e  allowed %.3e" % (what, err_g, yg, max(4 * yg, 1e-5)))
        assert err_g <= max(4 * yg, 1e-5), (what, err_g, yg)
    assert err_l <= max(4 * yl, 2e-6), (what, err_l, yl)
    out_dir = os.environ.get("CTGCN_PARITY_OUT")                 # a measuring run keeps the observed errors
    if out_dir:
        import json
        with open(os.path.join(out_dir, "vgrnn_nll_%s.json" % what.replace(" ", "_")), "w") as fp:
            json.dump({"loss": err_l, "loss_stock_fp32": yl, "grad": err_g, "grad_stock_fp32": yg}, fp)


@pytest.mark.parametrize("d", [1, 3, 16, 128, 130])
@pytest.mark.parametrize("n", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 3])
def test_vae_nll_loss_and_gradient_at_the_tile_boundaries(n, d):
    from ctgcn_amd import _lib
    assert _lib.load().ctgcn_vae_nll_tile() == TILE
    z, target = make_case(n, d)
    loss, grad, _ = kernel(z, target)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and tuple(grad.shape) == (n, d)
    held("n%d d%d" % (n, d), loss, grad, z, target)


def test_vae_nll_more_than_one_block_of_row_tiles():
    z, target = make_case(4 * TILE + 5, 20)                      # five row tiles: two blocks of four waves
    loss, grad, _ = kernel(z, target)
    held("n133 d20", loss, grad, z, target)


@pytest.mark.parametrize("case", ["large", "zero"])
def test_vae_nll_extreme_logits(case):
    """logits beyond +-90 (softplus and the sigmoids saturate), and z = 0 (every logit 0, a zero gradient)"""
    z, target = make_case(TILE + 9, 16, scale=1.0)
    if case == "large":
        z = z * 40.0
        assert float((z @ z.t()).max()) > 90 and float((z @ z.t()).min()) < -90
    else:
        z = torch.zeros_like(z)
    loss, grad, _ = kernel(z, target)
    held("extreme " + case, loss, grad, z, target)


@pytest.mark.parametrize("d", [5, 16])
def test_vae_nll_long_rows_and_strided_views(d):
    """row 0 holds 40 entries: with long_threshold 4 it is cut into pieces in the gathers of both the CSR and its transpose (column 3
    is as long); z is a view with a row stride above d"""
    n = 2 * TILE + 3
    z, target = make_case(n, d, seed=7)
    extra = torch.sparse_coo_tensor(torch.stack((torch.cat([torch.zeros(40, dtype=torch.int64), torch.arange(40)]),
                                                 torch.cat([torch.arange(40), torch.full((40,), 3)]))), torch.full((80,), 0.5), (n, n))
    target = (target + extra).coalesce()
    loss, grad, adj = kernel(z, target, long_threshold=4, view=True)
    assert adj.long_rows is not None and adj.transposed().long_rows is not None
    held("long rows d%d" % d, loss, grad, z, target)
    plain_loss, plain_grad, _ = kernel(z, target)
    assert torch.equal(plain_loss, loss)                         # the loss reads no gather: the same arithmetic whatever the loads


def test_vae_nll_is_bit_identical_when_repeated_and_refuses_an_empty_adjacency():
    from ctgcn_amd import ops
    z, target = make_case(3 * TILE + 1, 128)
    a = kernel(z, target)
    b = kernel(z, target)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    with torch.no_grad():                                        # the loss alone: no gradient pass, the same number
        assert torch.equal(ops.vae_nll(z.to(DEV), a[2]), a[0])
    empty = ops.GcnAdj(torch.zeros(6, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                       torch.zeros(0, device=DEV))
    with pytest.raises(ValueError, match="sum to 0"):
        ops.vae_nll(torch.zeros(5, 4, device=DEV), empty)
    with pytest.raises(TypeError):
        ops.vae_nll(z.double().to(DEV), a[2])


# ------------------------------------------------------------------------------------------------ the model
def build(seed=None, layers=1, **kw):
    import ctgcn_amd
    model = V.build(ctgcn_amd.VGRNN, layers, **kw)
    seeded_parameters(model, int(V.fixture()["seed"]) if seed is None else seed)
    return model.to(DEV).train()


def window(long_threshold=None):
    from ctgcn_amd import ops
    from ctgcn_amd.baseline import gcn_conv_adjacency
    key = ("window", long_threshold)
    if key not in _runs:
        edges = V.edge_lists(DEV)
        adj = V.target_adjacency(device=DEV)
        if long_threshold:
            edges = [gcn_conv_adjacency(e, V.N, long_threshold=long_threshold) for e in edges]
            adj = [ops.GcnAdj.from_sparse_tensor(a, DEV, long_threshold=long_threshold, check_symmetric=False) for a in adj]
        _runs[key] = (V.identity_features(device=DEV), edges, adj, V.noise(device=DEV))
    return _runs[key]


def gpu_run(long_threshold=None, fused=True):
    from ctgcn_amd import VAELoss
    key = ("run", long_threshold, fused)
    if key not in _runs:
        model = build(fused=fused)
        x, edges, adj, noise = window(long_threshold)
        loss_fn = VAELoss()

        def forward_loss():
            emb, h, data = model(x, edges, None, noise)
            return emb, h, loss_fn(data + [adj])

        losses, (outs, h, grads) = V.adam_run(model, forward_loss)
        _runs[key] = (losses, [o.cpu() for o in outs], h.cpu(), {k: v.cpu() for k, v in grads.items()})
    return _runs[key]


def measure(g, key, got, yard, floor):
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    err = float(np.abs((got if pick is None else got[pick]) - ref).max() / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (key, err, used, float(yard), floor))
    return used


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("long_threshold", [None, 16], ids=["rows", "pieces"])
def test_outputs_gradients_and_losses_match_the_reference(long_threshold, fused):
    g = V.fixture()
    if long_threshold:
        assert all(a.long_rows is not None for a in window(long_threshold)[1])
    losses, outs, h, grads = gpu_run(long_threshold, fused)
    used = {}
    for t in range(V.T):
        used["out_t%d" % t] = measure(g, "out_t%d" % t, outs[t], g["yard_out"][t], 2e-6)
    used["h"] = measure(g, "h", h, g["yard_h"], 2e-6)
    for k, yard in zip(g["keys"], g["yard_grad"]):
        used["grad_" + str(k)] = measure(g, "grad_%s" % k, grads[str(k)], yard, 1e-5)
    err = float(np.abs(np.asarray(losses) - g["losses"]).max() / np.abs(g["losses"]).max())
    used["losses"] = err / max(4 * float(g["yard_losses"]), 2e-6)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of the tolerance" % ("losses", err, used["losses"]))
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "share of the tolerance used %s" % over


def test_a_training_step_is_bit_identical_when_run_twice_and_draws_from_torch_s_generator():
    from ctgcn_amd import VAELoss
    model = build()
    x, edges, adj, _ = window()

    def step():
        model.zero_grad()
        torch.manual_seed(77)
        emb, h, data = model(x, edges)
        loss = VAELoss()(data + [adj])
        loss.backward()
        return [e.detach().clone() for e in emb], h.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters()}

    a, b = step(), step()
    assert all(torch.equal(u, v) for u, v in zip(a[0], b[0])) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]) and all(float(v.abs().max()) > 0 for v in a[3].values())
    torch.manual_seed(77)                                          # noise_list overrides the draw: the same numbers handed in
    noise = [torch.randn(V.N, V.OUT, device=DEV) for _ in range(V.T)]
    emb, h, _ = model(x, edges, None, noise)
    assert all(torch.equal(u, v) for u, v in zip(a[0], emb)) and torch.equal(a[1], h)


def test_state_dicts_move_between_the_module_and_the_mirror_and_two_layers_match_it():
    g = V.fixture()
    x, edges, adj, noise = window()
    for layers in (1, 2):
        model = build(layers=layers)
        mirror = V.build(V.VgrnnMirror, layers).double()
        mirror.load_state_dict({k: v.detach().cpu().double() for k, v in model.state_dict().items()})
        x64, noise64 = V.identity_features(torch.float64), V.noise(torch.float64)
        with torch.no_grad():
            want, want_h, _ = mirror(x64, V.edge_lists(), None, noise64)
            other = build(seed=99, layers=layers)
            other.load_state_dict({k: v.float() for k, v in mirror.state_dict().items()})
            hx = torch.zeros(layers, V.N, V.HID, device=DEV)
            got, got_h, _ = other(x, edges, hx, noise)             # a given hx of zeros is the default start
        for t in range(V.T):
            top = float(want[t].abs().max())
            err = float((got[t].cpu().double() - want[t]).abs().max()) / top
            print("  [tol] %d layer(s) out t%d |err| / max|ref| %.3e" % (layers, t, err))
            assert err <= max(4 * float(g["yard_out"][t]), 2e-6)
        assert float((got_h.cpu().double() - want_h).abs().max()) / float(want_h.abs().max()) <= max(4 * float(g["yard_h"]), 2e-6)


def test_stacked_dense_features_and_single_calls_of_the_layers():
    from ctgcn_amd import GCNConv, graph_gru_gcn
    from ctgcn_amd.baseline import gcn_conv_adjacency
    x, edges, _, noise = window()
    model = build()
    with torch.no_grad():
        want, want_h, _ = model(x, edges, None, noise)
        dense = torch.stack([torch.eye(V.N, device=DEV) for _ in range(V.T)])
        got, got_h, _ = model(dense, edges, None, noise)           # a stacked dense tensor goes through the Linear
        for a, b in zip(got, want):
            assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())
        conv = GCNConv(V.HID, 8, bias=True).to(DEV)
        s = torch.randn(V.N, V.HID, device=DEV)
        adj = gcn_conv_adjacency(edges[0], V.N)
        ref = torch.relu(torch.sparse.mm(V.normalized_adjacency(edges[0], V.N, torch.float32), s @ conv.weight) + conv.bias)
        assert float((conv(s, edges[0]) - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
        assert torch.equal(conv(s, edges[0]), conv(s, adj))        # the index tensor and its prepared adjacency
        rnn = graph_gru_gcn(2 * V.HID, V.HID, 1).to(DEV)
        h0 = torch.randn(1, V.N, V.HID, device=DEV)
        xin = torch.randn(V.N, 2 * V.HID, device=DEV)
        out, h1 = rnn(xin, edges[0], h0)
        comp, _ = rnn(xin, edges[0], h0, fused=False)              # the two-gather cell against the six convolutions
        assert tuple(out.shape) == (1, V.N, V.HID) and float((h1 - comp).abs().max()) <= 1e-5


# ------------------------------------------------------------------------------------------------ the trainers
NAMES = ["n%d" % i for i in range(V.N)]


def _folders(tmp_path):
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t in range(V.T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _exported(folder):
    files = sorted(os.listdir(folder))
    assert len(files) == V.T
    for f in files:
        lines = open(os.path.join(folder, f)).read().strip().split("\n")[1:]              # after the header line
        assert len(lines) == V.N and all(len(line.split("\t")) == 1 + V.OUT for line in (lines[0], lines[-1]))
    return np.loadtxt(os.path.join(folder, files[-1]), delimiter="\t", skiprows=1, usecols=range(1, 1 + V.OUT))


def _same_rule(g, runs):
    """fused against composed by the fixture rule: the losses of every epoch as one tensor within max(4 x the stored yardstick, 2e-6) of
    its largest magnitude, the exported embedding within max(4 x the largest stored output yardstick, 2e-6) of its largest magnitude"""
    (la, ea), (lb, eb) = runs
    assert len(la) == len(lb)
    err_l = max(abs(u - v) for u, v in zip(la, lb)) / max(abs(v) for v in lb)
    err_e = float(np.abs(ea - eb).max() / np.abs(eb).max())
    tol_l, tol_e = max(4 * float(g["yard_losses"]), 2e-6), max(4 * float(g["yard_out"].max()), 2e-6)
    print("  [tol] fused vs composed: losses %.3e of %.3e allowed, export %.3e of %.3e allowed" % (err_l, tol_l, err_e, tol_e))
    assert err_l <= tol_l and err_e <= tol_e


def test_unsupervised_trainer_two_epochs_fused_against_composed(tmp_path):
    from ctgcn_amd import UnsupervisedEmbedding, VAELoss
    g = V.fixture()
    x, edges, adj, _ = window()
    runs = []
    for fused in (True, False):
        model = build()
        tr = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb_%d" % fused, NAMES, model, VAELoss(), has_cuda=True)
        if fused:
            with pytest.raises(ValueError, match="edge_list"):
                tr.learn_embedding(adj, x, epoch=1, export=False)
        torch.manual_seed(4321)
        sums = []
        step = torch.optim.Adam.step

        def record(self, *a, **kw):
            sums.append(tr.last_epoch_losses)
            return step(self, *a, **kw)

        torch.optim.Adam.step = record
        try:
            tr.learn_embedding(adj, x, edge_list=edges, epoch=2, batch_size=1000, lr=1e-3, model_file="m_%d.pt" % fused, fused=fused)
        finally:
            torch.optim.Adam.step = step
        history = [v for epoch in sums for v in epoch]              # the batch losses of both epochs, as each Adam step found them
        assert [len(epoch) for epoch in sums] == [2, 2] and all(np.isfinite(v) for v in history)          # ceil(1899 / 1000) batches
        assert os.path.exists(os.path.join(str(tmp_path), "model", "m_%d.pt" % fused))
        runs.append((history, _exported(os.path.join(str(tmp_path), "emb_%d" % fused))))
    _same_rule(g, runs)


def test_supervised_trainer_two_epochs_fused_against_composed(tmp_path):
    from ctgcn_amd import MLPClassifier, SupervisedEmbedding, VAEClassificationLoss
    g = V.fixture()
    x, edges, adj, _ = window()
    labels = [torch.stack((torch.arange(V.N), (torch.arange(V.N) * 7 + t) % 4), 1).to(DEV) for t in range(V.T)]
    runs = []
    for fused in (True, False):
        model = build()
        classifier = MLPClassifier(V.OUT, V.OUT, 4, 1, V.T, bias=True, activate_type="N")
        seeded_parameters(classifier, 31)
        tr = SupervisedEmbedding(_folders(tmp_path), "origin", "sup_%d" % fused, NAMES, model, VAEClassificationLoss(4), classifier, has_cuda=True)
        torch.manual_seed(4321)
        tr.learn_embedding(adj, x, node_labels=labels, edge_list=edges, learning_type="S-node", epoch=2, lr=1e-3, model_file="s_%d" % fused,
                           classifier_file="c_%d" % fused, fused=fused)
        hist = [h["loss_train"] for h in tr.history]
        assert len(hist) == 2 and all(np.isfinite(v) for v in hist) and np.isfinite(tr.test_result[0])
        runs.append((hist, _exported(os.path.join(str(tmp_path), "sup_%d" % fused))))
    _same_rule(g, runs)
