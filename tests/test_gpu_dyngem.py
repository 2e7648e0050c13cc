"""ctgcn_amd.baseline.DynGEM / DynAE and their trainer on the GPU.

The models against the reference's recorded float64 results (tests/golden/dyngem_uci.npz) by tests/test_gpu_vgrnn.py's rule: error <=
max(4 x the stored yardstick, 2e-6) max|ref| for outputs and losses, 1e-5 for gradients; the kernel path and the composed path (dense
rows and penalties in stock torch ops) are held to it separately.  CTGCN_PARITY_OUT=<dir> keeps the shares of the tolerance used."""
import json
import os

import numpy as np
import pytest
import torch

import _dyngem_ref as D
from conftest import seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def rows_of(method):
    from ctgcn_amd import ops
    if ("rows", method) not in _runs:
        _runs[("rows", method)] = ops.SnapshotRows(D.dyngem_window() if method == "dyngem" else D.dynae_window(), DEV)
    return _runs[("rows", method)]


def build(method, seed=None):
    import ctgcn_amd
    if method == "dyngem":
        model = ctgcn_amd.DynGEM(input_dim=D.N, output_dim=D.OUT, n_units=D.UNITS, bias=True)
    else:
        model = ctgcn_amd.DynAE(input_dim=D.N, output_dim=D.OUT, look_back=D.LOOK_BACK, n_units=D.UNITS, bias=True)
    seeded_parameters(model, int(D.fixture()["seed"]) if seed is None else seed)
    return model.to(DEV).train()


def fixture_batch(method):
    """the fixture's drawn batch as the generators would hand it over"""
    from ctgcn_amd.baseline.dynae import RowBatch
    from ctgcn_amd.baseline.dyngem import PairBatch
    g = D.fixture()
    rows = rows_of(method)
    if method == "dyngem":
        idx = np.concatenate((g["dyngem_i"], g["dyngem_j"])).astype(np.int64)
        return PairBatch(rows, idx, idx, D.DYNGEM["beta"], g["dyngem_w"].astype(np.float32))
    idx, tgt = D.dynae_rows(g)
    return RowBatch(rows, idx, tgt, D.DYNAE["beta"])


def loss_module(method):
    import ctgcn_amd
    if method == "dyngem":
        c = D.DYNGEM
        return ctgcn_amd.DynGEMLoss(c["alpha"], c["beta"], c["nu1"], c["nu2"])
    c = D.DYNAE
    return ctgcn_amd.DynGraph2VecLoss(c["beta"], c["nu1"], c["nu2"])


def step_fn(method, model, fused):
    """forward_loss() -> (loss, first-side embedding, first-side prediction) through the trainer's own get_model_res"""
    from ctgcn_amd import DynamicEmbedding
    loss_fn = loss_module(method)
    batch = fixture_batch(method)
    B = D.BATCH

    def forward_loss():
        res = DynamicEmbedding.get_model_res(model, iter([batch]), fused)
        if fused:
            pred = torch.relu(res[0].detach()[:B])                   # a copy, made before the loss consumes z
            hx = res[1][:B] if method == "dyngem" else None
        else:
            pred, hx = res[0], (res[6] if method == "dyngem" else None)
        if hx is None:                                               # DynAE's step does not keep the embedding
            with torch.no_grad():
                hx = model.encode(batch) if fused else model.encoder(batch.dense()[0])
        return loss_fn(model, res), hx, pred

    return forward_loss


def gpu_run(method, fused):
    if (method, fused) not in _runs:
        model = build(method)
        losses, (hx, pred, grads) = D.adam_run(model, step_fn(method, model, fused))
        _runs[(method, fused)] = (losses, hx.cpu(), pred.cpu(), {k: v.cpu() for k, v in grads.items()})
    return _runs[(method, fused)]


def measure(g, key, got, yard, floor):
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    err = float(np.abs((got if pick is None else got[pick]) - ref).max() / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (key, err, used, float(yard), floor))
    return used


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_outputs_gradients_and_losses_match_the_reference(method, fused):
    g = D.fixture()
    losses, hx, pred, grads = gpu_run(method, fused)
    used = {"hx": measure(g, method + "_hx", hx, g[method + "_yard_hx"], 2e-6),
            "pred": measure(g, method + "_pred", pred, g[method + "_yard_pred"], 2e-6)}
    for k, yard in zip(g[method + "_keys"], g[method + "_yard_grad"]):
        used["grad_" + str(k)] = measure(g, "%s_grad_%s" % (method, k), grads[str(k)], yard, 1e-5)
    ref = g[method + "_losses"]
    err = float(np.abs(np.asarray(losses) - ref).max() / np.abs(ref).max())
    used["losses"] = err / max(4 * float(g[method + "_yard_losses"]), 2e-6)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of the tolerance" % (method + " losses", err, used["losses"]))
    out_dir = os.environ.get("CTGCN_PARITY_OUT")                     # a measuring run keeps the observed errors
    if out_dir:
        with open(os.path.join(out_dir, "dyngem_%s_%s.json" % (method, "fused" if fused else "composed")), "w") as fp:
            json.dump(used, fp, indent=1, sort_keys=True)
        parts = {"%s_%s" % (m, p): os.path.join(out_dir, "dyngem_%s_%s.json" % (m, p)) for m in ("dyngem", "dynae") for p in ("fused", "composed")}
        if all(os.path.exists(f) for f in parts.values()):           # the last of the four cases: profiles/dyngem_parity_errors.json
            joined = {"rule": "share used of max(4 x the reference's own fp32-vs-fp64 error, floor) of the largest reference magnitude; "
                              "floor 2e-6 for outputs and losses, 1e-5 for gradients",
                      "fixture": "tests/golden/dyngem_uci.npz", "cases": {k: json.load(open(f)) for k, f in parts.items()}}
            with open(os.path.join(out_dir, "dyngem_parity_errors.json"), "w") as fp:
                json.dump(joined, fp, indent=1, sort_keys=True)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "share of the tolerance used %s" % over


@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_a_fused_training_step_is_bit_identical_when_run_twice(method):
    def run():
        torch.manual_seed(77)
        model = build(method)
        losses, (hx, pred, grads) = D.adam_run(model, step_fn(method, model, True))
        return losses, hx, pred, grads

    a, b = run(), run()
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]) and all(float(v.abs().max()) > 0 for v in a[3].values())


@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_predictors_and_the_dense_forward(method):
    import ctgcn_amd
    model = build(method)
    rows = rows_of(method)
    cls = ctgcn_amd.DynGEMBatchPredictor if method == "dyngem" else ctgcn_amd.BatchPredictor
    start = 0 if method == "dyngem" else rows.T - D.LOOK_BACK
    pred = cls(list(range(D.N)), 700)                                # 1899 nodes: two full batches and a remainder
    emb, x_pred = pred.predict(model, rows, start=start)
    emb_c, x_pred_c = pred.predict(model, rows, fused=False, start=start)
    only, none = pred.predict(model, rows, need_pred=False, start=start)
    assert tuple(emb.shape) == (D.N, D.OUT) and tuple(x_pred.shape) == (D.N, D.N) and none is None and torch.equal(only, emb)
    assert float((emb - emb_c).abs().max()) <= 1e-5 * float(emb_c.abs().max())
    assert float((x_pred - x_pred_c).abs().max()) <= 1e-5 * float(x_pred_c.abs().max())
    batch = fixture_batch(method)
    with torch.no_grad():
        hx, x = model(batch)                                         # a RowBatch, (SnapshotRows, idx) and the dense rows agree
        hx2, _ = model((rows, batch.host_idx))
        hx3, x3 = model(batch.dense()[0])
    assert torch.equal(hx, hx2) and float((hx - hx3).abs().max()) <= 1e-5 * float(hx3.abs().max())
    assert float((x - x3).abs().max()) <= 1e-5 * float(x3.abs().max())


# ------------------------------------------------------------------------------------------------ the trainer
NAMES = ["n%d" % i for i in range(D.N)]
TRAINER_LR = 1e-4


def _window_through_the_loader(tmp_path, mats):
    """the snapshots written as the reference's edge files (every undirected edge once) into tmp_path/origin and read back with
    DataLoader.get_date_adj_list(..., data_type='matrix'), as the reference's driver hands them to the trainer"""
    import scipy.sparse as sp
    from ctgcn_amd import DataLoader
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t, m in enumerate(mats):
        coo = sp.triu(m, k=1).tocoo()
        rows = ["%s\t%s\t%d" % (NAMES[i], NAMES[j], int(w)) for i, j, w in zip(coo.row, coo.col, coo.data)]
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("from_id\tto_id\tweight\n" + "\n".join(rows) + "\n")
    window = DataLoader(NAMES, len(mats), has_cuda=True).get_date_adj_list(str(origin), start_idx=0, duration=len(mats), data_type='matrix')
    assert all((abs(sp.csr_matrix(w) - m)).nnz == 0 for w, m in zip(window, mats))
    return window


def _generators(method, batch_size):
    import ctgcn_amd
    if method == "dyngem":
        return (ctgcn_amd.DynGEMBatchGenerator(NAMES, batch_size, D.DYNGEM["beta"], shuffle=True, has_cuda=True),
                ctgcn_amd.DynGEMBatchPredictor(NAMES, batch_size, has_cuda=True))
    return (ctgcn_amd.BatchGenerator(NAMES, batch_size, D.LOOK_BACK, D.DYNAE["beta"], shuffle=True, has_cuda=True),
            ctgcn_amd.BatchPredictor(NAMES, batch_size, has_cuda=True))


@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_dynamic_embedding_two_epochs_fused_against_composed(method, tmp_path):
    """Two epochs of the trainer on both paths under one seed, on a 3-snapshot folder read through the DataLoader.  The batch losses and
    the exported embedding of the two paths are held to each other by the fixture rule: max(4 x the stored yardstick, 2e-6) of the
    largest magnitude.

    The learning rate is 1e-4.  Adam's update lr g / (|g| + eps) has the slope lr eps / (|g| + eps)^2 in g: up to lr / eps (1e5 at lr 1e-3)
    where an accumulated gradient entry is as small as eps = 1e-8, and with the L1 / L2 terms (about 1.7e-5 per weight) some
    entry of the first layer's 91 000 cancels that far.  At lr 1e-3 one such weight of DynAE (gradient -5.84e-9 on one path, -5.90e-9 on
    the other: 1.5e-9 of the largest gradient entry apart, far inside the rule for gradients) ends 2.3e-6 apart and moves the export by
    2.0e-6 of its largest entry; the slope is proportional to lr, so at 1e-4 the same entry moves it by 1.4e-7, and what the test
    sees is the paths, not the optimiser's division by a number near its eps."""
    import ctgcn_amd
    g = D.fixture()
    mats = [D.weighted_snapshot(0)] * 3 if method == "dyngem" else D.dynae_window()
    loaded = _window_through_the_loader(tmp_path, mats)
    window = loaded[:1] if method == "dyngem" else loaded            # DynGEM trains on one snapshot
    batch_size, batches = 1024, (4 if method == "dyngem" else 2)    # 3542 entries: 4 batches; 1899 records: 2 batches
    idx = 0 if method == "dyngem" else 2                             # the snapshot the embedding belongs to
    runs = []
    for fused in (True, False):
        model = build(method)
        gen, pred = _generators(method, batch_size)
        tr = ctgcn_amd.DynamicEmbedding(str(tmp_path), "origin", "emb_%d" % fused, NAMES, model, loss_module(method), gen, pred, has_cuda=True)
        torch.manual_seed(4321)
        tr.learn_embedding(window, epoch=2, lr=TRAINER_LR, idx=idx, model_file="m_%d" % fused, fused=fused)
        history = tr.loss_history
        assert [len(e) for e in history] == [batches] * 2
        flat = [v for e in history for v in e]
        assert all(np.isfinite(v) for v in flat) and len(set(flat)) == len(flat)          # finite, and no two alike
        folder = os.path.join(str(tmp_path), "emb_%d" % fused)
        assert os.listdir(folder) == ["2020-0%d.csv" % (idx + 1)]                         # under the snapshot's file stem
        lines = open(os.path.join(folder, os.listdir(folder)[0])).read().strip().split("\n")[1:]
        assert len(lines) == D.N and all(len(line.split("\t")) == 1 + D.OUT for line in (lines[0], lines[-1]))
        emb = np.loadtxt(os.path.join(folder, os.listdir(folder)[0]), delimiter="\t", skiprows=1, usecols=range(1, 1 + D.OUT))
        other = build(method, seed=99)
        other.load_state_dict(torch.load(os.path.join(str(tmp_path), "model", "m_%d" % fused), map_location="cpu"))       # loads back
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(other.state_dict().values(), tr.model.state_dict().values()))
        runs.append((flat, emb))
    (la, ea), (lb, eb) = runs
    err_l = max(abs(u - v) for u, v in zip(la, lb)) / max(abs(v) for v in lb)
    err_e = float(np.abs(ea - eb).max() / np.abs(eb).max())
    tol_l, tol_e = max(4 * float(g[method + "_yard_losses"]), 2e-6), max(4 * float(g[method + "_yard_hx"]), 2e-6)
    print("  [tol] %s fused vs composed: losses %.3e of %.3e allowed, export %.3e of %.3e allowed" % (method, err_l, tol_l, err_e, tol_e))
    assert float(np.abs(eb).max()) > 0 and err_l <= tol_l and err_e <= tol_e
