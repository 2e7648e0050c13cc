"""DynamicEmbedding with DynRNN and DynAERNN on the GPU: two epochs on a folder of 5 small snapshots read through the DataLoader, the
kernel path against the composed one under one seed, by the fixture rule (tests/test_gpu_dynrnn.py); the export, the checkpoint and
BatchPredictor.predict on both paths.  37 nodes in batches of 16: 74 records make 5 batches, the last of them padded with 6 empty
records (row id -1), which so reach the gathers and the LSTM path."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _dynrnn_ref as R
from conftest import seeded_parameters

pytestmark = pytest.mark.gpu
NODES, SNAPSHOTS, BATCH, LOOK_BACK = 37, 5, 16, 3
UNITS, RNN_UNITS, OUT = [12, 10], [12], 6
NAMES = ["n%d" % i for i in range(NODES)]
TRAINER_LR = 1e-4                    # see tests/test_gpu_dyngem.py: at 1e-3 Adam's division by a gradient near its eps decides, not the paths


def small_window():
    """symmetric snapshots with weights 1, 2, 3; node 36 is isolated in every one"""
    rng = np.random.default_rng(12)
    mats = []
    for _ in range(SNAPSHOTS):
        upper = sp.triu(sp.random(NODES - 1, NODES - 1, density=0.15, random_state=int(rng.integers(1 << 30)), format="csr"), k=1).tocoo()
        w = 1.0 + ((upper.row + upper.col) % 3)
        m = sp.csr_matrix((w, (upper.row, upper.col)), shape=(NODES, NODES))
        mats.append((m + m.T).tocsr())
    return mats


def window_through_the_loader(tmp_path, mats):
    from ctgcn_amd import DataLoader
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t, m in enumerate(mats):
        coo = sp.triu(m, k=1).tocoo()
        lines = ["%s\t%s\t%d" % (NAMES[i], NAMES[j], int(w)) for i, j, w in zip(coo.row, coo.col, coo.data)]
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("from_id\tto_id\tweight\n" + "\n".join(lines) + "\n")
    window = DataLoader(NAMES, len(mats), has_cuda=True).get_date_adj_list(str(origin), start_idx=0, duration=len(mats), data_type='matrix')
    assert len(window) == SNAPSHOTS and all((abs(sp.csr_matrix(w) - m)).nnz == 0 for w, m in zip(window, mats))
    return window


def build(method, seed=6):
    import ctgcn_amd
    if method == "dynrnn":
        model = ctgcn_amd.DynRNN(input_dim=NODES, output_dim=OUT, look_back=LOOK_BACK, n_units=UNITS, bias=True)
    else:
        model = ctgcn_amd.DynAERNN(input_dim=NODES, output_dim=OUT, look_back=LOOK_BACK, ae_units=UNITS, rnn_units=RNN_UNITS, bias=True)
    seeded_parameters(model, seed)
    return model


@pytest.mark.parametrize("method", R.METHODS)
def test_dynamic_embedding_two_epochs_fused_against_composed(method, tmp_path):
    import ctgcn_amd
    g = R.fixture()
    window = window_through_the_loader(tmp_path, small_window())
    batches, idx = 5, SNAPSHOTS - 1
    tol_l, tol_e = max(4 * float(g[method + "_yard_losses"]), 2e-6), max(4 * float(g[method + "_yard_hx"]), 2e-6)
    tol_p = max(4 * float(g[method + "_yard_pred"]), 2e-6)
    runs = []
    for fused in (True, False):
        model = build(method)
        gen = ctgcn_amd.BatchGenerator(NAMES, BATCH, LOOK_BACK, R.BETA, shuffle=True, has_cuda=True)
        pred = ctgcn_amd.BatchPredictor(NAMES, BATCH, has_cuda=True)
        tr = ctgcn_amd.DynamicEmbedding(str(tmp_path), "origin", "emb_%d" % fused, NAMES, model, ctgcn_amd.DynGraph2VecLoss(R.BETA, R.NU1, R.NU2),
                                        gen, pred, has_cuda=True)
        assert tr.get_batch_info(ctgcn_amd.ops.SnapshotRows(window, "cuda:0"), model) == (BATCH, batches, SNAPSHOTS - LOOK_BACK)
        torch.manual_seed(4321)
        tr.learn_embedding(window, epoch=2, lr=TRAINER_LR, idx=idx, model_file="m_%d" % fused, fused=fused)
        history = tr.loss_history
        assert [len(e) for e in history] == [batches] * 2
        flat = [v for e in history for v in e]
        assert all(np.isfinite(v) for v in flat) and len(set(flat)) == len(flat)          # finite, and no two alike
        folder = os.path.join(str(tmp_path), "emb_%d" % fused)
        assert os.listdir(folder) == ["2020-0%d.csv" % (idx + 1)]                         # under the snapshot's file stem
        lines = open(os.path.join(folder, os.listdir(folder)[0])).read().strip().split("\n")[1:]
        assert len(lines) == NODES and all(len(line.split("\t")) == 1 + OUT for line in (lines[0], lines[-1]))
        emb = np.loadtxt(os.path.join(folder, os.listdir(folder)[0]), delimiter="\t", skiprows=1, usecols=range(1, 1 + OUT))
        other = build(method, seed=99)
        other.load_state_dict(torch.load(os.path.join(str(tmp_path), "model", "m_%d" % fused), map_location="cpu"))       # loads back
        assert all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(other.state_dict().values(), tr.model.state_dict().values()))
        # the predictor on the trained model, on both paths: the last look_back snapshots
        rows = ctgcn_amd.ops.SnapshotRows(window, "cuda:0")
        start = SNAPSHOTS - LOOK_BACK
        e_f, p_f = pred.predict(tr.model, rows, start=start)
        e_c, p_c = pred.predict(tr.model, rows, fused=False, start=start)
        only_f, none_f = pred.predict(tr.model, rows, need_pred=False, start=start)
        only_c, none_c = pred.predict(tr.model, rows, need_pred=False, fused=False, start=start)
        assert tuple(e_f.shape) == (NODES, OUT) and tuple(p_f.shape) == (NODES, NODES) and none_f is None and none_c is None
        assert torch.equal(only_f, e_f) and torch.equal(only_c, e_c)
        assert float((e_f - e_c).abs().max()) <= tol_e * float(e_c.abs().max()) and float((p_f - p_c).abs().max()) <= tol_p * float(p_c.abs().max())
        mine = e_f if fused else e_c                                                      # the export is this path's prediction
        assert float(np.abs(emb - mine.double().cpu().numpy()).max()) <= 1e-6 * float(np.abs(emb).max())
        runs.append((flat, emb))
    (la, ea), (lb, eb) = runs
    err_l = max(abs(u - v) for u, v in zip(la, lb)) / max(abs(v) for v in lb)
    err_e = float(np.abs(ea - eb).max() / np.abs(eb).max())
    print("  [tol] %s fused vs composed: losses %.3e of %.3e allowed, export %.3e of %.3e allowed" % (method, err_l, tol_l, err_e, tol_e))
    assert float(np.abs(eb).max()) > 0 and err_l <= tol_l and err_e <= tol_e
