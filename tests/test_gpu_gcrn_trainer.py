"""GCRN through both trainers: the epoch-fused and the per-batch unsupervised paths on its [T, N, d] output, export and checkpoint; the
supervised trainer on node labels.  tests/test_gpu_egcn_trainer.py's two tests and bounds, for GCRN(N, 0, 20, 128, duration=3)."""
import os

import numpy as np
import pytest
import torch

import _egcn_ref as E
import _gcrn_ref as R
import _sup_fixture as SF
from conftest import load_golden, seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = 128


def _folders(tmp_path):
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t in range(R.T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _window():
    from ctgcn_amd import GCRN, ops
    g = R.fixture()
    model = GCRN(R.N, 0, R.HID, OUT, dropout=0.0, duration=R.T)
    seeded_parameters(model, int(g["seed"]))
    adj = [ops.GcnAdj.from_scipy(R.row_normalized_csr(t, np.float32), DEV) for t in range(R.T)]
    return g, model, adj, R.features("gcrn_gru", device=DEV)


def _neg_loss(seed):
    """negative-sampling loss whose pair CSR is the snapshot graph itself and whose table is a random node list"""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import WalkPairs
    rng = np.random.default_rng(seed)
    pairs, tables = [], []
    for t in range(R.T):
        m = E.snapshot_csr(t, with_eye=False)
        pairs.append(WalkPairs(torch.from_numpy(m.indptr.astype(np.int32)).to(DEV), torch.from_numpy(m.indices.astype(np.int32)).to(DEV)))
        tables.append(rng.integers(0, R.N, size=300).astype(np.int32))
    return NegativeSamplingLoss(pairs, tables, neg_num=6, Q=2.0, seed=seed)


def _train(tmp_path, fused, monkeypatch):
    from ctgcn_amd import UnsupervisedEmbedding
    g, model, adj, x = _window()
    folder = "emb_fused" if fused else "emb_batch"
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", folder, ["n%d" % i for i in range(R.N)], model, _neg_loss(7), has_cuda=True)
    sums = []
    step = torch.optim.Adam.step

    def record(opt, *a, **k):                       # once per epoch, right after the epoch's batch losses are in place
        sums.append(np.asarray(emb.last_epoch_losses, dtype=np.float64))
        return step(opt, *a, **k)

    torch.manual_seed(123)                          # the epoch orders: all_nodes[torch.randperm(N)]
    monkeypatch.setattr(torch.optim.Adam, "step", record)
    emb.learn_embedding(adj, x, epoch=2, batch_size=512, lr=1e-3, model_file="m_%d.pt" % fused, fused=fused)
    monkeypatch.setattr(torch.optim.Adam, "step", step)
    return g, sums, os.path.join(str(tmp_path), folder)


def test_fused_and_per_batch_epochs_agree_export_and_checkpoint(tmp_path, monkeypatch):
    g, sums_f, dir_f = _train(tmp_path, True, monkeypatch)
    _, sums_b, dir_b = _train(tmp_path, False, monkeypatch)
    assert [len(v) for v in sums_f] == [len(v) for v in sums_b] == [4, 4]  # two epochs of 1899 / 512: three full batches and a partial one
    for lf, lb in zip(sums_f, sums_b):
        # tests/test_gpu_trainer.py's bound for this comparison: every batch loss within 1e-5 of the largest one, so the epoch's sum of
        # 4 within 4e-5 of it
        assert np.isfinite(lf).all() and np.all(np.abs(lf - lb) <= 1e-5 * np.abs(lb).max()), (sums_f, sums_b)
        assert abs(lf.sum() - lb.sum()) <= 4e-5 * np.abs(lb).max()
    names = sorted(os.listdir(dir_f))
    assert names == sorted(os.listdir(dir_b)) == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    for f in names:
        rows = open(os.path.join(dir_f, f)).read().rstrip("\n").split("\n")[1:]           # after the header line
        assert len(rows) == R.N and all(len(r.split("\t")) == 1 + OUT for r in rows)      # node name + 128 columns
    for fused in (1, 0):
        sd = torch.load(os.path.join(str(tmp_path), "model", "m_%d.pt" % fused), map_location="cpu")
        assert sorted(sd) == [str(k) for k in g["gcrn_gru_keys"]]


def test_supervised_node_classification_runs_and_exports(tmp_path):
    from ctgcn_amd import ClassificationLoss, MLPClassifier, SupervisedEmbedding
    g, model, adj, x = _window()
    snapshots = load_golden("uci_snapshots.npz")
    labels = [torch.from_numpy(SF.node_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS]
    classifier = MLPClassifier(OUT, OUT, 4, 1, R.T, bias=True, activate_type="N")
    seeded_parameters(classifier, SF.CLS_SEED)
    tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_sup", ["n%d" % i for i in range(R.N)], model, ClassificationLoss(4), classifier,
                             has_cuda=True)
    tr.learn_embedding(adj, x, node_labels=labels, learning_type="S-node", epoch=2, lr=1e-3, model_file="sup_m", classifier_file="sup_c")
    assert len(tr.history) == 2 and all(np.isfinite(h["loss_train"]) for h in tr.history)
    assert tr.test_result is not None and np.isfinite(tr.test_result[0])
    names = sorted(os.listdir(os.path.join(str(tmp_path), "emb_sup")))
    assert names == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    rows = open(os.path.join(str(tmp_path), "emb_sup", names[0])).read().rstrip("\n").split("\n")[1:]
    assert len(rows) == R.N and len(rows[0].split("\t")) == 1 + OUT
