"""GAT through both trainers: the epoch-fused and the per-batch unsupervised paths on its list of per-snapshot outputs, export and
checkpoint; the supervised trainer on node and on edge labels.  tests/test_gpu_egcn_trainer.py's tests and bounds, for
GAT(N, 8, 16, head_num=8) on identity features (the gat_uneg fixture case, dropout 0)."""
import os

import numpy as np
import pytest
import torch

import _egcn_ref as E
import _gat_ref as A
import _gcrn_ref as R
import _sup_fixture as SF
from conftest import load_golden, seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUT = 16


def _folders(tmp_path):
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t in range(A.T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _window(learning_type="U-neg"):
    from ctgcn_amd import GAT, ops
    g = A.fixture()
    model = GAT(A.N, 8, OUT, dropout=0.0, alpha=0.2, head_num=8, learning_type=learning_type)
    seeded_parameters(model, int(g["seed"]))
    adj = [ops.GcnAdj.from_scipy(R.row_normalized_csr(t, np.float32), DEV) for t in range(A.T)]
    return g, model, adj, A.features("gat_uneg", device=DEV)


def _neg_loss(seed):
    """negative-sampling loss whose pair CSR is the snapshot graph itself and whose table is a random node list"""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import WalkPairs
    rng = np.random.default_rng(seed)
    pairs, tables = [], []
    for t in range(A.T):
        m = E.snapshot_csr(t, with_eye=False)
        pairs.append(WalkPairs(torch.from_numpy(m.indptr.astype(np.int32)).to(DEV), torch.from_numpy(m.indices.astype(np.int32)).to(DEV)))
        tables.append(rng.integers(0, A.N, size=300).astype(np.int32))
    return NegativeSamplingLoss(pairs, tables, neg_num=6, Q=2.0, seed=seed)


def _train(tmp_path, fused, monkeypatch):
    from ctgcn_amd import UnsupervisedEmbedding
    g, model, adj, x = _window()
    folder = "emb_fused" if fused else "emb_batch"
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", folder, ["n%d" % i for i in range(A.N)], model, _neg_loss(7), has_cuda=True)
    sums, grads = [], []
    step = torch.optim.Adam.step

    def record(opt, *a, **k):                       # once per epoch, right after the epoch's batch losses and gradients are in place
        sums.append(np.asarray(emb.last_epoch_losses, dtype=np.float64))
        grads.append({n: p.grad.detach().cpu().double().numpy().copy() for n, p in model.named_parameters()})
        return step(opt, *a, **k)

    torch.manual_seed(123)                          # the epoch orders: all_nodes[torch.randperm(N)]
    monkeypatch.setattr(torch.optim.Adam, "step", record)
    emb.learn_embedding(adj, x, epoch=2, batch_size=512, lr=1e-3, model_file="m_%d.pt" % fused, fused=fused)
    monkeypatch.setattr(torch.optim.Adam, "step", step)
    return g, sums, grads, os.path.join(str(tmp_path), folder)


def test_fused_and_per_batch_epochs_agree_export_and_checkpoint(tmp_path, monkeypatch):
    g, sums_f, grads_f, dir_f = _train(tmp_path, True, monkeypatch)
    _, sums_b, grads_b, dir_b = _train(tmp_path, False, monkeypatch)
    assert [len(v) for v in sums_f] == [len(v) for v in sums_b] == [4, 4]  # two epochs of 1899 / 512: three full batches and a partial one
    for lf, lb in zip(sums_f, sums_b):
        # tests/test_gpu_trainer.py's bound for this comparison: every batch loss within 1e-5 of the largest one, so the epoch's sum of
        # 4 within 4e-5 of it
        assert np.isfinite(lf).all() and np.all(np.abs(lf - lb) <= 1e-5 * np.abs(lb).max()), (sums_f, sums_b)
        assert abs(lf.sum() - lb.sum()) <= 4e-5 * np.abs(lb).max()
    # the first epoch's accumulated gradient: one backward of the summed loss against four backward passes added up, each tensor within
    # 1e-4 of its largest entry (fp32 sums of 4 terms in another order, through two attention layers)
    for k in grads_f[0]:
        top = np.abs(grads_b[0][k]).max()
        assert top > 0 and np.abs(grads_f[0][k] - grads_b[0][k]).max() <= 1e-4 * top, k
    names = sorted(os.listdir(dir_f))
    assert names == sorted(os.listdir(dir_b)) == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    for f in names:
        rows = open(os.path.join(dir_f, f)).read().rstrip("\n").split("\n")[1:]           # after the header line
        assert len(rows) == A.N and all(len(r.split("\t")) == 1 + OUT for r in rows)      # node name + embed_dim columns
    for fused in (1, 0):
        sd = torch.load(os.path.join(str(tmp_path), "model", "m_%d.pt" % fused), map_location="cpu")
        assert sorted(sd) == [str(k) for k in g["gat_uneg_keys"]]


@pytest.mark.parametrize("learning_type", ["S-node", "S-edge"])
def test_supervised_classification_runs_and_exports(tmp_path, learning_type):
    from ctgcn_amd import ClassificationLoss, EdgeClassifier, MLPClassifier, SupervisedEmbedding
    g, model, adj, x = _window(learning_type)
    snapshots = load_golden("uci_snapshots.npz")
    if learning_type == "S-node":
        labels = dict(node_labels=[torch.from_numpy(SF.node_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS])
        classifier, n_class = MLPClassifier(OUT, OUT, 4, 1, A.T, bias=True, activate_type="N"), 4
    else:
        labels = dict(edge_labels=[torch.from_numpy(SF.edge_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS])
        classifier, n_class = EdgeClassifier(OUT, OUT, 3, 1, A.T, bias=True, activate_type="L"), 3
    seeded_parameters(classifier, SF.CLS_SEED)
    tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_sup", ["n%d" % i for i in range(A.N)], model, ClassificationLoss(n_class),
                             classifier, has_cuda=True)
    tr.learn_embedding(adj, x, learning_type=learning_type, epoch=2, lr=1e-3, model_file="sup_m", classifier_file="sup_c", **labels)
    assert len(tr.history) == 2 and all(np.isfinite(h["loss_train"]) for h in tr.history)
    assert tr.test_result is not None and np.isfinite(tr.test_result[0])
    names = sorted(os.listdir(os.path.join(str(tmp_path), "emb_sup")))
    assert names == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    rows = open(os.path.join(str(tmp_path), "emb_sup", names[0])).read().rstrip("\n").split("\n")[1:]
    assert len(rows) == A.N and len(rows[0].split("\t")) == 1 + OUT


def test_other_baselines_are_still_refused(tmp_path):
    from ctgcn_amd import UnsupervisedEmbedding
    g, model, adj, x = _window()
    model.method_name = "SAGE"
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb_x", ["n%d" % i for i in range(A.N)], model, _neg_loss(7), has_cuda=True)
    with pytest.raises(NotImplementedError):
        emb.learn_embedding(adj, x, epoch=1, export=False)
