"""GIN and GraphSAGE through both trainers, on tests/test_gpu_gat_trainer.py's fixtures: two epochs of the unsupervised trainer (fused
and per batch) on the list of per-snapshot outputs with export and checkpoint, and two epochs of the supervised trainer on node
labels.  The losses are finite and change from one epoch to the next, and the checkpoints carry the reference's keys."""
import os

import numpy as np
import pytest
import torch

import _gin_sage_ref as G
import _sup_fixture as SF
from conftest import load_golden, seeded_parameters
from test_gpu_gat_trainer import _folders, _neg_loss

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
MODELS = {"GIN": "gin_sum", "SAGE": "sage_sum"}


def _window(name):
    import ctgcn_amd
    from ctgcn_amd import ops
    g = G.fixture()
    model = G.build(MODELS[name], ctgcn_amd.GIN, ctgcn_amd.SAGE, dropout=0.5)
    seeded_parameters(model, int(g["seed"]))
    adj = [ops.GcnAdj.from_scipy(G.raw_csr(t, np.float32), DEV) for t in range(G.T)]
    return g, model, adj, G.features(MODELS[name], device=DEV)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-batch"])
@pytest.mark.parametrize("name", MODELS)
def test_unsupervised_training_runs_exports_and_checkpoints(tmp_path, name, fused):
    from ctgcn_amd import UnsupervisedEmbedding
    g, model, adj, x = _window(name)
    assert model.method_name == name
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb", ["n%d" % i for i in range(G.N)], model, _neg_loss(7), has_cuda=True)
    sums = []
    step = torch.optim.Adam.step

    def record(opt, *a, **k):                       # once per epoch, right after the epoch's batch losses are in place
        sums.append(float(np.sum(emb.last_epoch_losses)))
        return step(opt, *a, **k)

    torch.manual_seed(123)
    torch.optim.Adam.step = record
    try:
        emb.learn_embedding(adj, x, epoch=2, batch_size=512, lr=1e-3, model_file="m.pt", fused=fused)
    finally:
        torch.optim.Adam.step = step
    assert len(sums) == 2 and np.isfinite(sums).all() and sums[0] != sums[1], sums
    folder = os.path.join(str(tmp_path), "emb")
    names = sorted(os.listdir(folder))
    assert names == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    rows = open(os.path.join(folder, names[0])).read().rstrip("\n").split("\n")[1:]
    assert len(rows) == G.N and all(len(r.split("\t")) == 1 + G.OUT for r in rows)
    sd = torch.load(os.path.join(str(tmp_path), "model", "m.pt"), map_location="cpu")
    assert sorted(sd) == [str(k) for k in g[MODELS[name] + "_state_keys"]]


@pytest.mark.parametrize("name", MODELS)
def test_supervised_node_classification_runs_and_exports(tmp_path, name):
    from ctgcn_amd import ClassificationLoss, MLPClassifier, SupervisedEmbedding
    g, model, adj, x = _window(name)
    snapshots = load_golden("uci_snapshots.npz")
    labels = [torch.from_numpy(SF.node_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS]
    classifier = MLPClassifier(G.OUT, G.OUT, 4, 1, G.T, bias=True, activate_type="N")
    seeded_parameters(classifier, SF.CLS_SEED)
    tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_sup", ["n%d" % i for i in range(G.N)], model, ClassificationLoss(4), classifier,
                             has_cuda=True)
    tr.learn_embedding(adj, x, learning_type="S-node", epoch=2, lr=1e-3, model_file="sup_m", classifier_file="sup_c", node_labels=labels)
    losses = [h["loss_train"] for h in tr.history]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[0] != losses[1], losses
    assert tr.test_result is not None and np.isfinite(tr.test_result[0])
    names = sorted(os.listdir(os.path.join(str(tmp_path), "emb_sup")))
    assert names == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]


def test_a_module_that_only_carries_the_name_is_refused(tmp_path):
    """the trainers run GIN and SAGE as this package's modules (ctgcn_pool.hip); anything else under that name has no such path"""
    from ctgcn_amd import ClassificationLoss, MLPClassifier, SupervisedEmbedding, UnsupervisedEmbedding
    g, model, adj, x = _window("GIN")
    model.method_name = "SAGE"
    names = ["n%d" % i for i in range(G.N)]
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb_x", names, model, _neg_loss(7), has_cuda=True)
    with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline.SAGE"):
        emb.learn_embedding(adj, x, epoch=1, export=False)
    stand_in = torch.nn.Linear(2, 2)
    stand_in.method_name = "GIN"
    tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_y", names, stand_in, ClassificationLoss(4),
                             MLPClassifier(G.OUT, G.OUT, 4, 1, G.T, bias=True, activate_type="N"), has_cuda=True)
    with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline.GIN"):
        tr.learn_embedding(adj, x, learning_type="S-node", epoch=1, node_labels=[])
