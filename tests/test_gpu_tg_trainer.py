"""TgGCN, TgGAT, TgSAGE and TgGIN through both trainers on the 3-snapshot UCI fixture, with adj_list = None as the reference's train.py
passes it for them: the epoch-fused and the per-batch unsupervised paths, the supervised trainer on node labels and on S-link-st
splits.  Losses are finite, two runs under the same torch seed and sample seed give identical losses, files and checkpoints, and the
exported files are the model's eval() forward."""
import contextlib
import os

import numpy as np
import pytest
import torch

import _egcn_ref as E
import _sup_fixture as SF
import _tg_ref as G
from conftest import load_golden, seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["n%d" % i for i in range(G.N)]


def _folders(tmp_path):
    origin = tmp_path / "origin"
    origin.mkdir(parents=True, exist_ok=True)
    for t in range(G.T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _model(kind, dropout=0.5):
    import ctgcn_amd
    model = G.build(kind, getattr(ctgcn_amd, kind), dropout=dropout)
    seeded_parameters(model, 31)
    return model


def _neg_loss(seed):
    """negative-sampling loss whose pair CSR is the snapshot graph itself and whose table is a random node list"""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import WalkPairs
    rng = np.random.default_rng(seed)
    pairs, tables = [], []
    for t in range(G.T):
        m = E.snapshot_csr(t, with_eye=False)
        pairs.append(WalkPairs(torch.from_numpy(m.indptr.astype(np.int32)).to(DEV), torch.from_numpy(m.indices.astype(np.int32)).to(DEV)))
        tables.append(rng.integers(0, G.N, size=300).astype(np.int32))
    return NegativeSamplingLoss(pairs, tables, neg_num=6, Q=2.0, seed=seed)


def _read(folder):
    return {f: open(os.path.join(folder, f)).read() for f in sorted(os.listdir(folder))}


def _check_export(files, model, x, edges):
    """the exported rows are the model's eval() forward on the trained weights"""
    assert sorted(files) == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    model.eval()
    with torch.no_grad():
        outs = model(x, edges)
    for t, f in enumerate(sorted(files)):
        rows = files[f].rstrip("\n").split("\n")[1:]                             # after the header line
        assert len(rows) == G.N and all(len(r.split("\t")) == 1 + G.OUT for r in rows)
        got = np.array([[float(v) for v in r.split("\t")[1:]] for r in rows])
        want = outs[t].cpu().double().numpy()
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()              # the file's decimal digits


@contextlib.contextmanager
def fixed_order(on):
    """torch's own kernels in their deterministic forms (the indexing backward of the unfused loss path) while `on`"""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    if on:
        torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per_batch"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_unsupervised_training_repeats_and_exports(kind, fused, tmp_path):
    """dropout 0, so that the exported rows (the last epoch's training-mode forward, as in the reference) are also the eval() forward of
    the weights that forward saw: the checkpoint of a run that is one epoch shorter"""
    from ctgcn_amd import UnsupervisedEmbedding
    x, edges = G.identity_features(device=DEV), G.edge_lists(DEV)

    def train(folder, epochs):
        base = _folders(tmp_path / folder)
        model = _model(kind, dropout=0.0)
        emb = UnsupervisedEmbedding(base, "origin", "emb", NAMES, model, _neg_loss(7), has_cuda=True)
        torch.manual_seed(123)
        with fixed_order(not fused):
            emb.learn_embedding(None, x, edge_list=edges, epoch=epochs, batch_size=512, lr=1e-3, model_file="m.pt", fused=fused)
        losses = np.asarray(emb.last_epoch_losses)
        assert losses.shape == (4,) and np.isfinite(losses).all()         # 1899 / 512: three full batches and a partial one
        return losses, _read(os.path.join(base, "emb")), torch.load(os.path.join(base, "model", "m.pt"), map_location="cpu")

    first, second, shorter = train("a", 2), train("b", 2), train("c", 1)
    assert sorted(first[2]) == sorted(_model(kind).state_dict())
    assert np.array_equal(first[0], second[0]) and first[1] == second[1]
    assert all(torch.equal(first[2][k], second[2][k]) for k in first[2])
    before_last_step = _model(kind, dropout=0.0)
    before_last_step.load_state_dict(shorter[2])
    _check_export(first[1], before_last_step.to(DEV), x, edges)


@pytest.mark.parametrize("learning_type", ["S-node", "S-link-st"])
@pytest.mark.parametrize("kind", G.KINDS)
def test_supervised_training_repeats_and_exports(kind, learning_type, tmp_path):
    from ctgcn_amd import ClassificationLoss, InnerProduct, MLPClassifier, SupervisedEmbedding
    x, edges = G.identity_features(device=DEV), G.edge_lists(DEV)
    snapshots = load_golden("uci_snapshots.npz")
    runs = []
    for k in range(2):
        base = _folders(tmp_path / ("run%d" % k))
        model = _model(kind)
        if learning_type == "S-node":
            extra = dict(node_labels=[torch.from_numpy(SF.node_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS])
            classifier, n_class = MLPClassifier(G.OUT, G.OUT, 4, 1, G.T, bias=True, activate_type="N"), 4
            seeded_parameters(classifier, SF.CLS_SEED)
        else:
            extra = dict(seed=1234)
            classifier, n_class = InnerProduct(), 2
        tr = SupervisedEmbedding(base, "origin", "emb", NAMES, model, ClassificationLoss(n_class), classifier, has_cuda=True)
        torch.manual_seed(5)
        tr.learn_embedding(None, x, edge_list=edges, learning_type=learning_type, epoch=2, lr=1e-3, model_file="m.pt", classifier_file="c.pt",
                           **extra)
        assert len(tr.history) == 2 and all(np.isfinite(h["loss_train"]) for h in tr.history) and np.isfinite(tr.test_result[0])
        runs.append(([h["loss_train"] for h in tr.history] + list(tr.test_result), _read(os.path.join(base, "emb")), model.state_dict()))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
    assert all(torch.equal(runs[0][2][k], runs[1][2][k]) for k in runs[0][2])
    _check_export(runs[1][1], model, x, edges)


def test_a_missing_edge_list_is_refused(tmp_path):
    from ctgcn_amd import UnsupervisedEmbedding
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb", NAMES, _model("TgSAGE"), _neg_loss(7), has_cuda=True)
    x = G.identity_features(device=DEV)
    with pytest.raises(ValueError, match="TgSAGE needs edge_list"):
        emb.learn_embedding(None, x, epoch=1, export=False)
    with pytest.raises(ValueError, match="TgSAGE needs edge_list"):
        emb.learn_embedding(None, x, edge_list=G.edge_lists(DEV)[:2], epoch=1, export=False)
