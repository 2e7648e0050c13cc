"""PGNN through both trainers on the UCI window of tests/golden/pgnn_uci.npz: two epochs of the unsupervised trainer (U-neg) and of
the supervised trainer (S-node, S-link-dy), fused and per batch.  The losses are finite and, under torch.manual_seed, the same from run
to run (the anchor sets come from torch's generator); the export has anchor_set_count(1899) columns; a run with the anchor sets pinned
equals, bit for bit, a step made by hand from ops.pgnn_conv and the loss module; a missing node_dist_list raises.

Reproducible means bit for bit, both epochs, on every path.  The fused paths' kernels add in a fixed order.  The unfused paths gather
embedding rows with torch's indexing, whose backward accumulates with float atomics in whatever order the hardware takes unless torch
is told otherwise; those runs are made under torch.use_deterministic_algorithms(True), which gives that backward a fixed order, so
that a second-epoch anchor draw or a PGNN backward that differed between two seeded runs cannot hide behind the atomics' noise."""
import os

import numpy as np
import pytest
import torch

import _pgnn_ref as P
import _sup_fixture as SF
from conftest import load_golden, seeded_parameters
from test_gpu_gat_trainer import _folders, _neg_loss

import contextlib

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAMES = ["n%d" % i for i in range(P.N)]


@contextlib.contextmanager
def fixed_order(on):
    """torch's own kernels in their deterministic forms (the indexing backward of the unfused loss and head paths) while `on`"""
    before, warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    if on:
        torch.use_deterministic_algorithms(True, warn_only=True)      # warn only: bincount in the index build has no such form and needs none
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before, warn_only=warn)


def _edges():
    out = []
    for t in range(P.T):
        coo = P.G.raw_csr(t).tocoo()
        out.append(torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64)).to(DEV))
    return out


def _window(dropout=0.5):
    import ctgcn_amd
    from ctgcn_amd.baseline import precompute_dist_data
    model = P.build("pgnn_l2", ctgcn_amd.PGNN, dropout=dropout)
    seeded_parameters(model, int(P.fixture()["seed"]))
    return model, P.features(device=DEV), precompute_dist_data(_edges(), P.N, -1)


def _unsupervised(tmp_path, folder, fused, seed, dropout=0.5, epoch=2, export=True):
    from ctgcn_amd import UnsupervisedEmbedding
    model, x, dist = _window(dropout)
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", folder, NAMES, model, _neg_loss(7), has_cuda=True)
    sums, grads = [], []
    step = torch.optim.Adam.step

    def record(opt, *a, **k):                       # once per epoch, right after the epoch's batch losses are in place
        sums.append(list(emb.last_epoch_losses))
        grads.append({n: (None if p.grad is None else p.grad.detach().clone()) for n, p in model.named_parameters()})
        return step(opt, *a, **k)

    torch.manual_seed(seed)
    torch.optim.Adam.step = record
    try:
        with fixed_order(not fused):
            emb.learn_embedding(None, x, node_dist_list=dist, epoch=epoch, batch_size=512, lr=1e-3, model_file="m.pt", fused=fused,
                                export=export)
    finally:
        torch.optim.Adam.step = step
    return sums, grads


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "per-batch"])
def test_unsupervised_training_is_reproducible_and_exports_the_anchor_width(tmp_path, fused):
    from ctgcn_amd.baseline import anchor_set_count
    sums, grads = _unsupervised(tmp_path, "emb", fused, 123)
    again, _ = _unsupervised(tmp_path, "emb2", fused, 123)
    other, _ = _unsupervised(tmp_path, "emb3", fused, 124, epoch=1, export=False)
    assert len(sums) == 2 and len(sums[0]) == 4 and np.isfinite(sums).all() and sums[0] != sums[1], sums
    print("  [repeat] %s: batch losses of epoch 2, run 1 %s, run 2 %s" % ("fused" if fused else "per batch", sums[1], again[1]))
    assert sums == again and other[0] != sums[0]                  # both epochs, every batch, bit for bit
    assert all(grads[0][k] is None for k in grads[0] if k.startswith("conv_first.linear_out_position."))
    assert all(v is not None and bool(v.any()) for k, v in grads[0].items() if not k.startswith("conv_first.linear_out_position."))
    folder = os.path.join(str(tmp_path), "emb")
    names = sorted(os.listdir(folder))
    assert names == ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    rows = open(os.path.join(folder, names[0])).read().rstrip("\n").split("\n")[1:]
    assert anchor_set_count(P.N) == 100 and len(rows) == P.N and all(len(r.split("\t")) == 1 + 100 for r in rows)
    sd = torch.load(os.path.join(str(tmp_path), "model", "m.pt"), map_location="cpu")
    assert sorted(sd) == [str(k) for k in P.fixture()["pgnn_l2_state_keys"]]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("learning_type", ["S-node", "S-link-dy"])
def test_supervised_training_is_reproducible(tmp_path, learning_type, fused):
    from ctgcn_amd import ClassificationLoss, InnerProduct, MLPClassifier, SupervisedEmbedding
    from ctgcn_amd.baseline import anchor_set_count
    snapshots = load_golden("uci_snapshots.npz")
    width = anchor_set_count(P.N)
    runs = []
    for k in range(2):
        model, x, dist = _window()
        kwargs = {}
        if learning_type == "S-node":
            classifier = MLPClassifier(width, width, 4, 1, P.T, bias=True, activate_type="N")
            seeded_parameters(classifier, SF.CLS_SEED)
            loss = ClassificationLoss(4)
            kwargs["node_labels"] = [torch.from_numpy(SF.node_label_rows(snapshots, t, 5)).to(DEV) for t in SF.MONTHS]
        else:
            classifier, loss = InnerProduct(), ClassificationLoss(2)
            kwargs.update(edge_list=[torch.from_numpy(SF.edge_list(snapshots, t)).to(DEV) for t in SF.MONTHS], seed=1234)
        tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_sup%d" % k, NAMES, model, loss, classifier, has_cuda=True)
        torch.manual_seed(321)
        with fixed_order(not fused):
            tr.learn_embedding(None, x, node_dist_list=dist, learning_type=learning_type, epoch=2, lr=1e-3, model_file="sup_m",
                               classifier_file="sup_c", fused=fused, **kwargs)
        runs.append(([h["loss_train"] for h in tr.history], tr.history[1]["loss_val"], tr.test_result))
    losses = runs[0][0]
    assert len(losses) == 2 and np.isfinite(losses).all() and losses[0] != losses[1] and np.isfinite(runs[0][2][0]), runs[0]
    print("  [repeat] %s %s: run 1 %s, run 2 %s" % (learning_type, "fused" if fused else "unfused", runs[0], runs[1]))
    assert runs[0] == runs[1]                                     # both epochs' train losses, loss_val and the test result, bit for bit
    names = sorted(os.listdir(os.path.join(str(tmp_path), "emb_sup0")))
    assert names == (["2020-01.csv", "2020-02.csv", "2020-03.csv"] if learning_type == "S-node" else ["2020-01.csv", "2020-02.csv"])
    rows = open(os.path.join(str(tmp_path), "emb_sup0", names[0])).read().rstrip("\n").split("\n")[1:]
    assert len(rows) == P.N and all(len(r.split("\t")) == 1 + width for r in rows)


def test_a_run_with_pinned_anchor_sets_equals_a_step_made_by_hand(tmp_path, monkeypatch):
    """fused epoch, dropout 0: the trainer's gradient of epoch 1 against the same forward written out with ops.pgnn_conv, the loss
    module's epoch_loss with the trainer's seeds, and backward: the same kernels in the same order, so bit for bit"""
    from ctgcn_amd import ops
    from ctgcn_amd.baseline import pgnn
    from ctgcn_amd.embedding import batch_count
    from ctgcn_amd.metrics import epoch_batch_seed
    sets = [torch.from_numpy(s.astype(np.int64)).to(DEV) for s in P.anchor_sets(P.fixture())]
    monkeypatch.setattr(pgnn, "get_random_anchorset", lambda n, c=0.5, device=None: sets)
    sums, grads = _unsupervised(tmp_path, "emb", True, 55, dropout=0.0, epoch=1, export=False)

    model, x, dist = _window(0.0)
    model = model.to(DEV).train()
    loss = _neg_loss(7).to(DEV)
    torch.manual_seed(55)
    order = torch.randperm(P.N).to(DEV)
    dms, das = pgnn.get_dist_max(sets, dist, DEV)
    emb = []
    for t in range(P.T):
        h = pgnn.linear64(x[t], model.linear_pre.weight, model.linear_pre.bias)
        for k, layer in enumerate((model.conv_first, model.conv_out)):
            W, b = layer.linear_hidden.weight, layer.linear_hidden.bias
            half = W.shape[1] // 2
            PS = pgnn.linear64(h, torch.cat((W[:, :half], W[:, half:]), dim=0), torch.cat((torch.zeros_like(b), b)))
            table = layer.dist_compute(ops.pgnn_prepare(dms[t], das[t]).values.unsqueeze(-1)).squeeze(-1)
            pos, h = ops.pgnn_conv(PS, dms[t], das[t], layer.linear_out_position.weight, layer.linear_out_position.bias, table=table,
                                   need_pos=k == 1, need_struct=k == 0, epi=ops.PGNN_EPI_NORM if k == 1 else ops.PGNN_EPI_NONE)
        emb.append(pos)
    B = batch_count(P.N, 512)
    grad = [torch.zeros_like(e) for e in emb]
    losses = loss.epoch_loss(emb, order, 512, [[epoch_batch_seed(7, 0, b, t) for b in range(B)] for t in range(P.T)], grad)
    torch.autograd.backward(emb, grad)
    assert losses.sum(0).tolist() == sums[0]
    for k, p in model.named_parameters():
        assert (p.grad is None and grads[0][k] is None) or torch.equal(p.grad, grads[0][k]), k


def test_a_pgnn_without_node_dist_list_is_refused(tmp_path):
    from ctgcn_amd import ClassificationLoss, MLPClassifier, SupervisedEmbedding, UnsupervisedEmbedding
    model, x, dist = _window()
    emb = UnsupervisedEmbedding(_folders(tmp_path), "origin", "emb_x", NAMES, model, _neg_loss(7), has_cuda=True)
    with pytest.raises(ValueError, match="node_dist_list"):
        emb.learn_embedding(None, x, epoch=1, export=False)
    tr = SupervisedEmbedding(_folders(tmp_path), "origin", "emb_y", NAMES, model, ClassificationLoss(4),
                             MLPClassifier(100, 100, 4, 1, P.T, bias=True, activate_type="N"), has_cuda=True)
    with pytest.raises(ValueError, match="node_dist_list"):
        tr.learn_embedding(None, x, learning_type="S-node", epoch=1, node_labels=[])
