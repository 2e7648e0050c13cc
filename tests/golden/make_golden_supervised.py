#!/usr/bin/env python3
"""Generate tests/golden/supervised_uci.npz by RUNNING the reference's supervised trainer (embedding.py:93-290).

Like its siblings this script runs only where the reference tree is: it imports the reference in-process and stores inputs and
outputs as data, no source text.  Three run-time shims of its own (reference files untouched): np.int = int, metrics.label_binarize
called with the keyword sklearn now requires, and metrics.roc_auc_score wrapped to return np.float64 (the trainer calls .item() on it).
Re-run:  python tests/golden/make_golden_supervised.py

Setup (tests/_sup_fixture.py): the 3-month UCI window w4_* of uci_core_adj.npz (n = 1899), CTGCN(24, 128, 128, 1, 2, 3, 'C', 'L') and
the -S twin of models_w128.npz (CGCN(24, 128, 128, 1, 2, 'C', 'L') on the first month for edge_cgcn), formula_tensor inputs,
conftest.seeded_parameters for model and classifier (rebuilt by the tests, not stored), labels with seeded row permutations,
ratios 0.5 / 0.3 / 0.2, 3 epochs, lr 1e-3, a single-Linear head ('N' for S-node, 'L' for S-edge).

The trainer is run through a subclass that keeps the splits it drew (so the float64 and the float32 run score the same items) and a
loss wrapper that records every call; the modules that compute are the reference's.  S-edge: the reference's EdgeClassifier.forward
hands Hadamard matrices to a classifier that indexes batch_indices (models.py:123-125, :69-76) and fails on the trainer's per-snapshot
index lists, for CGCN as for CTGCN; both S-edge cases are therefore computed with the reference's own InnerProduct(reduce=False) and
MLPClassifier.mlp_classifier called per snapshot, the evident intent.

Per case <c> (node_c, node_s, link_st, link_dy, edge_cgcn, edge_ctgcn), from the float64 run (the truth) unless marked f32:
  <c>_hist / <c>_f32_hist       [3, 6]: loss, acc, auc of train and of val per epoch (NaN where the reference has no val pass)
  <c>_test / <c>_f32_test       [3]; <c>_best / <c>_f32_best: the epoch (1-based) whose checkpoint the test pass used, 0 for none
  <c>_acc_val                   [3]: acc_val per epoch (NaN for epoch 1), for the best-epoch comparison
  <c>_grad_<parameter>*         the model's gradients at the first Adam step, in make_golden.put_tensor form
  <c>_classifier_unchanged      the classifier's weights are bit-equal before and after learn_embedding
  <c>_gap, <c>_gap_start        decision gap (top-two logit gap, or |z|) of every scored item, float32, calls x snapshots concatenated in
                                _sup_fixture.CALLS order; gap_start [calls, snapshots + 1] are the offsets
  <c>_max_logit, <c>_tau        [calls, snapshots]: max |logit| and tau = 2 r max |logit| (r = 1e-4 NODE, 2e-4 pair modes)
  <c>_near_tie                  [calls, snapshots]: items with a gap below tau; <c>_items: items per (call, snapshot)
  <c>_auc_pairs                 [calls, snapshots]: (positive, negative) score pairs closer than tau, over n_pos n_neg: how far the
                                AUC can move when every score moves by at most tau / 2 (probabilities move by at most tau / 4)
  1-D cases: the hist / test AUC is sklearn's of the float64 z (the ranking sigmoid(sigmoid(z)) has in exact arithmetic);
  <c>_ref_auc / <c>_f32_ref_auc [calls]: what the reference printed (its AUC of sigmoid(sigmoid(z)), mean over snapshots), for the record
  link cases: <c>_snapshots and <c>_split_<part>_<s> uint16 [2, n]: the reference's own splits (positives then negatives)
  state_keys_<module>           the state-dict keys of the reference's MLPClassifier / InnerProduct / EdgeClassifier (duration 3)
label_seed: the first seed from SEED on for which the items with a gap below tau are at most 0.5 % of every split at every epoch.
"""
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
import scipy.sparse as sp
import torch

warnings.filterwarnings("ignore")
np.int = int
REF = "/root/reference"
sys.path.insert(0, REF)
import embedding as ref_embedding  # noqa: E402
import metrics as ref_metrics  # noqa: E402
import models as ref_models  # noqa: E402
import utils as ref_utils  # noqa: E402
from sklearn.metrics import roc_auc_score  # noqa: E402
from sklearn.preprocessing import label_binarize  # noqa: E402

ref_metrics.label_binarize = lambda y, classes: label_binarize(y, classes=classes)
ref_metrics.roc_auc_score = lambda *a, **k: np.float64(roc_auc_score(*a, **k))

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _sup_fixture as SF  # noqa: E402
from conftest import formula_tensor, seeded_parameters  # noqa: E402

SEED = 20261101
MAX_TIE_FRACTION = 0.005


class PerSnapshotEdge(torch.nn.Module):
    """the reference's EdgeClassifier with its two modules composed per snapshot"""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, x, edge_index):
        return [self.inner.classifier.mlp_classifier(self.inner.conv.inner_product(x[i], edge_index[i])) for i in range(len(x))]


class RecordingLoss(torch.nn.Module):
    def __init__(self, inner, s_model):
        super().__init__()
        self.inner, self.s_model, self.calls = inner, s_model, []

    def forward(self, input_list, labels):
        res = self.inner(input_list, labels)
        cls = input_list[0] if self.s_model else input_list
        cls = [cls] if not isinstance(cls, list) and cls.dim() == 2 else cls
        self.calls.append(dict(loss=float(res[0]), acc=float(res[1]), auc=float(res[2]), logits=[c.detach().double().numpy() for c in cls],
                               labels=[np.asarray(l.detach().numpy()) for l in labels]))
        return res


class Trainer(ref_embedding.SupervisedEmbedding):
    splits = None

    def get_batch_info(self, *a, **k):
        if Trainer.splits is None:
            Trainer.splits = super().get_batch_info(*a, **k)
        dt = next(self.model.parameters()).dtype
        return tuple([t.to(dt) if t.is_floating_point() else t for t in part] for part in Trainer.splits)


def adjacency(dtype, months):
    ca = np.load(os.path.join(OUT, "uci_core_adj.npz"))
    out = []
    for t in months:
        mats = []
        for j in range(int(ca["w4_K"][t])):
            m = sp.csr_matrix((ca["w4_t%d_j%d_data" % (t, j)].astype(np.float32), ca["w4_t%d_j%d_indices" % (t, j)],
                               ca["w4_t%d_j%d_indptr" % (t, j)]), shape=(SF.N_NODES, SF.N_NODES))
            mats.append(ref_utils.sparse_mx_to_torch_sparse_tensor(m).to(dtype))
        out.append(mats)
    return out


def build(case, dtype):
    ltype, mname, _, n_class = SF.CASES[case]
    dur = 1 if mname == "CGCN-C" else 3
    if mname == "CGCN-C":
        model = ref_models.CGCN(24, 128, 128, 1, 2, rnn_type="GRU", model_type="C", trans_activate_type="L")
    elif mname == "CTGCN-C":
        model = ref_models.CTGCN(24, 128, 128, 1, 2, 3, rnn_type="GRU", model_type="C", trans_activate_type="L")
    else:
        model = ref_models.CTGCN(24, 128, 128, 3, 1, 3, rnn_type="GRU", model_type="S", trans_activate_type="N")
    seeded_parameters(model, SF.MODEL_SEED[mname])
    if ltype == "S-node":
        inner = classifier = ref_models.MLPClassifier(128, 128, n_class, 1, dur, bias=True, activate_type=SF.CLS_ACT[ltype])
    elif ltype == "S-edge":
        inner = ref_models.EdgeClassifier(128, 128, n_class, 1, dur, bias=True, activate_type=SF.CLS_ACT[ltype])
        classifier = PerSnapshotEdge(inner)
    else:
        inner = classifier = ref_models.InnerProduct()
    seeded_parameters(inner, SF.CLS_SEED)
    loss = (ref_metrics.StructureClassificationLoss if mname.endswith("-S") else ref_metrics.ClassificationLoss)(n_class)
    x = [torch.from_numpy(v).to(dtype) for v in formula_tensor((3, SF.N_NODES, 24), 0.11, 0.3)][:dur]
    return model.to(dtype), classifier.to(dtype), inner, RecordingLoss(loss, mname.endswith("-S")), x, adjacency(dtype, range(dur)), dur


def run(case, dtype, snapshots, label_seed, base):
    ltype = SF.CASES[case][0]
    model, classifier, inner, loss, x, adj, dur = build(case, dtype)
    node_labels = edge_labels = edges = None
    if ltype == "S-node":
        node_labels = [torch.from_numpy(SF.node_label_rows(snapshots, t, label_seed)) for t in SF.MONTHS[:dur]]
    elif ltype == "S-edge":
        edge_labels = [torch.from_numpy(SF.edge_label_rows(snapshots, t, label_seed)) for t in SF.MONTHS[:dur]]
    else:
        edges = [torch.from_numpy(SF.edge_list(snapshots, t)) for t in SF.MONTHS[:dur]]
    before = {k: v.clone() for k, v in inner.state_dict().items()}
    grads = {}
    orig = torch.optim.Adam.step

    def step(opt, *a, **k):
        if not grads:
            for name, p in model.named_parameters():
                grads[name] = (p.grad if p.grad is not None else torch.zeros_like(p)).detach().clone()
        return orig(opt, *a, **k)

    torch.optim.Adam.step = step
    try:
        tr = Trainer(base, "origin", "emb_" + case, ["n%d" % i for i in range(SF.N_NODES)], model, loss, classifier, has_cuda=False)
        tr.learn_embedding(adj, x, node_labels, edge_labels, edges, None, learning_type=ltype, epoch=SF.EPOCHS, batch_size=1024, lr=SF.LR,
                           train_ratio=SF.RATIOS[0], val_ratio=SF.RATIOS[1], test_ratio=SF.RATIOS[2], model_file=case + "_m",
                           classifier_file=case + "_c", export=False)
    finally:
        torch.optim.Adam.step = orig
    unchanged = all(torch.equal(before[k], v) for k, v in inner.state_dict().items())
    assert len(loss.calls) == len(SF.CALLS)
    return loss.calls, grads, unchanged


def gaps_of(logits):
    if logits.ndim == 1:
        return np.abs(logits)
    top = np.sort(logits, axis=1)
    return top[:, -1] - top[:, -2]


def pair_fraction(scores, pos, tau):
    """(positive, negative) pairs with |s_p - s_n| < tau, over n_pos n_neg"""
    sp_, sn = scores[pos], np.sort(scores[~pos])
    cnt = (np.searchsorted(sn, sp_ + tau, "left") - np.searchsorted(sn, sp_ - tau, "right")).sum()
    return cnt / (len(sp_) * float(len(sn)))


def softmax(z):
    e = np.exp(z - z.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def summarise(case, calls, d, prefix):
    """hist / test / best of a run; 1-D cases: the AUC of z (the printed one is kept as ref_auc)"""
    n_class = SF.CASES[case][3]
    hist = np.full((SF.EPOCHS, 6), np.nan)
    test = np.zeros(3)
    ref_auc = np.zeros(len(calls))
    for k, ((part, ep), c) in enumerate(zip(SF.CALLS, calls)):
        ref_auc[k] = c["auc"]
        auc = c["auc"]
        if c["logits"][0].ndim == 1:
            auc = float(np.mean([roc_auc_score(l, z) for z, l in zip(c["logits"], c["labels"])]))
        row = (c["loss"], c["acc"], auc)
        if part == "test":
            test[:] = row
        else:
            hist[ep, (0 if part == "train" else 3):(3 if part == "train" else 6)] = row
    best, best_acc = 0, 0
    for ep in range(1, SF.EPOCHS):
        if hist[ep, 4] > best_acc:
            best, best_acc = ep + 1, hist[ep, 4]
    d[prefix + "hist"], d[prefix + "test"], d[prefix + "best"] = hist, test, np.int64(best)
    if n_class == 2:
        d[prefix + "ref_auc"] = ref_auc
    return hist


def put_tensor(d, key, g, full_below=6000):
    g = g.detach().numpy().astype(np.float64)
    d[key + "__sum"] = np.float64(g.sum())
    d[key + "__abssum"] = np.float64(np.abs(g).sum())
    if g.size <= full_below:
        d[key] = g.astype(np.float32)
    else:
        flat = g.reshape(-1)
        pick = np.linspace(0, flat.size - 1, 256).astype(np.int64)
        d[key + "__pick"] = pick
        d[key + "__vals"] = flat[pick].astype(np.float32)


def generate(label_seed, snapshots, base):
    d = {"label_seed": np.int64(label_seed)}
    worst = 0.0
    for case, (ltype, mname, r, n_class) in SF.CASES.items():
        Trainer.splits = None
        np.random.seed(label_seed)
        calls, grads, unchanged = run(case, torch.float64, snapshots, label_seed, base)
        splits = Trainer.splits
        calls32, _, unchanged32 = run(case, torch.float32, snapshots, label_seed, base)
        hist = summarise(case, calls, d, case + "_")
        summarise(case, calls32, d, case + "_f32_")
        d[case + "_acc_val"] = hist[:, 4]
        d[case + "_classifier_unchanged"] = np.bool_(unchanged and unchanged32)
        for name, g in grads.items():
            put_tensor(d, "%s_grad_%s" % (case, name), g)
        S = len(calls[0]["logits"])
        shape = (len(calls), S)
        gap, start = [], np.zeros((len(calls), S + 1), np.int64)
        max_logit, tau, near, items, pairs = (np.zeros(shape) for _ in range(5))
        off = 0
        for k, c in enumerate(calls):
            for s, (z, lab) in enumerate(zip(c["logits"], c["labels"])):
                g_ = gaps_of(z)
                max_logit[k, s] = np.abs(z).max()
                tau[k, s] = 2 * r * max_logit[k, s]
                near[k, s] = (g_ < tau[k, s]).sum()
                items[k, s] = len(g_)
                if z.ndim == 1:
                    pairs[k, s] = pair_fraction(z, lab > 0.5, tau[k, s])
                else:
                    onehot = lab[:, None] == np.arange(n_class)[None, :]
                    pairs[k, s] = pair_fraction(softmax(z).reshape(-1), onehot.reshape(-1), tau[k, s])
                start[k, s] = off
                off += len(g_)
                gap.append(g_.astype(np.float32))
            start[k, S] = off
        worst = max(worst, float((near / items).max()))
        d[case + "_gap"], d[case + "_gap_start"] = np.concatenate(gap), start
        d[case + "_max_logit"], d[case + "_tau"], d[case + "_near_tie"], d[case + "_items"], d[case + "_auc_pairs"] = max_logit, tau, near, items, pairs
        if ltype.startswith("S-link"):
            d[case + "_snapshots"] = np.int64(S)
            for p, part in enumerate(("train", "val", "test")):
                for s in range(S):
                    d["%s_split_%s_%d" % (case, part, s)] = splits[2 * p][s].numpy().astype(np.uint16)
        print(case, "best", int(d[case + "_best"]), "worst near-tie fraction so far %.4f" % worst, "hist", np.round(hist, 4).tolist(), flush=True)
    return d, worst


def main():
    torch.set_num_threads(8)
    snapshots = np.load(os.path.join(OUT, "uci_snapshots.npz"))
    base = tempfile.mkdtemp()
    try:
        os.makedirs(os.path.join(base, "origin"))
        for t in SF.MONTHS:
            open(os.path.join(base, "origin", str(snapshots["files"][t])), "w").close()
        seed = SEED
        while True:
            d, worst = generate(seed, snapshots, base)
            if worst <= MAX_TIE_FRACTION:
                break
            print("label seed", seed, "has a split with %.4f near-tie items: next seed" % worst)
            seed += 1
    finally:
        shutil.rmtree(base, ignore_errors=True)
    for name, mod in (("MLPClassifier", ref_models.MLPClassifier(128, 128, 4, 1, 3)), ("InnerProduct", ref_models.InnerProduct()),
                      ("EdgeClassifier", ref_models.EdgeClassifier(128, 128, 3, 1, 3))):
        d["state_keys_" + name] = np.array(list(mod.state_dict().keys()), dtype="U64")
    path = os.path.join(OUT, "supervised_uci.npz")
    np.savez_compressed(path, **d)
    print("wrote", path, os.path.getsize(path), "bytes; label_seed", seed)


if __name__ == "__main__":
    main()
