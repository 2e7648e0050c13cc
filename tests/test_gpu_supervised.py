"""SupervisedEmbedding (ctgcn_amd/embedding.py) on the GPU: every case of tests/golden/supervised_uci.npz (the reference's float64 run)
with the fused head and with stock torch ops, fused against unfused on a synthetic window, the S-link splits of the GPU sampler,
and bit-identical repeated training steps.

Fixture bounds (tests/golden/make_golden_supervised.py): losses within r·|loss| of the float64 value, r = 1e-4 (NODE) or 2e-4 (pair
modes), the project's forward rule (rtol 1e-4 on embeddings in test_gpu_models.TOL, once per factor); accuracies within the stored
count of items whose decision gap is below tau = 2·r·max|logit|; AUCs within the stored fraction of score pairs closer than tau."""
import os

import numpy as np
import pytest
import torch

import _sup_fixture as SF
from conftest import check_sampled_tensor, csr_from, formula_tensor, load_golden, seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ------------------------------------------------------------------------------------------------ against the fixture
@pytest.fixture(scope="module")
def gold():
    return load_golden("supervised_uci.npz")


@pytest.fixture(scope="module")
def window():
    import ctgcn_amd
    ca = load_golden("uci_core_adj.npz")
    adj = [ctgcn_amd.CoreAdj.from_matrices([csr_from(ca, "w4_t%d_j%d" % (t, j), SF.N_NODES, np.float32) for j in range(int(k))], device=DEV)
           for t, k in enumerate(ca["w4_K"])]
    xs = [torch.from_numpy(a).to(DEV) for a in formula_tensor((3, SF.N_NODES, 24), 0.11, 0.3)]
    return adj, xs, load_golden("uci_snapshots.npz")


def _folders(tmp_path, T):
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t in range(T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _modules(case):
    import ctgcn_amd
    ltype, mname, _, n_class = SF.CASES[case]
    dur = 1 if mname == "CGCN-C" else 3
    if mname == "CGCN-C":
        model = ctgcn_amd.CGCN(24, 128, 128, 1, 2, rnn_type="GRU", model_type="C", trans_activate_type="L")
    elif mname == "CTGCN-C":
        model = ctgcn_amd.CTGCN(24, 128, 128, 1, 2, 3, rnn_type="GRU", model_type="C", trans_activate_type="L")
    else:
        model = ctgcn_amd.CTGCN(24, 128, 128, 3, 1, 3, rnn_type="GRU", model_type="S", trans_activate_type="N")
    seeded_parameters(model, SF.MODEL_SEED[mname])
    if ltype == "S-node":
        classifier = ctgcn_amd.MLPClassifier(128, 128, n_class, 1, dur, bias=True, activate_type=SF.CLS_ACT[ltype])
    elif ltype == "S-edge":
        classifier = ctgcn_amd.EdgeClassifier(128, 128, n_class, 1, dur, bias=True, activate_type=SF.CLS_ACT[ltype])
    else:
        classifier = ctgcn_amd.InnerProduct()
    seeded_parameters(classifier, SF.CLS_SEED)
    loss = (ctgcn_amd.StructureClassificationLoss if mname.endswith("-S") else ctgcn_amd.ClassificationLoss)(n_class)
    return model, classifier, loss, dur


def _batch_info(gold, case, snapshots, dur):
    from ctgcn_amd.embedding import label_splits
    ltype = SF.CASES[case][0]
    seed = int(gold["label_seed"])
    if ltype == "S-node":
        return label_splits([torch.from_numpy(SF.node_label_rows(snapshots, t, seed)).to(DEV) for t in SF.MONTHS[:dur]], *SF.RATIOS)
    if ltype == "S-edge":
        return label_splits([torch.from_numpy(SF.edge_label_rows(snapshots, t, seed)).to(DEV) for t in SF.MONTHS[:dur]], *SF.RATIOS)
    return tuple([torch.from_numpy(x).to(DEV) for x in part] for part in SF.stored_splits(gold, case))      # the reference's own draws


def _run_case(tmp_path, gold, window, case, fused, train_classifier=False, epoch=SF.EPOCHS):
    from ctgcn_amd import SupervisedEmbedding
    adj, xs, snapshots = window
    model, classifier, loss, dur = _modules(case)
    before = {k: v.detach().clone() for k, v in classifier.state_dict().items()}
    grads = {}

    def on_backward(i, m, c):
        if i == 0:
            for name, p in m.named_parameters():
                grads[name] = None if p.grad is None else p.grad.detach().cpu().numpy().copy()

    tr = SupervisedEmbedding(_folders(tmp_path, 3), "origin", "emb_%s_%d" % (case, fused), ["n%d" % i for i in range(SF.N_NODES)], model, loss,
                             classifier, has_cuda=True)
    tr.on_backward = on_backward
    tr.learn_embedding(adj[:dur], xs[:dur], learning_type=SF.CASES[case][0], epoch=epoch, lr=SF.LR, model_file=case + "_m",
                       classifier_file=case + "_c", export=False, fused=fused, train_classifier=train_classifier,
                       batch_info=_batch_info(gold, case, snapshots, dur))
    changed = any(not torch.equal(before[k].to(v.device), v) for k, v in classifier.state_dict().items())
    return tr, grads, changed


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("case", list(SF.CASES))
def test_fixture_case(tmp_path, gold, window, case, fused):
    r = SF.CASES[case][2]
    tr, grads, changed = _run_case(tmp_path, gold, window, case, fused)
    assert not changed                                              # the default leaves the classifier the fixed random head it was
    assert bool(gold[case + "_classifier_unchanged"])
    hist, test = gold[case + "_hist"], gold[case + "_test"]
    near, items, pairs = gold[case + "_near_tie"], gold[case + "_items"], gold[case + "_auc_pairs"]
    acc_allow = (near / items).mean(1)                              # accuracy is the mean over snapshots of correct / items
    auc_allow = pairs.mean(1)
    got = {}
    for ep, rec in enumerate(tr.history):
        got[("train", ep)] = (rec["loss_train"], rec["acc_train"], rec["auc_train"])
        if rec["loss_val"] is not None:
            got[("val", ep)] = (rec["loss_val"], rec["acc_val"], rec["auc_val"])
    got[("test", 3)] = tr.test_result
    assert len(tr.history) == SF.EPOCHS and tr.history[0]["loss_val"] is None
    failures = []
    for k, (part, ep) in enumerate(SF.CALLS):
        want = test if part == "test" else hist[ep, (0 if part == "train" else 3):(3 if part == "train" else 6)]
        loss, acc, auc = got[(part, ep)]
        print("  [fixture] %-10s %-5s epoch %d: loss %.6f (f64 %.6f, rel err %.2e of %g)  acc %.6f (f64 %.6f, |d| %.2e of %.2e)  "
              "auc %.6f (f64 %.6f, |d| %.2e of %.2e)" % (case, part, ep + 1, loss, want[0], abs(loss - want[0]) / abs(want[0]), r, acc, want[1],
                                                       abs(acc - want[1]), acc_allow[k], auc, want[2], abs(auc - want[2]), auc_allow[k]))
        if abs(loss - want[0]) > r * abs(want[0]):
            failures.append("loss of %s epoch %d: %.8f against %.8f" % (part, ep + 1, loss, want[0]))
        if abs(acc - want[1]) > acc_allow[k] + 1e-12:
            failures.append("acc of %s epoch %d: %.8f against %.8f (allowance %.3e)" % (part, ep + 1, acc, want[1], acc_allow[k]))
        if abs(auc - want[2]) > auc_allow[k] + 1e-12:
            failures.append("auc of %s epoch %d: %.8f against %.8f (allowance %.3e)" % (part, ep + 1, auc, want[2], auc_allow[k]))
    assert not failures, failures
    # gradients at the first Adam step: the tolerance test_gpu_models.py applies to the same model's gradients
    assert grads
    for name, g in grads.items():
        if "diffusion_list" in name and ".linear." in name:         # CoreDiffusion.linear is never used in forward (as in the reference)
            assert g is None or not np.any(g)
            continue
        check_sampled_tensor(gold, "%s_grad_%s" % (case, name), g, 1e-3, 2e-4)
    # best epoch: equal, unless two epochs' float64 acc_val are within the near-tie allowance of each other
    want_best = int(gold[case + "_best"]) or None
    acc_val = gold[case + "_acc_val"]
    val_allow = {ep: acc_allow[k] for k, (part, ep) in enumerate(SF.CALLS) if part == "val"}
    ambiguous = any(abs(acc_val[a] - acc_val[b]) <= val_allow[a] + val_allow[b] for a in val_allow for b in val_allow if a < b)
    assert tr.best_epoch == want_best or ambiguous, (tr.best_epoch, want_best, acc_val)


@pytest.mark.parametrize("case", ["node_c", "edge_ctgcn"])
def test_train_classifier_changes_the_head(tmp_path, gold, window, case):
    _, _, changed = _run_case(tmp_path, gold, window, case, True, train_classifier=True, epoch=1)
    assert changed


# ------------------------------------------------------------------------------------------------ fused against unfused
def _synthetic(kind, n, T, seed):
    from ctgcn_amd import CTGCN, ClassificationLoss, MLPClassifier, StructureClassificationLoss
    from ctgcn_amd.helper import core_adj_from_scipy
    from ctgcn_amd.synth import dynamic_graph
    graphs = dynamic_graph(n, avg_deg=5, snapshots=T, seed=seed)
    adjs = [core_adj_from_scipy(g, 4, torch.device(DEV))[0] for g in graphs]
    if kind == "CTGCN-C":
        model, loss = CTGCN(48, 500, 128, 1, 2, T, model_type="C", trans_activate_type="L"), ClassificationLoss(4)
    else:
        model, loss = CTGCN(48, 96, 128, 2, 1, T, model_type="S", trans_activate_type="N"), StructureClassificationLoss(4)
    classifier = MLPClassifier(128, 64, 4, 1, T, bias=True, activate_type="N")
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, 48, generator=g).to(DEV) for _ in range(T)]
    labels = [torch.stack([torch.randperm(n, generator=g)[:n - 100 * t], torch.randint(0, 4, (n,), generator=g)[:n - 100 * t]], 1).to(DEV)
              for t in range(T)]
    return graphs, model, loss, classifier, adjs, xs, labels


def _train(tmp_path, kind, fused, n=1100, T=3, seed=7, epoch=2, load_model=False, modules=None, tag=None, train_classifier=False):
    from ctgcn_amd import SupervisedEmbedding
    torch.manual_seed(seed)                         # the same initial weights in every run
    _, model, loss, classifier, adjs, xs, labels = _synthetic(kind, n, T, seed)
    if modules is not None:
        model, classifier = modules
    grads = []
    folder = "emb_%s_%s" % (kind, tag or ("fused" if fused else "torch"))
    tr = SupervisedEmbedding(_folders(tmp_path, T), "origin", folder, ["node%d" % i for i in range(n)], model, loss, classifier, has_cuda=True)
    tr.on_backward = lambda i, m, c: grads.append({k: p.grad.detach().clone() for k, p in list(m.named_parameters()) + list(c.named_parameters())
                                                   if p.grad is not None})
    tr.learn_embedding(adjs, xs, node_labels=labels, learning_type="S-node", epoch=epoch, lr=1e-3, model_file="m_%s.pt" % folder,
                       classifier_file="c_%s.pt" % folder, load_model=load_model, fused=fused, train_classifier=train_classifier)
    return tr, grads, os.path.join(str(tmp_path), folder)


@pytest.mark.parametrize("kind", ["CTGCN-C", "CTGCN-S"])
def test_fused_matches_stock_torch_ops(tmp_path, kind):
    from ctgcn_amd import CTGCN, MLPClassifier
    tf, gf, dir_f = _train(tmp_path, kind, True)
    tb, gb, dir_b = _train(tmp_path, kind, False)
    lf = np.array([[h["loss_train"], h["loss_val"] or 0.0] for h in tf.history] + [[tf.test_result[0], 0.0]])
    lb = np.array([[h["loss_train"], h["loss_val"] or 0.0] for h in tb.history] + [[tb.test_result[0], 0.0]])
    print("  [fused/torch] losses", lf.tolist(), lb.tolist())
    assert np.all(np.abs(lf - lb) <= 1e-5 * np.abs(lb).max()), (lf, lb)
    assert len(gf) == len(gb) == 2 and set(gf[0]) == set(gb[0]) and len(gf[0]) > 5
    for k in gb[0]:
        scale = gb[0][k].abs().max().item()
        err = (gf[0][k] - gb[0][k]).abs().max().item()
        assert err <= 1e-4 * scale + 1e-9, "parameter %s: max|err| %.3e, max|grad| %.3e" % (k, err, scale)
    names = sorted(os.listdir(dir_f))
    assert names == sorted(os.listdir(dir_b)) and len(names) == 3 and names[0] == "2020-01.csv"
    if kind == "CTGCN-S":                          # -S exports the structure list, the MLP outputs (width 128 here)
        row = open(os.path.join(dir_f, names[0])).readline().rstrip("\n").split("\t")
        assert len(row) == 129
    # checkpoints load strict into fresh modules
    assert tf.best_epoch == 2
    base = os.path.join(str(tmp_path), "model")
    folder = os.path.basename(dir_f)
    sd_m = torch.load(os.path.join(base, "m_%s.pt" % folder), map_location="cpu")
    sd_c = torch.load(os.path.join(base, "c_%s.pt" % folder), map_location="cpu")
    fresh_m = CTGCN(48, 500, 128, 1, 2, 3, model_type="C", trans_activate_type="L") if kind == "CTGCN-C" else \
        CTGCN(48, 96, 128, 2, 1, 3, model_type="S", trans_activate_type="N")
    fresh_c = MLPClassifier(128, 64, 4, 1, 3, bias=True, activate_type="N")
    fresh_m.load_state_dict(sd_m, strict=True)
    fresh_c.load_state_dict(sd_c, strict=True)
    assert all(torch.equal(v.detach().cpu(), sd_m[k]) for k, v in tf.model.state_dict().items())      # the best checkpoint was reloaded
    # load_model=True with epoch=0: nothing changes
    t0, g0, _ = _train(tmp_path, kind, True, epoch=0, load_model=True, modules=(fresh_m, fresh_c))
    assert not g0 and t0.best_epoch is None and t0.history == []
    assert all(torch.equal(v.detach().cpu(), sd_m[k]) for k, v in t0.model.state_dict().items())
    assert all(torch.equal(v.detach().cpu(), sd_c[k]) for k, v in t0.classifier.state_dict().items())
    assert abs(t0.test_result[0] - tf.test_result[0]) <= 1e-6 * abs(tf.test_result[0])


def test_repeated_fused_step_is_bit_identical(tmp_path):
    """one fused training step twice from the same weights: bit-identical parameters after Adam, classifier included"""
    for k in (0, 1):
        (tmp_path / ("r%d" % k)).mkdir()
    runs = [_train(tmp_path / ("r%d" % k), "CTGCN-C", True, epoch=1, train_classifier=True)[0] for k in (0, 1)]
    for mod in ("model", "classifier"):
        a, b = getattr(runs[0], mod).state_dict(), getattr(runs[1], mod).state_dict()
        assert all(torch.equal(a[k], b[k]) for k in a), mod
    assert runs[0].history == runs[1].history and runs[0].test_result == runs[1].test_result


# ------------------------------------------------------------------------------------------------ S-link through the GPU sampler
def test_link_splits_from_the_gpu_sampler(tmp_path):
    from ctgcn_amd import CTGCN, ClassificationLoss, InnerProduct, SupervisedEmbedding
    import scipy.sparse as sp
    n, T = 1100, 3
    graphs, _, _, _, adjs, xs, _ = _synthetic("CTGCN-C", n, T, 7)
    edge_list = []
    for g in graphs:
        coo = sp.coo_matrix(g)
        e = np.stack([coo.row, coo.col]).astype(np.int64)
        e = np.concatenate([e, np.array([[3, 5], [3, 5]])], 1)                     # two self-loop columns: dropped
        edge_list.append(torch.from_numpy(e).to(DEV))
    torch.manual_seed(7)
    tr = SupervisedEmbedding(_folders(tmp_path, T), "origin", "emb", ["node%d" % i for i in range(n)],
                             CTGCN(48, 500, 128, 1, 2, T, model_type="C", trans_activate_type="L"), ClassificationLoss(2), InnerProduct(),
                             has_cuda=True)
    tr.learn_embedding(adjs, xs, edge_list=edge_list, learning_type="S-link-st", epoch=2, seed=1234, export=False)
    assert tr.split_seed == 1234 and len(tr.history) == 2 and 0.0 <= tr.test_result[2] <= 1.0
    a = tr.get_batch_info("S-link-st", None, None, edge_list, 1024, True, 0.5, 0.3, 0.2, seed=1234)
    b = tr.get_batch_info("S-link-st", None, None, edge_list, 1024, True, 0.5, 0.3, 0.2, seed=1234)
    c = tr.get_batch_info("S-link-st", None, None, edge_list, 1024, True, 0.5, 0.3, 0.2, seed=1235)
    dy = tr.get_batch_info("S-link-dy", None, None, edge_list, 1024, True, 0.5, 0.3, 0.2, seed=1234)
    assert all(len(part) == T for part in a) and all(len(part) == T - 1 for part in dy)
    assert all(torch.equal(x, y) for pa, pb in zip(a, b) for x, y in zip(pa, pb))           # one seed draws the same sets
    assert not all(torch.equal(x, y) for x, y in zip(a[0], c[0]))
    for t in range(T):
        e = edge_list[t].cpu().numpy()
        E = int((e[0] != e[1]).sum())
        keys = set((e[0] * n + e[1]).tolist()) | set((e[1] * n + e[0]).tolist())
        negs = []
        for k, ratio in enumerate((0.5, 0.3, 0.2)):
            idx, lab = a[2 * k][t].cpu().numpy(), a[2 * k + 1][t].cpu().numpy()
            cnt = int(np.floor(E * ratio))
            assert idx.shape == (2, 2 * cnt) and lab.tolist() == [1.0] * cnt + [0.0] * cnt            # counts are floor of the ratios
            pos, neg = idx[:, :cnt], idx[:, cnt:]
            assert all(int(p) in keys for p in pos[0] * n + pos[1]) and not np.any(pos[0] == pos[1])
            assert not np.any(neg[0] == neg[1])                                                       # no negative is a self-loop
            assert not any(int(q) in keys for q in neg[0] * n + neg[1])                               # nor an edge in either direction
            negs.append(neg)
        allneg = np.concatenate(negs, 1)
        unordered = np.minimum(allneg[0], allneg[1]) * n + np.maximum(allneg[0], allneg[1])
        assert len(set(unordered.tolist())) == allneg.shape[1]                                        # none is a duplicate, in either direction
    with pytest.raises(NotImplementedError):
        class Other(torch.nn.Module):
            method_name = "GCN"
        SupervisedEmbedding(_folders(tmp_path, T), "origin", "emb", ["a"], Other(), ClassificationLoss(2), InnerProduct(),
                            has_cuda=True).learn_embedding(adjs, xs, edge_list=edge_list, learning_type="S-link-st", epoch=1)
