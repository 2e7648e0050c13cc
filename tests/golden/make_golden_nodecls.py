#!/usr/bin/env python3
"""Generate tests/golden/node_classification_uci.npz by RUNNING the reference's node-classification evaluation.

Like make_golden_lp.py, this script runs only where the reference tree is: it imports the reference's
evaluation/node_classification.py in-process and stores inputs and outputs as data, no source text.  Files are walked in sorted
order (os.listdir is wrapped), the order the port uses.  Re-run:  python tests/golden/make_golden_nodecls.py

Contents (the 7 bundled UCI months; labels from tests/_nc_fixture.month_labels; embeddings from tests/_lp_fixture.month_embedding):
  node_names, files, C_list        the node file, the snapshot file names, the Air configs' C list (max_iter 10000)
  emb_sha256                       [7]: digests of the float32 embeddings the reference was given (rebuilt by the tests)
  labels_<t>_{node,label}          the label file of month t (node index, label), in file order
  split_<r>_<t>_<part>_{node,label} the reference DataGenerator's <date>_<part>.csv of repetition r under np.random.seed(SEED)
  table_dates, table_acc           [REPS, 7]: the reference NodeClassifier's <method>_acc_record.csv of each repetition
  agg_columns, agg_values          the aggregate_results table
  tight_coef                       float32 [REPS, 7, |C|, 4, 129]: OvR fits at tol=1e-12 (w then b), the exact optima
  tight_val_acc / tight_test_acc   [REPS, 7, |C|]; tight_best [REPS, 7]: chosen C index (last of ties)
  tight_{val,test}_pred / _margin  per split row (rows of (r, t) consecutive) and C: predicted class and top-two probability margin
  shipped_val_acc / shipped_test_acc  the same fits at sklearn's shipped tol (1e-4); tol_gap: max |shipped - tight| accuracy,
                                   per C and over the reference's tables (whose chosen C may differ from the tight one)
  edge_<case>_*                    tiny cases run through the reference's NodeClassifier.train / test: k2 (two classes), absent (a
                                   class missing from train: the constant predictor), ties (equal val accuracy across C)
"""
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
import pandas as pd

warnings.filterwarnings("ignore")
REF = "/root/reference"
sys.path.insert(0, REF)
_listdir = os.listdir
os.listdir = lambda p=".": sorted(_listdir(p))
from evaluation.node_classification import DataGenerator, NodeClassifier, aggregate_results  # noqa: E402
from sklearn import preprocessing  # noqa: E402
from sklearn.linear_model import LogisticRegression  # noqa: E402
from sklearn.multiclass import OneVsRestClassifier  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _lp_fixture  # noqa: E402
import _nc_fixture  # noqa: E402
SEED = 20261016
C_LIST = [0.01, 0.1, 1, 5, 10, 20]
REPS = 2
METHOD = "CTGCN-C"


def ovr(C, tol, X, Y):
    lr = LogisticRegression(C=C, solver='lbfgs', max_iter=10000 if tol >= 1e-4 else 200000, tol=tol, class_weight='balanced')
    return OneVsRestClassifier(lr).fit(X, Y)


def scored(model, lb, X, y):
    pr = model.predict_proba(X)
    pred = np.argmax(pr, 1)
    s = np.sort(pr, 1)
    return float(np.mean(pred == y)), pred, s[:, -1] - s[:, -2]


def edge_case(K, n, d, seed, absent=None, sep=3.0):
    rng = np.random.RandomState(seed)
    y = rng.randint(0, K, n)
    centers = rng.randn(K, d) * sep
    emb = (centers[y] + rng.randn(n, d)).astype(np.float32)
    idx = rng.permutation(n)
    tr, va, te = idx[:n * 6 // 10], idx[n * 6 // 10:n * 8 // 10], idx[n * 8 // 10:]
    if absent is not None:
        keep = y[tr] != absent
        tr = tr[keep]
    nodes = np.stack([np.arange(n), y], 1)
    nc = NodeClassifier.__new__(NodeClassifier)
    nc.C_list, nc.max_iter = C_LIST, 10000
    lb = preprocessing.LabelBinarizer()
    lb.fit(np.arange(K))
    model = nc.train(nodes[tr], nodes[va], emb.astype(np.float64), lb)
    acc = NodeClassifier.test(nodes[te], emb.astype(np.float64), model, lb, "d")[1]
    val = []
    for C in C_LIST:
        m = ovr(C, 1e-12, emb.astype(np.float64)[tr], lb.transform(y[tr]))
        val.append(scored(m, lb, emb.astype(np.float64)[va], y[va])[0])
    return {"emb": emb, "y": y, "train": tr, "val": va, "test": te, "K": np.array(K), "ref_acc": np.array(acc),
            "ref_C": np.array(model.estimators_[0].C if hasattr(model.estimators_[0], "C") else model.estimators_[-1].C),
            "tight_val_acc": np.array(val)}


def main():
    data = os.path.join(REF, "data", "uci")
    tmp = tempfile.mkdtemp()
    try:
        shutil.copytree(os.path.join(data, "1.format"), os.path.join(tmp, "1.format"))
        shutil.copytree(os.path.join(data, "nodes_set"), os.path.join(tmp, "nodes_set"))
        files = sorted(os.listdir(os.path.join(tmp, "1.format")))
        names = pd.read_csv(os.path.join(tmp, "nodes_set", "nodes.csv"), names=['node'])['node'].tolist()
        n, d = len(names), 128
        snapshots = np.load(os.path.join(OUT, "uci_snapshots.npz"))
        assert list(snapshots["node_names"]) == names and list(snapshots["files"]) == files
        out = {"node_names": np.array(names), "files": np.array(files), "C_list": np.array(C_LIST)}
        os.makedirs(os.path.join(tmp, "nodes_label"))
        os.makedirs(os.path.join(tmp, "2.embedding", METHOD))
        embs, labels = [], []
        for t, f in enumerate(files):
            nodes, lab = _nc_fixture.month_labels(snapshots, t)
            labels.append((nodes, lab))
            out["labels_%d_node" % t], out["labels_%d_label" % t] = nodes.astype(np.uint16), lab.astype(np.uint8)
            pd.DataFrame({'node': [names[i] for i in nodes], 'label': lab}).to_csv(os.path.join(tmp, "nodes_label", f), sep='\t', index=False)
            e = _lp_fixture.month_embedding(snapshots, t, n, d, SEED)
            embs.append(e)
            pd.DataFrame(e, index=names).to_csv(os.path.join(tmp, "2.embedding", METHOD, f), sep='\t')
        out["emb_sha256"] = np.array([_lp_fixture.digest(e) for e in embs])

        np.random.seed(SEED)
        for r in range(REPS):
            gen = DataGenerator(tmp, "1.format", "nodecls_data_%d" % r, "nodes_set/nodes.csv", "nodes_label", file_sep='\t',
                                train_ratio=0.7, val_ratio=0.2, test_ratio=0.1)
            gen.generate_node_samples_all_time(sep='\t')
            nc = NodeClassifier(tmp, "1.format", "2.embedding", "nodecls_data_%d" % r, "nodecls_res_%d" % r, "nodes_set/nodes.csv",
                                "nodes_label", file_sep='\t', C_list=C_LIST, max_iter=10000)
            nc.node_classification_all_method([METHOD])
            print("rep", r, "reference done", flush=True)
        aggregate_results(tmp, "nodecls_res", 0, REPS, [METHOD])
        tables = [pd.read_csv(os.path.join(tmp, "nodecls_res_%d" % r, METHOD + "_acc_record.csv")) for r in range(REPS)]
        out["table_dates"] = np.array(tables[0]["date"].astype(str).tolist())
        out["table_acc"] = np.stack([tb["acc"].values for tb in tables])
        agg = pd.read_csv(os.path.join(tmp, "nodecls_res", METHOD + "_acc_record.csv"))
        out["agg_columns"] = np.array(list(agg.columns))
        out["agg_values"] = agg.iloc[:, 1:].values

        T, G = len(files), len(C_LIST)
        out["tight_coef"] = np.zeros((REPS, T, G, 4, d + 1), np.float32)
        for tag in ("tight", "shipped"):
            out[tag + "_val_acc"] = np.zeros((REPS, T, G))
            out[tag + "_test_acc"] = np.zeros((REPS, T, G))
        out["tight_best"] = np.zeros((REPS, T), np.int64)
        preds = {"val": [], "test": []}
        lb = preprocessing.LabelBinarizer()
        lb.fit(np.arange(4))
        for r in range(REPS):
            for t, f in enumerate(files):
                date = f.split('.')[0]
                sp = {p: pd.read_csv(os.path.join(tmp, "nodecls_data_%d" % r, date + '_' + p + '.csv'), sep='\t').values
                      for p in ('train', 'val', 'test')}
                for p, v in sp.items():
                    out["split_%d_%d_%s_node" % (r, t, p)] = v[:, 0].astype(np.uint16)
                    out["split_%d_%d_%s_label" % (r, t, p)] = v[:, 1].astype(np.uint8)
                X = embs[t].astype(np.float64)
                pv, pt = [], []
                for ci, C in enumerate(C_LIST):
                    for tag, tol in (("tight", 1e-12), ("shipped", 1e-4)):
                        model = ovr(C, tol, X[sp['train'][:, 0]], lb.transform(sp['train'][:, 1]))
                        va = scored(model, lb, X[sp['val'][:, 0]], sp['val'][:, 1])
                        te = scored(model, lb, X[sp['test'][:, 0]], sp['test'][:, 1])
                        out[tag + "_val_acc"][r, t, ci], out[tag + "_test_acc"][r, t, ci] = va[0], te[0]
                        if tag == "tight":
                            for k, est in enumerate(model.estimators_):
                                out["tight_coef"][r, t, ci, k] = np.r_[est.coef_[0], est.intercept_[0]]
                            pv.append(va[1:])
                            pt.append(te[1:])
                best, bi = 0, -1
                for ci, a in enumerate(out["tight_val_acc"][r, t]):
                    if a >= best:
                        best, bi = a, ci
                out["tight_best"][r, t] = bi
                preds["val"].append((np.stack([x[0] for x in pv], 1), np.stack([x[1] for x in pv], 1)))
                preds["test"].append((np.stack([x[0] for x in pt], 1), np.stack([x[1] for x in pt], 1)))
                print("rep", r, "month", date, "done", flush=True)
        for p in ("val", "test"):
            out["tight_%s_pred" % p] = np.concatenate([a for a, _ in preds[p]]).astype(np.uint8)
            out["tight_%s_margin" % p] = np.concatenate([b for _, b in preds[p]]).astype(np.float32)
        # the chosen C can differ between the two tolerances: bound the table entries as well as the per-C accuracies
        tight_table = np.take_along_axis(out["tight_test_acc"], out["tight_best"][..., None], 2)[..., 0]
        out["tol_gap"] = np.array(max(np.abs(out["shipped_val_acc"] - out["tight_val_acc"]).max(),
                                      np.abs(out["shipped_test_acc"] - out["tight_test_acc"]).max(),
                                      np.abs(out["table_acc"] - tight_table).max()))
        for name, kw in (("k2", dict(K=2, n=120, d=8, seed=1, sep=0.6)), ("absent", dict(K=4, n=160, d=8, seed=2, absent=3, sep=0.8)),
                         ("ties", dict(K=3, n=90, d=6, seed=3, sep=6.0))):
            for k, v in edge_case(**kw).items():
                out["edge_%s_%s" % (name, k)] = v
        np.savez_compressed(os.path.join(OUT, "node_classification_uci.npz"), **out)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
