#!/usr/bin/env python3
"""Generate tests/golden/link_prediction_uci.npz by RUNNING the reference's link-prediction evaluation.

Like make_golden.py, this script runs only in the build container (where the reference tree is): it imports the reference's
evaluation/link_prediction.py in-process with the same run-time shims and stores inputs and outputs as data, no source text.
Re-run:  python tests/golden/make_golden_lp.py

Contents (months t = 1..6 of the bundled UCI data are predicted from the embedding of month t-1):
  node_names, files             the node file and the snapshot file names
  emb_sha256                    [6]: digests of the float32 embeddings of months 0..5 the reference was given.  The embeddings are
                                not stored: tests/_lp_fixture.month_embedding rebuilds them bit for bit from uci_snapshots.npz
  split_<t>_<part>_{pos,neg}    the reference DataGenerator's splits under np.random.seed(SEED), part in train / val / test: positive
                                and negative rows as tests/_lp_fixture.encode_rows (decode_split restores [n, 3], positives first)
  counts                        int64 [7, 4]: lines, train_num, val_num, test_num per month
  C_list, measures              the shipped settings (max_iter 10000)
  ref_val_auc / ref_test_auc    [6, 4, |C|]: LogisticRegression(C, lbfgs, class_weight='balanced', tol=1e-4): roc_auc_score of
                                predict_proba[:, 1] on the val / test split
  ref_best                      [6, 4]: the reference's chosen C index (last of ties)
  tight_val_auc / tight_test_auc / tight_best   the same with tol=1e-12 (the exact optima)
  tight_coef / tight_intercept  float32 [6, 4, |C|, 128] / [6, 4, |C|]: those optima
  sigmoid_auc                   [6]: the 'sigmoid' measure's test AUC
  table_dates, table_auc        the <method>_auc_record.csv the reference's LinkPredictor writes (measures Avg Had L1 L2 sigmoid)
  auc_ties_*                    roc_auc_score on tied scores
"""
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
import pandas as pd
import scipy.sparse as sp
import networkx as nx

warnings.filterwarnings("ignore")
np.int = int  # shim 1 (make_golden.py)
nx.to_scipy_sparse_matrix = lambda G, nodelist=None: sp.csr_matrix(nx.to_scipy_sparse_array(G, nodelist=nodelist))  # shim 2

REF = "/root/reference"
sys.path.insert(0, REF)
from evaluation.link_prediction import DataGenerator, LinkPredictor  # noqa: E402
from sklearn.linear_model import LogisticRegression  # noqa: E402
from sklearn.metrics import roc_auc_score  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
import _lp_fixture  # noqa: E402
SEED = 20261015
C_LIST = [0.01, 0.1, 1, 10]
MEASURES = ["Avg", "Had", "L1", "L2"]
METHOD = "CTGCN-C"


def main():
    data = os.path.join(REF, "data", "uci")
    tmp = tempfile.mkdtemp()
    try:
        shutil.copytree(os.path.join(data, "1.format"), os.path.join(tmp, "1.format"))
        shutil.copytree(os.path.join(data, "nodes_set"), os.path.join(tmp, "nodes_set"))
        files = sorted(os.listdir(os.path.join(tmp, "1.format")))
        names = pd.read_csv(os.path.join(tmp, "nodes_set", "nodes.csv"), names=['node'])['node'].tolist()
        idx = {v: i for i, v in enumerate(names)}
        n, d = len(names), 128
        out = {"node_names": np.array(names), "files": np.array(files), "C_list": np.array(C_LIST), "measures": np.array(MEASURES)}

        np.random.seed(SEED)
        gen = DataGenerator(tmp, "1.format", "lp_data_0", "nodes_set/nodes.csv", file_sep='\t', train_ratio=0.5, val_ratio=0.3,
                            test_ratio=0.2)
        gen.generate_edge_samples_all_time(sep='\t')

        snapshots = np.load(os.path.join(OUT, "uci_snapshots.npz"))
        assert list(snapshots["node_names"]) == names and list(snapshots["files"]) == files
        embs, counts = [], []
        for t, f in enumerate(files):
            df = pd.read_csv(os.path.join(tmp, "1.format", f), sep='\t')
            assert (df.iloc[:, 0].map(idx).values == snapshots["t%d_src" % t]).all()
            date = f.split('.')[0]
            sizes = [len(pd.read_csv(os.path.join(tmp, "lp_data_0", date + '_' + p + '.csv'), sep='\t')) // 2 for p in ('train', 'val', 'test')]
            counts.append([len(df)] + sizes)
            if t < len(files) - 1:
                embs.append(_lp_fixture.month_embedding(snapshots, t, n, d, SEED))
        out["counts"] = np.array(counts, dtype=np.int64)
        out["emb_sha256"] = np.array([_lp_fixture.digest(e) for e in embs])
        os.makedirs(os.path.join(tmp, "2.embedding", METHOD))
        for t in range(len(files) - 1):      # the reference trainer's save_embedding format
            pd.DataFrame(embs[t], index=names).to_csv(os.path.join(tmp, "2.embedding", METHOD, files[t]), sep='\t')

        pred = LinkPredictor(tmp, "1.format", "2.embedding", "lp_data_0", "lp_res_0", "nodes_set/nodes.csv", file_sep='\t', C_list=C_LIST,
                             measure_list=MEASURES + ["sigmoid"], max_iter=10000)
        pred.link_prediction_all_time(METHOD)
        table = pd.read_csv(os.path.join(tmp, "lp_res_0", METHOD + "_auc_record.csv"))
        out["table_dates"] = np.array(table["date"].astype(str).tolist())
        out["table_auc"] = table[MEASURES + ["sigmoid"]].values

        T, K = len(files) - 1, len(C_LIST)
        for tag, tol in (("ref", 1e-4), ("tight", 1e-12)):
            out[tag + "_coef"] = np.zeros((T, 4, K, d))
            out[tag + "_intercept"] = np.zeros((T, 4, K))
            out[tag + "_val_auc"] = np.zeros((T, 4, K))
            out[tag + "_test_auc"] = np.zeros((T, 4, K))
            out[tag + "_best"] = np.zeros((T, 4), dtype=np.int64)
        out["sigmoid_auc"] = np.zeros(T)
        pred.measure_list = MEASURES + ["sigmoid"]
        for t in range(1, len(files)):
            date = files[t].split('.')[0]
            sp_ = {p: pd.read_csv(os.path.join(tmp, "lp_data_0", date + '_' + p + '.csv'), sep='\t').values for p in ('train', 'val', 'test')}
            for p, v in sp_.items():
                h = len(v) // 2
                assert (v[:h, 2] == 1).all() and (v[h:, 2] == 0).all()
                out["split_%d_%s_pos" % (t, p)] = _lp_fixture.encode_rows(v[:h, :2], n)
                out["split_%d_%s_neg" % (t, p)] = _lp_fixture.encode_rows(v[h:, :2], n)
            emb = embs[t - 1].astype(np.float64)
            feats = {p: pred.get_edge_feature(v, emb) for p, v in sp_.items()}
            out["sigmoid_auc"][t - 1] = roc_auc_score(sp_['test'][:, 2], feats['test']['sigmoid'])
            for mi, m in enumerate(MEASURES):
                for tag, tol in (("ref", 1e-4), ("tight", 1e-12)):
                    best, best_i = 0, -1
                    for ci, C in enumerate(C_LIST):
                        model = LogisticRegression(C=C, solver='lbfgs', max_iter=10000 if tag == "ref" else 200000, tol=tol,
                                                   class_weight='balanced')
                        model.fit(feats['train'][m], sp_['train'][:, 2])
                        out[tag + "_coef"][t - 1, mi, ci] = model.coef_[0]
                        out[tag + "_intercept"][t - 1, mi, ci] = model.intercept_[0]
                        va = roc_auc_score(sp_['val'][:, 2], model.predict_proba(feats['val'][m])[:, 1])
                        out[tag + "_val_auc"][t - 1, mi, ci] = va
                        out[tag + "_test_auc"][t - 1, mi, ci] = roc_auc_score(sp_['test'][:, 2], model.predict_proba(feats['test'][m])[:, 1])
                        if va >= best:
                            best, best_i = va, ci
                    out[tag + "_best"][t - 1, mi] = best_i
            print("month", date, "done", flush=True)

        rng = np.random.default_rng(SEED)
        y = rng.integers(0, 2, 500)
        s = np.round(rng.random(500) * 8) / 8       # heavy ties
        out["auc_ties_y"], out["auc_ties_s"], out["auc_ties_auc"] = y, s, np.array(roc_auc_score(y, s))
        del out["ref_coef"], out["ref_intercept"]
        out["tight_coef"] = out["tight_coef"].astype(np.float32)
        out["tight_intercept"] = out["tight_intercept"].astype(np.float32)
        np.savez_compressed(os.path.join(OUT, "link_prediction_uci.npz"), **out)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
