#!/usr/bin/env python3
"""Generate tests/golden/centrality_uci.npz by RUNNING the reference's centrality-prediction evaluation.

Like make_golden_lp.py, this script runs only in the build container (where the reference tree is): it imports the reference's
evaluation/centrality_prediction.py in-process with the same run-time shims and stores inputs and outputs as data, no source text.
Re-run:  python tests/golden/make_golden_cent.py   (needs the built library: the embeddings are written by ctgcn_amd.export)

Contents (the 7 bundled UCI months; embeddings: tests/_lp_fixture.month_embedding of every month, digests in emb_sha256):
  node_names, files             the node file and the snapshot file names
  cent_<t>                      float64 [n, 4]: the reference DataGenerator's <date>_centrality.csv of month t (closeness,
                                betweenness, eigenvector, kcore), read back exactly (float_precision='round_trip')
  eig_stop                      int64 [7]: networkx's eigenvector stop step (the smallest max_iter that does not raise)
  alpha_list, split_fold        the shipped settings
  emb_sha256                    [7]: digests of the float32 embeddings written through ctgcn_amd.export
  err_tsv                       [7, |alpha|, 4]: get_prediction_error with one alpha at a time, embeddings read from the TSV as the
                                reference reads them (float64, index_col=0)
  err_f32                       the same with the float32 embeddings converted exactly to float64 (the in-memory path)
  table_dates, table_mse        the <method>_mse_record.csv the reference's CentralityPredictor writes
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
from evaluation.centrality_prediction import CentralityPredictor, DataGenerator  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import _lp_fixture  # noqa: E402
from ctgcn_amd import export  # noqa: E402
SEED = 20261015
ALPHAS = [0.05, 0.5, 1, 2, 5, 10]
METHOD = "CTGCN-C"


def eig_stop_step(graph):
    for k in range(1, 101):
        try:
            nx.eigenvector_centrality(graph, max_iter=k)
            return k
        except nx.PowerIterationFailedConvergence:
            pass
    raise RuntimeError("no stop within 100 steps")


def main():
    data = os.path.join(REF, "data", "uci")
    tmp = tempfile.mkdtemp()
    try:
        shutil.copytree(os.path.join(data, "1.format"), os.path.join(tmp, "1.format"))
        shutil.copytree(os.path.join(data, "nodes_set"), os.path.join(tmp, "nodes_set"))
        files = sorted(os.listdir(os.path.join(tmp, "1.format")))
        names = pd.read_csv(os.path.join(tmp, "nodes_set", "nodes.csv"), names=['node'])['node'].tolist()
        n = len(names)
        out = {"node_names": np.array(names), "files": np.array(files), "alpha_list": np.array(ALPHAS), "split_fold": np.array(5)}

        gen = DataGenerator(tmp, "1.format", "centrality_data", "nodes_set/nodes.csv", file_sep='\t')
        gen.generate_all_node_samples(sep='\t')
        stops = []
        for t, f in enumerate(files):
            date = f.split('.')[0]
            out["cent_%d" % t] = pd.read_csv(os.path.join(tmp, "centrality_data", date + "_centrality.csv"), sep='\t',
                                             float_precision='round_trip').iloc[:, 1:].values
            df = pd.read_csv(os.path.join(tmp, "1.format", f), sep='\t')
            if df.shape[1] == 2:
                df['weight'] = 1.0
            g = nx.from_pandas_edgelist(df, "from_id", "to_id", edge_attr='weight', create_using=nx.Graph)
            g.add_nodes_from(names)
            g.remove_edges_from(nx.selfloop_edges(g))
            stops.append(eig_stop_step(g))
        out["eig_stop"] = np.array(stops, dtype=np.int64)

        snapshots = np.load(os.path.join(OUT, "uci_snapshots.npz"))
        assert list(snapshots["node_names"]) == names and list(snapshots["files"]) == files
        embs = [_lp_fixture.month_embedding(snapshots, t, n, 128, SEED) for t in range(len(files))]
        lp = np.load(os.path.join(OUT, "link_prediction_uci.npz"))
        assert all(_lp_fixture.digest(embs[t]) == lp["emb_sha256"][t] for t in range(len(lp["emb_sha256"])))
        out["emb_sha256"] = np.array([_lp_fixture.digest(e) for e in embs])
        os.makedirs(os.path.join(tmp, "2.embedding", METHOD))
        for t, f in enumerate(files):
            export.write_embedding(os.path.join(tmp, "2.embedding", METHOD, f), embs[t], names, sep='\t')

        pred = CentralityPredictor(tmp, "1.format", "2.embedding", "centrality_data", "centrality_res", "nodes_set/nodes.csv", file_sep='\t',
                                   alpha_list=ALPHAS, split_fold=5)
        pred.centrality_prediction_all_time(METHOD)
        table = pd.read_csv(os.path.join(tmp, "centrality_res", METHOD + "_mse_record.csv"))
        out["table_dates"] = np.array(table["date"].astype(str).tolist())
        out["table_mse"] = table[["closeness", "betweenness", "eigenvector", "kcore"]].values

        err_tsv = np.zeros((len(files), len(ALPHAS), 4))
        err_f32 = np.zeros_like(err_tsv)
        for t, f in enumerate(files):
            cent = out["cent_%d" % t]
            tsv = pd.read_csv(os.path.join(tmp, "2.embedding", METHOD, f), sep='\t', index_col=0).loc[names].values
            for a, alpha in enumerate(ALPHAS):
                pred.alpha_list = [alpha]
                err_tsv[t, a] = pred.get_prediction_error(cent, tsv, "x")[1:]
                err_f32[t, a] = pred.get_prediction_error(cent, embs[t].astype(np.float64), "x")[1:]
            print("month", f, "done", flush=True)
        out["err_tsv"], out["err_f32"] = err_tsv, err_f32
        np.savez_compressed(os.path.join(OUT, "centrality_uci.npz"), **out)
    finally:
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
