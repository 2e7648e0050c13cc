#!/usr/bin/env python3
"""Generate tests/golden/similarity_uci.npz by RUNNING the reference's similarity-prediction evaluation.

Like make_golden_cent.py, this script runs only in the build container (where the reference tree is): it imports the reference's
evaluation/similarity_prediction.py in-process with the same run-time shims and stores inputs and outputs as data, no source text.
Re-run:  python tests/golden/make_golden_sim.py   (needs the built library: the embeddings are written by ctgcn_amd.export)

Contents (the 7 bundled UCI months, alpha 0.5 and iter_num 100 as in config/uci.json; embeddings: tests/_lp_fixture.month_embedding):
  node_names, files             the node file and the snapshot file names
  lambda_1                      float64 [7]: the eigenvalue the reference's own eigsh call returned for each month
  nnz                           int64 [7]: stored entries of the reference's <date>_similarity.npz
  sha_row, sha_col, sha_data    [7]: sha256 of the saved row (int32), col (int32) and data (float64) arrays, in file order
  sample_<t>_{row,col,data}     a seeded sample of SAMPLE stored entries of month t (for diagnosis when a digest differs)
  zero_<t>_{row,col}            a seeded sample of ZEROS positions of month t that store nothing
  emb_sha256                    [7]: digests of the float32 embeddings written through ctgcn_amd.export
  sp_tsv                        [7]: get_prediction_error's Spearman value, embeddings read from the TSV as the reference reads them
  sp_f32                        [7]: the same with the float32 embeddings converted exactly to float64 (the in-memory path)
  table_dates, table_mse        the <method>_mse_record.csv the reference's similarity_prediction_all_time writes (it reads the
                                dense <date>_similarity.csv text, which this script writes with np.savetxt from the .npz first)
"""
import hashlib
import os
import shutil
import sys
import tempfile
import warnings

import numpy as np
import pandas as pd
import scipy.sparse as sp
import scipy.sparse.linalg

warnings.filterwarnings("ignore")
np.int = int  # shim 1 (make_golden.py)

REF = "/root/reference"
sys.path.insert(0, REF)
from evaluation.similarity_prediction import DataGenerator, SimilarityPredictor  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
import _lp_fixture  # noqa: E402
from ctgcn_amd import export  # noqa: E402
SEED = 20261015
METHOD = "CTGCN-C"
ALPHA, ITER = 0.5, 100
SAMPLE, ZEROS = 2048, 256


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    data = os.path.join(REF, "data", "uci")
    tmp = tempfile.mkdtemp()
    eigs = []
    real_eigsh = scipy.sparse.linalg.eigsh

    def eigsh(*a, **k):
        r = real_eigsh(*a, **k)
        eigs.append(float(r[0]))
        return r

    scipy.sparse.linalg.eigsh = eigsh
    try:
        shutil.copytree(os.path.join(data, "1.format"), os.path.join(tmp, "1.format"))
        shutil.copytree(os.path.join(data, "nodes_set"), os.path.join(tmp, "nodes_set"))
        files = sorted(os.listdir(os.path.join(tmp, "1.format")))
        names = pd.read_csv(os.path.join(tmp, "nodes_set", "nodes.csv"), names=['node'])['node'].tolist()
        n = len(names)
        out = {"node_names": np.array(names), "files": np.array(files)}

        gen = DataGenerator(tmp, "1.format", "similarity_data", "nodes_set/nodes.csv", file_sep='\t', alpha=ALPHA, iter_num=ITER)
        rng = np.random.default_rng(SEED)
        nnz, sr, sc, sd, dense = [], [], [], [], []
        for t, f in enumerate(files):
            gen.generate_node_similarity(f)
            date = f.split('.')[0]
            z = np.load(os.path.join(tmp, "similarity_data", date + "_similarity.npz"))
            row, col, val = z["row"], z["col"], z["data"]
            assert row.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float64
            nnz.append(len(val))
            sr.append(sha(row))
            sc.append(sha(col))
            sd.append(sha(val))
            pick = np.sort(rng.choice(len(val), min(SAMPLE, len(val)), replace=False))
            out["sample_%d_row" % t], out["sample_%d_col" % t], out["sample_%d_data" % t] = row[pick], col[pick], val[pick]
            S = sp.coo_matrix((val, (row, col)), shape=(n, n)).toarray()
            zr, zc = [], []
            while len(zr) < ZEROS:
                i, j = (int(x) for x in rng.integers(0, n, 2))
                if S[i, j] == 0:
                    zr.append(i)
                    zc.append(j)
            out["zero_%d_row" % t], out["zero_%d_col" % t] = np.array(zr, np.int32), np.array(zc, np.int32)
            np.savetxt(os.path.join(tmp, "similarity_data", date + "_similarity.csv"), S)
            dense.append(S)
            print("month", f, "nnz", len(val), "lambda_1", eigs[-1], flush=True)
        assert len(eigs) == len(files)
        out["lambda_1"] = np.array(eigs)
        out["nnz"] = np.array(nnz, np.int64)
        out["sha_row"], out["sha_col"], out["sha_data"] = np.array(sr), np.array(sc), np.array(sd)

        snapshots = np.load(os.path.join(OUT, "uci_snapshots.npz"))
        assert list(snapshots["node_names"]) == names and list(snapshots["files"]) == files
        embs = [_lp_fixture.month_embedding(snapshots, t, n, 128, SEED) for t in range(len(files))]
        lp = np.load(os.path.join(OUT, "link_prediction_uci.npz"))
        assert all(_lp_fixture.digest(embs[t]) == lp["emb_sha256"][t] for t in range(len(lp["emb_sha256"])))
        out["emb_sha256"] = np.array([_lp_fixture.digest(e) for e in embs])
        os.makedirs(os.path.join(tmp, "2.embedding", METHOD))
        for t, f in enumerate(files):
            export.write_embedding(os.path.join(tmp, "2.embedding", METHOD, f), embs[t], names, sep='\t')

        pred = SimilarityPredictor(tmp, "1.format", "2.embedding", "similarity_data", "similarity_res", "nodes_set/nodes.csv",
                                   file_sep='\t')
        pred.similarity_prediction_all_time(METHOD)
        table = pd.read_csv(os.path.join(tmp, "similarity_res", METHOD + "_mse_record.csv"))
        out["table_dates"] = np.array(table["date"].astype(str).tolist())
        out["table_mse"] = table["mse"].values.astype(np.float64)

        sp_tsv, sp_f32 = [], []
        for t, f in enumerate(files):
            tsv = pd.read_csv(os.path.join(tmp, "2.embedding", METHOD, f), sep='\t', index_col=0).loc[names].values
            sp_tsv.append(pred.get_prediction_error(METHOD, dense[t], tsv, "x")[1])
            sp_f32.append(pred.get_prediction_error(METHOD, dense[t], embs[t].astype(np.float64), "x")[1])
        out["sp_tsv"], out["sp_f32"] = np.array(sp_tsv), np.array(sp_f32)
        np.savez_compressed(os.path.join(OUT, "similarity_uci.npz"), **out)
    finally:
        scipy.sparse.linalg.eigsh = real_eigsh
        shutil.rmtree(tmp)


if __name__ == "__main__":
    main()
