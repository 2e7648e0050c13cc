"""Similarity-prediction host logic (no GPU): the C ABI's argument checks, the snapshot matrix, the host lambda_1 against the
reference's values (tests/golden/similarity_uci.npz) and the file layer of SimilarityPredictor."""
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import torch

import importlib

import _sim_ref
from ctgcn_amd import _lib

SIM = importlib.import_module("ctgcn_amd.evaluation.similarity_prediction")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "similarity_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
N = len(NAMES)


def test_sim_symbols_and_invalid_arguments():
    assert _lib.ABI_VERSION == 31
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctgcn_hip.h")).read()
    for name in ("ctgcn_sim_panel_cols", "ctgcn_sim_series_workspace_bytes", "ctgcn_sim_series", "ctgcn_sim_finish_workspace_bytes",
                 "ctgcn_sim_finish", "ctgcn_sim_coo", "ctgcn_sim_gram_f32", "ctgcn_sim_gram_f64", "ctgcn_sim_normalize_workspace_bytes",
                 "ctgcn_sim_normalize", "ctgcn_sim_spearman_workspace_bytes", "ctgcn_sim_spearman"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert "%s(" % name in header
    assert lib.ctgcn_sim_panel_cols(1436, 20000) == 1436                 # UCI: one panel
    p = lib.ctgcn_sim_panel_cols(87036, 1060568)
    assert 64 <= p < 87036 and p % 64 == 0 and 2 * 8 * 87036 * p + 12 * 1060568 <= 200 << 20
    assert lib.ctgcn_sim_series_workspace_bytes(100, 40) == 2 * 8 * 100 * 40
    assert lib.ctgcn_sim_series_workspace_bytes(100, 400) == 2 * 8 * 100 * 100
    q = 1     # never dereferenced: every call below fails its argument check first
    assert lib.ctgcn_sim_series(0, q, q, q, 0.1, 100, 4, 0, 0, q, q, 1 << 30, None) == -1          # m < 1
    assert lib.ctgcn_sim_series(10, q, q, q, 0.1, 0, 4, 0, 10, q, q, 1 << 30, None) == -1          # iter_num < 1
    assert lib.ctgcn_sim_series(10, q, q, q, 0.1, 100, 4, 0, 11, q, q, 1 << 30, None) == -1        # col1 > m
    assert lib.ctgcn_sim_series(10, None, q, q, 0.1, 100, 4, 0, 10, q, q, 1 << 30, None) == -1     # null row_ptr
    assert lib.ctgcn_sim_series(10, q, q, q, 0.1, 100, 4, 0, 10, q, q, 2 * 8 * 10 * 4 - 1, None) == -3   # workspace
    assert lib.ctgcn_sim_finish(10, 1, 1e-6, q, q, q, q, 0, None) == -3
    assert lib.ctgcn_sim_finish(0, 1, 1e-6, q, q, q, q, 1 << 30, None) == -1
    assert lib.ctgcn_sim_coo(10, q, q, q, q, q, None, None) == -1
    assert lib.ctgcn_sim_gram_f32(10, 0, q, 4, q, q, None) == -1                                   # d < 1
    assert lib.ctgcn_sim_gram_f64(10, 8, q, 4, q, q, None) == -1                                   # lde < d
    assert lib.ctgcn_sim_normalize(100, q, q, q, 0, None) == -3
    assert lib.ctgcn_sim_spearman(100, q, q, q, q, q, q, lib.ctgcn_sim_spearman_workspace_bytes(100) - 1, None) == -3
    assert lib.ctgcn_sim_spearman(0, q, q, q, q, q, q, 1 << 30, None) == -1


def test_snapshot_matrix_is_the_references(tmp_path):
    names = ["a", "b", "c", "d", "e", "f"]
    rows = [("a", "b", 2.5), ("b", "c", 1.0), ("c", "c", 7.0), ("b", "a", 4.0), ("d", "e", 0.0), ("e", "f", 3.0), ("f", "e", 0.0),
            ("c", "d", 0.5), ("a", "f", -1.5), ("d", "c", 0.25)]
    path = str(tmp_path / "snap.csv")
    pd.DataFrame(rows, columns=["from_id", "to_id", "weight"]).to_csv(path, sep="\t", index=False)
    A = SIM.graph_csr(path, names)
    idx = {v: i for i, v in enumerate(names)}
    R = _sim_ref.adjacency([idx[r[0]] for r in rows], [idx[r[1]] for r in rows], [r[2] for r in rows], len(names))
    assert A.has_sorted_indices and R.has_sorted_indices
    assert np.array_equal(A.indptr, R.indptr) and np.array_equal(A.indices, R.indices) and np.array_equal(A.data, R.data)
    assert A[0, 1] == 4.0 and A[4, 5] == 0 and A.nnz == 8      # last row wins, zero weights and self loops store nothing
    with pytest.raises(ValueError, match="not in the node file"):
        SIM.graph_csr(path, names[:-1])


@pytest.mark.parametrize("t", range(7))
def test_host_lambda_1_matches_the_reference(t):
    A = _sim_ref.adjacency(SNAPSHOTS["t%d_src" % t], SNAPSHOTS["t%d_dst" % t], SNAPSHOTS["t%d_w" % t], N)
    B = SIM.symmetric_csr_from_rows(SNAPSHOTS["t%d_src" % t], SNAPSHOTS["t%d_dst" % t], SNAPSHOTS["t%d_w" % t], N)
    B.eliminate_zeros()
    assert np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and np.array_equal(A.data, B.data)
    lam = SIM.host_lambda_1(A)
    assert abs(lam / GOLD["lambda_1"][t] - 1) <= 1e-13
    assert SIM.host_lambda_1(A) == lam                          # fixed start vector: repeatable


def test_argument_checks_without_gpu():
    rp = torch.tensor([0, 1, 2], dtype=torch.int32)
    col = torch.tensor([1, 0], dtype=torch.int32)
    val = torch.ones(2, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SIM.vertex_similarity(rp, col, val)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SIM.spearman(val, val)
    with pytest.raises(AssertionError):
        SIM.vertex_similarity(rp, col, val, alpha=1.0)
    with pytest.raises(AssertionError):
        SIM.vertex_similarity(rp, col, val, alpha=0.0)


def _layout(tmp_path, months, embedded):
    base = str(tmp_path)
    for d in ("1.format", "nodes_set", os.path.join("2.embedding", "M"), "similarity_data"):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    pd.DataFrame(["a", "b", "c"]).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    for f in months:
        pd.DataFrame({"from_id": ["a"], "to_id": ["b"], "weight": [1.0]}).to_csv(os.path.join(base, "1.format", f), sep="\t", index=False)
    for f in embedded:
        pd.DataFrame({"x": [1.0, 2.0, 3.0]}, index=["c", "a", "b"]).to_csv(os.path.join(base, "2.embedding", "M", f), sep="\t")
    return base


def test_file_layer(tmp_path, monkeypatch):
    months = ["2001-03.csv", "2001-01.csv", "2001-02.csv"]
    base = _layout(tmp_path, months, ["2001-01.csv", "2001-03.csv"])
    S = np.array([[0.0, 0.5, 0.0], [0.5, 0.0, 0.0], [0.0, 0.0, 0.0]])
    sp.save_npz(os.path.join(base, "similarity_data", "2001-01_similarity.npz"), sp.coo_matrix(S))
    sp.save_npz(os.path.join(base, "similarity_data", "2001-02_similarity.npz"), sp.coo_matrix(S))
    np.savetxt(os.path.join(base, "similarity_data", "2001-03_similarity.csv"), 2 * S)
    seen = []

    def fake(node_sim_mat, embedding, date=None, device=None):
        seen.append((date, sp.issparse(node_sim_mat), np.asarray(node_sim_mat.todense() if sp.issparse(node_sim_mat) else node_sim_mat),
                     np.asarray(embedding)))
        return [date, 0.25]

    monkeypatch.setattr(SIM, "prediction_error", fake)
    pred = SIM.SimilarityPredictor(base, "1.format", "2.embedding", "similarity_data", "similarity_res", "nodes_set/nodes.csv")
    pred.similarity_prediction_all_time("M")
    assert [s[0] for s in seen] == ["2001-01", "2001-03"]          # sorted walk; the month without an embedding is skipped
    assert seen[0][1] and not seen[1][1]                            # .npz read as sparse, .csv fallback read densely
    assert np.array_equal(seen[0][2], S) and np.array_equal(seen[1][2], 2 * S)
    assert np.array_equal(seen[0][3].ravel(), [2.0, 3.0, 1.0])      # embedding rows in node-file order
    out = pd.read_csv(os.path.join(base, "similarity_res", "M_mse_record.csv"))
    assert list(out.columns) == ["date", "mse"] and list(out["date"]) == ["2001-01", "2001-03"] and list(out["mse"]) == [0.25, 0.25]
    os.remove(os.path.join(base, "similarity_data", "2001-02_similarity.npz"))
    with pytest.raises(FileNotFoundError, match="2001-02"):
        pred.similarity_prediction_all_time("M")
    with pytest.raises(AssertionError):
        SIM.DataGenerator(base, "1.format", "similarity_data", "nodes_set/nodes.csv", alpha=1.5)
