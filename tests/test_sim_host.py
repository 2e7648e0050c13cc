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


# ------------------------------------------------------------------------------------------------ mirrors used by test_gpu_sim_shapes.py
NP_SUM_SIZES = [2, 7, 8, 9, 127, 128, 129, 136, 137, 4097, 8191, 8192, 8193, 16385, 2049 * 2049]


@pytest.mark.parametrize("N", NP_SUM_SIZES)
def test_np_sum_model_is_numpys_sum(N):
    """The Python model of numpy's float64 sum (chunks of 8192, pairwise down to blocks of 128 with 8 running sums) gives np.sum's
    bits at every boundary of that tree, for a 1-D array and for a square 2-D one.  The kernel is held to numpy directly; this test
    says whether a disagreement there comes from a numpy that sums in another order."""
    side = int(round(N ** 0.5))
    for draw in range(4 if N < 100_000 else 1):
        x = np.random.default_rng(1000 * draw + N).uniform(0.0, 1.0, N)
        want = _sim_ref.np_sum_model(x)
        assert want == x.sum() == np.sum(x)
        if side * side == N:
            assert want == x.reshape(side, side).sum()
        assert _sim_ref.normalize(x)[1][2] == _sim_ref.np_sum_model((x - x.min()) / (x.max() - x.min()))


def test_np_sum_model_depends_on_the_order():
    """The sizes above can tell the orders apart: a plain running sum, and a pairwise sum that is not cut into chunks of 8192,
    differ from numpy's on the same data."""
    x = np.random.default_rng(3).uniform(0.0, 1.0, 16385)
    running = 0.0
    for v in x.tolist():
        running = running + v
    assert running != x.sum()
    assert _sim_ref._np_pairwise(x.tolist()) != x.sum()


@pytest.mark.parametrize("pad_zero", [0, 1])
def test_finish_mirror_is_the_scipy_statement(pad_zero):
    """finish() on the block of the non-isolated vertices, with 0 joined to the extremes when isolated vertices exist, is the n x n
    statement of similarity()."""
    rng = np.random.default_rng(11)
    m, n = 9, 9 + 3 * pad_zero
    src, dst = np.triu_indices(m, 1)
    pick = rng.random(len(src)) < 0.4
    pick[:m - 1] = True                                           # vertex 0 is joined to all: no isolated vertex inside the block
    A = _sim_ref.adjacency(src[pick], dst[pick], rng.uniform(0.5, 2.0, pick.sum()), n)
    lam = SIM.host_lambda_1(A)
    want = _sim_ref.similarity(A, lam, 0.5, 7).toarray()
    S = np.zeros((n, n))
    for _ in range(7):
        S = (0.5 / lam) * A.dot(S) + np.eye(n)
    got, (mn, mx), nnz = _sim_ref.finish(S[:m, :m], pad_zero, 1e-6)
    assert np.array_equal(got, want[:m, :m]) and not want[m:].any() and not want[:, m:].any()
    assert np.array_equal(nnz, np.count_nonzero(want[:m, :m], axis=1))


def test_spearman_sums_mirror_matches_scipy():
    import scipy.stats
    rng = np.random.default_rng(2)
    for N in (2, 3, 257, 4097):
        x = rng.permutation(N).astype(np.float64)
        y = rng.integers(0, 5, N).astype(np.float64)
        y[0], y[-1] = -1.0, 9.0
        sxy, sxx, syy = _sim_ref.spearman_sums(x, y)
        rx, ry = scipy.stats.rankdata(x), scipy.stats.rankdata(y)
        mu = (N + 1) / 2
        assert (sxy, sxx, syy) == (((rx - mu) * (ry - mu)).sum(), ((rx - mu) ** 2).sum(), ((ry - mu) ** 2).sum())
        assert abs(sxy / np.sqrt(sxx * syy) - scipy.stats.spearmanr(x, y)[0]) <= 1e-14
    assert _sim_ref.spearman_sums(np.full(5, 0.3), np.arange(5.0))[1] == 0.0
