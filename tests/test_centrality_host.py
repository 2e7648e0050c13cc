"""CPU-only checks of the centrality-prediction host logic (ctgcn_amd/evaluation/centrality_prediction.py) and of the tests' numpy
reference (_central_ref.py) against networkx and sklearn, plus the ABI 31 surface."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _central_ref as R
from ctgcn_amd import _lib

try:                                  # only the tests that compare against them need networkx / sklearn (pytest.importorskip there)
    import networkx as nx
except ImportError:
    nx = None

CP = importlib.import_module("ctgcn_amd.evaluation.centrality_prediction")
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "centrality_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))


def _nx_graph(n, indptr, indices):
    g = nx.Graph()
    g.add_nodes_from(range(n))
    for u in range(n):
        g.add_edges_from((u, int(v)) for v in indices[indptr[u]:indptr[u + 1]])
    return g


def _graphs():
    rng = np.random.default_rng(7)
    out = [(n, R.path(n)) for n in (1, 2, 3, 7)]
    out += [(9, R.star(9)), R.cliques([4, 5, 3], isolated=4), R.diamonds(6), (40, R.power_law(40, 2, 3))]
    for n, p in ((30, 0.08), (25, 0.3), (60, 0.02)):
        a = np.triu(rng.random((n, n)) < p, 1)
        out.append((n, R.csr(n, np.argwhere(a))))
    out.append((5, R.csr(5, np.zeros((0, 2), np.int64))))
    return out


@pytest.mark.parametrize("case", range(len(_graphs())))
def test_numpy_reference_matches_networkx(case):
    pytest.importorskip("networkx")
    n, (indptr, indices) = _graphs()[case]
    g = _nx_graph(n, indptr, indices)
    bc, r, D = R.brandes(indptr, indices, n, batch=5)
    clo = nx.closeness_centrality(g)
    assert np.array_equal(R.closeness(r, D, n), np.array([clo[v] for v in range(n)]))     # bit-identical: the same float operations
    btw = nx.betweenness_centrality(g)
    ref = np.array([btw[v] for v in range(n)])
    got = bc * (1 / ((n - 1) * (n - 2))) if n > 2 else bc
    assert np.abs(got - ref).max() <= 1e-12 * max(ref.max(), 1.0)
    x, stop = R.eigenvector(indptr, indices, n)
    if stop is None:
        with pytest.raises(nx.PowerIterationFailedConvergence):
            nx.eigenvector_centrality(g)
    else:
        eig = nx.eigenvector_centrality(g)
        assert np.abs(x - np.array([eig[v] for v in range(n)])).max() <= 1e-14
        nx.eigenvector_centrality(g, max_iter=stop)
        with pytest.raises(nx.PowerIterationFailedConvergence):
            nx.eigenvector_centrality(g, max_iter=stop - 1)
    assert CP.closeness_from_counts(r, D, n).tolist() == R.closeness(r, D, n).tolist()


def test_diamond_chain_path_counts_pass_2_to_53():
    pytest.importorskip("networkx")
    n, (indptr, indices) = R.diamonds(60)           # 2^60 shortest paths end to end
    bc, r, D = R.brandes(indptr, indices, n, sources=[0])
    assert r[0] == n and D[0] == sum(2 * (2 * i + 1) + 2 * (i + 1) for i in range(60))
    btw = nx.betweenness_centrality(_nx_graph(n, indptr, indices))
    assert np.abs(R.betweenness(indptr, indices, n) - np.array([btw[v] for v in range(n)])).max() <= 1e-12


def test_fold_layout_matches_kfold():
    sklearn_ms = pytest.importorskip("sklearn.model_selection")
    for n, k in ((1899, 5), (10, 5), (13, 5), (7, 3)):
        b = CP.fold_bounds(n, k)
        assert np.array_equal(b, R.kfold_bounds(n, k))
        for f, (_, test) in enumerate(sklearn_ms.KFold(k).split(np.zeros(n))):
            assert np.array_equal(test, np.arange(b[f], b[f + 1]))


@pytest.mark.parametrize("d", [3, 37, 128])
def test_gram_form_ridge_matches_cross_val_predict(d):
    sklearn_lm = pytest.importorskip("sklearn.linear_model")
    sklearn_ms = pytest.importorskip("sklearn.model_selection")
    rng = np.random.default_rng(d)
    n = 523
    X = rng.standard_normal((n, d)) * 0.3 + 0.2
    Y = np.stack([X @ rng.standard_normal(d) + rng.standard_normal(n), rng.random(n), np.round(rng.random(n) * 4)], 1)
    alphas = [0.05, 1.0, 10.0]
    ours = R.ridge_cv_errors(X, Y, alphas, 5)
    ref = np.zeros_like(ours)
    for a, alpha in enumerate(alphas):
        for t in range(Y.shape[1]):
            pred = sklearn_ms.cross_val_predict(sklearn_lm.Ridge(alpha=alpha), X, Y[:, t], cv=5)
            ref[a, t] = ((Y[:, t] - pred) ** 2).mean() / Y[:, t].mean()
    assert np.abs(ours - ref).max() <= 1e-10 * np.abs(ref).max()
    # the product's host solve (ridge_weights) on the same Grams, on CPU tensors
    b = R.kfold_bounds(n, 5)
    Z = np.hstack([X, np.ones((n, 1)), Y])
    grams = torch.from_numpy(np.stack([Z[b[f]:b[f + 1], :d + 1].T @ Z[b[f]:b[f + 1]] for f in range(5)]))
    W = CP.ridge_weights(grams, d, alphas).numpy()                  # [F, |alpha| * T, d + 1]
    for f in range(5):
        for a in range(len(alphas)):
            for t in range(Y.shape[1]):
                w = W[f, a * Y.shape[1] + t]
                pred = X[b[f]:b[f + 1]] @ w[:d] + w[d]
                ref_pred = sklearn_lm.Ridge(alpha=alphas[a]).fit(np.delete(X, np.s_[b[f]:b[f + 1]], 0),
                                                                 np.delete(Y[:, t], np.s_[b[f]:b[f + 1]])).predict(X[b[f]:b[f + 1]])
                assert np.abs(pred - ref_pred).max() <= 1e-9 * max(1.0, np.abs(ref_pred).max())


def test_min_over_alphas_follows_python_min():
    e = np.array([[3.0, np.nan, np.inf], [2.0, np.nan, 1.0], [5.0, 0.5, np.nan]])
    assert CP.min_over_alphas(e) == [2.0, 0.5, 1.0]
    assert CP.min_over_alphas(np.array([[np.nan], [np.nan]])) == [float("inf")]


def test_betweenness_scale_and_closeness_formula():
    assert CP.betweenness_scale(2) is None and CP.betweenness_scale(1) is None
    assert CP.betweenness_scale(5) == 1 / 12
    r, D = np.array([1, 3, 4]), np.array([0, 3, 7])
    assert CP.closeness_from_counts(r, D, 10).tolist() == [0.0, (2 / 3) * (2 / 9), (3 / 7) * (3 / 9)]
    assert CP.closeness_from_counts(np.array([1]), np.array([0]), 1).tolist() == [0.0]


def _reference_graph(path, names, sep='\t'):
    df = pd.read_csv(path, sep=sep)
    if df.shape[1] == 2:
        df['weight'] = 1.0
    g = nx.from_pandas_edgelist(df, "from_id", "to_id", edge_attr='weight', create_using=nx.Graph)
    g.add_nodes_from(names)
    g.remove_edges_from(nx.selfloop_edges(g))
    return g


def _structure(g, names):
    idx = {v: i for i, v in enumerate(names)}
    return sorted((min(idx[u], idx[v]), max(idx[u], idx[v])) for u, v in g.edges())


@pytest.mark.parametrize("header,rows", [
    ("from_id\tto_id\tweight", ["a\tb\t1", "b\ta\t0", "c\tc\t2", "c\td\t0", "d\te\t3.5", "d\te\t0", "a\tb\t2"]),
    ("from_id\tto_id", ["a\tb", "b\tc", "a\tb", "e\te", "b\ta"]),
])
def test_csr_structure_equals_reference_graph(tmp_path, header, rows):
    pytest.importorskip("networkx")
    names = ["a", "b", "c", "d", "e", "f"]
    path = tmp_path / "2004-05.csv"
    path.write_text("\n".join([header] + rows) + "\n")
    rp, col = CP.graph_csr(str(path), names)
    g = _reference_graph(str(path), names)
    assert len(rp) == len(names) + 1 and g.number_of_nodes() == len(names)
    ours = sorted((u, int(v)) for u in range(len(names)) for v in col[rp[u]:rp[u + 1]] if u < v)
    assert ours == _structure(g, names)
    for u in range(len(names)):                       # symmetric, sorted, no self loops
        row = col[rp[u]:rp[u + 1]]
        assert np.all(np.diff(row) > 0) and u not in row
        assert all(u in col[rp[v]:rp[v + 1]] for v in row)


def test_csr_structure_of_uci_months_equals_reference_graph(tmp_path):
    pytest.importorskip("networkx")
    names = [str(v) for v in GOLD["node_names"]]
    for t, f in enumerate(GOLD["files"]):
        df = pd.DataFrame({"from_id": np.asarray(names)[SNAPSHOTS["t%d_src" % t]], "to_id": np.asarray(names)[SNAPSHOTS["t%d_dst" % t]]})
        cols = [c for c in SNAPSHOTS.files if c.startswith("t%d_" % t) and c not in ("t%d_src" % t, "t%d_dst" % t)]
        if cols:
            df["weight"] = SNAPSHOTS[cols[0]]
        path = tmp_path / str(f)
        df.to_csv(str(path), sep='\t', index=False)
        rp, col = CP.graph_csr(str(path), names)
        ours = sorted((u, int(v)) for u in range(len(names)) for v in col[rp[u]:rp[u + 1]] if u < v)
        assert ours == _structure(_reference_graph(str(path), names), names)


def test_unknown_node_raises_value_error(tmp_path):
    path = tmp_path / "x.csv"
    path.write_text("from_id\tto_id\na\tzz\n")
    with pytest.raises(ValueError, match="not in the node file"):
        CP.graph_csr(str(path), ["a", "b"])


def test_numpy_reference_reproduces_golden_months():
    n = len(GOLD["node_names"])
    for t in range(len(GOLD["files"])):
        indptr, indices = R.csr(n, np.stack([SNAPSHOTS["t%d_src" % t], SNAPSHOTS["t%d_dst" % t]], 1))
        gold = GOLD["cent_%d" % t]
        bc, r, D = R.brandes(indptr, indices, n)
        assert np.array_equal(R.closeness(r, D, n), gold[:, 0])
        b = bc * (1 / ((n - 1) * (n - 2)))
        assert np.abs(b - gold[:, 1]).max() <= 1e-10 * gold[:, 1].max()
        x, stop = R.eigenvector(indptr, indices, n)
        assert stop == GOLD["eig_stop"][t]
        assert np.abs(x - gold[:, 2]).max() <= 1e-12


def test_cent_symbols_in_abi_31():
    assert _lib.ABI_VERSION == 31
    for name in ("ctgcn_cent_brandes", "ctgcn_cent_brandes_workspace_bytes", "ctgcn_cent_eigenvector",
                 "ctgcn_cent_eigenvector_workspace_bytes", "ctgcn_ridge_gram_f32", "ctgcn_ridge_gram_f64", "ctgcn_ridge_gram_workspace_bytes",
                 "ctgcn_ridge_sse_f32", "ctgcn_ridge_sse_f64", "ctgcn_ridge_sse_workspace_bytes"):
        assert name in _lib.SIGNATURES
        assert hasattr(_lib.load(), name)
    lib = _lib.load()
    assert lib.ctgcn_cent_brandes_workspace_bytes(1000, 0, 1000) >= 1000 * 36
    assert lib.ctgcn_ridge_gram_workspace_bytes(128, 4, 5) >= 5 * 129 * 133 * 8
    assert lib.ctgcn_cent_brandes(10, None, None, 0, 10, None, None, None, None, 0, None) == -1          # CTGCN_E_INVALID
    assert lib.ctgcn_ridge_gram_f32(100, 513, 4, 5, 1, 513, 1, 1, 1, 1 << 30, None) == -4               # CTGCN_E_UNSUPPORTED: d > 512


def test_cpu_tensors_fail_loudly():
    rp = torch.tensor([0, 1, 2], dtype=torch.int32)
    col = torch.tensor([1, 0], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.centralities(rp, col)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        CP.ridge_cv_errors(torch.zeros(10, 4), torch.ones(10, 4), [1.0])


# ------------------------------------------------------------------------------------------------ mirrors used by test_gpu_cent_shapes.py
def test_layered_graph_has_the_stated_levels():
    n, (indptr, indices), levels = R.layered(isolated=6)
    assert n == sum(R.LAYER_SIZES) + 6
    A = R.adjacency(indptr, indices, n)
    assert (A != A.T).nnz == 0 and A.diagonal().sum() == 0
    dist = np.full(n, -1)
    dist[0], front, k = 0, np.array([0]), 0
    while len(front):                                              # a plain BFS, apart from R.brandes
        k += 1
        nxt = np.unique(np.concatenate([indices[indptr[v]:indptr[v + 1]] for v in front]))
        front = nxt[dist[nxt] < 0]
        dist[front] = k
    assert np.array_equal(dist, levels)
    assert [int((dist == k).sum()) for k in range(len(R.LAYER_SIZES))] == list(R.LAYER_SIZES)
    deg = np.diff(indptr)
    assert np.all(deg[levels >= 0] > 0) and not deg[levels < 0].any()
    # rows shorter and longer than 16 lanes where a level gets 16 lanes per vertex, and a row of more than 64 for a single source
    assert deg[levels == 5].min() < 16 < deg[levels == 5].max() and deg[levels == 10].min() > 64
    bc, r, D = R.brandes(indptr, indices, n, sources=[0, n - 1])
    assert r.tolist() == [n - 6, 1] and D.tolist() == [int((np.arange(len(R.LAYER_SIZES)) * R.LAYER_SIZES).sum()), 0]


def test_star_closed_form_is_the_references():
    """What test_gpu_cent_shapes.py asserts at 120 001 vertices, on a star small enough for R.brandes: from the hub every leaf is at
    distance 1 and nothing lies between; from a leaf the hub is at 1 and the other n - 2 leaves at 2, each reached through the hub
    alone, so the hub's dependency is n - 2."""
    n, k = 50, 7
    bc, r, D = R.brandes(*R.star(n), n, sources=np.arange(k))
    want = np.zeros(n)
    want[0] = (k - 1) * (n - 2)
    assert np.array_equal(bc, want) and np.array_equal(r, np.full(k, n))
    assert np.array_equal(D, [n - 1] + [1 + 2 * (n - 2)] * (k - 1))


def test_long_double_ridge_mirrors():
    rng = np.random.default_rng(5)
    n, d, T, F, P = 37, 6, 3, 4, 5
    X, Y = rng.standard_normal((n, d)), rng.random((n, T))
    Z = np.hstack([X, np.ones((n, 1)), Y])
    b = R.kfold_bounds(n, F)
    for f, (g, absg, rows) in enumerate(R.fold_grams(X, Y, F)):
        Zf = Z[b[f]:b[f + 1]]
        assert rows == len(Zf) and g.dtype == np.longdouble and g.shape == (d + 1, d + 1 + T)
        assert np.all(np.abs(Zf[:, :d + 1].T @ Zf - g) <= rows * 2.0 ** -52 * absg)
        assert g[d, d] == rows
    W = rng.standard_normal((F, P, d + 1))
    tgt = [2, 0, 0, 1, 2]
    sse, bound = R.fold_sse(X, Y, W, tgt, F, chain=n)
    for f in range(F):
        Xf, Yf = X[b[f]:b[f + 1]], Y[b[f]:b[f + 1]]
        for p in range(P):
            plain = ((Yf[:, tgt[p]] - (Xf @ W[f, p, :d] + W[f, p, d])) ** 2).sum()
            assert abs(plain - sse[f, p]) <= bound[f, p] <= 1e-13 * sse[f, p]
            short = ((Yf[1:, tgt[p]] - (Xf[1:] @ W[f, p, :d] + W[f, p, d])) ** 2).sum()      # one row dropped: far outside the bound
            assert abs(short - sse[f, p]) > 1e6 * bound[f, p]
