"""Centrality-prediction evaluation on the GPU (ctgcn_cent.hip + ctgcn_amd/evaluation/centrality_prediction.py) against the reference
fixture centrality_uci.npz (the reference's own DataGenerator / CentralityPredictor on the UCI months) and the numpy reference
_central_ref.py.  No networkx or sklearn here."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import importlib

import _central_ref as R
import _lp_fixture
from ctgcn_amd import export

CP = importlib.import_module("ctgcn_amd.evaluation.centrality_prediction")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "centrality_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
N = len(NAMES)
ALPHAS = [float(a) for a in GOLD["alpha_list"]]
KINDS = ["closeness", "betweenness", "eigenvector", "kcore"]


def _month_csr(t):
    return R.csr(N, np.stack([SNAPSHOTS["t%d_src" % t], SNAPSHOTS["t%d_dst" % t]], 1))


def _dev(indptr, indices):
    return torch.from_numpy(np.asarray(indptr, np.int32)).to(DEV), torch.from_numpy(np.asarray(indices, np.int32)).to(DEV)


def _emb_np(t):
    e = _lp_fixture.month_embedding(SNAPSHOTS, t, N)
    assert _lp_fixture.digest(e) == GOLD["emb_sha256"][t], "rebuilt embedding differs from what the reference was given"
    return e


def _check_against_gold(c, gold, stop, t):
    assert np.array_equal(c["closeness"], gold[:, 0]), "month %d closeness" % t
    bmax = np.abs(gold[:, 1]).max()
    assert np.abs(c["betweenness"] - gold[:, 1]).max() <= 1e-10 * bmax, "month %d betweenness" % t
    assert np.abs(c["eigenvector"] - gold[:, 2]).max() <= 1e-12, "month %d eigenvector" % t
    assert np.array_equal(c["kcore"], gold[:, 3].astype(np.int64)), "month %d kcore" % t


# ------------------------------------------------------------------------------------------------ ground truth vs the reference
def test_uci_months_match_reference():
    for t in range(len(FILES)):
        rp, col = _dev(*_month_csr(t))
        c = {k: v.cpu().numpy() for k, v in CP.centralities(rp, col, n=N).items()}
        _check_against_gold(c, GOLD["cent_%d" % t], GOLD["eig_stop"][t], t)
        assert CP.eigenvector(rp, col)[1] == GOLD["eig_stop"][t]


def test_eigenvector_raises_one_step_short():
    t = int(np.argmax(GOLD["eig_stop"]))
    rp, col = _dev(*_month_csr(t))
    stop = int(GOLD["eig_stop"][t])
    assert CP.eigenvector(rp, col, max_iter=stop)[1] == stop
    with pytest.raises(CP.PowerIterationFailedConvergence):
        CP.eigenvector(rp, col, max_iter=stop - 1)
    with pytest.raises(CP.PowerIterationFailedConvergence):
        CP.centralities(rp, col, kinds=("eigenvector",), max_iter=stop - 1)


def test_repeated_calls_are_bit_identical():
    rp, col = _dev(*_month_csr(3))
    a = CP.centralities(rp, col)
    b = CP.centralities(rp, col)
    assert all(torch.equal(a[k], b[k]) for k in KINDS)
    X = torch.from_numpy(_emb_np(3)).to(DEV)
    Y = torch.stack([a[k].to(torch.float64) for k in KINDS], 1)
    e1 = CP.ridge_cv_errors(X, Y, ALPHAS, 5)
    e2 = CP.ridge_cv_errors(X, Y, ALPHAS, 5)
    assert np.array_equal(e1, e2)


# ------------------------------------------------------------------------------------------------ Brandes vs the numpy reference
def _check_brandes(n, indptr, indices, sources=None):
    rp, col = _dev(indptr, indices)
    s0, s1 = (0, n) if sources is None else (int(sources[0]), int(sources[-1]) + 1)
    bc, r, D = CP.brandes(rp, col, s0, s1)
    ref_bc, ref_r, ref_D = R.brandes(indptr, indices, n, sources=np.arange(s0, s1))
    assert np.array_equal(r.cpu().numpy(), ref_r) and np.array_equal(D.cpu().numpy(), ref_D)
    assert np.abs(bc.cpu().numpy() - ref_bc).max() <= 1e-10 * max(np.abs(ref_bc).max(), 1.0)
    return bc


@pytest.mark.parametrize("n,hub_frac", [(5000, 0.3)])
def test_power_law_with_hub_all_sources(n, hub_frac):
    indptr, indices = R.power_law(n, 3, seed=n, hub_frac=hub_frac)
    assert indptr[1] - indptr[0] >= n // 4
    _check_brandes(n, indptr, indices)
    rp, col = _dev(indptr, indices)
    x, stop = CP.eigenvector(rp, col)
    ref_x, ref_stop = R.eigenvector(indptr, indices, n)
    assert stop == ref_stop and np.abs(x.cpu().numpy() - ref_x).max() <= 1e-12


def test_power_law_20k_source_range():
    n = 20000
    indptr, indices = R.power_law(n, 4, seed=11, hub_frac=0.25)
    assert indptr[1] - indptr[0] >= n // 4
    _check_brandes(n, indptr, indices, sources=np.arange(0, 768))           # the hub's BFS and 767 more, tail vertices included
    _check_brandes(n, indptr, indices, sources=np.arange(n - 300, n))       # the isolated tail and low-degree sources


def test_path_5000_closed_form():
    n = 5000
    rp, col = _dev(*R.path(n))
    bc, r, D = CP.brandes(rp, col)
    i = np.arange(n, dtype=np.int64)
    assert np.array_equal(bc.cpu().numpy(), (2 * i * (n - 1 - i)).astype(np.float64))
    assert np.array_equal(r.cpu().numpy(), np.full(n, n)) and np.array_equal(D.cpu().numpy(), i * (i + 1) // 2 + (n - 1 - i) * (n - i) // 2)


def test_diamond_chain_beyond_2_to_53_paths():
    n, (indptr, indices) = R.diamonds(70)                 # 2^70 shortest paths end to end
    bc = _check_brandes(n, indptr, indices).cpu().numpy()
    assert bc[1] > 0 and bc[1] == bc[2]


@pytest.mark.parametrize("n", [1, 2, 3, 50])
def test_edgeless_and_tiny_graphs(n):
    for indptr, indices in (R.csr(n, np.zeros((0, 2), np.int64)), R.path(n)):
        rp, col = _dev(indptr, indices)
        x, stop = R.eigenvector(indptr, indices, n)
        kinds = ("degree", "closeness", "betweenness", "kcore") + (("eigenvector",) if stop is not None else ())
        c = {k: v.cpu().numpy() for k, v in CP.centralities(rp, col, kinds=kinds).items()}
        bc, r, D = R.brandes(indptr, indices, n)
        assert np.array_equal(c["closeness"], R.closeness(r, D, n))
        assert np.abs(c["betweenness"] - (R.betweenness(indptr, indices, n))).max() <= 1e-12
        if stop is None:                    # the 50-vertex path: networkx raises as well
            with pytest.raises(CP.PowerIterationFailedConvergence):
                CP.eigenvector(rp, col)
        else:
            assert np.abs(c["eigenvector"] - x).max() <= 1e-12 and CP.eigenvector(rp, col)[1] == stop
        deg = np.diff(indptr).astype(np.float64)
        assert np.array_equal(c["degree"], deg * (1.0 / (n - 1.0)) if n > 1 else np.ones(n))
        assert c["kcore"].max(initial=0) == (1 if indices.size else 0)


# ------------------------------------------------------------------------------------------------ ridge
@pytest.mark.parametrize("d", [37, 128, 500])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_ridge_matches_numpy_gram_form(d, dtype):
    rng = np.random.default_rng(d)
    n = 2003
    X = (rng.standard_normal((n, d)) * 0.3 + 0.1).astype(np.float32 if dtype == torch.float32 else np.float64)
    Y = np.stack([X @ rng.standard_normal(d) * 0.1 + rng.random(n), rng.random(n), np.round(rng.random(n) * 5), rng.random(n) ** 4], 1)
    ours = CP.ridge_cv_errors(torch.from_numpy(X).to(DEV), torch.from_numpy(Y).to(DEV), ALPHAS, 5)
    ref = R.ridge_cv_errors(X.astype(np.float64), Y, ALPHAS, 5)
    assert np.abs(ours / ref - 1).max() <= 1e-8


def test_ridge_zero_mean_target_gives_numpy_value():
    X = torch.randn(100, 8, device=DEV, dtype=torch.float64)
    Y = torch.stack([torch.zeros(100, device=DEV, dtype=torch.float64), torch.rand(100, device=DEV, dtype=torch.float64)], 1)
    e = CP.ridge_cv_errors(X, Y, [1.0], 5)
    assert np.isnan(e[0, 0]) and np.isfinite(e[0, 1])
    assert CP.min_over_alphas(e)[0] == float("inf")


def test_ridge_refuses_d_over_512():
    with pytest.raises(Exception, match="unsupported"):
        CP.ridge_cv_errors(torch.zeros(50, 513, device=DEV), torch.ones(50, 4, device=DEV), [1.0], 5)


def test_in_memory_fp32_errors_match_reference():
    for t in range(len(FILES)):
        X = torch.from_numpy(_emb_np(t)).to(DEV)
        Y = torch.from_numpy(GOLD["cent_%d" % t]).to(DEV)
        e = CP.ridge_cv_errors(X, Y, ALPHAS, 5)
        ref = GOLD["err_f32"][t]
        assert np.abs(e / ref - 1).max() <= 1e-8, t
        rp, col = _dev(*_month_csr(t))
        mse = CP.evaluate(X, rp, col, ALPHAS, 5, date="d")
        assert mse[0] == "d"
        assert np.abs(np.array(mse[1:]) / ref.min(0) - 1).max() <= 1e-8, t


# ------------------------------------------------------------------------------------------------ end to end through the files
def test_centrality_prediction_end_to_end(tmp_path):
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    names = np.asarray(NAMES, dtype=object)
    for t, f in enumerate(FILES):
        pd.DataFrame({"from_id": names[SNAPSHOTS["t%d_src" % t]], "to_id": names[SNAPSHOTS["t%d_dst" % t]],
                      "weight": SNAPSHOTS["t%d_w" % t]}).to_csv(os.path.join(base, "1.format", f), sep="\t", index=False)
    pd.DataFrame(NAMES).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb_np(t) for t in range(len(FILES))])), FILES, 0,
                          os.path.join(base, "2.embedding", "CTGCN-C"), NAMES)
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                centrality_data_folder="centrality_data", centrality_res_folder="centrality_res", file_sep="\t", generate=True,
                method_list=["CTGCN-C"], alpha_list=ALPHAS, split_fold=5, worker=-1)
    CP.centrality_prediction(args)
    for t, f in enumerate(FILES):
        df = pd.read_csv(os.path.join(base, "centrality_data", f.split('.')[0] + "_centrality.csv"), sep="\t", float_precision="round_trip")
        assert list(df.columns) == ["node"] + KINDS
        assert np.array_equal(df["node"].values, np.arange(N))
        _check_against_gold({k: df[k].values for k in KINDS}, GOLD["cent_%d" % t], GOLD["eig_stop"][t], t)
    out = pd.read_csv(os.path.join(base, "centrality_res", "CTGCN-C_mse_record.csv"))
    assert list(out.columns) == ["date"] + KINDS
    assert list(out["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
    ref = GOLD["table_mse"]
    assert np.abs(out[KINDS].values / ref - 1).max() <= 1e-8
    assert np.abs(GOLD["err_tsv"].min(1) / ref - 1).max() <= 1e-12     # the table is the per-alpha minimum
    # an existing <date>_centrality.csv is kept
    path = os.path.join(base, "centrality_data", FILES[0].split('.')[0] + "_centrality.csv")
    before = os.path.getmtime(path)
    CP.DataGenerator(base, "1.format", "centrality_data", "nodes_set/nodes.csv").generate_node_samples(FILES[0])
    assert os.path.getmtime(path) == before
