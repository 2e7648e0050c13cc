"""Similarity-prediction evaluation on the GPU (ctgcn_sim.hip + ctgcn_amd/evaluation/similarity_prediction.py) against the
reference fixture similarity_uci.npz (the reference's own DataGenerator / SimilarityPredictor on the UCI months) and the scipy
statement of the algorithm in _sim_ref.py."""
import hashlib
import os

import numpy as np
import pandas as pd
import pytest
import scipy.sparse as sp
import scipy.stats
import torch

import importlib

import _lp_fixture
import _sim_ref
from ctgcn_amd import export

SIM = importlib.import_module("ctgcn_amd.evaluation.similarity_prediction")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "similarity_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
N = len(NAMES)


def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def _month(t):
    A = SIM.symmetric_csr_from_rows(SNAPSHOTS["t%d_src" % t], SNAPSHOTS["t%d_dst" % t], SNAPSHOTS["t%d_w" % t], N)
    A.eliminate_zeros()
    return A


def _dev(A):
    return (torch.from_numpy(A.indptr.astype(np.int32)).to(DEV), torch.from_numpy(A.indices.astype(np.int32)).to(DEV),
            torch.from_numpy(A.data.astype(np.float64)).to(DEV))


def _coo(sim):
    return tuple(x.cpu().numpy() for x in sim.coo())


def _emb(t):
    e = _lp_fixture.month_embedding(SNAPSHOTS, t, N)
    assert _lp_fixture.digest(e) == GOLD["emb_sha256"][t], "rebuilt embedding differs from what the reference was given"
    return e


def _diagnose(t, row, col, val):
    got = sp.coo_matrix((val, (row, col)), shape=(N, N)).tocsr()
    s = got[GOLD["sample_%d_row" % t], GOLD["sample_%d_col" % t]].A1
    ref = GOLD["sample_%d_data" % t]
    z = got[GOLD["zero_%d_row" % t], GOLD["zero_%d_col" % t]].A1
    return "sample: %d of %d differ (max rel %.3g); %d stored where the reference has zeros" % (
        (s != ref).sum(), len(ref), np.abs(s / ref - 1).max(), (z != 0).sum())


# ------------------------------------------------------------------------------------------------ 1. bit-identity on UCI
@pytest.mark.parametrize("t", range(7))
def test_uci_bit_identical_with_the_references_lambda(t):
    sim = SIM.vertex_similarity(*_dev(_month(t)), alpha=0.5, iter_num=100, lambda_1=float(GOLD["lambda_1"][t]))
    row, col, val = _coo(sim)
    assert row.dtype == np.int32 and col.dtype == np.int32 and val.dtype == np.float64
    assert len(val) == GOLD["nnz"][t], _diagnose(t, row, col, val)
    assert (_sha(row), _sha(col), _sha(val)) == (GOLD["sha_row"][t], GOLD["sha_col"][t], GOLD["sha_data"][t]), _diagnose(t, row, col, val)


# ------------------------------------------------------------------------------------------------ 2. own lambda_1, end to end
@pytest.mark.parametrize("t", [0, 1, 6])
def test_uci_with_the_ports_lambda(t):
    A = _month(t)
    pinned = SIM.vertex_similarity(*_dev(A), lambda_1=float(GOLD["lambda_1"][t]))
    own = SIM.vertex_similarity(*_dev(A))
    assert own.lambda_1 == SIM.host_lambda_1(A) and abs(own.lambda_1 / GOLD["lambda_1"][t] - 1) <= 1e-13
    rr, rc, rv = _coo(pinned)
    gr, gc, gv = _coo(own)
    rk, gk = rr.astype(np.int64) * N + rc, gr.astype(np.int64) * N + gc
    common, ri, gi = np.intersect1d(rk, gk, assume_unique=True, return_indices=True)
    # off the diagonal every value is a sum of positive terms: relative 1e-12.  A diagonal value is s_ii - 1 with s_ii >= 1, so a
    # change of lambda_1 in its last bits moves it by ulps of 1, not of the value: absolute 1e-12 there
    diag = rr[ri] == rc[ri]
    err = np.abs(gv[gi] - rv[ri])
    assert np.all(err[~diag] <= 1e-12 * np.abs(rv[ri][~diag]) + 1e-16) and np.all(err[diag] <= 1e-12)
    only = np.concatenate([np.delete(rv, ri), np.delete(gv, gi)])
    assert np.all(np.abs(only / 1e-6 - 1) <= 1e-9)                 # a pattern difference only at the threshold


# ------------------------------------------------------------------------------------------------ 3. random graphs against scipy
def _random_graph(seed):
    rng = np.random.default_rng(seed)
    n = 300
    src, dst, w = [], [], []
    core = np.arange(0, 150)                                        # a dense non-bipartite component: it holds lambda_1
    for _ in range(1200):
        u, v = rng.choice(core, 2)
        src.append(u), dst.append(v), w.append(float(rng.integers(1, 6)) * 0.75)
    src += [0, 0, 5, 7]                                             # duplicates (the last row wins) and a self loop
    dst += [1, 1, 5, 8]
    w += [3.0, 0.5, 9.0, 0.0]
    left, right = np.arange(160, 175), np.arange(175, 190)           # a bipartite component
    for _ in range(60):
        src.append(int(rng.choice(left))), dst.append(int(rng.choice(right))), w.append(float(rng.uniform(0.1, 0.4)))
    for k in range(200, 239):                                       # a path: the second component kind; 240..299 and 150..159 isolated
        src.append(k), dst.append(k + 1), w.append(1.0 + (k % 3))
    A = _sim_ref.adjacency(src, dst, w, n)
    return A


@pytest.mark.parametrize("seed", [1, 2])
def test_random_graphs_bit_identical_to_scipy(seed):
    A = _random_graph(seed)
    lam = SIM.host_lambda_1(A)
    assert lam > 0
    iters = 60
    ref = _sim_ref.similarity(A, lam, 0.5, iters)
    one = _coo(SIM.vertex_similarity(*_dev(A), alpha=0.5, iter_num=iters, lambda_1=lam))
    multi = _coo(SIM.vertex_similarity(*_dev(A), alpha=0.5, iter_num=iters, lambda_1=lam, panel_cols=37))
    again = _coo(SIM.vertex_similarity(*_dev(A), alpha=0.5, iter_num=iters, lambda_1=lam, panel_cols=37))
    for got in (one, multi, again):
        assert np.array_equal(got[0], ref.row) and np.array_equal(got[1], ref.col)
        assert np.array_equal(got[2].view(np.int64), ref.data.view(np.int64))
    assert not np.isin(np.arange(240, 300), ref.row).any() and not np.isin(np.arange(150, 160), ref.row).any()
    # the series' first steps as well (iter_num = 1 leaves S - I = 0: a constant matrix, refused)
    with pytest.raises(ValueError, match="constant"):
        SIM.vertex_similarity(*_dev(A), iter_num=1, lambda_1=lam)
    for it in (2, 3):
        r = _sim_ref.similarity(A, lam, 0.3, it)
        g = _coo(SIM.vertex_similarity(*_dev(A), alpha=0.3, iter_num=it, lambda_1=lam, panel_cols=64))
        assert np.array_equal(g[0], r.row) and np.array_equal(g[1], r.col) and np.array_equal(g[2].view(np.int64), r.data.view(np.int64))


# ------------------------------------------------------------------------------------------------ 4. spearman
def test_spearman_matches_scipy_with_ties():
    rng = np.random.default_rng(5)
    for n in (17, 1000, 300_000):
        x = rng.integers(0, 7, n).astype(np.float64) * 0.1
        y = np.where(rng.random(n) < 0.6, 0.0, rng.random(n))
        y[: n // 3] = x[: n // 3] * 2 + 0.5
        want = scipy.stats.spearmanr(x, y)[0]
        got = SIM.spearman(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV))
        assert abs(got - want) <= 1e-12, (n, got, want)
        assert SIM.spearman(torch.from_numpy(x).to(DEV), torch.from_numpy(y).to(DEV)) == got       # bit-identical repeat
    c = torch.full((50,), 0.3, dtype=torch.float64, device=DEV)
    assert np.isnan(SIM.spearman(c, torch.arange(50, dtype=torch.float64, device=DEV)))


# ------------------------------------------------------------------------------------------------ 5. reference values
def test_uci_spearman_values():
    for t in range(len(FILES)):
        e = _emb(t)
        sim = SIM.vertex_similarity(*_dev(_month(t)), lambda_1=float(GOLD["lambda_1"][t]))
        got = SIM.prediction_error(sim, torch.from_numpy(e).to(DEV), "d")
        assert got[0] == "d" and abs(got[1] - GOLD["sp_f32"][t]) <= 1e-9, (t, got[1], GOLD["sp_f32"][t])
        got = SIM.prediction_error(sim.to_scipy(), e.astype(np.float64), "d")
        assert abs(got[1] - GOLD["sp_f32"][t]) <= 1e-9
        rp, col, val = _dev(_month(t))
        assert abs(SIM.evaluate(torch.from_numpy(e).to(DEV), rp, col, val, lambda_1=float(GOLD["lambda_1"][t]))[1] - GOLD["sp_f32"][t]) <= 1e-9


def test_similarity_prediction_end_to_end(tmp_path, monkeypatch):
    # the table is pinned to the reference's lambda_1: the real block holds many values that are equal in exact arithmetic but
    # differ in their last bits, so lambda_1's last bits reorder them and move the correlation by up to 3e-7 (the port's own
    # lambda_1 is checked against the same table with that tolerance below)
    lams = iter([float(x) for x in GOLD["lambda_1"]])
    monkeypatch.setattr(SIM, "host_lambda_1", lambda A: next(lams))
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    names = np.asarray(NAMES, dtype=object)
    for t, f in enumerate(FILES):
        pd.DataFrame({"from_id": names[SNAPSHOTS["t%d_src" % t]], "to_id": names[SNAPSHOTS["t%d_dst" % t]],
                      "weight": SNAPSHOTS["t%d_w" % t]}).to_csv(os.path.join(base, "1.format", f), sep="\t", index=False)
    pd.DataFrame(NAMES).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb(t) for t in range(len(FILES))])), FILES, 0,
                          os.path.join(base, "2.embedding", "CTGCN-C"), NAMES)
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                similarity_data_folder="similarity_data", similarity_res_folder="similarity_res", file_sep="\t", generate=True,
                method_list=["CTGCN-C"], alpha=0.5, iter_num=100, worker=-1)
    SIM.similarity_prediction(args)
    for t, f in enumerate(FILES):
        z = np.load(os.path.join(base, "similarity_data", f.split('.')[0] + "_similarity.npz"))
        assert z["row"].dtype == np.int32 and z["col"].dtype == np.int32 and z["data"].dtype == np.float64
        assert str(z["format"].item()) in ("coo", "b'coo'")
        assert tuple(z["shape"]) == (N, N)
        assert abs(len(z["data"]) - GOLD["nnz"][t]) <= max(2, GOLD["nnz"][t] // 10 ** 5)
    out_path = os.path.join(base, "similarity_res", "CTGCN-C_mse_record.csv")
    out = pd.read_csv(out_path)
    assert list(out.columns) == ["date", "mse"]
    assert list(out["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
    assert np.abs(out["mse"].values - GOLD["table_mse"]).max() <= 1e-9
    assert np.abs(GOLD["sp_tsv"] - GOLD["table_mse"]).max() <= 1e-12
    assert next(lams, None) is None                                 # one lambda_1 per month, in the sorted walk
    # the dense .csv text the reference's predictor reads: the same table
    for f in FILES[:2]:
        date = f.split('.')[0]
        npz = os.path.join(base, "similarity_data", date + "_similarity.npz")
        np.savetxt(os.path.join(base, "similarity_data", date + "_similarity.csv"), sp.load_npz(npz).toarray())
        os.remove(npz)
    os.remove(out_path)
    args["generate"] = False
    SIM.similarity_prediction(args)
    out2 = pd.read_csv(out_path)
    assert list(out2["date"].astype(str)) == list(out["date"].astype(str))
    assert np.abs(out2["mse"].values - GOLD["table_mse"]).max() <= 1e-9


# ------------------------------------------------------------------------------------------------ 6. errors
def test_error_cases(tmp_path):
    rp = torch.zeros(6, dtype=torch.int32, device=DEV)
    empty = torch.zeros(0, dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="no edges"):
        SIM.vertex_similarity(rp, empty, empty.to(torch.float64))
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    pd.DataFrame(["a", "b", "c"]).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    pd.DataFrame({"from_id": ["a"], "to_id": ["a"], "weight": [1.0]}).to_csv(os.path.join(base, "1.format", "x.csv"), sep="\t", index=False)
    gen = SIM.DataGenerator(base, "1.format", "similarity_data", "nodes_set/nodes.csv")
    with pytest.raises(ValueError, match="x.csv"):
        gen.generate_node_similarity("x.csv")
    n = 1_000_000                                                   # config 5's size: 8 TB of n² values
    idx = torch.arange(n, dtype=torch.int32, device=DEV)
    rp = torch.cat([torch.zeros(1, dtype=torch.int32, device=DEV), torch.arange(1, n + 1, dtype=torch.int32, device=DEV)])
    col = (idx + 1) % n
    before = torch.cuda.memory_allocated(DEV)
    with pytest.raises(ValueError, match="GB of device memory"):
        SIM.vertex_similarity(rp, col, torch.ones(n, dtype=torch.float64, device=DEV), lambda_1=2.0)
    assert torch.cuda.memory_allocated(DEV) <= before + 8 * n      # nothing n²-sized was allocated
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        SIM.vertex_similarity(rp.cpu(), col.cpu(), torch.ones(n, dtype=torch.float64))
    with pytest.raises(ValueError, match="1e-6"):
        SIM.prediction_error(np.zeros((3, 3)), np.ones((3, 2)), "d")


def test_similarity_prediction_with_the_ports_lambda(tmp_path):
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    names = np.asarray(NAMES, dtype=object)
    for t, f in enumerate(FILES):
        pd.DataFrame({"from_id": names[SNAPSHOTS["t%d_src" % t]], "to_id": names[SNAPSHOTS["t%d_dst" % t]],
                      "weight": SNAPSHOTS["t%d_w" % t]}).to_csv(os.path.join(base, "1.format", f), sep="\t", index=False)
    pd.DataFrame(NAMES).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb(t) for t in range(len(FILES))])), FILES, 0,
                          os.path.join(base, "2.embedding", "CTGCN-C"), NAMES)
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                similarity_data_folder="similarity_data", similarity_res_folder="similarity_res", file_sep="\t", generate=True,
                method_list=["CTGCN-C"], alpha=0.5, iter_num=100, worker=-1)
    SIM.similarity_prediction(args)
    out = pd.read_csv(os.path.join(base, "similarity_res", "CTGCN-C_mse_record.csv"))
    assert list(out["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
    assert np.abs(out["mse"].values - GOLD["table_mse"]).max() <= 1e-6
