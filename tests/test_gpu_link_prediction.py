"""Link-prediction evaluation on the GPU (ctgcn_eval.hip + ctgcn_amd/evaluation) against float64 autograd and the reference fixture
link_prediction_uci.npz (the reference's own splits, sklearn fits at the shipped tol and at tol=1e-12)."""
import os
import time

import numpy as np
import pandas as pd
import pytest
import torch

import importlib

import _lp_fixture
from ctgcn_amd import export
from ctgcn_amd.evaluation import _logreg

LP = importlib.import_module("ctgcn_amd.evaluation.link_prediction")   # the package also exports the function link_prediction

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "link_prediction_uci.npz"))
T = len(GOLD["files"]) - 1
C_LIST = [float(c) for c in GOLD["C_list"]]
MEASURES = [str(m) for m in GOLD["measures"]]
N = len(GOLD["node_names"])
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))


def _split(t, part):
    return torch.from_numpy(_lp_fixture.decode_split(GOLD, t, part, N)).to(DEV)


def _emb_np(t):
    e = _lp_fixture.month_embedding(SNAPSHOTS, t, N)
    assert _lp_fixture.digest(e) == GOLD["emb_sha256"][t], "rebuilt embedding differs from what the reference was given"
    return e


def _emb(t):
    return torch.from_numpy(_emb_np(t)).to(DEV)


# ------------------------------------------------------------------------------------------------ sampler
def _keys(n, edges):
    e = torch.tensor(edges, dtype=torch.int64, device=DEV).reshape(-1, 2)
    return LP.membership_keys(torch.cat([e, e.flip(1)]), n)


def test_sampler_valid_exact_and_deterministic():
    g = torch.randint(0, 500, (4000, 2), generator=torch.Generator().manual_seed(3))
    keys = _keys(500, g.tolist())
    a = LP.sample_negatives(keys, 500, 123457, seed=11, device=DEV)
    assert a.shape == (123457, 2)
    assert (a[:, 0] != a[:, 1]).all()
    ks = set(keys.tolist())
    for u, v in a.tolist():
        assert u * 500 + v not in ks and v * 500 + u not in ks
    b = LP.sample_negatives(keys, 500, 123457, seed=11, device=DEV)
    assert torch.equal(a, b)
    c = LP.sample_negatives(keys, 500, 123457, seed=12, device=DEV)
    assert not torch.equal(a, c)
    # slot s depends on (seed, s) only
    assert torch.equal(LP.sample_negatives(keys, 500, 1000, seed=11, device=DEV), a[:1000])


def test_sampler_uniform_over_valid_pairs():
    n = 12
    edges = [(0, 1), (1, 2), (2, 3), (3, 0), (4, 5), (5, 6), (7, 7), (8, 9), (9, 10), (10, 11), (11, 8), (0, 6)]
    keys = _keys(n, edges)
    draws = LP.sample_negatives(keys, n, 10 ** 6, seed=2026, device=DEV).cpu().numpy()
    und = {(u, v) for u, v in edges} | {(v, u) for u, v in edges}
    valid = [(u, v) for u in range(n) for v in range(n) if u != v and (u, v) not in und]
    assert LP.valid_pair_count(keys, n) == len(valid)
    counts = np.bincount(draws[:, 0] * n + draws[:, 1], minlength=n * n)
    obs = np.array([counts[u * n + v] for u, v in valid])
    assert obs.sum() == 10 ** 6
    exp = 10 ** 6 / len(valid)
    chi2 = ((obs - exp) ** 2 / exp).sum()
    dof = len(valid) - 1
    assert chi2 < dof + 5 * np.sqrt(2 * dof), (chi2, dof)     # ~5 sigma; deterministic under the fixed seed


def test_sampler_complete_graph_raises_before_launch():
    n = 5
    keys = _keys(n, [(u, v) for u in range(n) for v in range(u + 1, n)])
    with pytest.raises(ValueError, match="no negative edge"):
        LP.sample_negatives(keys, n, 10, seed=1, device=DEV)


# ------------------------------------------------------------------------------------------------ fused passes vs float64 autograd
def _feat(m, a, b):
    return {"Avg": (a + b) / 2, "Had": a * b, "L1": (a - b).abs(), "L2": (a - b) ** 2}[m]


@pytest.mark.parametrize("d", [128, 37])
def test_pass_loss_grad_hess_scores_vs_float64(d):
    g = torch.Generator().manual_seed(d)
    N, n = 300, 5000
    E = torch.randn(N, d, generator=g).to(DEV)
    edges = torch.stack([torch.randint(0, N, (n,), generator=g), torch.randint(0, N, (n,), generator=g),
                         (torch.rand(n, generator=g) < 0.3).long()], 1).to(DEV)
    es = _logreg.EdgeSet(edges, N)
    measures = ["Avg", "Had", "L1", "L2", "Had", "L2", "Avg", "L1", "L1"]
    W = (torch.randn(len(measures), d + 1, generator=g) * 0.2).to(DEV)
    loss, grad = _logreg.loss_grad(E, es, measures, W)
    H = _logreg.hessian(E, es, measures, W)
    z = _logreg.scores(E, es, measures, W)
    Ed, Wd = E.double(), W.double()
    a, b = Ed[edges[:, 0]], Ed[edges[:, 1]]
    y = edges[:, 2].double()
    s = torch.where(y > 0, es.w_pos, es.w_neg)
    for m, meas in enumerate(measures):
        phi = torch.cat([_feat(meas, a, b), torch.ones(n, 1, dtype=torch.float64, device=DEV)], 1)
        th = Wd[m].clone().requires_grad_(True)
        zz = phi @ th
        L = (s * torch.nn.functional.softplus(torch.where(y > 0, -zz, zz))).sum()
        L.backward()
        sig = torch.sigmoid(zz.detach())
        Href = (phi * (s * sig * (1 - sig))[:, None]).t() @ phi
        scale = float(s.sum())
        assert abs(loss[m].item() - L.item()) <= 1e-6 * scale, meas
        assert (grad[m] - th.grad).abs().max().item() <= 1e-6 * scale, meas
        assert (H[m] - Href).abs().max().item() <= 1e-5 * scale, meas
        assert (z[m].double() - zz.detach()).abs().max().item() <= 1e-4, meas
    # bit-identical repeats
    loss2, grad2 = _logreg.loss_grad(E, es, measures, W)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2)
    assert torch.equal(H, _logreg.hessian(E, es, measures, W))


# ------------------------------------------------------------------------------------------------ fits vs the reference fixture
@pytest.fixture(scope="module")
def uci_fits():
    out = []
    for t in range(1, T + 1):
        E = _emb(t - 1)
        train, val, test = _split(t, "train"), _split(t, "val"), _split(t, "test")
        es = _logreg.EdgeSet(train, E.shape[0])
        ms = [m for m in MEASURES for _ in C_LIST]
        cs = [c for _ in MEASURES for c in C_LIST]
        theta, rep = _logreg.fit(E, es, ms, cs)
        res = LP.evaluate(E, train, val, test, C_LIST, MEASURES + ["sigmoid"])
        out.append((theta.cpu().numpy().reshape(len(MEASURES), len(C_LIST), -1), rep, res))
    return out


def test_fits_converge_to_the_tight_optima(uci_fits):
    for t, (theta, rep, _) in enumerate(uci_fits):
        assert all(r.converged for r in rep), [(r.measure, r.C, r.grad_norm) for r in rep]
        coef, icpt = GOLD["tight_coef"][t], GOLD["tight_intercept"][t]
        ref = np.concatenate([coef, icpt[..., None]], -1)
        err = np.abs(theta - ref).max(-1) / np.abs(ref).max(-1)
        assert err.max() <= 1e-4, (t, err.max())


def test_test_aucs_match_tight_and_reference(uci_fits):
    for t, (_, _, res) in enumerate(uci_fits):
        for mi, m in enumerate(MEASURES):
            ci = C_LIST.index(res["C"][m])
            np.testing.assert_allclose(res["val_auc"][m], GOLD["tight_val_auc"][t, mi], atol=1e-5, rtol=0)
            assert abs(res["auc"][m] - GOLD["tight_test_auc"][t, mi, ci]) <= 1e-5
            gap = np.abs(GOLD["ref_test_auc"][t, mi] - GOLD["tight_test_auc"][t, mi]).max()
            assert abs(res["auc"][m] - GOLD["ref_test_auc"][t, mi, ci]) <= gap + 1e-5 + 1e-6
            # the chosen C is the reference's wherever the val-AUC margin exceeds the default-tol gap
            vg = np.abs(GOLD["ref_val_auc"][t, mi] - GOLD["tight_val_auc"][t, mi]).max()
            v = np.sort(GOLD["ref_val_auc"][t, mi])
            if v[-1] - v[-2] > 2 * vg + 2e-5:
                assert ci == GOLD["ref_best"][t, mi], (t, m)
        assert abs(res["auc"]["sigmoid"] - GOLD["sigmoid_auc"][t]) <= 1e-12
        assert 0.5 < min(res["auc"].values()) < 1.0


# ------------------------------------------------------------------------------------------------ end to end through the files
def test_link_prediction_end_to_end(tmp_path):
    names = [str(x) for x in GOLD["node_names"]]
    files = [str(f) for f in GOLD["files"]]
    base = str(tmp_path)
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    for f in files:
        with open(os.path.join(base, "1.format", f), "w") as fh:
            fh.write("from_id\tto_id\tweight\n")
    pd.DataFrame(names).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb_np(t) for t in range(T)])), files, 0, os.path.join(base, "2.embedding", "CTGCN-C"), names)
    os.makedirs(os.path.join(base, "lp_data_0"))
    for t in range(1, T + 1):
        date = files[t].split('.')[0]
        for p in ("train", "val", "test"):
            LP.write_split(os.path.join(base, "lp_data_0", "%s_%s.csv" % (date, p)), _split(t, p), "\t")
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                lp_edge_folder="lp_data", lp_res_folder="lp_res", file_sep="\t", start_idx=0, rep_num=1, train_ratio=0.5, val_ratio=0.3,
                test_ratio=0.2, do_lp=True, generate=False, aggregate=True, method_list=["CTGCN-C"], c_list=C_LIST,
                measure_list=MEASURES + ["sigmoid"], max_iter=10000, worker=-1)
    LP.link_prediction(args)
    df = pd.read_csv(os.path.join(base, "lp_res_0", "CTGCN-C_auc_record.csv"))
    assert list(df.columns) == ["date"] + MEASURES + ["sigmoid"]
    assert list(df["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
    ref = GOLD["table_auc"]
    gap = np.abs(GOLD["ref_test_auc"] - GOLD["tight_test_auc"]).max()
    assert np.abs(df[MEASURES + ["sigmoid"]].values - ref).max() <= max(gap, 0.02) + 1e-6
    assert os.path.exists(os.path.join(base, "lp_res", "CTGCN-C_Had_record.csv"))


def test_generate_then_predict_in_memory():
    """DataGenerator's GPU path: splits of UCI month files with the reference's counts, negatives valid, reproducible by seed."""
    pos = torch.from_numpy(np.stack([np.arange(0, 400), (np.arange(0, 400) * 7 + 1) % 500], 1)).to(DEV)
    a = LP.make_splits(pos, 500, 0.5, 0.3, 0.2, seed=5)
    b = LP.make_splits(pos, 500, 0.5, 0.3, 0.2, seed=5)
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    train_num, val_num, test_num = LP.split_counts(800, 0.5, 0.3, 0.2)
    assert [x.shape[0] for x in a] == [2 * train_num, 2 * val_num, 2 * test_num]
    E = torch.randn(500, 64, device=DEV)
    res = LP.evaluate_window([E, E], [pos, pos], [1.0], ["Had", "sigmoid"], seed=3)
    assert len(res) == 1 and 0.0 <= res[0]["auc"]["Had"] <= 1.0


# ------------------------------------------------------------------------------------------------ size: one Enron-like snapshot
def test_enron_like_snapshot_converges():
    from ctgcn_amd.synth import dynamic_graph
    n, d = 87000, 128
    g = dynamic_graph(n, avg_deg=12, snapshots=1, seed=7)[0].tocoo()
    keep = g.row < g.col
    pos = torch.from_numpy(np.stack([g.row[keep], g.col[keep]], 1).astype(np.int64)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(1)
    # planted signal: endpoints of an edge share a component along a random direction
    base = torch.randn(n, d, device=DEV, generator=gen)
    A = torch.sparse_coo_tensor(torch.cat([pos.t(), pos.flip(1).t()], 1), torch.ones(2 * pos.shape[0], device=DEV), (n, n))
    E = (base + 0.5 * torch.sparse.mm(A, base) / 12).contiguous()
    torch.cuda.synchronize()
    t0 = time.time()
    train, val, test = LP.make_splits(pos, n, 0.5, 0.3, 0.2, seed=9)
    res = LP.evaluate(E, train, val, test, [0.01, 0.1, 1, 10], ["Avg", "Had", "L1", "L2"])
    torch.cuda.synchronize()
    print("enron-like: %d undirected edges, %d train rows: %.2f s" % (pos.shape[0], train.shape[0], time.time() - t0))
    assert len(res["report"]) == 16 and all(r.converged for r in res["report"])
    for m, a in res["auc"].items():
        assert np.isfinite(a) and a > 0.5, (m, a)
