"""Node-classification evaluation on the GPU (ctgcn_nodecls.hip + ctgcn_amd/evaluation) against float64 numpy and the reference
fixture node_classification_uci.npz (the reference's own splits and tables, sklearn one-vs-rest fits at tol=1e-12)."""
import importlib
import os
import time

import numpy as np
import pandas as pd
import pytest
import torch

import _lp_fixture
import _nc_fixture
from ctgcn_amd import export
from ctgcn_amd.evaluation import _ovr

NC = importlib.import_module("ctgcn_amd.evaluation.node_classification")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "node_classification_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
C_LIST = [float(c) for c in GOLD["C_list"]]
T, REPS, N = len(FILES), GOLD["table_acc"].shape[0], len(GOLD["node_names"])
SEED = 20261016
NEAR_TIE = 1e-6


def _emb_np(t):
    e = _lp_fixture.month_embedding(SNAPSHOTS, t, N, 128, SEED)
    assert _lp_fixture.digest(e) == GOLD["emb_sha256"][t], "rebuilt embedding differs from what the reference was given"
    return e


# ------------------------------------------------------------------------------------------------ passes vs float64 numpy
def _problems(g, sizes, K, R):
    out = []
    for n in sizes:
        y = torch.randint(0, K, (n,), generator=g)
        y[:min(n, K)] = torch.arange(min(n, K))
        out.append(_ovr.Problem(torch.randint(0, R, (n,), generator=g).to(DEV), y.to(torch.int32).to(DEV), K))
    return out


def _sigmoid(z):
    return 0.5 * (1 + np.tanh(0.5 * z))


@pytest.mark.parametrize("d,K", [(128, 4), (37, 2), (37, 7), (128, 2)])
def test_passes_vs_float64(d, K):
    g = torch.Generator().manual_seed(d * 10 + K)
    R = 400
    E = torch.randn(R, d, generator=g).to(DEV)
    sizes = [1, 45, 300, 1000]
    probs = _problems(g, sizes, K, R)
    Cs = [0.1, 1.0, 10.0]
    tb = _ovr.Table(E, probs, Cs, hess_max=256)
    theta = (torch.randn(tb.M, d + 1, generator=g, dtype=torch.float64) * 0.2).to(DEV)
    loss, grad = tb.loss_grad(theta)
    H = tb.hessian(theta, 0, tb.P)
    pred, correct = tb.predict(theta, probs)
    En, th = E.double().cpu().numpy(), theta.cpu().numpy()
    mpg = _ovr.models_per_group(K)
    row = 0
    for pi, p in enumerate(probs):
        rows, y = p.rows.cpu().numpy(), p.y.cpu().numpy().astype(np.int64)
        X = np.concatenate([En[rows], np.ones((len(rows), 1))], 1)
        step = 1 if len(rows) <= 256 else -(-len(rows) // 256)
        m0 = int(tb.model_start_h[pi])
        probs_all = np.zeros((len(rows), len(Cs), mpg))
        for k in range(len(Cs) * mpg):
            m = m0 + k
            yy = (y == tb.m_cls[m]).astype(np.float64)
            s = np.where(yy > 0, *tb.model_w[m].cpu().numpy()[::-1])
            z = X @ th[m]
            probs_all[:, k // mpg, k % mpg] = _sigmoid(z)
            if tb.flags_h[m]:
                assert loss[m].item() == 0 and grad[m].abs().max().item() == 0 and H[m - 0].abs().max().item() == 0
                probs_all[:, k // mpg, k % mpg] = 0.0 if tb.flags_h[m] == 1 else 1.0
                continue
            L = (s * np.logaddexp(0, np.where(yy > 0, -z, z))).sum()
            G = X.T @ (s * (_sigmoid(z) - yy))
            sub = np.arange(0, len(rows), step)
            a = (s * _sigmoid(z) * (1 - _sigmoid(z)))[sub]
            Href = (X[sub] * a[:, None]).T @ X[sub]
            scale = s.sum()
            assert abs(loss[m].item() - L) <= 1e-6 * scale
            assert np.abs(grad[m].cpu().numpy() - G).max() <= 1e-6 * scale
            assert np.abs(H[m].cpu().numpy() - Href).max() <= 1e-5 * scale
        if mpg == 1:
            ref_pred = (probs_all[:, :, 0] > 1 - probs_all[:, :, 0]).astype(np.int64)
            margin = np.abs(2 * probs_all[:, :, 0] - 1)
        else:
            ref_pred = probs_all.argmax(2)
            srt = np.sort(probs_all, 2)
            margin = srt[:, :, -1] - srt[:, :, -2]
        got = pred[row:row + len(rows)].cpu().numpy()
        sure = margin > NEAR_TIE
        assert (got[sure] == ref_pred[sure]).all()
        assert (correct[pi].cpu().numpy() == (got == y[:, None]).sum(0)).all()
        row += len(rows)
    # repeated calls are bit-identical, and each problem's outputs do not depend on its batch mates
    loss2, grad2 = tb.loss_grad(theta)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(H, tb.hessian(theta, 0, tb.P))
    for pi in (0, 2, 3):
        alone = _ovr.Table(E, [probs[pi]], Cs, hess_max=256)
        m0, m1 = int(tb.model_start_h[pi]), int(tb.model_start_h[pi + 1])
        la, ga = alone.loss_grad(theta[m0:m1])
        assert torch.equal(la, loss[m0:m1]) and torch.equal(ga, grad[m0:m1])
        assert torch.equal(alone.hessian(theta[m0:m1], 0, 1), H[m0:m1])
        pa, ca = alone.predict(theta[m0:m1], [probs[pi]])
        r0 = sum(sizes[:pi])
        assert torch.equal(pa, pred[r0:r0 + sizes[pi]]) and torch.equal(ca[0], correct[pi])


# ------------------------------------------------------------------------------------------------ fits vs the reference fixture
@pytest.fixture(scope="module")
def uci_fit():
    E = torch.from_numpy(np.concatenate([_emb_np(t) for t in range(T)])).to(DEV)
    splits = []
    for r in range(REPS):
        for t in range(T):
            s = []
            for part in ("train", "val", "test"):
                rows = _nc_fixture.split_rows(GOLD, r, t, part)
                s.append((torch.from_numpy(rows[:, 0] + t * N).to(DEV), torch.from_numpy(rows[:, 1].astype(np.int32)).to(DEV)))
            splits.append(tuple(s))
    # tol 1e-7: at the default 1e-6 the weakly regularised models (C = 20, 1/(C n) ~ 5e-5) sit up to ~1e-4 relative from the optimum
    return NC.evaluate_batch(E, splits, C_LIST, 4, tol=1e-7)


def test_uci_fits_match_the_tight_optima(uci_fit):
    res, reports = uci_fit
    assert all(r.converged for r in reports), [(r.problem, r.cls, r.C, r.grad_norm) for r in reports if not r.converged]
    offs = {p: 0 for p in ("val", "test")}
    for i, o in enumerate(res):
        r, t = divmod(i, T)
        ref = GOLD["tight_coef"][r, t].astype(np.float64)
        theta = o["theta"].cpu().numpy()
        err = np.abs(theta - ref).max(-1) / np.abs(ref).max(-1)
        assert err.max() <= 1e-4, (r, t, err.max())
        for part in ("val", "test"):
            n = len(_nc_fixture.split_rows(GOLD, r, t, part))
            want = GOLD["tight_%s_pred" % part][offs[part]:offs[part] + n]
            margin = GOLD["tight_%s_margin" % part][offs[part]:offs[part] + n]
            got = o[part + "_pred"].cpu().numpy()
            sure = margin >= NEAR_TIE
            assert (got[sure] == want[sure]).all(), (r, t, part)
            offs[part] += n
        np.testing.assert_allclose(o["val_acc"], GOLD["tight_val_acc"][r, t], rtol=0, atol=1e-15)
        np.testing.assert_allclose(o["test_acc"], GOLD["tight_test_acc"][r, t], rtol=0, atol=1e-15)
        assert o["C_index"] == GOLD["tight_best"][r, t]
        assert abs(o["acc"] - GOLD["table_acc"][r, t]) <= float(GOLD["tol_gap"]) + 1e-12


@pytest.mark.parametrize("case", ["k2", "absent", "ties"])
def test_edge_cases_match_the_reference(case):
    gk = lambda k: GOLD["edge_%s_%s" % (case, k)]
    emb, y, K = torch.from_numpy(gk("emb")).to(DEV), gk("y"), int(gk("K"))
    split = {p: torch.from_numpy(np.stack([gk(p), y[gk(p)]], 1).astype(np.int64)).to(DEV) for p in ("train", "val", "test")}
    res = NC.evaluate(emb, split["train"], split["val"], split["test"], C_LIST, list(range(K)))
    np.testing.assert_allclose(res["val_acc"], gk("tight_val_acc"), rtol=0, atol=1e-15)
    assert res["C"] == float(gk("ref_C"))
    assert abs(res["acc"] - float(gk("ref_acc"))) <= 1e-15
    if case == "absent":
        assert sum(r.constant for r in res["report"]) == len(C_LIST)
    assert all(r.converged for r in res["report"])


# ------------------------------------------------------------------------------------------------ end to end through the files
def test_node_classification_end_to_end(tmp_path):
    base = str(tmp_path)
    for sub in ("1.format", "nodes_set", "nodes_label"):
        os.makedirs(os.path.join(base, sub))
    for t, f in enumerate(FILES):
        with open(os.path.join(base, "1.format", f), "w") as fh:
            fh.write("from_id\tto_id\tweight\n")
        pd.DataFrame({"node": [NAMES[i] for i in GOLD["labels_%d_node" % t]], "label": GOLD["labels_%d_label" % t]}).to_csv(
            os.path.join(base, "nodes_label", f), sep="\t", index=False)
    pd.DataFrame(NAMES).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb_np(t) for t in range(T)])), FILES, 0, os.path.join(base, "2.embedding", "CTGCN-C"), NAMES)
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                nlabel_folder="nodes_label", nodecls_data_folder="nodecls_data", nodecls_res_folder="nodecls_res", file_sep="\t",
                start_idx=0, rep_num=REPS, train_ratio=0.7, val_ratio=0.2, test_ratio=0.1, do_nodecls=True, generate=True,
                aggregate=True, method_list=["CTGCN-C"], c_list=C_LIST, max_iter=10000, worker=-1)
    np.random.seed(SEED)
    NC.node_classification(args)
    for r in range(REPS):
        for t, f in enumerate(FILES):
            rows = np.loadtxt(os.path.join(base, "nodecls_data_%d" % r, f.split(".")[0] + "_train.csv"), skiprows=1, dtype=np.int64)
            assert np.array_equal(rows, _nc_fixture.split_rows(GOLD, r, t, "train"))
        df = pd.read_csv(os.path.join(base, "nodecls_res_%d" % r, "CTGCN-C_acc_record.csv"))
        assert list(df.columns) == ["date", "acc"] and list(df["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
        tight = np.array([GOLD["tight_test_acc"][r, t, GOLD["tight_best"][r, t]] for t in range(T)])
        np.testing.assert_allclose(df["acc"].values, tight, rtol=0, atol=1e-15)
    agg = pd.read_csv(os.path.join(base, "nodecls_res", "CTGCN-C_acc_record.csv"))
    assert list(agg.columns) == [str(c) for c in GOLD["agg_columns"]]
    assert np.abs(agg.iloc[:, 1:].values - GOLD["agg_values"]).max() <= float(GOLD["tol_gap"]) + 1e-12


# ------------------------------------------------------------------------------------------------ a window in one solve
def _quartiles(deg):
    order = np.lexsort((np.arange(len(deg)), deg))
    lab = np.empty(len(deg), np.int64)
    lab[order] = (4 * np.arange(len(deg))) // len(deg)
    return lab


def test_window_equals_separate_evaluations():
    from ctgcn_amd.synth import dynamic_graph
    n, Tw, d, reps = 1190, 10, 128, 10
    graphs = dynamic_graph(n, avg_deg=10, snapshots=Tw, seed=4)
    gen = torch.Generator(device=DEV).manual_seed(3)
    embs, labels = [], []
    for gph in graphs:
        deg = np.asarray(gph.sum(1)).ravel()
        lab = _quartiles(deg)
        x = torch.randn(n, d, device=DEV, generator=gen) + 0.3 * torch.from_numpy(lab).to(DEV, torch.float32)[:, None]
        embs.append(x)
        labels.append((np.arange(n), lab))
    C = [0.01, 0.1, 1, 5, 10, 20]
    win = NC.evaluate_window(torch.stack(embs, 1), labels, C, rep_num=reps, seed=11)
    assert win["acc"].shape == (reps, Tw) and len(win["reports"]) == reps * Tw * 24
    assert all(r.converged for r in win["reports"])
    rng = np.random.RandomState(11)
    for r in range(reps):
        for t in range(Tw):
            nodes, lab = labels[t]
            ix = NC.shuffle_split(n, 0.7, 0.2, 0.1, rng)
            sp = [torch.from_numpy(np.stack([nodes[i], lab[i]], 1)).to(DEV) for i in ix]
            one = NC.evaluate(embs[t], sp[0], sp[1], sp[2], C, 4)
            w = win["results"][r * Tw + t]
            assert (one["theta"] - w["theta"]).abs().max().item() <= 1e-9 * max(1.0, w["theta"].abs().max().item())
            same = lambda a, b: torch.equal(a, b)
            if same(one["val_pred"], w["val_pred"]) and same(one["test_pred"], w["test_pred"]):
                assert one["val_acc"] == w["val_acc"] and one["C"] == w["C"] and one["acc"] == w["acc"]


# ------------------------------------------------------------------------------------------------ size
def test_powerlaw_200k_converges():
    from ctgcn_amd.synth import powerlaw_edges
    n, d = 200_000, 128
    u, v = powerlaw_edges(n, 1_000_000, 5)
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    lab = _quartiles(deg)
    gen = torch.Generator(device=DEV).manual_seed(5)
    E = (torch.randn(n, d, device=DEV, generator=gen) + 0.2 * torch.from_numpy(lab).to(DEV, torch.float32)[:, None]).contiguous()
    ix = NC.shuffle_split(n, 0.7, 0.2, 0.1, np.random.RandomState(0))
    sp = [torch.from_numpy(np.stack([i, lab[i]], 1)).to(DEV) for i in ix]
    torch.cuda.synchronize()
    t0 = time.time()
    res = NC.evaluate(E, sp[0], sp[1], sp[2], [0.01, 0.1, 1, 5, 10, 20], 4)
    torch.cuda.synchronize()
    print("powerlaw-200k: %d train rows, %.2f s, iterations %s" % (len(ix[0]), time.time() - t0, sorted({r.iterations for r in res["report"]})))
    assert len(res["report"]) == 24 and all(r.converged for r in res["report"])
    assert res["acc"] > 0.3
