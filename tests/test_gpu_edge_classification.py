"""Edge-classification evaluation on the GPU (the pair-gather passes of ctgcn_nodecls.hip + ctgcn_amd/evaluation) against float64
numpy, against the node table on materialised products, and against the reference fixture edge_classification_uci.npz (the
reference's own splits and tables, sklearn one-vs-rest fits at tol=1e-12)."""
import importlib
import os
import time

import numpy as np
import pandas as pd
import pytest
import torch

import _ec_fixture
import _lp_fixture
from ctgcn_amd import export
from ctgcn_amd.evaluation import _ovr

EC = importlib.import_module("ctgcn_amd.evaluation.edge_classification")

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "edge_classification_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
C_LIST = [float(c) for c in GOLD["C_list"]]
T, REPS, N = len(FILES), GOLD["table_acc"].shape[0], len(GOLD["node_names"])
SEED = 20261017           # the embeddings
SPLIT_SEED = 20261022     # the reference drew its splits under np.random.seed(SPLIT_SEED) (make_golden_edgecls.py)
NEAR_TIE = 1e-6


def _emb_np(t):
    e = _lp_fixture.month_embedding(SNAPSHOTS, t, N, 128, SEED)
    assert _lp_fixture.digest(e) == GOLD["emb_sha256"][t], "rebuilt embedding differs from what the reference was given"
    return e


# ------------------------------------------------------------------------------------------------ passes vs float64 numpy
def _problems(g, sizes, K, R):
    """Pair problems with random endpoints; every fifth entry has u == v."""
    out = []
    for n in sizes:
        y = torch.randint(0, K, (n,), generator=g)
        y[:min(n, K)] = torch.arange(min(n, K))
        u, v = torch.randint(0, R, (n,), generator=g), torch.randint(0, R, (n,), generator=g)
        v[::5] = u[::5]
        out.append(_ovr.Problem(u.to(DEV), y.to(torch.int32).to(DEV), K, rows2=v.to(DEV)))
    return out


def _sigmoid(z):
    return 0.5 * (1 + np.tanh(0.5 * z))


@pytest.mark.parametrize("d,K", [(128, 3), (37, 2), (37, 7), (128, 2)])
def test_passes_vs_float64(d, K):
    """Loss, gradient, Hessian and predictions of the pair passes against float64 numpy on φ = E[u]·E[v].  The bounds are the node
    test's (1e-6 loss and gradient, 1e-5 Hessian) on a scale derived from the inputs: a row's terms are bounded by its weight times
    its largest |φ| (squared in the Hessian), and products of normals have heavier tails than the node test's rows, so the scale is
    Σ_i s_i max(1, max_j |φ_ij|) for loss and gradient and Σ_i s_i max(1, max_j |φ_ij|)² for the Hessian (the node test's Σ_i s_i
    when no |φ| exceeds 1)."""
    g = torch.Generator().manual_seed(d * 10 + K)
    R = 400
    E = torch.randn(R, d, generator=g).to(DEV)
    sizes = [1, 45, 300, 1000]
    probs = _problems(g, sizes, K, R)
    Cs = [0.1, 1.0, 10.0]
    tb = _ovr.Table(E, probs, Cs, hess_max=256)
    assert tb.pair
    theta = (torch.randn(tb.M, d + 1, generator=g, dtype=torch.float64) * 0.2).to(DEV)
    loss, grad = tb.loss_grad(theta)
    H = tb.hessian(theta, 0, tb.P)
    pred, correct = tb.predict(theta, probs)
    En, th = E.double().cpu().numpy(), theta.cpu().numpy()
    mpg = _ovr.models_per_group(K)
    row = 0
    for pi, p in enumerate(probs):
        u, v, y = p.rows.cpu().numpy(), p.rows2.cpu().numpy(), p.y.cpu().numpy().astype(np.int64)
        assert (u == v).any()
        phi = En[u] * En[v]
        X = np.concatenate([phi, np.ones((len(u), 1))], 1)
        big = np.maximum(1.0, np.abs(phi).max(1))
        step = 1 if len(u) <= 256 else -(-len(u) // 256)
        m0 = int(tb.model_start_h[pi])
        probs_all = np.zeros((len(u), len(Cs), mpg))
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
            sub = np.arange(0, len(u), step)
            a = (s * _sigmoid(z) * (1 - _sigmoid(z)))[sub]
            Href = (X[sub] * a[:, None]).T @ X[sub]
            scale, scale2 = (s * big).sum(), (s * big * big).sum()
            e_loss, e_grad = abs(loss[m].item() - L), np.abs(grad[m].cpu().numpy() - G).max()
            e_hess = np.abs(H[m].cpu().numpy() - Href).max()
            if k == 0:
                print("d %d K %d n %d: loss %.2e grad %.2e of scale, hess %.2e of scale2" % (d, K, len(u), e_loss / scale, e_grad / scale,
                                                                                              e_hess / scale2))
            assert e_loss <= 1e-6 * scale
            assert e_grad <= 1e-6 * scale
            assert e_hess <= 1e-5 * scale2
        if mpg == 1:
            ref_pred = (probs_all[:, :, 0] > 1 - probs_all[:, :, 0]).astype(np.int64)
            margin = np.abs(2 * probs_all[:, :, 0] - 1)
        else:
            ref_pred = probs_all.argmax(2)
            srt = np.sort(probs_all, 2)
            margin = srt[:, :, -1] - srt[:, :, -2]
        got = pred[row:row + len(u)].cpu().numpy()
        sure = margin > NEAR_TIE
        assert (got[sure] == ref_pred[sure]).all()
        assert (correct[pi].cpu().numpy() == (got == y[:, None]).sum(0)).all()
        row += len(u)
    # repeated calls are bit-identical, and each problem's outputs do not depend on its batch mates
    loss2, grad2 = tb.loss_grad(theta)
    assert torch.equal(loss, loss2) and torch.equal(grad, grad2) and torch.equal(H, tb.hessian(theta, 0, tb.P))
    pred2, correct2 = tb.predict(theta, probs)
    assert torch.equal(pred, pred2) and torch.equal(correct, correct2)
    for pi in (0, 2, 3):
        alone = _ovr.Table(E, [probs[pi]], Cs, hess_max=256)
        m0, m1 = int(tb.model_start_h[pi]), int(tb.model_start_h[pi + 1])
        la, ga = alone.loss_grad(theta[m0:m1])
        assert torch.equal(la, loss[m0:m1]) and torch.equal(ga, grad[m0:m1])
        assert torch.equal(alone.hessian(theta[m0:m1], 0, 1), H[m0:m1])
        pa, ca = alone.predict(theta[m0:m1], [probs[pi]])
        r0 = sum(sizes[:pi])
        assert torch.equal(pa, pred[r0:r0 + sizes[pi]]) and torch.equal(ca[0], correct[pi])


# ------------------------------------------------------------------------------------------------ pair table vs node table on the products
def _layout(name, g, R):
    if name == "d128":                                  # contiguous, 16-byte aligned rows: the float4 staging
        return torch.randn(R, 128, generator=g).to(DEV)
    if name == "d37":                                   # d % 4 != 0: the scalar staging
        return torch.randn(R, 37, generator=g).to(DEV)
    wide = torch.randn(R, 132, generator=g).to(DEV)    # d = 128 and lde % 4 == 0, but rows start 4 bytes off 16-byte alignment: scalar
    return wide[:, 1:129]


@pytest.mark.parametrize("layout", ["d128", "d37", "d128-unaligned-view"])
def test_pair_path_equals_materialised_rows(layout):
    """The pair table stages E[u] ⊙ E[v]; a node table on X = E[u] * E[v] (fp32) stages the same values, and the chunking depends on
    the row counts only: every output must be bit-identical.  Entries with an endpoint outside [0, R) read as zero features."""
    g = torch.Generator().manual_seed(7)
    R, K, Cs = 400, 3, [0.1, 1.0, 10.0]
    E = _layout(layout, g, R)
    d = E.shape[1]
    assert (E.data_ptr() % 16 == 0 and E.stride(0) % 4 == 0 and d % 4 == 0) == (layout == "d128")
    sizes = [1, 45, 300, 1000]
    pair = _problems(g, sizes, K, R)
    pair[2].rows[3], pair[2].rows2[4], pair[3].rows2[999] = -1, R, R + 5
    u, v = torch.cat([p.rows for p in pair]), torch.cat([p.rows2 for p in pair])
    inside = ((u >= 0) & (u < R) & (v >= 0) & (v < R))
    X = torch.where(inside[:, None], E[u.clamp(0, R - 1)] * E[v.clamp(0, R - 1)], torch.zeros((), device=DEV)).contiguous()
    assert int((~inside).sum()) == 3 and X[~inside].abs().max().item() == 0
    offs = np.concatenate([[0], np.cumsum(sizes)])
    node = [_ovr.Problem(torch.arange(offs[i], offs[i + 1], device=DEV), p.y, K) for i, p in enumerate(pair)]
    tp, tn = _ovr.Table(E, pair, Cs, hess_max=256), _ovr.Table(X, node, Cs, hess_max=256)
    assert tp.pair and not tn.pair and tp.total_chunks == tn.total_chunks
    theta = (torch.randn(tp.M, d + 1, generator=g, dtype=torch.float64) * 0.2).to(DEV)
    (lp, gp), (ln, gn) = tp.loss_grad(theta), tn.loss_grad(theta)
    assert torch.equal(lp, ln) and torch.equal(gp, gn)
    assert torch.equal(tp.hessian(theta, 0, tp.P), tn.hessian(theta, 0, tn.P))
    (pp, cp), (pn, cn) = tp.predict(theta, pair), tn.predict(theta, node)
    assert torch.equal(pp, pn) and torch.equal(cp, cn)


# ------------------------------------------------------------------------------------------------ fits vs the reference fixture
def _uci_splits():
    splits = []
    for r in range(REPS):
        for t in range(T):
            s = []
            for part in ("train", "val", "test"):
                rows = _ec_fixture.split_rows(GOLD, r, t, part)
                s.append((torch.from_numpy(rows[:, 0] + t * N).to(DEV), torch.from_numpy(rows[:, 1] + t * N).to(DEV),
                          torch.from_numpy(rows[:, 2].astype(np.int32)).to(DEV)))
            splits.append(tuple(s))
    return splits


@pytest.fixture(scope="module")
def uci_fit():
    E = torch.from_numpy(np.concatenate([_emb_np(t) for t in range(T)])).to(DEV)
    # tol 1e-7: at the default 1e-6 the weakly regularised models (C = 20) sit up to ~1e-4 relative from the optimum
    return EC.evaluate_batch(E, _uci_splits(), C_LIST, 3, tol=1e-7)


def test_uci_fits_match_the_tight_optima(uci_fit):
    res, reports = uci_fit
    assert len(res) == REPS * T and len(reports) == REPS * T * len(C_LIST) * 3
    assert all(r.converged for r in reports), [(r.problem, r.cls, r.C, r.grad_norm) for r in reports if not r.converged]
    offs = {p: 0 for p in ("val", "test")}
    worst = 0.0
    for i, o in enumerate(res):
        r, t = divmod(i, T)
        ref = GOLD["tight_coef"][r, t].astype(np.float64)
        theta = o["theta"].cpu().numpy()
        err = np.abs(theta - ref).max(-1) / np.abs(ref).max(-1)
        worst = max(worst, err.max())
        assert err.max() <= 1e-4, (r, t, err.max())
        all_sure = {}
        for part in ("val", "test"):
            n = len(_ec_fixture.split_rows(GOLD, r, t, part))
            want = GOLD["tight_%s_pred" % part][offs[part]:offs[part] + n]
            margin = GOLD["tight_%s_margin" % part][offs[part]:offs[part] + n]
            got = o[part + "_pred"].cpu().numpy()
            sure = margin >= NEAR_TIE
            assert (got[sure] == want[sure]).all(), (r, t, part)
            all_sure[part] = sure.all(0)                 # per C
            tight = GOLD["tight_%s_acc" % part][r, t]
            np.testing.assert_allclose(np.array(o[part + "_acc"])[all_sure[part]], tight[all_sure[part]], rtol=0, atol=1e-15)
            offs[part] += n
        if all_sure["val"].all():
            assert o["C_index"] == GOLD["tight_best"][r, t]
        assert abs(o["acc"] - GOLD["table_acc"][r, t]) <= float(GOLD["tol_gap"]) + 1e-12
    print("uci: worst relative coefficient error %.2e" % worst)


def test_uci_near_ties_are_rare():
    """At most 0.5 % of any split's rows, at any C, may fall out of the prediction comparison above (tight margin below NEAR_TIE); in a
    split of fewer than 200 rows that means none.  A property of the reference's tight fits alone, which the fixture generator
    asserts too: the split seed is the first from 20261017 on that meets it (tests/golden/make_golden_edgecls.py)."""
    offs = {p: 0 for p in ("val", "test")}
    over = []
    for r in range(REPS):
        for t in range(T):
            for part in ("val", "test"):
                n = len(GOLD["split_%d_%d_%s" % (r, t, part)])
                unsure = (GOLD["tight_%s_margin" % part][offs[part]:offs[part] + n] < NEAR_TIE).sum(0)
                offs[part] += n
                if unsure.any():
                    print("rep %d month %d %s: %s of %d rows below the margin, per C" % (r, t, part, unsure, n))
                if unsure.max() > 0.005 * n:
                    over.append((r, t, part, n, unsure.tolist()))
    assert not over, over


@pytest.mark.parametrize("case", ["k2", "absent", "ties"])
def test_edge_cases_match_the_reference(case):
    gk = lambda k: GOLD["edge_%s_%s" % (case, k)]
    emb, edges, K = torch.from_numpy(gk("emb")).to(DEV), gk("edges"), int(gk("K"))
    split = {p: torch.from_numpy(edges[gk(p)]).to(DEV) for p in ("train", "val", "test")}
    assert (edges[:, 0] == edges[:, 1]).any()
    res = EC.evaluate(emb, split["train"], split["val"], split["test"], C_LIST, list(range(K)))
    np.testing.assert_allclose(res["val_acc"], gk("tight_val_acc"), rtol=0, atol=1e-15)
    assert res["C"] == float(gk("ref_C"))
    assert abs(res["acc"] - float(gk("ref_acc"))) <= 1e-15
    if case == "absent":
        assert sum(r.constant for r in res["report"]) == len(C_LIST)
    assert all(r.converged for r in res["report"])


def test_bad_indices_and_labels_raise():
    emb = torch.zeros(5, 4, device=DEV)
    ok = torch.tensor([[0, 1, 0], [1, 2, 1], [3, 3, 0]], device=DEV)
    with pytest.raises(ValueError, match="endpoint index outside"):
        EC.evaluate(emb, ok, torch.tensor([[0, 5, 0]], device=DEV), ok, [1.0], 2)
    with pytest.raises(ValueError, match="endpoint index outside"):
        EC.evaluate(emb, torch.tensor([[-1, 2, 0], [1, 2, 1]], device=DEV), ok, ok, [1.0], 2)
    with pytest.raises(ValueError, match="outside the classes"):
        EC.evaluate(emb, ok, ok, torch.tensor([[0, 1, 2]], device=DEV), [1.0], 2)


# ------------------------------------------------------------------------------------------------ end to end through the files
def test_edge_classification_end_to_end(tmp_path):
    base = str(tmp_path)
    for sub in ("1.format", "nodes_set", "edges_label"):
        os.makedirs(os.path.join(base, sub))
    for t, f in enumerate(FILES):
        with open(os.path.join(base, "1.format", f), "w") as fh:
            fh.write("from_id\tto_id\tweight\n")
        pd.DataFrame({"from_id": [NAMES[i] for i in GOLD["labels_%d_from" % t]], "to_id": [NAMES[i] for i in GOLD["labels_%d_to" % t]],
                      "label": GOLD["labels_%d_label" % t]}).to_csv(os.path.join(base, "edges_label", f), sep="\t", index=False)
    pd.DataFrame(NAMES).to_csv(os.path.join(base, "nodes_set", "nodes.csv"), header=False, index=False)
    export.save_embedding(torch.from_numpy(np.stack([_emb_np(t) for t in range(T)])), FILES, 0, os.path.join(base, "2.embedding", "CTGCN-C"), NAMES)
    args = dict(base_path=base, origin_folder="1.format", embed_folder="2.embedding", node_file="nodes_set/nodes.csv",
                elabel_folder="edges_label", edgecls_data_folder="edgecls_data", edgecls_res_folder="edgecls_res", file_sep="\t",
                start_idx=0, rep_num=REPS, train_ratio=0.7, val_ratio=0.2, test_ratio=0.1, do_edgecls=True, generate=True,
                aggregate=True, method_list=["CTGCN-C"], c_list=C_LIST, max_iter=10000, worker=-1)
    np.random.seed(SPLIT_SEED)
    EC.edge_classification(args)
    for r in range(REPS):
        for t, f in enumerate(FILES):
            for part in ("train", "val", "test"):
                rows = np.loadtxt(os.path.join(base, "edgecls_data_%d" % r, "%s_%s.csv" % (f.split(".")[0], part)), skiprows=1, dtype=np.int64)
                assert np.array_equal(rows.reshape(-1, 3), _ec_fixture.split_rows(GOLD, r, t, part))
        df = pd.read_csv(os.path.join(base, "edgecls_res_%d" % r, "CTGCN-C_acc_record.csv"))
        assert list(df.columns) == ["date", "acc"] and list(df["date"].astype(str)) == [str(d) for d in GOLD["table_dates"]]
        tight = np.array([GOLD["tight_test_acc"][r, t, GOLD["tight_best"][r, t]] for t in range(T)])
        np.testing.assert_allclose(df["acc"].values, tight, rtol=0, atol=1e-15)
    agg = pd.read_csv(os.path.join(base, "edgecls_res", "CTGCN-C_acc_record.csv"))
    assert list(agg.columns) == [str(c) for c in GOLD["agg_columns"]]
    assert np.abs(agg.iloc[:, 1:].values - GOLD["agg_values"]).max() <= float(GOLD["tol_gap"]) + 1e-12


# ------------------------------------------------------------------------------------------------ a window in one solve
def _tertiles(key):
    order = np.lexsort((np.arange(len(key)), key))
    lab = np.empty(len(key), np.int64)
    lab[order] = (3 * np.arange(len(key))) // len(key)
    return lab


def _planted(n, d, deg, strength, gen):
    """Noise plus a per-node term that grows with the node's degree quantile: E_u ⊙ E_v then has mean strength² q_u q_v per column."""
    q = np.empty(n, np.float32)
    q[np.lexsort((np.arange(n), deg))] = np.arange(n, dtype=np.float32) / n
    return (torch.randn(n, d, device=DEV, generator=gen) + strength * torch.from_numpy(q).to(DEV)[:, None]).contiguous()


def test_window_equals_separate_evaluations():
    from ctgcn_amd.synth import dynamic_graph
    import scipy.sparse as sp
    n, Tw, d, reps = 1190, 5, 128, 3
    graphs = dynamic_graph(n, avg_deg=10, snapshots=Tw, seed=4)
    gen = torch.Generator(device=DEV).manual_seed(3)
    embs, labels = [], []
    for gph in graphs:
        a = sp.triu(sp.csr_matrix(gph), 1).tocoo()
        u, v = a.row.astype(np.int64), a.col.astype(np.int64)
        deg = np.bincount(np.concatenate([u, v]), minlength=n)
        embs.append(_planted(n, d, deg, 0.7, gen))
        labels.append((u, v, _tertiles(deg[u] * deg[v])))
    C = [0.01, 0.1, 1, 5, 10, 20]
    win = EC.evaluate_window(torch.stack(embs, 1), labels, C, rep_num=reps, seed=11)
    assert win["acc"].shape == (reps, Tw) and len(win["reports"]) == reps * Tw * 18
    assert all(r.converged for r in win["reports"])
    rng = np.random.RandomState(11)
    for r in range(reps):
        for t in range(Tw):
            arr = np.stack(labels[t], 1)
            ix = EC.shuffle_split(len(arr), 0.7, 0.2, 0.1, rng)
            sp3 = [torch.from_numpy(arr[i]).to(DEV) for i in ix]
            one = EC.evaluate(embs[t], sp3[0], sp3[1], sp3[2], C, 3)
            w = win["results"][r * Tw + t]
            assert (one["theta"] - w["theta"]).abs().max().item() <= 1e-9 * max(1.0, w["theta"].abs().max().item())
            if torch.equal(one["val_pred"], w["val_pred"]) and torch.equal(one["test_pred"], w["test_pred"]):
                assert one["val_acc"] == w["val_acc"] and one["C"] == w["C"] and one["acc"] == w["acc"]


# ------------------------------------------------------------------------------------------------ size
def test_powerlaw_1m_edges_converges():
    """1 M edges on 200 k nodes, ~700 k train rows, labels = tertiles of the degree product, planted strength 0.7.  The reference
    (sklearn OneVsRest lbfgs, balanced, C = 1, float64) trained on a 20 000-row subsample of the same edges and labels, the embedding
    drawn the same way on the host, scores 0.5165 on 10 000 held-out rows (strength 0.5: 0.456; 0.3: 0.372), so the bar 1/3 + 0.05
    is cleared with room."""
    from ctgcn_amd.synth import powerlaw_edges
    n, d = 200_000, 128
    u, v = powerlaw_edges(n, 1_000_000, 5)
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    lab = _tertiles(deg[u] * deg[v])
    E = _planted(n, d, deg, 0.7, torch.Generator(device=DEV).manual_seed(5))
    arr = np.stack([u, v, lab], 1)
    ix = EC.shuffle_split(len(arr), 0.7, 0.2, 0.1, np.random.RandomState(0))
    sp3 = [torch.from_numpy(arr[i]).to(DEV) for i in ix]
    torch.cuda.synchronize()
    t0 = time.time()
    res = EC.evaluate(E, sp3[0], sp3[1], sp3[2], [0.01, 0.1, 1, 5, 10, 20], 3)
    torch.cuda.synchronize()
    print("powerlaw-1m-edges: %d train rows, %.2f s, iterations %s, acc %.4f" % (len(ix[0]), time.time() - t0,
                                                                                sorted({r.iterations for r in res["report"]}), res["acc"]))
    assert len(res["report"]) == 18 and all(r.converged for r in res["report"])
    assert res["acc"] > 1 / 3 + 0.05
