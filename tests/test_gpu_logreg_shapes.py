"""The logistic-regression kernels (ctgcn_eval.hip, ctgcn_nodecls.hip, ctgcn_logreg.h) at every dispatch boundary of the accepted
range 1 <= d <= 256, any model count, any row count, against the float64 reference of _logreg_ref.py (pinned on the CPU by
test_logreg_ref_host.py).  Each case names the code path it is there for; DESIGN.md ("Shape coverage of the logistic-regression
kernels") lists them by path.

Inputs: E = randn(400, d), parameters randn * 0.2 * min(1, sqrt(128 / d)) in float64, so |z| keeps the distribution of the d = 128
cases of the link, node and edge tests.  Bounds, on the scales of the edge test (Σ s·max(1, max|x|) over the rows of the sum, squared
in the Hessian): 1e-6 of the scale for loss and gradient, 1e-5 of the squared scale for the Hessian, 1e-4 absolute for link-prediction
scores.  Predictions are compared on the rows whose float64 margin exceeds 1e-6 in every C group, and at most 1 % of a case's rows
may fall out.  Every case prints its worst error as a fraction of the bound and repeats every call for bit-identity.

Worst fractions of the bound measured on an MI355X, over the cases of a family (loss / gradient / Hessian / scores):
  link prediction   0.164 / 0.119 / 0.004 / 0.181   (loss and gradient at n = 1, scores at d = 256, n = 40000)
  node tables       0.500 / 0.186 / 0.010           (loss at d = 256, K = 32; the mixed, long and absent-class tables included)
  pair tables       0.257 / 0.368 / 0.007           (gradient at d = 132, K = 32)
No case needed a bound of its own.  At most 3 of a case's 1164 rows (0.26 %) fell out of the prediction comparison.
"""
import numpy as np
import pytest
import torch

import _logreg_ref as R
from ctgcn_amd.evaluation import _logreg, _ovr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
ROWS = 400                # rows of every embedding
NEAR_TIE = 1e-6
SIZES = [1, 33, 130, 1000]
B_LOSS, B_GRAD, B_HESS, B_SCORE = 1e-6, 1e-6, 1e-5, 1e-4


def _param_scale(d):
    return 0.2 * min(1.0, (128.0 / d) ** 0.5)


def _weights(n_neg, n_pos):
    """Balanced class weights n / (2 n_class), 0 for an absent class, written out here independently of the package."""
    n = n_neg + n_pos
    return (n / (2.0 * n_neg) if n_neg else 0.0), (n / (2.0 * n_pos) if n_pos else 0.0)


class _Worst:
    """Largest error / bound of a case, per quantity."""

    def __init__(self):
        self.f = {}

    def add(self, what, err, bound):
        self.f[what] = max(self.f.get(what, 0.0), float(err) / bound)

    def report(self, name):
        print("%s: %s of the bound" % (name, ", ".join("%s %.3f" % kv for kv in self.f.items())))
        over = {k: v for k, v in self.f.items() if not v <= 1.0}
        assert not over, "%s: over the bound by these factors: %s" % (name, over)


# ================================================================================================ link prediction (ctgcn_eval.hip)
def _lp_inputs(d, M, n, view):
    g = torch.Generator().manual_seed(1000 * d + 10 * M + n % 997)
    if view:                                              # lde = d + 3, first column offset 1: rows 4 bytes off any wider alignment
        E = torch.randn(ROWS, d + 3, generator=g).to(DEV)[:, 1:d + 1]
        assert E.stride(0) == d + 3 and E.stride(1) == 1 and E.storage_offset() == 1
    else:
        E = torch.randn(ROWS, d, generator=g).to(DEV)
    edges = torch.stack([torch.randint(0, ROWS, (n,), generator=g), torch.randint(0, ROWS, (n,), generator=g),
                         (torch.rand(n, generator=g) < 0.3).long()], 1)
    edges[0, 2] = 1
    if n > 1:
        edges[1, 2] = 0
    measures = [R.MEASURES[(m + d) % 4] for m in range(M)]       # cycles through all four: every half and group of models sees each
    assert M < 4 or all(set(measures[s:s + 4]) == set(R.MEASURES) for s in range(0, M - 3, 4))
    W = (torch.randn(M, d + 1, generator=g, dtype=torch.float64) * _param_scale(d)).to(DEV)
    return E, edges, measures, W


def _lp_run(E, edges, measures, W):
    es = _logreg.EdgeSet(edges.to(DEV), ROWS)
    out = [(*_logreg.loss_grad(E, es, measures, W), _logreg.hessian(E, es, measures, W), _logreg.scores(E, es, measures, W))
           for _ in range(2)]
    for a, b in zip(*out):
        assert torch.equal(a, b), "a second call differs"
    assert all(bool(torch.isfinite(a).all()) for a in out[0])
    return es, out[0]


LP_CASES = [
    # d sweep at M = 16: column groups of the gradient phase (4 up to d = 64, 2 up to 128, 1 above), KM = 4 / 8 / 16 models each
    pytest.param(1, 16, 1000, False, id="d1-M16-narrowest"),
    pytest.param(64, 16, 1000, False, id="d64-M16-last-of-4-groups-KM4"),
    pytest.param(65, 16, 1000, False, id="d65-M16-first-of-2-groups-KM8"),
    pytest.param(129, 16, 1000, False, id="d129-M16-one-group-KM16-hess9"),
    pytest.param(200, 16, 1000, False, id="d200-M16-one-group-hess9"),
    pytest.param(256, 16, 1000, False, id="d256-M16-column-255-hess9-2145-blocks-lds98k"),
    # model counts at d = 256: one model, second half of the models empty, one model in the second half
    pytest.param(256, 1, 1000, False, id="d256-M1"),
    pytest.param(256, 8, 1000, False, id="d256-M8-second-half-empty"),
    pytest.param(256, 9, 1000, False, id="d256-M9"),
    # row counts around one tile
    pytest.param(64, 16, 1, False, id="d64-M16-n1"),
    pytest.param(64, 16, 31, False, id="d64-M16-n31"),
    pytest.param(64, 16, 32, False, id="d64-M16-n32-full-tile"),
    pytest.param(64, 16, 33, False, id="d64-M16-n33-two-tiles"),
    # a strided view of a wider matrix
    pytest.param(200, 5, 1000, True, id="d200-M5-lde203-offset1-view"),
]


@pytest.mark.parametrize("d,M,n,view", LP_CASES)
def test_link_prediction_passes(d, M, n, view):
    E, edges, measures, W = _lp_inputs(d, M, n, view)
    es, (loss, grad, H, z) = _lp_run(E, edges, measures, W)
    En, Wn, ed = E.double().cpu().numpy(), W.cpu().numpy(), edges.numpy()
    a, b, y = En[ed[:, 0]], En[ed[:, 1]], ed[:, 2]
    w_neg, w_pos = _weights(int((y == 0).sum()), int((y == 1).sum()))
    assert (es.w_neg, es.w_pos) == (w_neg, w_pos)
    s = np.where(y > 0, w_pos, w_neg)
    worst = _Worst()
    for m, meas in enumerate(measures):
        X = R.features(meas, a, b)
        L, G, Href, zz = R.loss_grad_hess(X, y, w_neg, w_pos, Wn[m])
        scale, scale2 = R.error_scales(X, s)
        worst.add("loss", abs(loss[m].item() - L), B_LOSS * scale)
        worst.add("grad", np.abs(grad[m].cpu().numpy() - G).max(), B_GRAD * scale)
        worst.add("hess", np.abs(H[m].cpu().numpy() - Href).max(), B_HESS * scale2)
        worst.add("score", np.abs(z[m].double().cpu().numpy() - zz).max(), B_SCORE)
    worst.report("lp d %d M %d n %d%s" % (d, M, n, " view" if view else ""))


def _lp_ref_device(E, edges, w_neg, w_pos, meas, theta):
    """_logreg_ref.loss_grad_hess and error_scales of one measure in float64 torch on the device (the same formulas; checked against
    the numpy ones on a slice by the caller)."""
    Ed = E.double()
    a, b, y = Ed[edges[:, 0]], Ed[edges[:, 1]], edges[:, 2] > 0
    X = {"Avg": (a + b) / 2, "Had": a * b, "L1": (a - b).abs(), "L2": (a - b) ** 2}[meas]
    X1 = torch.cat([X, torch.ones(len(X), 1, dtype=torch.float64, device=X.device)], 1)
    s = torch.where(y, torch.tensor(w_pos, dtype=torch.float64, device=y.device), torch.tensor(w_neg, dtype=torch.float64, device=y.device))
    z = X1 @ theta
    sg = 0.5 * (1.0 + torch.tanh(0.5 * z))
    loss = (s * torch.logaddexp(torch.zeros_like(z), torch.where(y, -z, z))).sum()
    grad = X1.t() @ (s * (sg - y.double()))
    hess = (X1 * (s * sg * (1.0 - sg))[:, None]).t() @ X1
    big = X.abs().max(1).values.clamp(min=1.0)
    return loss.item(), grad, hess, z, float((s * big).sum()), float((s * big * big).sum())


def test_link_prediction_grid_stride_and_all_hessian_parts():
    """d = 256, M = 16, n = 40000: 1250 tiles on 1024 blocks (a block takes a second tile), 64 Hessian parts of 625 edges (not a
    multiple of the 32-edge tile), 98 KiB of LDS.  The reference runs in float64 torch on the device."""
    d, M, n = 256, 16, 40000
    E, edges, measures, W = _lp_inputs(d, M, n, False)
    es, (loss, grad, H, z) = _lp_run(E, edges, measures, W)
    ed = edges.to(DEV)
    w_neg, w_pos = _weights(es.n_neg, es.n_pos)
    assert es.n_neg == int((edges[:, 2] == 0).sum()) and (es.w_neg, es.w_pos) == (w_neg, w_pos)
    # the device formulas against the numpy reference, on the first 500 edges with the full set's weights
    En, k = E.double().cpu().numpy(), 500
    for m in (0, 1, 2, 3):
        Xs = R.features(measures[m], En[edges[:k, 0].numpy()], En[edges[:k, 1].numpy()])
        Ln, Gn, Hn, zn = R.loss_grad_hess(Xs, edges[:k, 2].numpy(), w_neg, w_pos, W[m].cpu().numpy())
        Lt, Gt, Ht, zt, sc, sc2 = _lp_ref_device(E, ed[:k], w_neg, w_pos, measures[m], W[m])
        ref = R.error_scales(Xs, np.where(edges[:k, 2].numpy() > 0, w_pos, w_neg))
        assert abs(Lt - Ln) <= 1e-12 * ref[0] and np.abs(Gt.cpu().numpy() - Gn).max() <= 1e-12 * ref[0]
        assert np.abs(Ht.cpu().numpy() - Hn).max() <= 1e-12 * ref[1] and np.abs(zt.cpu().numpy() - zn).max() <= 1e-12
        assert abs(sc - ref[0]) <= 1e-12 * ref[0] and abs(sc2 - ref[1]) <= 1e-12 * ref[1]
    worst = _Worst()
    for m, meas in enumerate(measures):
        L, G, Href, zz, scale, scale2 = _lp_ref_device(E, ed, w_neg, w_pos, meas, W[m])
        worst.add("loss", abs(loss[m].item() - L), B_LOSS * scale)
        worst.add("grad", (grad[m] - G).abs().max().item(), B_GRAD * scale)
        worst.add("hess", (H[m] - Href).abs().max().item(), B_HESS * scale2)
        worst.add("score", (z[m].double() - zz).abs().max().item(), B_SCORE)
    worst.report("lp d %d M %d n %d" % (d, M, n))


# ================================================================================================ node and pair tables (ctgcn_nodecls.hip)
def _problems(g, sizes, K, pair, classes=None):
    """Problems of the given sizes; labels random over `classes` (default all K), the first rows running through them so that every
    one of them occurs when the problem is long enough.  Pair problems: random endpoints, every fifth entry with u == v."""
    classes = torch.arange(K) if classes is None else torch.tensor(classes)
    out = []
    for n in sizes:
        y = classes[torch.randint(0, len(classes), (n,), generator=g)]
        y[:min(n, len(classes))] = classes[:min(n, len(classes))]
        u = torch.randint(0, ROWS, (n,), generator=g)
        v = None
        if pair:
            v = torch.randint(0, ROWS, (n,), generator=g)
            v[::5] = u[::5]
            v = v.to(DEV)
        out.append(_ovr.Problem(u.to(DEV), y.to(torch.int32).to(DEV), K, rows2=v))
    return out


def _run_table(tb, theta, probs):
    out = [(*tb.loss_grad(theta), tb.hessian(theta, 0, tb.P), *tb.predict(theta, probs)) for _ in range(2)]
    for a, b in zip(*out):
        assert torch.equal(a, b), "a second call differs"
    assert all(bool(torch.isfinite(a).all()) for a in out[0][:3])
    return out[0]


def _check_table(name, tb, E, probs, Cs, theta, outs, hess_max):
    """Every model's loss, gradient and subsample Hessian, and every problem's predictions and correct counts, against float64."""
    loss, grad, H, pred, correct = [o.cpu().numpy() for o in outs]
    En, th = E.double().cpu().numpy(), theta.cpu().numpy()
    worst, row, left_out, wrong, constant = _Worst(), 0, 0, 0, 0
    assert tb.M == sum(len(Cs) * _ovr.models_per_group(p.K) for p in probs) and loss.shape == (tb.M,)
    assert grad.shape == (tb.M, tb.d + 1) and H.shape == (tb.M, tb.d + 1, tb.d + 1)
    for pi, p in enumerate(probs):
        u, y = p.rows.cpu().numpy(), p.y.cpu().numpy().astype(np.int64)
        X = R.features("node", En[u]) if p.rows2 is None else R.features("Had", En[u], En[p.rows2.cpu().numpy()])
        n, mpg = len(u), _ovr.models_per_group(p.K)
        classes = [1] if p.K == 2 else list(range(p.K))
        sub = R.hess_subsample(n, hess_max)
        assert len(sub) == tb.n_sub[pi]
        m0 = int(tb.model_start_h[pi])
        assert int(tb.model_start_h[pi + 1]) - m0 == len(Cs) * mpg
        P = np.zeros((n, len(Cs), mpg))
        for k in range(len(Cs) * mpg):
            m, c = m0 + k, classes[k % mpg]
            yy = y == c
            n_pos = int(yy.sum())
            if n_pos == 0 or n_pos == n:                   # a constant column: not fitted, exact zeros, probability 0 or 1
                assert tb.flags_h[m] == (_ovr.FLAG_ZERO if n_pos == 0 else _ovr.FLAG_ONE)
                assert loss[m] == 0 and not grad[m].any() and not H[m].any()
                P[:, k // mpg, k % mpg] = 0.0 if n_pos == 0 else 1.0
                constant += 1
                continue
            assert tb.flags_h[m] == _ovr.FLAG_FIT
            w_neg, w_pos = _weights(n - n_pos, n_pos)
            L, G, Href, z = R.loss_grad_hess(X, yy, w_neg, w_pos, th[m], sub)
            P[:, k // mpg, k % mpg] = R.sigmoid(z)
            s = np.where(yy, w_pos, w_neg)
            scale, scale2 = R.error_scales(X, s)[0], R.error_scales(X[sub], s[sub])[1]
            worst.add("loss", abs(loss[m] - L), B_LOSS * scale)
            worst.add("grad", np.abs(grad[m] - G).max(), B_GRAD * scale)
            worst.add("hess", np.abs(H[m] - Href).max(), B_HESS * scale2)
            assert np.array_equal(H[m], H[m].T)
        ref_pred, margin = R.ovr_predict(P)
        got = pred[row:row + n]
        sure = margin > NEAR_TIE
        wrong += int((got[sure] != ref_pred[sure]).sum())
        left_out += int((~sure).any(1).sum())
        assert ((got >= 0) & (got < p.K)).all()
        assert np.array_equal(correct[pi], (got == y[:, None]).sum(0))
        row += n
    assert pred.shape == (row, len(Cs))
    print("%s: %d models (%d constant), %d of %d rows left out of the prediction comparison" % (name, tb.M, constant, left_out, row))
    worst.report(name)
    assert wrong == 0, "%s: %d predictions differ from float64 on rows with a margin above %g" % (name, wrong, NEAR_TIE)
    assert left_out <= 0.01 * row, "%s: %d of %d rows have a float64 margin within %g" % (name, left_out, row, NEAR_TIE)
    return worst


def _table_case(name, d, Ks, Cs, pair, sizes=SIZES, hess_max=256, classes=None):
    g = torch.Generator().manual_seed(100000 * int(pair) + 100 * d + 7 * max(Ks) + len(Cs))
    E = torch.randn(ROWS, d, generator=g).to(DEV)
    probs = []
    for i, n in enumerate(sizes):
        probs += _problems(g, [n], Ks[i % len(Ks)], pair, classes)
    kw = {} if hess_max is None else {"hess_max": hess_max}
    tb = _ovr.Table(E, probs, Cs, **kw)
    assert tb.pair == pair
    theta = (torch.randn(tb.M, d + 1, generator=g, dtype=torch.float64) * _param_scale(d)).to(DEV)
    outs = _run_table(tb, theta, probs)
    _check_table(name, tb, E, probs, Cs, theta, outs, tb.hess_max)
    return E, probs, tb, theta, outs


C7 = [0.01, 0.1, 1.0, 5.0, 10.0, 20.0, 50.0]
TABLE_CASES = [
    pytest.param(127, 64, [1.0], id="d127-K64-64-models-one-block-ML64-stride-bump"),
    pytest.param(131, 22, [0.1, 1.0, 10.0], id="d131-K22-66-models-two-blocks-last-64-wide-d"),
    pytest.param(132, 11, [0.1, 1.0, 10.0], id="d132-K11-33-models-two-blocks-first-32-wide-d"),
    pytest.param(132, 32, [0.1, 1.0, 10.0], id="d132-K32-three-blocks-predict-one-group-per-block"),
    pytest.param(200, 5, C7, id="d200-K5-35-models-predict-6-of-7-groups-per-block-hess9"),
    pytest.param(256, 32, [0.1, 1.0], id="d256-K32-64-models-two-blocks-lds104k-hess9"),
    pytest.param(256, 2, [0.1, 1.0, 10.0], id="d256-K2-three-models-ML8"),
    pytest.param(255, 5, C7, id="d255-K5-stride-bump-at-256"),
    pytest.param(1, 2, [1.0], id="d1-K2-one-model"),
    pytest.param(3, 3, [0.1, 1.0], id="d3-K3-stride-bump-at-4"),
    pytest.param(64, 9, [0.1, 1.0, 10.0], id="d64-K9-27-models-ML32"),
]


@pytest.mark.parametrize("d,K,Cs", TABLE_CASES)
def test_node_table_passes(d, K, Cs):
    _table_case("node d %d K %d |C| %d" % (d, K, len(Cs)), d, [K], Cs, False)


@pytest.mark.parametrize("d,K,Cs", [
    pytest.param(131, 22, [0.1, 1.0, 10.0], id="d131-K22-66-models-two-blocks"),
    pytest.param(132, 32, [0.1, 1.0, 10.0], id="d132-K32-three-blocks-float4-staging"),
    pytest.param(256, 32, [0.1, 1.0], id="d256-K32-lds104k-float4-staging-two-passes"),
])
def test_pair_table_passes(d, K, Cs):
    _table_case("pair d %d K %d |C| %d" % (d, K, len(Cs)), d, [K], Cs, True)


@pytest.mark.parametrize("d,Ks,Cs", [
    pytest.param(128, [2, 7, 3, 5], [0.01, 0.03, 0.1, 0.3, 1.0, 3.0, 10.0, 30.0, 100.0, 300.0], id="d128-K2-7-3-5-ten-C"),
    pytest.param(200, [2, 32, 3], [0.1, 1.0], id="d200-K2-32-3-two-C"),
])
def test_mixed_class_counts_in_one_table(d, Ks, Cs):
    """Problems of different K in one table: the launcher sizes the predict blocks from max(K) and the kernel recomputes the groups
    per block for each problem, the gradient pass launches ⌈max models / block⌉ model blocks for every problem.  Each problem must
    come out as it does alone in its own table, bit for bit, and match float64."""
    sizes = SIZES                                          # the class counts cycle over the four problems
    E, probs, tb, theta, (loss, grad, H, pred, correct) = _table_case("mixed d %d K %s |C| %d" % (d, Ks, len(Cs)), d, Ks, Cs, False)
    assert [p.K for p in probs] == [Ks[i % len(Ks)] for i in range(len(sizes))] and len({p.K for p in probs}) == len(Ks)
    row = 0
    for pi, p in enumerate(probs):
        m0, m1 = int(tb.model_start_h[pi]), int(tb.model_start_h[pi + 1])
        alone = _ovr.Table(E, [p], Cs, hess_max=256)
        la, ga, Ha, pa, ca = _run_table(alone, theta[m0:m1], [p])
        assert torch.equal(la, loss[m0:m1]) and torch.equal(ga, grad[m0:m1]), "problem %d (K = %d)" % (pi, p.K)
        assert torch.equal(Ha, H[m0:m1]), "problem %d (K = %d)" % (pi, p.K)
        assert torch.equal(pa, pred[row:row + sizes[pi]]) and torch.equal(ca[0], correct[pi]), "problem %d (K = %d)" % (pi, p.K)
        row += sizes[pi]


def test_long_problem_reaches_the_chunk_and_part_caps():
    """d = 37, K = 3, n = 140000 at the default hess_max = 131072: ⌈n / 128⌉ = 1094 pass chunks capped at 1024 (a chunk takes a fifth
    tile), the Hessian on every second row, 70000 rows in ⌈70000 / 1024⌉ = 69 parts capped at 64 of 1094 rows."""
    n = 140000
    E, probs, tb, theta, outs = _table_case("node d 37 K 3 n %d" % n, 37, [3], [1.0], False, sizes=[n], hess_max=None)
    assert tb.hess_max == 1 << 17 and tb.total_chunks == 1024 and int(tb.part_start_h[-1]) == 64 and int(tb.n_sub[0]) == 70000
    assert -(-70000 // 64) == 1094


def test_absent_class_gives_exact_zeros():
    """d = 200, K = 4 with class 2 absent from every problem's rows: its models are constant (probability 0), not fitted, and their
    loss, gradient and Hessian are exact zeros (_check_table asserts that for every constant column)."""
    Cs = [0.1, 1.0, 10.0]
    E, probs, tb, theta, (loss, grad, H, pred, correct) = _table_case("node d 200 K 4 class 2 absent", 200, [4], Cs, False,
                                                                      classes=[0, 1, 3])
    absent = [m for m in range(tb.M) if tb.m_cls[m] == 2]
    assert len(absent) == len(Cs) * len(probs) and all(tb.flags_h[m] == _ovr.FLAG_ZERO for m in absent)
    assert loss[absent].abs().max().item() == 0 and grad[absent].abs().max().item() == 0 and H[absent].abs().max().item() == 0
    assert not bool((pred == 2).any())
    # the 1000-row problem has every other class: only the absent one is constant there
    m0 = int(tb.model_start_h[3])
    assert [int(f) for f in tb.flags_h[m0:m0 + 4]] == [0, 0, _ovr.FLAG_ZERO, 0]


@pytest.mark.parametrize("d,K,limit", [pytest.param(132, 33, 32, id="d132-K33-over-32"), pytest.param(128, 65, 64, id="d128-K65-over-64")])
def test_predict_refuses_more_classes_than_a_block_holds(d, K, limit):
    """A C group's models share one block of the predict pass: at most 64 classes up to d = 131, 32 above.  predict() says so; the
    fit-side passes have no such limit (they split the models over blocks) and still run."""
    g = torch.Generator().manual_seed(d + K)
    E = torch.randn(ROWS, d, generator=g).to(DEV)
    assert _ovr.max_classes(d) == limit and _ovr.max_classes(d - 1 if d == 132 else d + 3) == 64
    probs = _problems(g, [130], K, False)
    tb = _ovr.Table(E, probs, [1.0], hess_max=256)
    theta = (torch.randn(tb.M, d + 1, generator=g, dtype=torch.float64) * _param_scale(d)).to(DEV)
    with pytest.raises(ValueError, match="%d classes, at most %d classes" % (K, limit)):
        tb.predict(theta, probs)
    # within the limit the same table kind predicts
    ok = _problems(g, [130], limit, False)
    tk = _ovr.Table(E, ok, [1.0], hess_max=256)
    pred, _ = tk.predict(theta[:tk.M], ok)
    assert pred.shape == (130, 1) and int(pred.min()) >= 0 and int(pred.max()) < limit


# ------------------------------------------------------------------------------------------------ pair staging vs materialised rows
@pytest.mark.parametrize("d", [pytest.param(4, id="d4-float4-one-quad"), pytest.param(124, id="d124-float4-bias-quad-31"),
                               pytest.param(252, id="d252-float4-two-passes-short-second"),
                               pytest.param(256, id="d256-float4-two-full-passes"), pytest.param(255, id="d255-scalar-staging")])
def test_pair_staging_equals_materialised_rows(d):
    """test_pair_path_equals_materialised_rows of the edge test at the other widths of the float4 staging (its bias-quad tail and
    its second pass of the quad loop) and at d = 255, which stages by the scalar loop: a node table on X = E[u] * E[v] (fp32) stages
    the same values, so every output is bit-identical.  Three entries have an endpoint outside [0, R) and read as zero features."""
    g = torch.Generator().manual_seed(7 + d)
    K, Cs = 3, [0.1, 1.0, 10.0]
    E = torch.randn(ROWS, d, generator=g).to(DEV)
    assert (E.data_ptr() % 16 == 0 and E.stride(0) % 4 == 0 and d % 4 == 0) == (d != 255)
    sizes = [1, 45, 300, 1000]
    pair = _problems(g, sizes, K, True)
    pair[2].rows[3], pair[2].rows2[4], pair[3].rows2[999] = -1, ROWS, ROWS + 5
    u, v = torch.cat([p.rows for p in pair]), torch.cat([p.rows2 for p in pair])
    inside = ((u >= 0) & (u < ROWS) & (v >= 0) & (v < ROWS))
    X = torch.where(inside[:, None], E[u.clamp(0, ROWS - 1)] * E[v.clamp(0, ROWS - 1)], torch.zeros((), device=DEV)).contiguous()
    assert int((~inside).sum()) == 3 and X[~inside].abs().max().item() == 0
    offs = np.concatenate([[0], np.cumsum(sizes)])
    node = [_ovr.Problem(torch.arange(offs[i], offs[i + 1], device=DEV), p.y, K) for i, p in enumerate(pair)]
    tp, tn = _ovr.Table(E, pair, Cs, hess_max=256), _ovr.Table(X, node, Cs, hess_max=256)
    assert tp.pair and not tn.pair and tp.total_chunks == tn.total_chunks
    theta = (torch.randn(tp.M, d + 1, generator=g, dtype=torch.float64) * _param_scale(d)).to(DEV)
    for a, b in zip(_run_table(tp, theta, pair), _run_table(tn, theta, node)):
        assert torch.equal(a, b)
