"""The float64 logistic-regression reference (_logreg_ref.py) pinned on the CPU: its gradient and Hessian against float64 torch
autograd of the loss written independently, its predictions against a direct loop, its subsample against the row-count arithmetic of
_ovr.Table, its scales against a loop.  The GPU sweeps (test_gpu_logreg_shapes.py) compare the kernels with this module only."""
import numpy as np
import pytest
import torch

import _logreg_ref as R


def _case(n, d, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, d))
    y = (rng.random(n) < 0.35).astype(np.int64)
    theta = rng.standard_normal(d + 1) * 0.3
    return X, y, theta


@pytest.mark.parametrize("n,d", [(1, 1), (50, 3), (300, 37), (200, 130), (64, 256)])
def test_loss_grad_hess_match_float64_autograd(n, d):
    X, y, theta = _case(n, d, 100 * n + d)
    w_neg, w_pos = 0.7, 2.3
    sub = R.hess_subsample(n, 40)
    loss, grad, hess, z = R.loss_grad_hess(X, y, w_neg, w_pos, theta, sub)
    Xt = torch.cat([torch.from_numpy(X), torch.ones(n, 1, dtype=torch.float64)], 1)
    yt = torch.from_numpy(y).double()
    st = torch.where(yt > 0, torch.tensor(w_pos, dtype=torch.float64), torch.tensor(w_neg, dtype=torch.float64))

    def f(th, rows):
        zz = Xt[rows] @ th
        return (st[rows] * torch.nn.functional.binary_cross_entropy_with_logits(zz, yt[rows], reduction="none")).sum()

    every = torch.arange(n)
    th = torch.from_numpy(theta).clone().requires_grad_(True)
    L = f(th, every)
    L.backward()
    Hs = torch.autograd.functional.hessian(lambda t: f(t, torch.from_numpy(sub)), torch.from_numpy(theta))
    scale = float(st.sum()) * max(1.0, float(np.abs(X).max())) ** 2
    assert abs(loss - L.item()) <= 1e-13 * scale
    assert np.abs(grad - th.grad.numpy()).max() <= 1e-13 * scale
    assert np.abs(hess - Hs.numpy()).max() <= 1e-13 * scale
    assert np.abs(hess - hess.T).max() <= 1e-13 * scale
    assert np.abs(z - (Xt @ torch.from_numpy(theta)).numpy()).max() <= 1e-13 * (1 + np.abs(z).max())
    # sub=None is every row
    assert np.array_equal(R.loss_grad_hess(X, y, w_neg, w_pos, theta)[2], R.loss_grad_hess(X, y, w_neg, w_pos, theta, np.arange(n))[2])


def test_sigmoid_and_softplus_hold_at_large_arguments():
    z = np.array([-800.0, -40.0, 0.0, 40.0, 800.0])
    assert np.array_equal(R.sigmoid(z), [0.0, R.sigmoid(-40.0), 0.5, R.sigmoid(40.0), 1.0])
    X = z[:, None]
    loss, grad, hess, _ = R.loss_grad_hess(X, [1, 1, 0, 0, 0], 1.0, 1.0, [1.0, 0.0])
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(hess).all()
    assert abs(loss - (800.0 + 40.0 + np.log(2.0) + 40.0 + 800.0)) <= 1e-12 * 1680


def test_features():
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((7, 4)).astype(np.float32), rng.standard_normal((7, 4)).astype(np.float32)
    ad, bd = a.astype(np.float64), b.astype(np.float64)
    for i in range(7):
        for j in range(4):
            assert R.features("Avg", a, b)[i, j] == (ad[i, j] + bd[i, j]) / 2
            assert R.features("Had", a, b)[i, j] == ad[i, j] * bd[i, j]
            assert R.features("L1", a, b)[i, j] == abs(ad[i, j] - bd[i, j])
            assert R.features("L2", a, b)[i, j] == (ad[i, j] - bd[i, j]) ** 2
    assert R.features("node", a).dtype == np.float64 and np.array_equal(R.features("node", a), ad)
    assert all(R.features(m, a, b).dtype == np.float64 for m in R.MEASURES)
    with pytest.raises(ValueError):
        R.features("cosine", a, b)


def _predict_loop(P):
    n, G, mpg = P.shape
    pred, margin = np.zeros((n, G), np.int64), np.zeros((n, G))
    for i in range(n):
        for g in range(G):
            if mpg == 1:
                p = P[i, g, 0]
                pred[i, g] = 1 if p > 1 - p else 0
                margin[i, g] = abs(2 * p - 1)
                continue
            best, bp, second = 0, P[i, g, 0], -np.inf
            for k in range(1, mpg):
                if P[i, g, k] > bp:
                    best, bp, second = k, P[i, g, k], bp
                elif P[i, g, k] > second:
                    second = P[i, g, k]
            pred[i, g], margin[i, g] = best, bp - second
    return pred, margin


@pytest.mark.parametrize("mpg", [1, 3, 7, 32])
def test_ovr_predict_matches_a_direct_loop(mpg):
    rng = np.random.default_rng(mpg)
    P = rng.random((200, 3, mpg))
    P[::7, :, mpg // 2] = 1.0          # a constant-one model wins (or ties with another one)
    P[::5, 1, 0] = 0.0                 # a constant-zero model
    P[3] = 0.5                         # every model tied: the first class (K = 2: p > 1 - p is false, class 0)
    if mpg > 1:
        P[4, :, -1] = P[4, :, 0] = 2.0  # first argmax among equals
    pred, margin = R.ovr_predict(P)
    lp, lm = _predict_loop(P)
    assert pred.dtype == np.int64 and np.array_equal(pred, lp)
    assert np.array_equal(margin, lm)
    assert (pred[3] == 0).all() and (margin[3] == 0).all()
    if mpg > 1:
        assert (pred[4] == 0).all() and (margin[4] == 0).all()
        assert (pred[0] == mpg // 2).all() or mpg // 2 == 0


def test_ovr_predict_constant_models_and_k2_rule():
    # K = 2: one model; constant 0 predicts class 0, constant 1 class 1, both with margin 1
    pred, margin = R.ovr_predict(np.array([[[0.0]], [[1.0]], [[0.5]], [[0.5 + 1e-9]]]))
    assert pred[:, 0].tolist() == [0, 1, 0, 1]
    assert margin[:2, 0].tolist() == [1.0, 1.0] and margin[2, 0] == 0.0 and 0 < margin[3, 0] < 1e-8
    # K = 3 with an absent class (constant 0): it never wins against a positive probability; a constant 1 always does
    pred, margin = R.ovr_predict(np.array([[[0.0, 0.2, 0.1]], [[0.3, 1.0, 0.9]], [[0.0, 0.0, 0.0]]]))
    assert pred[:, 0].tolist() == [1, 1, 0]
    np.testing.assert_allclose(margin[:, 0], [0.1, 0.1, 0.0], rtol=0, atol=1e-15)
    with pytest.raises(ValueError):
        R.ovr_predict(np.zeros((3, 2)))


def _table_n_sub(k, hess_max):
    """Table.n_sub of a problem of k rows (ctgcn_amd/evaluation/_ovr.py), the arithmetic alone."""
    return -(-k // (-(-k // hess_max) if k > hess_max else 1)) if k else 0


def test_hess_subsample_follows_the_documented_rule():
    sizes = [0, 1, 2, 31, 32, 33, 255, 256, 257, 511, 512, 513, 1000, 65536, 65537, 131072, 131073, 140000, 200000, 262145]
    for hess_max in (1, 7, 256, 1 << 16, 1 << 17, 1 << 18):
        for n in sizes:
            sub = R.hess_subsample(n, hess_max)
            assert sub.dtype == np.int64
            assert len(sub) == _table_n_sub(n, hess_max), (n, hess_max)
            assert len(sub) <= hess_max
            if n <= hess_max:
                assert np.array_equal(sub, np.arange(n))
            else:
                step = -(-n // hess_max)
                assert step >= 2 and np.array_equal(sub, np.arange(len(sub)) * step) and sub[-1] < n <= sub[-1] + step
    # the cases the GPU sweeps lean on
    assert len(R.hess_subsample(1000, 256)) == 250 and R.hess_subsample(1000, 256)[1] == 4
    assert len(R.hess_subsample(140000, 1 << 17)) == 70000
    with pytest.raises(ValueError):
        R.hess_subsample(10, 0)


def test_link_prediction_subsample_is_the_same_rule():
    """EdgeSet.subsample takes [::k] with k = ceil(n / limit) when n > limit: the same index set."""
    for n, limit in [(1000, 256), (40000, 1 << 18), (300000, 1 << 18), (7, 3)]:
        k = 1 if n <= limit else -(-n // limit)
        assert np.array_equal(R.hess_subsample(n, limit), np.arange(n)[::k])


def test_error_scales():
    rng = np.random.default_rng(9)
    X = rng.standard_normal((40, 6)) * 2
    X[0] = 0.01                         # below 1: the bias column's 1 is the row's largest entry
    s = rng.random(40) + 0.5
    a = sum(s[i] * max(1.0, max(abs(v) for v in X[i])) for i in range(40))
    b = sum(s[i] * max(1.0, max(abs(v) for v in X[i])) ** 2 for i in range(40))
    got = R.error_scales(X, s)
    assert abs(got[0] - a) <= 1e-12 * a and abs(got[1] - b) <= 1e-12 * b
    assert R.error_scales(np.full((3, 2), 0.5), np.array([1.0, 2.0, 3.0])) == (6.0, 6.0)
