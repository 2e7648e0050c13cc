"""The batched Newton driver (ctgcn_amd/evaluation/_newton.py) on the CPU, through the one-vs-rest adapter _ovr.fit: the kernels'
passes are replaced by dense torch fp64 sums on the tiny reference cases of node_classification_uci.npz (90-160 rows, d <= 8), and
the results are held against numpy formulas written here.  Nothing is loaded from the shared library."""
import os

import numpy as np
import pytest
import torch

from ctgcn_amd.evaluation import _newton, _ovr
from ctgcn_amd.evaluation._logreg import balanced_weights

GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "node_classification_uci.npz"))
C_LIST = [float(c) for c in GOLD["C_list"]]
CASES = ["k2", "absent", "ties"]
TOL = 1e-10


def _case(case):
    gk = lambda k: GOLD["edge_%s_%s" % (case, k)]
    tr = gk("train")
    return gk("emb")[tr].astype(np.float64), gk("y")[tr].astype(np.int64), int(gk("K"))


class DenseTable:
    """What _ovr.fit reads of an _ovr.Table, for one problem (X [n, d] float64, y in [0, K)), with dense fp64 passes."""

    def __init__(self, X, y, K, C_list):
        n, self.d = X.shape
        self.E = torch.from_numpy(X)
        self.X1 = torch.cat([self.E, torch.ones(n, 1, dtype=torch.float64)], 1)
        self.m_problem, self.m_cls, self.m_C, self.m_n = [], [], [], []
        Y, S, flags = [], [], []
        for C in C_list:
            for c in ([1] if K == 2 else range(K)):
                pos = y == c
                w_neg, w_pos = balanced_weights(int((~pos).sum()), int(pos.sum()))
                self.m_problem.append(0), self.m_cls.append(c), self.m_C.append(C), self.m_n.append(n)
                Y.append(pos.astype(np.float64))
                S.append(np.where(pos, w_pos, w_neg))
                flags.append(_ovr.FLAG_ZERO if not pos.any() else (_ovr.FLAG_ONE if pos.all() else _ovr.FLAG_FIT))
        self.Y, self.S = torch.from_numpy(np.array(Y)), torch.from_numpy(np.array(S))
        self.M = len(flags)
        self.flags_h = np.array(flags, dtype=np.int32)
        self.model_flag = torch.from_numpy(self.flags_h)
        self.model_start_h = np.array([0, self.M], dtype=np.int32)
        self.n_sub = np.array([n], dtype=np.int64)

    def hess_chunks(self):
        return [(0, 1)]

    def loss_grad(self, theta, flags=None):
        skip = (self.model_flag if flags is None else flags) != 0
        z = theta @ self.X1.t()
        loss = (self.S * torch.nn.functional.softplus(torch.where(self.Y > 0, -z, z))).sum(1)
        grad = (self.S * (torch.sigmoid(z) - self.Y)) @ self.X1
        loss[skip] = 0
        grad[skip] = 0
        return loss, grad

    def hessian(self, theta, p0, p1, flags=None):
        skip = (self.model_flag if flags is None else flags) != 0
        sg = torch.sigmoid(theta @ self.X1.t())
        H = torch.einsum("mn,nj,nk->mjk", self.S * sg * (1 - sg), self.X1, self.X1)
        H[skip] = 0
        return H


def _np_grad(tb, m, theta):
    """∇f of model m in sklearn's scaling, in numpy."""
    X1, y, s, n = tb.X1.numpy(), tb.Y[m].numpy(), tb.S[m].numpy(), tb.m_n[m]
    g = X1.T @ (s * (1.0 / (1.0 + np.exp(-(X1 @ theta))) - y)) / n
    g[:-1] += theta[:-1] / (tb.m_C[m] * n)
    return g


def _np_newton(tb, m):
    """Plain Newton on model m from zero until max|∇f| <= TOL, a step halved while it does not lower max|∇f|."""
    X1, s, n = tb.X1.numpy(), tb.S[m].numpy(), tb.m_n[m]
    reg = np.diag(np.r_[np.full(tb.d, 1.0 / (tb.m_C[m] * n)), 0.0])
    theta = np.zeros(tb.d + 1)
    for _ in range(100):
        g = _np_grad(tb, m, theta)
        if np.abs(g).max() <= TOL:
            break
        sg = 1.0 / (1.0 + np.exp(-(X1 @ theta)))
        p = np.linalg.solve((X1 * (s * sg * (1 - sg))[:, None]).T @ X1 / n + reg, g)
        t = 1.0
        while np.abs(_np_grad(tb, m, theta - t * p)).max() >= np.abs(g).max() and t > 1e-6:
            t *= 0.5
        theta = theta - t * p
    return theta


@pytest.mark.parametrize("case", CASES)
def test_fits_reach_the_optimum(case):
    tb = DenseTable(*_case(case), C_LIST)
    theta, reports = _ovr.fit(tb, tol=TOL, max_iter=100)
    theta = theta.numpy()
    fitted = tb.flags_h == _ovr.FLAG_FIT
    assert fitted.any()
    if case == "absent":
        assert (~fitted).sum() == len(C_LIST)
    for m, r in enumerate(reports):
        assert (r.problem, r.cls, r.C) == (0, tb.m_cls[m], tb.m_C[m])
        if not fitted[m]:                      # a constant predictor is outside the fitted mask: never touched
            assert r.constant and r.converged and r.iterations == 0 and r.grad_norm == 0 and not theta[m].any()
            continue
        g = np.abs(_np_grad(tb, m, theta[m])).max()
        print(case, m, "iterations", r.iterations, "max|grad|", g, "reported", r.grad_norm)
        assert not r.constant and r.converged and r.iterations >= 1
        assert g <= TOL
        ref = _np_newton(tb, m)
        assert np.abs(_np_grad(tb, m, ref)).max() <= TOL
        gap = np.abs(theta[m] - ref).max()
        print(case, m, "theta gap to the numpy Newton", gap)
        assert gap <= 1e-9


def test_start_within_tol_takes_no_iteration():
    tb = DenseTable(*_case("k2"), C_LIST)
    at_zero = max(np.abs(_np_grad(tb, m, np.zeros(tb.d + 1))).max() for m in range(tb.M))
    theta, reports = _ovr.fit(tb, tol=2 * at_zero, max_iter=100)
    assert not theta.numpy().any()
    assert all(r.converged and r.iterations == 0 and r.grad_norm <= 2 * at_zero for r in reports)


def test_max_iter_is_reported_and_warned():
    tb = DenseTable(*_case("ties"), C_LIST)
    _, full = _ovr.fit(tb, tol=TOL, max_iter=100)
    assert min(r.iterations for r in full) > 1
    with pytest.warns(RuntimeWarning, match="did not converge"):
        theta, reports = _ovr.fit(tb, tol=TOL, max_iter=1)
    assert all(not r.converged and r.iterations == 1 and r.grad_norm > TOL for r in reports)
    for m in range(tb.M):
        assert np.abs(_np_grad(tb, m, theta[m].numpy())).max() == pytest.approx(reports[m].grad_norm, rel=1e-9)


def test_driver_alone_on_a_quadratic():
    """minimize() needs nothing of the adapters: two quadratics 0.5 xᵀA x - bᵀx, one of them outside `fitted`."""
    A = torch.tensor([[[2.0, 0.5], [0.5, 1.0]], [[1.0, 0.0], [0.0, 3.0]]], dtype=torch.float64)
    b = torch.tensor([[1.0, -1.0], [2.0, 0.5]], dtype=torch.float64)
    fitted = torch.tensor([True, False])

    def objective(x, live):
        Ax = torch.einsum("mjk,mk->mj", A, x)
        g = Ax - b
        g[~fitted] = 0
        return 0.5 * (x * Ax).sum(1) - (b * x).sum(1), g

    x, iters, gmax = _newton.minimize(torch.zeros(2, 2, dtype=torch.float64), objective, lambda x, active: [(0, 2, A.clone())], 1e-12, 10,
                                      fitted)
    assert iters == [1, 0] and gmax[0] <= 1e-12 and gmax[1] == 0
    assert torch.allclose(x[0], torch.linalg.solve(A[0], b[0]), rtol=0, atol=1e-14) and not x[1].any()
