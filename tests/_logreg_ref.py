"""Float64 reference of the three logistic-regression evaluations (link prediction, node and edge classification): plain numpy,
written from the formulas of ctgcn_amd/evaluation/_logreg.py and _ovr.py, never calling the library.

  features        the edge feature of a pair of rows (Avg, Had, L1, L2) or the row itself (node)
  loss_grad_hess  Σ s·softplus, Σ s(σ - y)(x, 1) and Σ s σ(1-σ)(x, 1)(x, 1)ᵀ of one weighted binary model
  ovr_predict     one-vs-rest predictions and margins from the per-model probabilities
  hess_subsample  the strided row subset the Hessian passes take
  error_scales    the scales the error bounds of the GPU tests are stated on

The sigmoid is 0.5(1 + tanh(z/2)) and the softplus logaddexp(0, ·): neither over- nor underflows, and neither is how the kernels
compute them.
"""
import numpy as np

MEASURES = ("Avg", "Had", "L1", "L2")


def sigmoid(z):
    return 0.5 * (1.0 + np.tanh(0.5 * np.asarray(z, dtype=np.float64)))


def features(kind, a, b=None):
    """[n, d] float64 features: of the row pairs (a, b) for a measure, of the rows a themselves for 'node'."""
    a = np.asarray(a, dtype=np.float64)
    if kind == "node":
        return a
    b = np.asarray(b, dtype=np.float64)
    if kind == "Avg":
        return (a + b) / 2
    if kind == "Had":
        return a * b
    if kind == "L1":
        return np.abs(a - b)
    if kind == "L2":
        return (a - b) ** 2
    raise ValueError("unknown feature kind %r" % (kind,))


def loss_grad_hess(X, y01, w_neg, w_pos, theta, sub=None):
    """Of the model theta ([d+1]: w then b) on the rows X [n, d] with labels y01 (0 / 1) and class weights (w_neg, w_pos):
    loss = Σ_i s_i softplus(∓z_i), grad [d+1] = Σ_i s_i (σ(z_i) - y_i)(x_i, 1), and hess [d+1, d+1] = Σ_{i in sub} s_i σ(1-σ)(x_i, 1)
    (x_i, 1)ᵀ on the row subset sub (all rows when None).  Also returns z [n]."""
    X = np.asarray(X, dtype=np.float64)
    theta = np.asarray(theta, dtype=np.float64)
    y = np.asarray(y01, dtype=np.float64)
    X1 = np.concatenate([X, np.ones((X.shape[0], 1))], 1)
    s = np.where(y > 0, float(w_pos), float(w_neg))
    z = X1 @ theta
    sg = sigmoid(z)
    loss = float((s * np.logaddexp(0.0, np.where(y > 0, -z, z))).sum())
    grad = X1.T @ (s * (sg - y))
    idx = np.arange(X.shape[0]) if sub is None else np.asarray(sub, dtype=np.int64)
    a = (s * sg * (1.0 - sg))[idx]
    hess = (X1[idx] * a[:, None]).T @ X1[idx]
    return loss, grad, hess, z


def ovr_predict(P):
    """P [n, groups, mpg]: the probability of each model of each C group on each row (a constant model contributes 0 or 1).
    mpg = 1 is the K = 2 rule: class 1 where p > 1 - p, margin |2p - 1|.  Otherwise the first argmax, margin = top minus second.
    Returns (pred int64 [n, groups], margin float64 [n, groups])."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim != 3:
        raise ValueError("P must be [n, groups, models per group]")
    if P.shape[2] == 1:
        p = P[:, :, 0]
        return (p > 1.0 - p).astype(np.int64), np.abs(2.0 * p - 1.0)
    srt = np.sort(P, 2)
    return P.argmax(2).astype(np.int64), srt[:, :, -1] - srt[:, :, -2]


def hess_subsample(n, hess_max):
    """Indices of the rows a Hessian pass takes of n: every row when n <= hess_max, else every step-th from 0 with
    step = ceil(n / hess_max)."""
    n, hess_max = int(n), int(hess_max)
    if hess_max < 1:
        raise ValueError("hess_max must be positive")
    step = 1 if n <= hess_max else -(-n // hess_max)
    return np.arange(0, n, step, dtype=np.int64)


def error_scales(X, s):
    """(Σ s_i max(1, max_j |x_ij|), Σ s_i max(1, max_j |x_ij|)²): a row's terms of the loss and the gradient are bounded by its
    weight times its largest |x| (at least the bias column's 1), squared in the Hessian."""
    X = np.asarray(X, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    big = np.maximum(1.0, np.abs(X).max(1)) if X.shape[1] else np.ones(X.shape[0])
    return float((s * big).sum()), float((s * big * big).sum())
