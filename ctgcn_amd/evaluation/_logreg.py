"""Balanced L2 logistic regression on edge features, fitted on the GPU (ctgcn_eval.hip).

The model the reference fits (evaluation/link_prediction.py: LogisticRegression(C, lbfgs, class_weight='balanced')) minimises, in
sklearn's scaling (intercept not penalised),

    f(w, b) = (1/n) Σ_i s_i logloss(y_i, w·φ_i + b) + ||w||² / (2 C n),    s_i = n / (2 n_{class(y_i)}),

which is strictly convex: one optimum, fixed by ∇f = 0 alone.  fit() runs Newton's method with Armijo backtracking on all models at
once: one fused pass gives f and ∇f of every model (the edge features are formed in registers from the two gathered embedding rows,
never stored), one pass gives the Hessians (on a deterministic strided subsample of at most `hess_max` edges: its precision only
changes the number of iterations), and one batched fp64 Cholesky solves all Newton systems.  A model stops when max |∇f| <= tol.
"""
import warnings
from dataclasses import dataclass
from functools import partial

import torch

from .. import _lib
from .._lib import check, ptr
from . import _common, _newton
from ._common import stream as _stream

MEASURES = ("Avg", "Had", "L1", "L2")
MAX_MODELS = 16          # models per kernel pass (ctgcn_eval.hip); more are fitted in several groups


require_cuda = partial(_common.require_cuda, task="link-prediction")


def measure_code(measures):
    code = 0
    for m, name in enumerate(measures):
        code |= MEASURES.index(name) << (2 * m)
    return code


def balanced_weights(n_neg, n_pos):
    """sklearn's compute_class_weight('balanced'): n / (n_classes * bincount), for labels 0 and 1 (0 for an absent class)."""
    n = n_neg + n_pos
    return (n / (2.0 * n_neg) if n_neg else 0.0), (n / (2.0 * n_pos) if n_pos else 0.0)


class EdgeSet:
    """One split as the kernels read it: src, dst int64, label uint8 on the embedding's device, plus balanced class weights."""

    def __init__(self, edges, n_nodes):
        require_cuda(edges, "edge array")
        edges = edges.to(torch.int64)
        if edges.dim() != 2 or edges.shape[1] != 3:
            raise ValueError("edges must be [n, 3] (from_id, to_id, label)")
        self.src = edges[:, 0].contiguous()
        self.dst = edges[:, 1].contiguous()
        self.label = (edges[:, 2] != 0).to(torch.uint8).contiguous()
        self.n = edges.shape[0]
        if self.n and (int(torch.minimum(self.src.min(), self.dst.min())) < 0 or int(torch.maximum(self.src.max(), self.dst.max())) >= n_nodes):
            raise ValueError("edge endpoint outside [0, %d)" % n_nodes)
        self.n_pos = int(self.label.sum()) if self.n else 0
        self.n_neg = self.n - self.n_pos
        self.w_neg, self.w_pos = balanced_weights(self.n_neg, self.n_pos)

    def subsample(self, limit):
        """Every k-th edge (k = ceil(n / limit)), weights of the full set kept; self when n <= limit."""
        if self.n <= limit:
            return self
        k = -(-self.n // limit)
        sub = EdgeSet.__new__(EdgeSet)
        sub.src, sub.dst, sub.label = self.src[::k].contiguous(), self.dst[::k].contiguous(), self.label[::k].contiguous()
        sub.n = sub.src.shape[0]
        sub.n_pos = int(sub.label.sum())
        sub.n_neg = sub.n - sub.n_pos
        sub.w_pos, sub.w_neg = self.w_pos, self.w_neg
        return sub


def _check_emb(E):
    require_cuda(E, "embedding")
    if E.dtype != torch.float32 or E.dim() != 2 or E.stride(1) != 1:
        raise ValueError("embedding must be a float32 [N, d] tensor with unit column stride")
    if not 1 <= E.shape[1] <= 256:
        raise ValueError("embedding width d must be in [1, 256]")


def _hi_lo(W):
    """[2, M, d+1] float32: W as hi + lo (W float64), or W and zeros."""
    hi = W.to(torch.float32)
    lo = (W - hi.to(W.dtype)).to(torch.float32) if W.dtype == torch.float64 else torch.zeros_like(hi)
    return torch.stack([hi, lo]).contiguous()


def loss_grad(E, es, measures, W):
    """Σ s_i logloss (double[M]) and Σ s_i (σ - y)(φ, 1) (double[M, d+1]) of the models W ([M, d+1], fp32 or fp64) on edge set es."""
    _check_emb(E)
    M, d = W.shape[0], E.shape[1]
    lib = _lib.load()
    loss = torch.empty(M, dtype=torch.float64, device=E.device)
    grad = torch.empty(M, d + 1, dtype=torch.float64, device=E.device)
    ws = torch.empty(max(1, lib.ctgcn_lp_grad_workspace_bytes(es.n, d, M)), dtype=torch.uint8, device=E.device)
    W = _hi_lo(W)
    check(lib.ctgcn_lp_grad_f32(es.n, d, M, measure_code(measures), E.shape[0], ptr(E), E.stride(0), ptr(es.src), ptr(es.dst),
                                ptr(es.label), es.w_neg, es.w_pos, ptr(W), ptr(loss), ptr(grad), ptr(ws), ws.numel(), _stream()),
          "ctgcn_lp_grad_f32")
    return loss, grad


def hessian(E, es, measures, W):
    """Σ s_i σ(1-σ)(φ, 1)(φ, 1)ᵀ (double[M, d+1, d+1])."""
    _check_emb(E)
    M, d = W.shape[0], E.shape[1]
    lib = _lib.load()
    hess = torch.empty(M, d + 1, d + 1, dtype=torch.float64, device=E.device)
    ws = torch.empty(max(1, lib.ctgcn_lp_hess_workspace_bytes(es.n, d, M)), dtype=torch.uint8, device=E.device)
    W = W.to(torch.float32).contiguous()
    check(lib.ctgcn_lp_hess_f32(es.n, d, M, measure_code(measures), E.shape[0], ptr(E), E.stride(0), ptr(es.src), ptr(es.dst),
                                ptr(es.label), es.w_neg, es.w_pos, ptr(W), ptr(hess), ptr(ws), ws.numel(), _stream()),
          "ctgcn_lp_hess_f32")
    return hess


def scores(E, es, measures, W):
    """z = w·φ + b of every model on every edge (float32 [M, n])."""
    _check_emb(E)
    M, d = W.shape[0], E.shape[1]
    out = torch.empty(M, es.n, dtype=torch.float32, device=E.device)
    W = _hi_lo(W)
    check(_lib.load().ctgcn_lp_scores_f32(es.n, d, M, measure_code(measures), E.shape[0], ptr(E), E.stride(0), ptr(es.src), ptr(es.dst),
                                          ptr(W), ptr(out), _stream()), "ctgcn_lp_scores_f32")
    return out


@dataclass
class FitReport:
    measure: str
    C: float
    converged: bool
    iterations: int
    grad_norm: float      # max |∇f| of sklearn's scaled objective at the returned parameters


def _fit_group(E, es, hs, measures, Cs, tol, max_iter):
    M, D1 = len(measures), E.shape[1] + 1
    dev = E.device
    inv_cn = torch.tensor([1.0 / (C * es.n) for C in Cs], dtype=torch.float64, device=dev)
    reg = torch.zeros(M, D1, D1, dtype=torch.float64, device=dev)
    idx = torch.arange(D1 - 1, device=dev)
    reg[:, idx, idx] = inv_cn[:, None]

    def objective(theta, live):                 # every model of a group is evaluated: the pass has no per-model skip
        loss, g = loss_grad(E, es, measures, theta)
        w = theta[:, :-1]
        f = loss / es.n + 0.5 * inv_cn * (w * w).sum(1)
        g = g / es.n
        g[:, :-1] += inv_cn[:, None] * w
        return f, g

    def hessians(theta, active):                # one call on the strided subsample; inactive systems are solved as they are
        yield 0, M, hessian(E, hs, measures, theta.to(torch.float32)) / hs.n + reg

    theta, iters, gmax = _newton.minimize(torch.zeros(M, D1, dtype=torch.float64, device=dev), objective, hessians, tol, max_iter)
    return theta, [FitReport(measures[m], float(Cs[m]), gmax[m] <= tol, iters[m], gmax[m]) for m in range(M)]


def groups(n_models):
    """The [s, e) ranges of at most MAX_MODELS models that one kernel pass takes."""
    return [(s, min(s + MAX_MODELS, n_models)) for s in range(0, n_models, MAX_MODELS)]


def fit(E, train, measures, Cs, tol=1e-6, max_iter=100, hess_max=1 << 18):
    """Fit one model per (measures[m], Cs[m]) on the EdgeSet train.  Returns theta (double[M, d+1], w then b) and the FitReports.
    A model that does not reach tol is reported (converged=False) and warned about."""
    _check_emb(E)
    if train.n_pos == 0 or train.n_neg == 0:
        raise ValueError("This solver needs samples of at least 2 classes in the data, but the train set has only one class")
    hs = train.subsample(hess_max)
    thetas, reports = [], []
    for s, e in groups(len(measures)):
        th, rep = _fit_group(E, train, hs, list(measures[s:e]), list(Cs[s:e]), tol, max_iter)
        thetas.append(th)
        reports += rep
    for r in reports:
        if not r.converged:
            warnings.warn("logistic regression (%s, C=%g) did not converge: max|grad| %.3g > tol %.3g after %d Newton iterations"
                          % (r.measure, r.C, r.grad_norm, tol, r.iterations), RuntimeWarning)
    return torch.cat(thetas), reports


def scores_all(E, es, measures, W):
    """scores() of any number of models, MAX_MODELS per pass."""
    return torch.cat([scores(E, es, measures[s:e], W[s:e]) for s, e in groups(len(measures))])


def roc_auc(labels, score):
    """sklearn roc_auc_score semantics in float64 (ties take midranks).  labels, score: 1-D tensors on one device."""
    y = labels.to(torch.bool).flatten()
    s = score.to(torch.float64).flatten()
    n_pos = int(y.sum())
    n_neg = y.numel() - n_pos
    if n_pos == 0 or n_neg == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    s_sorted, order = torch.sort(s, stable=True)
    _, inverse, counts = torch.unique_consecutive(s_sorted, return_inverse=True, return_counts=True)
    start = torch.cumsum(counts, 0) - counts
    midrank = start.to(torch.float64) + (counts.to(torch.float64) + 1.0) / 2.0
    rank_pos = midrank[inverse][y[order]].sum()
    return float((rank_pos - n_pos * (n_pos + 1) / 2.0) / (float(n_pos) * float(n_neg)))
