"""One-vs-rest balanced L2 logistic regressions of many node- or edge-classification problems, fitted together on the GPU
(ctgcn_nodecls.hip).

A problem is one (train rows, labels) set on the rows of one float32 embedding E [R, d] (several snapshots are passed as one stacked
[T·N, d] view and the row index carries the snapshot offset).  For each C of the problem's C list it owns one binary model per class
(K >= 3) or one model for class 1 (K = 2), as sklearn's OneVsRestClassifier on LabelBinarizer output does.  Each binary model minimises
sklearn's scaled objective (see _logreg.py), with the balanced weights of its own column; a column that is constant on the train
rows is sklearn's _ConstantPredictor (probability 0 or 1) and is not fitted.

fit() runs batched Newton over every model of every problem: per iteration one gradient pass and one Hessian pass over all problems
(each row tile gathered once for all models of its problem) and one batched fp64 Cholesky, in bounded chunks of models, with a per-model
active mask, by the driver of _newton.py.  A model stops when max |∇f| <= tol.

A pair problem (edge classification) carries a second index rows2: its feature is E[rows] ⊙ E[rows2], formed by the kernels while
they stage a tile (the ctgcn_ec_* entry points); nothing else differs, fit() included.
"""
import warnings
from dataclasses import dataclass
from functools import partial

import numpy as np
import torch

from .. import _lib
from .._lib import check, ptr
from . import _common, _newton
from ._common import stream as _stream
from ._logreg import _check_emb, _hi_lo, balanced_weights

FLAG_FIT, FLAG_ZERO, FLAG_ONE = 0, 1, 2
HESS_BYTES = 1 << 28          # bound on one Hessian call's partials and output


require_cuda = partial(_common.require_cuda, task="node-classification")


def _pair(problems):
    """True for pair problems, False for node problems; ValueError for a mixed list."""
    kinds = {p.rows2 is not None for p in problems}
    if len(kinds) > 1:
        raise ValueError("the problems of a table must all have rows2 (pair problems) or all lack it")
    return bool(kinds and kinds.pop())


def _cat_rows(problems, pair, task, dev):
    """(rows, rows2 or None, y) of the problems back to back; one dummy entry when there is none (the kernels read an entry pointer)."""
    for p in problems:
        _common.require_cuda(p.rows, "row index", task)
        _common.require_cuda(p.y, "labels", task)
        if pair:
            _common.require_cuda(p.rows2, "second row index", task)
            if p.rows2.numel() != p.rows.numel():
                raise ValueError("rows and rows2 of a pair problem must have the same length")
    rows = torch.cat([p.rows.reshape(-1).to(torch.int64) for p in problems]).contiguous()
    rows2 = torch.cat([p.rows2.reshape(-1).to(torch.int64) for p in problems]).contiguous() if pair else None
    y = torch.cat([p.y.reshape(-1).to(torch.int32) for p in problems]).contiguous()
    if rows.numel() == 0:
        rows = torch.zeros(1, dtype=torch.int64, device=dev)
        rows2 = torch.zeros(1, dtype=torch.int64, device=dev) if pair else None
        y = torch.zeros(1, dtype=torch.int32, device=dev)
    return rows, rows2, y


def models_per_group(K):
    return 1 if K == 2 else K


def max_classes(d):
    """The most classes predict() takes at width d: a C group's models share one block of the pass kernel (ctgcn_nodecls.hip)."""
    return 64 if d <= 131 else 32


@dataclass
class Problem:
    """One split on the embedding: rows (int64 CUDA, indices into E) and y (class index in [0, K), int32 CUDA).  With rows2 (int64 CUDA,
    parallel to rows) the feature of an entry is E[rows] ⊙ E[rows2] instead of E[rows]."""
    rows: torch.Tensor
    y: torch.Tensor
    K: int
    rows2: torch.Tensor = None


@dataclass
class FitReport:
    problem: int
    cls: int
    C: float
    converged: bool
    iterations: int
    grad_norm: float      # max |∇f| of sklearn's scaled objective at the returned parameters (0 for a constant predictor)
    constant: bool = False


class Table:
    """The kernels' problem table (include/ctgcn_hip.h) for a list of Problems and a shared C list, on the embedding's device."""

    def __init__(self, E, problems, C_list, hess_max=1 << 17):
        self.pair = _pair(problems)
        self.task = "edge-classification" if self.pair else "node-classification"
        if self.pair:
            _common.require_cuda(E, "embedding", self.task)
        _check_emb(E)
        dev = E.device
        lib = _lib.load()
        self.E, self.d, self.P = E, E.shape[1], len(problems)
        self.C_list = [float(c) for c in C_list]
        self.K = [int(p.K) for p in problems]
        n = [int(p.rows.numel()) for p in problems]
        self.n = n
        self.row_start_h = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
        if not problems:
            raise ValueError("no problem to fit")
        self.rows, self.rows2, self.y = _cat_rows(problems, self.pair, self.task, dev)
        self.row_start = torch.from_numpy(self.row_start_h).to(dev)
        chunk_start = np.concatenate([[0], np.cumsum([lib.ctgcn_nc_chunks(k) for k in n])]).astype(np.int64)
        self.total_chunks = int(chunk_start[-1])
        self.chunk_start = torch.from_numpy(chunk_start).to(dev)
        self.hess_max = int(hess_max)
        hp = [lib.ctgcn_nc_hess_parts(k, self.hess_max) for k in n]
        self.part_start_h = np.concatenate([[0], np.cumsum(hp)]).astype(np.int64)
        self.part_start = torch.from_numpy(self.part_start_h).to(dev)
        self.n_classes = torch.tensor(self.K, dtype=torch.int32, device=dev)
        G = len(self.C_list)
        mpp = [G * models_per_group(k) for k in self.K]
        self.model_start_h = np.concatenate([[0], np.cumsum(mpp)]).astype(np.int32)
        self.model_start = torch.from_numpy(self.model_start_h).to(dev)
        self.M = int(self.model_start_h[-1])
        self.max_models = max(mpp) if mpp else 1
        # per-model metadata (host): problem, class, C, balanced weights, flag
        self.m_problem, self.m_cls, self.m_C, self.m_n = [], [], [], []
        w, flags = [], []
        y_h = [p.y.reshape(-1).to(torch.int64).cpu().numpy() for p in problems]
        for pi, k in enumerate(self.K):
            counts = np.bincount(y_h[pi], minlength=k) if n[pi] else np.zeros(k, np.int64)
            classes = [1] if k == 2 else list(range(k))
            for C in self.C_list:
                for c in classes:
                    n_pos = int(counts[c])
                    n_neg = n[pi] - n_pos
                    self.m_problem.append(pi)
                    self.m_cls.append(c)
                    self.m_C.append(C)
                    self.m_n.append(n[pi])
                    w.append(balanced_weights(n_neg, n_pos))
                    flags.append(FLAG_ZERO if n_pos == 0 else (FLAG_ONE if n_neg == 0 else FLAG_FIT))
        self.model_pos = torch.tensor(self.m_cls, dtype=torch.int32, device=dev)
        self.model_w = torch.tensor(w, dtype=torch.float64, device=dev).reshape(-1, 2).contiguous()
        self.flags_h = np.array(flags, dtype=np.int32)
        self.model_flag = torch.from_numpy(self.flags_h).to(dev)
        self.n_sub = np.array([-(-k // (-(-k // self.hess_max) if k > self.hess_max else 1)) if k else 0 for k in n], dtype=np.int64)

    def _entry(self, which, rows, rows2):
        """The C entry point of this table's kind and its index arguments: (rows,) or (rows, rows2)."""
        lib = _lib.load()
        if self.pair:
            return getattr(lib, "ctgcn_ec_%s_f32" % which), (ptr(rows), ptr(rows2))
        return getattr(lib, "ctgcn_nc_%s_f32" % which), (ptr(rows),)

    def loss_grad(self, theta, flags=None):
        """Σ s_i logloss (double[M]) and Σ s_i (σ - y)(x, 1) (double[M, d+1]) of every model; theta [M, d+1] fp32 or fp64."""
        lib = _lib.load()
        E, d, M = self.E, self.d, self.M
        loss = torch.empty(M, dtype=torch.float64, device=E.device)
        grad = torch.empty(M, d + 1, dtype=torch.float64, device=E.device)
        total = self.total_chunks
        ws = torch.empty(max(1, lib.ctgcn_nc_grad_workspace_bytes(total, d, self.max_models)), dtype=torch.uint8, device=E.device)
        W = _hi_lo(theta)
        flags = self.model_flag if flags is None else flags
        fn, idx = self._entry("grad", self.rows, self.rows2)
        check(fn(self.P, d, self.max_models, ptr(self.row_start), ptr(self.chunk_start), total, *idx, ptr(self.y), ptr(self.model_start),
                 ptr(self.model_pos), ptr(self.model_w), ptr(flags), E.shape[0], ptr(E), E.stride(0), ptr(W), M, ptr(loss), ptr(grad),
                 ptr(ws), ws.numel(), _stream()), fn.__name__)
        return loss, grad

    def hessian(self, theta, p0, p1, flags=None):
        """Σ s_i σ(1-σ)(x, 1)(x, 1)ᵀ (double[models of problems p0..p1-1, d+1, d+1]) on each problem's subsample."""
        lib = _lib.load()
        E, d = self.E, self.d
        m0, m1 = int(self.model_start_h[p0]), int(self.model_start_h[p1])
        mm = int(max(self.model_start_h[p + 1] - self.model_start_h[p] for p in range(p0, p1)))
        hess = torch.empty(m1 - m0, d + 1, d + 1, dtype=torch.float64, device=E.device)
        if m1 == m0:
            return hess
        part_start = self.part_start[p0:p1 + 1] - int(self.part_start_h[p0])
        total = int(self.part_start_h[p1] - self.part_start_h[p0])
        ws = torch.empty(max(1, lib.ctgcn_nc_hess_workspace_bytes(total, d, mm)), dtype=torch.uint8, device=E.device)
        W = theta[m0:m1].to(torch.float32).contiguous()
        flags = (self.model_flag if flags is None else flags)[m0:m1]
        fn, idx = self._entry("hess", self.rows, self.rows2)
        check(fn(p1 - p0, d, mm, ptr(self.row_start[p0:]), ptr(part_start), total, self.hess_max, *idx, ptr(self.y),
                 ptr(self.model_start[p0:]), ptr(self.model_pos[m0:]), ptr(self.model_w[m0:]), ptr(flags), E.shape[0], ptr(E), E.stride(0),
                 ptr(W), m1 - m0, ptr(hess), ptr(ws), ws.numel(), _stream()), fn.__name__)
        return hess

    def hess_chunks(self):
        """Problem ranges [p0, p1) whose Hessian partials and outputs stay within HESS_BYTES."""
        D2 = (self.d + 1) ** 2
        out, p0 = [], 0
        while p0 < self.P:
            p1, parts, models, mm = p0, 0, 0, 0
            while p1 < self.P:
                k = int(self.model_start_h[p1 + 1] - self.model_start_h[p1])
                pp = int(self.part_start_h[p1 + 1] - self.part_start_h[p1])
                nm, nmm = models + k, max(mm, k)
                if p1 > p0 and ((parts + pp) * nmm * D2 * 4 + nm * D2 * 8 > HESS_BYTES):
                    break
                parts, models, mm, p1 = parts + pp, nm, nmm, p1 + 1
            out.append((p0, p1))
            p0 = p1
        return out

    def predict(self, theta, problems):
        """Predicted class of every entry of `problems` (Problems on the same embedding, one per problem of this table) for every C
        group (int32 [entries, |C|]) and correct counts per (problem, C) (int64 [P, |C|]), under this table's models theta."""
        lib = _lib.load()
        E = self.E
        n = [int(p.rows.numel()) for p in problems]
        if _pair(problems) != self.pair:
            raise ValueError("the problems to score must be of the table's kind (rows2 given or not)")
        if max(self.K) > max_classes(self.d):
            raise ValueError("%s predict: %d classes, at most %d classes at embedding width d = %d"
                             % (self.task, max(self.K), max_classes(self.d), self.d))
        rows, rows2, y = _cat_rows(problems, self.pair, self.task, E.device)
        G = len(self.C_list)
        pred = torch.empty(max(1, sum(n)), G, dtype=torch.int32, device=E.device)
        correct = torch.empty(self.P, G, dtype=torch.int64, device=E.device)
        row_start = torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64, device=E.device)
        chunk_h = np.concatenate([[0], np.cumsum([lib.ctgcn_nc_chunks(k) for k in n])]).astype(np.int64)
        chunk_start = torch.from_numpy(chunk_h).to(E.device)
        W = _hi_lo(theta)
        fn, idx = self._entry("predict", rows, rows2)
        check(fn(self.P, self.d, max(self.K), G, ptr(row_start), ptr(chunk_start), int(chunk_h[-1]), *idx, ptr(y), ptr(self.n_classes),
                 ptr(self.model_start), ptr(self.model_flag), E.shape[0], ptr(E), E.stride(0), ptr(W), self.M, ptr(pred), ptr(correct),
                 _stream()), fn.__name__)
        return pred[:sum(n)], correct


def fit(table, tol=1e-6, max_iter=100):
    """Fit every model of the table.  Returns theta (double[M, d+1], w then b; zero for constant models) and one FitReport per model.
    A model that does not reach tol is reported (converged=False) and warned about."""
    dev, M, D1 = table.E.device, table.M, table.d + 1
    n_m = torch.tensor([max(k, 1) for k in table.m_n], dtype=torch.float64, device=dev)
    inv_cn = torch.tensor([1.0 / (C * max(k, 1)) for C, k in zip(table.m_C, table.m_n)], dtype=torch.float64, device=dev)
    n_sub = torch.tensor([max(int(table.n_sub[p]), 1) for p in table.m_problem], dtype=torch.float64, device=dev)
    fitted = torch.from_numpy(table.flags_h == FLAG_FIT).to(dev)
    eye = torch.eye(D1, dtype=torch.float64, device=dev)
    idx = torch.arange(D1 - 1, device=dev)
    chunks = table.hess_chunks()

    def flags_for(mask):            # kernels skip every model outside mask
        return torch.where(mask, table.model_flag, torch.full_like(table.model_flag, FLAG_ZERO)).contiguous()

    def objective(th, live):
        loss, g = table.loss_grad(th, None if live is None else flags_for(live))
        w = th[:, :-1]
        f = loss / n_m + 0.5 * inv_cn * (w * w).sum(1)
        g = g / n_m[:, None]
        g[:, :-1] += inv_cn[:, None] * w
        g[~fitted] = 0
        return f, g

    def hessians(th, active):       # in chunks of problems within HESS_BYTES; those without an active model are left out
        hflags = flags_for(active)
        for p0, p1 in chunks:
            m0, m1 = int(table.model_start_h[p0]), int(table.model_start_h[p1])
            if m1 == m0 or not bool(active[m0:m1].any()):
                continue
            H = table.hessian(th, p0, p1, hflags) / n_sub[m0:m1, None, None]
            H[:, idx, idx] += inv_cn[m0:m1, None]
            H[~active[m0:m1]] = eye                      # inactive systems: identity (their step is discarded)
            yield m0, m1, H

    theta, it, gmax = _newton.minimize(torch.zeros(M, D1, dtype=torch.float64, device=dev), objective, hessians, tol, max_iter, fitted)
    reports = [FitReport(table.m_problem[m], table.m_cls[m], table.m_C[m], table.flags_h[m] != FLAG_FIT or gmax[m] <= tol, it[m],
                         gmax[m], bool(table.flags_h[m] != FLAG_FIT)) for m in range(M)]
    for r in reports:
        if not r.converged:
            warnings.warn("one-vs-rest logistic regression (problem %d, class %d, C=%g) did not converge: max|grad| %.3g > tol %.3g "
                          "after %d Newton iterations" % (r.problem, r.cls, r.C, r.grad_norm, tol, r.iterations), RuntimeWarning)
    return theta, reports
