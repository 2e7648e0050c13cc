"""TIMERS: error-bounded SVD restart on dynamic networks (https://arxiv.org/abs/1711.09541), with the function names and arguments of
the reference's baseline/timers.py.  The only baseline that is not a neural network: an incremental truncated SVD of the cumulative
adjacency matrix (TRIP's first-order eigenpair update) that is recomputed from scratch when the loss ‖S − U Vᵀ‖²_F passes (1 + Theta)
times a matrix-perturbation lower bound.  Everything is fp64.

Where the work runs:
  * The static decomposition is ops.sym_topk of the matrix itself (block subspace iteration with Rayleigh–Ritz and CholeskyQR2 on
    ctgcn_spmm_csr_f64 / ctgcn_tsgemm_tn_f64 / ctgcn_tsgemm_nn_f64; it stops when every pair has ‖A x − w x‖₂ <= tol·|w₁|), with
    U = X, S = |w|, V = X·sign(w): the SVD of a symmetric matrix.  For an exact ±λ pair scipy's singular vectors are not unique (any
    rotation inside the two-dimensional singular space is an SVD); the eigenvector choice here is the one TRIP assumes, since TRIP
    reads U as eigenvectors and recovers the eigenvalue signs from U against V.  Columns are in svds' order, ascending singular value.
  * Obj is one ctgcn_timers_obj_f64 pass over the stored entries plus two Gram products: Σs² − 2 Σ s⟨U_r, V_c⟩ + ⟨UᵀU, VᵀV⟩.  The
    reference's K-chunk loop partitions the entries to bound memory; one pass is the same sum.
  * RefineBound never forms a sparse product.  trace_change = ‖S_ori + S_add‖²_F − ‖S_ori‖²_F (equal to the reference's
    diag(T·T).sum() − diag(S·S).sum() for symmetric matrices), and the eigenvalues are sym_topk's of the operator
    x ↦ S_ori (S_add x) + S_add ((S_ori + S_add) x): three SpMMs, the last one over the side-by-side matrix [S_ori | S_add].
  * TRIP is one SpMM and one Gram for Xᵀ(Δ X), the K pseudo-inverses of K x K matrices on the host with numpy.linalg.pinv (the
    reference's cut-off), and one ctgcn_tsgemm_nn_f64 for X·(I + [alpha]) with its column norms.

Deviations from the reference, both on purpose:
  * timers() writes through export.write_embedding like every other method here, so the files hold float32 values; the reference
    prints float64.
  * A non-symmetric input, n < 2 K + 2, and a RefineBound whose operator has no non-negative eigenvalue among the 2 K computed (where
    the reference dies on an IndexError) raise ValueError.
Random_Com, the reference's synthetic-graph generator that timers() never calls, is not here."""
import os

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch

from .. import _lib, ops
from ..export import write_embedding
from ..utils import get_sp_adj_mat


def _device(device=None):
    if device is None:
        if not torch.cuda.is_available():
            raise _lib.CtgcnHipError("ctgcn_amd runs on MI355X only: TIMERS needs a GPU; there is no CPU fallback.")
        return torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CtgcnHipError("ctgcn_amd runs on MI355X only: TIMERS on %s; there is no CPU fallback." % device)
    return device


def _canonical(mat):
    m = sp.csr_matrix(mat, dtype=np.float64)
    m.sum_duplicates()
    m.eliminate_zeros()
    m.sort_indices()
    return m


class DeviceCsr(object):
    """A scipy matrix as canonical CSR (no duplicates, no explicit zeros, sorted) on the host and on the device."""

    def __init__(self, mat, device):
        self.host = mat.host if isinstance(mat, DeviceCsr) else _canonical(mat)
        self.shape = self.host.shape
        self.device = torch.device(device)
        self.row_ptr = torch.from_numpy(self.host.indptr.astype(np.int32)).to(self.device)
        self.col = torch.from_numpy(self.host.indices.astype(np.int32)).to(self.device)
        self.val = torch.from_numpy(self.host.data.astype(np.float64)).to(self.device)

    def matmul(self, x, out=None, accumulate=False):
        return ops.spmm_csr_f64(self.row_ptr, self.col, self.val, x, out=out, accumulate=accumulate)


def _as_csr(mat, like):
    return mat if isinstance(mat, DeviceCsr) else DeviceCsr(mat, like.device)


def _host(mat):
    return mat.host if isinstance(mat, DeviceCsr) else _canonical(mat)


def _factor(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError("%s must be a device tensor" % what)
    ops._need_cuda(t)
    return t.to(torch.float64)


def get_sp_delta_adj_mat(A_pre, file_path, node2idx_dict, sep='\t'):
    """The change from A_pre to the snapshot in file_path as CSR, explicit zeros eliminated: the matrix the reference builds with its
    two dict loops.  node2idx_dict: the reference's name -> index dict (indices 0..n-1 in insertion order) or the node list itself."""
    node_list = list(node2idx_dict.keys()) if isinstance(node2idx_dict, dict) else node2idx_dict
    A_cur = get_sp_adj_mat(file_path, node_list, sep=sep).tocsr()
    delta = (A_cur - sp.csr_matrix(A_pre)).tocsr()
    delta.eliminate_zeros()
    return delta


def Obj(Sim, U, V):
    """‖Sim − U Vᵀ‖²_F for a sparse Sim (scipy or DeviceCsr) and device factors U, V [n, K]"""
    U, V = _factor(U, "U"), _factor(V, "V")
    S = _as_csr(Sim, U)
    sums = ops.timers_obj(S.row_ptr, S.col, S.val, U, V).cpu().numpy()
    third = (ops.tsgemm_tn(U, U) * ops.tsgemm_tn(V, V)).sum().item()
    return float(sums[0] - 2.0 * sums[1] + third)


def Obj_SimChange(S_ori, S_add, U, V, loss_ori):
    """‖S_ori + S_add − U Vᵀ‖²_F from loss_ori = ‖S_ori − U Vᵀ‖²_F: one pass over S_add's entries with S_ori's values on that pattern"""
    U, V = _factor(U, "U"), _factor(V, "V")
    add = _as_csr(S_add, U)
    rows = np.repeat(np.arange(add.shape[0]), np.diff(add.host.indptr))
    old = np.asarray(_host(S_ori)[rows, add.host.indices], dtype=np.float64).ravel() if add.host.nnz else np.zeros(0)
    sums = ops.timers_obj(add.row_ptr, add.col, add.val, U, V, s_old=torch.from_numpy(old).to(U.device)).cpu().numpy()
    return float(loss_ori + sums[0])


def bound_operator(S_ori, S_add, device):
    """x ↦ S_ori (S_add x) + S_add ((S_ori + S_add) x) on [n, b] device blocks, and trace_change = ‖S_ori + S_add‖²_F − ‖S_ori‖²_F"""
    ori, add = _host(S_ori), _host(S_add)
    total = _canonical(ori + add)
    n = ori.shape[0]
    d_add, d_total, d_side = DeviceCsr(add, device), DeviceCsr(total, device), DeviceCsr(sp.hstack((ori, add), format="csr"), device)
    trace_change = float((total.data * total.data).sum() - (ori.data * ori.data).sum())

    def apply(x):
        stack = torch.empty(2 * n, x.shape[1], dtype=torch.float64, device=x.device)
        d_add.matmul(x, out=stack[:n])
        d_total.matmul(x, out=stack[n:])
        return d_side.matmul(stack)
    return apply, trace_change


def RefineBound(S_ori, S_add, Loss_ori, K, tol=1e-12, max_iter=5000, seed=0, device=None):
    """A lower bound of the loss for S_ori + S_add from the one for S_ori by the matrix-perturbation inequality:
    Loss_ori + trace_change − (the K largest non-negative of the 2 K eigenvalues of largest magnitude of Δ(S Sᵀ))."""
    device = _device(device)
    n = _host(S_ori).shape[0]
    apply, trace_change = bound_operator(S_ori, S_add, device)
    w, _ = ops.sym_topk(apply, n, min(2 * int(K), n), tol=tol, max_iter=max_iter, seed=seed, device=device, _deficient_ok=True)
    eigen_sum, _ = bound_eigen_sum(w.cpu().numpy(), K)
    return float(Loss_ori + trace_change - eigen_sum)


def bound_eigen_sum(w, K):
    """The reference's selection: keep the eigenvalues >= 0, descending; the sum of the top K, a shortfall padded with the smallest kept.
    Returns (sum, kept)."""
    kept = np.sort(w[w >= 0])[::-1]
    if len(kept) == 0:
        raise ValueError("RefineBound: none of the %d eigenvalues of largest magnitude is non-negative (the reference fails here with "
                         "an IndexError)" % len(w))
    if len(kept) >= K:
        return float(kept[:K].sum()), kept
    return float(kept.sum() + kept[-1] * (K - len(kept))), kept


def trip_alpha(Old_L, temp_sum):
    """Host part of TRIP: ΔL = diag(temp_sum) and the K coefficient vectors alpha_i = pinv(D_i − temp_sum)·temp_sum[:, i],
    D_i = diag(L_i + ΔL_i − L), as the [K, K] matrix of columns"""
    K = len(Old_L)
    Delta_L = np.diag(temp_sum).copy()
    alpha = np.zeros((K, K))
    for i in range(K):
        temp_D = np.diag(np.ones(K) * (Old_L[i] + Delta_L[i]) - Old_L)
        alpha[:, i] = np.linalg.pinv(temp_D - temp_sum).dot(temp_sum[:, i])
    return Delta_L, alpha


def TRIP(Old_U, Old_S, Old_V, Delta):
    """TRIP (Chen and Tong, SDM 2015) step for step as in the reference: (New_U, New_S, New_V), New_S a [K, K] diagonal matrix.  Old_S may
    be that matrix or its diagonal; Delta is scipy or DeviceCsr."""
    Old_U, Old_V = _factor(Old_U, "Old_U"), _factor(Old_V, "Old_V")
    dev = Old_U.device
    K = Old_U.shape[1]
    s = torch.as_tensor(Old_S, dtype=torch.float64).to(dev)
    s = torch.diagonal(s) if s.dim() == 2 else s
    cols = torch.arange(K, device=dev)
    X = Old_U.clone()
    lead = X[X.abs().argmax(dim=0), cols]                       # unify the sign by the entry of largest magnitude
    X = X * torch.where(lead < 0, -torch.ones_like(lead), torch.ones_like(lead))
    temp_v, temp_i = Old_U.max(dim=0)
    Old_L = (s * torch.sign(temp_v * Old_V[temp_i, cols])).cpu().numpy()
    temp_sum = ops.tsgemm_tn(X, _as_csr(Delta, X).matmul(X)).cpu().numpy()
    Delta_L, alpha = trip_alpha(Old_L, temp_sum)
    New_U, sq = ops.tsgemm_nn(X, torch.from_numpy(np.eye(K) + alpha).to(dev), colsq=True)      # Old_X + Old_X·[alpha]
    New_U = New_U / torch.sqrt(sq)
    New_L = torch.from_numpy(Old_L + Delta_L).to(dev)
    return New_U, torch.diag(New_L.abs()), New_U * torch.sign(New_L)


class TIMERS(object):
    """The state of one TIMERS run on the device: the CSR matrices Sim (at the last restart), S_cum (now) and S_perturb (their
    difference), the factors U [n, K], S [K], V [n, K], and per step Loss_store, Loss_bound and the restart steps Run_t.

    fit_first(A) decomposes the first snapshot; step(S_add) advances by one change matrix and returns True when it restarted (the rule:
    Loss_store[i] >= (1 + Theta)·Loss_bound[i], then everything is rebuilt from S_cum); embedding() is [U√S, V√S], [n, 2 K].
    Update=False keeps the factors fixed between restarts and tracks the loss with Obj_SimChange, as in the reference."""

    def __init__(self, K, Theta=0.17, Update=True, tol=1e-12, max_iter=5000, seed=0, device=None):
        self.K, self.Theta, self.Update = int(K), float(Theta), bool(Update)
        self.tol, self.max_iter, self.seed = tol, max_iter, seed
        self.device = device                 # resolved by fit_first, after the checks that need no GPU
        self.Loss_store, self.Loss_bound, self.Run_t, self.tested = [], [], [], []
        self.iterations = []          # sym_topk iterations: one entry per decomposition and per bound

    def _decompose(self, csr):
        w, X = ops.sym_topk(csr.matmul, csr.shape[0], self.K, tol=self.tol, max_iter=self.max_iter, seed=self.seed, device=self.device)
        self.iterations.append(("decomposition", ops.sym_topk.last[0]))
        w, X = torch.flip(w, dims=(0,)), torch.flip(X, dims=(1,)).contiguous()        # svds' order: ascending singular value
        self.U, self.S, self.V = X, w.abs(), X * torch.sign(w)

    def _current(self):
        root = torch.sqrt(self.S)
        return self.U * root, self.V * root

    def fit_first(self, A):
        A = _canonical(A)
        n = A.shape[0]
        if A.shape[0] != A.shape[1] or (A != A.T).nnz:
            raise ValueError("TIMERS decomposes a symmetric matrix (get_sp_adj_mat makes no other)")
        if n < 2 * self.K + 2:
            raise ValueError("TIMERS needs n >= 2 K + 2, got n=%d K=%d" % (n, self.K))
        self.device = _device(self.device)
        self.Sim = self.S_cum = DeviceCsr(A, self.device)
        self.S_perturb = DeviceCsr(sp.csr_matrix((n, n)), self.device)
        self._decompose(self.Sim)
        self.U_cur, self.V_cur = self._current()
        self.loss_rerun = Obj(self.Sim, self.U_cur, self.V_cur)
        self.Loss_store, self.Loss_bound, self.Run_t, self.tested = [self.loss_rerun], [self.loss_rerun], [], []
        return self

    def step(self, S_add):
        S_add = _canonical(S_add)
        n = self.S_cum.shape[0]
        if S_add.shape != (n, n):
            raise ValueError("S_add must be [%d, %d]" % (n, n))
        i = len(self.Loss_store)
        add = DeviceCsr(S_add, self.device)
        self.S_perturb = DeviceCsr(self.S_perturb.host + S_add, self.device)
        new_cum = DeviceCsr(self.S_cum.host + S_add, self.device)
        if self.Update:
            self.U, S_mat, self.V = TRIP(self.U, self.S, self.V, add)
            self.S = torch.diagonal(S_mat).clone()
            self.U_cur, self.V_cur = self._current()
            loss = Obj(new_cum, self.U_cur, self.V_cur)
        else:
            loss = Obj_SimChange(self.S_cum, add, self.U_cur, self.V_cur, self.Loss_store[i - 1])
        bound = RefineBound(self.Sim, self.S_perturb, self.loss_rerun, self.K, tol=self.tol, max_iter=self.max_iter, seed=self.seed,
                            device=self.device)
        self.iterations.append(("bound", ops.sym_topk.last[0]))
        self.S_cum = new_cum
        restart = loss >= (1 + self.Theta) * bound
        self.tested.append((loss, bound))            # the pair the rule compared (a restart overwrites both entries below)
        if restart:
            self.Sim = self.S_cum
            self.S_perturb = DeviceCsr(sp.csr_matrix((n, n)), self.device)
            self.Run_t.append(i)
            self._decompose(self.Sim)
            self.U_cur, self.V_cur = self._current()
            self.loss_rerun = loss = bound = Obj(self.Sim, self.U_cur, self.V_cur)
        self.Loss_store.append(loss)
        self.Loss_bound.append(bound)
        return bool(restart)

    def embedding(self):
        return torch.cat((self.U_cur, self.V_cur), dim=1)


def timers(nodes_file, input_base_path, output_base_path, Theta=0.17, dim=128, sep='\t', Update=True):
    """One embedding file per snapshot of input_base_path (sorted), named like the input file: index = node names, header 0..2 dim − 1,
    values float32 (the reference prints float64).  dim is K, the rank of the decomposition."""
    if not os.path.exists(output_base_path):
        os.makedirs(output_base_path)
    full_node_list = pd.read_csv(nodes_file, names=['node'])['node'].tolist()
    f_list = sorted(os.listdir(input_base_path))
    model = TIMERS(dim, Theta=Theta, Update=Update)
    model.fit_first(get_sp_adj_mat(os.path.join(input_base_path, f_list[0]), full_node_list, sep=sep))
    write_embedding(os.path.join(output_base_path, f_list[0]), model.embedding(), full_node_list, sep=sep)
    for i in range(1, len(f_list)):
        S_add = get_sp_delta_adj_mat(model.S_cum.host, os.path.join(input_base_path, f_list[i]), full_node_list, sep=sep)
        model.step(S_add)
        write_embedding(os.path.join(output_base_path, f_list[i]), model.embedding(), full_node_list, sep=sep)
    return model


def timers_embedding(args):
    """The reference's entry: base_path, origin_folder, embed_folder, node_file, file_sep, embed_dim, theta; K = embed_dim // 2"""
    base_path = args['base_path']
    origin_base_path = os.path.abspath(os.path.join(base_path, args['origin_folder']))
    embedding_base_path = os.path.abspath(os.path.join(base_path, args['embed_folder']))
    node_file_path = os.path.abspath(os.path.join(base_path, args['node_file']))
    return timers(node_file_path, origin_base_path, embedding_base_path, Theta=args['theta'], dim=args['embed_dim'] // 2, sep=args['file_sep'],
                  Update=True)
