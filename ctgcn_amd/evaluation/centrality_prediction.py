"""Centrality-prediction evaluation with the reference's interface and file contract (evaluation/centrality_prediction.py), on the GPU.

DataGenerator / CentralityPredictor / centrality_prediction(args) keep the reference's constructor and method signatures, config
keys (`cent_pred`) and file formats: <date>_centrality.csv and <method>_mse_record.csv written by either implementation are read by
the other.  What runs differently:
  - the ground truth (closeness, exact betweenness, eigenvector, k-core) comes from the GPU kernels of ctgcn_cent.hip and ops.kcore
    on the project's symmetric int32 CSR instead of networkx: one Brandes BFS per source serves betweenness and closeness;
  - the 5-fold ridge regressions of every (alpha, target) come from two passes over the embedding (per-fold augmented Grams, then
    held-out squared errors) and fp64 Cholesky solves of the (d+1)-sized systems, instead of sklearn's cross_val_predict(Ridge);
  - a node named in a snapshot file but missing from the node file raises ValueError (the reference's networkx graph silently
    grows, which also changes n in every formula).
`worker` is accepted and ignored.  There is no CPU fallback: without a GPU every entry point raises.
"""
import ctypes
import os
import time
from functools import partial

import numpy as np
import pandas as pd
import torch

from .. import _lib, ops
from .._lib import check, ptr
from ..utils import symmetric_csr_from_rows
from . import _common
from ._common import method_snapshots, read_embedding, read_nodes as _read_nodes, snapshot_rows, stream as _stream

CENTRALITY_LIST = ('closeness', 'betweenness', 'eigenvector', 'kcore')
ALL_KINDS = ('degree',) + CENTRALITY_LIST


class PowerIterationFailedConvergence(RuntimeError):
    """networkx.PowerIterationFailedConvergence: the eigenvector iteration did not pass its stop test within max_iter steps."""

    def __init__(self, max_iter):
        super().__init__("power iteration failed to converge within %d iterations" % max_iter)
        self.max_iter = max_iter


_device = partial(_common.device, task="centrality-prediction")
_require_cuda = partial(_common.require_cuda, task="centrality-prediction")


def _csr(row_ptr, col):
    """int32 contiguous (row_ptr, col); an edgeless graph gets a one-entry col so that no kernel argument is a null pointer."""
    row_ptr, col = row_ptr.to(torch.int32).contiguous(), col.to(torch.int32).contiguous()
    if col.numel() == 0:
        col = torch.zeros(1, dtype=torch.int32, device=col.device)
    return row_ptr, col


def graph_csr(file_path, full_node_list, sep='\t'):
    """(row_ptr, col) int32 numpy arrays of the reference's graph of a snapshot file: every pair in the file is an edge whatever its
    weight (zero included), duplicates collapse, self loops are dropped, and every node of full_node_list is a vertex.  A node in the
    file but not in full_node_list raises ValueError."""
    src, dst, _ = snapshot_rows(file_path, full_node_list, sep, " (the reference would add it as a vertex)")
    # weight 1 everywhere: the structure is what counts, and an explicit zero weight must still be an edge
    m = symmetric_csr_from_rows(src, dst, np.ones(len(src)), len(full_node_list))
    return m.indptr.astype(np.int32), m.indices.astype(np.int32)


def brandes(row_ptr, col, s0=0, s1=None):
    """Unscaled Brandes sums over the sources [s0, s1) (double[n]) and the closeness counts r, D (int64[s1 - s0])."""
    _require_cuda(row_ptr, "row_ptr")
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    s1 = n if s1 is None else s1
    lib = _lib.load()
    row_ptr, col = _csr(row_ptr, col)
    bc = torch.empty(n, dtype=torch.float64, device=dev)
    r = torch.empty(max(s1 - s0, 1), dtype=torch.int64, device=dev)
    D = torch.empty_like(r)
    with torch.cuda.device(dev):
        nbytes = lib.ctgcn_cent_brandes_workspace_bytes(n, s0, s1)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_cent_brandes(n, ptr(row_ptr), ptr(col), s0, s1, ptr(bc), ptr(r), ptr(D), ptr(ws), nbytes, _stream(dev)),
              "ctgcn_cent_brandes")
    return bc, r[:s1 - s0], D[:s1 - s0]


def eigenvector(row_ptr, col, max_iter=100, tol=1e-6):
    """networkx.eigenvector_centrality (unweighted): returns (x double[n] on the device, stop step).  Raises
    PowerIterationFailedConvergence when no step within max_iter passes the stop test."""
    _require_cuda(row_ptr, "row_ptr")
    dev = row_ptr.device
    n = row_ptr.numel() - 1
    if n == 0:
        raise ValueError("cannot compute centrality for the null graph")
    lib = _lib.load()
    row_ptr, col = _csr(row_ptr, col)
    x = torch.empty(n, dtype=torch.float64, device=dev)
    stop = ctypes.c_int32(0)
    with torch.cuda.device(dev):
        nbytes = lib.ctgcn_cent_eigenvector_workspace_bytes(n)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        check(lib.ctgcn_cent_eigenvector(n, ptr(row_ptr), ptr(col), int(max_iter), float(tol), ptr(x), ctypes.byref(stop), ptr(ws),
                                         nbytes, _stream(dev)), "ctgcn_cent_eigenvector")
    if stop.value == 0:
        raise PowerIterationFailedConvergence(max_iter)
    return x, int(stop.value)


def closeness_from_counts(r, D, n):
    """networkx.closeness_centrality (wf_improved) from the BFS counts, with the reference's float operations in their order."""
    r = np.asarray(r, np.int64)
    D = np.asarray(D, np.int64)
    out = np.zeros(len(r), dtype=np.float64)
    ok = (D > 0) & (n > 1)
    rm1 = r[ok] - 1.0
    out[ok] = (rm1 / D[ok].astype(np.float64)) * (rm1 / (n - 1))
    return out


def betweenness_scale(n):
    """networkx's normalisation of undirected betweenness without endpoints; None below n = 3 (left unscaled)."""
    return None if n <= 2 else 1 / ((n - 1) * (n - 2))


def centralities(row_ptr, col, n=None, kinds=CENTRALITY_LIST, max_iter=100, tol=1e-6):
    """The reference's get_centrality of every kind in `kinds` on the GPU CSR (row_ptr, col): a symmetric int32 structure without self
    loops.  Returns {kind: tensor[n] on the device}: float64, except 'kcore' (int64).  One Brandes pass serves closeness and
    betweenness; eigenvector raises PowerIterationFailedConvergence as networkx does."""
    _require_cuda(row_ptr, "row_ptr")
    _require_cuda(col, "col")
    dev = row_ptr.device
    nn = row_ptr.numel() - 1
    if n is not None and n != nn:
        raise ValueError("n = %d but row_ptr describes %d vertices" % (n, nn))
    for k in kinds:
        if k not in ALL_KINDS:
            raise ValueError("unknown centrality %r" % (k,))
    out = {}
    if 'degree' in kinds:
        deg = (row_ptr[1:] - row_ptr[:-1]).to(torch.float64)
        out['degree'] = deg * (1.0 / (nn - 1.0)) if nn > 1 else torch.ones(nn, dtype=torch.float64, device=dev)
    if 'closeness' in kinds or 'betweenness' in kinds:
        bc, r, D = brandes(row_ptr, col)
        if 'closeness' in kinds:
            out['closeness'] = torch.from_numpy(closeness_from_counts(r.cpu().numpy(), D.cpu().numpy(), nn)).to(dev)
        if 'betweenness' in kinds:
            scale = betweenness_scale(nn)
            out['betweenness'] = bc * scale if scale is not None else bc
    if 'eigenvector' in kinds:
        out['eigenvector'] = eigenvector(row_ptr, col, max_iter, tol)[0]
    if 'kcore' in kinds:
        out['kcore'] = ops.kcore(*_csr(row_ptr, col))[0].to(torch.int64)
    return {k: out[k] for k in kinds}


def fold_bounds(n, split_fold):
    """sklearn's unshuffled KFold: contiguous folds, the first n % split_fold one row longer.  Returns [split_fold + 1] offsets."""
    sizes = np.full(split_fold, n // split_fold, dtype=np.int64)
    sizes[:n % split_fold] += 1
    return np.concatenate([[0], np.cumsum(sizes)])


def ridge_weights(gram_fold, d, alpha_list):
    """Ridge(alpha, fit_intercept=True) of every held-out fold and alpha from the per-fold augmented Grams (double[F, d+1, d+1+T]):
    the training Gram is the total minus the fold's own; X and Y are centred by the training means and (XcᵀXc + αI) w = Xcᵀ yc
    is solved by Cholesky.  Returns W double[F, |alpha| * T, d+1]: model a * T + t is (w, intercept) of alpha a and target t."""
    F = gram_fold.shape[0]
    total = gram_fold[0].clone()
    for f in range(1, F):
        total += gram_fold[f]
    tr = total.unsqueeze(0) - gram_fold                            # [F, d+1, d+1+T]
    m = tr[:, d, d]                                                # training rows
    sx, sy = tr[:, :d, d], tr[:, d, d + 1:]                        # column sums of X, Y
    xm, ym = sx / m[:, None], sy / m[:, None]
    xtx = tr[:, :d, :d] - sx[:, :, None] * xm[:, None, :]
    xty = tr[:, :d, d + 1:] - sx[:, :, None] * ym[:, None, :]
    eye = torch.eye(d, dtype=torch.float64, device=gram_fold.device)
    out = []
    for alpha in alpha_list:
        L = torch.linalg.cholesky(xtx + float(alpha) * eye)
        w = torch.cholesky_solve(xty, L)                           # [F, d, T]
        b = ym - (xm[:, :, None] * w).sum(1)                       # [F, T]
        out.append(torch.cat([w.transpose(1, 2), b[:, :, None]], 2))   # [F, T, d+1]
    return torch.cat(out, 1).contiguous()


def ridge_cv_errors(embeddings, targets, alpha_list, split_fold=5):
    """mean_squared_error(y, cross_val_predict(Ridge(alpha), X, y, cv=split_fold)) / mean(y) of every alpha and target column, on the
    GPU.  embeddings: CUDA [n, d] float32 or float64 (d <= 512); targets: CUDA [n, T] (T <= 8).  Returns double [|alpha|, T] on the
    host (numpy).  A target with mean 0 gives inf or nan, as numpy does."""
    _require_cuda(embeddings, "embeddings")
    _require_cuda(targets, "targets")
    dev = embeddings.device
    X = embeddings if embeddings.dtype in (torch.float32, torch.float64) else embeddings.to(torch.float64)
    if X.stride(1) != 1:
        X = X.contiguous()
    Y = targets.to(torch.float64).reshape(targets.shape[0], -1).contiguous()
    n, d = X.shape
    T = Y.shape[1]
    if Y.shape[0] != n:
        raise ValueError("embeddings and targets have different row counts")
    F, A = int(split_fold), len(alpha_list)
    P = A * T
    lib = _lib.load()
    suffix = "f32" if X.dtype == torch.float32 else "f64"
    with torch.cuda.device(dev):
        st = _stream(dev)
        gram = torch.empty(F, d + 1, d + 1 + T, dtype=torch.float64, device=dev)
        nb = lib.ctgcn_ridge_gram_workspace_bytes(d, T, F)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        check(getattr(lib, "ctgcn_ridge_gram_" + suffix)(n, d, T, F, ptr(X), X.stride(0), ptr(Y), ptr(gram), ptr(ws), nb, st),
              "ctgcn_ridge_gram_" + suffix)
        W = ridge_weights(gram, d, alpha_list)
        tgt = torch.arange(P, dtype=torch.int32, device=dev) % T
        sse = torch.empty(F, P, dtype=torch.float64, device=dev)
        nb = lib.ctgcn_ridge_sse_workspace_bytes(P, F)
        ws = torch.empty(max(nb, 1), dtype=torch.uint8, device=dev)
        check(getattr(lib, "ctgcn_ridge_sse_" + suffix)(n, d, T, F, P, ptr(X), X.stride(0), ptr(Y), ptr(W), ptr(tgt), ptr(sse), ptr(ws),
                                                       nb, st), "ctgcn_ridge_sse_" + suffix)
    total = sse[0].clone()
    for f in range(1, F):
        total += sse[f]
    mse = (total / n).reshape(A, T).cpu().numpy()
    mean = Y.mean(0).cpu().numpy()
    with np.errstate(divide='ignore', invalid='ignore'):
        return mse / mean[None, :]


def min_over_alphas(errors):
    """The reference's running min(min_error, error) from inf, per target: a nan never replaces the running value."""
    out = []
    for t in range(errors.shape[1]):
        best = float("inf")
        for e in errors[:, t]:
            best = min(best, float(e))
        out.append(best)
    return out


def evaluate(embedding, row_ptr, col, alpha_list, split_fold=5, date=None, max_iter=100, tol=1e-6):
    """One snapshot's get_prediction_error: [date] + the minimum over alphas of each centrality's error, with the centralities of
    the GPU CSR (row_ptr, col).  embedding: CUDA [n, d] float32 or float64, rows in node-file order."""
    c = centralities(row_ptr, col, kinds=CENTRALITY_LIST, max_iter=max_iter, tol=tol)
    Y = torch.stack([c[k].to(torch.float64) for k in CENTRALITY_LIST], 1)
    return [date] + min_over_alphas(ridge_cv_errors(embedding, Y, alpha_list, split_fold))


class DataGenerator(object):
    """Reference DataGenerator: writes <date>_centrality.csv (node, closeness, betweenness, eigenvector, kcore; sep = file_sep)."""

    def __init__(self, base_path, input_folder, output_folder, node_file, file_sep='\t', device=None):
        self.base_path = base_path
        self.input_base_path = os.path.abspath(os.path.join(base_path, input_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = _read_nodes(os.path.abspath(os.path.join(base_path, node_file)))
        self.node_num = len(self.full_node_list)
        self.device = device
        os.makedirs(self.input_base_path, exist_ok=True)
        os.makedirs(self.output_base_path, exist_ok=True)

    @staticmethod
    def get_centrality(network, type='degree', undirected=True):
        """Unlike the reference, `network` is the project's GPU CSR: a (row_ptr, col) pair of CUDA int32 tensors (symmetric, no self
        loops), not a networkx graph.  Returns a float64 (int64 for 'kcore') CUDA tensor indexed by node position."""
        assert type in ALL_KINDS
        row_ptr, col = network
        return centralities(row_ptr, col, kinds=(type,))[type]

    def graph(self, file, sep='\t'):
        """(row_ptr, col) on the device of a snapshot file of input_folder."""
        rp, col = graph_csr(os.path.join(self.input_base_path, file), self.full_node_list, sep)
        dev = _device(self.device)
        return torch.from_numpy(rp).to(dev), torch.from_numpy(col).to(dev)

    def generate_node_samples(self, file, sep='\t'):
        date = file.split('.')[0]
        output_path = os.path.join(self.output_base_path, date + '_centrality.csv')
        if os.path.exists(output_path):
            print('\t', date + '_centrality.csv exist')
            return
        t1 = time.time()
        row_ptr, col = self.graph(file, sep)
        c = centralities(row_ptr, col, kinds=CENTRALITY_LIST)
        df = pd.DataFrame({'node': np.arange(self.node_num, dtype=np.int64)})
        for k in CENTRALITY_LIST:
            df[k] = c[k].cpu().numpy()
        df.to_csv(output_path, sep=self.file_sep, index=False)
        print('finish generating', date + '_centrality.csv', 'cost time: ', time.time() - t1, ' seconds!')

    def generate_all_node_samples(self, sep='\t', worker=-1):
        for file in sorted(os.listdir(self.input_base_path)):
            self.generate_node_samples(file, sep=sep)


class CentralityPredictor(object):
    """Reference CentralityPredictor: <method>_mse_record.csv (date, closeness, betweenness, eigenvector, kcore; sep ',')."""

    def __init__(self, base_path, origin_folder, embedding_folder, centrality_folder, output_folder, node_file, file_sep='\t',
                 alpha_list=None, split_fold=5, device=None):
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.centrality_base_path = os.path.abspath(os.path.join(base_path, centrality_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = _read_nodes(os.path.abspath(os.path.join(base_path, node_file)))
        self.alpha_list = alpha_list
        self.split_fold = split_fold
        self.device = device
        for p in (self.embedding_base_path, self.origin_base_path, self.output_base_path):
            os.makedirs(p, exist_ok=True)

    def get_prediction_error(self, centrality_data, embeddings, date):
        """centrality_data: [n, 4] (numpy or tensor), embeddings: [n, d] (numpy or tensor); both moved to the GPU."""
        dev = _device(self.device)
        Y = torch.as_tensor(np.asarray(centrality_data, dtype=np.float64) if not isinstance(centrality_data, torch.Tensor)
                            else centrality_data).to(dev, torch.float64)
        X = embeddings if isinstance(embeddings, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(embeddings))
        if X.dtype not in (torch.float32, torch.float64):
            X = X.to(torch.float64)
        errors = ridge_cv_errors(X.to(dev), Y, self.alpha_list, self.split_fold)
        return [date] + min_over_alphas(errors)

    def centrality_prediction_all_time(self, method):
        all_mse_list = []
        for date, _, cur_embedding_path in method_snapshots(self.origin_base_path, self.embedding_base_path, method):
            df_centrality = pd.read_csv(os.path.join(self.centrality_base_path, date + '_centrality.csv'), sep=self.file_sep)
            centrality_data = df_centrality.iloc[:, 1:].values
            embedding = read_embedding(cur_embedding_path, self.file_sep, self.full_node_list, np.float64)
            all_mse_list.append(self.get_prediction_error(centrality_data, embedding, date))
        df_output = pd.DataFrame(all_mse_list, columns=['date'] + list(CENTRALITY_LIST))
        print(df_output)
        df_output.to_csv(os.path.join(self.output_base_path, method + '_mse_record.csv'), sep=',', index=False)

    def centrality_prediction_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = os.listdir(self.embedding_base_path)
        for method in method_list:
            self.centrality_prediction_all_time(method)


def centrality_prediction(args):
    """The reference's cent_pred driver: the same config keys ('worker' ignored)."""
    base_path = args['base_path']
    data_generator = DataGenerator(base_path=base_path, input_folder=args['origin_folder'], output_folder=args['centrality_data_folder'],
                                   node_file=args['node_file'], file_sep=args['file_sep'])
    if args['generate']:
        data_generator.generate_all_node_samples(sep=args['file_sep'], worker=args.get('worker', -1))
    predictor = CentralityPredictor(base_path=base_path, origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                    centrality_folder=args['centrality_data_folder'], output_folder=args['centrality_res_folder'],
                                    node_file=args['node_file'], file_sep=args['file_sep'], alpha_list=args['alpha_list'],
                                    split_fold=args['split_fold'])
    t1 = time.time()
    predictor.centrality_prediction_all_method(method_list=args['method_list'], worker=args.get('worker', -1))
    print('centrality prediction cost time: ', time.time() - t1, ' seconds!')
