"""Similarity-prediction evaluation with the reference's interface and file contract (evaluation/similarity_prediction.py), on the GPU.

DataGenerator / SimilarityPredictor / similarity_prediction(args) keep the reference's constructor and method signatures, config
keys (`sim_pred`) and file formats.  The ground truth is the vertex similarity of Leicht, Holme and Newman: iter_num steps of
S <- (alpha / lambda_1)·A·S + I, then (S + Sᵀ)/2 - I, min-max scaling over all n² entries and a 1e-6 threshold, saved as
<date>_similarity.npz.  The series runs in ctgcn_sim.hip on the m x m block of the non-isolated vertices, bit-identical to the
reference's scipy product for the same lambda_1.  The predictor scores E Eᵀ against it by Spearman correlation.  What runs
differently:
  - lambda_1 comes from eigsh with a fixed start vector (ones), so it does not depend on call order;
  - the predictor reads the <date>_similarity.npz the generator writes (the reference reads a <date>_similarity.csv nobody writes),
    falling back to the dense .csv text; and similarity_prediction(args) runs the predictor (the reference's call is commented out);
  - an edgeless snapshot, a constant similarity (iter_num = 1), a node missing from the node file and an empty kept-row set raise
    ValueError;
  - files and methods are walked in sorted order; `worker` is accepted and ignored.
There is no CPU fallback: without a GPU every entry point raises.
"""
import os
import time
from functools import partial

import numpy as np
import pandas as pd
import scipy.sparse as sp
import torch

from .. import _lib
from .._lib import check, ptr
from ..utils import symmetric_csr_from_rows
from . import _common
from ._common import method_snapshots, read_embedding, read_nodes as _read_nodes, snapshot_rows, stream as _stream

EPS = 1e-6


_device = partial(_common.device, task="similarity-prediction")
_require_cuda = partial(_common.require_cuda, task="similarity-prediction")


def _check_alpha(alpha):
    if not 0 < alpha < 1:
        raise AssertionError("alpha must lie in (0, 1), got %r" % (alpha,))


def _require_free(dev, nbytes, what):
    """Raise ValueError, before anything is allocated, when nbytes cannot fit in the device's free memory (plus torch's cached blocks)."""
    free, _ = torch.cuda.mem_get_info(dev)
    free += torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)
    if nbytes > free:
        raise ValueError("%s needs %.3g GB of device memory but %.3g GB are free" % (what, nbytes / 1e9, free / 1e9))


def graph_csr(file_path, full_node_list, sep='\t'):
    """The reference's get_sp_adj_mat(...).tocsr() of a snapshot file: scipy CSR float64 [n, n], symmetric, sorted columns.  The last
    row naming a pair sets its weight, self loops are dropped and a zero weight stores no entry.  A node missing from full_node_list
    raises ValueError."""
    src, dst, w = snapshot_rows(file_path, full_node_list, sep)
    m = symmetric_csr_from_rows(src, dst, w, len(full_node_list))
    m.eliminate_zeros()
    return m


def host_lambda_1(A):
    """The largest-magnitude eigenvalue of the symmetric scipy matrix A (the reference's eigsh(A, k=1, which='LM')), from the fixed
    start vector ones(n) so that repeated calls agree.  0.0 for a matrix without entries."""
    from scipy.sparse.linalg import eigsh
    A = sp.csr_matrix(A)
    if A.nnz == 0:
        return 0.0
    return float(eigsh(A, k=1, which='LM', return_eigenvectors=False, v0=np.ones(A.shape[0]))[0])


class Similarity(object):
    """vertex_similarity's result.  n: vertices of the graph; keep: int64 [m] (device) the non-isolated vertices, ascending; block:
    float64 [m, m] (device) the finished similarity restricted to them (every other entry of the n x n matrix is 0); row_nnz: int64
    [m] (device) the non-zeros per block row; lambda_1 and c = alpha / lambda_1 the values used; min / max the scaling bounds."""

    def __init__(self, n, keep, block, row_nnz, lambda_1, c, smin, smax):
        self.n, self.keep, self.block, self.row_nnz = n, keep, block, row_nnz
        self.lambda_1, self.c, self.min, self.max = lambda_1, c, smin, smax

    def kept(self):
        """Block indices of the rows the predictor keeps (row sum >= 1e-6, i.e. any non-zero: every stored value is >= 1e-6)."""
        return torch.nonzero(self.row_nnz > 0).flatten()

    def coo(self):
        """(row int32, col int32, data float64) on the device: the non-zeros of the n x n matrix in row-major order, the arrays the
        reference's sp.coo_matrix(S) holds."""
        dev = self.block.device
        m = self.keep.numel()
        off = torch.cumsum(self.row_nnz, 0) - self.row_nnz
        total = int(self.row_nnz.sum().item())
        row = torch.empty(max(total, 1), dtype=torch.int32, device=dev)
        col = torch.empty_like(row)
        data = torch.empty(max(total, 1), dtype=torch.float64, device=dev)
        with torch.cuda.device(dev):
            check(_lib.load().ctgcn_sim_coo(m, ptr(self.block), ptr(off), ptr(self.keep), ptr(row), ptr(col), ptr(data), _stream(dev)),
                  "ctgcn_sim_coo")
        return row[:total], col[:total], data[:total]

    def to_scipy(self):
        """scipy.sparse.coo_matrix of the n x n result, as the reference builds it before save_npz."""
        row, col, data = (t.cpu().numpy() for t in self.coo())
        return sp.coo_matrix((data, (row, col)), shape=(self.n, self.n))


def vertex_similarity(row_ptr, col, val, n=None, alpha=0.5, iter_num=100, lambda_1=None, panel_cols=None):
    """The reference's generate_node_similarity on the GPU CSR (row_ptr int32 [n+1], col int32, val float64: symmetric, sorted
    columns, no self loops).  lambda_1: the eigenvalue to use (default: the host eigsh with v0 = ones); panel_cols: the series'
    panel width (default: the widest whose buffers stay in the Infinity Cache; the result does not depend on it).  Returns a
    Similarity.  An edgeless graph, or one whose n² result would not fit in device memory, raises ValueError before any launch."""
    _check_alpha(alpha)
    for t, what in ((row_ptr, "row_ptr"), (col, "col"), (val, "val")):
        _require_cuda(t, what)
    if int(iter_num) < 1:
        raise ValueError("iter_num must be >= 1, got %r" % (iter_num,))
    dev = row_ptr.device
    nn = row_ptr.numel() - 1
    if n is not None and n != nn:
        raise ValueError("n = %d but row_ptr describes %d vertices" % (n, nn))
    row_ptr = row_ptr.to(torch.int32).contiguous()
    col = col.to(torch.int32).contiguous()
    val = val.to(torch.float64).contiguous()
    nnz = col.numel()
    if nnz == 0:
        raise ValueError("the graph has no edges: lambda_1 = 0 and the similarity is undefined (the reference writes NaNs)")
    deg = row_ptr[1:] - row_ptr[:-1]
    live = deg > 0
    m = int(live.sum().item())
    lib = _lib.load()
    panel = int(panel_cols) if panel_cols else int(lib.ctgcn_sim_panel_cols(m, nnz))
    panel = max(1, min(panel, m))
    _require_free(dev, 8 * m * m + lib.ctgcn_sim_series_workspace_bytes(m, panel) + lib.ctgcn_sim_finish_workspace_bytes(m) + 16 * m,
                  "the %d x %d similarity block" % (m, m))
    if lambda_1 is None:
        A = sp.csr_matrix((val.cpu().numpy(), col.cpu().numpy(), row_ptr.cpu().numpy()), shape=(nn, nn))
        lambda_1 = host_lambda_1(A)
    lambda_1 = float(lambda_1)
    if lambda_1 == 0.0:
        raise ValueError("lambda_1 = 0: the similarity is undefined (the reference writes NaNs)")
    c = alpha / lambda_1
    keep = torch.nonzero(live).flatten()
    newid = torch.cumsum(live.to(torch.int32), 0, dtype=torch.int32) - 1
    col_b = newid[col.long()].contiguous()                       # monotone relabel: CSR order, and the bits, are kept
    rp_b = torch.cat([torch.zeros(1, dtype=torch.int32, device=dev), row_ptr[1:][live]]).contiguous()
    S = torch.empty(m, m, dtype=torch.float64, device=dev)
    stats = torch.empty(2, dtype=torch.float64, device=dev)
    row_nnz = torch.empty(m, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _stream(dev)
        nb = lib.ctgcn_sim_series_workspace_bytes(m, panel)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        check(lib.ctgcn_sim_series(m, ptr(rp_b), ptr(col_b), ptr(val), c, int(iter_num), panel, 0, m, ptr(S), ptr(ws), nb, st),
              "ctgcn_sim_series")
        del ws
        nb = lib.ctgcn_sim_finish_workspace_bytes(m)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        check(lib.ctgcn_sim_finish(m, int(nn > m), EPS, ptr(S), ptr(stats), ptr(row_nnz), ptr(ws), nb, st), "ctgcn_sim_finish")
    smin, smax = (float(v) for v in stats.cpu().numpy())
    if smax == smin:
        raise ValueError("the similarity is constant (max == min): the reference's scaling gives NaN everywhere")
    if nn > m:
        z0 = (0.0 - smin) / (smax - smin)
        if not z0 < EPS:
            raise ValueError("the similarity has negative entries, so the zero rows of isolated vertices scale to %r >= 1e-6 and the "
                             "n x n result is dense: not supported" % z0)
    return Similarity(nn, keep, S, row_nnz, lambda_1, c, smin, smax)


def _normalize(x):
    """In place: the reference's (x - min)/(max - min), then x / sum(x).  Returns (min, max, sum)."""
    dev = x.device
    lib = _lib.load()
    N = x.numel()
    stats = torch.empty(3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        nb = lib.ctgcn_sim_normalize_workspace_bytes(N)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        check(lib.ctgcn_sim_normalize(N, ptr(x), ptr(stats), ptr(ws), nb, _stream(dev)), "ctgcn_sim_normalize")
    return tuple(float(v) for v in stats.cpu().numpy())


def spearman(x, y):
    """Spearman correlation of two CUDA tensors of equal size (flattened, compared as float64) with average ranks for ties, as
    pandas' corr(method='spearman') and scipy.stats.spearmanr give it.  NaN when either input is constant or has fewer than 2
    values."""
    _require_cuda(x, "x")
    _require_cuda(y, "y")
    x = x.reshape(-1).to(torch.float64)
    y = y.reshape(-1).to(torch.float64)
    if x.numel() != y.numel():
        raise ValueError("x and y have different sizes")
    N = x.numel()
    if N < 2:
        return float("nan")
    if bool(torch.isnan(x).any().item()) or bool(torch.isnan(y).any().item()):
        raise ValueError("spearman: NaN input")
    dev = x.device
    lib = _lib.load()
    _require_free(dev, N * (16 + 16 + 16) + lib.ctgcn_sim_spearman_workspace_bytes(N), "the Spearman correlation of %d values" % N)
    xs, xi = torch.sort(x, stable=True)
    ys, yi = torch.sort(y, stable=True)
    sums = torch.empty(3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        nb = lib.ctgcn_sim_spearman_workspace_bytes(N)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        check(lib.ctgcn_sim_spearman(N, ptr(xs), ptr(xi), ptr(ys), ptr(yi), ptr(sums), ptr(ws), nb, _stream(dev)), "ctgcn_sim_spearman")
    sxy, sxx, syy = (float(v) for v in sums.cpu().numpy())
    if sxx == 0.0 or syy == 0.0:
        return float("nan")
    return sxy / np.sqrt(sxx * syy)


def gram(embedding, rows):
    """E[rows] E[rows]ᵀ in float64 on the device (exactly symmetric).  embedding: CUDA [n, d] float32 or float64; rows: int64 indices."""
    _require_cuda(embedding, "embedding")
    dev = embedding.device
    E = embedding if embedding.dtype in (torch.float32, torch.float64) else embedding.to(torch.float64)
    if E.dim() != 2 or E.stride(1) != 1:
        E = E.reshape(E.shape[0], -1).contiguous()
    rows = torch.as_tensor(rows, dtype=torch.int64).to(dev).contiguous()
    k, d = rows.numel(), E.shape[1]
    if k and (int(rows.min().item()) < 0 or int(rows.max().item()) >= E.shape[0]):
        raise ValueError("gram: a row index is outside the embedding")
    out = torch.empty(k, k, dtype=torch.float64, device=dev)
    suffix = "f32" if E.dtype == torch.float32 else "f64"
    with torch.cuda.device(dev):
        check(getattr(_lib.load(), "ctgcn_sim_gram_" + suffix)(k, d, ptr(E), E.stride(0), ptr(rows), ptr(out), _stream(dev)),
              "ctgcn_sim_gram_" + suffix)
    return out


def block_error(real, pred):
    """The reference's score of two kept blocks (CUDA float64 [k, k], both consumed): each min-max scaled and divided by its sum,
    then the Spearman correlation of the flattened blocks.  NaN when a block is constant."""
    rmin, rmax, _ = _normalize(real)
    pmin, pmax, _ = _normalize(pred)
    if rmin == rmax or pmin == pmax:
        return float("nan")
    return spearman(real, pred)


def _embedding_tensor(embedding, dev):
    E = embedding if isinstance(embedding, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(embedding))
    if E.dtype not in (torch.float32, torch.float64):
        E = E.to(torch.float64)
    return E.to(dev)


def prediction_error(node_sim_mat, embedding, date=None, device=None):
    """get_prediction_error on the GPU: [date, Spearman correlation].  node_sim_mat: the n x n similarity as a Similarity, a scipy
    sparse matrix, a numpy array or a tensor; embedding: [n, d] (numpy or tensor; float32 stays float32, converted exactly).  The
    kept rows are those whose similarity row sums to at least 1e-6; none raises ValueError."""
    dev = _device(device) if not isinstance(embedding, torch.Tensor) or not embedding.is_cuda else embedding.device
    if isinstance(embedding, torch.Tensor) and not embedding.is_cuda:
        _require_cuda(embedding, "embedding")
    if isinstance(node_sim_mat, Similarity):
        kb = node_sim_mat.kept()
        k = kb.numel()
        if k:
            _require_free(dev, 64 * k * k, "the %d x %d kept blocks" % (k, k))
        real = node_sim_mat.block[kb][:, kb].contiguous()
        kept = node_sim_mat.keep[kb]
    elif sp.issparse(node_sim_mat):
        M = sp.csr_matrix(node_sim_mat)
        kept = np.nonzero(~(np.asarray(M.sum(1)).ravel() < EPS))[0]
        k = len(kept)
        if k:
            _require_free(dev, 64 * k * k, "the %d x %d kept blocks" % (k, k))
        real = torch.from_numpy(M[kept][:, kept].toarray().astype(np.float64)).to(dev)
    else:
        M = node_sim_mat if isinstance(node_sim_mat, torch.Tensor) else torch.from_numpy(np.asarray(node_sim_mat, dtype=np.float64))
        M = M.to(dev, torch.float64)
        kept = torch.nonzero(~(M.sum(1) < EPS)).flatten()
        k = kept.numel()
        if k:
            _require_free(dev, 64 * k * k, "the %d x %d kept blocks" % (k, k))
        real = M[kept][:, kept].contiguous()
    if k == 0:
        raise ValueError("no similarity row sums to 1e-6 or more: nothing to score (%s)" % (date,))
    pred = gram(_embedding_tensor(embedding, dev), torch.as_tensor(kept, dtype=torch.int64))
    return [date, block_error(real, pred)]


def evaluate(embedding, row_ptr, col, val, alpha=0.5, iter_num=100, lambda_1=None, panel_cols=None, date=None):
    """From the graph to the correlation, no files: vertex_similarity of the GPU CSR, then prediction_error of the embedding
    (CUDA [n, d], rows in node-file order).  Returns [date, Spearman correlation]."""
    _require_cuda(embedding, "embedding")
    sim = vertex_similarity(row_ptr, col, val, alpha=alpha, iter_num=iter_num, lambda_1=lambda_1, panel_cols=panel_cols)
    return prediction_error(sim, embedding, date)


class DataGenerator(object):
    """Reference DataGenerator: writes <date>_similarity.npz (scipy COO of the n x n similarity, int32 row/col, float64 data)."""

    def __init__(self, base_path, input_folder, output_folder, node_file, file_sep='\t', alpha=0.5, iter_num=100, device=None,
                 panel_cols=None):
        self.base_path = base_path
        self.input_base_path = os.path.abspath(os.path.join(base_path, input_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = _read_nodes(os.path.abspath(os.path.join(base_path, node_file)))
        self.node_num = len(self.full_node_list)
        self.alpha = alpha
        self.iter_num = iter_num
        _check_alpha(alpha)
        self.device = device
        self.panel_cols = panel_cols
        os.makedirs(self.input_base_path, exist_ok=True)
        os.makedirs(self.output_base_path, exist_ok=True)

    def similarity(self, file, lambda_1=None):
        """The Similarity of a snapshot file of input_folder."""
        path = os.path.join(self.input_base_path, file)
        A = graph_csr(path, self.full_node_list, sep=self.file_sep)
        if A.nnz == 0:
            raise ValueError("%s has no edges: the similarity is undefined (the reference writes NaNs)" % path)
        dev = _device(self.device)
        rp = torch.from_numpy(A.indptr.astype(np.int32)).to(dev)
        col = torch.from_numpy(A.indices.astype(np.int32)).to(dev)
        val = torch.from_numpy(A.data.astype(np.float64)).to(dev)
        return vertex_similarity(rp, col, val, alpha=self.alpha, iter_num=self.iter_num,
                                 lambda_1=lambda_1 if lambda_1 is not None else host_lambda_1(A), panel_cols=self.panel_cols)

    def generate_node_similarity(self, file):
        t1 = time.time()
        date = file.split('.')[0]
        sim = self.similarity(file)
        sp.save_npz(os.path.join(self.output_base_path, date + '_similarity.npz'), sim.to_scipy())
        print('finish generating', date + '_similarity.npz', 'lambda 1:', sim.lambda_1, 'cost time:', time.time() - t1, 'seconds!')

    def generate_node_similarity_all_time(self, worker=-1):
        for file in sorted(os.listdir(self.input_base_path)):
            self.generate_node_similarity(file)


class SimilarityPredictor(object):
    """Reference SimilarityPredictor: <method>_mse_record.csv (date, mse; sep ','), where mse holds the Spearman correlation."""

    def __init__(self, base_path, origin_folder, embedding_folder, similarity_folder, output_folder, node_file, file_sep='\t',
                 device=None):
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.similarity_base_path = os.path.abspath(os.path.join(base_path, similarity_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = _read_nodes(os.path.abspath(os.path.join(base_path, node_file)))
        self.device = device
        for p in (self.embedding_base_path, self.origin_base_path, self.output_base_path):
            os.makedirs(p, exist_ok=True)

    def load_similarity(self, date):
        """<date>_similarity.npz (scipy sparse), else the dense <date>_similarity.csv text (numpy); neither raises FileNotFoundError."""
        npz = os.path.join(self.similarity_base_path, date + '_similarity.npz')
        if os.path.exists(npz):
            return sp.load_npz(npz)
        csv = os.path.join(self.similarity_base_path, date + '_similarity.csv')
        if os.path.exists(csv):
            return np.loadtxt(csv)
        raise FileNotFoundError("no similarity file for %s: neither %s nor %s exists" % (date, npz, csv))

    def get_prediction_error(self, method, node_sim_mat, embedding_mat, date):
        return prediction_error(node_sim_mat, embedding_mat, date, self.device)

    def similarity_prediction_all_time(self, method):
        all_mse_list = []
        for date, _, cur_embedding_path, node_sim_mat in method_snapshots(self.origin_base_path, self.embedding_base_path, method,
                                                                          first=self.load_similarity):
            embedding = read_embedding(cur_embedding_path, self.file_sep, self.full_node_list)
            all_mse_list.append(self.get_prediction_error(method, node_sim_mat, embedding, date))
        df_output = pd.DataFrame(all_mse_list, columns=['date', 'mse'])
        print(df_output)
        df_output.to_csv(os.path.join(self.output_base_path, method + '_mse_record.csv'), sep=',', index=False)

    def similarity_prediction_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = sorted(os.listdir(self.embedding_base_path))
        for method in method_list:
            self.similarity_prediction_all_time(method)


def similarity_prediction(args):
    """The reference's sim_pred driver: the same config keys ('worker' ignored); unlike the reference it runs the predictor."""
    base_path = args['base_path']
    data_generator = DataGenerator(base_path=base_path, input_folder=args['origin_folder'], output_folder=args['similarity_data_folder'],
                                   node_file=args['node_file'], file_sep=args['file_sep'], alpha=args['alpha'], iter_num=args['iter_num'])
    if args['generate']:
        data_generator.generate_node_similarity_all_time(worker=args.get('worker', -1))
    predictor = SimilarityPredictor(base_path=base_path, origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                    similarity_folder=args['similarity_data_folder'], output_folder=args['similarity_res_folder'],
                                    node_file=args['node_file'], file_sep=args['file_sep'])
    t1 = time.time()
    predictor.similarity_prediction_all_method(method_list=args['method_list'], worker=args.get('worker', -1))
    print('node similarity prediction cost time: ', time.time() - t1, ' seconds!')
