"""Graph reconstruction and link prediction as a ranking of all node pairs: MAP and precision@k, the protocol of the DynGEM, DynAE,
DynRNN, DynAERNN and TIMERS papers.  This package's own extension: the reference has no such evaluation (its link_pred task is an AUC
over a balanced edge sample).

The ranking is ops.topk_scores (ctgcn_topk.hip): the k best admissible partners of every node from one fused pass over E Eᵀ on the
exact-fp32 matrix cores, no [n, n] matrix.  Everything else here is plain torch on whatever device its inputs live on:
  score_inputs        the operands of the three metrics ('dot', 'cosine', 'l2': −‖eᵢ − eⱼ‖²/2 as a dot product and two biases)
  ranked_hits         which entries of a ranked list are edges of the target CSR (searchsorted on int64 keys)
  average_precision   AP per node over its first K ranks, MAP over the nodes that have a target edge
  global_precision    precision@k over the unordered pairs i < j ranked by (score descending, i, j ascending), assembled from the
                      per-row upper-triangle lists with a certificate that no pair outside the lists can rank among the first k
A pattern (`target`, `known`) is an ops.GcnAdj or any object with row_ptr, col and n; only the stored positions are read.
"""
import os
import time
from functools import partial

import numpy as np
import pandas as pd
import torch

from . import _common
from ._common import method_snapshots, read_embedding, read_nodes

METRICS = ('dot', 'cosine', 'l2')
MODES = ('recon', 'pred')
START_WIDTH = 16            # first list width of global_precision

_device = partial(_common.device, task="graph-reconstruction")


class Pattern(object):
    """The stored positions of a square sparse matrix as int64 tensors: row_ptr [n + 1], col [nnz] ascending within a row."""

    def __init__(self, row_ptr, col):
        self.row_ptr, self.col = row_ptr.to(torch.int64), col.to(torch.int64)
        self.n = self.row_ptr.numel() - 1
        self.nnz = self.col.numel()
        self.device = self.col.device

    def rows(self):
        return torch.repeat_interleave(torch.arange(self.n, device=self.device), self.row_ptr[1:] - self.row_ptr[:-1])

    def keys(self):
        """row * n + col of every stored position"""
        return self.rows() * self.n + self.col


def _pattern(adj):
    return adj if isinstance(adj, Pattern) else Pattern(adj.row_ptr, adj.col)


def target_pattern(target, known=None):
    """The positions to be found: target's stored positions minus the diagonal, minus those of known.  Columns ascend within a row."""
    t = _pattern(target)
    keys = torch.unique(t.keys())
    keys = keys[(keys // t.n) != (keys % t.n)]
    if known is not None and keys.numel():
        kk = torch.unique(_pattern(known).keys())
        if kk.numel():
            pos = torch.searchsorted(kk, keys).clamp(max=kk.numel() - 1)
            keys = keys[kk[pos] != keys]
    row_ptr = torch.zeros(t.n + 1, dtype=torch.int64, device=keys.device)
    row_ptr[1:] = torch.bincount(keys // t.n, minlength=t.n).cumsum(0)
    return Pattern(row_ptr, keys % t.n)


def score_inputs(E, metric):
    """(X, row_bias, col_bias) with score(i, j) = X[i] · X[j] + col_bias[j] + row_bias[i]; the biases are per node (index a query's
    by its node) or None.  'dot': E as is.  'cosine': the rows of E divided by their L2 norm (a zero row stays zero).  'l2': the
    ranking by −‖eᵢ − eⱼ‖²/2 = eᵢ · eⱼ − ‖eᵢ‖²/2 − ‖eⱼ‖²/2.  Norms are taken in float64 and rounded to float32 once."""
    if metric not in METRICS:
        raise ValueError("metric must be one of %s, got %r" % (METRICS, metric))
    E = E.to(torch.float32)
    if metric == 'dot':
        return E, None, None
    sq = (E.double() ** 2).sum(1)
    if metric == 'cosine':
        norm = sq.sqrt()
        return (E.double() / torch.where(norm > 0, norm, torch.ones_like(norm))[:, None]).to(torch.float32), None, None
    bias = (-0.5 * sq).to(torch.float32)
    return E, bias, bias


def ranked_hits(index, rows, target):
    """bool [m, k]: whether (rows[i], index[i, r]) is a stored position of target (rows None: row i is node i).  Index -1 is a miss."""
    t = _pattern(target)
    m = index.shape[0]
    idx = index.to(torch.int64)
    q = torch.arange(m, device=idx.device) if rows is None else rows.to(torch.int64)
    keys = torch.unique(t.keys())
    if keys.numel() == 0:
        return torch.zeros_like(idx, dtype=torch.bool)
    want = q[:, None] * t.n + idx.clamp(min=0)
    pos = torch.searchsorted(keys, want.reshape(-1)).clamp(max=keys.numel() - 1).reshape(want.shape)
    return (keys[pos] == want) & (idx >= 0)


def average_precision(hits, n_rel, K):
    """(MAP, rows counted, AP [m]) in float64: AP_i = (1 / min(n_rel_i, K)) Σ_{r <= K} hit_i(r) (Σ_{s <= r} hit_i(s)) / r over the
    first K columns of hits; MAP is the mean over the rows with n_rel_i > 0 (NaN when there is none), whose number is returned."""
    K = int(K)
    if K < 1 or K > hits.shape[1]:
        raise ValueError("K = %d outside [1, %d], the width of the ranked lists" % (K, hits.shape[1]))
    h = hits[:, :K]
    found = h.cumsum(1).to(torch.float64)               # counts: exact in any order
    total = torch.zeros(h.shape[0], dtype=torch.float64, device=h.device)
    for r in range(K):                                  # rank by rank, so that a row's sum has one defined order on every device
        total = total + torch.where(h[:, r], found[:, r] / (r + 1.0), torch.zeros_like(total))
    n_rel = n_rel.to(torch.int64)
    ap = total / n_rel.clamp(min=1, max=K).to(torch.float64)
    counted = n_rel > 0
    rows = int(counted.sum())
    return (float(np.mean(ap[counted].cpu().numpy())) if rows else float("nan")), rows, ap     # the mean in row order, on the host


def global_select(score, index, k):
    """From the upper-triangle lists of every node (score, index [n, K'], row i ranking the nodes j > i; unused slots index -1): the
    first min(k, listed) pairs of the order (score descending, i ascending, j ascending) as (i, j) int64 tensors, and whether they
    are certified to be the first pairs of ALL admissible pairs.  A row whose list is full may hide further pairs behind its last
    entry; the selection is certified when no full row's last entry ranks at or before the k-th selected pair (with fewer than k
    pairs listed: when no row is full)."""
    n, width = index.shape
    valid = index >= 0
    i_all = torch.arange(n, device=index.device)[:, None].expand(n, width)[valid]
    j_all = index.to(torch.int64)[valid]
    s_all = score[valid]
    # row-major flattening is (i ascending; within a row score descending, j ascending): a stable sort by score keeps (i, j) ascending
    order = torch.sort(s_all, descending=True, stable=True)[1]
    full = valid[:, width - 1] if width else torch.zeros(n, dtype=torch.bool, device=index.device)
    listed = int(order.numel())
    take = min(int(k), listed)
    sel = order[:take]
    if not bool(full.any()):
        return i_all[sel], j_all[sel], True
    if listed < k:
        return i_all[sel], j_all[sel], False
    # position of every full row's last entry in the order: its flat offset is the row's last valid slot
    offsets = valid.sum(1).cumsum(0) - 1
    rank = torch.empty(listed, dtype=torch.int64, device=index.device)
    rank[order] = torch.arange(listed, device=index.device)
    certified = not bool((rank[offsets[full]] <= take - 1).any())
    return i_all[sel], j_all[sel], certified


def global_precision(X, row_bias, col_bias, target, known, k_list, width=None, max_width=None, topk=None):
    """Precision@k over the unordered pairs i < j that are not in known, ranked by (score descending, i, j ascending): the share of
    the first k pairs that are positions of target.  The pairs come from upper-triangle lists of width K' (START_WIDTH, or `width`),
    doubled until global_select certifies the selection; at max_width (ctgcn_topk_max_k()) an uncertified selection raises
    ValueError: the result is exact or refused.  With fewer than k admissible pairs the denominator is their number.
    Returns {'precision': {k: value}, 'pairs': {k: denominator}, 'width': K', 'doublings': count}.  topk: the ranking function
    (ops.topk_scores by default)."""
    from .. import ops
    topk = ops.topk_scores if topk is None else topk
    k_list = [int(k) for k in k_list]
    if not k_list or min(k_list) < 1:
        raise ValueError("k_list must hold positive integers")
    k_max = max(k_list)
    max_width = ops.topk_max_k() if max_width is None else int(max_width)
    width = min(START_WIDTH if width is None else int(width), max_width)
    doublings = 0
    while True:
        score, index = topk(X, width, row_bias=row_bias, col_bias=col_bias, upper_only=True, exclude=known)
        i_sel, j_sel, certified = global_select(score, index, k_max)
        if certified:
            break
        if width >= max_width:
            raise ValueError("precision@%d cannot be certified from per-node lists of width %d = ctgcn_topk_max_k(): a node's list is "
                             "full at or before the %d-th pair, further pairs may hide behind it" % (k_max, width, k_max))
        width = min(2 * width, max_width)
        doublings += 1
    t = _pattern(target)
    keys = torch.unique(t.keys())
    want = i_sel * t.n + j_sel
    if keys.numel() and want.numel():
        pos = torch.searchsorted(keys, want).clamp(max=keys.numel() - 1)
        hit = (keys[pos] == want).to(torch.float64)
    else:
        hit = torch.zeros(want.numel(), dtype=torch.float64, device=want.device)
    cum = hit.cumsum(0)
    precision, pairs = {}, {}
    for k in k_list:
        den = min(k, int(want.numel()))
        pairs[k] = den
        precision[k] = float(cum[den - 1]) / den if den else float("nan")
    return {'precision': precision, 'pairs': pairs, 'width': width, 'doublings': doublings}


def evaluate(E, target, k_list, max_k=100, metric='dot', known=None):
    """MAP over the nodes' first max_k ranks and precision@k of the global pair ranking for the embedding E (CUDA [n, d]).  target and
    known are GcnAdj of symmetric snapshots: the positions to find are target's minus the diagonal minus known's, and a node's
    candidates are every other node that is not its neighbour in known.  Returns {'MAP', 'rows' (nodes with a position to find),
    'precision' {k: P@k}, 'pairs' {k: denominator}, 'width', 'doublings'}."""
    from .. import ops
    _common.require_cuda(E, "embedding", "graph-reconstruction")
    X, row_bias, col_bias = score_inputs(E, metric)
    tgt = target_pattern(target, known)
    _, index = ops.topk_scores(X, max_k, row_bias=row_bias, col_bias=col_bias, exclude_self=True, exclude=known)
    hits = ranked_hits(index, None, tgt)
    mean_ap, rows, _ = average_precision(hits, tgt.row_ptr[1:] - tgt.row_ptr[:-1], max_k)
    out = global_precision(X, row_bias, col_bias, tgt, known, k_list)
    out.update({'MAP': mean_ap, 'rows': rows})
    return out


class GraphReconstructor(object):
    """<method>_<mode>.csv (date, MAP, P@k ...; sep ',') under output_folder, with a last row 'avg' of the column means.
    mode 'recon': a snapshot's embedding ranks the snapshot's own graph.  mode 'pred': the embedding of the snapshot before ranks the
    new edges of this one, the earlier snapshot's edges being known (excluded from candidates and targets); the first snapshot is
    skipped."""

    def __init__(self, base_path, origin_folder, embedding_folder, output_folder, node_file, file_sep='\t', k_list=None, max_k=100,
                 metric='dot', mode='recon', device=None):
        if mode not in MODES:
            raise ValueError("mode must be one of %s, got %r" % (MODES, mode))
        if metric not in METRICS:
            raise ValueError("metric must be one of %s, got %r" % (METRICS, metric))
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.output_base_path = os.path.abspath(os.path.join(base_path, output_folder))
        self.file_sep = file_sep
        self.full_node_list = read_nodes(os.path.abspath(os.path.join(base_path, node_file)))
        self.k_list = [10, 100, 1000] if k_list is None else [int(k) for k in k_list]
        self.max_k, self.metric, self.mode, self.device = int(max_k), metric, mode, device
        for p in (self.embedding_base_path, self.origin_base_path, self.output_base_path):
            os.makedirs(p, exist_ok=True)

    def graph(self, f_name, dev):
        """The GcnAdj of a snapshot file: symmetric, no self loops, every stored pair an edge"""
        from .. import ops
        from .centrality_prediction import graph_csr
        row_ptr, col = graph_csr(os.path.join(self.origin_base_path, f_name), self.full_node_list, sep=self.file_sep)
        col = torch.from_numpy(col).to(dev)
        return ops.GcnAdj(torch.from_numpy(row_ptr).to(dev), col, torch.ones(col.numel(), dtype=torch.float32, device=dev))

    def evaluate_snapshot(self, f_name, embedding_path, previous=None):
        dev = _device(self.device)
        E = torch.from_numpy(np.ascontiguousarray(read_embedding(embedding_path, self.file_sep, self.full_node_list, np.float32))).to(dev)
        known = self.graph(previous, dev) if previous is not None else None
        return evaluate(E, self.graph(f_name, dev), self.k_list, max_k=self.max_k, metric=self.metric, known=known)

    def graph_reconstruction_all_time(self, method):
        lag = 1 if self.mode == 'pred' else 0
        f_list = sorted(os.listdir(self.origin_base_path))
        records = []
        for date, f_name, cur_embedding_path in method_snapshots(self.origin_base_path, self.embedding_base_path, method, lag=lag):
            previous = f_list[f_list.index(f_name) - 1] if lag else None
            res = self.evaluate_snapshot(f_name, cur_embedding_path, previous)
            records.append([date, res['MAP']] + [res['precision'][k] for k in self.k_list])
        cols = ['date', 'MAP'] + ['P@%d' % k for k in self.k_list]
        df_output = pd.DataFrame(records, columns=cols)
        if len(df_output):
            df_output.loc[len(df_output)] = ['avg'] + [df_output[c].mean() for c in cols[1:]]
        print(df_output)
        df_output.to_csv(os.path.join(self.output_base_path, '%s_%s.csv' % (method, self.mode)), sep=',', index=False)
        return df_output

    def graph_reconstruction_all_method(self, method_list=None, worker=-1):
        if method_list is None:
            method_list = sorted(os.listdir(self.embedding_base_path))
        for method in method_list:
            self.graph_reconstruction_all_time(method)


def graph_reconstruction(args):
    """The graph_recon driver entry.  Config keys: base_path, origin_folder, embed_folder, graph_recon_res_folder, node_file, file_sep,
    method_list, and optionally k_list, max_k, metric, mode ('recon' or 'pred') and worker (ignored)."""
    reconstructor = GraphReconstructor(base_path=args['base_path'], origin_folder=args['origin_folder'], embedding_folder=args['embed_folder'],
                                       output_folder=args['graph_recon_res_folder'], node_file=args['node_file'], file_sep=args['file_sep'],
                                       k_list=args.get('k_list'), max_k=args.get('max_k', 100), metric=args.get('metric', 'dot'),
                                       mode=args.get('mode', 'recon'))
    t1 = time.time()
    reconstructor.graph_reconstruction_all_method(method_list=args['method_list'], worker=args.get('worker', -1))
    print('graph reconstruction cost time: ', time.time() - t1, ' seconds!')
