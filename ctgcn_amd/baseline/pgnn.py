"""Position-aware GNN (https://arxiv.org/abs/1906.04817) with the constructors, forward signatures, initialisers and state_dict keys of
the reference's baseline/pgnn.py (Nonlinear / PGNN_layer / PGNN), so checkpoints move both ways.

Anchor distances.  The reference builds a dense float64 [N, N] matrix of 1 / (d + 1) per snapshot from all-pairs BFS and slices it per
anchor set on the host on every forward.  max / argmax of 1 / (d + 1) over an anchor set is a multi-source BFS from that set in which
every reached node inherits the smallest anchor position among its parents on the previous level, so nothing of [N, N] is needed:
precompute_dist_data returns light handles (the device CSR pattern and the cutoff) and get_dist_max / preselect_anchor run
ops.pgnn_anchor_dist (ctgcn_pgnn.hip) on them.  The reference's dense arrays are accepted too and take a plain torch max / argmax.

The layer.  The reference materialises [N, A, 2 in] and [N, A, out] tensors, A = int(log2 N)^2 anchor sets.  The Linear commutes with
the gather, linear_hidden(cat(d F[idx], F)) = d (F W1^T)[idx] + (F W2^T + b), so a layer is one product of width 2 out and one pass of
ops.pgnn_conv that forms relu(...) per (node, anchor set) in registers and emits the position output and / or the structure output;
hidden layers never compute the position output and the last layer never the structure output.  The trainable distance transform
(dist_compute, a 1 -> out -> 1 MLP on every scalar of [N, A]) runs under autograd on the few distinct values of dists_max and the
kernel indexes the result.

Departures from the reference, each on purpose: dists_max is always [N, A] (its bare .squeeze() mangles A == 1); a parameter whose
output is never used (linear_out_position of every layer but the last when layer_num > 1) keeps grad None, as in the reference, and
not a zero gradient; get_random_anchorset draws on the device from torch's generator; the single-snapshot branch of get_dist_max
returns (dist_max, dist_argmax) where the reference returns dist_max twice (pgnn.py:134).

Dropout is counter-based and nothing is stored: one base key per training-mode forward (gcn.draw_key; torch.manual_seed reproduces a
run bit for bit).  Entry (i, c) of the structure output of layer l (0-based) of snapshot t is dropped iff
u01(base + 4096 t + l, i, c) < dropout.
"""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F
from torch.nn import init

from .. import layers, ops
from .gcn import draw_key
from .gin import linear_input


# ------------------------------------------------------------------------------------------------ anchor sets and distances
class DistHandle(object):
    """What precompute_dist_data keeps of one snapshot: the CSR pattern of the undirected graph on the device, and the cutoff"""

    def __init__(self, row_ptr, col, num_nodes, cutoff):
        self.row_ptr, self.col, self.num_nodes, self.cutoff = row_ptr, col, int(num_nodes), int(cutoff)


def _handle(edge_index, num_nodes, approximate):
    if edge_index.shape[0] != 2:
        raise ValueError("edge_index must be [2, E]")
    ops._need_cuda(edge_index)
    src, dst = edge_index[0].to(torch.int64), edge_index[1].to(torch.int64)
    if src.numel() and (int(torch.minimum(src.min(), dst.min())) < 0 or int(torch.maximum(src.max(), dst.max())) >= num_nodes):
        raise ValueError("edge_index outside [0, %d)" % num_nodes)
    keys = torch.unique(torch.cat((src * num_nodes + dst, dst * num_nodes + src)))           # nx.Graph: undirected, each pair once
    row_ptr = torch.zeros(num_nodes + 1, dtype=torch.int64, device=edge_index.device)
    row_ptr[1:] = torch.bincount(torch.div(keys, num_nodes, rounding_mode="floor"), minlength=num_nodes).cumsum(0)
    if keys.numel() >= 2 ** 31:
        raise ValueError("more than 2^31-1 stored entries")
    return DistHandle(row_ptr.to(torch.int32), (keys % num_nodes).to(torch.int32), num_nodes, approximate if approximate > 0 else -1)


def precompute_dist_data(edge_indices, num_nodes, approximate):
    """The reference's signature: edge_indices a [2, E] CUDA tensor or a list of them, approximate == -1 exact shortest paths, > 0 paths of
    at most that many hops.  Returns a DistHandle per snapshot (a list for a list), not [N, N] arrays: the distances to the anchor sets
    are found per draw by get_dist_max."""
    if isinstance(edge_indices, list):
        return [_handle(e, num_nodes, approximate) for e in edge_indices]
    return _handle(edge_indices, num_nodes, approximate)


def anchor_set_count(node_num, c=1):
    """The number of anchor sets get_random_anchorset(node_num, c) draws: int(log2 n) sizes, int(c int(log2 n)) copies of each.  It is the
    embedding width of a PGNN, whatever its output_dim: callers size a classifier with it."""
    m = int(np.log2(node_num))
    return m * int(c * m)


def get_random_anchorset(n, c=0.5, device=None):
    """The reference's anchor sets: for i < int(log2 n), int(c int(log2 n)) sets of int(n / 2^(i + 1)) distinct nodes each.  Drawn on the
    device from torch's generator (torch.randperm), so torch.manual_seed reproduces a run; NOT numpy's stream, which the reference's
    np.random.choice reads: the same seed gives other sets than the reference."""
    m = int(np.log2(n))
    copy = int(c * m)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    out = []
    for i in range(m):
        size = int(n / np.exp2(i + 1))
        for _ in range(copy):
            out.append(torch.randperm(n, device=device)[:size])
    return out


def _one_dist_max(anchorset_list, node_dist, device, node_ids):
    if isinstance(node_dist, DistHandle):
        level, dist, pos, node = ops.pgnn_anchor_dist((node_dist.row_ptr, node_dist.col), anchorset_list, node_dist.cutoff, node_ids=node_ids)
        dist_argmax = (node if node_ids else pos).to(torch.int64)
        ops.pgnn_prepare(dist, dist_argmax, node_dist.num_nodes, levels=level)            # the integer levels spare the unique over floats
        return dist, dist_argmax
    dense = torch.as_tensor(node_dist).to(device)                                         # the reference's [N, N] array of 1 / (d + 1)
    dist_max = torch.zeros(dense.shape[0], len(anchorset_list), device=device)
    dist_argmax = torch.zeros(dense.shape[0], len(anchorset_list), dtype=torch.int64, device=device)
    for i, ids in enumerate(anchorset_list):
        ids = torch.as_tensor(ids).to(device=device, dtype=torch.int64)
        if ids.numel() == 0:
            continue
        top, arg = dense[:, ids].max(dim=1)
        arg = (dense[:, ids] == top[:, None]).to(torch.int8).argmax(dim=1)               # np.argmax: the first among equal values
        dist_max[:, i] = top.to(dist_max.dtype)
        dist_argmax[:, i] = ids[arg] if node_ids else arg
    return dist_max, dist_argmax


def get_dist_max(anchorset_list, node_dist_list, device, node_ids=False):
    """(dist_max float32 [N, A], dist_argmax int64 [N, A]) per snapshot, lists for a list: the reference's get_dist_max.  A DistHandle
    goes to the HIP distance pass; a dense [N, N] array of the reference's precompute_dist_data takes a torch max / argmax.  node_ids
    False reproduces the reference as written: dist_argmax is the position inside the anchor set, so the layer gathers features of the
    nodes 0 .. |set| - 1.  node_ids True gives the anchors' node ids, as the original P-GNN has them.  For a single snapshot the
    reference returns dist_max twice (pgnn.py:134); here the second value is dist_argmax."""
    if isinstance(node_dist_list, list):
        pairs = [_one_dist_max(anchorset_list, nd, device, node_ids) for nd in node_dist_list]
        return [p[0] for p in pairs], [p[1] for p in pairs]
    return _one_dist_max(anchorset_list, node_dist_list, device, node_ids)


def preselect_anchor(node_num, node_dist_list, device, node_ids=False):
    """One draw of anchor sets (get_random_anchorset(node_num, c=1)) and the distances to them: the reference's preselect_anchor"""
    anchorset_list = get_random_anchorset(node_num, c=1, device=device)
    return get_dist_max(anchorset_list, node_dist_list, device, node_ids=node_ids)


# ------------------------------------------------------------------------------------------------ modules
def linear64(x, weight, bias):
    """F.linear(x, weight, bias) with the product formed in fp64 and rounded to fp32 once.  Most (node, set) pairs of a real anchor draw
    are unreached and gather one and the same row, so a normalised position row is nearly constant and its gradient a small difference
    of large terms: the rounding of these small products (N x in x 2 out, nothing beside the N x A x out pass) is amplified a
    hundredfold in the weight gradients, and fp32 products leave them ten times further from the float64 result than the reference's
    own float32 run on the CPU is."""
    out = F.linear(x.double(), weight.double(), None if bias is None else bias.double())
    return out.to(x.dtype)


def _reset_relu_xavier(module):
    for m in module.modules():
        if isinstance(m, nn.Linear):
            m.weight.data = init.xavier_uniform_(m.weight.data, gain=nn.init.calculate_gain('relu'))
            if m.bias is not None:
                m.bias.data = init.constant_(m.bias.data, 0.0)


class Nonlinear(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, bias=True):
        super().__init__()
        self.linear1 = nn.Linear(input_dim, hidden_dim, bias=bias)
        self.linear2 = nn.Linear(hidden_dim, output_dim, bias=bias)
        self.act = nn.ReLU()
        self.reset_parameters()

    def reset_parameters(self):
        _reset_relu_xavier(self)

    def forward(self, x):
        return self.linear2(self.act(self.linear1(x)))


class PGNN_layer(nn.Module):
    """P-GNN layer that passes messages from the closest anchor of every anchor set alone"""

    def __init__(self, input_dim, output_dim, dist_trainable=True, bias=True):
        super().__init__()
        self.input_dim = input_dim
        self.dist_trainable = dist_trainable
        if self.dist_trainable:
            self.dist_compute = Nonlinear(1, output_dim, 1, bias=bias)
        self.linear_hidden = nn.Linear(input_dim * 2, output_dim, bias=bias)
        self.linear_out_position = nn.Linear(output_dim, 1, bias=bias)
        self.act = nn.ReLU()
        self.reset_parameters()

    def reset_parameters(self):
        _reset_relu_xavier(self)

    def product(self, feature):
        """PS [N, 2 out] = feature W1^T | feature W2^T + b, W1 | W2 the two halves of linear_hidden.weight"""
        W, b, k = self.linear_hidden.weight, self.linear_hidden.bias, self.input_dim
        stacked = torch.cat((W[:, :k], W[:, k:]), dim=0)
        bias = None if b is None else torch.cat((torch.zeros_like(b), b))
        if feature.is_sparse:
            if layers._is_identity(feature) and feature.shape[1] == k:
                return ops.linear_of_identity(stacked, bias)
            PS = torch.sparse.mm(feature, stacked.t())
            return PS if bias is None else PS + bias
        return linear64(feature, stacked, bias)

    def forward(self, feature, dists_max, dists_argmax, need_pos=True, need_struct=True, epi=ops.PGNN_EPI_NONE, p=0.0, key=0):
        """(out_position [N, A], out_structure [N, out]); an output that is not needed is None and costs nothing.  epi
        ops.PGNN_EPI_NORM: out_position's rows L2-normalised; p > 0: dropout on out_structure under `key`."""
        ops._need_cuda(feature)
        n = feature.shape[0]
        if dists_max.dim() != 2:
            raise ValueError("dists_max must be [N, A], got %s" % (tuple(dists_max.shape),))
        PS = self.product(feature)
        lin = self.linear_out_position
        prep = ops.pgnn_prepare(dists_max, dists_argmax, n)
        if prep.composed:
            d = self.dist_compute(dists_max.unsqueeze(-1)).squeeze(-1) if self.dist_trainable else dists_max
            return ops.pgnn_conv_composed(PS, d, dists_argmax.to(torch.int64), lin.weight.reshape(-1), lin.bias, need_pos, need_struct, epi, p, key)
        table = self.dist_compute(prep.values.unsqueeze(-1)).squeeze(-1) if self.dist_trainable else None
        return ops.pgnn_conv(PS, dists_max, dists_argmax, lin.weight, lin.bias, table=table, need_pos=need_pos, need_struct=need_struct,
                             epi=epi, p=p, key=key)


class PGNN(nn.Module):
    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True):
        super().__init__()
        self.input_dim = input_dim
        self.feature_dim = feature_dim
        self.hidden_dim = hidden_dim
        self.output_dim = output_dim
        self.feature_pre = feature_pre
        self.layer_num = layer_num
        self.dropout = dropout
        self.bias = bias
        self.method_name = 'PGNN'
        self.anchor_node_ids = False           # True: the trainers draw dist_argmax as node ids (the original P-GNN), not set positions

        if layer_num == 1:
            hidden_dim = output_dim
        if feature_pre:
            self.linear_pre = nn.Linear(input_dim, feature_dim, bias=bias)
            self.conv_first = PGNN_layer(feature_dim, hidden_dim, bias=bias)
        else:
            self.conv_first = PGNN_layer(input_dim, hidden_dim, bias=bias)
        if layer_num > 1:
            self.conv_hidden = nn.ModuleList([PGNN_layer(hidden_dim, hidden_dim, bias=bias) for i in range(layer_num - 2)])
            self.conv_out = PGNN_layer(hidden_dim, output_dim, bias=bias)

    def forward(self, x, dists_max, dists_argmax):
        """[N, A] position embeddings (A anchor sets, whatever output_dim), or a list of them for a list of snapshots"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self.pgnn(x[t], dists_max[t], dists_argmax[t], key + 4096 * t) for t in range(len(x))]
        return self.pgnn(x, dists_max, dists_argmax, key)

    def pgnn(self, x, dists_max, dists_argmax, key=0):
        """One snapshot; in training mode layer l's structure output is dropped under key + l"""
        ops._need_cuda(x)
        p = float(self.dropout) if self.training else 0.0
        if self.feature_pre:
            x = linear_input(self.linear_pre, x) if x.is_sparse else linear64(x, self.linear_pre.weight, self.linear_pre.bias)
        if self.layer_num == 1:
            return self.conv_first(x, dists_max, dists_argmax, need_struct=False)[0]
        _, x = self.conv_first(x, dists_max, dists_argmax, need_pos=False, p=p, key=key)
        for i in range(self.layer_num - 2):
            _, x = self.conv_hidden[i](x, dists_max, dists_argmax, need_pos=False, p=p, key=key + 1 + i)
        return self.conv_out(x, dists_max, dists_argmax, need_struct=False, epi=ops.PGNN_EPI_NORM)[0]
