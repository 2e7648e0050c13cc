"""GIN (https://arxiv.org/abs/1810.00826) with the constructors, forward signature and state_dict keys of the reference's
baseline/gin.py (its MLP / GIN pair), so checkpoints move both ways.

A layer pools the neighbours' rows, runs them through an MLP (Linear -> BatchNorm -> ReLU -> ... -> Linear), then BatchNorm, ReLU and,
on every layer but the last, dropout.  The pooling and everything elementwise are ctgcn_pool.hip:
  sum / average  the adjacency's weights plus a unit diagonal (average: each row over its weighted sum), one ops.gcn_conv over a matrix
                 built once per adjacency (layers.as_pool_adj);
  max            ops.pool_max over the stored pattern: no self loop, zeros for a row without entries, ties to the lowest index;
  learn_eps      the adjacency as given, plus (1 + eps[l]) h: ops.pool_conv with h as its own self term (max: added afterwards).
                 The reference cannot run sum / average with learn_eps (its Adj_block_idx is never assigned and it raises
                 UnboundLocalError); this is its evident intent, and a row without entries pools to 0;
  BatchNorm      ops.batch_norm_act: fp64 statistics, then one pass for the normalisation, the ReLU and the dropout; the backward keeps
                 x, the mean and rstd, and makes the ReLU mask and the draw again.
Each snapshot of a list is its own BatchNorm batch, and the running statistics are updated snapshot by snapshot, in order.

Dropout is counter-based and nothing is stored: one base key per training-mode forward (gcn.draw_key; torch.manual_seed reproduces a
run bit for bit).  Entry (i, c) of layer l of snapshot t is dropped iff u01(base + 4096 t + l, i, c) < dropout.
"""
import torch
from torch import nn

from .. import layers, ops
from .gcn import draw_key

MAX_LAYERS = 4096                       # a snapshot's layers own the keys [base + 4096 t, + 4096)


def batch_norm(bn, x, relu, p=0.0, key=0):
    """dropout(relu(bn(x))) through ops.batch_norm_act for an nn.BatchNorm1d, whose running buffers are updated as torch updates them:
    the biased variance for the output, the unbiased one for running_var, num_batches_tracked counting the batches"""
    if not bn.training and bn.track_running_stats:
        return ops.batch_norm_act(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, relu, 0.0, 0, bn.eps)[0]
    y, mean, var = ops.batch_norm_act(x, bn.weight, bn.bias, None, None, relu, p if bn.training else 0.0, key, bn.eps)
    if bn.training and bn.track_running_stats:
        with torch.no_grad():
            n = x.shape[0]
            bn.num_batches_tracked += 1
            m = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
            bn.running_mean.mul_(1.0 - m).add_(mean, alpha=m)
            bn.running_var.mul_(1.0 - m).add_(var, alpha=m * n / (n - 1.0))
    return y


def linear_input(linear, x):
    """linear(x) for a dense x or the loader's sparse features; the sparse identity needs no product (ops.linear_of_identity)"""
    if not x.is_sparse:
        return linear(x)
    if layers._is_identity(x) and x.shape[1] == linear.weight.shape[1]:
        return ops.linear_of_identity(linear.weight, linear.bias)
    out = torch.sparse.mm(x, linear.weight.t())
    return out if linear.bias is None else out + linear.bias


class MLP(nn.Module):
    """Linear -> BatchNorm -> ReLU, layer_num - 1 times, then Linear; layer_num 1 is a Linear alone"""

    def __init__(self, input_dim, hidden_dim, output_dim, layer_num, bias=True):
        super().__init__()
        self.linear_or_not = True
        self.layer_num = layer_num
        self.bias = bias
        if layer_num < 1:
            raise ValueError("number of layers should be positive!")
        if layer_num == 1:
            self.linear = nn.Linear(input_dim, output_dim, bias=bias)
        else:
            self.linear_or_not = False
            self.linears = nn.ModuleList()
            self.batch_norms = nn.ModuleList()
            self.linears.append(nn.Linear(input_dim, hidden_dim, bias=bias))
            for _ in range(layer_num - 2):
                self.linears.append(nn.Linear(hidden_dim, hidden_dim, bias=bias))
            self.linears.append(nn.Linear(hidden_dim, output_dim, bias=bias))
            for _ in range(layer_num - 1):
                self.batch_norms.append(nn.BatchNorm1d(hidden_dim))

    def forward(self, x):
        if self.linear_or_not:
            return self.linear(x)
        h = x
        for layer in range(self.layer_num - 1):
            h = batch_norm(self.batch_norms[layer], self.linears[layer](h), relu=True)
        return self.linears[self.layer_num - 1](h)


class GIN(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, layer_num, mlp_layer_num, learn_eps, neighbor_pooling_type='sum', dropout=0.5, bias=True):
        super().__init__()
        assert neighbor_pooling_type in ['sum', 'average', 'max']
        if layer_num > MAX_LAYERS:
            raise ValueError("layer_num %d above %d: the layers' dropout keys would run into the next snapshot's" % (layer_num, MAX_LAYERS))
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.layer_num, self.mlp_layer_num = layer_num, mlp_layer_num
        self.learn_eps = learn_eps
        self.neighbor_pooling_type = neighbor_pooling_type
        self.dropout = dropout
        self.bias = bias
        self.method_name = 'GIN'
        self.eps = nn.Parameter(torch.zeros(self.layer_num))
        self.linear = nn.Linear(input_dim, hidden_dim)
        self.mlps = nn.ModuleList()
        self.batch_norms = nn.ModuleList()
        for _ in range(self.layer_num - 1):
            self.mlps.append(MLP(hidden_dim, hidden_dim, hidden_dim, mlp_layer_num, bias=bias))
            self.batch_norms.append(nn.BatchNorm1d(hidden_dim))
        self.mlps.append(MLP(hidden_dim, hidden_dim, output_dim, mlp_layer_num, bias=bias))
        self.batch_norms.append(nn.BatchNorm1d(output_dim))

    def forward(self, x, adj):
        """[N, output_dim], or a list of them for a list of snapshots; adj an ops.GcnAdj or the loader's raw sparse adjacency"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self.gin(x[t], adj[t], key, t) for t in range(len(x))]
        return self.gin(x, adj, key)

    def pool(self, h, adj, layer):
        kind = self.neighbor_pooling_type
        if kind == 'max':
            pooled = ops.pool_max(h, adj)
            return pooled + (1 + self.eps[layer]) * h if self.learn_eps else pooled
        if not self.learn_eps:
            return ops.gcn_conv(h, layers.as_pool_adj(adj, kind, self_loop=True))
        return ops.pool_conv(h, layers.as_pool_adj(adj, kind), T=h, self_scale=1 + self.eps[layer])

    def gin(self, x, adj, key=0, t=0):
        """One snapshot under the base key `key` as snapshot t"""
        ops._need_cuda(x)
        adj = layers.as_gcn_adj(adj, x.device, symmetric=False)
        p = float(self.dropout) if self.training else 0.0
        h = linear_input(self.linear, x)
        for layer in range(self.layer_num):
            rep = self.mlps[layer](self.pool(h, adj, layer))
            last = layer == self.layer_num - 1
            h = batch_norm(self.batch_norms[layer], rep, relu=True, p=0.0 if last else p, key=key + MAX_LAYERS * t + layer)
        return h
