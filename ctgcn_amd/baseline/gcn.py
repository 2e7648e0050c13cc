"""GCN (https://arxiv.org/abs/1609.02907) with the constructor, forward signature and state_dict keys of the reference's
baseline/gcn.py, so checkpoints move both ways.

A layer is Â (X W) + b.  The N-sized work after the product — the aggregation over the normalised adjacency, the bias and what
follows it (ReLU and dropout after layer 1; nothing, or GCRN's row normalisation, after layer 2) — is one pass of ctgcn_gcn.hip
(ops.gcn_conv), and so is its backward: one N x d pre-pass and the plain aggregation over Â^T.  The matrix is taken as given and
need not be symmetric: the reference trains GCN / GCRN on D^-1 (A + I) (get_date_adj_list(normalize=True, row_norm=True)).

Dropout is counter-based: entry (i, c) of snapshot t is dropped iff u01(key + t, i, c) < p, with one base key per training-mode
forward drawn from torch's default CPU generator, so torch.manual_seed reproduces a run and no mask is stored.
"""
import math

import torch
from torch import nn

from .. import layers, ops


def draw_key(module):
    """The base dropout key of one training-mode forward (0 when nothing is dropped: no draw is made)."""
    if not (module.training and module.dropout > 0):
        return 0
    return int(torch.randint(0, 2 ** 62, (1,)))


class GraphConvolution(nn.Module):
    def __init__(self, input_dim, output_dim, bias=True):
        super().__init__()
        self.input_dim, self.output_dim = input_dim, output_dim
        self.weight = nn.Parameter(torch.empty(input_dim, output_dim))
        if bias:
            self.bias = nn.Parameter(torch.empty(output_dim))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        with torch.no_grad():
            self.weight.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def support(self, x):
        """X W.  The sparse identity (get_feature_list without a feature file) needs no product: X W = W, and dW is dS."""
        if x.is_sparse:
            if layers._is_identity(x) and x.shape[1] == self.weight.shape[0]:
                return self.weight
            return torch.sparse.mm(x, self.weight)
        return torch.matmul(x, self.weight)

    def aggregate(self, S, adj, epi, p, key, out):
        """epi(Â S + b): the fused pass; overridden by tools/gcrn_bench.py's composed variant"""
        return ops.gcn_conv(S, adj, self.bias, epi, p, key, out=out)

    def forward(self, input, adj, epi=ops.GCN_EPI_NONE, p=0.0, key=0, out=None):
        ops._need_cuda(input)
        adj = layers.as_gcn_adj(adj, input.device, symmetric=False)
        return self.aggregate(self.support(input), adj, epi, p, key, out)

    def __repr__(self):
        return '%s (%d -> %d)' % (self.__class__.__name__, self.input_dim, self.output_dim)


class GCN(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, dropout=0.5, bias=True):
        super().__init__()
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.dropout = dropout
        self.bias = bias
        self.method_name = 'GCN'
        self.gc1 = GraphConvolution(input_dim, hidden_dim, bias=bias)
        self.gc2 = GraphConvolution(hidden_dim, output_dim, bias=bias)

    def forward(self, x, adj):
        """[N, output_dim], or a list of them for a list of snapshots; adj an ops.GcnAdj or the loader's normalised sparse tensor"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self.gcn(x[t], adj[t], key + t) for t in range(len(x))]
        return self.gcn(x, adj, key)

    def gcn(self, x, adj, key=0, epi=ops.GCN_EPI_NONE, out=None):
        """One snapshot: layer 1 with ReLU and (in training mode) dropout under `key`, layer 2 with `epi`, written to `out` if given."""
        ops._need_cuda(x)
        adj = layers.as_gcn_adj(adj, x.device, symmetric=False)
        p = float(self.dropout) if self.training else 0.0
        h = self.gc1(x, adj, ops.GCN_EPI_RELU, p, key)
        return self.gc2(h, adj, epi, out=out)
