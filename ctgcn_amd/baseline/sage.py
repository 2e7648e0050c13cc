"""GraphSAGE (https://arxiv.org/abs/1706.02216) with the constructors, forward signature and state_dict keys of the reference's
baseline/sage.py (its Aggregator / SAGE_Layer / SAGE), so checkpoints move both ways.

A layer is normalize(relu(Linear([h | pool(h)]))) with gcn=False and normalize(relu(Linear(pool(h)))) with gcn=True, where pool reads the
pattern of the adjacency alone (weights are ignored) and, with gcn=True, the node joins its own neighbour set, as a set.  sum and average
commute with the Linear, [h | pool(h)] W^T = h W_self^T + Â (h W_neigh^T), so a layer is one product Z = h [W_self ; W_neigh]^T of
width 2 out and one pass of ops.pool_conv (ctgcn_pool.hip) over its two halves: the gather at the output width, the self half, the bias,
ReLU, the row's L2 normalisation and the dropout between the layers.  Neither the pooled [N, in] matrix nor the [N, 2 in] concatenation
exists, and no dense [N, N] mask.  The pattern matrix (values 1, or 1 / set size; an empty set gives zeros) is built once per adjacency
(layers.as_pool_adj).  max is ops.pool_max (zeros for an empty set, ties to the lowest index), two products into one output, and the
same pass without a matrix as the epilogue.

num_sample=None (no sampling) is what every config of the reference uses and what is built.  Any other value raises
NotImplementedError: the reference samples with Python's random.sample per node and per forward, and no device sampler exists yet.

Dropout is counter-based and nothing is stored: one base key per training-mode forward (gcn.draw_key; torch.manual_seed reproduces a
run bit for bit).  Entry (i, c) of layer 1's output of snapshot t is dropped iff u01(base + t, i, c) < dropout.
"""
import torch
from torch import nn
from torch.nn import functional as F

from .. import layers, ops
from .gcn import draw_key
from .gin import linear_input


class Aggregator(nn.Module):
    """pool(features) over the neighbour sets of an adjacency's pattern: sum, average or max"""

    def __init__(self, num_sample=None, pooling_type='sum', gcn=False):
        super().__init__()
        if num_sample is not None:
            raise NotImplementedError("num_sample=%r: the reference samples neighbours with Python's random.sample per node and per forward, and "
                                      "no device sampler exists yet; num_sample=None (no sampling, what every config uses) is supported" % (num_sample,))
        assert pooling_type in ['sum', 'average', 'max']
        self.num_sample = num_sample
        self.pooling_type = pooling_type
        self.gcn = gcn

    def matrix(self, adj):
        """the GcnAdj this aggregator reads: adj itself for max without a self loop (ops.pool_max reads the pattern alone), else the
        pattern matrix built once and cached on adj.  A GcnAdj holds each entry once, as from_scipy and from_sparse_tensor build it"""
        if self.pooling_type == 'max' and not self.gcn:
            return adj
        kind = 'pattern-average' if self.pooling_type == 'average' else 'pattern-sum'
        return layers.as_pool_adj(adj, kind, self_loop=self.gcn)

    def forward(self, features, adj):
        ops._need_cuda(features)
        m = self.matrix(layers.as_gcn_adj(adj, features.device, symmetric=False))
        if self.pooling_type == 'max':
            return ops.pool_max(features, m)
        return ops.gcn_conv(features, m)


class SAGE_Layer(nn.Module):
    def __init__(self, input_dim, output_dim, num_sample=10, pooling_type='sum', gcn=False, bias=True):
        super().__init__()
        self.input_dim, self.output_dim = input_dim, output_dim
        self.num_sample = num_sample
        self.pooling_type = pooling_type
        self.gcn = gcn
        self.bias = bias
        self.aggregator = Aggregator(num_sample=num_sample, pooling_type=pooling_type, gcn=gcn)
        self.linear = nn.Linear(input_dim if self.gcn else 2 * input_dim, output_dim, bias=bias)

    def forward(self, features, adj, p=0.0, key=0):
        """dropout(normalize(relu(Linear([features | pool(features)])))): dropout with probability p under `key` (0: none)"""
        ops._need_cuda(features)
        adj = layers.as_gcn_adj(adj, features.device, symmetric=False)
        m = self.aggregator.matrix(adj)
        W, b, k = self.linear.weight, self.linear.bias, self.input_dim
        if self.pooling_type == 'max':
            pooled = ops.pool_max(features, m)
            pre = F.linear(pooled, W) if self.gcn else torch.addmm(F.linear(features, W[:, :k]), pooled, W[:, k:].t())
            return ops.pool_conv(None, None, T=pre, bias=b, epi=ops.POOL_EPI_NORM, p=p, key=key)
        if self.gcn:
            return ops.pool_conv(F.linear(features, W), m, bias=b, epi=ops.POOL_EPI_NORM, p=p, key=key)
        out = self.output_dim
        Z = F.linear(features, torch.cat((W[:, :k], W[:, k:]), dim=0))                 # [N, 2 out] = [h W_self^T | h W_neigh^T]
        return ops.pool_conv(Z[:, out:], m, T=Z[:, :out], bias=b, epi=ops.POOL_EPI_NORM, p=p, key=key)


class SAGE(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_sample=10, pooling_type='sum', gcn=False, dropout=0.5, bias=True):
        super().__init__()
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.num_sample = num_sample
        self.pooling_type = pooling_type
        self.dropout = dropout
        self.bias = bias
        self.method_name = 'SAGE'
        self.linear = nn.Linear(input_dim, hidden_dim, bias=bias)
        self.sage1 = SAGE_Layer(hidden_dim, hidden_dim, num_sample, pooling_type=pooling_type, gcn=gcn, bias=bias)
        self.sage2 = SAGE_Layer(hidden_dim, output_dim, num_sample, pooling_type=pooling_type, gcn=gcn, bias=bias)

    def forward(self, x, adj):
        """[N, output_dim], or a list of them for a list of snapshots; adj an ops.GcnAdj or the loader's raw sparse adjacency"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self.sage(x[t], adj[t], key + t) for t in range(len(x))]
        return self.sage(x, adj, key)

    def sage(self, x, adj, key=0):
        """One snapshot: layer 1 with (in training mode) dropout under `key`, then layer 2"""
        ops._need_cuda(x)
        adj = layers.as_gcn_adj(adj, x.device, symmetric=False)
        p = float(self.dropout) if self.training else 0.0
        h = self.sage1(linear_input(self.linear, x), adj, p, key)
        return self.sage2(h, adj)
