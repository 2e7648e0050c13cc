"""TgGCN, TgGAT, TgSAGE and TgGIN: the PyTorch-Geometric variants of the reference's baseline/gcn.py, gat.py, sage.py and gin.py, with
their constructors, forward signature (x, edge_index on a raw [2, E] index, no adjacency) and state_dict keys.  torch_geometric is
not needed: the four conv layers below carry PyG 1.6.0's parameters, initialisers and formulas, so checkpoints move both ways.

    TgGCNConv   Â (x W) + b over the edge index's own normalisation: a unit self loop per node, D^-1/2 (A + I) D^-1/2 with the degree
                counted on the target side and repeated pairs with multiplicity (ops.TgGraph.looped, ops.gcn_conv)
    TgGATConv   one head of softmax_j(leakyrelu_0.2(att_r · x_i W + att_l · x_j W)) over the same looped pattern, plus b (ops.tgat_conv)
    TgSAGEConv  lin_l(mean_j x_j) + lin_r(x_i): one product of width 2 out, then ops.tg_conv over TgGraph.mean
    TgGINConv   nn((1 + eps) x_i + sum_j x_j) for a Linear nn, which commutes with the sum: ops.tg_conv over TgGraph.sum, T = S

Everything after a layer's product is one fused pass of ctgcn_tg.hip / ctgcn_gcn.hip / ctgcn_gat.hip, the ReLU and the dropout the
models put after it included.  An edge_index is turned into an ops.TgGraph on first sight and kept, keyed by its data pointer, shape
and version counter, so an epoch loop builds nothing; a prepared ops.TgGraph may be passed in its place.

Dropout is counter-based as in baseline/gcn.py: one base key per training-mode forward (gcn.draw_key, so torch.manual_seed
reproduces a run), and layer l of snapshot t draws entry (i, c) from u01(base + 2^32 l + t, i, c).  Reproduced from the reference:
TgGAT discards the dropout of its hidden layers (gat.py:210), so only conv_first is followed by one; TgGIN's default dropout=True
is p = 1 in F.dropout, which zeroes the layer.
"""
import math

import torch
from torch import nn

from .. import layers, ops
from .._lib import CtgcnHipError
from .gcn import draw_key
from .gin import linear_input

LAYER_KEY = 2 ** 32                     # layer l of snapshot t draws from base + LAYER_KEY * l + t
_GRAPH_CACHE = 64                       # edge indices a model keeps prepared


def glorot_(t):
    """PyG's glorot: uniform in ±sqrt(6 / (size(-2) + size(-1)))"""
    bound = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-bound, bound)


def _need_gpu(what, *tensors):
    for t in tensors:
        if isinstance(t, torch.Tensor) and not t.is_cuda:
            raise CtgcnHipError("%s runs on the MI355X only: got a %s tensor; there is no CPU fallback" % (what, t.device))


def _product(x, weight_t):
    """x @ weight_t^T for weight_t [out, in]: dense, the loader's sparse features, or the sparse identity (no product)"""
    if not x.is_sparse:
        return torch.nn.functional.linear(x, weight_t)
    if layers._is_identity(x) and x.shape[1] == weight_t.shape[1]:
        return ops.linear_of_identity(weight_t, None)
    return torch.sparse.mm(x, weight_t.t())


class TgGCNConv(nn.Module):
    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.weight = nn.Parameter(torch.empty(in_channels, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.weight)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, graph, epi=ops.TG_EPI_NONE, p=0.0, key=0):
        if x.is_sparse:
            S = self.weight if (layers._is_identity(x) and x.shape[1] == self.in_channels) else torch.sparse.mm(x, self.weight)
        else:
            S = torch.matmul(x, self.weight)
        return ops.gcn_conv(S, graph.looped, self.bias, ops.GCN_EPI_RELU if epi == ops.TG_EPI_RELU else ops.GCN_EPI_NONE, p, key)

    def __repr__(self):
        return '%s(%d, %d)' % (self.__class__.__name__, self.in_channels, self.out_channels)


class TgGATConv(nn.Module):
    """heads = 1, concat, negative_slope 0.2, no attention dropout: the defaults the reference builds it with"""
    negative_slope = 0.2

    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_l = nn.Linear(in_channels, out_channels, bias=False)
        self.lin_r = self.lin_l                          # an int in_channels: PyG registers one Linear under both names
        self.att_l = nn.Parameter(torch.empty(1, 1, out_channels))
        self.att_r = nn.Parameter(torch.empty(1, 1, out_channels))
        if bias:
            self.bias = nn.Parameter(torch.empty(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot_(self.lin_l.weight)
        glorot_(self.att_l)
        glorot_(self.att_r)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def forward(self, x, graph, epi=ops.TG_EPI_NONE, p=0.0, key=0):
        S = _product(x, self.lin_l.weight)
        return ops.tgat_conv(S, self.att_r.view(1, -1), self.att_l.view(1, -1), graph.looped, 1, self.negative_slope, self.bias, epi, p, key)

    def __repr__(self):
        return '%s(%d, %d, heads=1)' % (self.__class__.__name__, self.in_channels, self.out_channels)


class TgSAGEConv(nn.Module):
    def __init__(self, in_channels, out_channels, bias=True):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.lin_l = nn.Linear(in_channels, out_channels, bias=bias)
        self.lin_r = nn.Linear(in_channels, out_channels, bias=False)

    def reset_parameters(self):
        self.lin_l.reset_parameters()
        self.lin_r.reset_parameters()

    def forward(self, x, graph, epi=ops.TG_EPI_NONE, p=0.0, key=0):
        d = self.out_channels
        Z = _product(x, torch.cat((self.lin_l.weight, self.lin_r.weight), dim=0))     # [x W_l^T | x W_r^T]
        return ops.tg_conv(Z[:, :d], graph.mean, Z[:, d:], 1.0, self.lin_l.bias, epi, p, key)

    def __repr__(self):
        return '%s(%d, %d)' % (self.__class__.__name__, self.in_channels, self.out_channels)


class TgGINConv(nn.Module):
    """GINConv(nn) with eps = 0 and train_eps = False, for the nn the reference gives it: one Linear"""

    def __init__(self, nn_module, eps=0.0):
        super().__init__()
        if not isinstance(nn_module, nn.Linear):
            raise TypeError("TgGINConv fuses a Linear nn (what TgGIN builds it with), got %s" % type(nn_module).__name__)
        self.nn = nn_module
        self.initial_eps = eps
        self.register_buffer('eps', torch.Tensor([eps]))
        self._eps_seen = (None, eps)

    def reset_parameters(self):
        self.nn.reset_parameters()
        self.eps.data.fill_(self.initial_eps)

    def eps_value(self):
        """the buffer as a float (the kernel takes the scale by value): read back once per change of the buffer, not per call"""
        tag = (self.eps.data_ptr(), self.eps._version)
        if self._eps_seen[0] != tag:
            self._eps_seen = (tag, float(self.eps))
        return self._eps_seen[1]

    def forward(self, x, graph, epi=ops.TG_EPI_NONE, p=0.0, key=0):
        S = _product(x, self.nn.weight)
        return ops.tg_conv(S, graph.sum, S, 1.0 + self.eps_value(), self.nn.bias, epi, p, key)

    def __repr__(self):
        return '%s(nn=%s)' % (self.__class__.__name__, self.nn)


class _TgModel(nn.Module):
    """What the four models share: the reference's attributes, the list / single-snapshot forward, the graph cache and the keys."""
    method_name = None
    hidden_dropout = True               # False: the hidden layers' dropout is discarded (TgGAT)

    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre, layer_num, dropout, bias):
        super().__init__()
        self.input_dim, self.feature_dim, self.hidden_dim, self.output_dim = input_dim, feature_dim, hidden_dim, output_dim
        self.feature_pre, self.layer_num, self.dropout, self.bias = feature_pre, layer_num, dropout, bias
        self.method_name = type(self).method_name
        self._graphs = {}
        if feature_pre:
            self.linear_pre = nn.Linear(input_dim, feature_dim, bias=bias)

    def graph(self, edge_index, n):
        """The ops.TgGraph of an edge index: itself when prepared, else built on first sight and kept"""
        if isinstance(edge_index, ops.TgGraph):
            if edge_index.n != n:
                raise ValueError("a TgGraph of %d nodes for features of %d rows" % (edge_index.n, n))
            return edge_index
        _need_gpu(self.method_name, edge_index)
        assert edge_index.shape[0] == 2
        tag = (edge_index.data_ptr(), tuple(edge_index.shape), edge_index._version, n)
        g = self._graphs.get(tag)
        if g is None:
            if len(self._graphs) >= _GRAPH_CACHE:
                self._graphs.pop(next(iter(self._graphs)))
            g = self._graphs[tag] = ops.TgGraph(edge_index.to(torch.int64), n)
        return g

    def forward(self, x, edge_index):
        """[N, output_dim], or a list of them for a list of snapshots; edge_index an int64 [2, E] CUDA tensor or an ops.TgGraph"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self._snapshot(x[t], edge_index[t], key + t) for t in range(len(x))]
        return self._snapshot(x, edge_index, key)

    def _snapshot(self, x, edge_index, key=0):
        _need_gpu(self.method_name, x)
        g = self.graph(edge_index, x.shape[0])
        p = float(self.dropout) if self.training else 0.0
        if self.feature_pre:
            x = linear_input(self.linear_pre, x)
        convs = [self.conv_first] + list(self.conv_hidden)
        for l, conv in enumerate(convs):
            pl = p if (l == 0 or self.hidden_dropout) else 0.0
            x = conv(x, g, ops.TG_EPI_RELU, pl if pl < 1.0 else 0.0, key + LAYER_KEY * l)
            if pl >= 1.0:
                x = x * 0.0                                      # F.dropout(p = 1): every entry dropped
        return self.conv_out(x, g)


class TgGCN(_TgModel):
    method_name = 'TgGCN'

    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True, **kwargs):
        super().__init__(input_dim, feature_dim, hidden_dim, output_dim, feature_pre, layer_num, dropout, bias)
        self.conv_first = TgGCNConv(feature_dim if feature_pre else input_dim, hidden_dim, bias=bias)
        self.conv_hidden = nn.ModuleList([TgGCNConv(hidden_dim, hidden_dim, bias=bias) for _ in range(layer_num - 2)])
        self.conv_out = TgGCNConv(hidden_dim, output_dim, bias=bias)

    gcn = _TgModel._snapshot


class TgGAT(_TgModel):
    method_name = 'TgGAT'
    hidden_dropout = False

    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True, **kwargs):
        super().__init__(input_dim, feature_dim, hidden_dim, output_dim, feature_pre, layer_num, dropout, bias)
        self.conv_first = TgGATConv(feature_dim if feature_pre else input_dim, hidden_dim, bias=bias)
        self.conv_hidden = nn.ModuleList([TgGATConv(hidden_dim, hidden_dim, bias=bias) for _ in range(layer_num - 2)])
        self.conv_out = TgGATConv(hidden_dim, output_dim, bias=bias)

    gat = _TgModel._snapshot


class TgSAGE(_TgModel):
    method_name = 'TgSAGE'

    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True, **kwargs):
        super().__init__(input_dim, feature_dim, hidden_dim, output_dim, feature_pre, layer_num, dropout, bias)
        self.conv_first = TgSAGEConv(feature_dim if feature_pre else input_dim, hidden_dim, bias=bias)
        self.conv_hidden = nn.ModuleList([TgSAGEConv(hidden_dim, hidden_dim, bias=bias) for _ in range(layer_num - 2)])
        self.conv_out = TgSAGEConv(hidden_dim, output_dim, bias=bias)

    sage = _TgModel._snapshot


class TgGIN(_TgModel):
    method_name = 'TgGIN'

    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=True, bias=True, **kwargs):
        super().__init__(input_dim, feature_dim, hidden_dim, output_dim, feature_pre, layer_num, dropout, bias)
        # the reference registers each Linear under its own name and again inside its GINConv: both sets of keys, one parameter
        self.conv_first_nn = nn.Linear(feature_dim if feature_pre else input_dim, hidden_dim, bias=bias)
        self.conv_first = TgGINConv(self.conv_first_nn)
        self.conv_hidden_nn = nn.ModuleList([nn.Linear(hidden_dim, hidden_dim, bias=bias) for _ in range(layer_num - 2)])
        self.conv_hidden = nn.ModuleList([TgGINConv(self.conv_hidden_nn[i]) for i in range(layer_num - 2)])
        self.conv_out_nn = nn.Linear(hidden_dim, output_dim, bias=bias)
        self.conv_out = TgGINConv(self.conv_out_nn)

    gin = _TgModel._snapshot
