"""The project's own mirrors of ctgcn_amd.baseline.gin / sage in stock torch ops (index gather, index_add, scatter_reduce,
nn.BatchNorm1d, F.normalize, autograd), in any dtype and on any device, with the same state_dict keys and shapes as the modules.  They
are written from the formulas: sparse sums instead of the reference's dense masks and Python loops.  tests/test_gin_sage_host.py pins
them to the reference's recorded results (tests/golden/gin_sage_uci.npz); the GPU tests then use them as their reference, because the
reference tree is not present where they run, and for the one case the reference cannot run (GIN sum / average with learn_eps).
Dropout is an explicit argument: keep masks, which the GPU tests compute with the host model of the draw (_gcrn_ref.keep_mask)."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _egcn_ref as E
import _gcrn_ref as R
from conftest import formula_tensor, load_golden

N, T, HID, OUT, DENSE_IN = R.N, R.T, 20, 16, R.DENSE_IN
ADAM_STEPS, LR = 3, 1e-3
# fixture prefix -> (model, input width, constructor arguments)
CASES = {
    "gin_sum": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=False, neighbor_pooling_type="sum")),      # the configs' shape
    "gin_average": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=False, neighbor_pooling_type="average")),
    "gin_max": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=False, neighbor_pooling_type="max")),
    "gin_max_eps": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=True, neighbor_pooling_type="max")),
    "gin_sum_mlp1": ("GIN", N, dict(layer_num=2, mlp_layer_num=1, learn_eps=False, neighbor_pooling_type="sum")),
    "gin_dense": ("GIN", DENSE_IN, dict(layer_num=2, mlp_layer_num=2, learn_eps=False, neighbor_pooling_type="sum")),
    "sage_sum": ("SAGE", N, dict(num_sample=None, pooling_type="sum", gcn=False)),
    "sage_average": ("SAGE", N, dict(num_sample=None, pooling_type="average", gcn=False)),
    "sage_max": ("SAGE", N, dict(num_sample=None, pooling_type="max", gcn=False)),
    "sage_sum_gcn": ("SAGE", N, dict(num_sample=None, pooling_type="sum", gcn=True)),
}
# the cases the reference cannot run (UnboundLocalError): held against the float64 mirror alone
EPS_CASES = {
    "gin_sum_eps": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=True, neighbor_pooling_type="sum")),
    "gin_average_eps": ("GIN", N, dict(layer_num=2, mlp_layer_num=2, learn_eps=True, neighbor_pooling_type="average")),
}


def entries(adj):
    """(rows, cols, vals) of a sparse COO tensor's stored entries in row-major order"""
    adj = adj.coalesce()
    idx = adj.indices()
    return idx[0], idx[1], adj.values()


def with_self(rows, cols, n):
    """the pattern with every node in its own set, as a set: (rows, cols) in row-major order"""
    keys = torch.unique(torch.cat((rows * n + cols, torch.arange(n, device=rows.device) * (n + 1))))
    return torch.div(keys, n, rounding_mode="floor"), keys % n


def pool_sum(h, rows, cols, vals=None):
    g = h[cols] if vals is None else h[cols] * vals[:, None]
    return torch.zeros_like(h).index_add(0, rows, g)


def pool_max(h, rows, cols):
    """the maximum over each row's entries (row-major, columns ascending), zeros for a row without entries; among equal values the
    first entry wins and the gradient goes there alone, as torch.max(h[neighbours], 0) has it on the CPU"""
    n, d = h.shape
    g = h[cols]
    index = rows[:, None].expand(-1, d)
    top = torch.zeros_like(h).scatter_reduce(0, index, g.detach(), "amax", include_self=False)
    hit = g.detach() == top[rows]
    count = hit.to(torch.int64).cumsum(0)
    first_entry = torch.zeros(n, dtype=torch.int64, device=h.device).scatter_reduce(0, rows, torch.arange(rows.numel(), device=h.device), "amin",
                                                                                   include_self=False)
    before = count[first_entry[rows]] - hit[first_entry[rows]].to(torch.int64)       # hits before the row's first entry
    first = hit & ((count - before) == 1)
    return torch.zeros_like(h).index_add(0, rows, g * first.to(h.dtype))


def linear_input(linear, x):
    if x.is_sparse:
        out = torch.sparse.mm(x, linear.weight.t())
        return out if linear.bias is None else out + linear.bias
    return linear(x)


class MlpMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, layer_num, bias=True):
        super().__init__()
        self.layer_num = layer_num
        if layer_num == 1:
            self.linear = nn.Linear(input_dim, output_dim, bias=bias)
        else:
            dims = [input_dim] + [hidden_dim] * (layer_num - 1) + [output_dim]
            self.linears = nn.ModuleList([nn.Linear(dims[k], dims[k + 1], bias=bias) for k in range(layer_num)])
            self.batch_norms = nn.ModuleList([nn.BatchNorm1d(hidden_dim) for _ in range(layer_num - 1)])

    def forward(self, x):
        if self.layer_num == 1:
            return self.linear(x)
        for k in range(self.layer_num - 1):
            x = F.relu(self.batch_norms[k](self.linears[k](x)))
        return self.linears[-1](x)


class GinMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, layer_num, mlp_layer_num, learn_eps, neighbor_pooling_type="sum", dropout=0.5, bias=True):
        super().__init__()
        self.layer_num, self.learn_eps, self.kind, self.dropout = layer_num, learn_eps, neighbor_pooling_type, dropout
        self.eps = nn.Parameter(torch.zeros(layer_num))
        self.linear = nn.Linear(input_dim, hidden_dim)
        outs = [hidden_dim] * (layer_num - 1) + [output_dim]
        self.mlps = nn.ModuleList([MlpMirror(hidden_dim, hidden_dim, o, mlp_layer_num, bias) for o in outs])
        self.batch_norms = nn.ModuleList([nn.BatchNorm1d(o) for o in outs])

    def pool(self, h, rows, cols, vals, layer):
        if self.kind == "max":
            pooled = pool_max(h, rows, cols)
            return pooled + (1 + self.eps[layer]) * h if self.learn_eps else pooled
        pooled = pool_sum(h, rows, cols, vals)
        degree = torch.zeros(h.shape[0], dtype=h.dtype, device=h.device).index_add(0, rows, vals)
        if not self.learn_eps:                                    # the unit diagonal
            pooled, degree = pooled + h, degree + 1
        if self.kind == "average":
            pooled = torch.where(degree[:, None] != 0, pooled / torch.where(degree != 0, degree, torch.ones_like(degree))[:, None],
                                 torch.zeros_like(pooled))
        return pooled + (1 + self.eps[layer]) * h if self.learn_eps else pooled

    def one(self, x, adj, keep=None):
        """keep: None or a list of bool [N, width] masks, one per layer but the last, of the entries dropout keeps"""
        rows, cols, vals = entries(adj)
        h = linear_input(self.linear, x)
        for layer in range(self.layer_num):
            h = F.relu(self.batch_norms[layer](self.mlps[layer](self.pool(h, rows, cols, vals.to(h.dtype), layer))))
            if keep is not None and layer < self.layer_num - 1:
                h = h * keep[layer].to(h.dtype) / (1.0 - self.dropout)
        return h

    def forward(self, x, adj, keep=None):
        if isinstance(x, list):
            return [self.one(x[t], adj[t], None if keep is None else keep[t]) for t in range(len(x))]
        return self.one(x, adj, keep)


class SageLayerMirror(nn.Module):
    def __init__(self, input_dim, output_dim, pooling_type, gcn, bias):
        super().__init__()
        self.kind, self.gcn = pooling_type, gcn
        self.linear = nn.Linear(input_dim if gcn else 2 * input_dim, output_dim, bias=bias)

    def forward(self, h, rows, cols):
        if self.gcn:
            rows, cols = with_self(rows, cols, h.shape[0])
        if self.kind == "max":
            neigh = pool_max(h, rows, cols)
        else:
            neigh = pool_sum(h, rows, cols)
            if self.kind == "average":
                count = torch.bincount(rows, minlength=h.shape[0]).clamp(min=1)
                neigh = neigh / count.to(h.dtype)[:, None]
        combined = neigh if self.gcn else torch.cat((h, neigh), dim=1)
        return F.normalize(F.relu(self.linear(combined)), p=2)


class SageMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, num_sample=10, pooling_type="sum", gcn=False, dropout=0.5, bias=True):
        super().__init__()
        assert num_sample is None
        self.dropout = dropout
        self.linear = nn.Linear(input_dim, hidden_dim, bias=bias)
        self.sage1 = SageLayerMirror(hidden_dim, hidden_dim, pooling_type, gcn, bias)
        self.sage2 = SageLayerMirror(hidden_dim, output_dim, pooling_type, gcn, bias)

    def one(self, x, adj, keep=None):
        """keep: None or the bool [N, hidden] mask of the entries of layer 1's output that dropout keeps"""
        rows, cols, _ = entries(adj)
        h = self.sage1(linear_input(self.linear, x), rows, cols)
        if keep is not None:
            h = h * keep.to(h.dtype) / (1.0 - self.dropout)
        return self.sage2(h, rows, cols)

    def forward(self, x, adj, keep=None):
        if isinstance(x, list):
            return [self.one(x[t], adj[t], None if keep is None else keep[t]) for t in range(len(x))]
        return self.one(x, adj, keep)


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("gin_sage_uci.npz")


def spec(case):
    return CASES[case] if case in CASES else EPS_CASES[case]


def build(case, gin_cls, sage_cls, dropout=0.0):
    kind, in_dim, kwargs = spec(case)
    if kind == "GIN":
        return gin_cls(in_dim, HID, OUT, dropout=dropout, **kwargs)
    return sage_cls(in_dim, HID, OUT, dropout=dropout, **kwargs)


def features(case, dtype=torch.float32, device="cpu"):
    return R.features("gcn_dense" if spec(case)[1] == DENSE_IN else "gcn", dtype, device)


def raw_csr(t, dtype=np.float64):
    """the raw (symmetric, weighted, no diagonal) adjacency of UCI snapshot t: get_date_adj_list(normalize=False)"""
    return E.snapshot_csr(t, with_eye=False).astype(dtype)


def adjacency(dtype=torch.float32, device="cpu"):
    return [E.sparse_tensor(raw_csr(t), dtype, device) for t in range(T)]


def surrogate_weights(dtype=torch.float32, device="cpu"):
    return [torch.from_numpy(formula_tensor((N, OUT), 0.05 + 0.01 * t, 1.0 + t)).to(dtype).to(device) for t in range(T)]


def adam_losses(model, forward, weights):
    return E.adam_losses(model, lambda: list(forward()), weights, ADAM_STEPS, LR)


def buffers(model):
    """the BatchNorm running buffers by state_dict key"""
    return {k: v.detach().clone() for k, v in model.state_dict().items() if "running_" in k or "num_batches" in k}
