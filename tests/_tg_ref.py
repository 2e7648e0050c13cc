"""The comparand of ctgcn_amd.baseline.tg: PyG 1.6.0's GCNConv, GATConv, SAGEConv and GINConv and the reference's four Tg models written
out edge by edge in stock torch ops (index_select, index_add, autograd), generic in dtype and device, with the modules' state_dict keys.
torch_geometric is not installed where the tests run, so the reference's own Tg classes cannot be executed; the formulas are those of
the version its README names.  tests/test_tg_host.py checks the edge-wise forms against dense-matrix ones in float64.  Dropout is an
explicit argument: keep masks, which the GPU tests regenerate from the run's base key."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _egcn_ref as E
from conftest import formula_tensor

N, T = E.N, E.T
ADAM_STEPS, LR, SLOPE = 3, 1e-3, 0.2
KINDS = ("TgGCN", "TgGAT", "TgSAGE", "TgGIN")
FEATURE_DIM, HIDDEN, OUT = 32, 16, 8
LAYER_KEY = 2 ** 32                      # ctgcn_amd.baseline.tg: layer l of snapshot t draws from base + LAYER_KEY l + t

# six nodes: the pair (0 -> 1) twice, node 2 with two loops, node 3 with one, node 4 with none, node 5 isolated
SMALL_N = 6
SMALL_EDGES = np.array([[0, 0, 2, 2, 3, 1, 4, 3, 0], [1, 1, 2, 2, 3, 0, 1, 4, 4]], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ the four layers, edge-wise
def looped_edges(edge_index, n):
    """(src, tgt) of GCNConv's and GATConv's pattern: the non-loop pairs as given, then one loop per node"""
    src, tgt = edge_index[0], edge_index[1]
    keep = src != tgt
    loops = torch.arange(n, dtype=src.dtype, device=src.device)
    return torch.cat((src[keep], loops)), torch.cat((tgt[keep], loops))


def gcn_norm(edge_index, n, dtype):
    """(src, tgt, w): w = deg^-1/2[src] deg^-1/2[tgt], the degree counted on the target side of the looped pattern"""
    src, tgt = looped_edges(edge_index, n)
    deg = torch.zeros(n, dtype=dtype, device=src.device).index_add(0, tgt, torch.ones(src.numel(), dtype=dtype, device=src.device))
    dis = deg.pow(-0.5)
    return src, tgt, dis[src] * dis[tgt]


def gcn_conv(x, weight, bias, edge_index):
    n = x.shape[0]
    src, tgt, w = gcn_norm(edge_index, n, x.dtype)
    S = x @ weight
    out = torch.zeros_like(S).index_add(0, tgt, w[:, None] * S.index_select(0, src))
    return out if bias is None else out + bias


def attention(S, att_l, att_r, src, tgt, heads=1, slope=SLOPE):
    """GATConv after its product over the entries (tgt[e] <- src[e]): att_l on the source's features, att_r on the target's"""
    n, d = S.shape
    Sh = S.reshape(n, heads, d // heads)
    al, ar = (Sh * att_l.reshape(1, heads, -1)).sum(-1), (Sh * att_r.reshape(1, heads, -1)).sum(-1)
    l = F.leaky_relu(ar[tgt] + al[src], slope)
    m = torch.zeros(n, heads, dtype=S.dtype, device=S.device).scatter_reduce(0, tgt[:, None].expand(-1, heads), l.detach(), "amax", include_self=False)
    e = torch.exp(l - m[tgt])
    Z = torch.zeros(n, heads, dtype=S.dtype, device=S.device).index_add(0, tgt, e)
    Y = torch.zeros_like(Sh).index_add(0, tgt, e[:, :, None] * Sh.index_select(0, src))
    return (Y / torch.where(Z > 0, Z, torch.ones_like(Z))[:, :, None]).reshape(n, d)


def gat_conv(x, lin_weight, att_l, att_r, bias, edge_index):
    src, tgt = looped_edges(edge_index, x.shape[0])
    out = attention(x @ lin_weight.t(), att_l, att_r, src, tgt)
    return out if bias is None else out + bias


def sage_conv(x, w_l, b_l, w_r, edge_index):
    src, tgt = edge_index[0], edge_index[1]
    n = x.shape[0]
    cnt = torch.zeros(n, dtype=x.dtype, device=x.device).index_add(0, tgt, torch.ones(src.numel(), dtype=x.dtype, device=x.device))
    mean = torch.zeros_like(x).index_add(0, tgt, x.index_select(0, src)) / cnt.clamp(min=1.0)[:, None]
    out = mean @ w_l.t() + x @ w_r.t()
    return out if b_l is None else out + b_l


def gin_conv(x, weight, bias, eps, edge_index):
    src, tgt = edge_index[0], edge_index[1]
    h = (1.0 + eps) * x + torch.zeros_like(x).index_add(0, tgt, x.index_select(0, src))
    out = h @ weight.t()
    return out if bias is None else out + bias


def tg_conv(S, Tm, self_scale, bias, src, tgt, val):
    """ops.tg_conv before its epilogue: sum_e val[e] S[src[e]] into row tgt[e], plus self_scale T + bias"""
    out = torch.zeros_like(S).index_add(0, tgt, val[:, None] * S.index_select(0, src))
    if Tm is not None:
        out = out + self_scale * Tm
    return out if bias is None else out + bias


def relu_dropout(y, keep=None, p=0.0):
    y = F.relu(y)
    return y if keep is None else y * keep.to(y.dtype) / (1.0 - p)


# ------------------------------------------------------------------------------------------------ dense-matrix forms (float64 checks)
def dense_counts(edge_index, n, looped=False):
    """A[t, s] = how often the pair (s -> t) is stored; looped: loops replaced by exactly one per node"""
    A = torch.zeros(n, n, dtype=torch.float64)
    A.index_put_((edge_index[1], edge_index[0]), torch.ones(edge_index.shape[1], dtype=torch.float64), accumulate=True)
    if looped:
        A = A - torch.diag(torch.diag(A)) + torch.eye(n, dtype=torch.float64)
    return A


def dense_gcn(x, weight, bias, edge_index):
    A = dense_counts(edge_index, x.shape[0], looped=True)
    dis = A.sum(1).pow(-0.5)
    return (dis[:, None] * A * dis[None, :]) @ (x @ weight) + bias


def dense_gat(x, lin_weight, att_l, att_r, bias, edge_index):
    A = dense_counts(edge_index, x.shape[0], looped=True)
    S = x @ lin_weight.t()
    z = (S * att_r.reshape(1, -1)).sum(1)[:, None] + (S * att_l.reshape(1, -1)).sum(1)[None, :]
    w = A * torch.exp(F.leaky_relu(z, SLOPE))
    return (w / w.sum(1, keepdim=True)) @ S + bias


def dense_sage(x, w_l, b_l, w_r, edge_index):
    A = dense_counts(edge_index, x.shape[0])
    return ((A @ x) / A.sum(1).clamp(min=1.0)[:, None]) @ w_l.t() + b_l + x @ w_r.t()


def dense_gin(x, weight, bias, eps, edge_index):
    return ((1.0 + eps) * x + dense_counts(edge_index, x.shape[0]) @ x) @ weight.t() + bias


# ------------------------------------------------------------------------------------------------ the four models
class ConvMirror(nn.Module):
    def __init__(self, kind, in_dim, out_dim, bias=True, nn_module=None):
        super().__init__()
        self.kind = kind
        if kind == "TgGCN":
            self.weight = nn.Parameter(torch.zeros(in_dim, out_dim))
        elif kind == "TgGAT":
            self.lin_l = nn.Linear(in_dim, out_dim, bias=False)
            self.lin_r = self.lin_l
            self.att_l = nn.Parameter(torch.zeros(1, 1, out_dim))
            self.att_r = nn.Parameter(torch.zeros(1, 1, out_dim))
        elif kind == "TgSAGE":
            self.lin_l = nn.Linear(in_dim, out_dim, bias=bias)
            self.lin_r = nn.Linear(in_dim, out_dim, bias=False)
        else:
            self.nn = nn_module
            self.register_buffer("eps", torch.Tensor([0.0]))
        if kind in ("TgGCN", "TgGAT"):
            self.bias = nn.Parameter(torch.zeros(out_dim)) if bias else None

    def forward(self, x, edge_index):
        if self.kind == "TgGCN":
            return gcn_conv(x, self.weight, self.bias, edge_index)
        if self.kind == "TgGAT":
            return gat_conv(x, self.lin_l.weight, self.att_l, self.att_r, self.bias, edge_index)
        if self.kind == "TgSAGE":
            return sage_conv(x, self.lin_l.weight, self.lin_l.bias, self.lin_r.weight, edge_index)
        return gin_conv(x, self.nn.weight, self.nn.bias, self.eps, edge_index)


class TgMirror(nn.Module):
    def __init__(self, kind, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True):
        super().__init__()
        self.kind, self.feature_pre, self.layer_num, self.dropout = kind, feature_pre, layer_num, dropout
        if feature_pre:
            self.linear_pre = nn.Linear(input_dim, feature_dim, bias=bias)
        dims = [(feature_dim if feature_pre else input_dim, hidden_dim)] + [(hidden_dim, hidden_dim)] * (layer_num - 2) + [(hidden_dim, output_dim)]
        if kind == "TgGIN":
            self.conv_first_nn = nn.Linear(*dims[0], bias=bias)
            self.conv_first = ConvMirror(kind, *dims[0], nn_module=self.conv_first_nn)
            self.conv_hidden_nn = nn.ModuleList([nn.Linear(*d, bias=bias) for d in dims[1:-1]])
            self.conv_hidden = nn.ModuleList([ConvMirror(kind, *d, nn_module=m) for d, m in zip(dims[1:-1], self.conv_hidden_nn)])
            self.conv_out_nn = nn.Linear(*dims[-1], bias=bias)
            self.conv_out = ConvMirror(kind, *dims[-1], nn_module=self.conv_out_nn)
        else:
            self.conv_first = ConvMirror(kind, *dims[0], bias=bias)
            self.conv_hidden = nn.ModuleList([ConvMirror(kind, *d, bias=bias) for d in dims[1:-1]])
            self.conv_out = ConvMirror(kind, *dims[-1], bias=bias)

    def one(self, x, edge_index, keep=None):
        """keep: None, or one bool [N, hidden] mask (or None) per ReLU'd layer: what that layer's dropout keeps"""
        if x.is_sparse:
            x = x.to_dense()
        if self.feature_pre:
            x = self.linear_pre(x)
        for l, conv in enumerate([self.conv_first] + list(self.conv_hidden)):
            x = relu_dropout(conv(x, edge_index), None if keep is None else keep[l], self.dropout)
        return self.conv_out(x, edge_index)

    def forward(self, x, edge_index, keep=None):
        if isinstance(x, list):
            return [self.one(x[t], edge_index[t], None if keep is None else keep[t]) for t in range(len(x))]
        return self.one(x, edge_index, keep)


def model_keep(kind, base, t, layer_num, hidden, p, n=N):
    """the masks of snapshot t of a training-mode forward of ctgcn_amd's model under the base key `base`, as TgMirror.one takes them.
    TgGAT discards its hidden layers' dropout, like the reference."""
    import _gcrn_ref as R
    return [torch.from_numpy(R.keep_mask(base + LAYER_KEY * l + t, n, hidden, p)) if (l == 0 or kind != "TgGAT") else None
            for l in range(layer_num - 1)]


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
_edges = {}


def uci_edges(t, device="cpu"):
    """int64 [2, E] edge list of UCI snapshot t as the loader's adj._indices() gives it: both directions of every edge, no loops"""
    if t not in _edges:
        coo = E.snapshot_csr(t, with_eye=False).tocoo()
        _edges[t] = torch.from_numpy(np.vstack((coo.col, coo.row)).astype(np.int64))
    return _edges[t].to(device)


def edge_lists(device="cpu"):
    return [uci_edges(t, device) for t in range(T)]


def identity_features(dtype=torch.float32, device="cpu"):
    import _gcrn_ref as R
    eye = R.identity_features(dtype, device)
    return [eye for _ in range(T)]


def build(kind, cls=None, feature_pre=True, layer_num=2, dropout=0.0, bias=True):
    if cls is None:
        return TgMirror(kind, N, FEATURE_DIM, HIDDEN, OUT, feature_pre=feature_pre, layer_num=layer_num, dropout=dropout, bias=bias)
    return cls(N, FEATURE_DIM, HIDDEN, OUT, feature_pre=feature_pre, layer_num=layer_num, dropout=dropout, bias=bias)


def surrogate_weights(dtype=torch.float32, device="cpu", out_dim=OUT):
    return [torch.from_numpy(formula_tensor((N, out_dim), 0.05 + 0.01 * t, 1.0 + t)).to(dtype).to(device) for t in range(T)]


def surrogate(outs, weights):
    return E.surrogate(outs, weights)


def adam_losses(model, forward, weights):
    """the losses of 3 Adam steps on the surrogate sum_t sum(out_t * C_t) of _gat_ref, with the first outputs and gradients"""
    return E.adam_losses(model, lambda: list(forward()), weights, ADAM_STEPS, LR)


def small_graph():
    return torch.from_numpy(SMALL_EDGES.copy()), SMALL_N


# ------------------------------------------------------------------------------------------------ numpy host model of ops.TgGraph
def host_graph(edge_index, n):
    """{looped: (row_ptr, col, val64), raw: (row_ptr, col, mean64)} of an int64 [2, E] numpy edge index: rows = targets, columns
    ascending, the looped values dis_s dis_t of the fp64 formula, the mean values 1 / (entries of the row)"""
    src, tgt = np.asarray(edge_index[0], dtype=np.int64), np.asarray(edge_index[1], dtype=np.int64)
    order = np.lexsort((src, tgt))
    rs, rt = src[order], tgt[order]
    raw_ptr = np.concatenate(([0], np.cumsum(np.bincount(rt, minlength=n)))).astype(np.int64)
    cnt = np.diff(raw_ptr)
    keep = src != tgt
    ls, lt = np.concatenate((src[keep], np.arange(n))), np.concatenate((tgt[keep], np.arange(n)))
    order = np.lexsort((ls, lt))
    ls, lt = ls[order], lt[order]
    c = np.bincount(lt, minlength=n).astype(np.float64)
    dis = c ** -0.5
    return {"looped": (np.concatenate(([0], np.cumsum(c.astype(np.int64)))), ls, dis[ls] * dis[lt]),
            "raw": (raw_ptr, rs, 1.0 / cnt[rt].astype(np.float64) if rt.size else np.zeros(0))}
