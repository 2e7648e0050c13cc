"""The project's own mirror of ctgcn_amd.baseline.gat in stock torch ops (index gather, scatter / index_add, autograd), in any dtype and
on any device, with the same state_dict keys and shapes as the module.  tests/test_gat_host.py pins it to the reference's recorded
results (tests/golden/gat_uci.npz); the GPU tests then use it as their reference, because the reference tree is not present where
they run.  The softmax is shifted by the row maximum like the kernels' (shifted=False gives the reference's unshifted form, for the
test that shows where that one breaks).  Dropout is an explicit argument: keep masks, which the GPU tests compute with the host models
of the two draws below (built on _gcrn_ref.u01: ctgcn_rng.h in uint64 arithmetic)."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _gcrn_ref as R
from conftest import load_golden

N, T, DENSE_IN = R.N, R.T, R.DENSE_IN
ADAM_STEPS, LR, ALPHA = 3, 1e-3, 0.2
# fixture prefix -> (input width, heads, width of a head, output width, learning type)
CASES = {
    "gat_uneg": (N, 8, 8, 16, "U-neg"),
    "gat_cfg": (N, 1, 20, 16, "S-node"),          # the configs' head count
    "gat_dense": (DENSE_IN, 3, 6, 128, "S-node"), # d = 18: head boundaries inside a float4, the scalar path
}
_M64 = 0xFFFFFFFFFFFFFFFF


def attention(S, a_src, a_dst, rows, cols, heads, alpha=ALPHA, keep=None, p_att=0.0, shifted=True):
    """(Y [n, d], m [n, heads], Z [n, heads]) of one attention layer over the entries (rows[e], cols[e]); keep: None or bool
    [E, heads], the entries attention dropout keeps (scaled by 1 / (1 - p_att)).  A row without entries: zeros, m = Z = 0."""
    n, d = S.shape
    Sh = S.reshape(n, heads, d // heads)
    u, v = (Sh * a_src).sum(-1), (Sh * a_dst).sum(-1)
    l = -F.leaky_relu(u[rows] + v[cols], alpha)                                   # [E, heads]
    m = torch.zeros(n, heads, dtype=S.dtype, device=S.device)
    if shifted:
        m = m.scatter_reduce(0, rows[:, None].expand(-1, heads), l.detach(), "amax", include_self=False)
    e = torch.exp(l - m[rows])
    Z = torch.zeros(n, heads, dtype=S.dtype, device=S.device).index_add(0, rows, e)
    w = e if keep is None else e * keep.to(S.dtype) / (1.0 - p_att)
    Y = torch.zeros_like(Sh).index_add(0, rows, w[:, :, None] * Sh[cols])
    if shifted:
        Y = Y / torch.where(Z > 0, Z, torch.ones_like(Z))[:, :, None]
    else:
        Y = Y / Z[:, :, None]                                                       # the reference's: 0 / 0 and inf / inf included
    return Y.reshape(n, d), m, Z


def epilogue(Y, epi, keep=None, p_feat=0.0):
    """epi 0 none, 1 ELU, 2 ELU then feature dropout with the bool [n, d] keep mask (None: nothing dropped)"""
    if epi == 0:
        return Y
    out = F.elu(Y)
    if epi == 2 and keep is not None:
        out = out * keep.to(Y.dtype) / (1.0 - p_feat)
    return out


def entries(adj):
    """(rows, cols) int64 of a sparse COO tensor's stored entries in row-major order, or of a scipy matrix"""
    if isinstance(adj, torch.Tensor):
        idx = adj.coalesce().indices()
        return idx[0], idx[1]
    coo = adj.tocsr().tocoo()
    return torch.from_numpy(coo.row.astype(np.int64)), torch.from_numpy(coo.col.astype(np.int64))


class GatLayerMirror(nn.Module):
    def __init__(self, in_features, out_features):
        super().__init__()
        self.W = nn.Parameter(torch.zeros(in_features, out_features))
        self.a = nn.Parameter(torch.zeros(1, 2 * out_features))


class GatMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, dropout=0.6, alpha=ALPHA, head_num=8, learning_type="U-neg"):
        super().__init__()
        self.dropout, self.alpha, self.head_num, self.hidden_dim, self.output_dim = dropout, alpha, head_num, hidden_dim, output_dim
        self.learning_type = learning_type
        for i in range(head_num):
            self.add_module("attention_%d" % i, GatLayerMirror(input_dim, hidden_dim))
        self.out_att = GatLayerMirror(hidden_dim * head_num, output_dim)

    def one(self, x, adj, keep=None):
        """keep: None or {"att0": [E, heads], "feat": [N, hidden * heads], "att1": [E, 1]} bool masks of what dropout keeps"""
        rows, cols = entries(adj)
        heads = [getattr(self, "attention_%d" % i) for i in range(self.head_num)]
        W = torch.cat([h.W for h in heads], dim=1)
        a_src = torch.cat([h.a[:, :self.hidden_dim] for h in heads], dim=0)
        a_dst = torch.cat([h.a[:, self.hidden_dim:] for h in heads], dim=0)
        p = self.dropout
        k = keep or {}
        S = torch.sparse.mm(x, W) if x.is_sparse else x @ W
        h = epilogue(attention(S, a_src, a_dst, rows, cols, self.head_num, self.alpha, k.get("att0"), p)[0], 2, k.get("feat"), p)
        o = self.out_att
        out = F.elu(attention(h @ o.W, o.a[:, :self.output_dim], o.a[:, self.output_dim:], rows, cols, 1, self.alpha, k.get("att1"), p)[0])
        return F.log_softmax(out, dim=1) if self.learning_type == "U-neg" else out

    def forward(self, x, adj, keep=None):
        if isinstance(x, list):
            return [self.one(x[t], adj[t], None if keep is None else keep[t]) for t in range(len(x))]
        return self.one(x, adj, keep)


# ------------------------------------------------------------------------------------------------ host models of the two draws
def att_keep(key, rows, cols, heads, p):
    """bool [E, heads]: entry (rows[e], cols[e]) of head h survives attention dropout under `key` iff u01(key + h, i, j) >= p"""
    rows, cols = np.asarray(rows, dtype=np.uint64), np.asarray(cols, dtype=np.uint64)
    return np.stack([R.u01((int(key) + h) & _M64, rows, cols) >= p for h in range(heads)], axis=1)


def feat_keep(fkey, n, d, p):
    """bool [n, d]: entry (i, c) survives feature dropout under `fkey` iff u01(fkey, i, c) >= p"""
    return R.keep_mask(fkey, n, d, p)


def model_keep(base, t, rows, cols, heads, hidden, p):
    """the masks of snapshot t of a training-mode forward of ctgcn_amd.GAT under the base key `base`, as GatMirror.one takes them"""
    return {"att0": torch.from_numpy(att_keep(base + 4096 * t, rows, cols, heads, p)),
            "att1": torch.from_numpy(att_keep(base + 4096 * t + 2048, rows, cols, 1, p)),
            "feat": torch.from_numpy(feat_keep(base + 2 ** 40 + t, N, heads * hidden, p))}


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("gat_uci.npz")


def build(case, cls, dropout=0.0):
    in_dim, heads, hid, out_dim, learning_type = CASES[case]
    return cls(in_dim, hid, out_dim, dropout=dropout, alpha=ALPHA, head_num=heads, learning_type=learning_type)


def features(case, dtype=torch.float32, device="cpu"):
    return R.features("gcn_dense" if case == "gat_dense" else "gcn", dtype, device)


def adjacency(dtype=torch.float32, device="cpu"):
    return R.adjacency(dtype, device)


def surrogate_weights(case, dtype=torch.float32, device="cpu"):
    from conftest import formula_tensor
    out_dim = CASES[case][3]
    return [torch.from_numpy(formula_tensor((N, out_dim), 0.05 + 0.01 * t, 1.0 + t)).to(dtype).to(device) for t in range(T)]


def adam_losses(model, forward, weights):
    return R.adam_losses(model, forward, weights)
