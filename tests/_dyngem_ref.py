"""The project's own mirror of the DynGEM / DynAE passes in stock torch ops, in any dtype and on any device: the three operations of
ctgcn_dyngem.hip in their dense definition (dense adjacency rows times a matrix; the reference's sum(((pred − x) penalty)²); an
index_add), the two auto-encoders with the reference's state_dict keys, and their losses.  It does not reuse the kernels' rewrite (no
gather, no correction at stored entries).  tests/test_dyngem_host.py pins it to the reference's recorded results
(tests/golden/dyngem_uci.npz); the GPU tests then use it as their reference, because the reference tree is not present where they run."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _egcn_ref as E
from conftest import load_golden

N = E.N
UNITS, OUT = [24, 16], 8
LOOK_BACK = 2
BATCH = 64
ADAM_STEPS, LR = 3, 1e-3
DYNGEM = dict(alpha=0.5, beta=10.0, nu1=1e-4, nu2=1e-4, snapshot=1)
DYNAE = dict(beta=5.0, nu1=1e-4, nu2=1e-4, snapshots=(0, 1, 2))


# ------------------------------------------------------------------------------------------------ the operations, densely
def dense_rows(csr, idx, dtype=torch.float64, device="cpu"):
    """rows idx [B] or [B, L] of a scipy CSR (the stacked window) as a dense [B, L, N] tensor; -1 is a zero row"""
    idx = np.asarray(idx, dtype=np.int64)
    idx = idx[:, None] if idx.ndim == 1 else idx
    flat = idx.reshape(-1)
    out = csr.tocsr()[np.maximum(flat, 0)].toarray().astype(np.float64)
    out[flat < 0] = 0.0
    return torch.from_numpy(out.reshape(idx.shape + (csr.shape[1],))).to(dtype).to(device)


def rowsel_conv(S, x, bias=None, relu=False, col_stride=0):
    """Y = epi(bias + Σ_s x[:, s] @ S[s col_stride : s col_stride + N]) for dense rows x [B, L, N]"""
    n = x.shape[2]
    y = sum(x[:, s] @ S[s * col_stride:s * col_stride + n] for s in range(x.shape[1]))
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


def bucket(G, idx_s, rows):
    """out[r] = Σ G[b] over the positions b with idx_s[b] = r"""
    idx_s = torch.as_tensor(np.asarray(idx_s, dtype=np.int64), device=G.device)
    keep = idx_s >= 0
    return torch.zeros(rows, G.shape[1], dtype=G.dtype, device=G.device).index_add(0, idx_s[keep], G[keep])


def wrecon_loss(Z, x, beta, div=None, scale=1.0, relu=True):
    """scale Σ_b Σ_j ((p − x) pen)² / div_b with pen = beta where x != 0, 1 elsewhere: the reference's expression on dense tensors"""
    p = torch.relu(Z) if relu else Z
    pen = torch.ones_like(x)
    pen[x != 0] = beta
    per_row = torch.sum(torch.square((p - x) * pen), dim=1)
    if div is not None:
        per_row = per_row / div
    return scale * per_row.sum()


# ------------------------------------------------------------------------------------------------ the models and their losses
class MlpMirror(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, bias=True):
        super().__init__()
        dims = [input_dim] + list(n_units) + [output_dim]
        self.layer_list = nn.ModuleList([nn.Linear(a, b, bias=bias) for a, b in zip(dims[:-1], dims[1:])])

    def forward(self, x):
        for layer in self.layer_list:
            x = F.relu(layer(x))
        return x


class AeMirror(nn.Module):
    """DynGEM (look_back 1) and DynAE: encoder over [B, look_back N] dense rows, decoder back to [B, N]"""

    def __init__(self, input_dim, output_dim, n_units, look_back=1, bias=True):
        super().__init__()
        self.encoder = MlpMirror(input_dim * look_back, output_dim, n_units, bias)
        self.decoder = MlpMirror(output_dim, input_dim, n_units[::-1], bias)

    def forward(self, x):
        hx = self.encoder(x)
        return hx, self.decoder(hx)


def regularization(model, nu1, nu2):
    weights = [p for name, p in model.named_parameters() if "weight" in name]
    if nu1 == 0 and nu2 == 0:
        return torch.zeros(1, dtype=weights[0].dtype, device=weights[0].device)
    l1 = sum(p.abs().sum() for p in weights) if nu1 > 0 else 0
    l2 = sum(p.pow(2).sum().sqrt() for p in weights) if nu2 > 0 else 0
    return nu1 * l1 / len(weights) + nu2 * l2 / len(weights)


def dyngem_loss(model, xi, xj, values, alpha, beta, nu1, nu2):
    """(loss, hx of the i side, prediction of the i side): the reference's DynGEMLoss, its [B] x [B, 1] broadcast written as the
    product of two means"""
    hx_i, pi = model(xi)
    hx_j, pj = model(xj)
    x_loss = wrecon_loss(pi, xi, beta, xi.sum(1), 1.0 / xi.shape[0], relu=False) + wrecon_loss(pj, xj, beta, xj.sum(1), 1.0 / xj.shape[0], relu=False)
    hx_loss = (hx_i - hx_j).pow(2).sum(1).mean() * values.mean()
    return x_loss + alpha * hx_loss + regularization(model, nu1, nu2), hx_i, pi


def dynae_loss(model, x_pre, x_cur, beta, nu1, nu2):
    hx, pred = model(x_pre)
    return wrecon_loss(pred, x_cur, beta, None, 1.0 / x_cur.shape[0], relu=False) + regularization(model, nu1, nu2), hx, pred


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("dyngem_uci.npz")


def weighted_snapshot(t):
    """UCI snapshot t with entry (i, j) given the weight 1 + (i + j) mod 3: UCI's stored weights are all 1, which would hide a
    confusion of weight, count and degree"""
    import scipy.sparse as sp
    m = E.snapshot_csr(t, with_eye=False).tocoo()
    w = 1.0 + ((m.row.astype(np.int64) + m.col.astype(np.int64)) % 3)
    out = sp.csr_matrix((w.astype(np.float64), (m.row, m.col)), shape=m.shape)
    out.sort_indices()
    return out


def dyngem_window():
    return [weighted_snapshot(DYNGEM["snapshot"])]


def dynae_window():
    return [weighted_snapshot(t) for t in DYNAE["snapshots"]]


def stacked(mats):
    import scipy.sparse as sp
    return sp.vstack(mats, format="csr")


def dynae_rows(g):
    """(idx [B, look_back], tgt [B]) stacked row ids of the fixture's records"""
    graph, node = g["dynae_graph"].astype(np.int64), g["dynae_node"].astype(np.int64)
    idx = np.stack([(graph + s) * N + node for s in range(LOOK_BACK)], axis=1)
    return idx, (graph + LOOK_BACK) * N + node


def adam_run(model, forward_loss, steps=ADAM_STEPS, lr=LR):
    """losses of `steps` Adam steps; forward_loss() -> (loss, hx, pred).  Also the first step's embedding, prediction and gradients."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses, first = [], None
    for _ in range(steps):
        opt.zero_grad()
        loss, hx, pred = forward_loss()
        loss = loss.reshape(())
        loss.backward()
        if first is None:
            first = (hx.detach().clone(), pred.detach().clone(),
                     {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()})
        losses.append(float(loss.detach()))
        opt.step()
    return losses, first

