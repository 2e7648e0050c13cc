"""The project's own mirror of ctgcn_amd.baseline.egcn in stock torch ops (torch.sparse.mm, F.rrelu, autograd), in any dtype and on
any device.  tests/test_egcn_host.py pins it to the reference's recorded results (tests/golden/egcn_uci.npz); the GPU tests then use
it as their reference, because the reference tree is not present where they run.  Same state_dict keys and shapes as the module."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

from conftest import formula_tensor, load_golden

N, IN, HID, OUT, T = 1899, 24, 16, 16, 3
CASES = ("egcnh", "egcno", "onehot")          # fixture prefixes: EGCNH and EGCNO on formula features, EGCNH on one-hot degree features
ADAM_STEPS, LR = 3, 1e-3


class Gate(nn.Module):
    def __init__(self, rows, cols, act):
        super().__init__()
        self.act = act
        self.W = nn.Parameter(torch.zeros(rows, rows))
        self.U = nn.Parameter(torch.zeros(rows, rows))
        self.bias = nn.Parameter(torch.zeros(rows, cols))

    def forward(self, x, h):
        return self.act(self.W @ x + self.U @ h + self.bias)


class Scorer(nn.Module):
    def __init__(self, feats, k):
        super().__init__()
        self.scorer = nn.Parameter(torch.zeros(feats, 1))
        self.k = k

    def forward(self, x):
        scores = (x @ self.scorer / self.scorer.norm()).view(-1)
        idx = scores.topk(self.k).indices
        return (x[idx] * torch.tanh(scores[idx]).view(-1, 1)).t()


class Cell(nn.Module):
    def __init__(self, rows, cols, kind):
        super().__init__()
        self.kind = kind
        self.update, self.reset, self.htilda = Gate(rows, cols, torch.sigmoid), Gate(rows, cols, torch.sigmoid), Gate(rows, cols, torch.tanh)
        self.choose_topk = Scorer(rows, cols)

    def forward(self, q, x):
        z = q if self.kind == "EGCNO" else self.choose_topk(x)
        u, r = self.update(z, q), self.reset(z, q)
        return (1 - u) * q + u * self.htilda(z, r * q)


class Layer(nn.Module):
    def __init__(self, rows, cols, kind):
        super().__init__()
        self.evolve_weights = Cell(rows, cols, kind)
        self.GCN_init_weights = nn.Parameter(torch.zeros(rows, cols))

    def forward(self, adjs, xs):
        q, out = self.GCN_init_weights, []
        for a, x in zip(adjs, xs):
            q = self.evolve_weights(q, x)
            out.append(F.rrelu(torch.sparse.mm(a, x @ q)))
        return out


class EgcnMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, egcn_type="EGCNH"):
        super().__init__()
        self.GRCU_layers = nn.ModuleList([Layer(input_dim, hidden_dim, egcn_type), Layer(hidden_dim, output_dim, egcn_type)])

    def forward(self, xs, adjs):
        xs = [x.to_dense() if x.is_sparse else x for x in xs]
        for layer in self.GRCU_layers:
            xs = layer(adjs, xs)
        return xs


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("egcn_uci.npz")


def snapshot_csr(t, with_eye=True):
    """scipy CSR float64 of UCI snapshot t (+ I), sorted indices: the matrix the reference normalises"""
    import scipy.sparse as sp
    from ctgcn_amd.utils import symmetric_csr_from_rows
    s = load_golden("uci_snapshots.npz")
    m = symmetric_csr_from_rows(s["t%d_src" % t], s["t%d_dst" % t], s["t%d_w" % t], N)
    if with_eye:
        m = (m + sp.eye(N)).tocsr()
    m.sort_indices()
    return m


def normalized_csr(g, t, row_norm=False, dtype=np.float64):
    """the reference's normalised matrix of snapshot t from the fixture's stored values (float32 after its .float())"""
    import scipy.sparse as sp
    m = snapshot_csr(t)
    return sp.csr_matrix((g["norm%d_t%d" % (int(row_norm), t)].astype(dtype), m.indices, m.indptr), shape=m.shape)


def sparse_tensor(csr, dtype, device="cpu"):
    coo = csr.tocoo()
    idx = torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64))
    return torch.sparse_coo_tensor(idx, torch.from_numpy(coo.data).to(dtype), torch.Size(coo.shape)).to(device)


def features(case, g, dtype=torch.float32, device="cpu"):
    if case != "onehot":
        return [torch.from_numpy(formula_tensor((N, IN), 0.07 + 0.02 * t, 0.4 * t)).to(dtype).to(device) for t in range(T)]
    width = int(g["onehot_width"])
    out = []
    for t in range(T):
        idx = torch.from_numpy(np.vstack((np.arange(N), g["onehot_deg_t%d" % t])).astype(np.int64))
        out.append(torch.sparse_coo_tensor(idx, torch.ones(N, dtype=dtype), torch.Size((N, width))).to(device))
    return out


def input_dim(case, g):
    return int(g["onehot_width"]) if case == "onehot" else IN


def egcn_type(case):
    return "EGCNO" if case == "egcno" else "EGCNH"


def surrogate_weights(dtype=torch.float32, device="cpu"):
    return [torch.from_numpy(formula_tensor((N, OUT), 0.05 + 0.01 * t, 1.0 + t)).to(dtype).to(device) for t in range(T)]


def surrogate(outs, weights):
    return sum((o * c).sum() for o, c in zip(outs, weights))


def adam_losses(model, forward, weights, steps=ADAM_STEPS, lr=LR):
    """losses of `steps` Adam steps on the surrogate; forward() -> outputs of the current weights.  Also returns the first outputs/grads."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses, first = [], None
    for _ in range(steps):
        opt.zero_grad()
        outs = forward()
        loss = surrogate(outs, weights)
        loss.backward()
        if first is None:
            first = ([o.detach().clone() for o in outs],
                     {k: (p.grad.detach().clone() if p.grad is not None else torch.zeros_like(p)) for k, p in model.named_parameters()})
        losses.append(float(loss.detach()))
        opt.step()
    return losses, first
