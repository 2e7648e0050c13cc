"""The project's own mirror of the DynRNN / DynAERNN passes in stock torch ops, in any dtype and on any device: the LSTM step of
ctgcn_lstmcell.hip and a whole layer in their dense definition (the explicit cell equations, not nn.LSTM), the two models with the
reference's state_dict keys, and their loss (tests/_dyngem_ref.py's dense rows, reconstruction term and regulariser).
tests/test_dynrnn_host.py pins it to the reference's recorded results (tests/golden/dynrnn_uci.npz); the GPU tests then use it as their
reference, because the reference tree is not present where they run."""
import math

import numpy as np
import torch
from torch import nn

import _dyngem_ref as D
from conftest import load_golden

N = D.N
UNITS, RNN_UNITS, OUT = D.UNITS, [24], D.OUT
LOOK_BACK = 3
SNAPSHOTS = (0, 1, 2, 3, 4)
BATCH = D.BATCH
BETA, NU1, NU2 = 5.0, 1e-4, 1e-4
METHODS = ("dynrnn", "dynaernn")


# ------------------------------------------------------------------------------------------------ the step and the layer, densely
def cell_fwd(gi, gh=None, bias=None, c_prev=None):
    """(h, c, activated gates [B, 4 H]) of one step; gate order i, f, g, o"""
    z = gi
    if gh is not None:
        z = z + gh
    if bias is not None:
        z = z + bias
    zi, zf, zg, zo = z.chunk(4, dim=1)
    i, f, g, o = torch.sigmoid(zi), torch.sigmoid(zf), torch.tanh(zg), torch.sigmoid(zo)
    c = i * g if c_prev is None else f * c_prev + i * g
    return o * torch.tanh(c), c, torch.cat((i, f, g, o), dim=1)


def cell_bwd(gates, c, c_prev=None, dh_out=None, dh_rec=None, dc_next=None):
    """(dgates [B, 4 H] with respect to the pre-activations, dc_prev) of one step, written out"""
    i, f, g, o = gates.chunk(4, dim=1)
    tc = torch.tanh(c)
    dh = torch.zeros_like(c)
    if dh_out is not None:
        dh = dh + dh_out
    if dh_rec is not None:
        dh = dh + dh_rec
    dc = dh * o * (1 - tc * tc)
    if dc_next is not None:
        dc = dc + dc_next
    cp = torch.zeros_like(c) if c_prev is None else c_prev
    return torch.cat((dc * g * i * (1 - i), dc * cp * f * (1 - f), dc * i * (1 - g * g), dh * tc * o * (1 - o)), dim=1), dc * f


def lstm_dense(x, w_ih, w_hh, b_ih=None, b_hh=None, gi=None):
    """h_seq [B, L, H] of a batch_first single-layer LSTM with zero initial state; gi [B, L, 4 H] replaces x w_ihᵀ + b_ih"""
    if gi is None:
        gi = x @ w_ih.t()
        if b_ih is not None:
            gi = gi + b_ih
    h = c = None
    out = []
    for t in range(gi.shape[1]):
        h, c, _ = cell_fwd(gi[:, t], None if h is None else h @ w_hh.t(), b_hh, c)
        out.append(h)
    return torch.stack(out, dim=1)


# ------------------------------------------------------------------------------------------------ the models
class LstmMirror(nn.Module):
    """the parameters of a single-layer nn.LSTM under its names, the forward as the cell equations"""

    def __init__(self, input_dim, hidden, bias=True):
        super().__init__()
        bound = 1.0 / math.sqrt(hidden)
        shapes = [("weight_ih_l0", (4 * hidden, input_dim)), ("weight_hh_l0", (4 * hidden, hidden))]
        if bias:
            shapes += [("bias_ih_l0", (4 * hidden,)), ("bias_hh_l0", (4 * hidden,))]
        for name, shape in shapes:
            setattr(self, name, nn.Parameter(torch.empty(shape).uniform_(-bound, bound)))
        self.has_bias = bias

    def forward(self, x):
        return lstm_dense(x, self.weight_ih_l0, self.weight_hh_l0, self.bias_ih_l0 if self.has_bias else None,
                          self.bias_hh_l0 if self.has_bias else None)


class MllstmMirror(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, bias=True):
        super().__init__()
        dims = [input_dim] + list(n_units) + [output_dim]
        self.layer_list = nn.ModuleList([LstmMirror(a, b, bias) for a, b in zip(dims[:-1], dims[1:])])

    def forward(self, x):
        for layer in self.layer_list:
            x = layer(x)
        return x, x[:, -1, :]


class RnnMirror(nn.Module):
    """DynRNN: the decoder reads the encoder's output sequence; the prediction is its last step"""

    def __init__(self, input_dim, output_dim, n_units, bias=True):
        super().__init__()
        self.encoder = MllstmMirror(input_dim, output_dim, n_units, bias)
        self.decoder = MllstmMirror(output_dim, input_dim, n_units[::-1], bias)

    def forward(self, x):
        output, hx = self.encoder(x)
        return hx, self.decoder(output)[1]


class MtmlpMirror(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, look_back, bias=True):
        super().__init__()
        self.layer_list = nn.ModuleList([D.MlpMirror(input_dim, output_dim, n_units, bias) for _ in range(look_back)])

    def forward(self, x):
        return torch.stack([mlp(x[:, t]) for t, mlp in enumerate(self.layer_list)], dim=1)


class AernnMirror(nn.Module):
    """DynAERNN: one MLP per step, an LSTM stack over their outputs, DynAE's decoder on the last hidden state"""

    def __init__(self, input_dim, output_dim, look_back, ae_units, rnn_units, bias=True):
        super().__init__()
        self.ae_encoder = MtmlpMirror(input_dim, output_dim, ae_units, look_back, bias)
        self.rnn_encoder = MllstmMirror(output_dim, output_dim, rnn_units, bias)
        self.decoder = D.MlpMirror(output_dim, input_dim, ae_units[::-1], bias)

    def forward(self, x):
        hx = self.rnn_encoder(self.ae_encoder(x))[1]
        return hx, self.decoder(hx)


def mirror(method, bias=True):
    if method == "dynrnn":
        return RnnMirror(N, OUT, UNITS, bias)
    return AernnMirror(N, OUT, LOOK_BACK, UNITS, RNN_UNITS, bias)


def model_loss(model, x_pre, x_cur):
    """(loss, hx, prediction): the reference's DynGraph2VecLoss on the model's prediction (DynRNN's has no ReLU, DynAERNN's has had it)"""
    return D.dynae_loss(model, x_pre, x_cur, BETA, NU1, NU2)


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("dynrnn_uci.npz")


def window():
    return [D.weighted_snapshot(t) for t in SNAPSHOTS]


def batch_rows(g):
    """(idx [B, look_back], tgt [B]) stacked row ids of the fixture's records"""
    graph, node = g["graph"].astype(np.int64), g["node"].astype(np.int64)
    idx = np.stack([(graph + s) * N + node for s in range(LOOK_BACK)], axis=1)
    return idx, (graph + LOOK_BACK) * N + node


def stored(g, key):
    """(values, their positions in the flattened tensor or None for all, the tensor's largest magnitude)"""
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def dense_share(what, got, ref64, ref32, floor):
    """the same rule for an operation: the yardstick is the float32 evaluation of the dense definition against its float64 one"""
    ref64 = ref64.detach().double()
    top = max(float(ref64.abs().max()), 1e-30)
    err = float((got.detach().double() - ref64).abs().max()) / top
    yard = float((ref32.detach().double() - ref64).abs().max()) / top
    used = err / max(4 * yard, floor)
    print("  [tol] %-58s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (what, err, used, yard, floor))
    return used


def record_parity(part, used):
    """with CTGCN_PARITY_OUT=<dir>: keep the shares of the tolerance a test used as <dir>/dynrnn_part_<part>.json, and join the parts
    kept so far into <dir>/dynrnn_parity_errors.json (the copy under profiles/ is such a file)"""
    import glob
    import json
    import os
    out_dir = os.environ.get("CTGCN_PARITY_OUT")
    if not out_dir:
        return
    with open(os.path.join(out_dir, "dynrnn_part_%s.json" % part), "w") as fp:
        json.dump(used, fp, indent=1, sort_keys=True)
    cases = {}
    for f in sorted(glob.glob(os.path.join(out_dir, "dynrnn_part_*.json"))):
        with open(f) as fp:
            cases[os.path.basename(f)[len("dynrnn_part_"):-len(".json")]] = json.load(fp)
    joined = {"rule": "share used of max(4 x yardstick, floor) of the largest reference magnitude; floor 2e-6 for outputs and losses, 1e-5 for "
                      "gradients; the yardstick is the reference's own fp32-vs-fp64 error (models) or that of the dense definition (ops)",
              "fixture": "tests/golden/dynrnn_uci.npz", "largest": max(v for c in cases.values() for v in c.values()), "cases": cases}
    with open(os.path.join(out_dir, "dynrnn_parity_errors.json"), "w") as fp:
        json.dump(joined, fp, indent=1, sort_keys=True)


def share_used(g, key, got, yard, floor):
    """error over the largest reference magnitude, as a share of max(4 x yardstick, floor): tests/test_gpu_vgrnn.py's rule"""
    ref, pick, top = stored(g, key)
    got = got.detach().double().cpu().numpy().reshape(-1)
    err = float(np.abs((got if pick is None else got[pick]) - ref).max() / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-58s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (key, err, used, float(yard), floor))
    return used
