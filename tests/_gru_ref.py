"""The GRU step of ctgcn_grucell.hip and a whole layer in their dense definition, written out by hand in stock torch ops (the explicit
cell equations, not nn.GRU), in any dtype and on any device: the reference of tests/test_gpu_gru_cell.py and
tests/test_gpu_rnn_widths.py.  tests/test_gru_cell_host.py pins it to nn.GRU and to autograd in float64.  Gate order r, z, n."""
import glob
import json
import os

import torch

from _dynrnn_ref import dense_share  # noqa: F401  (the tolerance rule, shared with the LSTM cell's tests)


def cell_fwd(gi, gh=None, b_hh=None, h_prev=None):
    """(h, activated gates r, z, n [B, 3 H], q [B, H]) of one step: q = gh_n + b_hn, n = tanh(gi_n + r q), h = (1 − z) n + z h_prev"""
    H = gi.shape[1] // 3
    a = gi
    if gh is not None:
        a = a + gh
    if b_hh is not None:
        a = a + b_hh
    r, z = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H])
    q = torch.zeros_like(gi[:, 2 * H:])
    if gh is not None:
        q = q + gh[:, 2 * H:]
    if b_hh is not None:
        q = q + b_hh[2 * H:]
    n = torch.tanh(gi[:, 2 * H:] + r * q)
    h = (1 - z) * n
    if h_prev is not None:
        h = h + z * h_prev
    return h, torch.cat((r, z, n), dim=1), q


def cell_bwd(gates, q, h_prev=None, dh_out=None, dh_rec=None):
    """(dgi [B, 3 H], dgh [B, 3 H] with respect to the pre-activations of gi and gh, the direct part dh z of dh_prev), written out"""
    r, z, n = gates.chunk(3, dim=1)
    dh = torch.zeros_like(q)
    if dh_out is not None:
        dh = dh + dh_out
    if dh_rec is not None:
        dh = dh + dh_rec
    hp = torch.zeros_like(q) if h_prev is None else h_prev
    dan = dh * (1 - z) * (1 - n * n)
    daz = dh * (hp - n) * z * (1 - z)
    dar = dan * q * r * (1 - r)
    return torch.cat((dar, daz, dan), dim=1), torch.cat((dar, daz, dan * r), dim=1), dh * z


def gru_dense(x, w_ih, w_hh, b_ih=None, b_hh=None, gi=None, reduce_sum=False):
    """h_seq [B, L, H] (or its sum over the steps) of a batch_first single-layer GRU with zero initial state; gi [B, L, 3 H] replaces
    x w_ihᵀ + b_ih"""
    if gi is None:
        gi = x @ w_ih.t()
        if b_ih is not None:
            gi = gi + b_ih
    h = None
    out = []
    for t in range(gi.shape[1]):
        h = cell_fwd(gi[:, t], None if h is None else h @ w_hh.t(), b_hh, h)[0]
        out.append(h)
    out = torch.stack(out, dim=1)
    return out.sum(dim=1) if reduce_sum else out


def record_parity(part, used):
    """with CTGCN_PARITY_OUT=<dir>: keep the shares of the tolerance a test used as <dir>/gru_part_<part>.json, and join the parts kept
    so far into <dir>/gru_width_parity_errors.json (the copy under profiles/ is such a file)"""
    out_dir = os.environ.get("CTGCN_PARITY_OUT")
    if not out_dir:
        return
    with open(os.path.join(out_dir, "gru_part_%s.json" % part), "w") as fp:
        json.dump(used, fp, indent=1, sort_keys=True)
    cases = {}
    for f in sorted(glob.glob(os.path.join(out_dir, "gru_part_*.json"))):
        with open(f) as fp:
            cases[os.path.basename(f)[len("gru_part_"):-len(".json")]] = json.load(fp)
    joined = {"rule": "share used of max(4 x yardstick, floor) of the largest reference magnitude; floor 2e-6 for outputs, 1e-5 for "
                      "gradients; the yardstick is the fp32-vs-fp64 error of the same dense definition (ops) or of the reference modules",
              "largest": max(v for c in cases.values() for v in c.values()), "cases": cases}
    with open(os.path.join(out_dir, "gru_width_parity_errors.json"), "w") as fp:
        json.dump(joined, fp, indent=1, sort_keys=True)
