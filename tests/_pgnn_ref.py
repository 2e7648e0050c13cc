"""The project's own references for ctgcn_amd.baseline.pgnn, in numpy and stock torch ops, on any device and in any dtype.

host_dist is a host model of the anchor-distance pass: per anchor set a level-synchronous BFS in which every reached node takes the
smallest anchor position among its neighbours on the previous level.  LayerMirror / PgnnMirror are the layer and the model written in
the reference's materialising form ([N, A, 2 in] and [N, A, out] tensors) with the modules' state_dict keys; dropout is an explicit
argument: keep masks, which the GPU tests compute with the host model of the draw (_gcrn_ref.keep_mask).
tests/test_pgnn_host.py pins both to the reference's recorded results (tests/golden/pgnn_uci.npz); the GPU tests then use them as their
reference, because the reference tree is not present where they run."""
import numpy as np
import torch
from torch import nn
from torch.nn import functional as F

import _egcn_ref as E
import _gcrn_ref as R
import _gin_sage_ref as G
from conftest import formula_tensor, load_golden

N, T, DENSE_IN = R.N, R.T, R.DENSE_IN
ADAM_STEPS, LR = 3, 1e-3
CUTOFFS = (-1, 2)
# fixture prefix -> constructor arguments (input_dim, feature_dim, hidden_dim, output_dim, then keywords)
CASES = {
    "pgnn_l2": ((DENSE_IN, 32, 32, 128), dict(feature_pre=True, layer_num=2)),          # the configs' shape
    "pgnn_l1": ((DENSE_IN, 32, 32, 16), dict(feature_pre=True, layer_num=1)),           # one layer: the unnormalised position output
    "pgnn_l3_nopre": ((DENSE_IN, 32, 32, 16), dict(feature_pre=False, layer_num=3)),    # conv_hidden, and conv_first on the raw features
}


# ------------------------------------------------------------------------------------------------ host model of the distance pass
def host_dist(indptr, indices, sets, cutoff=-1):
    """(level int32, dist_max float32, pos int32, node int32), each [n, A], over the pattern (indptr, indices) as given"""
    n, A = len(indptr) - 1, len(sets)
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(indptr))
    level = np.full((n, A), -1, dtype=np.int32)
    pos = np.zeros((n, A), dtype=np.int32)
    node = np.zeros((n, A), dtype=np.int32)
    big = np.iinfo(np.int64).max
    for a, members in enumerate(sets):
        members = np.asarray(members, dtype=np.int64)
        lab = np.full(n, big, dtype=np.int64)
        lev = np.full(n, -1, dtype=np.int64)
        np.minimum.at(lab, members, np.arange(len(members), dtype=np.int64))
        lev[members] = 0
        L = 0
        while cutoff <= 0 or L < cutoff:
            on = (lev[indices] == L) & (lev[rows] == -1)         # entries (v, u) with u on level L and v unreached
            if not on.any():
                break
            new = np.full(n, big, dtype=np.int64)
            np.minimum.at(new, rows[on], lab[indices[on]])
            hit = new != big
            lab[hit], lev[hit] = new[hit], L + 1
            L += 1
        reached = lev >= 0
        level[:, a] = lev
        pos[reached, a] = lab[reached]
        if len(members):
            node[:, a] = members[pos[:, a]]
    return level, dist_of(level), pos, node


def dist_of(level):
    """float32(1) / float32(level + 1), 0 where unreached (level -1)"""
    return np.where(level >= 0, np.float32(1) / np.maximum(level + 1, 1).astype(np.float32), np.float32(0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ mirrors
def _reset(module):
    for m in module.modules():
        if isinstance(m, nn.Linear):
            nn.init.xavier_uniform_(m.weight.data, gain=nn.init.calculate_gain("relu"))
            if m.bias is not None:
                nn.init.constant_(m.bias.data, 0.0)


class NonlinearMirror(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, bias=True):
        super().__init__()
        self.linear1 = nn.Linear(input_dim, hidden_dim, bias=bias)
        self.linear2 = nn.Linear(hidden_dim, output_dim, bias=bias)
        _reset(self)

    def forward(self, x):
        return self.linear2(F.relu(self.linear1(x)))


class LayerMirror(nn.Module):
    def __init__(self, input_dim, output_dim, dist_trainable=True, bias=True):
        super().__init__()
        self.dist_trainable = dist_trainable
        if dist_trainable:
            self.dist_compute = NonlinearMirror(1, output_dim, 1, bias=bias)
        self.linear_hidden = nn.Linear(input_dim * 2, output_dim, bias=bias)
        self.linear_out_position = nn.Linear(output_dim, 1, bias=bias)
        _reset(self)

    def forward(self, feature, dists_max, dists_argmax):
        dists_max = dists_max.to(feature.dtype)
        if self.dist_trainable:
            dists_max = self.dist_compute(dists_max.unsqueeze(-1)).squeeze(-1)
        subset = feature[dists_argmax.flatten(), :].reshape(dists_argmax.shape[0], dists_argmax.shape[1], feature.shape[1])
        messages = subset * dists_max.unsqueeze(-1)
        self_feature = feature.unsqueeze(1).repeat(1, dists_max.shape[1], 1)
        messages = F.relu(self.linear_hidden(torch.cat((messages, self_feature), dim=-1)))
        return self.linear_out_position(messages).squeeze(-1), torch.mean(messages, dim=1)


class PgnnMirror(nn.Module):
    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True):
        super().__init__()
        self.feature_pre, self.layer_num, self.dropout = feature_pre, layer_num, dropout
        if layer_num == 1:
            hidden_dim = output_dim
        if feature_pre:
            self.linear_pre = nn.Linear(input_dim, feature_dim, bias=bias)
        self.conv_first = LayerMirror(feature_dim if feature_pre else input_dim, hidden_dim, bias=bias)
        if layer_num > 1:
            self.conv_hidden = nn.ModuleList([LayerMirror(hidden_dim, hidden_dim, bias=bias) for _ in range(layer_num - 2)])
            self.conv_out = LayerMirror(hidden_dim, output_dim, bias=bias)

    def drop(self, x, keep, layer):
        return x if keep is None else x * keep[layer].to(x.dtype).to(x.device) / (1.0 - self.dropout)

    def one(self, x, dists_max, dists_argmax, keep=None):
        """keep: None or a list of bool [N, hidden] masks, one per layer but the last, of the entries dropout keeps"""
        if self.feature_pre:
            x = self.linear_pre(x)
        x_position, x = self.conv_first(x, dists_max, dists_argmax)
        if self.layer_num == 1:
            return x_position
        x = self.drop(x, keep, 0)
        for i in range(self.layer_num - 2):
            _, x = self.conv_hidden[i](x, dists_max, dists_argmax)
            x = self.drop(x, keep, 1 + i)
        x_position, _ = self.conv_out(x, dists_max, dists_argmax)
        return F.normalize(x_position, p=2, dim=-1)

    def forward(self, x, dists_max, dists_argmax, keep=None):
        if isinstance(x, list):
            return [self.one(x[t], dists_max[t], dists_argmax[t], None if keep is None else keep[t]) for t in range(len(x))]
        return self.one(x, dists_max, dists_argmax, keep)


# ------------------------------------------------------------------------------------------------ the fixture's setup, shared by the tests
def fixture():
    return load_golden("pgnn_uci.npz")


def build(case, cls, dropout=0.0):
    args, kwargs = CASES[case]
    return cls(*args, dropout=dropout, **kwargs)


def hidden_width(case):
    args, kwargs = CASES[case]
    return args[3] if kwargs["layer_num"] == 1 else args[2]


def features(dtype=torch.float32, device="cpu"):
    return R.features("gcn_dense", dtype, device)


def pattern(t):
    """(indptr, indices) of UCI snapshot t: symmetric, no diagonal"""
    m = G.raw_csr(t)
    return m.indptr, m.indices


def anchor_sets(g):
    off = g["anchor_offsets"]
    return [g["anchor_members"][off[a]:off[a + 1]] for a in range(len(off) - 1)]


def recorded_dist(g, t, cutoff):
    """(level int32, dist_max float32, pos int64) of snapshot t as the reference's get_dist_max gave them"""
    tag = "exact" if cutoff <= 0 else "cut%d" % cutoff
    level = g["level_%s_t%d" % (tag, t)].astype(np.int32)
    dist = dist_of(level)
    if cutoff <= 0:
        return level, dist, g["pos_exact_t%d" % t].astype(np.int64)
    pos = g["posxor_%s_t%d" % (tag, t)] ^ np.where(level >= 0, g["pos_exact_t%d" % t], 0).astype(np.int32)      # as make_golden_pgnn.py stores it
    return level, dist, pos.astype(np.int64)


def anchor_tensors(g, device="cpu", cutoff=-1):
    """(dists_max list, dists_argmax list) of the fixture's snapshots: float32 and int64 [N, A]"""
    rec = [recorded_dist(g, t, cutoff) for t in range(T)]
    return [torch.from_numpy(r[1]).to(device) for r in rec], [torch.from_numpy(r[2]).to(device) for r in rec]


def surrogate_weights(width, dtype=torch.float32, device="cpu"):
    return [torch.from_numpy(formula_tensor((N, width), 0.05 + 0.01 * t, 1.0 + t)).to(dtype).to(device) for t in range(T)]


def adam_losses(model, forward, weights):
    """E.adam_losses, but a parameter whose gradient is None is recorded as None (E.adam_losses stores zeros)"""
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    losses, first = [], None
    for _ in range(ADAM_STEPS):
        opt.zero_grad()
        outs = list(forward())
        loss = E.surrogate(outs, weights)
        loss.backward()
        if first is None:
            first = ([o.detach().clone() for o in outs], {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()})
        losses.append(float(loss.detach()))
        opt.step()
    return losses, first
