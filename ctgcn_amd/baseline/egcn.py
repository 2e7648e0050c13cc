"""EvolveGCN (EGCN-O / EGCN-H, https://arxiv.org/abs/1902.10191) with the constructor, forward signature and state_dict keys of the
reference's baseline/egcn.py, so checkpoints move both ways.

Per layer and snapshot the weight matrix Q_t [in, out] is evolved by a matrix GRU (EGCN-H feeds it a top-k summary of the node
features, EGCN-O the weights themselves), then the GCN step Y = rrelu(Â (X Q_t)) runs.  The N-sized work of that step — the
aggregation over the normalised adjacency, the activation and, for the next layer's top-k, the score Y · p/‖p‖ — is one pass of
ctgcn_gcn.hip (ops.gcn_layer), forward and backward.  The matrix GRU and the summary work on k x in and in x in operands and stay
torch ops under autograd.  F.rrelu is called by the reference with its default training=False, also under model.train(): the slope
is the constant (1/8 + 1/3) / 2 and nothing is random.
"""
import math
import weakref

import torch
from torch import nn

from .. import ops
from ..layers import as_gcn_adj

_dense_cache = {}


def _dense(x):
    """A sparse feature tensor (the one-hot degree features) as a dense one, made once per tensor and cached by identity.  The entry
    does not hold the source: it is dropped when the source tensor dies (so its id cannot be met again while the entry exists), and
    the dense [N, 1 + max degree] copy goes with it."""
    if not x.is_sparse:
        return x
    key = (id(x), x._values().data_ptr())
    hit = _dense_cache.get(key)
    if hit is None:
        hit = _dense_cache[key] = x.to_dense()
        weakref.finalize(x, _dense_cache.pop, key, None)
    return hit


def _uniform_by(t, fan):
    bound = 1. / math.sqrt(fan)
    with torch.no_grad():
        t.uniform_(-bound, bound)


class mat_GRU_gate(nn.Module):
    """act(W x + U h + bias) on [rows, cols] matrices, W and U [rows, rows]"""

    def __init__(self, rows, cols, activation):
        super().__init__()
        self.activation = activation
        self.W = nn.Parameter(torch.empty(rows, rows))
        self.U = nn.Parameter(torch.empty(rows, rows))
        self.bias = nn.Parameter(torch.empty(rows, cols))
        for p in (self.W, self.U, self.bias):
            _uniform_by(p, p.size(1))

    def forward(self, x, hidden):
        return self.activation(self.W.matmul(x) + self.U.matmul(hidden) + self.bias)


class TopK(nn.Module):
    """The k rows of X with the largest X · p / ‖p‖, each scaled by tanh of its score, transposed to [feats, k]."""

    def __init__(self, feats, k):
        super().__init__()
        self.scorer = nn.Parameter(torch.empty(feats, 1))
        _uniform_by(self.scorer, feats)
        self.k = k

    def unit_scorer(self):
        with torch.no_grad():
            return (self.scorer / self.scorer.norm()).view(-1)

    def forward(self, node_embs, select_scores=None):
        """select_scores [N]: the selection scores when a previous pass already has them (no gradient goes through the selection);
        the differentiable part is recomputed on the k picked rows only, which is the reference's function of (X, p)."""
        if select_scores is None:
            with torch.no_grad():
                select_scores = node_embs.matmul(self.unit_scorer())
        idx = select_scores.view(-1).topk(self.k).indices          # N < k fails here, as in the reference
        picked = node_embs[idx]
        scores = picked.matmul(self.scorer) / self.scorer.norm()
        return (picked * torch.tanh(scores)).t()


class mat_GRU_cell(nn.Module):
    def __init__(self, input_dim, output_dim, egcn_type='EGCNH'):
        super().__init__()
        assert egcn_type in ('EGCNO', 'EGCNH')
        self.egcn_type = egcn_type
        self.update = mat_GRU_gate(input_dim, output_dim, nn.Sigmoid())
        self.reset = mat_GRU_gate(input_dim, output_dim, nn.Sigmoid())
        self.htilda = mat_GRU_gate(input_dim, output_dim, nn.Tanh())
        self.choose_topk = TopK(feats=input_dim, k=output_dim)      # present (and in the state dict) for EGCNO too, unused there

    def forward(self, prev_Q, prev_Z=None, select_scores=None):
        z = prev_Q if self.egcn_type == 'EGCNO' else self.choose_topk(prev_Z, select_scores)
        update = self.update(z, prev_Q)
        reset = self.reset(z, prev_Q)
        h_cap = self.htilda(z, reset * prev_Q)
        return (1 - update) * prev_Q + update * h_cap


class GRCU(nn.Module):
    def __init__(self, input_dim, output_dim, egcn_type='EGCNH'):
        super().__init__()
        assert egcn_type in ('EGCNO', 'EGCNH')
        self.egcn_type = egcn_type
        self.evolve_weights = mat_GRU_cell(input_dim, output_dim, egcn_type)
        self.GCN_init_weights = nn.Parameter(torch.empty(input_dim, output_dim))
        _uniform_by(self.GCN_init_weights, output_dim)

    def aggregate(self, S, adj, score_vec):
        """(rrelu(Â S), Y · score_vec or None): the fused pass; overridden by tools/egcn_bench.py's composed variants"""
        if score_vec is None:
            return ops.gcn_layer(S, adj, ops.GCN_ACT_RRELU), None
        return ops.gcn_layer(S, adj, ops.GCN_ACT_RRELU, score_vec)

    def forward(self, A_list, node_embs_list, select_scores_list=None, next_scorer=None):
        """next_scorer: the unit scorer of the layer that consumes this one's output; its scores come back as the second result"""
        Q = self.GCN_init_weights
        out_seq, score_seq = [], []
        for t, adj in enumerate(A_list):
            X = node_embs_list[t]
            if self.egcn_type == 'EGCNO':
                Q = self.evolve_weights(Q)
            else:
                Q = self.evolve_weights(Q, X, None if select_scores_list is None else select_scores_list[t])
            Y, scores = self.aggregate(X.matmul(Q), adj, next_scorer)
            out_seq.append(Y)
            score_seq.append(scores)
        return out_seq, (score_seq if next_scorer is not None else None)


class EvolveGCN(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, egcn_type='EGCNH'):
        super().__init__()
        assert egcn_type in ('EGCNO', 'EGCNH')
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.method_name = 'EvolveGCN'
        self.egcn_type = egcn_type
        self.GRCU_layers = nn.ModuleList([GRCU(input_dim, hidden_dim, egcn_type), GRCU(hidden_dim, output_dim, egcn_type)])

    def forward(self, Nodes_list, A_list, nodes_mask_list=None):
        """list[T] of [N, output_dim]: Nodes_list[t] dense (or sparse one-hot) features, A_list[t] an ops.GcnAdj or the loader's
        normalised sparse tensor (get_date_adj_list(normalize=True, add_eye=True))."""
        if nodes_mask_list is not None:
            raise NotImplementedError("nodes_mask_list is not supported (no caller of the reference passes one)")
        xs = [_dense(x) for x in Nodes_list]
        ops._need_cuda(*xs)
        adjs = [as_gcn_adj(a, xs[0].device) for a in A_list]
        scores = None
        for j, unit in enumerate(self.GRCU_layers):
            nxt = self.GRCU_layers[j + 1] if j + 1 < len(self.GRCU_layers) else None
            scorer = nxt.evolve_weights.choose_topk.unit_scorer() if (nxt is not None and self.egcn_type == 'EGCNH') else None
            xs, scores = unit(adjs, xs, scores, scorer)
        return xs
