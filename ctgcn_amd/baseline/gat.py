"""GAT (https://arxiv.org/abs/1710.10903) with the constructors, forward signature and state_dict keys of the reference's
baseline/gat.py (its sparse SpGraphAttentionLayer / GAT pair), so checkpoints move both ways.

A layer is the row-wise softmax of -leakyrelu(a · [W x_i ; W x_j]) over the stored entries of the adjacency, applied to W x.  All
of it after the product x W is ops.gat_conv (ctgcn_gat.hip): the scores, the softmax-weighted gather, attention dropout, ELU and the
dropout on the concatenated heads, and a backward over the CSR and its transpose.  The head_num heads of layer 1 share x and the
adjacency and are one call: their W and a are concatenated on the fly and autograd splits the gradient.  Only the pattern of the
adjacency is read, as in the reference (adj._indices()).

Dropout is counter-based and nothing is stored: one base key per training-mode forward (gcn.draw_key; torch.manual_seed reproduces
a run bit for bit).  The attention draw of snapshot t, layer l (0 the heads, 1 out_att), head h and entry (i, j) is
u01(base + 4096 t + 2048 l + h, i, j); the feature draw of snapshot t on entry (i, c) of the concatenated heads is
u01(base + 2^40 + t, i, c).  A dense input is dropped out by stock F.dropout first, as in the reference.
"""
import torch
from torch import nn
from torch.nn import functional as F

from .. import layers, ops
from .gcn import draw_key

MAX_HEADS = 2048                        # a layer's heads own the keys [base + 4096 t + 2048 l, + 2048)
FEATURE_KEY = 2 ** 40


def support(x, W):
    """x W; the sparse identity (get_feature_list without a feature file) needs no product, like GraphConvolution.support"""
    if x.is_sparse:
        if layers._is_identity(x) and x.shape[1] == W.shape[0]:
            return W
        return torch.sparse.mm(x, W)
    return torch.matmul(x, W)


class SpGraphAttentionLayer(nn.Module):
    """One attention head.  forward(input, adj): elu(attention(input W)) with concat=True, the plain attention output otherwise."""

    def __init__(self, in_features, out_features, dropout, alpha, concat=True):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        self.alpha, self.concat = alpha, concat
        self.p = dropout
        self.W = nn.Parameter(torch.empty(in_features, out_features))
        self.a = nn.Parameter(torch.empty(1, 2 * out_features))
        nn.init.xavier_normal_(self.W.data, gain=1.414)
        nn.init.xavier_normal_(self.a.data, gain=1.414)

    def halves(self):
        """(a_src, a_dst), each [1, out_features]"""
        return self.a[:, :self.out_features], self.a[:, self.out_features:]

    def forward(self, input, adj, key=None):
        """key: the attention-dropout key of this call; None draws one in training mode (none in eval mode or at dropout 0)"""
        ops._need_cuda(input)
        adj = layers.as_gcn_adj(adj, input.device, symmetric=False)
        p = float(self.p) if self.training else 0.0
        if key is None:
            key = int(torch.randint(0, 2 ** 62, (1,))) if p > 0 else 0
        a_src, a_dst = self.halves()
        return ops.gat_conv(support(input, self.W), a_src, a_dst, adj, 1, self.alpha, ops.GAT_EPI_ELU if self.concat else ops.GAT_EPI_NONE, p, key)

    def __repr__(self):
        return '%s (%d -> %d)' % (self.__class__.__name__, self.in_features, self.out_features)


class GAT(nn.Module):
    def __init__(self, input_dim, hidden_dim, output_dim, dropout=0.6, alpha=0.2, head_num=8, learning_type='U-neg'):
        super().__init__()
        assert learning_type in ['U-neg', 'S-node', 'S-edge', 'S-link-st', 'S-link-dy']
        if head_num > MAX_HEADS:
            raise ValueError("head_num %d above %d: the heads' dropout keys would run into the next layer's" % (head_num, MAX_HEADS))
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.dropout, self.alpha, self.head_num = dropout, alpha, head_num
        self.learning_type = learning_type
        self.method_name = 'GAT'
        self.attentions = [SpGraphAttentionLayer(input_dim, hidden_dim, dropout=dropout, alpha=alpha, concat=True) for _ in range(head_num)]
        for i, attention in enumerate(self.attentions):
            self.add_module('attention_{}'.format(i), attention)
        self.out_att = SpGraphAttentionLayer(hidden_dim * head_num, output_dim, dropout=dropout, alpha=alpha, concat=False)

    def forward(self, x, adj):
        """[N, output_dim], or a list of them for a list of snapshots; adj an ops.GcnAdj or the loader's sparse tensor"""
        key = draw_key(self)
        if isinstance(x, list):
            return [self.gat(x[t], adj[t], key, t) for t in range(len(x))]
        return self.gat(x, adj, key)

    def gat(self, x, adj, key=0, t=0):
        """One snapshot under the base key `key` as snapshot t"""
        ops._need_cuda(x)
        adj = layers.as_gcn_adj(adj, x.device, symmetric=False)
        p = float(self.dropout) if self.training else 0.0
        if not x.is_sparse:
            x = F.dropout(x, self.dropout, training=self.training)
        heads = self.attentions
        if len(heads) == 1:
            W, (a_src, a_dst) = heads[0].W, heads[0].halves()
        else:
            W = torch.cat([att.W for att in heads], dim=1)
            a_src = torch.cat([att.halves()[0] for att in heads], dim=0)
            a_dst = torch.cat([att.halves()[1] for att in heads], dim=0)
        h = ops.gat_conv(support(x, W), a_src, a_dst, adj, len(heads), self.alpha, ops.GAT_EPI_ELU_DROPOUT, p, key + 4096 * t, p,
                         key + FEATURE_KEY + t)
        a_src, a_dst = self.out_att.halves()
        out = ops.gat_conv(torch.matmul(h, self.out_att.W), a_src, a_dst, adj, 1, self.alpha, ops.GAT_EPI_ELU, p, key + 4096 * t + 2048)
        if self.learning_type == 'U-neg':
            return F.log_softmax(out, dim=1)
        return out
