"""GCRN (GCN per snapshot, then a GRU or LSTM over the snapshots, then LayerNorm; https://arxiv.org/abs/1612.07659) with the
constructor, forward signature and state_dict keys of the reference's baseline/gcrn.py, so checkpoints move both ways.

Snapshot t goes through its own GCN (baseline/gcn.py); the row normalisation the reference applies to its output is the epilogue of
layer 2's aggregation (ops.GCN_EPI_L2NORM).  LayerNorm(RNN(seq)) over the [N, T, output_dim] sequence is layers.rnn_reduce_norm: the
fused GRU / LSTM kernels (forward, and the step-wise backward) at output_dim 128, library GEMMs plus one fused cell pass per step
(ops.gru_layer / ops.lstm_layer) at any other width.
Without grad the snapshots' rows are written straight into the sequence buffer.
"""
import torch
from torch import nn

from .. import layers, ops
from .gcn import GCN, draw_key


class GCRN(nn.Module):
    def __init__(self, input_dim, feature_dim, hidden_dim, output_dim, feature_pre=True, layer_num=2, dropout=0.5, bias=True, duration=1,
                 rnn_type='GRU'):
        super().__init__()
        assert rnn_type in ('LSTM', 'GRU')
        self.input_dim, self.feature_dim, self.hidden_dim, self.output_dim = input_dim, feature_dim, hidden_dim, output_dim
        self.feature_pre, self.layer_num = feature_pre, layer_num          # unused, as in the reference
        self.dropout, self.bias, self.duration, self.rnn_type = dropout, bias, duration, rnn_type
        self.method_name = 'GCRN'
        self.gcn_list = nn.ModuleList([GCN(input_dim, hidden_dim, output_dim, dropout=dropout, bias=bias) for _ in range(duration)])
        rnn = nn.LSTM if rnn_type == 'LSTM' else nn.GRU
        self.rnn = rnn(output_dim, output_dim, num_layers=1, bias=bias, batch_first=True)
        self.norm = nn.LayerNorm(output_dim)

    def forward(self, x_list, edge_list):
        """[T, N, output_dim] (a transposed view of [N, T, output_dim]): x_list[t] features, edge_list[t] an ops.GcnAdj or the
        loader's normalised sparse tensor (get_date_adj_list(normalize=True, row_norm=True, add_eye=True))."""
        steps = len(x_list)
        ops._need_cuda(*x_list)
        key = draw_key(self)
        wants_grad = torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or any(x.requires_grad for x in x_list))
        if wants_grad:
            seq = torch.stack([self.gcn_list[t].gcn(x_list[t], edge_list[t], key + t, ops.GCN_EPI_L2NORM) for t in range(steps)], dim=1)
        else:
            seq = torch.empty(x_list[0].shape[0], steps, self.output_dim, dtype=torch.float32, device=x_list[0].device)
            for t in range(steps):
                self.gcn_list[t].gcn(x_list[t], edge_list[t], key + t, ops.GCN_EPI_L2NORM, out=seq[:, t, :])
        # the GRU's step-wise HIP backward: the row normalisation's backward divides d seq by the row norms, and the parameter gradients
        # are sums over all nodes with much cancellation, so the resident-weight kernels' noise (ten times an fp32 run's) shows in them
        return layers.rnn_reduce_norm(self.rnn, self.norm, seq, reduce_sum=False, resident_backward=False).transpose(0, 1)
