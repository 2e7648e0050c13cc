"""DynRNN (dyngraph2vec, https://arxiv.org/abs/1809.02657) with the class names, constructors, method_name and state_dict keys of the
reference's baseline/dynRNN.py (encoder.layer_list.0.weight_ih_l0, ... : the nn.LSTM modules stay the parameter holders), so a reference
checkpoint loads.  It trains through dynae.DynamicEmbedding with dynae's generator, predictor and DynGraph2VecLoss.

The reference feeds dense [B, look_back, N] adjacency rows to a stack of nn.LSTM, and its decoder's last layer has hidden size N.  On
the kernel path a batch is a RowBatch (row ids into an ops.SnapshotRows):
    first layer   the input projection of all B look_back selected rows is one ops.rowsel_conv over weight_ih_l0.t() with bias_ih_l0
                  (a gather; the rows are taken step after step, so the result is the time-major gi of ops.lstm_layer);
    every layer   ops.lstm_layer (ctgcn_lstmcell.hip): library GEMMs for the products, one fused pass per step between them;
    decoder       over the encoder's output sequence (not over hx: that is what the reference's decoder reads), its last layer in
                  last-only mode; the prediction is that layer's last h, with no ReLU, and goes to ops.wrecon_loss(relu=False).
A dense CUDA tensor goes through the nn.LSTM modules one after the other, the reference's expression: the composed path."""
import torch
import torch.nn as nn

from .. import ops
from .dynae import _as_batch


class MLLSTM(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, bias=True):
        super(MLLSTM, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.bias = bias

        self.layer_list = nn.ModuleList()
        self.layer_list.append(nn.LSTM(input_dim, n_units[0], bias=bias, batch_first=True))

        layer_num = len(n_units)
        for i in range(1, layer_num):
            self.layer_list.append(nn.LSTM(n_units[i - 1], n_units[i], bias=bias, batch_first=True))
        self.layer_list.append(nn.LSTM(n_units[-1], output_dim, bias=bias, batch_first=True))
        self.layer_num = layer_num + 1

    def forward(self, x):
        """(outputs [B, L, output_dim], the last step's [B, output_dim]) through the nn.LSTM modules"""
        ops._need_cuda(x)
        for i in range(self.layer_num):
            x, _ = self.layer_list[i](x)
        return x, x[:, -1, :]

    def _biases(self, i):
        layer = self.layer_list[i]
        return (layer.bias_ih_l0, layer.bias_hh_l0) if self.bias else (None, None)

    def forward_layers(self, x, last_only=False, gi=None):
        """every layer through ops.lstm_layer: the output sequence [B, L, output_dim], or with last_only the last layer's h_{L-1}
        [B, output_dim] alone.  gi: the first layer's input projection in place of x, made by the caller with bias_ih folded in."""
        for i in range(self.layer_num):
            layer = self.layer_list[i]
            b_ih, b_hh = self._biases(i)
            last = last_only and i == self.layer_num - 1
            if gi is not None:
                x, gi = ops.lstm_layer(None, None, layer.weight_hh_l0, None, b_hh, last_only=last, gi=gi), None
            else:
                x = ops.lstm_layer(x, layer.weight_ih_l0, layer.weight_hh_l0, b_ih, b_hh, last_only=last)
        return x

    def first_transposed(self):
        """the first layer's weight_ih as the gather reads it: [in, 4 H] rows (a copy; the predictors make it once for all batches)"""
        return self.layer_list[0].weight_ih_l0.t().contiguous()

    def forward_rows(self, rows, sel, first_t=None, last_only=False):
        """the same over the adjacency rows sel [B, L] selects from a SnapshotRows: the first layer's input projection as one gather
        over the B L rows (first_t: first_transposed())"""
        sel = rows.select(sel)
        first = self.layer_list[0]
        if first.input_size != rows.n:
            raise ValueError("the first layer reads %d columns, the batch has %d" % (first.input_size, rows.n))
        flat = sel.host_idx.T.reshape(-1)                                   # step after step: position t B + b is row idx[b, t]
        gi = ops.rowsel_conv(self.first_transposed() if first_t is None else first_t, rows, flat, self._biases(0)[0], relu=False, col_stride=0)
        return self.forward_layers(None, last_only, gi=gi.view(sel.L, sel.B, -1).transpose(0, 1))


class DynRNN(nn.Module):
    def __init__(self, input_dim, output_dim, look_back=3, n_units=None, bias=True, **kwargs):
        super(DynRNN, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.look_back = look_back
        self.bias = bias
        self.method_name = 'DynRNN'

        self.encoder = MLLSTM(input_dim, output_dim, n_units, bias=bias)
        self.decoder = MLLSTM(output_dim, input_dim, n_units[::-1], bias=bias)

    def first_transposed(self):
        return self.encoder.first_transposed()

    def encode(self, batch, first_t=None):
        """(the encoder's output sequence [B, L, output_dim], hx = its last step) of a RowBatch or (SnapshotRows, idx)"""
        batch = _as_batch(batch)
        if batch is None:
            raise TypeError("a RowBatch or (SnapshotRows, idx) expected")
        seq = self.encoder.forward_rows(batch.rows, batch.idx, first_t)
        return seq, seq[:, -1, :]

    def decode(self, seq):
        """the prediction [B, N] from the encoder's output sequence: the last h of the decoder's last layer, no ReLU"""
        return self.decoder.forward_layers(seq, last_only=True)

    def forward(self, x):
        if isinstance(x, torch.Tensor):
            output, hx = self.encoder(x)
            _, x_pred = self.decoder(output)
            return hx, x_pred
        seq, hx = self.encode(x)
        return hx, self.decode(seq)
