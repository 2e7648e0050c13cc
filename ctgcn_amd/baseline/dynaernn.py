"""DynAERNN (dyngraph2vec, https://arxiv.org/abs/1809.02657) with the class names, constructors, method_name and state_dict keys of the
reference's baseline/dynAERNN.py (ae_encoder.layer_list.<t>.layer_list.<i>.weight, rnn_encoder.layer_list.<i>.weight_ih_l0,
decoder.layer_list.<i>.weight, ...), so a reference checkpoint loads.  It trains through dynae.DynamicEmbedding.

ae_encoder holds one MLP per step of the window, rnn_encoder is an LSTM stack over their outputs, decoder is DynAE's MLP on the last
hidden state.  On the kernel path MLP s takes its first layer from ops.rowsel_conv over column s of the batch's row ids (look_back
gathers), the LSTM stack runs through ops.lstm_layer with its last layer in last-only mode, and the decoder's pre-activation goes to
ops.wrecon_loss(relu=True), as DynAE's does.  A dense CUDA tensor [B, look_back, N] goes through the reference's expression in stock
torch ops.  Unlike the reference, which reads the first look_back steps of whatever it is given, a window of another length is
refused."""
import torch
import torch.nn as nn

from .. import ops
from .dynae import MLP, _as_batch
from .dynrnn import MLLSTM


class MTMLP(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, look_back, bias=True):
        super(MTMLP, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.look_back = look_back
        self.bias = bias

        self.layer_list = nn.ModuleList()
        for timestamp in range(look_back):
            self.layer_list.append(MLP(input_dim, output_dim, n_units, bias=bias))

    def _check(self, steps):
        if steps != self.look_back:
            raise ValueError("a window of %d steps, the model has look_back %d" % (steps, self.look_back))

    def forward(self, x):
        """x [B, look_back, input_dim] -> [B, look_back, output_dim]"""
        self._check(x.shape[1])
        ops._need_cuda(x)
        hx_list = []
        for timestamp in range(self.look_back):
            hx_list.append(self.layer_list[timestamp](x[:, timestamp, :]))
        return torch.stack(hx_list, dim=0).transpose(0, 1)

    def first_transposed(self):
        """the first weights of the look_back MLPs as the gathers read them"""
        return [mlp.first_transposed() for mlp in self.layer_list]

    def forward_rows(self, rows, sel, first_t=None):
        """the same over the adjacency rows sel [B, look_back] selects from a SnapshotRows"""
        sel = rows.select(sel)
        self._check(sel.L)
        hx_list = []
        for timestamp in range(self.look_back):
            step = rows.select(sel.host_idx[:, timestamp])
            hx_list.append(self.layer_list[timestamp].forward_rows(rows, step, 0, None if first_t is None else first_t[timestamp]))
        return torch.stack(hx_list, dim=0).transpose(0, 1)


class DynAERNN(nn.Module):
    def __init__(self, input_dim, output_dim, look_back=3, ae_units=None, rnn_units=None, bias=True, **kwargs):
        super(DynAERNN, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.look_back = look_back
        self.bias = bias
        self.method_name = 'DynAERNN'

        self.ae_encoder = MTMLP(input_dim, output_dim, ae_units, look_back, bias=bias)
        self.rnn_encoder = MLLSTM(output_dim, output_dim, rnn_units, bias=bias)
        self.decoder = MLP(output_dim, input_dim, ae_units[::-1], bias=bias)

    def first_transposed(self):
        return self.ae_encoder.first_transposed()

    def encode(self, batch, first_t=None):
        """hx [B, output_dim] of a RowBatch or (SnapshotRows, idx)"""
        batch = _as_batch(batch)
        if batch is None:
            raise TypeError("a RowBatch or (SnapshotRows, idx) expected")
        ae_hx = self.ae_encoder.forward_rows(batch.rows, batch.idx, first_t)
        return self.rnn_encoder.forward_layers(ae_hx, last_only=True)

    def decode(self, hx, pre_activation=False):
        return self.decoder(hx, pre_activation=pre_activation)

    def forward(self, x):
        if isinstance(x, torch.Tensor):
            ae_hx = self.ae_encoder(x)
            output, hx = self.rnn_encoder(ae_hx)
        else:
            hx = self.encode(x)
        return hx, self.decoder(hx)
