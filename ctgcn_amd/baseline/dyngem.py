"""DynGEM (https://arxiv.org/abs/1805.11273) with the class names, constructors, method_name and state_dict keys of the reference's
baseline/dynGEM.py; the MLP, the regularisation and the trainer (DynamicEmbedding) are baseline/dynae.py's, whose docstring describes
the kernel path and the composed one.

A batch is B drawn stored entries (i, j, w) of the snapshot.  Both sides run as one stacked batch of 2 B adjacency rows (the i rows,
then the j rows): one ops.rowsel_conv, one decoder pass, one ops.wrecon_loss with the rows' weight sums as divisors.  A node occurs
many times in such a batch; the gather's backward adds its positions in a fixed order (no atomics).

Reference behaviour that is reproduced because results depend on it:
  * DynGEMLoss multiplies a [B] tensor by a [B, 1] tensor, so its embedding term is the mean of a [B, B] outer product:
    alpha · mean_b(‖hx_i − hx_j‖²) · mean_b(w).  It is computed as that product of two means; no [B, B] tensor is made.
  * The penalty β is the generator's; the beta stored on DynGEMLoss is unused.
  * Every step is the first batch_size entries of a fresh shuffle (see baseline/dynae.py); the last batch is not padded, so a snapshot
    with fewer than batch_size entries gives batches of that many.
  * Entries are the stored non-zeros in row-major order (sp.find's order differs between scipy versions; it matters only with
    shuffle=False)."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from .dynae import MLP, RegularizationLoss, RowBatch, _AutoEncoder, _as_rows


class PairBatch(RowBatch):
    """RowBatch of 2 B rows: the i side, then the j side, of B drawn entries; values their weights"""

    @property
    def pairs(self):
        return len(self.host_values)

    def dense_sides(self):
        """[xi, xj], [yi, yj, value]: the reference generator's tensors (penalties with the degree column appended), made on the device"""
        x, _, pen = self.dense()
        pen = torch.cat((pen, torch.sum(x, dim=1).unsqueeze(1)), dim=1)
        B = self.pairs
        return [x[:B], x[B:]], [pen[:B], pen[B:], self.values.unsqueeze(1)]


class DynGEM(_AutoEncoder):
    def __init__(self, input_dim, output_dim, n_units=None, bias=True, **kwargs):
        super(DynGEM, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.bias = bias
        self.method_name = 'DynGEM'

        self.encoder = MLP(input_dim, output_dim, n_units, bias=bias)
        self.decoder = MLP(output_dim, input_dim, n_units[::-1], bias=bias)


def embedding_term(hx_i, hx_j, edge_weight):
    """The reference's torch.mean(torch.sum(torch.square(hx_i − hx_j), dim=1) * edge_weight) with edge_weight [B, 1]: a [B] tensor
    times a [B, 1] tensor is their [B, B] outer product, so the mean is mean_b(‖hx_i − hx_j‖²) · mean_b(w), not the mean of the paired
    products.  Computed as the product of the two means (stock torch ops, any device)."""
    return torch.mean(torch.sum(torch.square(hx_i - hx_j), dim=1)) * torch.mean(edge_weight)


class DynGEMLoss(nn.Module):
    def __init__(self, alpha, beta, nu1, nu2):
        super(DynGEMLoss, self).__init__()
        self.alpha = alpha
        self.beta = beta
        self.regularization = RegularizationLoss(nu1, nu2)

    def forward(self, model, input_list):
        """the reference's nine dense tensors, or [z, hx, batch] with z [2 B, N] the decoder's pre-activation and hx [2 B, d] the
        embedding of a PairBatch: the kernel path.  z is consumed: its memory receives the gradient."""
        if len(input_list) == 3:
            z, hx, batch = input_list
            B = batch.pairs
            x_loss = ops.wrecon_loss(z, batch.rows, batch.tgt, batch.beta, divide=True, scale=1.0 / B, relu=True, overwrite=True)
            hx_i, hx_j, edge_weight = hx[:B], hx[B:], batch.values
        else:
            assert len(input_list) == 9
            xi_pred, x_i, penalty_i = input_list[0], input_list[1], input_list[2]
            xj_pred, x_j, penalty_j = input_list[3], input_list[4], input_list[5]
            hx_i, hx_j, edge_weight = input_list[6], input_list[7], input_list[8]
            ops._need_cuda(*input_list)
            node_num = xj_pred.shape[1]
            xi_loss = torch.mean(torch.sum(torch.square((xi_pred - x_i) * penalty_i[:, 0:node_num]), dim=1) / penalty_i[:, node_num])
            xj_loss = torch.mean(torch.sum(torch.square((xj_pred - x_j) * penalty_j[:, 0:node_num]), dim=1) / penalty_j[:, node_num])
            x_loss = xi_loss + xj_loss
        return x_loss + self.alpha * embedding_term(hx_i, hx_j, edge_weight) + self.regularization(model)


def _elements(rows):
    """(row, col, value) of the stored non-zeros of snapshot 0, row-major; kept on the window (a generator is made per batch)"""
    hit = getattr(rows, "_dyngem_elements", None)
    if hit is None:
        n = rows.n
        hi = rows.host_ptr[n]
        row = np.repeat(np.arange(n, dtype=np.int64), rows.host_len[:n])
        col, val = rows.host_col[:hi].astype(np.int64), rows.host_val[:hi]
        keep = val != 0
        hit = rows._dyngem_elements = (row[keep], col[keep], val[keep])
    return hit


class DynGEMBatchGenerator:
    def __init__(self, node_list, batch_size, beta, shuffle=True, has_cuda=False):
        self.node_list = node_list
        self.node_num = len(node_list)
        self.batch_size = batch_size
        self.beta = beta
        self.shuffle = shuffle
        self.has_cuda = has_cuda

    def batch_num(self, graph):
        rows = _as_rows(graph, need_device=False)
        return -(-len(_elements(rows)[0]) // self.batch_size)

    def generate(self, graph):
        """yields PairBatch after PairBatch of the one snapshot in graph (an ops.SnapshotRows, or scipy: index arithmetic only)"""
        from ..embedding import epoch_order
        rows = _as_rows(graph, need_device=False)
        assert rows.T == 1 and rows.n == self.node_num
        row, col, val = _elements(rows)
        element_num = len(row)
        batch_num = -(-element_num // self.batch_size)
        element_indices = epoch_order(element_num, self.shuffle).numpy()
        counter = 0
        while True:
            pick = element_indices[self.batch_size * counter: min(element_num, self.batch_size * (counter + 1))]
            idx = np.concatenate((row[pick], col[pick]))
            counter += 1
            yield PairBatch(rows if isinstance(rows, ops.SnapshotRows) else None, idx, idx, self.beta, val[pick])
            if counter == batch_num:
                element_indices = epoch_order(element_num, self.shuffle).numpy()
                counter = 0


class DynGEMBatchPredictor:
    def __init__(self, node_list, batch_size, has_cuda=False):
        self.node_list = node_list
        self.node_num = len(node_list)
        self.batch_size = batch_size
        self.has_cuda = has_cuda

    def predict(self, model, graph, need_pred=True, fused=True, start=0):
        """(embedding [N, d], x_pred [N, N] or None) of snapshot `start` of graph"""
        rows = _as_rows(graph, next(model.parameters()).device)
        emb, pred = [], []
        with torch.no_grad():
            first_t = model.encoder.first_transposed() if fused else None       # one transposed copy for all batches
            for lo in range(0, self.node_num, self.batch_size):
                idx = start * rows.n + np.arange(lo, min(self.node_num, lo + self.batch_size), dtype=np.int64)
                hx = model.encode((rows, idx), first_t) if fused else model.encoder(rows.dense(idx)[:, 0])
                emb.append(hx)
                if need_pred:
                    pred.append(model.decode(hx))
        return torch.cat(emb, dim=0), (torch.cat(pred, dim=0) if need_pred else None)
