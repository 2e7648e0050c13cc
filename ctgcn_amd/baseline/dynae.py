"""DynAE (dyngraph2vec, https://arxiv.org/abs/1809.02657) and the trainer it shares with DynGEM, with the class names, constructors,
method_name and state_dict keys of the reference's baseline/dynAE.py (encoder.layer_list.0.weight, ... in the reference's shapes), so a
reference checkpoint loads.

The reference feeds dense adjacency rows to an MLP: per batch it slices scipy matrices on the host, builds a [B, look_back N] input, a
[B, N] target and a [B, N] penalty tensor, and runs an N-wide first layer over rows that are almost all zeros.  Here the window lives on
the device as one stacked CSR (ops.SnapshotRows) and a batch is a set of row ids into it (RowBatch):
    first layer   ops.rowsel_conv on weight.t() (ctgcn_dyngem.hip): the Linear over the selected rows as a gather, ReLU in its epilogue;
                  the other layers are relu(Linear) as in the reference.
    loss          ops.wrecon_loss on the last decoder layer's pre-activation: Σ_j ((relu(z) − x) pen)² = Σ_j p_j² plus a correction
                  (β² (p_j − v_j)² − p_j²) at the target row's stored entries; no target or penalty tensor.
A model takes a batch as a RowBatch or as (SnapshotRows, idx); a dense CUDA tensor goes through the reference's expressions in stock
torch ops.  fused=False on the trainer runs that composed path end to end (dense rows and penalties made on the GPU): it is the
comparand of the tests and of tools/dyngem_bench.py.  DynamicEmbedding, BatchGenerator, BatchPredictor and DynGraph2VecLoss also serve
DynRNN and DynAERNN (dynrnn.py, dynaernn.py), whose batches are [B, look_back] row ids read step by step and not flattened.

Reference behaviour that is reproduced because results depend on it:
  * learn_embedding makes a fresh generator for every batch, so every step trains on the first batch_size elements of a fresh shuffle
    (with shuffle=False: on the same first batch every time), and Adam steps once per epoch, after batch_num accumulated backward
    passes.  The order is drawn with torch.randperm from torch's CPU generator (embedding.epoch_order; the reference draws
    np.random.shuffle), so torch.manual_seed reproduces a run.
  * BatchGenerator always yields batch_size rows: past the end of the records they are zero rows with penalty 1 (row id -1 here), and
    the mean runs over batch_size.
  * The penalty β is the generator's; the beta stored on the loss modules is unused.
  * RegularizationLoss covers the parameters whose name contains 'weight', uses torch.norm(p=1) and the unsquared p=2 norm, divides
    both sums by the number of weights, and returns a zero of shape [1] when both nu are 0.
  * Prediction reads the last look_back snapshots, as adj_list[train_size:] does.  The predictors run the encoder only unless the
    reconstruction is asked for (need_pred=True, the default, returns (embedding, x_pred) as the reference does).
dyngem_embedding(method, args) is the reference's driver of the four methods over these classes."""
import os
import time

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from .._lib import CtgcnHipError
from ..export import save_embedding


def _as_rows(graph_list, device=None, need_device=True):
    """a SnapshotRows as it is; scipy matrices stacked into one on `device`, or, without a device and where only the generators' index
    arithmetic is wanted (need_device=False), into a host-side stand-in"""
    if isinstance(graph_list, ops.SnapshotRows):
        return graph_list
    mats = graph_list if isinstance(graph_list, (list, tuple)) else [graph_list]
    if device is None:
        if need_device:
            raise CtgcnHipError("DynGEM / DynAE run on the MI355X only: pass an ops.SnapshotRows or a CUDA device; there is no CPU fallback")
        return _HostRows(mats)
    return ops.SnapshotRows(mats, device)


class _HostRows(object):
    """what the generators read of a window, from scipy matrices alone"""

    def __init__(self, mats):
        import scipy.sparse as sp
        csr = sp.vstack([sp.csr_matrix(m) for m in mats], format='csr')
        csr.sum_duplicates()
        csr.sort_indices()
        self.T, self.n = len(mats), mats[0].shape[0]
        self.rows = self.T * self.n
        self.host_ptr, self.host_col, self.host_val = csr.indptr.astype(np.int64), csr.indices.astype(np.int32), csr.data.astype(np.float32)
        self.host_len = np.diff(self.host_ptr)


class RowBatch(object):
    """One training batch as row ids into a SnapshotRows: idx [B, L] input rows and tgt [B] target rows (-1: a zero row), the
    generator's β, and for DynGEM the edge weights of the B drawn entries (idx and tgt are then the same 2 B rows: the i side, then
    the j side).  The selections are uploaded on first use."""

    def __init__(self, rows, idx, tgt, beta, values=None):
        self.rows, self.host_idx, self.host_tgt, self.beta, self.host_values = rows, idx, tgt, float(beta), values
        self._idx = self._tgt = self._values = None

    @property
    def idx(self):
        if self._idx is None:
            self._idx = self.rows.select(self.host_idx)
        return self._idx

    @property
    def tgt(self):
        if self._tgt is None:
            self._tgt = self.idx if self.host_tgt is self.host_idx else self.rows.select(self.host_tgt)
        return self._tgt

    @property
    def values(self):
        if self._values is None:
            self._values = torch.from_numpy(np.asarray(self.host_values, dtype=np.float32)).to(self.rows.device)
        return self._values

    def dense(self):
        """(x [B, L N], x_cur [B, N], penalty [B, N]): the reference generator's tensors, made on the device"""
        x = self.rows.dense(self.idx)
        cur = x[:, 0] if self.host_tgt is self.host_idx else self.rows.dense(self.tgt)[:, 0]
        pen = torch.ones_like(cur)
        pen[cur != 0] = self.beta
        return x.reshape(x.shape[0], -1), cur, pen


def _as_batch(x):
    if isinstance(x, RowBatch):
        return x
    if isinstance(x, (tuple, list)) and len(x) == 2 and isinstance(x[0], ops.SnapshotRows):
        return RowBatch(x[0], x[1], x[1], 1.0)
    return None


class MLP(nn.Module):
    def __init__(self, input_dim, output_dim, n_units, bias=True):
        super(MLP, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.bias = bias

        self.layer_list = nn.ModuleList()
        self.layer_list.append(nn.Linear(input_dim, n_units[0], bias=bias))

        layer_num = len(n_units)
        for i in range(1, layer_num):
            self.layer_list.append(nn.Linear(n_units[i - 1], n_units[i], bias=bias))
        self.layer_list.append(nn.Linear(n_units[-1], output_dim, bias=bias))
        self.layer_num = layer_num + 1

    def forward(self, x, pre_activation=False):
        """relu(Linear) layer by layer; pre_activation=True leaves the last layer's ReLU to the caller (ops.wrecon_loss applies it)"""
        ops._need_cuda(x)
        for i in range(self.layer_num):
            x = self.layer_list[i](x)
            if not (pre_activation and i == self.layer_num - 1):
                x = F.relu(x)
        return x

    def first_transposed(self):
        """the first weight as the gather reads it: [in, d] rows.  A copy (weight.t() is no row view); the predictors make it once for
        all their batches, a training step once per forward, where its backward transposes the gradient back."""
        return self.layer_list[0].weight.t().contiguous()

    def forward_rows(self, rows, sel, col_stride=0, first_t=None):
        """the same over the adjacency rows sel selects from a SnapshotRows: the first layer as a gather over first_t (default:
        first_transposed())"""
        first = self.layer_list[0]
        if first.in_features != max(sel.L - 1, 0) * col_stride + rows.n:
            raise ValueError("the first layer reads %d columns, the batch has %d" % (first.in_features, max(sel.L - 1, 0) * col_stride + rows.n))
        x = ops.rowsel_conv(self.first_transposed() if first_t is None else first_t, rows, sel, first.bias, relu=True, col_stride=col_stride)
        for i in range(1, self.layer_num):
            x = F.relu(self.layer_list[i](x))
        return x


class _AutoEncoder(nn.Module):
    """what DynAE and DynGEM share: encode a batch of rows, decode an embedding"""

    def encode(self, batch, first_t=None):
        batch = _as_batch(batch)
        if batch is None:
            raise TypeError("a RowBatch or (SnapshotRows, idx) expected")
        return self.encoder.forward_rows(batch.rows, batch.idx, batch.rows.n, first_t)

    def decode(self, hx, pre_activation=False):
        return self.decoder(hx, pre_activation=pre_activation)

    def forward(self, x):
        hx = self.encoder(x) if isinstance(x, torch.Tensor) else self.encode(x)
        return hx, self.decoder(hx)


class DynAE(_AutoEncoder):
    def __init__(self, input_dim, output_dim, look_back=3, n_units=None, bias=True, **kwargs):
        super(DynAE, self).__init__()
        self.input_dim = input_dim
        self.output_dim = output_dim
        self.look_back = look_back
        self.bias = bias
        self.method_name = 'DynAE'

        self.encoder = MLP(input_dim * look_back, output_dim, n_units, bias=bias)
        self.decoder = MLP(output_dim, input_dim, n_units[::-1], bias=bias)


class RegularizationLoss(nn.Module):
    def __init__(self, nu1, nu2):
        super(RegularizationLoss, self).__init__()
        self.nu1 = nu1
        self.nu2 = nu2

    @staticmethod
    def get_weight(model):
        return [(name, param) for name, param in model.named_parameters() if 'weight' in name]

    def forward(self, model):
        weight_list = self.get_weight(model)
        if self.nu1 == 0. and self.nu2 == 0.:
            device = weight_list[0][1].device if weight_list else None
            return torch.zeros(1, device=device)
        weight_num = len(weight_list)
        l1_reg_loss, l2_reg_loss = 0, 0
        for name, weight in weight_list:
            if self.nu1 > 0:
                l1_reg_loss = l1_reg_loss + torch.norm(weight, p=1)
            if self.nu2 > 0:
                l2_reg_loss = l2_reg_loss + torch.norm(weight, p=2)
        return self.nu1 * l1_reg_loss / weight_num + self.nu2 * l2_reg_loss / weight_num


class DynGraph2VecLoss(nn.Module):
    def __init__(self, beta, nu1, nu2):
        super(DynGraph2VecLoss, self).__init__()
        self.beta = beta
        self.regularization = RegularizationLoss(nu1, nu2)

    def forward(self, model, input_list):
        """[x_reconstruct, x_real, y_penalty] as dense tensors (the reference's expression), or [z, batch] with z the decoder's
        pre-activation [B, N] and batch the RowBatch it came from: the kernel path.  z is consumed: its memory receives the gradient.
        A decoder that ends in an LSTM (DynRNN) hands over its prediction itself, the last h, which has no ReLU; ops.lstm_layer's
        backward does not read that h, so it may be consumed too."""
        if len(input_list) == 2:
            from .dynrnn import MLLSTM
            z, batch = input_list
            relu = not isinstance(getattr(model, 'decoder', None), MLLSTM)
            reconstruct_loss = ops.wrecon_loss(z, batch.rows, batch.tgt, batch.beta, divide=False, scale=1.0 / z.shape[0], relu=relu,
                                               overwrite=True)
        else:
            assert len(input_list) == 3
            x_reconstruct, x_real, y_penalty = input_list
            ops._need_cuda(x_reconstruct, x_real, y_penalty)
            reconstruct_loss = torch.mean(torch.sum(torch.square((x_reconstruct - x_real) * y_penalty), dim=1))
        return reconstruct_loss + self.regularization(model)


class BatchGenerator:
    def __init__(self, node_list, batch_size, look_back, beta, shuffle=True, has_cuda=False):
        self.node_list = node_list
        self.node_num = len(node_list)
        self.batch_size = batch_size
        self.look_back = look_back
        self.beta = beta
        self.shuffle = shuffle
        self.has_cuda = has_cuda

    def batch_num(self, graph_list):
        rows = _as_rows(graph_list, need_device=False)
        train_size = rows.T - self.look_back
        assert train_size > 0
        return -(-(self.node_num * train_size) // self.batch_size)

    def generate(self, graph_list):
        """yields RowBatch after RowBatch: record r = (graph g, node v) reads rows (g + s) N + v, s < look_back, and targets row
        (g + look_back) N + v.  graph_list: an ops.SnapshotRows, or scipy matrices (index arithmetic only: such a batch has no device
        side)."""
        from ..embedding import epoch_order
        rows = _as_rows(graph_list, need_device=False)
        assert rows.n == self.node_num
        train_size = rows.T - self.look_back
        assert train_size > 0
        all_node_num = self.node_num * train_size
        batch_num = -(-all_node_num // self.batch_size)
        node_indices = epoch_order(all_node_num, self.shuffle).numpy()
        counter = 0
        while True:
            rec = node_indices[self.batch_size * counter: min(all_node_num, self.batch_size * (counter + 1))]
            idx = np.full((self.batch_size, self.look_back), -1, dtype=np.int64)
            tgt = np.full((self.batch_size,), -1, dtype=np.int64)
            graph_idx, node_idx = rec // self.node_num, rec % self.node_num
            for step in range(self.look_back):
                idx[:len(rec), step] = (graph_idx + step) * self.node_num + node_idx
            tgt[:len(rec)] = (graph_idx + self.look_back) * self.node_num + node_idx
            counter += 1
            yield RowBatch(rows if isinstance(rows, ops.SnapshotRows) else None, idx, tgt, self.beta)
            if counter == batch_num:
                node_indices = epoch_order(all_node_num, self.shuffle).numpy()
                counter = 0


class BatchPredictor:
    def __init__(self, node_list, batch_size, has_cuda=False):
        self.node_list = node_list
        self.node_num = len(node_list)
        self.batch_size = batch_size
        self.has_cuda = has_cuda

    def predict(self, model, graph_list, need_pred=True, fused=True, start=0):
        """(embedding [N, d], x_pred [N, N] or None) from the snapshots start .. of graph_list (all of them are the look_back inputs)"""
        rows = _as_rows(graph_list, next(model.parameters()).device)
        look_back = rows.T - start
        name = getattr(model, 'method_name', 'DynAE')
        emb, pred = [], []
        with torch.no_grad():
            if not fused:
                first_t = None
            elif name in ('DynRNN', 'DynAERNN'):
                first_t = model.first_transposed()
            else:
                first_t = model.encoder.first_transposed()                      # one transposed copy for all batches
            for lo in range(0, self.node_num, self.batch_size):
                nodes = np.arange(lo, min(self.node_num, lo + self.batch_size), dtype=np.int64)
                idx = (start + np.arange(look_back, dtype=np.int64))[None, :] * rows.n + nodes[:, None]
                if name == 'DynRNN':                                            # the reconstruction comes from the sequence, not from hx
                    seq, hx = model.encode((rows, idx), first_t) if fused else model.encoder(rows.dense(idx))
                    emb.append(hx)
                    if need_pred:
                        pred.append(model.decode(seq) if fused else model.decoder(seq)[1])
                    continue
                if name == 'DynAERNN':
                    hx = model.encode((rows, idx), first_t) if fused else model.rnn_encoder(model.ae_encoder(rows.dense(idx)))[1]
                elif fused:
                    hx = model.encode((rows, idx), first_t)
                else:
                    hx = model.encoder(rows.dense(idx).reshape(len(nodes), -1))
                emb.append(hx)
                if need_pred:
                    pred.append(model.decode(hx))
        return torch.cat(emb, dim=0), (torch.cat(pred, dim=0) if need_pred else None)


class DynamicEmbedding(object):
    def __init__(self, base_path, origin_folder, embedding_folder, node_list, model, loss, batch_generator, batch_predictor, model_folder="model",
                 has_cuda=False):
        if not has_cuda:
            raise CtgcnHipError("DynamicEmbedding runs on the MI355X only (has_cuda=True); there is no CPU fallback")
        from . import dynaernn, dyngem, dynrnn
        if not isinstance(model, (DynAE, dyngem.DynGEM, dynrnn.DynRNN, dynaernn.DynAERNN)):
            raise NotImplementedError("DynamicEmbedding trains ctgcn_amd.baseline.DynGEM and ctgcn_amd.baseline.DynAE, DynRNN and DynAERNN, got %s"
                                      % type(model).__name__)
        self.base_path = base_path
        self.origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
        self.embedding_base_path = os.path.abspath(os.path.join(base_path, embedding_folder))
        self.model_base_path = os.path.abspath(os.path.join(base_path, model_folder))
        self.has_cuda = has_cuda
        self.device = torch.device('cuda', torch.cuda.current_device())
        self.model = model
        self.loss = loss
        self.file_sep = '\t'
        self.full_node_list = node_list
        self.node_num = len(node_list)
        self.timestamp_list = sorted(os.listdir(self.origin_base_path))
        self.batch_generator = batch_generator
        self.batch_predictor = batch_predictor
        self.loss_history = []              # per epoch, the loss of each of its batches
        os.makedirs(self.embedding_base_path, exist_ok=True)
        os.makedirs(self.model_base_path, exist_ok=True)

        assert batch_generator.batch_size == batch_predictor.batch_size
        assert batch_generator.node_num == batch_predictor.node_num

    def prepare(self, load_model, model_file, lr=1e-3, weight_decay=0.):
        if load_model:
            model_path = os.path.join(self.model_base_path, model_file)
            if os.path.exists(model_path):
                self.model.load_state_dict(torch.load(model_path, map_location='cpu'))
                self.model.eval()
        self.model = self.model.to(self.device)
        self.loss = self.loss.to(self.device)
        optimizer = torch.optim.Adam(self.model.parameters(), lr=lr, weight_decay=weight_decay)
        optimizer.zero_grad()
        return self.model, self.loss, optimizer

    def get_batch_info(self, adj_list, model):
        batch_size = self.batch_generator.batch_size
        batch_num = self.batch_generator.batch_num(adj_list)
        train_size = 0 if model.method_name == 'DynGEM' else adj_list.T - self.batch_generator.look_back
        return batch_size, batch_num, train_size

    @staticmethod
    def get_model_res(model, generator, fused=True):
        """the loss's input list of the generator's next batch: the kernel path, or the reference's dense tensors"""
        batch = next(generator)
        if model.method_name == 'DynGEM':
            if fused:
                hx = model.encode(batch)                                   # both sides as one stacked batch of 2 B rows
                return [model.decode(hx, pre_activation=True), hx, batch]
            [xi_batch, xj_batch], [yi_batch, yj_batch, value_batch] = batch.dense_sides()
            hx_i, xi_pred = model(xi_batch)
            hx_j, xj_pred = model(xj_batch)
            return [xi_pred, xi_batch, yi_batch, xj_pred, xj_batch, yj_batch, hx_i, hx_j, value_batch]
        if fused:
            if model.method_name == 'DynRNN':                              # the decoder reads the sequence; its last h is the prediction
                return [model.decode(model.encode(batch)[0]), batch]
            return [model.decode(model.encode(batch), pre_activation=True), batch]
        x_pre_batches, x_cur_batch, y_batch = batch.dense()
        if model.method_name != 'DynAE':                                   # DynAE alone takes the window flattened
            x_pre_batches = x_pre_batches.view(x_pre_batches.shape[0], batch.idx.L, -1)
        _, x_pred_batch = model(x_pre_batches)
        return [x_pred_batch, x_cur_batch, y_batch]

    def learn_embedding(self, adj_list, epoch=50, lr=1e-3, idx=0, weight_decay=0., model_file='dynAE', load_model=False, export=True, fused=True):
        """reference baseline/dynAE.py:293-328; adj_list: the window's scipy matrices or an ops.SnapshotRows"""
        model, loss_model, optimizer = self.prepare(load_model, model_file, lr=lr, weight_decay=weight_decay)
        rows = _as_rows(adj_list, self.device)
        batch_size, batch_num, train_size = self.get_batch_info(rows, model)
        self.loss_history = []
        st = time.time()
        model.train()
        for i in range(epoch):
            t1 = time.time()
            losses = []
            for j in range(batch_num):
                generator = self.batch_generator.generate(rows)             # a fresh generator per batch, as the reference makes one
                loss = loss_model(model, self.get_model_res(model, generator, fused))
                loss.backward()
                losses.append(loss.detach().reshape(()))
                if j == batch_num - 1:                                      # gradient accumulation over the epoch's batches
                    optimizer.step()
                    model.zero_grad()
            self.loss_history.append(torch.stack(losses).tolist())
            print('epoch', i + 1, ', batches =', batch_num, ', loss:', sum(self.loss_history[-1]), ', cost time: ', time.time() - t1, ' seconds!')
        model.eval()
        embedding_mat, _ = self.batch_predictor.predict(model, rows, need_pred=False, fused=fused, start=train_size)
        cost_time = time.time() - st
        if export:
            save_embedding(embedding_mat, self.timestamp_list, idx, self.embedding_base_path, self.full_node_list, sep=self.file_sep)
        if model_file:
            torch.save(model.state_dict(), os.path.join(self.model_base_path, model_file))
        del embedding_mat
        torch.cuda.empty_cache()
        return cost_time


def dyngem_embedding(method, args):
    """The reference's driver of DynGEM, DynAE, DynRNN and DynAERNN (baseline/dynAE.py:331-425) from a method's config section: one
    window per idx in the configured range, covering the snapshots idx - duration + 1 .. idx, with a fresh model, loss, generator and
    predictor each; with load_model a window starts from the checkpoint the previous one wrote (DynGEM's warm start).  The window's
    scipy matrices go to DynamicEmbedding.learn_embedding as the loader returns them.  The optional `seed` key (not the reference's)
    seeds torch, numpy.random and random before each window."""
    assert method in ['DynGEM', 'DynAE', 'DynRNN', 'DynAERNN']
    import pandas as pd
    from ..helper import DataLoader
    from ..train import resolve_range, seed_everything, write_time_file
    from .dynaernn import DynAERNN
    from .dyngem import DynGEM, DynGEMBatchGenerator, DynGEMBatchPredictor, DynGEMLoss
    from .dynrnn import DynRNN
    model_dict = {'DynGEM': DynGEM, 'DynAE': DynAE, 'DynRNN': DynRNN, 'DynAERNN': DynAERNN}

    base_path = args['base_path']
    origin_folder = args['origin_folder']
    embedding_folder = args['embed_folder']
    model_folder = args['model_folder']
    model_file = args['model_file']
    file_sep = args['file_sep']
    duration = args['duration']
    embed_dim = args['embed_dim']
    has_cuda = args['has_cuda']
    epoch = args['epoch']
    lr = args['lr']
    batch_size = args['batch_size']
    load_model = args['load_model']
    shuffle = args['shuffle']
    export = args['export']
    record_time = args['record_time']
    seed = args.get('seed', None)

    n_units, ae_units, rnn_units = [], [], []
    look_back, alpha = 0, 0
    if method in ['DynGEM', 'DynAE', 'DynRNN']:
        n_units = args['n_units']
    else:
        ae_units = args['ae_units']
        rnn_units = args['rnn_units']
    if method in ['DynAE', 'DynRNN', 'DynAERNN']:
        look_back = args['look_back']
        assert look_back > 0
    else:
        alpha = args['alpha']
    beta = args['beta']
    nu1 = args['nu1']
    nu2 = args['nu2']
    bias = args['bias']

    origin_base_path = os.path.abspath(os.path.join(base_path, origin_folder))
    max_time_num = len(os.listdir(origin_base_path))
    node_list = pd.read_csv(os.path.abspath(os.path.join(base_path, args['node_file'])), names=['node'])['node'].tolist()
    node_num = len(node_list)
    data_loader = DataLoader(node_list, max_time_num, has_cuda=has_cuda)
    start_idx, end_idx = resolve_range(max_time_num, args['start_idx'], args['end_idx'])

    if method == 'DynGEM':
        assert duration == 1
    assert start_idx + 1 - duration >= 0
    assert duration > look_back

    t1 = time.time()
    time_list = []
    print('start ' + method + ' embedding!')
    for idx in range(start_idx, end_idx):
        print('idx = ', idx)
        seed_everything(seed)
        # the raw adjacency matrices are the input: no normalisation, no self loops
        adj_list = data_loader.get_date_adj_list(origin_base_path, start_idx=idx - duration + 1, duration=duration, sep=file_sep,
                                                 normalize=False, add_eye=False, data_type='matrix')
        model = model_dict[method](input_dim=node_num, output_dim=embed_dim, look_back=look_back, n_units=n_units, ae_units=ae_units,
                                   rnn_units=rnn_units, bias=bias)
        if method == 'DynGEM':
            loss = DynGEMLoss(alpha=alpha, beta=beta, nu1=nu1, nu2=nu2)
            batch_generator = DynGEMBatchGenerator(node_list=node_list, batch_size=batch_size, beta=beta, shuffle=shuffle, has_cuda=has_cuda)
            batch_predictor = DynGEMBatchPredictor(node_list=node_list, batch_size=batch_size, has_cuda=has_cuda)
        else:
            loss = DynGraph2VecLoss(beta=beta, nu1=nu1, nu2=nu2)
            batch_generator = BatchGenerator(node_list=node_list, batch_size=batch_size, look_back=look_back, beta=beta, shuffle=shuffle,
                                             has_cuda=has_cuda)
            batch_predictor = BatchPredictor(node_list=node_list, batch_size=batch_size, has_cuda=has_cuda)
        trainer = DynamicEmbedding(base_path=base_path, origin_folder=origin_folder, embedding_folder=embedding_folder, node_list=node_list,
                                   model=model, loss=loss, batch_generator=batch_generator, batch_predictor=batch_predictor,
                                   model_folder=model_folder, has_cuda=has_cuda)
        time_list.append(trainer.learn_embedding(adj_list, epoch=epoch, lr=lr, idx=idx, model_file=model_file, load_model=load_model,
                                                 export=export))

    if record_time:
        write_time_file(base_path, method, time_list)
    print('finish ' + method + ' embedding! cost time: ', time.time() - t1, ' seconds!')
