"""CoreDiffusion and MLP layers with the reference's constructor/forward signatures and state_dict keys
(reference layers.py:9-63 and :67-106), running the sparse aggregation on the HIP kernel.

The aggregation (reference layers.py:41-48 + the stack/transpose of :58) runs in ctgcn_core_aggregate_f32; the
core-axis GRU/LSTM + sum over cores + LayerNorm (layers.py:59-62) in the fused recurrence kernels when hidden = 128
(ops.gru_sequence / ops.lstm_sequence), at other widths in library GEMMs plus one fused HIP cell pass per step (ops.gru_layer /
ops.lstm_layer), and otherwise (several layers, bidirectional, proj_size) in the PyTorch-ROCm modules, chunked over rows.
"""
import torch
from torch import nn
from torch.nn import functional as F

from . import ops
from .core_adj import CoreAdj

_RNN = {"GRU": nn.GRU, "LSTM": nn.LSTM}
_RNN_MAX_ELEMS = 1 << 29     # MIOpen's RNN indexes its gate workspace with 32-bit ints: keep batch*seq*4*hidden below 2^31


def rnn_reduce_norm(rnn, norm, seq, reduce_sum, out=None, resident_backward=True):
    """norm(rnn(seq).sum(1)) or norm(rnn(seq)).  GRU(hidden=128) and LSTM(hidden=128): fused HIP kernels, forward and backward.
    A single-layer, unidirectional, batch_first GRU of any other width, or such an LSTM without projection: library GEMMs and one
    fused HIP cell pass per step (ops.gru_layer / ops.lstm_layer, forward and backward), then norm as a torch module; CTGCN_RNN_CELL=0
    sends these to the PyTorch-ROCm modules instead.  Everything else (several layers, bidirectional, proj_size) goes through the
    PyTorch-ROCm modules.  out (inference only, reduce_sum): a [rows, hidden] strided view that receives the result.
    resident_backward: see ops.gru_sequence (GCRN passes False)."""
    if out is not None and torch.is_grad_enabled() and (seq.requires_grad or any(p.requires_grad for p in rnn.parameters())):
        out = None                                   # training: autograd needs its own tensors
    if ops.gru_fused_ok(rnn, seq):
        if out is not None and reduce_sum:
            return ops.gru_sequence(rnn, seq, norm, reduce_sum, out=out)
        res = ops.gru_sequence(rnn, seq, norm, reduce_sum, resident_backward=resident_backward)
    elif ops.lstm_fused_ok(rnn, seq):
        res = ops.lstm_sequence(rnn, seq, norm, reduce_sum)
    elif ops.rnn_cell_ok(rnn, seq):
        res = norm(rnn_cells_over_rows(rnn, seq, reduce_sum))
    else:
        res = norm(rnn_over_rows(rnn, seq, reduce_sum))
    if out is not None:
        out.copy_(res)
        return out
    return res


def rnn_cells_over_rows(rnn, seq, reduce_sum):
    """rnn(seq)[0], or its sum over the steps, for what ops.rnn_cell_ok admits: the GRU through ops.gru_layer, which chunks the rows
    and sums inside its cell pass; the LSTM through ops.lstm_layer in row chunks of the same bound (ops._GI_MAX_ELEMS elements of
    gates), summed chunk by chunk.  No MIOpen call, so its 2^31 limit plays no part."""
    bias = lambda name: getattr(rnn, name) if rnn.bias else None  # noqa: E731
    args = (rnn.weight_ih_l0, rnn.weight_hh_l0, bias("bias_ih_l0"), bias("bias_hh_l0"))
    if isinstance(rnn, nn.GRU):
        return ops.gru_layer(seq, *args, reduce_sum=reduce_sum)
    rows, steps, _ = seq.shape
    chunk = max(1, ops._GI_MAX_ELEMS // max(1, steps * 4 * rnn.hidden_size))
    parts = []
    for lo in range(0, max(rows, 1), chunk):
        out = ops.lstm_layer(seq[lo:lo + chunk], *args)
        parts.append(out.sum(dim=1) if reduce_sum else out)
    return parts[0] if len(parts) == 1 else torch.cat(parts, 0)


def rnn_over_rows(rnn, seq, reduce_sum):
    """rnn(seq)[0] for seq [rows, steps, feat], evaluated in row chunks (rows are independent sequences, so this is
    exact).  MIOpen rejects (miopenStatusBadParm) problems whose gate buffers exceed 2^31 elements — 1M nodes x 8
    cores x 3*128 already does.  With reduce_sum the per-row sum over steps is taken chunk by chunk, so the
    [rows, steps, hidden] output of the full problem is never materialised."""
    rows, steps, _ = seq.shape
    gates = 4 if isinstance(rnn, nn.LSTM) else 3
    chunk = max(1, _RNN_MAX_ELEMS // max(1, steps * gates * rnn.hidden_size))
    if rows <= chunk:
        out = rnn(seq)[0]
        return out.sum(dim=1) if reduce_sum else out
    parts = []
    for lo in range(0, rows, chunk):
        out = rnn(seq[lo:lo + chunk])[0]
        parts.append(out.sum(dim=1) if reduce_sum else out)
    return torch.cat(parts, 0)
_adj_cache = {}


def as_core_adj(adj_list, device):
    """Accept what the reference's callers pass: a CoreAdj (our loader) or a python list of torch sparse
    matrices (reference loader, helper.py:51-82).  Lists are fused once and cached by identity."""
    if isinstance(adj_list, CoreAdj):
        return adj_list if adj_list.device == device else adj_list.to(device)    # .to() keeps the moved copy on the source object
    key = tuple((id(a), a._values().data_ptr() if a.is_sparse else a.data_ptr()) for a in adj_list) + (str(device),)
    hit = _adj_cache.get(key)
    if hit is None:
        if len(_adj_cache) > 64:
            _adj_cache.clear()
        # the entry keeps the source tensors alive, so their ids cannot be recycled while the entry exists
        hit = _adj_cache[key] = (CoreAdj.from_matrices(list(adj_list), device=device), list(adj_list))
    return hit[0]


_gcn_adj_cache = {}


def as_gcn_adj(adj, device, symmetric=True):
    """Accept what an EvolveGCN / GCN caller passes: an ops.GcnAdj (prebuilt) or a torch sparse matrix (the loader's normalised
    adjacency, helper.get_date_adj_list(normalize=True)).  A tensor is converted once and cached by identity.  symmetric=True
    (EvolveGCN: ops.gcn_layer's backward reads the same CSR) checks A = A^T on the device and raises ValueError otherwise;
    symmetric=False (GCN / GCRN: ops.gcn_conv, row-normalised matrices) skips the check and is cached separately."""
    if isinstance(adj, ops.GcnAdj):
        if adj.device != torch.device(device):
            raise ValueError("GcnAdj on %s but features on %s" % (adj.device, device))
        return adj
    if not (isinstance(adj, torch.Tensor) and adj.is_sparse):
        raise TypeError("a GcnAdj or a torch sparse matrix expected, got %s" % type(adj).__name__)
    key = (id(adj), adj._values().data_ptr(), str(device), bool(symmetric))
    hit = _gcn_adj_cache.get(key)
    if hit is None:
        if len(_gcn_adj_cache) > 256:
            _gcn_adj_cache.clear()
        # the entry keeps the source tensor alive, so its id cannot be recycled while the entry exists
        hit = _gcn_adj_cache[key] = (ops.GcnAdj.from_sparse_tensor(adj, device, check_symmetric=bool(symmetric)), adj)
    return hit[0]


def as_pool_adj(adj, kind, self_loop=False):
    """The matrix a GIN / GraphSAGE pooling step reads, derived from a GcnAdj once and cached on it (so it lives exactly as long as
    the as_gcn_adj entry it came from).  kind:
      'sum', 'average'                   the raw adjacency's weights, plus a unit diagonal with self_loop (added to a stored one); 'average'
                                         divides each row by its weighted sum (ops.gcn_normalize(row_norm=True); an empty row stays 0)
      'pattern-sum', 'pattern-average'   the pattern alone: values 1, or 1 / the number of entries; with self_loop the node joins its
                                         own set, as a set (a stored self loop is not counted twice)"""
    cache = adj.__dict__.setdefault("_pool", {})
    hit = cache.get((kind, bool(self_loop)))
    if hit is not None:
        return hit
    n, dev = adj.n, adj.device
    rows, cols = adj._rows(), adj.col.to(torch.int64)
    eye = torch.arange(n, device=dev)
    if kind in ("sum", "average"):
        vals = adj.val
        if self_loop:
            rows, cols, vals = torch.cat((rows, eye)), torch.cat((cols, eye)), torch.cat((vals, torch.ones(n, device=dev)))
        t = torch.sparse_coo_tensor(torch.stack((rows, cols)), vals, torch.Size((n, n)))
        out = ops.GcnAdj.from_sparse_tensor(t, dev, long_threshold=adj.long_threshold, check_symmetric=False)
        if kind == "average":
            out.val = ops.gcn_normalize(out.row_ptr, out.col, out.val, row_norm=True)
    elif kind in ("pattern-sum", "pattern-average"):
        keys = rows * n + cols
        if self_loop:
            keys = torch.unique(torch.cat((keys, eye * (n + 1))))
        else:
            keys = torch.unique(keys)                              # sorted: row-major order, columns ascending
        rows, cols = torch.div(keys, n, rounding_mode="floor"), keys % n
        counts = torch.bincount(rows, minlength=n)
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        row_ptr[1:] = counts.cumsum(0)
        vals = torch.ones(keys.numel(), dtype=torch.float32, device=dev)
        if kind == "pattern-average":
            vals = (1.0 / counts.to(torch.float64))[rows].to(torch.float32)
        out = ops.GcnAdj(row_ptr.to(torch.int32), cols.to(torch.int32), vals, adj.long_threshold)
    else:
        raise ValueError("unknown pooling matrix %r" % (kind,))
    cache[kind, bool(self_loop)] = out
    return out


_identity_cache = {}


def _is_identity(sp_tensor):
    """True iff the sparse COO tensor is exactly the N x N identity (what get_feature_list builds for one-hot
    node features).  Checked once per tensor (one small reduction + host read), then cached by identity; the
    cache entry holds the tensor, so its id cannot be recycled while the entry exists."""
    key = (id(sp_tensor), sp_tensor._values().data_ptr())
    entry = _identity_cache.get(key)
    if entry is None:
        n, m = sp_tensor.shape
        idx, val = sp_tensor._indices(), sp_tensor._values()
        flag = bool(n == m and val.numel() == n and idx.shape[0] == 2
                    and bool(((idx[0] == idx[1]) & (val == 1)).all())
                    and bool((idx[0].sort().values == torch.arange(n, device=idx.device)).all()))
        if len(_identity_cache) > 256:
            _identity_cache.clear()
        entry = _identity_cache[key] = (flag, sp_tensor)
    return entry[0]


class CoreDiffusion(nn.Module):
    """K-core diffusion layer: H_j = relu(sum_{i<=j} A_i x), RNN over j, sum over j, LayerNorm."""

    def __init__(self, input_dim, output_dim, core_num=1, bias=True, rnn_type='GRU'):
        super().__init__()
        assert rnn_type in _RNN
        self.input_dim, self.output_dim = input_dim, output_dim
        self.core_num, self.bias, self.rnn_type = core_num, bias, rnn_type
        # `linear` is never used in forward (nor in the reference, layers.py:24) but is part of the checkpoint schema
        self.linear = nn.Linear(input_dim, output_dim)
        self.rnn = _RNN[rnn_type](input_size=input_dim, hidden_size=output_dim, num_layers=1, bias=bias, batch_first=True)
        self.norm = nn.LayerNorm(output_dim)

    def aggregate(self, x, adj_list, gather_bias=None):
        """[N, K, input_dim] = all K rectified cumulative aggregations, one kernel launch."""
        if gather_bias is None:
            return ops.core_aggregate(x, as_core_adj(adj_list, x.device), relu=True)
        return ops.core_aggregate(x, as_core_adj(adj_list, x.device), relu=True, gather_bias=gather_bias)

    def forward(self, x, adj_list, out=None, gather_bias=None):
        """out (optional, inference): a [N, output_dim] view (unit column stride) that receives the result.
        gather_bias (optional, [input_dim]): x is the first Linear's weight stored by input row (ops.to_gather_layout) and the layer's
        input is x + gather_bias = Linear(one-hot features), which the aggregation kernels form row by row in registers."""
        if torch.is_tensor(x) and not x.is_sparse and x.is_cuda:
            adj = as_core_adj(adj_list, x.device)
            if ops.aggregate_split_ok(self.rnn, x, adj):
                # inference, GRU input projection on the split GEMM (d_in != 128): the aggregation writes the GEMM's fp16 operand
                # planes, the fp32 [N, K, input_dim] tensor is never materialised
                return ops.core_diffusion_split(x, adj, self.rnn, self.norm, out=out, gather_bias=gather_bias)
            if torch.is_grad_enabled() and ops.core_diffusion_fused_ok(self.rnn, self.norm, x, adj):
                # training, d_in = hidden = 128: the inference forward under autograd (planes + row plan kept for the backward kernels)
                return ops.core_diffusion_fused(x, adj, self.rnn, self.norm, gather_bias=gather_bias)
        seq = self.aggregate(x, adj_list, gather_bias)            # [batch = N, seq = K, feat]
        return rnn_reduce_norm(self.rnn, self.norm, seq, reduce_sum=True, out=out)


class MLP(nn.Module):
    """Stack of Linear layers, SELU after each when activate_type == 'N' (reference layers.py:67-106).
    Key names: `linear.*` for one layer, `linears.{i}.*` otherwise."""

    def __init__(self, input_dim, hidden_dim, output_dim, layer_num, bias=True, activate_type='N'):
        super().__init__()
        assert activate_type in ['L', 'N']
        assert layer_num > 0
        self.input_dim, self.hidden_dim, self.output_dim = input_dim, hidden_dim, output_dim
        self.layer_num, self.bias, self.activate_type = layer_num, bias, activate_type
        if layer_num == 1:
            self.linear = nn.Linear(input_dim, output_dim, bias=bias)
        else:
            widths = [input_dim] + [hidden_dim] * (layer_num - 1) + [output_dim]
            self.linears = nn.ModuleList(nn.Linear(a, b, bias=bias) for a, b in zip(widths[:-1], widths[1:]))

    @staticmethod
    def _apply_linear(layer, h, selu=False, static_x=False):
        """layer(h), followed by F.selu when asked (fused into the split GEMM's epilogue on that path)"""
        out, fused = MLP._linear(layer, h, selu, static_x)
        return F.selu(out) if (selu and not fused) else out

    @staticmethod
    def _linear(layer, h, selu, static_x=False):
        """(layer(h), whether the activation was already applied)"""
        if h.is_sparse:          # one-hot / sparse features (helper.py:161-172)
            if _is_identity(h):  # Linear(I) = W^T + b: one pass over W instead of an N x N SpMM
                if h.is_cuda and layer.weight.dtype == torch.float32:
                    return ops.linear_of_identity(layer.weight, layer.bias), False      # HIP transpose, forward and backward
                return (layer.weight.t() + layer.bias if layer.bias is not None else layer.weight.t().contiguous()), False
            out = torch.sparse.mm(h, layer.weight.t())
            return (out if layer.bias is None else out + layer.bias), False
        needs_grad = torch.is_grad_enabled() and (h.requires_grad or any(p.requires_grad for p in layer.parameters()))
        # a weight that one-hot forwards re-laid by input row (ops.to_gather_layout) meets dense features: a row-major copy, same products
        weight = layer.weight.contiguous() if ops.in_gather_layout(layer.weight) else layer.weight
        if not needs_grad and h.dim() == 2 and ops.linear_split_ok(h, weight):
            # fp32-accurate split GEMM on the 16-bit matrix cores (inference), SELU in its epilogue
            return ops.linear_split(h, weight, layer.bias, selu=selu, static_x=static_x), bool(selu)
        if needs_grad and h.dim() == 2 and ops.linear_train_enabled() and ops.linear_split_ok(h, weight) and ops.plane_cache_enabled() \
                and h.shape[0] >= 4096:
            # training: forward and dx on the same GEMM (ops._LinearSplit); small inputs stay with the library (launch-bound either way)
            return ops.linear_split_train(h, weight, layer.bias, static_x=static_x), False
        return (layer(h) if weight is layer.weight else F.linear(h, weight, layer.bias)), False

    def forward(self, x):
        stack = [self.linear] if self.layer_num == 1 else list(self.linears)
        selu = self.activate_type == 'N'
        if len(stack) > 1 and not (torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters()) or
                                                              (torch.is_tensor(x) and x.requires_grad))):
            # inference through dense layers: a hidden activation leaves its GEMM as the next GEMM's operand planes (ops.linear_chain_ok /
            # ctgcn_linear_packed_chain_f32) — no fp32 rows written, read back and split between two layers
            i = 0
            while i + 1 < len(stack) and ops.linear_chain_ok(x, stack[i].weight, stack[i + 1].weight):
                x = ops.linear_split(x, stack[i].weight, stack[i].bias, selu=selu, static_x=(i == 0 and ops.is_static(x)), planes_out=True)
                i += 1
            if i:
                x = ops.linear_split(x, stack[i].weight, stack[i].bias, selu=selu)       # the chain's last GEMM: fp32 rows
                stack = stack[i + 1:]
        for i, layer in enumerate(stack):
            # the first layer's operand is the module's input: when the caller has declared it static (ops.mark_static — node features
            # built once and passed to every forward, train.py:72-76, embedding.py:318; ctgcn_amd.helper.DataLoader does) its operand
            # planes are kept between calls (ops._PlaneCache, validated by the version counter)
            x = self._apply_linear(layer, x, selu=self.activate_type == 'N', static_x=(i == 0 and ops.is_static(x)))
        return x
