"""Torch-facing wrappers over the C ABI (include/ctgcn_hip.h).  PyTorch is plumbing here: it owns
device memory, streams and the autograd graph; every kernel is in libctgcn_hip.so.

All entry points require CUDA (ROCm) tensors and raise otherwise — there is no CPU path.
"""
import ctypes

import torch

from . import _lib
from ._lib import check, ptr


def _need_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise _lib.CtgcnHipError(
                "ctgcn_amd runs on MI355X only: got a %s tensor. Move inputs (features and CoreAdj) to the GPU; "
                "there is no CPU fallback." % t.device)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_launch_timer = None


def set_launch_timer(callback):
    """callback(name, start_event, end_event, meta) is invoked for every aggregation launch with HIP events
    recorded on the launch stream right before / after the kernel (bench.py's roofline measurement).
    None disables it (default)."""
    global _launch_timer
    _launch_timer = callback


class _timed(object):
    def __init__(self, name, **meta):
        self.name, self.meta = name, meta

    def __enter__(self):
        if _launch_timer is not None:
            self.start = torch.cuda.Event(enable_timing=True)
            self.end = torch.cuda.Event(enable_timing=True)
            self.start.record()
        return self

    def __exit__(self, *exc):
        if _launch_timer is not None and exc[0] is None:
            self.end.record()
            _launch_timer(self.name, self.start, self.end, self.meta)
        return False


def _i32(t):
    return t if t.dtype == torch.int32 and t.is_contiguous() else t.to(torch.int32).contiguous()


# ------------------------------------------------------------------------------------------- ingest
def edges_to_csr(src, dst, w, n):
    """Edge rows (file order; CUDA int32/int32/float32 or None) -> (row_ptr, col, val) of the symmetric,
    de-duplicated (last row wins), zero-diagonal CSR — reference utils.py:23-58 graph semantics, on the GPU."""
    _need_cuda(src, dst, w)
    lib = _lib.load()
    src, dst = _i32(src), _i32(dst)
    if w is not None:
        w = w if (w.dtype == torch.float32 and w.is_contiguous()) else w.to(torch.float32).contiguous()
    m = src.numel()
    dev = src.device
    row_ptr = torch.empty(n + 1, dtype=torch.int32, device=dev)
    col = torch.empty(2 * m, dtype=torch.int32, device=dev)
    val = torch.empty(2 * m, dtype=torch.float32, device=dev)
    nnz = ctypes.c_int64(0)
    with torch.cuda.device(dev):
        nbytes = lib.ctgcn_workspace_bytes(_lib.OP_INGEST, n, m, 0, 0)
        ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_edges_to_csr(n, m, ptr(src), ptr(dst), ptr(w), ptr(row_ptr), ptr(col), ptr(val), ctypes.byref(nnz),
                                     ptr(ws), nbytes, _stream()), "ctgcn_edges_to_csr")
    k = int(nnz.value)
    return row_ptr, col[:k], val[:k]


# ------------------------------------------------------------------------------------------- k-core
def kcore(row_ptr, col, level_cap=-1):
    """Core number of every vertex (reference: networkx.core_number at structure_generation.py:35).
    row_ptr/col: symmetric CSR structure on the GPU.  Returns (core int32[n] on the GPU, max core).
    level_cap = L > 0 peels only levels below L and reports every core number >= L as L."""
    _need_cuda(row_ptr, col)
    lib = _lib.load()
    row_ptr, col = _i32(row_ptr), _i32(col)
    n = row_ptr.numel() - 1
    core = torch.empty(n, dtype=torch.int32, device=row_ptr.device)
    if n == 0:
        return core, 0
    with torch.cuda.device(row_ptr.device):
        nbytes = lib.ctgcn_workspace_bytes(_lib.OP_KCORE, n, col.numel(), 0, 0)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=row_ptr.device)
        mx = ctypes.c_int32(0)
        check(lib.ctgcn_kcore_i32(n, ptr(row_ptr), ptr(col), ptr(core), ptr(ws), nbytes, int(level_cap), ctypes.byref(mx),
                                  _stream()), "ctgcn_kcore_i32")
    return core, int(mx.value)


def edge_levels(row_ptr, col, val, core, hist_len):
    """level[e] = min(core[row], core[col]) plus the per-level entry count / weight sum."""
    _need_cuda(row_ptr, col, val, core)
    lib = _lib.load()
    n = row_ptr.numel() - 1
    dev = row_ptr.device
    level = torch.empty(col.numel(), dtype=torch.int32, device=dev)
    count = torch.zeros(hist_len, dtype=torch.int64, device=dev)
    wsum = torch.zeros(hist_len, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        check(lib.ctgcn_edge_levels_i32(n, ptr(row_ptr), ptr(col), ptr(val), ptr(core), ptr(level), ptr(count), ptr(wsum),
                                        hist_len, _stream()), "ctgcn_edge_levels_i32")
    return level, count, wsum


def slot_reorder(row_ptr, col, val, level, table, K):
    _need_cuda(row_ptr, col, val, level, table)
    lib = _lib.load()
    n = row_ptr.numel() - 1
    col2, val2 = torch.empty_like(col), torch.empty_like(val)
    slot2 = torch.empty(col.numel(), dtype=torch.uint8, device=col.device)
    with torch.cuda.device(col.device):
        check(lib.ctgcn_slot_reorder(n, K, ptr(row_ptr), ptr(col), ptr(val), ptr(level), ptr(table), table.numel(),
                                     ptr(col2), ptr(val2), ptr(slot2), _stream()), "ctgcn_slot_reorder")
    return col2, val2, slot2


# ------------------------------------------------------------------------------------- plain SpMM
def spmm_csr(row_ptr, col, val, x, out=None, accumulate=False):
    """Y = A·X (or Y += A·X): one torch.sparse.mm of layers.py:43/45."""
    _need_cuda(row_ptr, col, val, x)
    lib = _lib.load()
    if x.dtype != torch.float32:
        raise TypeError("fp32 features expected")
    x = x if x.stride(-1) == 1 else x.contiguous()
    n = row_ptr.numel() - 1
    d = x.shape[1]
    if out is None:
        out = torch.empty(n, d, dtype=torch.float32, device=x.device)
        accumulate = False
    with torch.cuda.device(x.device):
        check(lib.ctgcn_spmm_csr_f32(n, d, ptr(row_ptr), ptr(col), ptr(val), ptr(x), x.stride(0), ptr(out), out.stride(0),
                                     1 if accumulate else 0, _stream()), "ctgcn_spmm_csr_f32")
    return out


def linear_gather_enabled():
    """CTGCN_LINEAR_GATHER=0: the first CoreDiffusion layer of a one-hot CTGCN-C branch reads a materialised Linear(I) = W^T + b
    (ctgcn_transpose_bias_f32 per snapshot and forward) instead of gathering the weight's rows and adding the bias in registers, and the
    weight keeps its [out, N] row-major memory — for A/B runs."""
    import os
    return os.environ.get("CTGCN_LINEAR_GATHER", "1") != "0"


def in_gather_layout(weight):
    """True when weight [out, N] is stored by input row: weight.t() is a contiguous [N, out] buffer (strides (1, out))."""
    return weight.dim() == 2 and weight.stride(1) != 1 and weight.t().is_contiguous()


def to_gather_layout(weight):
    """Re-lay the parameter weight [out, N] in place as the .t() view of a contiguous [N, out] buffer (one copy, once): same shape, same
    values, same state_dict entry; row v of the buffer is what Linear makes of one-hot node v before the bias.  load_state_dict
    (copy_ into the parameter), deepcopy and .to() (preserve_format) keep the layout; the optimizer's per-element updates do not see it."""
    if weight.dim() != 2 or weight.t().is_contiguous():
        return weight
    with torch.no_grad():
        weight.data = weight.detach().t().contiguous().t()
    return weight


def _transpose_bias(src, bias):
    """out[n, d] = src[d, n]^T + bias[d] (bias may be None), row-major, one pass (ctgcn_transpose_bias_f32)"""
    lib = _lib.load()
    d, n = src.shape
    if in_gather_layout(src):          # stored by input row already (to_gather_layout): the same fp32 add per element, no transpose
        return src.t() + bias if bias is not None else src.t().clone()
    w = src if src.stride(1) == 1 else src.contiguous()
    out = torch.empty(n, d, dtype=torch.float32, device=src.device)
    with torch.cuda.device(src.device):
        check(lib.ctgcn_transpose_bias_f32(n, d, ptr(w), w.stride(0), ptr(bias.contiguous() if bias is not None else None),
                                           ptr(out), out.stride(0), _stream()), "ctgcn_transpose_bias_f32")
    return out


class _LinearOfIdentity(torch.autograd.Function):
    """weight^T + bias with autograd: d weight = (d out)^T is the same transpose the other way (the framework accumulates it through a
    strided copy at 0.4 TB/s — 2.4 ms per 1 M x 128 snapshot, and its forward leaves a column-major tensor the aggregation has to copy)."""

    @staticmethod
    def forward(ctx, weight, bias):
        ctx.has_bias = bias is not None
        return _transpose_bias(weight.detach(), None if bias is None else bias.detach())

    @staticmethod
    def backward(ctx, dout):
        if dout.shape[0] > 64 * 65535:                       # beyond the transpose kernel's grid: the framework's strided copy
            dw = dout.t().contiguous()
        else:
            dw = _transpose_bias(dout if dout.stride(1) == 1 else dout.contiguous(), None)  # [d, n] = dout[n, d]^T
        return dw, (dout.sum(0) if ctx.has_bias else None)


def linear_of_identity(weight, bias):
    """nn.Linear(weight, bias) applied to the N x N identity (one-hot node features): [N, out] = weight^T + bias, written
    row-major in one pass (weight.t() + bias in torch yields a column-major tensor that the next layer has to copy); differentiable."""
    _need_cuda(weight)
    if torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad)):
        return _LinearOfIdentity.apply(weight, bias)
    return _transpose_bias(weight.detach(), None if bias is None else bias.detach())


# -------------------------------------------------------------------- CoreDiffusion aggregation
def _hub_pieces(lib, adj, long_rows, slots, d, device, transposed=False):
    """(hub_split, workspace, bytes) for hub rows long enough to be cut into pieces (several blocks per row + a fixed-order second pass)"""
    split = adj.hub_split(transposed) if long_rows is not None else 1
    if split <= 1:
        return 1, None, 0
    nbytes = int(lib.ctgcn_hub_workspace_bytes(long_rows.numel(), split, slots, d))
    return split, torch.empty(nbytes, dtype=torch.uint8, device=device), nbytes


def _check_gather_bias(x, gather_bias):
    """the operand of the *_bias_f32 entry points: x [n, d] dense rows (a Linear weight stored by input row), gather_bias fp32 [d]"""
    if not x.is_contiguous():
        raise ValueError("gather_bias goes with dense [n, d] rows (a weight in gather layout), got strides %s" % (tuple(x.stride()),))
    if gather_bias.dtype != torch.float32 or gather_bias.shape != (x.shape[1],) or gather_bias.device != x.device or not gather_bias.is_contiguous():
        raise ValueError("gather_bias must be a contiguous fp32 [%d] vector on %s" % (x.shape[1], x.device))


def _aggregate_fwd(adj, x, relu, gather_bias=None):
    """gather_bias [d] (optional): the operand rows are x[row] + gather_bias, added in registers (ctgcn_core_aggregate_bias_f32)"""
    lib = _lib.load()
    n, d = x.shape
    H = torch.empty(n, adj.K, d, dtype=torch.float32, device=x.device)
    flags = adj.flags | (_lib.F_RELU if relu else 0)
    with torch.cuda.device(x.device), _timed("agg_fwd", n=n, d=d, K=adj.K, nnz=adj.nnz):
        long_rows = adj.long_rows()
        split, hub_ws, hub_bytes = _hub_pieces(lib, adj, long_rows, adj.K, d, x.device)
        if gather_bias is not None:
            _check_gather_bias(x, gather_bias)
            check(lib.ctgcn_core_aggregate_bias_f32(n, d, adj.K, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot), ptr(x),
                                                    ptr(gather_bias), ptr(H), flags, ptr(long_rows), 0 if long_rows is None else long_rows.numel(),
                                                    adj.LONG_ROW, split, ptr(hub_ws), hub_bytes, _stream()), "ctgcn_core_aggregate_bias_f32")
            return H
        check(lib.ctgcn_core_aggregate_f32(n, d, adj.K, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot), ptr(x),
                                           x.stride(0), ptr(H), flags, ptr(long_rows), 0 if long_rows is None else long_rows.numel(),
                                           adj.LONG_ROW, split, ptr(hub_ws), hub_bytes, _stream()), "ctgcn_core_aggregate_f32")
    return H


def _aggregate_gather(adj, Z, S0, relu):
    """dX[r] = S0[r] + sum_e val_e Z[col_e, slot_e] (ctgcn_core_aggregate_bwd_f32) for Z [n, K, d] / S0 [n, d] in matrix-row order"""
    lib = _lib.load()
    n, K, d = Z.shape
    flags = adj.flags | (_lib.F_RELU if relu else 0)
    dX = torch.empty(n, d, dtype=torch.float32, device=Z.device)
    t_ptr, t_col, t_val, t_slot = adj.transposed()
    long_rows = adj.long_rows(transposed=True)
    split, hub_ws, hub_bytes = _hub_pieces(lib, adj, long_rows, 1, d, Z.device, transposed=True)
    with torch.cuda.device(Z.device), _timed("agg_bwd", n=n, d=d, K=K, nnz=adj.nnz):
        check(lib.ctgcn_core_aggregate_bwd_f32(n, d, K, ptr(t_ptr), ptr(t_col), ptr(t_val), ptr(t_slot), ptr(Z), ptr(S0),
                                               ptr(dX), d, flags, ptr(long_rows), 0 if long_rows is None else long_rows.numel(),
                                               adj.LONG_ROW, split, ptr(hub_ws), hub_bytes, _stream()), "ctgcn_core_aggregate_bwd_f32")
    return dX


def _aggregate_bwd(adj, H, dH, relu):
    lib = _lib.load()
    n, K, d = dH.shape
    flags = adj.flags | (_lib.F_RELU if relu else 0)
    Z = torch.empty_like(dH)
    S0 = torch.empty(n, d, dtype=torch.float32, device=dH.device) if adj.self_loop else None
    with torch.cuda.device(dH.device), _timed("agg_bwd_prep", n=n, d=d, K=K, self_loop=adj.self_loop):
        check(lib.ctgcn_core_aggregate_bwd_prep_f32(n, d, K, ptr(dH), ptr(H), ptr(Z), ptr(S0), flags, _stream()),
              "ctgcn_core_aggregate_bwd_prep_f32")
    return _aggregate_gather(adj, Z, S0, relu)


class _CoreAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, adj, relu, gather_bias):
        H = _aggregate_fwd(adj, x, relu, None if gather_bias is None else gather_bias.detach())
        ctx.adj, ctx.relu = adj, relu
        ctx.save_for_backward(H)
        return H

    @staticmethod
    def backward(ctx, dH):
        (H,) = ctx.saved_tensors
        dH = dH.contiguous()
        dX = _aggregate_bwd(ctx.adj, H, dH, ctx.relu)
        # every operand row is x[row] + gather_bias: dX is the gradient of that sum, the bias takes its column sum (what
        # _LinearOfIdentity.backward makes of the same dX)
        return dX, None, None, (dX.sum(0) if ctx.needs_input_grad[3] else None)


def core_aggregate(x, adj, relu=True, gather_bias=None):
    """H[N, K, d] with H[:, j, :] = relu(sum_{i<=j} A_i x)  — layers.py:41-48 and the layout of :58.
    gather_bias [d] (optional): x is a Linear weight stored by input row and the aggregated operand is x + gather_bias, never
    materialised (see _aggregate_fwd); differentiable in both."""
    _need_cuda(x, adj.col)
    if adj.K < 1:
        raise ValueError("empty k-core adjacency list")
    if x.dim() != 2 or x.shape[0] != adj.n:
        raise ValueError("features must be [%d, d], got %s" % (adj.n, tuple(x.shape)))
    if x.dtype != torch.float32:
        raise TypeError("fp32 features expected")
    if x.device != adj.device:
        raise ValueError("features on %s but adjacency on %s" % (x.device, adj.device))
    x = x if x.stride(1) == 1 else x.contiguous()
    return _CoreAggregate.apply(x, adj, relu, gather_bias)


# ------------------------------------------------------------- GRU over the core / time axis (+ sum, LayerNorm)
import os as _os
_GI_MAX_ELEMS = int(_os.environ.get("CTGCN_GI_MAX_ELEMS", 1 << 30))   # row-chunk bound: rows * steps * 4 * hidden elements (4 GiB of saved gates)


def gru_fused_ok(rnn, seq):
    """The HIP recurrent kernels cover the configuration every shipped CTGCN config uses: single-layer
    unidirectional batch_first GRU with hidden 128 on fp32 CUDA tensors (forward and backward)."""
    return (isinstance(rnn, torch.nn.GRU) and rnn.hidden_size == 128 and rnn.num_layers == 1 and not rnn.bidirectional
            and rnn.batch_first and seq.is_cuda and seq.dtype == torch.float32)


def _gru_bias(rnn, hid):
    """(b_ih + b_hh on r, z | b_ih on n,  b_hn): the two bias vectors the GRU kernels take.  Folded once per version of the two parameters
    (round 6: an AS-like forward spent 17 tiny torch kernels per window on re-folding them — clone, add, contiguous per GRU — and the
    fresh tensors changed the grouped launches' descriptors on every call); the folded vectors live in the operand-plane cache."""
    if not rnn.bias:
        return None, None
    b_ih, b_hh = rnn.bias_ih_l0, rnn.bias_hh_l0

    def fold():
        both = torch.empty(4 * hid, dtype=b_ih.dtype, device=b_ih.device)
        both[: 3 * hid] = b_ih.detach()
        both[: 2 * hid] += b_hh.detach()[: 2 * hid]           # r and z gates: both biases are simply added
        both[3 * hid:] = b_hh.detach()[2 * hid:]              # n gate: b_hn stays inside r * (W_hn h + b_hn)
        return both
    if plane_cache_enabled() and not b_ih.is_inference() and not b_hh.is_inference():
        tag = (b_hh.data_ptr(), b_hh._version)                # the cache validates b_ih (identity + version); b_hh rides along as a tag

        def make():
            both = fold()
            both._ctgcn_tag = tag
            return both, 16 * hid
        both = _plane_cache.get(b_ih, "gru_bias", make)
        if getattr(both, "_ctgcn_tag", None) != tag:
            _plane_cache.forget(b_ih, "gru_bias")
            both = _plane_cache.get(b_ih, "gru_bias", make)
    else:
        both = fold()
    return both[: 3 * hid], both[3 * hid:]


def _row_chunks(lib, rows, steps, hid):
    """Equal row chunks, multiples of the kernel's row granule (rows per block x CUs), bounded projection buffer."""
    if rows <= 0:
        return [(0, 0)]
    granule = int(lib.ctgcn_gru_row_granule())
    max_rows = max(granule, (_GI_MAX_ELEMS // (steps * 4 * hid)) // granule * granule)
    n_chunks = -(-rows // max_rows)
    chunk = -(-(-(-rows // n_chunks)) // granule) * granule
    return [(lo, min(chunk, rows - lo)) for lo in range(0, rows, chunk)]


def split_mfma_enabled():
    """fp32-accurate split arithmetic on the 16-bit matrix cores (default).  CTGCN_FP32_MFMA_ONLY=1 forces the
    plain fp32 paths (hipBLASLt fp32 GEMM + v_mfma_f32_16x16x4_f32 recurrence) for A/B comparisons."""
    import os
    return os.environ.get("CTGCN_FP32_MFMA_ONLY", "0") != "1"


def layer_kernel_enabled(reduce_sum=True):
    """ctgcn_gru_layer_f32: input projection and recurrence of a GRU with d_in = hidden = 128 in one kernel, both weight matrices
    resident on the CU (registers + LDS), the projection consumed from the MFMA accumulators (never materialised).  Bit-identical to
    the projection + recurrence kernel pair (tests/test_gpu_gru.py) at 1/7 of its HBM traffic.
    CTGCN_GRU_LAYER = 1 (default): both forms — the sum-over-steps form of CoreDiffusion (4.2-4.6 vs 6.4 ms per 1M x 8 call) and the
    per-step form of the temporal GRU (LayerNorm(h_t) emitted per unit through an LDS staging buffer: 11.8-12.4 vs 15.7 ms per 1M x 16 call).
    sum: the sum form only.  0: never.  CTGCN_GRU_LAYER_WAVES=4 selects the 4-wave builds (one wave per SIMD: 5.2 / 16.5 ms)."""
    import os
    mode = os.environ.get("CTGCN_GRU_LAYER", "1")
    if mode == "0":
        return False
    return bool(reduce_sum) or mode != "sum"


def forward_split_mode():
    """Arithmetic of the forward GRU products (include/ctgcn_hip.h CTGCN_SPLIT_*): 2 = fp16x2 (default: per-row scaled
    two-term fp16 split, three products — half the matrix work of bf16x3 and measured more accurate), 1 = bf16x3
    (CTGCN_GRU_SPLIT=bf16x3), 0 = fp32 MFMA (CTGCN_FP32_MFMA_ONLY=1)."""
    import os
    if not split_mfma_enabled():
        return 0
    return 1 if os.environ.get("CTGCN_GRU_SPLIT", "f16x2") == "bf16x3" else 2


_LINEAR_WS_MAX = 2 << 30       # bytes of fp16 planes per ctgcn_linear_f32 call (rows are chunked above that)


def linear_split_enabled():
    """CTGCN_LINEAR_SPLIT=0 (or CTGCN_FP32_MFMA_ONLY=1) selects the fp32 library GEMM instead of ctgcn_linear_f32."""
    import os
    return forward_split_mode() == 2 and os.environ.get("CTGCN_LINEAR_SPLIT", "1") != "0"


def linear_split_ok(x2d, weight):
    """ctgcn_linear_f32 covers fp32 CUDA operands with unit column stride and k >= 32 (any k and row stride: rows that are not
    16-byte aligned are read with scalar loads)."""
    return (linear_split_enabled() and x2d.is_cuda and x2d.dtype == torch.float32 and weight.dtype == torch.float32 and x2d.dim() == 2
            and x2d.stride(1) == 1 and weight.stride(1) == 1 and x2d.data_ptr() % 4 == 0 and weight.data_ptr() % 4 == 0
            and x2d.shape[0] > 0 and x2d.shape[1] >= 32 and x2d.stride(0) >= x2d.shape[1] and weight.stride(0) >= weight.shape[1])


class _PlaneCache(object):
    """Operand planes (ctgcn_split_rows_f32 / ctgcn_pack_weight_f32) of tensors that do not change between forwards: the weights of an
    inference run and node features the caller has marked static (mark_static: the reference builds them once and feeds them to every
    batch, train.py:72-76 -> embedding.py:318).  Keyed by storage address + shape + strides + kind, validated by identity (weak
    reference) and by the tensor's version counter: an in-place update — optimizer.step(), load_state_dict(), p.copy_() — re-splits.
    What the version counter does NOT see: writes through `.data` / raw pointers (p.data.mul_(2), dist.broadcast(p.data)).  After such
    an edit call ops.invalidate_plane_cache() (snapshot_parallel.shard_cgcn does).  Tensors created under torch.inference_mode() have no
    version counter: they are split on every call and never cached.  Entries die with their tensor; at most `limit` bytes are kept
    (least recently used first out)."""

    def __init__(self, limit=48 << 30):
        import collections
        self.limit, self.bytes, self.entries = limit, 0, collections.OrderedDict()
        self.capture_hold = None                 # a list while a frozen-weights capture runs (graph_capture.GraphedInference)

    def _drop(self, key):
        e = self.entries.pop(key, None)
        if e is not None:
            self.bytes -= e[3]

    def clear(self):
        self.entries.clear()
        self.bytes = 0

    def forget(self, t, kind):
        self._drop((t.data_ptr(), tuple(t.shape), tuple(t.stride()), str(t.device), kind))

    def get(self, t, kind, make):
        """make() -> (buffer, nbytes): the operand form `kind` of tensor t, built on the current stream"""
        import weakref
        capturing = torch.cuda.is_current_stream_capturing()
        if t.is_inference() or (capturing and self.capture_hold is None):
            # no version counter to validate against (t._version raises): never cached.  Under hipGraph capture the operand form is built
            # INSIDE the graph, from the tensor's storage at replay time: a replay sees in-place weight updates (graph_capture.py's contract)
            return make()[0]
        key = (t.data_ptr(), tuple(t.shape), tuple(t.stride()), str(t.device), kind)
        e = self.entries.get(key)
        cur = torch.cuda.current_stream(t.device)
        if e is not None and e[0]() is t and e[1] == t._version:
            self.entries.move_to_end(key)
            if capturing:
                # GraphedInference(frozen_weights=True): the graph reads the operand form built by the warm-up forwards (the device was
                # synchronised before the capture began).  The runner keeps the buffer alive for as long as the graph exists.
                self.capture_hold.append(e[2])
                return e[2]
            if e[5] != cur:                      # built on another stream: order behind it, keep the buffer alive for this stream too
                cur.wait_event(e[4])
                e[2].record_stream(cur)
            return e[2]
        if capturing:
            return make()[0]                     # a miss under capture: built in-graph, nothing kept (the buffer belongs to the capture's pool)
        self._drop(key)
        buf, nbytes = make()
        ev = torch.cuda.Event()
        ev.record(cur)
        self.entries[key] = (weakref.ref(t, lambda _r, key=key: self._drop(key)), t._version, buf, nbytes, ev, cur)
        self.bytes += nbytes
        while self.bytes > self.limit and len(self.entries) > 1:
            self._drop(next(iter(self.entries)))
        return buf

    def planes(self, t, lib):
        """row-major fp16 planes + row scales of t [rows, k] (the A operand form of the split GEMM)"""
        def make():
            rows, k = t.shape
            nbytes = int(lib.ctgcn_split_planes_bytes(rows, k))
            buf = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
            check(lib.ctgcn_split_rows_f32(rows, k, ptr(t), t.stride(0), ptr(buf), nbytes, _stream()), "ctgcn_split_rows_f32")
            return buf, nbytes
        return self.get(t, "planes", make)

    def packed(self, t, lib):
        """packed W operand of the weight t [n_out, k] (ctgcn_pack_weight_f32: the split in matrix-core fragment order + column scales)"""
        def make():
            n_out, k = t.shape
            nbytes = int(lib.ctgcn_pack_weight_bytes(n_out, k))
            buf = torch.empty(nbytes, dtype=torch.uint8, device=t.device)
            check(lib.ctgcn_pack_weight_f32(n_out, k, ptr(t), t.stride(0), ptr(buf), nbytes, _stream()), "ctgcn_pack_weight_f32")
            return buf, nbytes
        return self.get(t, "packed", make)


_plane_cache = _PlaneCache()


def invalidate_plane_cache():
    """Forget every cached operand plane.  Needed after weights or static features were edited behind the version counter's back
    (writes through `.data`, raw pointers, collectives on `.data`)."""
    _plane_cache.clear()


def mark_static(x):
    """Declare that the feature tensor x is fed to every forward unchanged (what the reference's loader output is: built once in
    train.py:72-76, passed to every batch, embedding.py:318): the first dense Linear keeps x's operand planes between forwards instead of
    splitting x on every call.  ctgcn_amd.helper.DataLoader marks what it returns; in-place edits through the autograd-visible API
    re-split (version counter), edits through `.data` need invalidate_plane_cache().  Returns x."""
    x._ctgcn_static = True
    return x


def is_static(x):
    return bool(getattr(x, "_ctgcn_static", False))


def plane_cache_enabled():
    """CTGCN_PLANE_CACHE=0: ctgcn_linear_f32 splits both operands on every call (round 3's behaviour) for A/B runs."""
    import os
    return os.environ.get("CTGCN_PLANE_CACHE", "1") != "0"      # (under hipGraph capture _PlaneCache.get builds in-graph and keeps nothing)


class Planes(object):
    """the operand form of a dense activation [rows, k] that never existed as fp32 rows: per-row scale + two fp16 planes, written by the GEMM
    that produced it (ctgcn_linear_packed_chain_f32) for the GEMM that consumes it"""
    __slots__ = ("buf", "rows", "k", "device")

    def __init__(self, buf, rows, k):
        self.buf, self.rows, self.k, self.device = buf, rows, k, buf.device

    @property
    def shape(self):
        return (self.rows, self.k)


def _linear_chunk_rows(k):
    kp = -(-k // 64) * 64
    return max(128, (_LINEAR_WS_MAX // (kp * 4 + 4)) // 128 * 128)


def mlp_chain_enabled():
    """CTGCN_MLP_CHAIN=0: every Linear of an MLP writes fp32 rows and the next one splits them again (A/B runs)"""
    import os
    return os.environ.get("CTGCN_MLP_CHAIN", "1") != "0"


def linear_chain_ok(x, weight, next_weight):
    """Inference through two consecutive dense Linear layers (layers.py:95-106): the first one's output can leave as the second one's operand
    planes (linear_split(..., planes_out=True)) — both on the split GEMM in one row chunk, the hidden width at most 512."""
    if not (mlp_chain_enabled() and linear_split_enabled() and plane_cache_enabled()):
        return False
    if isinstance(x, Planes):
        rows, k = x.rows, x.k
        if not (weight.is_cuda and weight.dtype == torch.float32 and weight.stride(1) == 1 and weight.data_ptr() % 4 == 0 and weight.stride(0) >= k):
            return False
    else:
        if not (torch.is_tensor(x) and not x.is_sparse and x.dim() == 2 and linear_split_ok(x, weight)):
            return False
        rows, k = x.shape
    hidden = weight.shape[0]
    if weight.shape[1] != k or next_weight.shape[1] != hidden or hidden < 32 or hidden > 512:
        return False
    if not (next_weight.is_cuda and next_weight.dtype == torch.float32 and next_weight.dim() == 2 and next_weight.stride(1) == 1
            and next_weight.data_ptr() % 4 == 0 and next_weight.stride(0) >= next_weight.shape[1] and next_weight.device == weight.device
            and weight.device == x.device):
        return False
    return rows > 0 and rows <= _linear_chunk_rows(k) and rows <= _linear_chunk_rows(hidden)


def linear_split(x2d, weight, bias, out=None, selu=False, static_x=False, planes_out=False):
    """out[rows, n_out] = x2d @ weight^T + bias in fp32-accurate fp16x2 split arithmetic on the matrix cores (gemm_h2_panel_kernel);
    selu: F.selu applied in the GEMM's epilogue (one pass over the output less).
    The weight's packed operand is built once per weight version (_PlaneCache); static_x: x2d is a tensor the caller feeds to every
    forward unchanged (mark_static): its planes are kept too.
    x2d may be a Planes object (the output of a call with planes_out=True: the hidden activations of an MLP go from GEMM to GEMM as operand
    planes, never as fp32 rows; linear_chain_ok says when)."""
    lib = _lib.load()
    rows, k = x2d.shape
    n_out = weight.shape[0]
    chunk = _linear_chunk_rows(k)
    b = None if bias is None else bias.detach().contiguous()
    w = weight.detach()
    act = _lib.ACT_SELU if selu else _lib.ACT_NONE
    if isinstance(x2d, Planes) or planes_out:
        if not (rows <= chunk and plane_cache_enabled()) or (planes_out and n_out > 512):
            raise ValueError("linear_split: operand planes in / out need one row chunk, the plane cache and n_out <= 512 (linear_chain_ok)")
        dev = x2d.device
        with torch.cuda.device(dev):
            wp = _plane_cache.packed(weight, lib)
            if isinstance(x2d, Planes):
                xp = x2d.buf
            elif static_x and not x2d.requires_grad:
                xp = _plane_cache.planes(x2d, lib)
            else:
                nbytes = int(lib.ctgcn_split_planes_bytes(rows, k))
                xp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
                with _timed("linear_aux", rows=rows, k=k, split=True):
                    check(lib.ctgcn_split_rows_f32(rows, k, ptr(x2d), x2d.stride(0), ptr(xp), nbytes, _stream()), "ctgcn_split_rows_f32")
            if planes_out:
                obytes = int(lib.ctgcn_split_planes_bytes(rows, n_out))
                obuf = torch.empty(obytes, dtype=torch.uint8, device=dev)
                with _timed("linear_split", rows=rows, k=k, n_out=n_out, planes=True, chain=True):
                    check(lib.ctgcn_linear_packed_chain_f32(rows, n_out, k, ptr(xp), ptr(wp), ptr(b), act, ptr(obuf), obytes, _stream()),
                          "ctgcn_linear_packed_chain_f32")
                return Planes(obuf, rows, n_out)
            if out is None:
                out = torch.empty(rows, n_out, dtype=torch.float32, device=dev)
            with _timed("linear_split", rows=rows, k=k, n_out=n_out, planes=True):
                check(lib.ctgcn_linear_packed_f32(rows, n_out, k, ptr(xp), ptr(wp), ptr(b), act, ptr(out), out.stride(0), _stream()), "ctgcn_linear_packed_f32")
        return out
    if out is None:
        out = torch.empty(rows, n_out, dtype=torch.float32, device=x2d.device)
    if rows <= chunk and plane_cache_enabled():
        with torch.cuda.device(x2d.device):
            wp = _plane_cache.packed(weight, lib)
            if static_x and not x2d.requires_grad:
                xp = _plane_cache.planes(x2d, lib)
            else:
                nbytes = int(lib.ctgcn_split_planes_bytes(rows, k))
                xp = torch.empty(nbytes, dtype=torch.uint8, device=x2d.device)
                with _timed("linear_aux", rows=rows, k=k, split=True):
                    check(lib.ctgcn_split_rows_f32(rows, k, ptr(x2d), x2d.stride(0), ptr(xp), nbytes, _stream()), "ctgcn_split_rows_f32")
            with _timed("linear_split", rows=rows, k=k, n_out=n_out, planes=True):
                check(lib.ctgcn_linear_packed_f32(rows, n_out, k, ptr(xp), ptr(wp), ptr(b), act, ptr(out), out.stride(0), _stream()), "ctgcn_linear_packed_f32")
        return out
    with torch.cuda.device(x2d.device):
        ws_bytes = int(lib.ctgcn_linear_workspace_bytes(min(rows, chunk), n_out, k))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x2d.device)
        for lo in range(0, rows, chunk):
            n = min(chunk, rows - lo)
            xs, ys = x2d[lo:lo + n], out[lo:lo + n]
            with _timed("linear_split", rows=n, k=k, n_out=n_out):
                check(lib.ctgcn_linear_f32(n, n_out, k, ptr(xs), xs.stride(0), ptr(w), w.stride(0), ptr(b), act,
                                           ptr(ys), ys.stride(0), ptr(ws), ws_bytes, _stream()), "ctgcn_linear_f32")
    return out


def linear_train_enabled():
    """CTGCN_LINEAR_TRAIN=0: nn.Linear under autograd stays torch's (fp32 library GEMMs) for A/B runs"""
    import os
    return os.environ.get("CTGCN_LINEAR_TRAIN", "1") != "0"


class _LinearSplit(torch.autograd.Function):
    """nn.Linear on dense rows under autograd (layers.py:95-106 in training: the MLP of CTGCN-S, 1 737 -> 500 -> 500 -> 128 on the
    Facebook-like config): y = x W^T + b and dx = dy W on the split GEMM (the forward's arithmetic), dW = dy^T x — a product that contracts
    over the ROWS, which the panel kernel does not do — and db stay with the library.  Facebook-like training step: the fp32 library GEMMs
    of the three layers were 88 of 139 ms."""

    @staticmethod
    def forward(ctx, x, weight, bias, static_x):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return linear_split(x, weight, bias, static_x=static_x)       # x itself: the plane cache knows a static x by identity

    @staticmethod
    def backward(ctx, dy):
        x, weight = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:                                # dx = dy @ w_t^T with w_t = weight^T [k, n_out], transposed + packed once per version
            dx = linear_split(dy, _transposed(weight), None) if _transposed_split_ok(dy, weight) else dy @ weight.detach()
        if ctx.needs_input_grad[1]:
            dw = torch.mm(dy.t(), x.detach())
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = dy.sum(0)
        return dx, dw, db, None


def linear_split_train(x2d, weight, bias, static_x=False):
    return _LinearSplit.apply(x2d, weight, bias, bool(static_x))


def _project(x2d, w_ih, bias, out, steps_blocked=0):
    """out = x2d @ w_ih^T + bias — the GRU input projection.  Returns True when `out` was written in the recurrence
    kernel's blocked tile layout (only asked for with steps_blocked > 0, only done by the fp16x2 kernel), else [rows, 3h]."""
    mode = forward_split_mode()
    if mode and x2d.shape[1] == 128 and w_ih.shape[0] == 384 and x2d.stride(1) == 1 \
            and x2d.stride(0) % 4 == 0 and x2d.data_ptr() % 16 == 0 and w_ih.is_contiguous():
        lib = _lib.load()
        blocked = steps_blocked if mode == 2 else 0
        with _timed("gru_proj", rows=x2d.shape[0]):
            check(lib.ctgcn_gru_input_proj_f32(x2d.shape[0], 128, 128, ptr(x2d), x2d.stride(0), ptr(w_ih), ptr(bias), ptr(out),
                                               mode, blocked, _stream()), "ctgcn_gru_input_proj_f32")
        return blocked > 0
    out = out[: x2d.shape[0] * w_ih.shape[0]].view(x2d.shape[0], w_ih.shape[0])
    if linear_split_ok(x2d, w_ih):
        linear_split(x2d, w_ih, bias, out=out)
        return False
    if bias is None:
        torch.mm(x2d, w_ih.t(), out=out)
    else:
        torch.addmm(bias, x2d, w_ih.t(), out=out)
    return False


def _gi_buffer(rows, steps, hid, device):
    """flat fp32 buffer for the projection of `rows` sequences; whole 64-row tiles (the blocked layout writes by tile)"""
    return torch.empty(-(-rows // 64) * 64 * steps * 3 * hid, dtype=torch.float32, device=device)


def _transposed(w):
    """w^T as a contiguous tensor, built once per version of w (every backward re-transposed the weight and pushed the temporary
    through the packed-operand cache, which keys on the tensor object — an entry added and dropped per call).  The cached transpose is a
    stable object, so its packed form (linear_split -> _PlaneCache.packed) is kept with it and dies with it when w changes."""
    def make():
        t = w.detach().t().contiguous()
        return t, t.numel() * t.element_size()
    if not plane_cache_enabled():
        return make()[0]
    return _plane_cache.get(w, "transposed", make)


def _transposed_split_ok(x2d, w):
    """linear_split_ok(x2d, w^T contiguous) without building the transpose"""
    return (linear_split_enabled() and x2d.is_cuda and w.is_cuda and x2d.device == w.device and x2d.dtype == torch.float32 and w.dtype == torch.float32
            and x2d.dim() == 2 and w.dim() == 2 and x2d.stride(1) == 1 and x2d.data_ptr() % 4 == 0 and x2d.shape[0] > 0 and x2d.shape[1] >= 32
            and x2d.stride(0) >= x2d.shape[1] and x2d.shape[1] == w.shape[0])


def _project_grad(dgi, w_ih, out):
    """out[rows, d_in] = dgi[rows, 3h] @ w_ih — gradient of the input projection w.r.t. its input."""
    if split_mfma_enabled() and w_ih.shape == (384, 128) and w_ih.is_contiguous() and dgi.is_contiguous() \
            and out.stride(1) == 1 and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0:
        lib = _lib.load()
        check(lib.ctgcn_gru_input_grad_f32(dgi.shape[0], 128, 128, ptr(dgi), ptr(w_ih.detach()), ptr(out), out.stride(0), _stream()),
              "ctgcn_gru_input_grad_f32")
        return
    if _transposed_split_ok(dgi, w_ih) and out.stride(1) == 1:
        # the 500-wide first layer (layers.py:59 with input_size = hid_dim): the fp32 library GEMM took 1.8 ms per Enron-like snapshot,
        # 14 % of the training step; split of dgi (0.3 ms) + gemm_h2_panel_kernel (0.45 ms).  Same fp32-accurate arithmetic as the forward.
        # w_t [d_in, 3h] is the "weight" of out = dgi @ w_t^T: transposed and packed once per weight version (_transposed)
        linear_split(dgi, _transposed(w_ih), None, out=out)
        return
    torch.mm(dgi, w_ih.detach(), out=out)


def keep_projection_enabled():
    """CTGCN_KEEP_GI=0: the backward of a GRU with d_in != 128 always recomputes its input projection (A/B runs)"""
    import os
    return os.environ.get("CTGCN_KEEP_GI", "1") != "0"


def wide_weight_grad_enabled():
    """CTGCN_WIDE_DW=0: dW_ih of a GRU with d_in > 128 stays an fp32 library GEMM (A/B runs)"""
    import os
    return os.environ.get("CTGCN_WIDE_DW", "1") != "0"


_DW_PAIRS = 128          # block pairs of ctgcn_gru_weight_grad_f32: 256 blocks = one per CU of an MI355X


def _weight_grad(part, g01, g2, x2d, steps, shift, accumulate):
    """part[p] (+)= block pair p's share of  sum_r [g01[r, :2h] | g2[r, :h]]^T x'[r]  (x' = x2d, or x2d shifted one step
    inside each sequence); part.sum(0) is the weight gradient."""
    lib = _lib.load()
    check(lib.ctgcn_gru_weight_grad_f32(g01.shape[0], steps, 128, ptr(g01), g01.stride(0), ptr(g2), g2.stride(0), ptr(x2d),
                                        x2d.stride(0), 1 if shift else 0, ptr(part), part.shape[0], 1 if accumulate else 0,
                                        _stream()), "ctgcn_gru_weight_grad_f32")


def _gru_forward(seq, w_ih, w_hh, bias, b_hn, ln_w, ln_b, eps, reduce_sum, out=None, keep_gi=None):
    """keep_gi: a list that receives (gi buffer, blocked layout flag) when the projection was materialised in one chunk (training: the
    backward's recompute pass starts from it instead of splitting x and multiplying by W_ih again)"""
    lib = _lib.load()
    rows, steps, d_in = seq.shape
    hid = w_hh.shape[1]
    if out is None:
        out = torch.empty((rows, hid) if reduce_sum else (rows, steps, hid), dtype=torch.float32, device=seq.device)
    elif not (reduce_sum and out.shape == (rows, hid) and out.dtype == torch.float32 and out.stride(1) == 1
              and out.stride(0) % 2 == 0 and out.stride(0) >= hid and out.device == seq.device):
        raise ValueError("gru: out must be a [rows, %d] fp32 view with unit column stride (reduce_sum only)" % hid)
    ldo = out.stride(0) if reduce_sum else 0
    if rows == 0:
        return out
    split = forward_split_mode()
    if split == 2 and d_in == hid and layer_kernel_enabled(reduce_sum) and seq.stride(2) == 1 and seq.stride(1) % 4 == 0 \
            and seq.stride(0) == steps * seq.stride(1) and seq.data_ptr() % 16 == 0 and w_ih.is_contiguous():
        # projection + recurrence in one kernel, both weight matrices in the register file, gi never materialised
        with torch.cuda.device(seq.device), _timed("gru_layer", rows=rows, steps=steps, reduce_sum=bool(reduce_sum)):
            check(lib.ctgcn_gru_layer_f32(rows, steps, d_in, hid, ptr(seq), seq.stride(1), ptr(w_ih), ptr(w_hh), ptr(bias), ptr(b_hn),
                                          ptr(ln_w), ptr(ln_b), eps, 1 if reduce_sum else 0, ptr(out), ldo, None, None, 0, _stream()), "ctgcn_gru_layer_f32")
        return out
    chunks = _row_chunks(lib, rows, steps, hid)
    gi_buf = _gi_buffer(chunks[0][1], steps, hid, seq.device)
    with torch.cuda.device(seq.device):
        for lo, n in chunks:
            blocked = _project(seq[lo:lo + n].reshape(n * steps, d_in), w_ih, bias, gi_buf, steps_blocked=steps)
            with _timed("gru_seq", rows=n, steps=steps):
                check(lib.ctgcn_gru_seq_f32(n, steps, hid, ptr(gi_buf), ptr(w_hh), ptr(b_hn), ptr(ln_w), ptr(ln_b), eps,
                                            1 if reduce_sum else 0, ptr(out[lo:lo + n]), ldo, None, split, 1 if blocked else 0,
                                            None, None, None, _stream()), "ctgcn_gru_seq_f32")
        if keep_gi is not None and len(chunks) == 1:
            keep_gi.append((gi_buf, blocked))
    return out


def gru_steps_scattered_ok(rnn, base, steps=None):
    """gru_sequence_scattered covers what the register-resident layer kernel covers: GRU 128 -> 128, fp16x2 arithmetic, 8-wave build,
    and at most 32 steps (the kernel keeps the per-step offset table in 32 LDS slots).  steps: the sequence length — pass it; without it
    the length is not checked here, and ctgcn_gru_layer_f32 refuses a longer table with CTGCN_E_UNSUPPORTED."""
    import os
    return ((steps is None or 1 <= steps <= 32) and gru_fused_ok(rnn, base) and rnn.input_size == rnn.hidden_size and forward_split_mode() == 2 and layer_kernel_enabled(False)
            and os.environ.get("CTGCN_GRU_LAYER_WAVES", "8") != "4" and rnn.weight_ih_l0.is_contiguous()
            and not (torch.is_grad_enabled() and any(p.requires_grad for p in rnn.parameters())))


def gru_sequence_scattered(rnn, norm, base, step_offsets, ld_row, rows):
    """LayerNorm(GRU(x)) -> [rows, steps, 128] (models.py:249-250) for an input whose steps live at base + step_offsets[t] + r * ld_row
    (floats) — e.g. the receive buffer of the snapshot-parallel exchange — without gathering them into a [rows, steps, 128] tensor first.
    Inference only; same kernel and arithmetic as gru_sequence(..., reduce_sum=False)."""
    lib = _lib.load()
    steps, hid = int(step_offsets.numel()), rnn.hidden_size
    bias, b_hn = _gru_bias(rnn, hid)
    ln_w = None if norm is None else norm.weight
    ln_b = None if norm is None else norm.bias
    eps = 0.0 if norm is None else float(norm.eps)
    out = torch.empty(rows, steps, hid, dtype=torch.float32, device=base.device)
    if rows == 0:
        return out
    with torch.cuda.device(base.device), _timed("gru_layer", rows=rows, steps=steps, reduce_sum=False):
        check(lib.ctgcn_gru_layer_f32(rows, steps, hid, hid, ptr(base), hid, ptr(rnn.weight_ih_l0.detach()), ptr(rnn.weight_hh_l0.detach().contiguous()),
                                      ptr(bias), ptr(b_hn), ptr(ln_w), ptr(ln_b), eps, 0, ptr(out), 0, None, ptr(step_offsets), int(ld_row), _stream()),
              "ctgcn_gru_layer_f32")
    return out


def aggregate_split_enabled():
    """CTGCN_AGG_SPLIT=0 keeps aggregation and GRU input projection apart (fp32 H in between) for A/B runs."""
    import os
    return linear_split_enabled() and os.environ.get("CTGCN_AGG_SPLIT", "1") != "0"


_AGG_SPLIT_MAX = 16 << 30     # bytes of fp16 planes the fused aggregation may write in one call (config 5: 4.1 GB per snapshot)


def aggregate_split_ok(rnn, x, adj):
    """Inference through a CoreDiffusion layer: the aggregation kernel can hand its consumer fp16 planes + row scales instead of
    fp32 rows (ctgcn_core_aggregate_split_f32) — the split GEMM of the GRU input projection when d_in != 128, the
    register-resident GRU layer kernel (ctgcn_gru_layer_presplit_f32) when d_in = hidden = 128."""
    if not aggregate_split_enabled() or x.dim() != 2 or not gru_fused_ok(rnn, x) or x.shape[0] != adj.n or x.device != adj.device:
        return False
    if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in rnn.parameters())):
        return False
    d, hid = x.shape[1], rnn.hidden_size
    if d % 4 or d < 32 or d > 512 or x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or adj.K < 1 or adj.n < 1:
        return False
    if d == hid:        # the layer kernel path
        return layer_kernel_enabled(True) and adj.n * adj.K * (d * 4 + 4) <= _AGG_SPLIT_MAX and rnn.weight_ih_l0.is_contiguous()
    if adj.n * adj.K * (-(-d // 64) * 64 * 4 + 4) > _LINEAR_WS_MAX:
        return False
    return len(_row_chunks(_lib.load(), adj.n, adj.K, hid)) == 1


def row_plan_enabled():
    """CTGCN_DEDUP=0: the inference path writes and multiplies every (node, core) row of H, repeated or not (A/B runs)."""
    import os
    return os.environ.get("CTGCN_DEDUP", "1") != "0"


def aggregate_split_planes(x, adj, n_out, plan=None, ws=None, gather_bias=None):
    """ctgcn_core_aggregate_split_f32: relu(cumulative A_k x) as fp16 planes + row scales in a workspace (returned).  n_out = width of
    the GEMM that follows (1: the GRU layer kernel).  plan = adj.row_plan(tile): repeated rows are not written — tile 16 with the layer
    kernel as consumer (holes in the [n K] row layout), tile 64 with the GEMM (compact operand rows, plan["operand_rows"] of them).
    gather_bias [d] (optional): operand rows x[row] + gather_bias, x dense (ctgcn_core_aggregate_split_bias_f32)."""
    lib = _lib.load()
    n, d = x.shape
    flags = adj.flags | _lib.F_RELU
    long_rows = adj.long_rows()
    n_long = 0 if long_rows is None else long_rows.numel()
    ws_bytes = int(lib.ctgcn_core_aggregate_split_workspace_bytes(n, d, adj.K, n_out, n_long))
    if ws is None:
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=x.device)
    compact = plan is not None and not (d == 128 and n_out == 1)
    if plan is not None and plan["tile"] != (adj.PLAN_TILE_GEMM if compact else adj.PLAN_TILE):
        raise ValueError("aggregate_split_planes: plan tile %d does not belong to this consumer" % plan["tile"])
    hub_dest = adj.plan_row_dest(plan, long_rows, compact) if (plan is not None and n_long) else None
    split, hub_ws, hub_bytes = _hub_pieces(lib, adj, long_rows, adj.K, d, x.device)
    with _timed("agg_fwd", n=n, d=d, K=adj.K, nnz=adj.nnz, split=True, rows_written=(plan["new_rows"] if plan is not None else n * adj.K)):
        if gather_bias is not None:
            _check_gather_bias(x, gather_bias)
            check(lib.ctgcn_core_aggregate_split_bias_f32(n, d, adj.K, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot), ptr(x), ptr(gather_bias),
                                                          flags, ptr(long_rows), n_long, adj.LONG_ROW, n_out,
                                                          ptr(plan["order"]) if plan is not None else None, ptr(plan["tile_mask"]) if plan is not None else None,
                                                          ptr(plan["tile_base"]) if compact else None, plan["operand_rows"] if compact else 0,
                                                          ptr(hub_dest), split, ptr(hub_ws), hub_bytes, ptr(ws), ws_bytes, _stream()),
                  "ctgcn_core_aggregate_split_bias_f32")
            return ws, ws_bytes
        check(lib.ctgcn_core_aggregate_split_f32(n, d, adj.K, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot), ptr(x), x.stride(0),
                                                 flags, ptr(long_rows), n_long, adj.LONG_ROW, n_out,
                                                 ptr(plan["order"]) if plan is not None else None, ptr(plan["tile_mask"]) if plan is not None else None,
                                                 ptr(plan["tile_base"]) if compact else None, plan["operand_rows"] if compact else 0,
                                                 ptr(hub_dest), split, ptr(hub_ws), hub_bytes, ptr(ws), ws_bytes, _stream()), "ctgcn_core_aggregate_split_f32")
    return ws, ws_bytes


def gru_layer_presplit(ws, n, K, rnn, norm, out, plan=None):
    """ctgcn_gru_layer_presplit_f32 on the planes aggregate_split_planes(x, adj, 1, plan) wrote: LayerNorm(sum_k GRU(H)_k) -> out."""
    lib = _lib.load()
    hid = rnn.hidden_size
    bias, b_hn = _gru_bias(rnn, hid)
    w_ih, w_hh = rnn.weight_ih_l0.detach(), rnn.weight_hh_l0.detach().contiguous()
    ln_w = None if norm is None else norm.weight
    ln_b = None if norm is None else norm.bias
    eps = 0.0 if norm is None else float(norm.eps)
    with _timed("gru_layer", rows=n, steps=K, reduce_sum=True, presplit=True, new_rows=(plan["new_rows"] if plan is not None else n * K)):
        check(lib.ctgcn_gru_layer_presplit_f32(n, K, hid, ptr(ws), ptr(w_ih), ptr(w_hh), ptr(bias), ptr(b_hn), ptr(ln_w), ptr(ln_b), eps,
                                               ptr(out), out.stride(0), ptr(plan["order"]) if plan is not None else None,
                                               ptr(plan["tile_mask"]) if plan is not None else None, _stream()), "ctgcn_gru_layer_presplit_f32")
    return out


def core_diffusion_split(x, adj, rnn, norm, out=None, gather_bias=None):
    """LayerNorm(sum_k GRU(relu(cumulative A_k x))_k) — CoreDiffusion.forward (layers.py:41-62) for inference, no fp32 H:
    aggregation -> fp16 planes + row scales, then  d_in = hidden = 128: the register-resident GRU layer kernel reads the planes
    (under the graph's row plan: rows of H that repeat the row before are neither written nor multiplied by W_ih again);
    d_in != 128: split GEMM -> gate pre-activations -> recurrence + sum + LayerNorm kernel.
    gather_bias: see aggregate_split_planes."""
    lib = _lib.load()
    n, d = x.shape
    K, hid = adj.K, rnn.hidden_size
    n_out = 3 * hid
    if out is None:
        out = torch.empty(n, hid, dtype=torch.float32, device=x.device)
    elif not (out.shape == (n, hid) and out.dtype == torch.float32 and out.stride(1) == 1 and out.stride(0) % 2 == 0
              and out.stride(0) >= hid and out.device == x.device):
        raise ValueError("core_diffusion_split: out must be a [rows, %d] fp32 view with unit column stride" % hid)
    with torch.cuda.device(x.device):
        if d == hid:                                       # -> ctgcn_gru_layer_presplit_f32; its weights need no plane workspace
            plan = adj.row_plan() if row_plan_enabled() else None
            ws, _ = aggregate_split_planes(x, adj, 1, plan, gather_bias=gather_bias)
            return gru_layer_presplit(ws, n, K, rnn, norm, out, plan)
        bias, b_hn = _gru_bias(rnn, hid)
        w_ih, w_hh = rnn.weight_ih_l0.detach(), rnn.weight_hh_l0.detach().contiguous()
        ln_w = None if norm is None else norm.weight
        ln_b = None if norm is None else norm.bias
        eps = 0.0 if norm is None else float(norm.eps)
        plan = adj.row_plan(adj.PLAN_TILE_GEMM) if (row_plan_enabled() and forward_split_mode() == 2) else None
        rows = plan["operand_rows"] if plan is not None else n * K          # under a plan the GEMM only sees rows that bring a new x
        ws, ws_bytes = aggregate_split_planes(x, adj, n_out, plan, gather_bias=gather_bias)
        gi_buf = torch.empty(rows * n_out, dtype=torch.float32, device=x.device) if plan is not None else _gi_buffer(n, K, hid, x.device)
        with _timed("linear_split", rows=rows, k=d, n_out=n_out, presplit=True):
            if plane_cache_enabled():          # W_ih's packed operand: built once per weight version, not per call
                wp = _plane_cache.packed(rnn.weight_ih_l0, lib)
                check(lib.ctgcn_linear_packed_f32(rows, n_out, d, ptr(ws), ptr(wp), ptr(bias), _lib.ACT_NONE, ptr(gi_buf), n_out, _stream()),
                      "ctgcn_linear_packed_f32")
            else:
                check(lib.ctgcn_linear_presplit_f32(rows, n_out, d, ptr(w_ih), w_ih.stride(0), ptr(bias), ptr(gi_buf), n_out, ptr(ws), ws_bytes,
                                                    _stream()), "ctgcn_linear_presplit_f32")
        with _timed("gru_seq", rows=n, steps=K):
            check(lib.ctgcn_gru_seq_f32(n, K, hid, ptr(gi_buf), ptr(w_hh), ptr(b_hn), ptr(ln_w), ptr(ln_b), eps, 1, ptr(out), out.stride(0),
                                        None, forward_split_mode(), 0, ptr(plan["order"]) if plan is not None else None,
                                        ptr(plan["tile_mask"]) if plan is not None else None, ptr(plan["tile_base"]) if plan is not None else None,
                                        _stream()), "ctgcn_gru_seq_f32")
    return out


# ------------------------------------------------------------- CoreDiffusion layer, training form (d_in = hidden = 128, row plan)
def train_fused_enabled():
    """CTGCN_TRAIN_FUSED=0: training keeps round 3's path (fp32 H, _CoreAggregate + _GruSeq) for A/B runs."""
    import os
    return os.environ.get("CTGCN_TRAIN_FUSED", "1") != "0"


def core_diffusion_fused_ok(rnn, norm, x, adj):
    """Training through a CoreDiffusion layer (layers.py:41-62) with d_in = hidden = 128: the forward is the inference path (planes + row
    plan, no fp32 H), the backward runs ctgcn_gru_bwd_rec_f32 / ctgcn_gru_bwd_in_f32 (see _CoreDiffusionFused).  The plan's backward
    relies on a row having no entry tagged with a slot it repeats, seen from the transposed side too: symmetric lists only."""
    if not train_fused_enabled() or not aggregate_split_enabled() or not layer_kernel_enabled(True) or forward_split_mode() != 2:
        return False
    if x.dim() != 2 or not gru_fused_ok(rnn, x) or x.shape[0] != adj.n or x.device != adj.device or not isinstance(norm, torch.nn.LayerNorm):
        return False
    if not norm.elementwise_affine or norm.bias is None:
        return False
    d, hid = x.shape[1], rnn.hidden_size
    if d != hid or rnn.input_size != hid or x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or adj.K < 1 or adj.K > 64 or adj.n < 1:
        return False              # (33-64 matrices — America-Air / Europe-Air depth — since round 6: two mask words per tile in the backward kernels too)
    return bool(adj.symmetric) and adj.n * adj.K * (d * 4 + 4) <= _AGG_SPLIT_MAX and rnn.weight_ih_l0.is_contiguous()


def _u32ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * int(offset)


_kept_planes = {"bytes": 0, "budget": int(float(_os.environ.get("CTGCN_TRAIN_PLANES_GB", "32")) * (1 << 30))}


def _release_planes(nbytes):
    _kept_planes["bytes"] -= nbytes


class _CoreDiffusionFused(torch.autograd.Function):
    """out = LayerNorm(sum_k GRU(relu(cumulative A_k x))_k) with autograd, d_in = hidden = 128.
    forward  = ctgcn_core_aggregate_split_f32 (fp16 planes, row plan) + ctgcn_gru_layer_presplit_f32: exactly the inference path; the planes
               are what is kept for the backward (the rows the plan skips are never written: 47 % of them on config 5).
    backward = per chunk of positions: recompute (gates, h, pre-norm sum) -> LayerNorm backward -> backward recurrence + dW_hh ->
               dx + dW_ih + the aggregation's mask / suffix sums (Z, S0); then ONE gather (ctgcn_core_aggregate_bwd_f32)."""

    @staticmethod
    def forward(ctx, x, adj, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, eps, gather_bias):
        lib = _lib.load()
        n, K, hid = adj.n, adj.K, w_hh.shape[1]
        plan = adj.row_plan() if row_plan_enabled() else None
        x_d = x.detach()
        gb = None if gather_bias is None else gather_bias.detach()     # operand rows x[row] + gather_bias (aggregate_split_planes)
        ctx.gather_bias = gb
        with torch.cuda.device(x.device):
            ws, _ = aggregate_split_planes(x_d, adj, 1, plan, gather_bias=gb)
            bias, b_hn = _fold_gru_bias(b_ih, b_hh, hid)
            out = torch.empty(n, hid, dtype=torch.float32, device=x.device)
            with _timed("gru_layer", rows=n, steps=K, reduce_sum=True, presplit=True, new_rows=(plan["new_rows"] if plan is not None else n * K)):
                check(lib.ctgcn_gru_layer_presplit_f32(n, K, hid, ptr(ws), ptr(w_ih.detach()), ptr(w_hh.detach().contiguous()), ptr(bias), ptr(b_hn),
                                                       ptr(ln_w.detach()), ptr(ln_b.detach()), eps, ptr(out), out.stride(0),
                                                       ptr(plan["order"]) if plan is not None else None,
                                                       ptr(plan["tile_mask"]) if plan is not None else None, _stream()), "ctgcn_gru_layer_presplit_f32")
        ctx.adj, ctx.plan, ctx.eps = adj, plan, eps
        # The planes are what the backward reads (recompute pass, dx / dW_ih kernel).  Keeping them for every layer of a config-5 window is
        # 132 GB (226 GB peak of 288); beyond a budget of kept bytes (CTGCN_TRAIN_PLANES_GB, default 32) a layer keeps only its INPUT — which
        # autograd holds anyway as the previous layer's output — and writes the planes again in its backward: the same kernel on the same
        # input, bit-identical gradients, +1 ms per 1 M-node layer.
        nbytes = ws.numel()
        keep = _kept_planes["bytes"] + nbytes <= _kept_planes["budget"]
        ctx.kept = keep
        if keep:                                          # accounted for as long as the planes live (freed by the backward, or with a dropped graph)
            import weakref
            _kept_planes["bytes"] += nbytes
            weakref.finalize(ws, _release_planes, nbytes)
        ctx.save_for_backward(ws if keep else x_d, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        ws, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b = ctx.saved_tensors
        if not ctx.kept:
            with torch.cuda.device(ws.device):
                ws, _ = aggregate_split_planes(ws, ctx.adj, 1, ctx.plan, gather_bias=ctx.gather_bias)          # ws was the layer's input x
        adj, plan, eps = ctx.adj, ctx.plan, ctx.eps
        n, K, hid = adj.n, adj.K, w_hh.shape[1]
        dev = ws.device
        w_ih_d, w_hh_d = w_ih.detach(), w_hh.detach().contiguous()
        bias, b_hn = _fold_gru_bias(b_ih, b_hh, hid)
        if not (dout.dim() == 2 and dout.stride(1) == 1 and dout.stride(0) >= hid and dout.stride(0) % 2 == 0 and dout.data_ptr() % 8 == 0):
            dout = dout.contiguous()       # a column of a [n, T, 128] gradient is read in place
        order = plan["order"] if plan is not None else None
        tmask = plan["tile_mask"] if plan is not None else None
        chunks = _row_chunks(lib, n, K, hid)
        cmax = chunks[0][1]
        nb = int(lib.ctgcn_gru_bwd_blocks(cmax))
        with torch.cuda.device(dev):
            gates = torch.empty(cmax * K, 3 * hid, dtype=torch.float32, device=dev)      # r, z, q: n is rebuilt in the backward kernel
            hseq = torch.empty(cmax * K, hid, dtype=torch.float32, device=dev)
            presum = torch.empty(cmax, hid, dtype=torch.float32, device=dev)
            dpre = torch.empty(cmax, hid, dtype=torch.float32, device=dev)
            dgi = torch.empty(cmax * K, 3 * hid, dtype=torch.float32, device=dev)
            dw_hh_part = torch.zeros(nb, 3 * hid, hid, dtype=torch.float32, device=dev)
            dw_ih_part = torch.zeros(nb, 3 * hid, hid, dtype=torch.float32, device=dev)
            dbn_part = torch.zeros(nb, hid, dtype=torch.float32, device=dev)
            dbi_part = torch.zeros(nb, 3 * hid, dtype=torch.float32, device=dev)
            ln_part = torch.empty(2048, 2 * hid, dtype=torch.float32, device=dev)
            ln_sum = torch.zeros(2 * hid, dtype=torch.float32, device=dev)
            Z = torch.empty(n, K, hid, dtype=torch.float32, device=dev)
            S0 = torch.empty(n, hid, dtype=torch.float32, device=dev) if adj.self_loop else None
            for lo, cnt in chunks:
                tm = _u32ptr(tmask, (lo // 16) * (2 if K > 32 else 1))      # one mask word per 16-row tile, two beyond 32 steps
                od = _u32ptr(order, lo)
                fresh = (plan["new_rows"] / float(n * K)) if plan is not None else 1.0     # fraction of (position, step) rows that bring a new x
                with _timed("gru_layer", rows=cnt, steps=K, reduce_sum=True, presplit=True, save=True, new_rows=int(cnt * K * fresh)):
                    check(lib.ctgcn_gru_layer_presplit_save_f32(cnt, K, hid, ptr(ws), n * K, lo, ptr(w_ih_d), ptr(w_hh_d), ptr(bias), ptr(b_hn), tm,
                                                                ptr(gates), ptr(hseq), ptr(presum), _stream()), "ctgcn_gru_layer_presplit_save_f32")
                dy = dout if order is not None else dout[lo:lo + cnt]
                check(lib.ctgcn_layernorm_bwd_f32(cnt, 1, hid, ptr(presum), ptr(dy), dy.stride(0), ptr(ln_w.detach()), eps, ptr(dpre), ptr(ln_part),
                                                  ln_part.shape[0], od, _stream()), "ctgcn_layernorm_bwd_f32")
                ln_sum += ln_part.sum(0)
                with _timed("gru_bwd_rec", rows=cnt, steps=K, fresh=fresh, per_step=False):
                    check(lib.ctgcn_gru_bwd_rec_f32(cnt, K, hid, ptr(gates), 3, ptr(hseq), ptr(dpre), None, ptr(w_hh_d), tm, ptr(dgi), ptr(dw_hh_part),
                                                    ptr(dbn_part), nb, 1, _stream()), "ctgcn_gru_bwd_rec_f32")
                with _timed("gru_bwd_in", rows=cnt, steps=K, fresh=fresh, z_out=True):
                    check(lib.ctgcn_gru_bwd_in_f32(cnt, K, hid, ptr(dgi), ptr(w_ih_d), tm, ptr(ws), n * K, lo, None, 0, None,
                                                   ptr(Z) if order is not None else ptr(Z[lo:]),
                                                   ptr(S0) if (S0 is None or order is not None) else ptr(S0[lo:]), od, 1 if adj.nested else 0,
                                                   ptr(dw_ih_part), ptr(dbi_part), nb, 1, _stream()), "ctgcn_gru_bwd_in_f32")
            need_gb = ctx.gather_bias is not None and ctx.needs_input_grad[9]
            dX = _aggregate_gather(adj, Z, S0, True) if (ctx.needs_input_grad[0] or need_gb) else None
        dw_ih = dw_ih_part.sum(0)
        dw_hh = dw_hh_part.sum(0)
        db_ih = db_hh = None
        if b_ih is not None:
            db_ih = dbi_part.sum(0)
            db_hh = torch.cat([db_ih[: 2 * hid], dbn_part.sum(0)])
        # (gather_bias: dX is the gradient of x[row] + gather_bias, so the bias takes its column sum, as in _LinearOfIdentity.backward)
        d_gb = dX.sum(0) if (ctx.gather_bias is not None and ctx.needs_input_grad[9]) else None
        return dX, None, dw_ih, dw_hh, db_ih, db_hh, ln_sum[:hid].clone(), ln_sum[hid:].clone(), None, d_gb


def _fold_gru_bias(b_ih, b_hh, hid):
    """(b_ih + b_hh on the r and z gates | b_ih on n,  b_hn) — the two bias vectors the GRU kernels take; (None, None) without bias"""
    if b_ih is None:
        return None, None
    bias = b_ih.detach().clone()
    bias[: 2 * hid] += b_hh.detach()[: 2 * hid]
    return bias, b_hh.detach()[2 * hid:].contiguous()


def core_diffusion_fused(x, adj, rnn, norm, gather_bias=None):
    """CoreDiffusion.forward (layers.py:41-62) with autograd, see _CoreDiffusionFused (core_diffusion_fused_ok decides)."""
    b_ih = rnn.bias_ih_l0 if rnn.bias else None
    b_hh = rnn.bias_hh_l0 if rnn.bias else None
    return _CoreDiffusionFused.apply(x, adj, rnn.weight_ih_l0, rnn.weight_hh_l0, b_ih, b_hh, norm.weight, norm.bias, float(norm.eps), gather_bias)


# ------------------------------------------------------------- a window of small snapshots: one launch per kernel
_GROUP_MAX_NODES = 200_000


def _compute_units(dev):
    """CUs the persistent kernels of `dev` run on — queried under THAT device (the gate asked the current device, the C side the
    tensors' device at launch; on a process with several GPUs the two could disagree and the launch refused what the gate had accepted)"""
    with torch.cuda.device(dev):
        return int(_lib.load().ctgcn_compute_units())


class _GroupTables(object):
    """(device table, host shadow) pairs of the grouped launches (include/ctgcn_hip.h, ABI 28), one per call site, window length and stream,
    kept between forwards: when a call's descriptors equal the shadow the C side writes nothing — the steady state of an inference loop,
    where the caching allocator hands the same buffers to the same places forward after forward.  The comparison is on the descriptor
    bytes, so an entry can never make a launch read a stale table; entries are small (a few KB) and least-recently-used ones go first.
    Under hipGraph capture nothing is cached: a fresh table from the capture's pool, written by the (capturable) writer kernel."""

    SLAB_BYTES = 8 << 20

    def __init__(self, limit=1024):
        import collections
        self.limit, self.entries = limit, collections.OrderedDict()
        self.slabs = {}                       # device -> [slab tensor, bytes used]: tables are carved from ONE allocation per device
        self.misses = {}                      # call site -> descriptor sets seen for the first time (diagnostic)

    def _carve(self, dev, nbytes):
        """256-byte aligned device memory for a table.  Not torch.empty per table: a table allocated on a miss changes the caching allocator's
        small pool, the next forward's bias / output tensors land elsewhere, their addresses are in the descriptors — another miss, another
        allocation: the cache never converged (measured: 4 of 6 tables rewritten per forward, for ever).  A full slab drops every entry of
        its device and starts over."""
        key = str(dev)
        need = -(-nbytes // 256) * 256
        slab = self.slabs.get(key)
        if slab is None or slab[1] + need > slab[0].numel():
            if slab is not None:
                for k in [k for k in self.entries if k[2] == key]:
                    del self.entries[k]
                self._retire(slab[0])
            slab = self.slabs[key] = [torch.empty(max(self.SLAB_BYTES, need), dtype=torch.uint8, device=dev), 0]
        view = slab[0][slab[1]: slab[1] + need]
        slab[1] += need
        return view

    def get(self, lib, site, groups, dev, desc=b""):
        """desc: the caller's descriptor bytes (its ctypes arrays).  They are part of the key: the caching allocator may alternate between two
        or three sets of addresses (a forward runs while the previous forward's output is still alive), and every set keeps its own table."""
        nbytes = int(lib.ctgcn_group_table_bytes(groups))
        if torch.cuda.is_current_stream_capturing():
            return torch.empty(nbytes, dtype=torch.uint8, device=dev), None, nbytes
        key = (site, groups, str(dev), torch.cuda.current_stream(dev).cuda_stream, hash(desc))
        e = self.entries.get(key)
        if e is None:
            self.misses[site] = self.misses.get(site, 0) + 1
            if len(self.entries) >= self.limit:            # (carved memory is not returned piecemeal: start over)
                self.entries.clear()
                for old in self.slabs.values():
                    self._retire(old[0])
                self.slabs.clear()
            e = self.entries[key] = (self._carve(dev, nbytes), ctypes.create_string_buffer(nbytes))
        else:
            self.entries.move_to_end(key)
        return e[0], e[1], nbytes

    def _retire(self, slab):
        """a slab leaves the cache: kernels queued on ANY stream may still read tables in it, so the device is drained before the caching
        allocator gets the block back (rare: a slab holds ~500 tables)"""
        torch.cuda.synchronize(slab.device)

    def clear(self):
        for old in self.slabs.values():
            self._retire(old[0])
        self.entries.clear()
        self.slabs.clear()


_group_tables = _GroupTables()


def group_launch_enabled():
    """CTGCN_GROUP=0: every snapshot launches its own kernels (round 3's path: four HIP streams overlap the tails) for A/B runs."""
    import os
    return os.environ.get("CTGCN_GROUP", "1") != "0"        # (capturable since ABI 28: the descriptor tables travel as kernel arguments)


def core_diffusion_group_ok(xs, adjs, rnns, norms):
    """The width-128 CoreDiffusion layer of a window's snapshots in ONE aggregation launch + ONE GRU layer launch
    (ctgcn_core_aggregate_split_group_f32 / ctgcn_gru_layer_presplit_group_f32): inference, >= 2 snapshots of a small graph that share
    the node set, no hub rows, every snapshot fit for the per-snapshot split path."""
    if not group_launch_enabled() or len(xs) < 2 or not xs[0].is_cuda or len(xs) > _compute_units(xs[0].device):
        return False          # the grouped GRU launch gives every snapshot at least one block of the persistent grid: longer windows take the per-snapshot path
    n = adjs[0].n
    if n > _GROUP_MAX_NODES:
        return False
    planned = None
    for x, adj, rnn, norm in zip(xs, adjs, rnns, norms):
        if adj.n != n or x.dim() != 2 or x.shape[1] != 128 or rnn.hidden_size != 128 or not aggregate_split_ok(rnn, x, adj):
            return False
        if adj.K > 32 or adj.long_rows() is not None or not isinstance(norm, torch.nn.LayerNorm) or norm.weight is None or norm.bias is None:
            return False
        p = (adj.row_plan() is not None) if row_plan_enabled() else False
        if planned is None:
            planned = p
        if p != planned:
            return False
    return True


def core_diffusion_split_group(xs, adjs, rnns, norms, outs):
    """outs[t] = LayerNorm(sum_k GRU_t(relu(cumulative A_{t,k} xs[t]))_k) for every snapshot t of the window — core_diffusion_split(d = 128)
    per snapshot, as two launches for the whole window.  Bit-identical to the per-snapshot calls (same kernels' code per snapshot)."""
    lib = _lib.load()
    T = len(xs)
    n = adjs[0].n
    dev = xs[0].device
    agg = (_lib.AggSplitGroup * T)()
    lay = (_lib.GruLayerGroup * T)()
    keep = []                                         # tensors the descriptors point at, alive until the launches are queued
    use_plan = row_plan_enabled()
    with torch.cuda.device(dev):
        for t, (x, adj, rnn, norm, out) in enumerate(zip(xs, adjs, rnns, norms, outs)):
            K = adj.K
            plan = adj.row_plan() if use_plan else None
            ws_bytes = int(lib.ctgcn_core_aggregate_split_workspace_bytes(n, 128, K, 1, 0))
            ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
            bias, b_hn = _gru_bias(rnn, 128)
            w_ih, w_hh = rnn.weight_ih_l0.detach(), rnn.weight_hh_l0.detach().contiguous()
            keep.append((ws, bias, b_hn, w_hh, x))
            a = agg[t]
            a.row_ptr, a.col_idx, a.val, a.slot = ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot)
            a.X, a.ldx, a.K, a.flags = ptr(x), x.stride(0), K, adj.flags | _lib.F_RELU
            a.row_order = ptr(plan["order"]) if plan is not None else None
            a.tile_mask = ptr(plan["tile_mask"]) if plan is not None else None
            a.workspace, a.workspace_bytes = ptr(ws), ws_bytes
            g = lay[t]
            g.planes, g.w_ih, g.w_hh, g.bias_gi, g.b_hn = ptr(ws), ptr(w_ih), ptr(w_hh), ptr(bias), ptr(b_hn)
            g.ln_weight, g.ln_bias, g.ln_eps, g.steps = ptr(norm.weight), ptr(norm.bias), float(norm.eps), K
            g.out, g.ld_out = ptr(out), out.stride(0)
            g.row_order, g.tile_mask = a.row_order, a.tile_mask
            g.work = (plan["new_rows"] if plan is not None else n * K) + n * K
        tb_agg, sh_agg, tb_bytes = _group_tables.get(lib, "agg128", T, dev, bytes(agg))
        tb_lay, sh_lay, _ = _group_tables.get(lib, "layer128", T, dev, bytes(lay))
        nnz = sum(adj.nnz for adj in adjs)
        rows_written = sum((adj.row_plan()["new_rows"] if use_plan else n * adj.K) for adj in adjs)
        with _timed("agg_fwd", n=n, d=128, K=max(adj.K for adj in adjs), nnz=nnz, split=True, group=T, rows_written=rows_written,
                    K_sum=sum(adj.K for adj in adjs)):
            check(lib.ctgcn_core_aggregate_split_group_f32(T, n, 128, agg, ptr(tb_agg), tb_bytes, sh_agg, _stream()), "ctgcn_core_aggregate_split_group_f32")
        with _timed("gru_layer", rows=n, steps=max(adj.K for adj in adjs), reduce_sum=True, presplit=True, group=T, new_rows=rows_written,
                    row_steps=sum(n * adj.K for adj in adjs)):
            check(lib.ctgcn_gru_layer_presplit_group_f32(T, n, 128, lay, ptr(tb_lay), tb_bytes, sh_lay, _stream()), "ctgcn_gru_layer_presplit_group_f32")
    del keep
    return outs


def core_diffusion_wide_group_ok(xs, adjs, rnns, norms):
    """The first CoreDiffusion layer (d_in != 128: the 500-wide GRU input of the 'C' configs, layers.py:59) of a window's snapshots in one
    launch per kernel — aggregation into operand planes shared by the window, ONE panel GEMM over all snapshots' rows, one recurrence launch:
    the conditions of core_diffusion_group_ok with the split GEMM (packed weights) as consumer."""
    if not group_launch_enabled() or len(xs) < 2 or not xs[0].is_cuda or len(xs) > _compute_units(xs[0].device):
        return False
    if forward_split_mode() != 2 or not plane_cache_enabled():
        return False
    n, d = adjs[0].n, xs[0].shape[1] if xs[0].dim() == 2 else 0
    if n > _GROUP_MAX_NODES or d == 128:
        return False
    planned = None
    for x, adj, rnn, norm in zip(xs, adjs, rnns, norms):
        if adj.n != n or x.dim() != 2 or x.shape[1] != d or rnn.hidden_size != 128 or not aggregate_split_ok(rnn, x, adj):
            return False
        if adj.K > 32 or adj.long_rows() is not None or not isinstance(norm, torch.nn.LayerNorm) or norm.weight is None or norm.bias is None:
            return False
        p = (adj.row_plan(adj.PLAN_TILE_GEMM) is not None) if row_plan_enabled() else False
        if planned is None:
            planned = p
        if p != planned:
            return False
    return True


_panel_group_cache = {}


def _panel_groups(padded, dev):
    """int32 [sum(padded) / 128] on the device: the group of every 128-row panel of the shared operand planes (a function of the graphs'
    row counts only: built once per window shape)"""
    key = (str(dev), tuple(padded))
    hit = _panel_group_cache.get(key)
    if hit is None:
        if len(_panel_group_cache) > 64:
            _panel_group_cache.clear()
        counts = torch.tensor([p // 128 for p in padded], dtype=torch.int64)
        hit = _panel_group_cache[key] = torch.repeat_interleave(torch.arange(len(padded), dtype=torch.int32), counts).to(dev)
    return hit


def core_diffusion_wide_group(xs, adjs, rnns, norms, outs):
    """outs[t] = LayerNorm(sum_k GRU_t(relu(cumulative A_{t,k} xs[t]))_k) for every snapshot t — core_diffusion_split(d_in != 128) per snapshot,
    as three launches for the whole window (reference models.py:243-247 loops over the snapshots).  The operand rows of all snapshots (compact
    under the row plans, every snapshot padded to whole 128-row panels) share one pair of planes and one gi buffer.  Bit-identical to the
    per-snapshot calls: the same kernels' code per row."""
    lib = _lib.load()
    T = len(xs)
    n, d = xs[0].shape
    dev = xs[0].device
    hid, n_out = 128, 384
    kp = -(-d // 64) * 64
    use_plan = row_plan_enabled()
    plans = [adj.row_plan(adj.PLAN_TILE_GEMM) if use_plan else None for adj in adjs]
    rows = [(pl["operand_rows"] if pl is not None else n * adj.K) for pl, adj in zip(plans, adjs)]
    padded = [-(-r // 128) * 128 for r in rows]
    first = [0] * T
    for t in range(1, T):
        first[t] = first[t - 1] + padded[t - 1]
    total = first[-1] + padded[-1]
    agg = (_lib.AggSplitGroup * T)()
    seq = (_lib.GruSeqGroup * T)()
    w_arr, b_arr = (ctypes.c_void_p * T)(), (ctypes.c_void_p * T)()
    keep = []
    with torch.cuda.device(dev):
        p1 = torch.empty(total * kp, dtype=torch.float16, device=dev)
        p2 = torch.empty(total * kp, dtype=torch.float16, device=dev)
        sc = torch.empty(total, dtype=torch.float32, device=dev)
        gi = torch.empty(total, n_out, dtype=torch.float32, device=dev)
        pg = _panel_groups(padded, dev)
        for t, (x, adj, rnn, norm, out, plan) in enumerate(zip(xs, adjs, rnns, norms, outs, plans)):
            K = adj.K
            bias, b_hn = _gru_bias(rnn, hid)
            w_hh = rnn.weight_hh_l0.detach().contiguous()
            wp = _plane_cache.packed(rnn.weight_ih_l0, lib)
            keep.append((bias, b_hn, w_hh, wp, x))
            a = agg[t]
            a.row_ptr, a.col_idx, a.val, a.slot = ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(adj.slot)
            a.X, a.ldx, a.K, a.flags = ptr(x), x.stride(0), K, adj.flags | _lib.F_RELU
            a.row_order = ptr(plan["order"]) if plan is not None else None
            a.tile_mask = ptr(plan["tile_mask"]) if plan is not None else None
            a.tile_base = ptr(plan["tile_base"]) if plan is not None else None
            a.workspace, a.workspace_bytes = None, 0
            a.planes1 = ctypes.c_void_p(p1.data_ptr() + first[t] * kp * 2)
            a.planes2 = ctypes.c_void_p(p2.data_ptr() + first[t] * kp * 2)
            a.scales = ctypes.c_void_p(sc.data_ptr() + first[t] * 4)
            w_arr[t], b_arr[t] = wp.data_ptr(), (bias.data_ptr() if bias is not None else None)
            g = seq[t]
            g.gi, g.w_hh, g.b_hn = ctypes.c_void_p(gi.data_ptr() + first[t] * n_out * 4), ptr(w_hh), ptr(b_hn)
            g.ln_weight, g.ln_bias, g.ln_eps, g.steps = ptr(norm.weight), ptr(norm.bias), float(norm.eps), K
            g.out, g.ld_out = ptr(out), out.stride(0)
            g.row_order, g.tile_mask, g.tile_base = a.row_order, a.tile_mask, a.tile_base
            g.work = n * K + rows[t]
        tb_agg, sh_agg, tb_bytes = _group_tables.get(lib, "aggwide", T, dev, bytes(agg))
        tb_lin, sh_lin, _ = _group_tables.get(lib, "linwide", T, dev, bytes(w_arr) + bytes(b_arr))
        tb_seq, sh_seq, _ = _group_tables.get(lib, "seqwide", T, dev, bytes(seq))
        nnz = sum(adj.nnz for adj in adjs)
        Kmax = max(adj.K for adj in adjs)
        with _timed("agg_fwd", n=n, d=d, K=Kmax, nnz=nnz, split=True, group=T, rows_written=sum(rows), K_sum=sum(adj.K for adj in adjs)):
            check(lib.ctgcn_core_aggregate_split_group_f32(T, n, d, agg, ptr(tb_agg), tb_bytes, sh_agg, _stream()), "ctgcn_core_aggregate_split_group_f32")
        with _timed("linear_split", rows=total, k=d, n_out=n_out, presplit=True, group=T):
            check(lib.ctgcn_linear_packed_group_f32(T, total, n_out, d, ptr(p1), ptr(p2), ptr(sc), ptr(pg), w_arr, b_arr, _lib.ACT_NONE, ptr(gi), n_out,
                                                    ptr(tb_lin), tb_bytes, sh_lin, _stream()), "ctgcn_linear_packed_group_f32")
        with _timed("gru_seq", rows=n, steps=Kmax, group=T, row_steps=sum(n * adj.K for adj in adjs)):
            check(lib.ctgcn_gru_seq_group_f32(T, n, hid, seq, ptr(tb_seq), tb_bytes, sh_seq, _stream()), "ctgcn_gru_seq_group_f32")
    del keep
    return outs


def linear_of_identity_group(weights, biases):
    """[W_t^T + b_t for t] — nn.Linear applied to one-hot features (helper.py:161-172 with x = I, layers.py:95-106) for every snapshot of a
    window in ONE transpose launch (inference; weights [d, n] fp32 of one shape and stride)."""
    lib = _lib.load()
    T = len(weights)
    d, n = weights[0].shape
    dev = weights[0].device
    ws = [w.detach() for w in weights]
    outs = [torch.empty(n, d, dtype=torch.float32, device=dev) for _ in range(T)]
    w_arr, o_arr = (ctypes.c_void_p * T)(*[w.data_ptr() for w in ws]), (ctypes.c_void_p * T)(*[o.data_ptr() for o in outs])
    has_bias = all(b is not None for b in biases)
    b_arr = (ctypes.c_void_p * T)(*[b.detach().data_ptr() for b in biases]) if has_bias else None
    with torch.cuda.device(dev):
        table, shadow, tb_bytes = _group_tables.get(lib, "transpose", T, dev, bytes(w_arr) + bytes(o_arr) + (bytes(b_arr) if has_bias else b""))
        with _timed("transpose_bias", n=n, d=d, group=T):
            check(lib.ctgcn_transpose_bias_group_f32(T, n, d, w_arr, ws[0].stride(0), b_arr, o_arr, d, ptr(table), tb_bytes, shadow, _stream()),
                  "ctgcn_transpose_bias_group_f32")
    return outs


def linear_of_identity_group_ok(weights, biases):
    if not group_launch_enabled() or len(weights) < 2 or len(weights) > 1024:
        return False
    w0 = weights[0]
    none = biases[0] is None
    for w, b in zip(weights, biases):
        if not (w.is_cuda and w.dtype == torch.float32 and w.dim() == 2 and w.shape == w0.shape and w.stride() == w0.stride() and w.stride(1) == 1
                and w.device == w0.device):
            return False
        if (b is None) != none or (b is not None and not (b.is_cuda and b.dtype == torch.float32 and b.is_contiguous())):
            return False
    return True


def _accumulate_tn(out, a2d, b2d):
    """out[M,N] += a2d[R,M]^T @ b2d[R,N] for R >> M,N (weight gradients: R = rows*steps).  A plain TN GEMM with a
    384x128 output only fills a few dozen workgroups; splitting R into S batches (strided batched GEMM, no copies)
    and summing the S partial products keeps all CUs busy."""
    R, M = a2d.shape
    S = 1
    while S < 256 and R % (2 * S) == 0 and R // (2 * S) >= 1024:
        S *= 2
    if S == 1:
        out.addmm_(a2d.t(), b2d)
        return
    part = torch.bmm(a2d.view(S, R // S, M).transpose(1, 2), b2d.view(S, R // S, b2d.shape[1]))
    out += part.sum(0)


def _zero_rnn_grads(seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b):
    """the nine gradients of _GruSeq / _LstmSeq for an input without rows"""
    z = lambda t: None if t is None else torch.zeros_like(t)
    return torch.zeros_like(seq), z(w_ih), z(w_hh), z(b_ih), z(b_hh), z(ln_w), z(ln_b), None, None


class _GruSeq(torch.autograd.Function):
    """LayerNorm(sum_t GRU(seq)_t) or LayerNorm(GRU(seq)).  Forward = the fused inference kernels.  Backward
    recomputes the raw h sequence and the gates chunk by chunk (so nothing but `seq` is kept alive between forward
    and backward), runs the HIP backward recurrence and leaves the weight/input GEMMs to hipBLASLt."""

    @staticmethod
    def forward(ctx, seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, eps, reduce_sum, resident_backward=True):
        hid = w_hh.shape[1]
        ctx.resident_backward = resident_backward
        if b_ih is not None:
            bias = b_ih.detach().clone()
            bias[: 2 * hid] += b_hh.detach()[: 2 * hid]
            b_hn = b_hh.detach()[2 * hid:].contiguous()
        else:
            bias, b_hn = None, None
        seq_c = seq.contiguous()
        # d_in != hidden (the 500-wide first layer): the projection gi of a call that runs in one chunk is kept for the backward when it fits
        # the budget of kept training buffers (CTGCN_TRAIN_PLANES_GB, shared with _CoreDiffusionFused's planes) — the recompute pass then
        # skips the split of x and the GEMM (Enron-like: 0.7 of ~6 ms per snapshot).  The same bits: it IS the forward's gi.
        kept = [] if (seq_c.shape[2] != hid and keep_projection_enabled()
                      and _kept_planes["bytes"] + seq_c.shape[0] * seq_c.shape[1] * 3 * hid * 4 <= _kept_planes["budget"]) else None
        out = _gru_forward(seq_c, w_ih.detach(), w_hh.detach().contiguous(), bias, b_hn, ln_w, ln_b, eps, reduce_sum, keep_gi=kept)
        ctx.save_for_backward(seq_c, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)
        ctx.eps, ctx.reduce_sum = eps, reduce_sum
        ctx.kept_gi = None
        if kept:
            import weakref
            gi_buf, blocked = kept[0]
            nbytes = gi_buf.numel() * 4
            _kept_planes["bytes"] += nbytes
            weakref.finalize(gi_buf, _release_planes, nbytes)
            ctx.kept_gi = (gi_buf, blocked)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b = ctx.saved_tensors
        reduce_sum, eps = ctx.reduce_sum, ctx.eps
        rows, steps, d_in = seq.shape
        hid = w_hh.shape[1]
        dev = seq.device
        if rows == 0:                     # an empty node slice (a snapshot-parallel rank that owns nothing): all gradients are zero
            return _zero_rnn_grads(seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)
        w_ih_d, w_hh_d = w_ih.detach(), w_hh.detach().contiguous()
        if b_ih is not None:
            bias = b_ih.detach().clone()
            bias[: 2 * hid] += b_hh.detach()[: 2 * hid]
            b_hn = b_hh.detach()[2 * hid:].contiguous()
        else:
            bias, b_hn = None, None
        # a [rows, 128] gradient that is a column of a [rows, T, 128] tensor (the last CoreDiffusion of a snapshot under the temporal GRU)
        # is read in place by the LayerNorm backward kernel; anything else is made dense
        strided_ok = (ln_w is not None and reduce_sum and dout.dim() == 2 and dout.stride(1) == 1 and dout.stride(0) >= hid
                      and dout.stride(0) % 2 == 0 and dout.data_ptr() % 8 == 0)
        if not strided_ok:
            dout = dout.contiguous()
        dseq = torch.empty_like(seq)
        dw_ih = torch.zeros_like(w_ih_d)
        dw_hh = torch.zeros_like(w_hh_d)
        db_all = torch.zeros(4 * hid, dtype=torch.float32, device=dev)                      # [d_gi (3h) | d_ghn (h)] column sums
        bias_part = torch.empty(512, 4 * hid, dtype=torch.float32, device=dev)
        dln_w = torch.zeros(hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        dln_b = torch.zeros(hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        ln_part = torch.empty(2048, 2 * hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        chunks = _row_chunks(lib, rows, steps, hid)
        cmax = chunks[0][1]
        kept_gi, ctx.kept_gi = ctx.kept_gi, None          # used once: the buffer becomes d_gi below (a second backward recomputes)
        if kept_gi is not None and len(chunks) != 1:
            kept_gi = None
        gi_flat = kept_gi[0] if kept_gi is not None else _gi_buffer(cmax, steps, hid, dev)      # reused as d_gi
        gates_buf = torch.empty(cmax * steps, 4 * hid, dtype=torch.float32, device=dev)
        hseq_buf = torch.empty(cmax, steps, hid, dtype=torch.float32, device=dev)
        dghn_buf = torch.empty(cmax * steps, hid, dtype=torch.float32, device=dev)
        split = split_mfma_enabled()
        # d_in = hidden = 128: the two resident-weight backward kernels of ctgcn_gru_bwd.hip (backward recurrence + dW_hh; dx + dW_ih) instead
        # of gru_seq_bwd_x3 + gru_dx_x3 + 2 x gru_dw_x3: d_gi is the only intermediate, dGH / dGHn never leave the CU
        # (resident_backward=False, GCRN: the step-wise kernels below, whose sums stay at an fp32 run's error)
        fused_bwd = ctx.resident_backward and split and train_fused_enabled() and forward_split_mode() == 2 and d_in == hid and steps <= 64 \
            and w_ih_d.is_contiguous()
        if fused_bwd:
            nb = int(lib.ctgcn_gru_bwd_blocks(cmax))
            dw_part_ih = torch.zeros(nb, 3 * hid, hid, dtype=torch.float32, device=dev)
            dw_part_hh = torch.zeros(nb, 3 * hid, hid, dtype=torch.float32, device=dev)
            dbn_part = torch.zeros(nb, hid, dtype=torch.float32, device=dev)
            dbi_part = torch.zeros(nb, 3 * hid, dtype=torch.float32, device=dev)
        elif split:
            dw_part_ih = torch.empty(_DW_PAIRS, 3 * hid, hid, dtype=torch.float32, device=dev)    # summed once at the end
            dw_part_hh = torch.empty(_DW_PAIRS, 3 * hid, hid, dtype=torch.float32, device=dev)
        wide_dw = split and not fused_bwd and hid < d_in <= 1024 and wide_weight_grad_enabled() and seq.stride(2) == 1
        if wide_dw:
            wide_cols = [min(c0, d_in - hid) for c0 in range(0, d_in, hid)]
            dw_part_wide = [torch.empty(_DW_PAIRS, 3 * hid, hid, dtype=torch.float32, device=dev) for _ in wide_cols]
        if not split:                                # read only by the library-GEMM weight gradients below (it was allocated and
            hprev_buf = torch.zeros(cmax, steps, hid, dtype=torch.float32, device=dev)     # zeroed on every split-path backward); [:, 0] stays 0
        with torch.cuda.device(dev):
            for lo, n in chunks:
                x2d = seq[lo:lo + n].reshape(n * steps, d_in)
                gates, hseq = gates_buf[: n * steps], hseq_buf[:n]
                gi = gi_flat[: n * steps * 3 * hid].view(n * steps, 3 * hid)                 # the [rows, 3h] view (d_gi later)
                xs = seq[lo:lo + n]
                if forward_split_mode() == 2 and d_in == hid and layer_kernel_enabled(False) and xs.stride(2) == 1 and xs.stride(1) % 4 == 0 \
                        and xs.stride(0) == steps * xs.stride(1) and xs.data_ptr() % 16 == 0 and w_ih_d.is_contiguous():
                    # recompute in the layer kernel: raw h sequence + gates, the projection consumed from the accumulators (bit-identical
                    # to the pair below, without writing and re-reading gi)
                    with _timed("gru_layer", rows=n, steps=steps, reduce_sum=False, save=True):
                        check(lib.ctgcn_gru_layer_f32(n, steps, d_in, hid, ptr(xs), xs.stride(1), ptr(w_ih_d), ptr(w_hh_d), ptr(bias), ptr(b_hn), None, None,
                                                      0.0, 0, ptr(hseq), 0, ptr(gates), None, 0, _stream()), "ctgcn_gru_layer_f32")
                else:
                    blocked = kept_gi[1] if kept_gi is not None else _project(x2d, w_ih_d, bias, gi_flat, steps_blocked=steps)
                    check(lib.ctgcn_gru_seq_f32(n, steps, hid, ptr(gi_flat), ptr(w_hh_d), ptr(b_hn), None, None, 0.0, 0, ptr(hseq), 0,
                                                ptr(gates), forward_split_mode(), 1 if blocked else 0, None, None, None, _stream()), "ctgcn_gru_seq_f32")
                # LayerNorm backward on the recomputed pre-norm values (dense, tiny next to the recurrence)
                g_out = dout[lo:lo + n]
                if ln_w is not None:
                    # one HIP pass: sum over steps (reduce_sum), mean / rstd recomputed, dpre, per-block partials of d gamma / d beta
                    ln_rows = n if reduce_sum else n * steps
                    dpre = torch.empty((n, hid) if reduce_sum else (n, steps, hid), dtype=torch.float32, device=dev)
                    check(lib.ctgcn_layernorm_bwd_f32(ln_rows, steps if reduce_sum else 1, hid, ptr(hseq), ptr(g_out), g_out.stride(0) if reduce_sum else 0,
                                                      ptr(ln_w.detach()), eps, ptr(dpre), ptr(ln_part), ln_part.shape[0], None, _stream()), "ctgcn_layernorm_bwd_f32")
                    ln_sum = ln_part.sum(0)
                    dln_w += ln_sum[:hid]
                    dln_b += ln_sum[hid:]
                else:
                    dpre = g_out
                dpre = dpre.contiguous()
                dgi, dghn = gi, dghn_buf[: n * steps]                                       # gi is dead: reuse as d_gi
                if fused_bwd:
                    dsq = dseq[lo:lo + n]
                    with _timed("gru_bwd_rec", rows=n, steps=steps, fresh=1.0, per_step=not reduce_sum):
                        check(lib.ctgcn_gru_bwd_rec_f32(n, steps, hid, ptr(gates), 4, ptr(hseq), ptr(dpre) if reduce_sum else None,
                                                        None if reduce_sum else ptr(dpre), ptr(w_hh_d), None, ptr(dgi), ptr(dw_part_hh), ptr(dbn_part),
                                                        nb, 1, _stream()), "ctgcn_gru_bwd_rec_f32")
                    with _timed("gru_bwd_in", rows=n, steps=steps, fresh=1.0, z_out=False):
                        check(lib.ctgcn_gru_bwd_in_f32(n, steps, hid, ptr(dgi), ptr(w_ih_d), None, None, 0, 0, ptr(xs), xs.stride(1), ptr(dsq), None, None,
                                                       None, 0, ptr(dw_part_ih), ptr(dbi_part), nb, 1, _stream()), "ctgcn_gru_bwd_in_f32")
                    continue
                check(lib.ctgcn_gru_seq_bwd_f32(n, steps, hid, ptr(gates), ptr(hseq), None if reduce_sum else ptr(dpre),
                                                ptr(dpre) if reduce_sum else None, ptr(w_hh_d), ptr(dgi), ptr(dghn),
                                                ptr(bias_part), bias_part.shape[0], 1 if split_mfma_enabled() else 0, _stream()),
                      "ctgcn_gru_seq_bwd_f32")
                _project_grad(dgi, w_ih, dseq[lo:lo + n].view(n * steps, d_in))        # the parameter itself: its transpose is cached by identity + version
                db_all += bias_part.sum(0)          # per-block column sums written by the kernel (no re-read of d_gi / d_ghn)
                if split and d_in == hid:
                    _weight_grad(dw_part_ih, dgi, dgi[:, 2 * hid:], x2d, steps, False, lo > 0)
                elif wide_dw:
                    # d_in = 500 (the 'C' configs' first layer): the 128-column weight-gradient kernel on column slices of x (the last one
                    # moved left to end at d_in: its overlap with the slice before is computed twice and stored once) — 4 x 0.26 ms per
                    # Enron-like snapshot against 1.6 ms of the fp32 library TN GEMM (which already runs at 104 TFLOP/s)
                    for part_, c0 in zip(dw_part_wide, wide_cols):
                        _weight_grad(part_, dgi, dgi[:, 2 * hid:], x2d[:, c0:], steps, False, lo > 0)
                else:
                    _accumulate_tn(dw_ih, dgi, x2d)
                if split:                            # h_{t-1} is read from the h sequence with the shift applied in the kernel
                    _weight_grad(dw_part_hh, dgi, dghn, hseq.view(n * steps, hid), steps, True, lo > 0)
                else:
                    hprev = hprev_buf[:n]
                    hprev[:, 1:] = hseq[:, :-1]
                    hp2d = hprev.view(n * steps, hid)
                    _accumulate_tn(dw_hh[: 2 * hid], dgi[:, : 2 * hid], hp2d)
                    _accumulate_tn(dw_hh[2 * hid:], dghn, hp2d)
        if fused_bwd:
            db_all[: 3 * hid] = dbi_part.sum(0)
            db_all[3 * hid:] = dbn_part.sum(0)
        if split:
            dw_hh += dw_part_hh.sum(0)
            if d_in == hid:
                dw_ih += dw_part_ih.sum(0)
            elif wide_dw:
                for part_, c0 in zip(dw_part_wide, wide_cols):
                    dw_ih[:, c0:c0 + hid] = part_.sum(0)
        db_ih = db_hh = None
        if b_ih is not None:
            db_ih = db_all[: 3 * hid].clone()
            db_hh = torch.cat([db_all[: 2 * hid], db_all[3 * hid:]])
        return dseq, dw_ih, dw_hh, db_ih, db_hh, dln_w, (dln_b if ln_b is not None else None), None, None, None


def lstm_fused_ok(rnn, seq):
    """Fused LSTM recurrence (forward and backward): hidden 128, single layer, batch_first, fp32 CUDA."""
    return (isinstance(rnn, torch.nn.LSTM) and rnn.hidden_size == 128 and rnn.num_layers == 1 and not rnn.bidirectional
            and rnn.batch_first and getattr(rnn, "proj_size", 0) == 0 and seq.is_cuda and seq.dtype == torch.float32)


def _lstm_forward(seq, w_ih, w_hh, bias, ln_w, ln_b, eps, reduce_sum):
    """LayerNorm(sum_t LSTM(seq)_t) / LayerNorm(LSTM(seq)): library GEMM for the input projection, recurrence in ctgcn_lstm_seq_f32."""
    lib = _lib.load()
    rows, steps, d_in = seq.shape
    hid = w_hh.shape[1]
    out = torch.empty((rows, hid) if reduce_sum else (rows, steps, hid), dtype=torch.float32, device=seq.device)
    if rows == 0:
        return out
    chunks = _row_chunks(lib, rows, steps, hid)
    gi_buf = torch.empty(chunks[0][1] * steps, 4 * hid, dtype=torch.float32, device=seq.device)
    with torch.cuda.device(seq.device):
        for lo, n in chunks:
            gi = gi_buf[: n * steps]
            x2d = seq[lo:lo + n].reshape(n * steps, d_in)
            if bias is None:
                torch.mm(x2d, w_ih.t(), out=gi)
            else:
                torch.addmm(bias, x2d, w_ih.t(), out=gi)
            with _timed("lstm_seq", rows=n, steps=steps):
                check(lib.ctgcn_lstm_seq_f32(n, steps, hid, ptr(gi), ptr(w_hh), ptr(ln_w), ptr(ln_b), eps, 1 if reduce_sum else 0,
                                             ptr(out[lo:lo + n]), None, _stream()), "ctgcn_lstm_seq_f32")
    return out


class _LstmSeq(torch.autograd.Function):
    """LayerNorm(sum_t LSTM(seq)_t) or LayerNorm(LSTM(seq)) with autograd (rnn_type = 'LSTM', layers.py:27-28 / models.py:234-235).
    Forward = the inference kernels; backward recomputes gates, cell states and the raw h sequence chunk by chunk
    (ctgcn_lstm_seq_f32 with gates_out), runs ctgcn_layernorm_bwd_f32 and ctgcn_lstm_seq_bwd_f32 and leaves d x / d W — plain GEMMs
    over the materialised d gi — to the library.  (MIOpen's LSTM needs ~27 000 tensor-op launches per config-5 window.)"""

    @staticmethod
    def forward(ctx, seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b, eps, reduce_sum):
        bias = (b_ih.detach() + b_hh.detach()) if b_ih is not None else None
        seq_c = seq.contiguous()
        out = _lstm_forward(seq_c, w_ih.detach(), w_hh.detach().contiguous(), bias, ln_w, ln_b, eps, reduce_sum)
        ctx.save_for_backward(seq_c, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)
        ctx.eps, ctx.reduce_sum = eps, reduce_sum
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b = ctx.saved_tensors
        reduce_sum, eps = ctx.reduce_sum, ctx.eps
        rows, steps, d_in = seq.shape
        hid = w_hh.shape[1]
        dev = seq.device
        if rows == 0:
            return _zero_rnn_grads(seq, w_ih, w_hh, b_ih, b_hh, ln_w, ln_b)
        w_ih_d, w_hh_d = w_ih.detach(), w_hh.detach().contiguous()
        bias = (b_ih.detach() + b_hh.detach()) if b_ih is not None else None
        dout = dout.contiguous()
        dseq = torch.empty_like(seq)
        dw_ih, dw_hh = torch.zeros_like(w_ih_d), torch.zeros_like(w_hh_d)
        db = torch.zeros(4 * hid, dtype=torch.float32, device=dev)
        bias_part = torch.empty(512, 4 * hid, dtype=torch.float32, device=dev)
        dln_w = torch.zeros(hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        dln_b = torch.zeros(hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        ln_part = torch.empty(2048, 2 * hid, dtype=torch.float32, device=dev) if ln_w is not None else None
        chunks = _row_chunks(lib, rows, steps, hid)
        cmax = chunks[0][1]
        gi_buf = torch.empty(cmax * steps, 4 * hid, dtype=torch.float32, device=dev)          # reused as d_gi
        gates_buf = torch.empty(cmax * steps, 5 * hid, dtype=torch.float32, device=dev)
        hseq_buf = torch.empty(cmax, steps, hid, dtype=torch.float32, device=dev)
        hprev_buf = torch.zeros(cmax, steps, hid, dtype=torch.float32, device=dev)            # [:, 0] stays 0
        with torch.cuda.device(dev):
            for lo, n in chunks:
                x2d = seq[lo:lo + n].reshape(n * steps, d_in)
                gi, gates, hseq = gi_buf[: n * steps], gates_buf[: n * steps], hseq_buf[:n]
                if bias is None:
                    torch.mm(x2d, w_ih_d.t(), out=gi)
                else:
                    torch.addmm(bias, x2d, w_ih_d.t(), out=gi)
                check(lib.ctgcn_lstm_seq_f32(n, steps, hid, ptr(gi), ptr(w_hh_d), None, None, 0.0, 0, ptr(hseq), ptr(gates), _stream()),
                      "ctgcn_lstm_seq_f32")
                g_out = dout[lo:lo + n]
                if ln_w is not None:
                    ln_rows = n if reduce_sum else n * steps
                    dpre = torch.empty((n, hid) if reduce_sum else (n, steps, hid), dtype=torch.float32, device=dev)
                    check(lib.ctgcn_layernorm_bwd_f32(ln_rows, steps if reduce_sum else 1, hid, ptr(hseq), ptr(g_out), 0, ptr(ln_w.detach()), eps,
                                                      ptr(dpre), ptr(ln_part), ln_part.shape[0], None, _stream()), "ctgcn_layernorm_bwd_f32")
                    ln_sum = ln_part.sum(0)
                    dln_w += ln_sum[:hid]
                    dln_b += ln_sum[hid:]
                else:
                    dpre = g_out
                dgi = gi                                                                        # gi is dead: reuse as d_gi
                check(lib.ctgcn_lstm_seq_bwd_f32(n, steps, hid, ptr(gates), None if reduce_sum else ptr(dpre), ptr(dpre) if reduce_sum else None,
                                                 ptr(w_hh_d), ptr(dgi), ptr(bias_part), bias_part.shape[0], _stream()), "ctgcn_lstm_seq_bwd_f32")
                torch.mm(dgi, w_ih_d, out=dseq[lo:lo + n].view(n * steps, d_in))
                db += bias_part.sum(0)
                _accumulate_tn(dw_ih, dgi, x2d)
                hprev = hprev_buf[:n]
                hprev[:, 1:] = hseq[:, :-1]
                _accumulate_tn(dw_hh, dgi, hprev.view(n * steps, hid))
        db_ih = db_hh = None
        if b_ih is not None:
            db_ih, db_hh = db, db.clone()
        return dseq, dw_ih, dw_hh, db_ih, db_hh, dln_w, (dln_b if ln_b is not None else None), None, None


def lstm_sequence(rnn, seq, norm, reduce_sum):
    """LayerNorm(sum_t LSTM(seq)_t) / LayerNorm(LSTM(seq)) with the recurrence in ctgcn_lstm_seq_f32; with autograd enabled the
    backward runs ctgcn_lstm_seq_bwd_f32 (see _LstmSeq)."""
    b_ih = rnn.bias_ih_l0 if rnn.bias else None
    b_hh = rnn.bias_hh_l0 if rnn.bias else None
    ln_w = None if norm is None else norm.weight
    ln_b = None if norm is None else norm.bias
    eps = 0.0 if norm is None else float(norm.eps)
    return _LstmSeq.apply(seq, rnn.weight_ih_l0, rnn.weight_hh_l0, b_ih, b_hh, ln_w, ln_b, eps, bool(reduce_sum))


def gru_sequence(rnn, seq, norm, reduce_sum, out=None, resident_backward=True):
    """LayerNorm(sum_t GRU(seq)_t) (reduce_sum) or LayerNorm(GRU(seq)) — layers.py:59-62 / models.py:249-250.
    seq [rows, steps, d_in].  Input projection (ctgcn_gru_input_proj_f32), then the recurrence, the sum over steps and the
    LayerNorm in ONE HIP kernel (ctgcn_gru_seq_f32); with autograd enabled the backward runs ctgcn_gru_seq_bwd_f32 (see
    _GruSeq).  out (inference, reduce_sum): a [rows, hidden] view with unit column stride that receives the result,
    e.g. column t of the temporal GRU's [rows, T, hidden] input.  resident_backward=False keeps the backward off the two
    resident-weight kernels (gru_bwd_rec / gru_bwd_in, d_in = hidden = 128, up to 64 steps) and on the step-wise HIP kernels every
    other shape takes (ctgcn_gru_seq_bwd_f32 + the weight-gradient kernels): slower, and as accurate as an fp32 run."""
    b_ih = rnn.bias_ih_l0 if rnn.bias else None
    b_hh = rnn.bias_hh_l0 if rnn.bias else None
    ln_w = None if norm is None else norm.weight
    ln_b = None if norm is None else norm.bias
    eps = 0.0 if norm is None else float(norm.eps)
    if out is not None:
        if torch.is_grad_enabled() and (seq.requires_grad or any(p.requires_grad for p in rnn.parameters())):
            raise RuntimeError("gru_sequence(out=...) is an inference path")
        bias, b_hn = _gru_bias(rnn, rnn.hidden_size)
        return _gru_forward(seq.contiguous(), rnn.weight_ih_l0.detach(), rnn.weight_hh_l0.detach().contiguous(), bias, b_hn,
                            ln_w, ln_b, eps, bool(reduce_sum), out=out)
    return _GruSeq.apply(seq, rnn.weight_ih_l0, rnn.weight_hh_l0, b_ih, b_hh, ln_w, ln_b, eps, bool(reduce_sum), bool(resident_backward))


# ------------------------------------------------------------------------ supervised classifier head (ctgcn_supervised.hip)
CLS_NODE, CLS_HADAMARD, CLS_DOT = _lib.CLS_NODE, _lib.CLS_HADAMARD, _lib.CLS_DOT
CLS_PULL_PIECE = 512            # incidences per piece of the pull backward (ctgcn_cls_pull_piece(); checked when the library loads an item set)
CLS_MAX_D, CLS_MAX_CLASSES = 256, 32


class ClsIncidence(object):
    """The incidence lists of one item set for ctgcn_cls_head_bwd_f32 (include/ctgcn_hip.h): node -> (item, other endpoint) in CSR
    form, cut into pieces of at most `piece` incidences, every node owning at least one (possibly empty) piece."""

    def __init__(self, row_ptr, inc_item, inc_other, piece_ptr, piece_node, piece_slot, hub_node, hub_slot_ptr):
        self.row_ptr, self.inc_item, self.inc_other = row_ptr, inc_item, inc_other
        self.piece_ptr, self.piece_node, self.piece_slot = piece_ptr, piece_node, piece_slot
        self.hub_node, self.hub_slot_ptr = hub_node, hub_slot_ptr
        self.n_pieces = piece_node.numel()
        self.n_hubs = hub_node.numel()
        self.hub_pieces = int(hub_slot_ptr[-1]) if self.n_hubs else 0


def cls_incidence(a, b, n_nodes, piece=CLS_PULL_PIECE):
    """ClsIncidence of the items (a[i]) (b None) or (a[i], b[i]); int64 tensors on any device, indices inside [0, n_nodes).
    A node's list holds its incidences as first endpoint in item order, then those as second endpoint in item order (a stable
    sort), so a pair with a == b appears twice in its node's list."""
    dev = a.device
    n = a.numel()
    item = torch.arange(n, dtype=torch.int64, device=dev)
    if b is None:
        nodes, items, other = a, item, a
    else:
        nodes, items, other = torch.cat([a, b]), torch.cat([item, item]), torch.cat([b, a])
    order = torch.sort(nodes, stable=True).indices
    deg = torch.bincount(nodes, minlength=n_nodes)
    row_ptr = torch.zeros(n_nodes + 1, dtype=torch.int64, device=dev)
    row_ptr[1:] = torch.cumsum(deg, 0)
    pieces = torch.clamp((deg + piece - 1) // piece, min=1)
    node_piece = torch.zeros(n_nodes + 1, dtype=torch.int64, device=dev)
    node_piece[1:] = torch.cumsum(pieces, 0)
    piece_node = torch.repeat_interleave(torch.arange(n_nodes, dtype=torch.int64, device=dev), pieces)
    within = torch.arange(piece_node.numel(), dtype=torch.int64, device=dev) - node_piece[piece_node]
    piece_ptr = torch.cat([row_ptr[piece_node] + within * piece, row_ptr[-1:]])
    hub_node = torch.nonzero(pieces > 1).flatten()
    hub_slot_ptr = torch.zeros(hub_node.numel() + 1, dtype=torch.int64, device=dev)
    hub_slot_ptr[1:] = torch.cumsum(pieces[hub_node], 0)
    in_hub = (pieces > 1)[piece_node]
    piece_slot = torch.where(in_hub, torch.cumsum(in_hub.to(torch.int64), 0) - 1, torch.full_like(piece_node, -1))
    return ClsIncidence(row_ptr, items[order].contiguous(), other[order].contiguous(), piece_ptr.contiguous(), piece_node.contiguous(),
                        piece_slot.contiguous(), hub_node.contiguous(), hub_slot_ptr)


class ClsItems(object):
    """One item set on the device: contiguous endpoint arrays, checked once against n_nodes by the library's host check, and the
    incidence lists of the pull backward, built on first use."""

    def __init__(self, idx, mode, n_nodes):
        _need_cuda(idx)
        idx = idx.to(torch.int64)
        if mode == CLS_NODE:
            if idx.dim() != 1:
                raise ValueError("node items are a 1-D index tensor, got shape %s" % (tuple(idx.shape),))
            self.a, self.b = idx.contiguous(), None
        else:
            if idx.dim() != 2 or idx.shape[0] != 2:
                raise ValueError("pair items are a [2, items] index tensor, got shape %s" % (tuple(idx.shape),))
            self.a, self.b = idx[0].contiguous(), idx[1].contiguous()
        self.mode, self.n_nodes, self.items = mode, int(n_nodes), self.a.numel()
        self._inc = None
        lib = _lib.load()
        if lib.ctgcn_cls_pull_piece() != CLS_PULL_PIECE:
            raise _lib.CtgcnHipError("libctgcn_hip.so cuts pull pieces at %d, ops.CLS_PULL_PIECE is %d; rebuild"
                                     % (lib.ctgcn_cls_pull_piece(), CLS_PULL_PIECE))
        with torch.cuda.device(idx.device):
            check(lib.ctgcn_cls_check_items(mode, self.items, ptr(self.a), ptr(self.b), self.n_nodes, _stream()), "ctgcn_cls_check_items")

    @property
    def incidence(self):
        if self._inc is None:
            self._inc = cls_incidence(self.a, self.b, self.n_nodes)
        return self._inc


_cls_items_cache = {}


def cls_items(idx, mode, n_nodes):
    """ClsItems of an index tensor, cached on the tensor's identity: the trainer passes the same index tensors every epoch.  The
    entry keeps the tensor alive, so its id cannot be recycled while the entry exists; an in-place change is seen by _version."""
    key = (id(idx), idx.data_ptr(), idx._version, tuple(idx.shape), int(mode), int(n_nodes))
    hit = _cls_items_cache.get(key)
    if hit is None:
        if len(_cls_items_cache) > 256:
            _cls_items_cache.clear()
        hit = _cls_items_cache[key] = (ClsItems(idx, mode, n_nodes), idx)
    return hit[0]


def _cls_rows(mat, what):
    _need_cuda(mat)
    if mat.dim() != 2 or mat.dtype != torch.float32 or (mat.shape[1] > 1 and mat.stride(1) != 1) or (mat.shape[0] > 1 and mat.stride(0) < mat.shape[1]):
        raise ValueError("%s must be a float32 [N, d] view with unit column stride" % what)
    return mat.data_ptr(), max(mat.stride(0), mat.shape[1])


def cls_head_forward(E, items, W, bias, act):
    """logits [items, C] = act(W·f + bias) (or z [items] for CLS_DOT) of ClsItems `items` over the rows of E; no autograd."""
    pe, lde = _cls_rows(E, "embedding")
    if items.n_nodes != E.shape[0]:
        raise ValueError("item set was checked against %d nodes, embedding has %d rows" % (items.n_nodes, E.shape[0]))
    dot = items.mode == CLS_DOT
    C = 0 if dot else W.shape[0]
    if not dot:
        _need_cuda(W, bias)
        if W.dtype != torch.float32 or W.dim() != 2 or W.shape[1] != E.shape[1]:
            raise ValueError("weight must be float32 [n_class, %d]" % E.shape[1])
        W = W.contiguous()
        bias = None if bias is None else bias.contiguous()
    out = torch.empty((items.items,) if dot else (items.items, C), dtype=torch.float32, device=E.device)
    if items.items == 0:
        return out
    with torch.cuda.device(E.device):
        check(_lib.load().ctgcn_cls_head_fwd_f32(items.mode, int(act), items.items, E.shape[1], C, ptr(items.a), ptr(items.b), items.n_nodes,
                                                 pe, lde, None if dot else ptr(W), None if dot else ptr(bias), ptr(out), _stream()),
              "ctgcn_cls_head_fwd_f32")
    return out


def cls_head_backward(E, items, W, dlogits, need_dE=True, need_dW=True, need_db=True, dE=None):
    """(dE, dW, db) of the head from dlogits (the gradient at the Linear's output).  dE has E's shape (dE: an optional buffer to fill)."""
    pe, lde = _cls_rows(E, "embedding")
    dot = items.mode == CLS_DOT
    d = E.shape[1]
    C = 1 if dot else W.shape[0]
    dev = E.device
    dlogits = dlogits.contiguous()
    if dlogits.dtype != torch.float32 or dlogits.numel() != items.items * C:
        raise ValueError("dlogits must be float32 with %d entries" % (items.items * C))
    need_dW = need_dW and not dot
    need_db = need_db and need_dW
    dW = torch.empty(C, d, dtype=torch.float32, device=dev) if need_dW else None
    db = torch.empty(C, dtype=torch.float32, device=dev) if need_db else None
    if need_dE and dE is None:
        dE = torch.empty_like(E)
    if items.items == 0:
        for t in (dE if need_dE else None, dW, db):
            if t is not None:
                t.zero_()
        return (dE if need_dE else None), dW, db
    inc = items.incidence if need_dE else None
    pde, ldde = _cls_rows(dE, "embedding gradient") if need_dE else (None, 0)
    lib = _lib.load()
    with torch.cuda.device(dev):
        hub_pieces = inc.hub_pieces if inc is not None else 0
        ws = torch.empty(max(lib.ctgcn_cls_head_bwd_workspace_bytes(items.items, d, C, hub_pieces), 16), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_cls_head_bwd_f32(items.mode, items.items, d, 0 if dot else C, ptr(items.a), ptr(items.b), items.n_nodes, pe, lde,
                                         None if dot else ptr(W.contiguous()), ptr(dlogits),
                                         inc.n_pieces if inc else 0, ptr(inc.piece_ptr) if inc else None, ptr(inc.piece_node) if inc else None,
                                         ptr(inc.piece_slot) if inc else None, ptr(inc.inc_item) if inc else None,
                                         ptr(inc.inc_other) if inc else None, inc.n_hubs if inc else 0,
                                         ptr(inc.hub_node) if inc and inc.n_hubs else None, ptr(inc.hub_slot_ptr) if inc and inc.n_hubs else None,
                                         hub_pieces, pde, ldde, ptr(dW), ptr(db), ptr(ws), ws.numel(), _stream()), "ctgcn_cls_head_bwd_f32")
    return (dE if need_dE else None), dW, db


def cls_loss(logits, labels, dot=False, act=0, want_prob=True, want_grad=True):
    """The loss pass: (mean loss float64[1], correct int64[1], prob or None, dlogits or None).  logits [items, C] with int64 labels
    in [0, C), or dot: logits [items] with labels in {0, 1} (BCE with logits).  act=1: dlogits also carries SELU' (see the header)."""
    _need_cuda(logits, labels)
    if logits.dtype != torch.float32 or logits.dim() != (1 if dot else 2):
        raise ValueError("logits must be float32 %s" % ("[items]" if dot else "[items, n_class]"))
    logits = logits.contiguous()
    labels = labels.to(torch.int64).contiguous()
    n = logits.shape[0]
    if labels.numel() != n or n == 0:
        raise ValueError("need one label per item and at least one item (%d labels, %d items)" % (labels.numel(), n))
    dev = logits.device
    loss = torch.empty(1, dtype=torch.float64, device=dev)
    correct = torch.empty(1, dtype=torch.int64, device=dev)
    prob = torch.empty_like(logits) if want_prob else None
    dl = torch.empty_like(logits) if want_grad else None
    lib = _lib.load()
    with torch.cuda.device(dev):
        ws = torch.empty(max(lib.ctgcn_cls_loss_workspace_bytes(n), 16), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_cls_loss_f32(CLS_DOT if dot else CLS_NODE, int(act), n, 0 if dot else logits.shape[1], ptr(logits), ptr(labels),
                                     ptr(loss), ptr(correct), ptr(prob), ptr(dl), ptr(ws), ws.numel(), _stream()), "ctgcn_cls_loss_f32")
    return loss, correct, prob, dl


_SELU_ALPHA, _SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946


class _ClsHead(torch.autograd.Function):
    """logits of an item set from (E_t, W, bias); backward: dE in E_t's layout by the pull kernel, dW, db."""

    @staticmethod
    def forward(ctx, E, W, bias, items, act):
        out = cls_head_forward(E.detach(), items, None if W is None else W.detach(), None if bias is None else bias.detach(), act)
        ctx.items, ctx.act, ctx.has_bias = items, act, bias is not None
        ctx.save_for_backward(E, W, out if act else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        E, W, out = ctx.saved_tensors
        if ctx.act:         # SELU' from the activated output: scale where out > 0, out + scale·alpha elsewhere
            dout = dout * torch.where(out > 0, torch.full_like(out, _SELU_SCALE), out + _SELU_SCALE * _SELU_ALPHA)
        need_dW = W is not None and ctx.needs_input_grad[1]
        need_db = ctx.has_bias and ctx.needs_input_grad[2]
        dE, dW, db = cls_head_backward(E.detach(), ctx.items, None if W is None else W.detach(), dout, need_dE=ctx.needs_input_grad[0],
                                       need_dW=need_dW or need_db, need_db=need_db)
        return dE, (dW if need_dW else None), db, None, None


class _ClsLoss(torch.autograd.Function):
    """(mean loss fp32 scalar, correct int64[1], probabilities) of logits; backward: grad · dlogits from the same pass."""

    @staticmethod
    def forward(ctx, logits, labels, dot):
        need = logits.requires_grad
        loss, correct, prob, dl = cls_loss(logits.detach(), labels, dot=dot, want_grad=need)
        ctx.save_for_backward(dl)
        ctx.mark_non_differentiable(correct, prob)
        return loss.to(torch.float32).reshape(()), correct, prob

    @staticmethod
    def backward(ctx, gloss, _gc, _gp):
        dl, = ctx.saved_tensors
        return (None if dl is None else dl * gloss), None, None


def cls_head(E, idx, W, bias, mode, act=0):
    """Differentiable logits [items, C] (z [items] for CLS_DOT) of the items idx over the rows of E (a strided [N, d] view is read in
    place).  idx: int64 [items] (CLS_NODE) or [2, items]; its derived tables are cached on the tensor's identity."""
    items = cls_items(idx, mode, E.shape[0])
    return _ClsHead.apply(E, W, bias, items, int(act))


def cls_loss_autograd(logits, labels, dot=False):
    """(loss, correct int64[1], prob): differentiable mean cross entropy / BCE with logits of the loss pass."""
    return _ClsLoss.apply(logits, labels, bool(dot))


# ------------------------------------------------------------------------- GCN step of the EvolveGCN baseline (ctgcn_gcn.hip)
GCN_ACT_NONE, GCN_ACT_RRELU = 0, 1
GCN_PIECE_FACTOR = 4                    # a long row's piece holds 4 x long_threshold entries (PIECE_FACTOR in ctgcn_gather.h)


def gcn_normalize(row_ptr, col, val, row_norm=False):
    """D^-1/2 A D^-1/2 (row_norm False) or D^-1 A (True) over a CSR that already holds the diagonal: the reference's
    get_normalized_adj (utils.py:65-85) in fp64 on the GPU, rounded to fp32 once.  A negative row sum raises its ValueError."""
    _need_cuda(row_ptr, col, val)
    lib = _lib.load()
    row_ptr, col = _i32(row_ptr), _i32(col)
    val = val if (val.dtype == torch.float32 and val.is_contiguous()) else val.to(torch.float32).contiguous()
    n = row_ptr.numel() - 1
    dev = val.device
    out = torch.empty_like(val)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        nbytes = lib.ctgcn_gcn_normalize_workspace_bytes(n)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_gcn_normalize_f32(n, ptr(row_ptr), ptr(col), ptr(val), 1 if row_norm else 0, ptr(out), ptr(flag), ptr(ws), nbytes,
                                          _stream()), "ctgcn_gcn_normalize_f32")
    if int(flag.item()):
        raise ValueError('invalid value encountered in power, x is negative, p is negative!')
    return out


class GcnAdj(object):
    """One normalised adjacency of the GCN step as the kernels read it: int32 row_ptr / col and fp32 val of the matrix as given, plus
    the rows longer than long_threshold entries.  gcn_layer's backward reads the same CSR as its forward, so its matrix has to be
    symmetric (check_symmetric=True verifies that once, on the device); gcn_conv's backward reads transposed(), so its need not be."""
    LONG_ROW = 2048

    def __init__(self, row_ptr, col, val, long_threshold=None, check_symmetric=False):
        _need_cuda(row_ptr, col, val)
        self.row_ptr, self.col = _i32(row_ptr), _i32(col)
        self.val = val if (val.dtype == torch.float32 and val.is_contiguous()) else val.to(torch.float32).contiguous()
        self.n = self.row_ptr.numel() - 1
        self.nnz = self.col.numel()
        self.device = self.val.device
        self.long_threshold = int(self.LONG_ROW if long_threshold is None else long_threshold)
        if self.long_threshold < 1:
            raise ValueError("long_threshold must be >= 1")
        lens = self.row_ptr[1:] - self.row_ptr[:-1]
        max_len = int(lens.max()) if self.n else 0
        self.long_rows = None
        self.pieces = 1
        if max_len > self.long_threshold:
            self.long_rows = (lens > self.long_threshold).nonzero().view(-1).to(torch.int32)
            piece = GCN_PIECE_FACTOR * self.long_threshold
            self.pieces = (max_len + piece - 1) // piece
        self.symmetric = False                   # True once _check_symmetric has passed: the matrix is then its own transpose
        if check_symmetric:
            self._check_symmetric()
        self._ws = {}
        self._transposed = None

    def _rows(self):
        counts = (self.row_ptr[1:] - self.row_ptr[:-1]).to(torch.int64)
        return torch.repeat_interleave(torch.arange(self.n, device=self.device), counts)

    def _check_symmetric(self):
        row, col = self._rows(), self.col.to(torch.int64)
        order = torch.argsort(col * self.n + row)           # the transpose's entries in row-major order
        key = row * self.n + col
        same = self.nnz == 0 or bool((key == (col * self.n + row)[order]).all())
        if same and self.nnz:
            vt = self.val[order]
            # r_i a r_j and r_j a r_i are each rounded once: two ulps of fp32 is as far apart as a symmetric matrix gets
            same = bool(((self.val - vt).abs() <= 2.0 ** -22 * torch.maximum(self.val.abs(), vt.abs())).all())
        if not same:
            raise ValueError("gcn_layer needs a symmetric matrix (its backward reads the same CSR): A != A^T")
        self.symmetric = True

    def transposed(self):
        """The GcnAdj of Â^T, with its own long-row list and workspaces: built once on the device by a stable sort of the entries by
        column (the adjacency is constant over the epochs) and cached; self when the symmetry check has passed."""
        if self.symmetric:
            return self
        if self._transposed is None:
            row, col = self._rows(), self.col.to(torch.int64)
            order = torch.argsort(col, stable=True)           # entries are in row-major order: rows stay ascending within a column
            row_ptr = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
            row_ptr[1:] = torch.bincount(col, minlength=self.n).cumsum(0)
            t = GcnAdj(row_ptr.to(torch.int32), row[order].to(torch.int32), self.val[order], self.long_threshold)
            t._transposed = self
            self._transposed = t
        return self._transposed

    @classmethod
    def from_scipy(cls, mat, device, long_threshold=None, check_symmetric=False):
        import numpy as np
        import scipy.sparse as sp
        csr = sp.csr_matrix(mat)
        csr.sum_duplicates()
        csr.sort_indices()
        if csr.nnz >= 2 ** 31 or csr.shape[0] >= 2 ** 31:
            raise ValueError("more than 2^31-1 rows or stored entries")
        return cls(torch.from_numpy(csr.indptr.astype(np.int32)).to(device), torch.from_numpy(csr.indices.astype(np.int32)).to(device),
                   torch.from_numpy(csr.data.astype(np.float32)).to(device), long_threshold, check_symmetric)

    @classmethod
    def from_sparse_tensor(cls, t, device, long_threshold=None, check_symmetric=True):
        if not t.is_sparse or t.dim() != 2 or t.shape[0] != t.shape[1]:
            raise ValueError("a square torch sparse COO matrix expected")
        t = t.to(device).coalesce()                          # row-major order, duplicates summed
        n = t.shape[0]
        idx = t.indices()
        if idx.shape[1] >= 2 ** 31 or n >= 2 ** 31:
            raise ValueError("more than 2^31-1 rows or stored entries")
        row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=idx.device)
        row_ptr[1:] = torch.bincount(idx[0], minlength=n).cumsum(0)
        return cls(row_ptr.to(torch.int32), idx[1].to(torch.int32), t.values().to(torch.float32), long_threshold, check_symmetric)

    def to_sparse_tensor(self):
        idx = torch.stack((self._rows(), self.col.to(torch.int64)))
        return torch.sparse_coo_tensor(idx, self.val, torch.Size((self.n, self.n)))

    def workspace(self, d):
        """(buffer, bytes) of the long rows' partial sums for width d; one buffer per width, reused by forward and backward"""
        if self.long_rows is None:
            return None, 0
        nbytes = self.long_rows.numel() * self.pieces * ((d + 3) // 4 * 4) * 4
        ws = self._ws.get(d)
        if ws is None:
            ws = self._ws[d] = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return ws, nbytes


def _gcn_long(adj, d):
    ws, nbytes = adj.workspace(d)
    return ptr(adj.long_rows), 0 if adj.long_rows is None else adj.long_rows.numel(), adj.long_threshold, ptr(ws), nbytes


def _gcn_fwd(adj, S, act, score_vec):
    lib = _lib.load()
    n, d = S.shape
    Y = torch.empty(n, d, dtype=torch.float32, device=S.device)
    scores = torch.empty(n, dtype=torch.float32, device=S.device) if score_vec is not None else None
    with torch.cuda.device(S.device), _timed("gcn_fwd", n=n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_gcn_layer_fwd_f32(n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(S), S.stride(0), ptr(Y), Y.stride(0), act,
                                          ptr(score_vec), ptr(scores), *_gcn_long(adj, d), _stream()), "ctgcn_gcn_layer_fwd_f32")
    return Y, scores


def _gcn_bwd(adj, dY, Y, act):
    lib = _lib.load()
    n, d = dY.shape
    dS = torch.empty(n, d, dtype=torch.float32, device=dY.device)
    with torch.cuda.device(dY.device), _timed("gcn_bwd", n=n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_gcn_layer_bwd_f32(n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(dY), dY.stride(0), ptr(Y),
                                          0 if Y is None else Y.stride(0), act, ptr(dS), dS.stride(0), *_gcn_long(adj, d), _stream()),
              "ctgcn_gcn_layer_bwd_f32")
    return dS


class _GcnLayer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, adj, act, score_vec):
        Y, scores = _gcn_fwd(adj, S, act, score_vec)
        ctx.adj, ctx.act = adj, act
        if act:
            ctx.save_for_backward(Y)
        if scores is None:
            return Y
        ctx.mark_non_differentiable(scores)
        return Y, scores

    @staticmethod
    def backward(ctx, dY, *_):
        Y = ctx.saved_tensors[0] if ctx.act else None
        return _gcn_bwd(ctx.adj, _row_view(dY), Y, ctx.act), None, None, None


def gcn_layer(S, adj, act=GCN_ACT_RRELU, score_vec=None):
    """Y = act(Â S) for a symmetric GcnAdj, differentiable in S; act 0 the identity, 1 F.rrelu as the reference calls it (eval mode,
    slope 11/48).  With score_vec [d] also returns scores = Y · score_vec from the same pass (no gradient: a top-k selects by it)."""
    _need_cuda(S, adj.val, score_vec)
    if act not in (GCN_ACT_NONE, GCN_ACT_RRELU):
        raise ValueError("act must be 0 (identity) or 1 (eval-mode RReLU)")
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if S.dtype != torch.float32:
        raise TypeError("fp32 features expected")
    if S.device != adj.device:
        raise ValueError("S on %s but adjacency on %s" % (S.device, adj.device))
    S = _row_view(S)
    if score_vec is not None:
        score_vec = score_vec.detach().reshape(-1).to(torch.float32).contiguous()
        if score_vec.numel() != S.shape[1]:
            raise ValueError("score_vec must have %d entries" % S.shape[1])
    return _GcnLayer.apply(S, adj, int(act), score_vec)


# ------------------------------------------------------------------------- GCN step of the GCN / GCRN baselines (ctgcn_gcn.hip)
GCN_EPI_NONE, GCN_EPI_RELU, GCN_EPI_L2NORM = 0, 1, 2


def _row_view(t):
    """t as the kernels take it: [n, d] rows with unit column stride and a row stride >= d"""
    return t if (t.stride(1) == 1 and t.stride(0) >= t.shape[1]) else t.contiguous()


def _gcn_conv_fwd(adj, S, bias, epi, p=0.0, key=0, out=None):
    """(Y, norm or None): ctgcn_gcn_conv_fwd_f32; Y is out when given"""
    lib = _lib.load()
    n, d = S.shape
    Y = torch.empty(n, d, dtype=torch.float32, device=S.device) if out is None else out
    norm = torch.empty(n, dtype=torch.float32, device=S.device) if epi == GCN_EPI_L2NORM else None
    with torch.cuda.device(S.device), _timed("gcn_conv_fwd", n=n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_gcn_conv_fwd_f32(n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(S), S.stride(0), ptr(bias), ptr(Y), Y.stride(0),
                                         epi, p, key, ptr(norm), *_gcn_long(adj, d), _stream()), "ctgcn_gcn_conv_fwd_f32")
    return Y, norm


def _gcn_conv_prep(dY, Y, norm, epi, p=0.0, want_db=False):
    """(G, db): ctgcn_gcn_conv_prep_f32.  G is dY itself for GCN_EPI_NONE; db None unless wanted."""
    lib = _lib.load()
    n, d = dY.shape
    dev = dY.device
    G = torch.empty(n, d, dtype=torch.float32, device=dev) if epi != GCN_EPI_NONE else None
    db = torch.zeros(d, dtype=torch.float32, device=dev) if want_db else None
    nbytes = int(lib.ctgcn_gcn_conv_prep_workspace_bytes(n, d)) if want_db else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev) if want_db else None
    with torch.cuda.device(dev), _timed("gcn_conv_prep", n=n, d=d):
        check(lib.ctgcn_gcn_conv_prep_f32(n, d, ptr(dY), dY.stride(0), ptr(Y), 0 if Y is None else Y.stride(0), ptr(norm), epi, p, ptr(G),
                                          0 if G is None else G.stride(0), ptr(db), ptr(ws), nbytes, _stream()), "ctgcn_gcn_conv_prep_f32")
    return (dY if G is None else G), db


class _GcnConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, bias, adj, epi, p, key):
        Y, norm = _gcn_conv_fwd(adj, S, bias, epi, p, key)
        ctx.adj, ctx.epi, ctx.p = adj, epi, p
        ctx.save_for_backward(*((Y,) if epi == GCN_EPI_RELU else (Y, norm) if epi == GCN_EPI_L2NORM else ()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        saved = ctx.saved_tensors
        Y = saved[0] if saved else None
        norm = saved[1] if len(saved) > 1 else None
        need_dS, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        G, db = _gcn_conv_prep(_row_view(dY), Y, norm, ctx.epi, ctx.p, want_db=need_db)
        dS = _gcn_conv_fwd(ctx.adj.transposed(), G, None, GCN_EPI_NONE)[0] if need_dS else None
        return dS, db, None, None, None, None


def gcn_conv(S, adj, bias=None, epi=GCN_EPI_NONE, p=0.0, key=0, out=None):
    """Y = epi(Â S + bias) for any GcnAdj (symmetric or not), differentiable in S and bias.  epi: GCN_EPI_NONE; GCN_EPI_RELU, followed
    by dropout with probability p when p > 0 (entry (i, c) kept iff the counter-based draw u01(key, i, c) >= p, kept entries scaled by
    1 / (1 - p)); GCN_EPI_L2NORM, F.normalize(p=2) over each row.  The backward is one N x d pre-pass (the gradient before the epilogue
    and the bias gradient) and the plain aggregation over adj.transposed().  out (inference only): a [n, d] view with unit column
    stride that receives Y, e.g. slot t of a [n, T, d] sequence buffer."""
    _need_cuda(S, adj.val, bias, out)
    if epi not in (GCN_EPI_NONE, GCN_EPI_RELU, GCN_EPI_L2NORM):
        raise ValueError("epi must be GCN_EPI_NONE, GCN_EPI_RELU or GCN_EPI_L2NORM")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if S.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise TypeError("fp32 features and bias expected")
    if S.device != adj.device or (bias is not None and bias.device != S.device):
        raise ValueError("S, bias and the adjacency must be on one device")
    if bias is not None and tuple(bias.shape) != (S.shape[1],):
        raise ValueError("bias must have %d entries" % S.shape[1])
    S = _row_view(S)
    key = int(key) & (2 ** 64 - 1)
    if out is None:
        return _GcnConv.apply(S, None if bias is None else bias.contiguous(), adj, int(epi), p, key)
    if torch.is_grad_enabled() and (S.requires_grad or (bias is not None and bias.requires_grad)):
        raise RuntimeError("gcn_conv(out=...) is an inference path")
    if out.dtype != torch.float32 or out.device != S.device or tuple(out.shape) != tuple(S.shape) or out.stride(1) != 1 or out.stride(0) < S.shape[1]:
        raise ValueError("out must be an fp32 [%d, %d] view with unit column stride on %s" % (S.shape[0], S.shape[1], S.device))
    return _gcn_conv_fwd(adj, S.detach(), None if bias is None else bias.detach().contiguous(), int(epi), p, key, out=out)[0]



# ------------------------------------------------------------------------- graph-attention step of the GAT baseline (ctgcn_gat.hip)
GAT_EPI_NONE, GAT_EPI_ELU, GAT_EPI_ELU_DROPOUT = 0, 1, 2


def _gat_long(adj, d, heads):
    """the long-row arguments of a gather: the pieces hold two [d] sums and a [heads] one"""
    ws, nbytes = adj.workspace(int(_lib.load().ctgcn_gat_piece_floats(d, heads)))
    return ptr(adj.long_rows), 0 if adj.long_rows is None else adj.long_rows.numel(), adj.long_threshold, ptr(ws), nbytes


def _gat_fwd(adj, S, a_src, a_dst, heads, alpha, epi, p_att=0.0, key=0, p_feat=0.0, fkey=0):
    """(out, Y, u, v, m, Z): ctgcn_gat_fwd_f32.  Y is the sum before the epilogue: out itself for GAT_EPI_NONE."""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    out = torch.empty(n, d, dtype=torch.float32, device=dev)
    Y = torch.empty(n, d, dtype=torch.float32, device=dev) if epi != GAT_EPI_NONE else None
    u, v, m, Z = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(4))
    with torch.cuda.device(dev), _timed("gat_fwd", n=n, d=d, heads=heads, nnz=adj.nnz):
        check(lib.ctgcn_gat_fwd_f32(n, d, heads, ptr(adj.row_ptr), ptr(adj.col), ptr(S), S.stride(0), ptr(a_src), ptr(a_dst), alpha, epi, p_att,
                                    key, p_feat, fkey, ptr(out), out.stride(0), ptr(Y), 0 if Y is None else Y.stride(0), ptr(u), ptr(v), ptr(m),
                                    ptr(Z), *_gat_long(adj, d, heads), _stream()), "ctgcn_gat_fwd_f32")
    return out, (out if Y is None else Y), u, v, m, Z


def _gat_bwd_prep(dY, Y, u, m, Z, heads, epi, p_feat=0.0, fkey=0):
    """(G, pack): ctgcn_gat_bwd_prep_f32.  G is dY itself for GAT_EPI_NONE; pack [n, heads, 4] = {u, m, 1 / Z, D}."""
    lib = _lib.load()
    n, d = dY.shape
    dev = dY.device
    G = torch.empty(n, d, dtype=torch.float32, device=dev) if epi != GAT_EPI_NONE else None
    pack = torch.empty(n, heads, 4, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev), _timed("gat_bwd_prep", n=n, d=d, heads=heads):
        check(lib.ctgcn_gat_bwd_prep_f32(n, d, heads, ptr(dY), dY.stride(0), ptr(Y), Y.stride(0), epi, p_feat, fkey, ptr(u), ptr(m), ptr(Z),
                                         ptr(G), 0 if G is None else G.stride(0), ptr(pack), _stream()), "ctgcn_gat_bwd_prep_f32")
    return (dY if G is None else G), pack


def _gat_bwd_row(adj, S, G, v, pack, heads, alpha, p_att=0.0, key=0):
    """du [n, heads]: ctgcn_gat_bwd_row_f32 over the CSR"""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    R = torch.empty(n, d, dtype=torch.float32, device=dev)
    csum, du = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(2))
    with torch.cuda.device(dev), _timed("gat_bwd_row", n=n, d=d, heads=heads, nnz=adj.nnz):
        check(lib.ctgcn_gat_bwd_row_f32(n, d, heads, ptr(adj.row_ptr), ptr(adj.col), ptr(S), S.stride(0), ptr(G), G.stride(0), ptr(v), ptr(pack),
                                        alpha, p_att, key, ptr(R), R.stride(0), ptr(csum), ptr(du), *_gat_long(adj, d, heads), _stream()),
              "ctgcn_gat_bwd_row_f32")
    return du


def _gat_bwd_col(adj_t, S, G, v, pack, a_src, a_dst, heads, alpha, p_att=0.0, key=0, du=None):
    """(dS or None, dv [n, heads]): ctgcn_gat_bwd_col_f32 over the transposed CSR; dS only with du"""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    dS = torch.empty(n, d, dtype=torch.float32, device=dev) if du is not None else None
    B = torch.empty(n, d, dtype=torch.float32, device=dev)
    ksum, dv = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(2))
    with torch.cuda.device(dev), _timed("gat_bwd_col", n=n, d=d, heads=heads, nnz=adj_t.nnz):
        check(lib.ctgcn_gat_bwd_col_f32(n, d, heads, ptr(adj_t.row_ptr), ptr(adj_t.col), ptr(G), G.stride(0), ptr(S), S.stride(0), ptr(v), ptr(pack),
                                        ptr(a_src), ptr(a_dst), alpha, p_att, key, ptr(du), ptr(dS), 0 if dS is None else dS.stride(0), ptr(B),
                                        B.stride(0), ptr(ksum), ptr(dv), *_gat_long(adj_t, d, heads), _stream()), "ctgcn_gat_bwd_col_f32")
    return dS, dv


def _gat_da(S, du, dv, heads):
    """(da_src, da_dst), each [heads, F] or None: ctgcn_gat_da_f32, sum_i du[i, h] S_i^h and sum_i dv[i, h] S_i^h from one read of S"""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    da_src = torch.empty(heads, d // heads, dtype=torch.float32, device=dev) if du is not None else None
    da_dst = torch.empty(heads, d // heads, dtype=torch.float32, device=dev) if dv is not None else None
    nbytes = int(lib.ctgcn_gat_da_workspace_bytes(n, d))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("gat_da", n=n, d=d, heads=heads):
        check(lib.ctgcn_gat_da_f32(n, d, heads, ptr(S), S.stride(0), ptr(du), ptr(dv), ptr(da_src), ptr(da_dst), ptr(ws), nbytes, _stream()),
              "ctgcn_gat_da_f32")
    return da_src, da_dst


class _GatConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, a_src, a_dst, adj, heads, alpha, epi, p_att, key, p_feat, fkey):
        out, Y, u, v, m, Z = _gat_fwd(adj, S, a_src, a_dst, heads, alpha, epi, p_att, key, p_feat, fkey)
        ctx.adj, ctx.cfg = adj, (heads, alpha, epi, p_att, key, p_feat, fkey)
        ctx.save_for_backward(S, a_src, a_dst, Y, u, v, m, Z)
        return out

    @staticmethod
    def backward(ctx, dY):
        S, a_src, a_dst, Y, u, v, m, Z = ctx.saved_tensors
        heads, alpha, epi, p_att, key, p_feat, fkey = ctx.cfg
        need_dS, need_src, need_dst = ctx.needs_input_grad[:3]
        dS = da_src = da_dst = None
        if need_dS or need_src or need_dst:
            G, pack = _gat_bwd_prep(_row_view(dY), Y, u, m, Z, heads, epi, p_feat, fkey)
            du = _gat_bwd_row(ctx.adj, S, G, v, pack, heads, alpha, p_att, key) if (need_dS or need_src) else None
            if need_dS or need_dst:
                dS, dv = _gat_bwd_col(ctx.adj.transposed(), S, G, v, pack, a_src, a_dst, heads, alpha, p_att, key, du if need_dS else None)
            if need_src or need_dst:
                da_src, da_dst = _gat_da(S, du if need_src else None, dv if need_dst else None, heads)
        return (dS, da_src, da_dst) + (None,) * 8


def gat_conv(S, a_src, a_dst, adj, heads, alpha=0.2, epi=GAT_EPI_NONE, p_att=0.0, key=0, p_feat=0.0, fkey=0):
    """One graph-attention layer of `heads` heads over the pattern of any GcnAdj (its values are not read; stored entries count even
    when their value is 0), differentiable in S, a_src and a_dst.  S [n, d] holds x W_h in columns [hF, (h+1)F), F = d / heads;
    a_src / a_dst [heads, F] are the two halves of the reference's a [1, 2F] per head.  For a stored entry (i, j) and head h:
        l_ij = -leakyrelu_alpha(a_src_h · S_i^h + a_dst_h · S_j^h),  e_ij = exp(l_ij - max_j l_ij),  Z_i = sum_j e_ij,
        Y_i^h = (sum_j q_ij e_ij S_j^h) / Z_i,  q_ij = [u01(key + h, i, j) >= p_att] / (1 - p_att)  (1 at p_att = 0: no draw is made)
    and the result is epi(Y): GAT_EPI_NONE; GAT_EPI_ELU; GAT_EPI_ELU_DROPOUT, ELU followed by dropout of entry (i, c) iff
    u01(fkey, i, c) < p_feat, kept entries scaled by 1 / (1 - p_feat).  The shift by the row maximum is the only departure from the
    reference's arithmetic (it exponentiates the unshifted logits and fails its NaN assertion once they leave fp32 exp's range).
    A row without stored entries gives an output row of exact zeros and no gradient; the reference would fail its NaN assertion there
    (0 / 0), and its loader's add_eye makes such rows impossible.  The backward runs over adj and adj.transposed() and computes only
    the gradients that are asked for; no mask and nothing of nnz x F elements is stored."""
    _need_cuda(S, a_src, a_dst, adj.val)
    heads = int(heads)
    if epi not in (GAT_EPI_NONE, GAT_EPI_ELU, GAT_EPI_ELU_DROPOUT):
        raise ValueError("epi must be GAT_EPI_NONE, GAT_EPI_ELU or GAT_EPI_ELU_DROPOUT")
    p_att, p_feat, alpha = float(p_att), float(p_feat), float(alpha)
    if not (0.0 <= p_att < 1.0 and 0.0 <= p_feat < 1.0):
        raise ValueError("dropout p must lie in [0, 1), got %r and %r" % (p_att, p_feat))
    if alpha != alpha or alpha in (float("inf"), float("-inf")):
        raise ValueError("alpha must be finite")
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if heads < 1 or S.shape[1] < 1 or S.shape[1] % heads:
        raise ValueError("d = %d is not a positive multiple of heads = %d" % (S.shape[1], heads))
    want = (heads, S.shape[1] // heads)
    if tuple(a_src.shape) != want or tuple(a_dst.shape) != want:
        raise ValueError("a_src and a_dst must be [%d, %d]" % want)
    if S.dtype != torch.float32 or a_src.dtype != torch.float32 or a_dst.dtype != torch.float32:
        raise TypeError("fp32 features and attention vectors expected")
    if S.device != adj.device or a_src.device != S.device or a_dst.device != S.device:
        raise ValueError("S, a_src, a_dst and the adjacency must be on one device")
    mask = 2 ** 64 - 1
    return _GatConv.apply(_row_view(S), a_src.contiguous(), a_dst.contiguous(), adj, heads, alpha, int(epi), p_att, int(key) & mask, p_feat,
                          int(fkey) & mask)


# ------------------------------------------------------------------------- pooling layers of the GIN / GraphSAGE baselines (ctgcn_pool.hip)
POOL_EPI_NONE, POOL_EPI_NORM = 0, 1


def _pool_conv_fwd(adj, S, T, self_scale, bias, epi, p=0.0, key=0, out=None):
    """(Y, norm or None, Ysave or None): ctgcn_pool_conv_fwd_f32.  adj None: no matrix, the epilogue of T alone.  Ysave: with dropout
    the normalised rows before it (what the backward reads); Y itself otherwise."""
    lib = _lib.load()
    n, d = (T if S is None else S).shape
    dev = (T if S is None else S).device
    Y = torch.empty(n, d, dtype=torch.float32, device=dev) if out is None else out
    norm = torch.empty(n, dtype=torch.float32, device=dev) if epi == POOL_EPI_NORM else None
    save = torch.empty(n, d, dtype=torch.float32, device=dev) if (epi == POOL_EPI_NORM and p > 0) else None
    matrix = (None, None, None) if adj is None else (ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val))
    long = (None, 0, 1, None, 0) if adj is None else _gcn_long(adj, d)
    with torch.cuda.device(dev), _timed("pool_conv_fwd", n=n, d=d, nnz=0 if adj is None else adj.nnz):
        check(lib.ctgcn_pool_conv_fwd_f32(n, d, *matrix, ptr(S), 0 if S is None else S.stride(0), ptr(T), 0 if T is None else T.stride(0),
                                          float(self_scale), ptr(bias), ptr(Y), Y.stride(0), epi, p, key, ptr(norm), ptr(save),
                                          0 if save is None else save.stride(0), *long, _stream()), "ctgcn_pool_conv_fwd_f32")
    return Y, norm, (Y if save is None else save)


def _pool_conv_prep(dY, Ysave, norm, p=0.0, key=0, want_db=False, out=None):
    """(G, db): ctgcn_pool_conv_prep_f32, the pre-pass of POOL_EPI_NORM.  G is written to out when given; db None unless wanted."""
    lib = _lib.load()
    n, d = dY.shape
    dev = dY.device
    G = torch.empty(n, d, dtype=torch.float32, device=dev) if out is None else out
    db = torch.zeros(d, dtype=torch.float32, device=dev) if want_db else None
    nbytes = int(lib.ctgcn_pool_prep_workspace_bytes(n, d)) if want_db else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev) if want_db else None
    with torch.cuda.device(dev), _timed("pool_conv_prep", n=n, d=d):
        check(lib.ctgcn_pool_conv_prep_f32(n, d, ptr(dY), dY.stride(0), ptr(Ysave), Ysave.stride(0), ptr(norm), p, key, ptr(G), G.stride(0),
                                           ptr(db), ptr(ws), nbytes, _stream()), "ctgcn_pool_conv_prep_f32")
    return G, db


class _PoolConv(torch.autograd.Function):
    """S, T: [n, d] or None.  pair: S is Z [n, 2 d] = [T | S], whose gradient is written as one buffer."""

    @staticmethod
    def forward(ctx, S, T, scale_t, bias, adj, scale, epi, p, key, pair):
        if pair:
            d = S.shape[1] // 2
            Y, norm, save = _pool_conv_fwd(adj, S[:, d:], S[:, :d], scale, bias, epi, p, key)
        else:
            Y, norm, save = _pool_conv_fwd(adj, S, T, scale, bias, epi, p, key)
        ctx.adj, ctx.scale, ctx.epi, ctx.p, ctx.key, ctx.pair = adj, scale, epi, p, key, pair
        ctx.has_T = T is not None
        need_T = ctx.has_T and scale_t is not None
        ctx.save_for_backward(*((save, norm) if epi == POOL_EPI_NORM else ()), *((T,) if need_T else ()))
        ctx.saved_T = need_T
        return Y

    @staticmethod
    def backward(ctx, dY):
        saved = ctx.saved_tensors
        need_S, need_T, need_scale, need_b = ctx.needs_input_grad[:4]
        dY = _row_view(dY)
        n, d = dY.shape
        dZ = torch.empty(n, 2 * d, dtype=torch.float32, device=dY.device) if ctx.pair else None
        direct = ctx.pair and ctx.scale == 1.0                       # dT = G: the pre-pass writes it in place
        if ctx.epi == POOL_EPI_NORM:
            G, db = _pool_conv_prep(dY, saved[0], saved[1], ctx.p, ctx.key, want_db=need_b, out=dZ[:, :d] if direct else None)
        else:
            G, db = _gcn_conv_prep(dY, None, None, GCN_EPI_NONE, want_db=need_b)
            if direct:
                dZ[:, :d].copy_(G)
        d_scale = (G * saved[-1]).sum() if (need_scale and ctx.saved_T) else None
        if ctx.pair:
            if not direct:
                torch.mul(G, ctx.scale, out=dZ[:, :d])
            _gcn_conv_fwd(ctx.adj.transposed(), G, None, GCN_EPI_NONE, out=dZ[:, d:])
            return dZ, None, d_scale, db, None, None, None, None, None, None
        dS = _gcn_conv_fwd(ctx.adj.transposed(), G, None, GCN_EPI_NONE)[0] if (need_S and ctx.adj is not None) else None
        dT = (G if ctx.scale == 1.0 else G * ctx.scale) if (need_T and ctx.has_T) else None
        return dS, dT, d_scale, db, None, None, None, None, None, None


def pool_conv(S, adj, T=None, self_scale=1.0, bias=None, epi=POOL_EPI_NONE, p=0.0, key=0):
    """Y = epi(Â S + self_scale T + bias) for any GcnAdj, differentiable in S, T, bias and (when it is a tensor) self_scale.  T [n, d]
    may be S itself, have its own row stride, or be another column slice of S's buffer; S = None with adj = None is the epilogue of
    self_scale T + bias alone.  epi: POOL_EPI_NONE, or POOL_EPI_NORM: ReLU, then F.normalize(p=2) over each row, then dropout with
    probability p when p > 0 (entry (i, c) kept iff u01(key, i, c) >= p, scaled by 1 / (1 - p)).  One pass is a GraphSAGE layer after
    its product, S and T the two halves of h [W_self ; W_neigh]^T.  The backward is one N x d pre-pass (the gradient before the epilogue
    and the bias gradient), dT = self_scale G and the plain aggregation dS = Â^T G over adj.transposed().
    A tensor self_scale is read back to the host (one device synchronisation per call): the kernel takes the scale by value."""
    if (S is None) != (adj is None):
        raise ValueError("S and adj go together")
    if S is None and T is None:
        raise ValueError("nothing to pool: S and T are both None")
    _need_cuda(S, T, bias, None if adj is None else adj.val)
    if epi not in (POOL_EPI_NONE, POOL_EPI_NORM):
        raise ValueError("epi must be POOL_EPI_NONE or POOL_EPI_NORM")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    first = T if S is None else S
    n = first.shape[0] if adj is None else adj.n
    for name, t in (("S", S), ("T", T)):
        if t is not None and (t.dim() != 2 or tuple(t.shape) != (n, first.shape[1])):
            raise ValueError("%s must be [%d, %d], got %s" % (name, n, first.shape[1], tuple(t.shape)))
    if any(t is not None and t.dtype != torch.float32 for t in (S, T, bias)):
        raise TypeError("fp32 features and bias expected")
    if any(t is not None and t.device != first.device for t in (S, T, bias)) or (adj is not None and adj.device != first.device):
        raise ValueError("S, T, bias and the adjacency must be on one device")
    if bias is not None and tuple(bias.shape) != (first.shape[1],):
        raise ValueError("bias must have %d entries" % first.shape[1])
    scale_t = self_scale if isinstance(self_scale, torch.Tensor) else None
    scale = float(self_scale if scale_t is None else scale_t.detach())
    key = int(key) & (2 ** 64 - 1)
    bias = None if bias is None else bias.contiguous()
    # the two halves of one [n, 2 d] buffer as [T | S]: the gradient is assembled in one buffer, with no zero-padded halves to add
    if (scale_t is None and S is not None and T is not None and S is not T and S._base is not None and S._base is T._base
            and S._base.dim() == 2 and S._base.is_contiguous() and tuple(S._base.shape) == (n, 2 * S.shape[1])
            and T.storage_offset() == S._base.storage_offset()
            and S.storage_offset() == T.storage_offset() + S.shape[1] and S.stride() == T.stride() == S._base.stride()):
        return _PoolConv.apply(S._base, None, scale_t, bias, adj, scale, int(epi), p, key, True)
    return _PoolConv.apply(None if S is None else _row_view(S), None if T is None else _row_view(T), scale_t, bias, adj, scale, int(epi), p, key,
                           False)


def _pool_max_fwd(adj, S):
    """(Y, arg int32 [n, d]): ctgcn_pool_max_fwd_f32"""
    lib = _lib.load()
    n, d = S.shape
    Y = torch.empty(n, d, dtype=torch.float32, device=S.device)
    arg = torch.empty(n, d, dtype=torch.int32, device=S.device)
    long = _gcn_long(adj, 2 * ((d + 3) // 4 * 4))                    # a partial maximum and its index per column
    with torch.cuda.device(S.device), _timed("pool_max_fwd", n=n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_pool_max_fwd_f32(n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(S), S.stride(0), ptr(Y), Y.stride(0), ptr(arg), arg.stride(0),
                                         *long, _stream()), "ctgcn_pool_max_fwd_f32")
    return Y, arg


def _pool_max_bwd(adj_t, dY, arg):
    """dS: ctgcn_pool_max_bwd_f32 over the transposed GcnAdj"""
    lib = _lib.load()
    n, d = dY.shape
    dS = torch.empty(n, d, dtype=torch.float32, device=dY.device)
    with torch.cuda.device(dY.device), _timed("pool_max_bwd", n=n, d=d, nnz=adj_t.nnz):
        check(lib.ctgcn_pool_max_bwd_f32(n, d, ptr(adj_t.row_ptr), ptr(adj_t.col), ptr(dY), dY.stride(0), ptr(arg), arg.stride(0), ptr(dS),
                                         dS.stride(0), *_gcn_long(adj_t, d), _stream()), "ctgcn_pool_max_bwd_f32")
    return dS


class _PoolMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, adj):
        Y, arg = _pool_max_fwd(adj, S)
        ctx.adj = adj
        ctx.save_for_backward(arg)
        return Y

    @staticmethod
    def backward(ctx, dY):
        return _pool_max_bwd(ctx.adj.transposed(), _row_view(dY), ctx.saved_tensors[0]), None


def pool_max(S, adj):
    """Y[i, c] = max over the stored entries j of row i of S[j, c] (the pattern alone: values are not read), zeros for an empty row;
    differentiable in S.  Among equal values the lowest column index wins, and the gradient goes there alone: the backward pulls
    dS[j, c] = sum_i [arg[i, c] == j] dY[i, c] over adj.transposed() in ascending i.  Inputs are finite."""
    _need_cuda(S, adj.val)
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if S.dtype != torch.float32:
        raise TypeError("fp32 features expected")
    if S.device != adj.device:
        raise ValueError("S on %s but adjacency on %s" % (S.device, adj.device))
    return _PoolMax.apply(_row_view(S), adj)


def _bn_stats(x, eps):
    """(mean, biased var, rstd), each [d]: ctgcn_bn_stats_f32"""
    lib = _lib.load()
    n, d = x.shape
    mean, var, rstd = (torch.empty(d, dtype=torch.float32, device=x.device) for _ in range(3))
    nbytes = int(lib.ctgcn_bn_stats_workspace_bytes(n, d))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device), _timed("bn_stats", n=n, d=d):
        check(lib.ctgcn_bn_stats_f32(n, d, ptr(x), x.stride(0), eps, ptr(mean), ptr(var), ptr(rstd), ptr(ws), nbytes, _stream()), "ctgcn_bn_stats_f32")
    return mean, var, rstd


def _bn_apply(x, mean, rstd, weight, bias, relu, p=0.0, key=0):
    lib = _lib.load()
    n, d = x.shape
    y = torch.empty(n, d, dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device), _timed("bn_apply", n=n, d=d):
        check(lib.ctgcn_bn_apply_f32(n, d, ptr(x), x.stride(0), ptr(mean), ptr(rstd), ptr(weight), ptr(bias), 1 if relu else 0, p, key, ptr(y),
                                     y.stride(0), _stream()), "ctgcn_bn_apply_f32")
    return y


def _bn_bwd(x, dy, mean, rstd, weight, bias, relu, p, key, batch_stats, need_dx=True):
    """(dx or None, dw, db): ctgcn_bn_bwd_f32"""
    lib = _lib.load()
    n, d = x.shape
    dev = x.device
    dx = torch.empty(n, d, dtype=torch.float32, device=dev) if need_dx else None
    dw, db = torch.empty(d, dtype=torch.float32, device=dev), torch.empty(d, dtype=torch.float32, device=dev)
    nbytes = int(lib.ctgcn_bn_bwd_workspace_bytes(n, d))
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("bn_bwd", n=n, d=d):
        check(lib.ctgcn_bn_bwd_f32(n, d, ptr(x), x.stride(0), ptr(dy), dy.stride(0), ptr(mean), ptr(rstd), ptr(weight), ptr(bias),
                                   1 if relu else 0, p, key, 1 if batch_stats else 0, ptr(dx), 0 if dx is None else dx.stride(0), ptr(dw), ptr(db),
                                   ptr(ws), nbytes, _stream()), "ctgcn_bn_bwd_f32")
    return dx, dw, db


class _BatchNormAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mean, var, relu, p, key, eps):
        batch_stats = mean is None
        if batch_stats:
            mean, var, rstd = _bn_stats(x, eps)
        else:
            rstd = torch.rsqrt(var.double() + eps).float()
        y = _bn_apply(x, mean, rstd, weight, bias, relu, p, key)
        ctx.relu, ctx.p, ctx.key, ctx.batch_stats = relu, p, key, batch_stats
        ctx.save_for_backward(x, mean, rstd, weight, bias)
        ctx.mark_non_differentiable(mean, var)
        return y, mean, var

    @staticmethod
    def backward(ctx, dy, *_):
        x, mean, rstd, weight, bias = ctx.saved_tensors
        dx, dw, db = _bn_bwd(x, _row_view(dy), mean, rstd, weight, bias, ctx.relu, ctx.p, ctx.key, ctx.batch_stats, ctx.needs_input_grad[0])
        return dx, dw, db, None, None, None, None, None, None


def batch_norm_act(x, weight, bias, mean=None, var=None, relu=True, p=0.0, key=0, eps=1e-5):
    """(y, mean, var) with y = dropout(relu((x - mean) / sqrt(var + eps) * weight + bias)) over the columns of x [n, d], differentiable
    in x, weight and bias.  mean / var None (training mode): the batch's own mean and biased variance, computed in fp64 and returned
    for the running buffers; a single row raises torch's ValueError.  Given (eval mode): used as constants.  relu False leaves the ReLU
    out; dropout as in gcn_conv (entry (i, c) kept iff u01(key, i, c) >= p).  The backward keeps x, mean and rstd alone: the ReLU mask
    and the draw are made again."""
    _need_cuda(x, weight, bias, mean, var)
    if x.dim() != 2 or x.shape[1] < 1:
        raise ValueError("x must be [n, d], got %s" % (tuple(x.shape),))
    d = x.shape[1]
    if (mean is None) != (var is None):
        raise ValueError("mean and var go together")
    for name, t in (("weight", weight), ("bias", bias), ("mean", mean), ("var", var)):
        if t is not None and (tuple(t.shape) != (d,) or t.dtype != torch.float32 or t.device != x.device):
            raise ValueError("%s must be an fp32 [%d] vector on %s" % (name, d, x.device))
    if x.dtype != torch.float32:
        raise TypeError("fp32 features expected")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    if mean is None and x.shape[0] == 1:
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (x.shape,))
    if x.shape[0] == 0:
        raise ValueError("batch_norm_act needs at least one row")
    mean = None if mean is None else mean.detach().contiguous()
    var = None if var is None else var.detach().contiguous()
    return _BatchNormAct.apply(_row_view(x), weight.contiguous(), bias.contiguous(), mean, var, bool(relu), p, int(key) & (2 ** 64 - 1), float(eps))


# ------------------------------------------------------------------------- PyG variants: TgGCN, TgGAT, TgSAGE, TgGIN (ctgcn_tg.hip)
TG_EPI_NONE, TG_EPI_RELU = 0, 1


class TgGraph(object):
    """The operators PyG's conv layers read off a raw edge index: edge_index int64 [2, E] on the GPU, row 0 the sources and row 1 the
    targets (adj._indices() of the loader), n nodes.  Three GcnAdj in pull form (row = target, stored columns = sources, ascending by
    source), built together on first use by the passes of ctgcn_tg.hip behind one stable sort of the keys target * n + source, and
    kept:
        looped   GCNConv's and GATConv's pattern: every non-loop pair (a repeated pair is a repeated entry) and exactly one loop per
                 node, however many the input had; value dis_s * dis_t, dis_v = c_v^-1/2 over the looped row lengths, formed in fp64
        mean     the pairs exactly as given (loops and repeats kept, nothing added), value 1 / (entries of the row)
        sum      the same row_ptr / col, value 1
    An index outside [0, n), E >= 2^31 - n or n >= 2^31 raises ValueError (one device flag, read once per build)."""
    builds = 0                              # builds made by this process (the models' cache is checked against it)

    def __init__(self, edge_index, n, long_threshold=None):
        _need_cuda(edge_index)
        if edge_index.dim() != 2 or edge_index.shape[0] != 2 or edge_index.dtype != torch.int64:
            raise ValueError("edge_index must be an int64 [2, E] tensor, got %s %s" % (edge_index.dtype, tuple(edge_index.shape)))
        self.n, self.E = int(n), int(edge_index.shape[1])
        if self.n < 0 or self.n >= 2 ** 31:
            raise ValueError("n = %d outside [0, 2^31)" % self.n)
        if self.E >= 2 ** 31 - self.n:
            raise ValueError("E = %d edges with n = %d nodes: E + n must stay below 2^31" % (self.E, self.n))
        self.edge_index, self.device, self.long_threshold = edge_index, edge_index.device, long_threshold
        self._adj = None

    def _build(self):
        lib = _lib.load()
        E, n, dev = self.E, self.n, self.device
        src, dst = self.edge_index[0].contiguous(), self.edge_index[1].contiguous()
        i32 = dict(dtype=torch.int32, device=dev)
        keys = torch.empty(E, dtype=torch.int64, device=dev)
        flag = torch.zeros(1, **i32)
        raw_ptr, loop_at, nloops = torch.empty(n + 1, **i32), torch.empty(n, **i32), torch.empty(n, **i32)
        col, mean = torch.empty(E, **i32), torch.empty(E, dtype=torch.float32, device=dev)
        col_l, val_l = torch.empty(E + n, **i32), torch.empty(E + n, dtype=torch.float32, device=dev)
        with torch.cuda.device(dev), _timed("tg_csr", n=n, nnz=E):
            check(lib.ctgcn_tg_keys(E, n, ptr(src), ptr(dst), ptr(keys), ptr(flag), _stream()), "ctgcn_tg_keys")
            keys = torch.sort(keys, stable=True).values
            check(lib.ctgcn_tg_csr_count(E, n, ptr(keys), ptr(raw_ptr), ptr(loop_at), ptr(nloops), _stream()), "ctgcn_tg_csr_count")
            looped_ptr = torch.zeros(n + 1, **i32)
            looped_ptr[1:] = (raw_ptr[1:] - raw_ptr[:-1] - nloops + 1).cumsum(0)          # E + n < 2^31: no overflow
            check(lib.ctgcn_tg_csr_emit(E, n, ptr(keys), ptr(raw_ptr), ptr(loop_at), ptr(nloops), ptr(looped_ptr), ptr(col), ptr(mean),
                                        ptr(col_l), ptr(val_l), _stream()), "ctgcn_tg_csr_emit")
        bad, nnz_l = torch.cat((flag, looped_ptr[-1:])).tolist()
        if bad:
            raise ValueError("edge_index holds a node id outside [0, %d)" % n)
        TgGraph.builds += 1
        looped = GcnAdj(looped_ptr, col_l[:nnz_l], val_l[:nnz_l], self.long_threshold)
        mean_adj = GcnAdj(raw_ptr, col, mean, self.long_threshold)
        sum_adj = GcnAdj(raw_ptr, col, torch.ones_like(mean), self.long_threshold)
        self._adj = (looped, mean_adj, sum_adj)

    def _get(self, k):
        if self._adj is None:
            self._build()
        return self._adj[k]

    looped = property(lambda self: self._get(0))
    mean = property(lambda self: self._get(1))
    sum = property(lambda self: self._get(2))


def _tg_conv_fwd(adj, S, T, self_scale, bias, epi, p=0.0, key=0):
    """Y: ctgcn_tg_conv_fwd_f32"""
    lib = _lib.load()
    n, d = S.shape
    Y = torch.empty(n, d, dtype=torch.float32, device=S.device)
    with torch.cuda.device(S.device), _timed("tg_conv_fwd", n=n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_tg_conv_fwd_f32(n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(S), S.stride(0), ptr(T), 0 if T is None else T.stride(0),
                                        float(self_scale), ptr(bias), ptr(Y), Y.stride(0), epi, p, key, *_gcn_long(adj, d), _stream()),
              "ctgcn_tg_conv_fwd_f32")
    return Y


def _tg_conv_prep(dY, Y, bias, epi, p=0.0, key=0, want_db=False, out=None):
    """(G, db): ctgcn_tg_conv_prep_f32.  G is dY itself for TG_EPI_NONE, else written to out when given; db None unless wanted."""
    n, d = dY.shape
    dev = dY.device
    if epi == TG_EPI_NONE and not want_db:
        return dY, None
    lib = _lib.load()
    G = (torch.empty(n, d, dtype=torch.float32, device=dev) if out is None else out) if epi != TG_EPI_NONE else None
    db = torch.zeros(d, dtype=torch.float32, device=dev) if want_db else None
    nbytes = int(lib.ctgcn_tg_prep_workspace_bytes(n, d)) if want_db else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev) if want_db else None
    with torch.cuda.device(dev), _timed("tg_conv_prep", n=n, d=d):
        check(lib.ctgcn_tg_conv_prep_f32(n, d, ptr(dY), dY.stride(0), ptr(Y), 0 if Y is None else Y.stride(0), ptr(bias), epi, p, key, ptr(G),
                                         0 if G is None else G.stride(0), ptr(db), ptr(ws), nbytes, _stream()), "ctgcn_tg_conv_prep_f32")
    return (dY if G is None else G), db


class _TgConv(torch.autograd.Function):
    """S, T: [n, d], T or None.  pair: S is Z [n, 2 d] = [S | T], whose gradient is written as one buffer.  same: T is S."""

    @staticmethod
    def forward(ctx, S, T, bias, adj, scale, epi, p, key, pair, same):
        if pair:
            d = S.shape[1] // 2
            Y = _tg_conv_fwd(adj, S[:, :d], S[:, d:], scale, bias, epi, p, key)
        else:
            Y = _tg_conv_fwd(adj, S, S if same else T, scale, bias, epi, p, key)
        ctx.adj, ctx.cfg = adj, (scale, epi, p, key, pair, same)
        ctx.save_for_backward(*((Y,) if epi != TG_EPI_NONE else ()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        scale, epi, p, key, pair, same = ctx.cfg
        need_S, need_T, need_b = ctx.needs_input_grad[:3]
        dY = _row_view(dY)
        n, d = dY.shape
        Y = ctx.saved_tensors[0] if epi != TG_EPI_NONE else None
        if pair and not need_S:                                         # the bias gradient alone
            return None, None, _tg_conv_prep(dY, Y, None, epi, p, key, want_db=need_b)[1], None, None, None, None, None, None, None
        adj_t = ctx.adj.transposed()
        if pair:
            dZ = torch.empty(n, 2 * d, dtype=torch.float32, device=dY.device)
            direct = scale == 1.0 and epi != TG_EPI_NONE                # dT = G: the pre-pass writes it in place
            G, db = _tg_conv_prep(dY, Y, None, epi, p, key, want_db=need_b, out=dZ[:, d:] if direct else None)
            if not direct:
                torch.mul(G, scale, out=dZ[:, d:])
            _gcn_conv_fwd(adj_t, G, None, GCN_EPI_NONE, out=dZ[:, :d])
            return dZ, None, db, None, None, None, None, None, None, None
        G, db = _tg_conv_prep(dY, Y, None, epi, p, key, want_db=need_b)
        dS = dT = None
        if same:
            if need_S:                                                 # dS = Â^T G + self_scale G, the forward's own pass over Â^T
                dS = _tg_conv_fwd(adj_t, G, G, scale, None, TG_EPI_NONE)
        else:
            if need_S:
                dS = _gcn_conv_fwd(adj_t, G, None, GCN_EPI_NONE)[0]
            if need_T:
                dT = G if scale == 1.0 else G * scale
        return dS, dT, db, None, None, None, None, None, None, None


def tg_conv(S, adj, T=None, self_scale=1.0, bias=None, epi=TG_EPI_NONE, p=0.0, key=0):
    """Y = epi(Â S + self_scale T + bias) for any GcnAdj, differentiable in S, T and bias.  T [n, d] may be None, S itself, or the
    other half of one contiguous [n, 2 d] buffer [S | T].  epi: TG_EPI_NONE, or TG_EPI_RELU: ReLU, then dropout with probability p
    when p > 0 (entry (i, c) kept iff u01(key, i, c) >= p, kept entries scaled by 1 / (1 - p): gcn_conv's draw).  One pass is PyG's
    SAGEConv after its product of width 2 d (adj = TgGraph.mean, bias = lin_l's) or its GINConv after the Linear, which commutes with
    the sum (adj = TgGraph.sum, T = S, self_scale = 1 + eps).  The backward is one N x d pre-pass (the gradient before the epilogue,
    the mask made again from key, and the bias gradient in a fixed block order), dT = self_scale G and the plain aggregation
    dS = Â^T G over adj.transposed().  No float atomics and no stored mask: repeated calls are bit-identical."""
    _need_cuda(S, T, bias, adj.val)
    if epi not in (TG_EPI_NONE, TG_EPI_RELU):
        raise ValueError("epi must be TG_EPI_NONE or TG_EPI_RELU")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if T is not None and tuple(T.shape) != tuple(S.shape):
        raise ValueError("T must be %s, got %s" % (tuple(S.shape), tuple(T.shape)))
    if any(t is not None and t.dtype != torch.float32 for t in (S, T, bias)):
        raise TypeError("fp32 features and bias expected")
    if any(t is not None and t.device != adj.device for t in (S, T, bias)):
        raise ValueError("S, T, bias and the adjacency must be on one device")
    if bias is not None and tuple(bias.shape) != (S.shape[1],):
        raise ValueError("bias must have %d entries" % S.shape[1])
    n, d = S.shape
    scale, key = float(self_scale), int(key) & (2 ** 64 - 1)
    bias = None if bias is None else bias.contiguous()
    if T is S:
        return _TgConv.apply(_row_view(S), None, bias, adj, scale, int(epi), p, key, False, True)
    # the two halves of one [n, 2 d] buffer as [S | T]: the gradient is assembled in one buffer, with no zero-padded halves to add
    if (T is not None and S._base is not None and S._base is T._base and S._base.dim() == 2 and S._base.is_contiguous()
            and tuple(S._base.shape) == (n, 2 * d) and S.storage_offset() == S._base.storage_offset()
            and T.storage_offset() == S.storage_offset() + d and S.stride() == T.stride() == S._base.stride()):
        return _TgConv.apply(S._base, None, bias, adj, scale, int(epi), p, key, True, False)
    return _TgConv.apply(_row_view(S), None if T is None else _row_view(T), bias, adj, scale, int(epi), p, key, False, False)


def _tgat_fwd(adj, S, a_tgt, a_src, heads, slope, bias, epi, p=0.0, key=0):
    """(out, Y, u, v, m, Z): ctgcn_tgat_fwd_f32.  Y is the sum before the bias and the epilogue: out itself without either."""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    out = torch.empty(n, d, dtype=torch.float32, device=dev)
    Y = torch.empty(n, d, dtype=torch.float32, device=dev) if (epi != TG_EPI_NONE or bias is not None) else None
    u, v, m, Z = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(4))
    with torch.cuda.device(dev), _timed("tgat_fwd", n=n, d=d, heads=heads, nnz=adj.nnz):
        check(lib.ctgcn_tgat_fwd_f32(n, d, heads, ptr(adj.row_ptr), ptr(adj.col), ptr(S), S.stride(0), ptr(a_tgt), ptr(a_src), slope, ptr(bias), epi,
                                     p, key, ptr(out), out.stride(0), ptr(Y), 0 if Y is None else Y.stride(0), ptr(u), ptr(v), ptr(m), ptr(Z),
                                     *_gat_long(adj, d, heads), _stream()), "ctgcn_tgat_fwd_f32")
    return out, (out if Y is None else Y), u, v, m, Z


def _tgat_bwd_row(adj, S, G, Y, v, pack, heads, slope):
    """du [n, heads]: ctgcn_tgat_bwd_row_f32 over the CSR; Y the forward's sums before the bias"""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    R = torch.empty(n, d, dtype=torch.float32, device=dev)
    csum, du = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(2))
    with torch.cuda.device(dev), _timed("tgat_bwd_row", n=n, d=d, heads=heads, nnz=adj.nnz):
        check(lib.ctgcn_tgat_bwd_row_f32(n, d, heads, ptr(adj.row_ptr), ptr(adj.col), ptr(S), S.stride(0), ptr(G), G.stride(0), ptr(Y), Y.stride(0), ptr(v),
                                         ptr(pack), slope, ptr(R), R.stride(0), ptr(csum), ptr(du), *_gat_long(adj, d, heads), _stream()),
              "ctgcn_tgat_bwd_row_f32")
    return du


def _tgat_bwd_col(adj_t, S, G, v, pack, a_tgt, a_src, heads, slope, du=None):
    """(dS or None, dv [n, heads]): ctgcn_tgat_bwd_col_f32 over the transposed CSR; dS only with du"""
    lib = _lib.load()
    n, d = S.shape
    dev = S.device
    dS = torch.empty(n, d, dtype=torch.float32, device=dev) if du is not None else None
    B = torch.empty(n, d, dtype=torch.float32, device=dev)
    ksum, dv = (torch.empty(n, heads, dtype=torch.float32, device=dev) for _ in range(2))
    with torch.cuda.device(dev), _timed("tgat_bwd_col", n=n, d=d, heads=heads, nnz=adj_t.nnz):
        check(lib.ctgcn_tgat_bwd_col_f32(n, d, heads, ptr(adj_t.row_ptr), ptr(adj_t.col), ptr(G), G.stride(0), ptr(S), S.stride(0), ptr(v), ptr(pack),
                                         ptr(a_tgt), ptr(a_src), slope, ptr(du), ptr(dS), 0 if dS is None else dS.stride(0), ptr(B), B.stride(0),
                                         ptr(ksum), ptr(dv), *_gat_long(adj_t, d, heads), _stream()), "ctgcn_tgat_bwd_col_f32")
    return dS, dv


class _TgatConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, a_tgt, a_src, bias, adj, heads, slope, epi, p, key):
        out, Y, u, v, m, Z = _tgat_fwd(adj, S, a_tgt, a_src, heads, slope, bias, epi, p, key)
        ctx.adj, ctx.cfg = adj, (heads, slope, epi, p, key)
        ctx.save_for_backward(S, a_tgt, a_src, bias, Y, u, v, m, Z)
        return out

    @staticmethod
    def backward(ctx, dY):
        S, a_tgt, a_src, bias, Y, u, v, m, Z = ctx.saved_tensors
        heads, slope, epi, p, key = ctx.cfg
        need_dS, need_tgt, need_src, need_b = ctx.needs_input_grad[:4]
        dS = da_tgt = da_src = db = None
        G, db = _tg_conv_prep(_row_view(dY), Y, bias, epi, p, key, want_db=need_b)
        if need_dS or need_tgt or need_src:
            _, pack = _gat_bwd_prep(G, Y, u, m, Z, heads, GAT_EPI_NONE)
            du = _tgat_bwd_row(ctx.adj, S, G, Y, v, pack, heads, slope) if (need_dS or need_tgt) else None
            if need_dS or need_src:
                dS, dv = _tgat_bwd_col(ctx.adj.transposed(), S, G, v, pack, a_tgt, a_src, heads, slope, du if need_dS else None)
            if need_tgt or need_src:
                da_tgt, da_src = _gat_da(S, du if need_tgt else None, dv if need_src else None, heads)
        return (dS, da_tgt, da_src, db) + (None,) * 6


def tgat_conv(S, a_tgt, a_src, adj, heads=1, slope=0.2, bias=None, epi=TG_EPI_NONE, p=0.0, key=0):
    """PyG's GATConv after its product, over the pattern of any GcnAdj (TgGraph.looped for the layer itself; the values are not read),
    differentiable in S, a_tgt, a_src and bias.  S [n, heads F]; a_tgt / a_src [heads, F] are PyG's att_r (the target's, the row's
    own features) and att_l (the source's, the gathered ones).  For a stored entry (i, j) and head h:
        z = a_tgt_h · S_i^h + a_src_h · S_j^h,  l = leakyrelu_slope(z),  e = exp(l - max_j l),  Y_i^h = (sum_j e S_j^h) / sum_j e
    and the result is epi(Y + bias), epi as in tg_conv.  There is no attention dropout (GATConv's own defaults to 0).  An empty row
    gives epi(bias) and no gradient to S.  The passes are ops.gat_conv's with the logit's sign turned (ctgcn_gat.hip); the backward
    computes only the gradients that are asked for, and nothing of nnz x F elements is stored."""
    _need_cuda(S, a_tgt, a_src, bias, adj.val)
    heads = int(heads)
    if epi not in (TG_EPI_NONE, TG_EPI_RELU):
        raise ValueError("epi must be TG_EPI_NONE or TG_EPI_RELU")
    p, slope = float(p), float(slope)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    if slope != slope or slope in (float("inf"), float("-inf")):
        raise ValueError("slope must be finite")
    if S.dim() != 2 or S.shape[0] != adj.n:
        raise ValueError("S must be [%d, d], got %s" % (adj.n, tuple(S.shape)))
    if heads < 1 or S.shape[1] < 1 or S.shape[1] % heads:
        raise ValueError("d = %d is not a positive multiple of heads = %d" % (S.shape[1], heads))
    want = (heads, S.shape[1] // heads)
    if tuple(a_tgt.shape) != want or tuple(a_src.shape) != want:
        raise ValueError("a_tgt and a_src must be [%d, %d]" % want)
    if bias is not None and tuple(bias.shape) != (S.shape[1],):
        raise ValueError("bias must have %d entries" % S.shape[1])
    if any(t is not None and t.dtype != torch.float32 for t in (S, a_tgt, a_src, bias)):
        raise TypeError("fp32 features, attention vectors and bias expected")
    if any(t is not None and t.device != adj.device for t in (S, a_tgt, a_src, bias)):
        raise ValueError("S, a_tgt, a_src, bias and the adjacency must be on one device")
    return _TgatConv.apply(_row_view(S), a_tgt.contiguous(), a_src.contiguous(), None if bias is None else bias.contiguous(), adj, heads, slope,
                           int(epi), p, int(key) & (2 ** 64 - 1))


# ------------------------------------------------------------------------- P-GNN baseline (ctgcn_pgnn.hip)
PGNN_EPI_NONE, PGNN_EPI_NORM = 0, 1
PGNN_PULL_PIECE = 512            # (n, a) items per piece of a pull list of the backward (one wave per piece)
PGNN_TABLE_PIECE = 4096          # items per piece of a table entry's list (one block per piece)
PGNN_MAX_TABLE = 4096            # distinct values of dists_max above which pgnn_conv takes the composed formulation


def _pack_anchor_sets(anchorset_list, device):
    """(offsets int32 [A + 1], members int32) on the device from a list of 1-D index arrays / tensors"""
    sets = [s if isinstance(s, torch.Tensor) else torch.as_tensor(s) for s in anchorset_list]
    if not sets:
        raise ValueError("no anchor sets")
    if any(s.dim() != 1 for s in sets):
        raise ValueError("every anchor set is a 1-D list of node ids")
    sizes = torch.tensor([0] + [int(s.numel()) for s in sets], dtype=torch.int64)
    offsets = sizes.cumsum(0).to(torch.int32).to(device)
    members = torch.cat([s.to(device=device, dtype=torch.int32) for s in sets]) if int(sizes.sum()) else torch.empty(0, dtype=torch.int32, device=device)
    return offsets, members.contiguous()


def pgnn_anchor_dist(adj_or_csr, anchorset_list, cutoff=-1, node_ids=False):
    """(level, dist_max, pos, node): ctgcn_pgnn_anchor_dist over the pattern of a GcnAdj or a (row_ptr, col) pair of device tensors, for
    a list of anchor sets (1-D arrays of node ids).  All [n, A]: level int32 (hops to the closest anchor of the set, -1 unreached),
    dist_max fp32 = 1 / (level + 1) (0 unreached), pos int32 the position inside the set of the closest anchor (the smallest among ties,
    0 unreached) and, with node_ids, node int32 = that anchor's node id (else None).  cutoff <= 0 is exact, > 0 keeps nodes within that
    many hops.  The pattern is read as given: an undirected graph is a symmetric pattern."""
    row_ptr, col = (adj_or_csr.row_ptr, adj_or_csr.col) if hasattr(adj_or_csr, "row_ptr") else adj_or_csr
    _need_cuda(row_ptr, col)
    lib = _lib.load()
    row_ptr, col = _i32(row_ptr), _i32(col)
    dev = row_ptr.device
    n, A = row_ptr.numel() - 1, len(anchorset_list)
    offsets, members = _pack_anchor_sets(anchorset_list, dev)
    level = torch.empty(n, A, dtype=torch.int32, device=dev)
    dist = torch.empty(n, A, dtype=torch.float32, device=dev)
    pos = torch.empty(n, A, dtype=torch.int32, device=dev)
    node = torch.empty(n, A, dtype=torch.int32, device=dev) if node_ids else None
    nbytes = int(lib.ctgcn_pgnn_dist_workspace_bytes())
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev), _timed("pgnn_anchor_dist", n=n, A=A, nnz=col.numel()):
        check(lib.ctgcn_pgnn_anchor_dist(n, col.numel(), ptr(row_ptr), ptr(col), A, ptr(offsets), ptr(members), members.numel(), int(cutoff),
                                         ptr(level), ptr(dist), ptr(pos), ptr(node), None, ptr(ws), nbytes, _stream()), "ctgcn_pgnn_anchor_dist")
    return level, dist, pos, node


class PgnnPrepared(object):
    """What the layer kernels read of one anchor draw: lvl int32 [n, A] indexing values fp32 [U] (the distinct entries of dists_max) and
    idx int32 [n, A]; for the backward, built on first use, the transposed index (the items n A + a sorted by idx, cut into pieces of
    at most `piece`) and the items sorted by lvl.  composed: more than PGNN_MAX_TABLE distinct values, no table."""

    def __init__(self, dists_max, dists_argmax, n, levels=None, piece=None):
        _need_cuda(dists_max, dists_argmax)
        if dists_max.dim() != 2 or tuple(dists_argmax.shape) != tuple(dists_max.shape) or dists_max.shape[0] != n or dists_max.shape[1] < 1:
            raise ValueError("dists_max and dists_argmax must be [%d, A] with A >= 1, got %s and %s" % (n, tuple(dists_max.shape), tuple(dists_argmax.shape)))
        self.n, self.A = int(n), int(dists_max.shape[1])
        if self.n * self.A >= 2 ** 31:
            raise ValueError("n A = %d reaches 2^31" % (self.n * self.A))
        self.device = dists_max.device
        self.piece = int(PGNN_PULL_PIECE if piece is None else piece)
        if self.piece < 1:
            raise ValueError("piece must be >= 1")
        if self.n and (int(dists_argmax.min()) < 0 or int(dists_argmax.max()) >= self.n):
            raise ValueError("dists_argmax outside [0, %d)" % self.n)
        self.idx = _i32(dists_argmax)
        if self.idx is dists_argmax:               # the cache watches the caller's tensor through a weak reference: hold a copy, not the tensor
            self.idx = self.idx.clone()
        self.composed = False
        if levels is not None:                                     # the distance pass's integer levels: entry u is 1 / u, entry 0 unreached
            self.lvl = (levels.to(torch.int32) + 1).contiguous()
            U = (int(self.lvl.max()) if self.n else 0) + 1
            self.values = torch.ones(U, dtype=torch.float32, device=self.device) / torch.arange(U, dtype=torch.float32, device=self.device)
            self.values[0] = 0.0
        else:
            values, inverse = torch.unique(dists_max.to(torch.float32), return_inverse=True)
            self.values = values
            self.composed = values.numel() > PGNN_MAX_TABLE
            self.lvl = None if self.composed else inverse.to(torch.int32).contiguous()
        self._pull = None
        self._table = None

    @staticmethod
    def _pieces(keys, buckets, piece):
        """keys int32 [items] in [0, buckets): (perm int32 of the items sorted by key, ascending inside a bucket; bucket of each piece;
        lo; hi; first piece of each bucket [buckets + 1]), pieces of at most `piece` items, none for an empty bucket"""
        dev = keys.device
        perm = torch.sort(keys, stable=True).indices.to(torch.int32)
        count = torch.bincount(keys, minlength=buckets)
        start = count.cumsum(0) - count
        np_ = (count + piece - 1) // piece
        first = torch.zeros(buckets + 1, dtype=torch.int64, device=dev)
        first[1:] = np_.cumsum(0)
        bucket = torch.repeat_interleave(torch.arange(buckets, device=dev), np_)
        k = torch.arange(bucket.numel(), device=dev) - first[bucket]
        lo = start[bucket] + k * piece
        hi = torch.minimum(lo + piece, start[bucket] + count[bucket])
        return perm, bucket, lo, hi, first, np_

    def pull(self):
        """(perm, pieces int32 [4, n_pieces], multi_node, multi_ptr, part_rows) of ctgcn_pgnn_conv_bwd_pull_f32"""
        if self._pull is None:
            perm, node, lo, hi, first, np_ = self._pieces(self.idx.view(-1), self.n, self.piece)
            multi = (np_ > 1).nonzero().view(-1)
            multi_ptr = torch.zeros(multi.numel() + 1, dtype=torch.int64, device=self.device)
            multi_ptr[1:] = np_[multi].cumsum(0)
            slot = torch.full((self.n,), -1, dtype=torch.int64, device=self.device)
            slot[multi] = multi_ptr[:-1]
            k = torch.arange(node.numel(), device=self.device) - first[node]
            dst = torch.where(slot[node] < 0, node, -1 - (slot[node] + k))
            pieces = torch.stack((node, lo, hi, dst)).to(torch.int32).contiguous()
            self._pull = (perm, pieces, multi.to(torch.int32), multi_ptr.to(torch.int32), int(multi_ptr[-1]))
        return self._pull

    def table_lists(self):
        """(perm, pieces int32 [2, n_pieces], piece_ptr int32 [U + 1]) of ctgcn_pgnn_table_grad_f32"""
        if self._table is None:
            perm, _, lo, hi, first, _ = self._pieces(self.lvl.view(-1), self.values.numel(), PGNN_TABLE_PIECE)
            self._table = (perm, torch.stack((lo, hi)).to(torch.int32).contiguous(), first.to(torch.int32))
        return self._table


_pgnn_cache = []                 # (weakref dists_max, weakref dists_argmax, versions, n, piece, prepared), the newest last
_PGNN_CACHE_SIZE = 64


def pgnn_prepare(dists_max, dists_argmax, n=None, levels=None, piece=None):
    """The PgnnPrepared of a (dists_max, dists_argmax) pair, built on first use and cached against the two tensors themselves (their
    identity and version counters, as the plane cache is keyed on its operands), so every layer and every epoch of one anchor draw
    shares one.  levels: the distance pass's integer levels, which spare the torch.unique over the floats."""
    import weakref
    n = dists_max.shape[0] if n is None else int(n)
    piece = int(PGNN_PULL_PIECE if piece is None else piece)
    versions = (dists_max._version, dists_argmax._version)
    live = []
    hit = None
    for entry in _pgnn_cache:
        a, b = entry[0](), entry[1]()
        if a is None or b is None:
            continue
        live.append(entry)
        if a is dists_max and b is dists_argmax and entry[2] == versions and entry[3] == n and entry[4] == piece:
            hit = entry[5]
    _pgnn_cache[:] = live[-_PGNN_CACHE_SIZE:]
    if hit is None:
        hit = PgnnPrepared(dists_max, dists_argmax, n, levels=levels, piece=piece)
        _pgnn_cache.append((weakref.ref(dists_max), weakref.ref(dists_argmax), versions, n, piece, hit))
    return hit


def _wrap64(v):
    v &= 2 ** 64 - 1
    return v - 2 ** 64 if v >= 2 ** 63 else v


def _mix64(z):
    """ctgcn_rng.h's splitmix64 finaliser on int64 tensors (two's complement wraps like uint64; shifts are made logical by masks)"""
    z = z + _wrap64(0x9e3779b97f4a7c15)
    z = (z ^ ((z >> 30) & (2 ** 34 - 1))) * _wrap64(0xbf58476d1ce4e5b9)
    z = (z ^ ((z >> 27) & (2 ** 37 - 1))) * _wrap64(0x94d049bb133111eb)
    return z ^ ((z >> 31) & (2 ** 33 - 1))


def dropout_keep_mask(key, n, d, p, device):
    """bool [n, d]: entry (i, c) is kept iff ctgcn_u01(key, i, c) >= p, the draw of every counter-based dropout epilogue, in torch
    integer ops (the composed fallback of pgnn_conv; the kernels make the draw themselves)"""
    rows = torch.arange(n, dtype=torch.int64, device=device)[:, None]
    cols = torch.arange(d, dtype=torch.int64, device=device)[None, :]
    a = _mix64(torch.full((1, 1), _wrap64(int(key)), dtype=torch.int64, device=device))
    x = _mix64(a ^ _mix64(rows * 0x100000001b3 + cols))
    u = ((x >> 11) & (2 ** 53 - 1)).to(torch.float64) * (1.0 / 9007199254740992.0)
    return u >= p


def pgnn_conv_composed(PS, dists_max, dists_argmax, w_p, b_p, need_pos=True, need_struct=True, epi=PGNN_EPI_NONE, p=0.0, key=0):
    """pgnn_conv in stock torch ops, materialising [n, A, out]: the route for a dists_max with more than PGNN_MAX_TABLE distinct
    values (no table to index), and what tools/pgnn_bench.py measures the fused pass against"""
    d = PS.shape[1] // 2
    m = torch.relu(dists_max.unsqueeze(-1) * PS[:, :d][dists_argmax.reshape(-1)].view(dists_argmax.shape[0], dists_argmax.shape[1], d)
                   + PS[:, None, d:])
    pos = strct = None
    if need_pos:
        pos = m.matmul(w_p) if b_p is None else m.matmul(w_p) + b_p
        if epi == PGNN_EPI_NORM:
            pos = torch.nn.functional.normalize(pos, p=2, dim=-1)
    if need_struct:
        strct = m.mean(dim=1)
        if p > 0:
            strct = strct * dropout_keep_mask(key, strct.shape[0], d, p, strct.device).to(strct.dtype) / (1.0 - p)
    return pos, strct


def _pgnn_common(prep, PS, table):
    n, d = PS.shape[0], PS.shape[1] // 2
    return (n, prep.A, d, ptr(PS), PS.stride(0), ptr(prep.lvl), ptr(table), table.numel())


class _PgnnConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, PS, table, w_p, b_p, prep, need_pos, need_struct, epi, p, key):
        lib = _lib.load()
        n, d, A, dev = PS.shape[0], PS.shape[1] // 2, prep.A, PS.device
        norm_on = need_pos and epi == PGNN_EPI_NORM
        pos = torch.empty(n, A, dtype=torch.float32, device=dev) if need_pos else None
        strct = torch.empty(n, d, dtype=torch.float32, device=dev) if need_struct else None
        xraw = torch.empty(n, A, dtype=torch.float32, device=dev) if norm_on else None
        with torch.cuda.device(dev), _timed("pgnn_conv_fwd", n=n, A=A, d=d):
            check(lib.ctgcn_pgnn_conv_fwd_f32(*_pgnn_common(prep, PS, table), ptr(prep.idx), ptr(w_p), ptr(b_p), ptr(pos), ptr(strct), d,
                                              1 if norm_on else 0, ptr(xraw), p if need_struct else 0.0, key, _stream()), "ctgcn_pgnn_conv_fwd_f32")
        ctx.prep, ctx.norm_on, ctx.p, ctx.key, ctx.has_b = prep, norm_on, (p if need_struct else 0.0), key, b_p is not None
        ctx.save_for_backward(PS, table, w_p, *((xraw,) if norm_on else ()))
        ctx.set_materialize_grads(False)
        return pos, strct

    @staticmethod
    def backward(ctx, g_pos, g_struct):
        if g_pos is None and g_struct is None:
            return (None,) * 10
        lib = _lib.load()
        PS, table, w_p = ctx.saved_tensors[:3]
        xraw = ctx.saved_tensors[3] if ctx.norm_on else None
        prep = ctx.prep
        n, d, A, dev = PS.shape[0], PS.shape[1] // 2, prep.A, PS.device
        g_pos = None if g_pos is None else g_pos.contiguous()
        g_struct = None if g_struct is None else _row_view(g_struct)
        gPS = torch.zeros(n, 2 * d, dtype=torch.float32, device=dev)
        gd = torch.empty(n, A, dtype=torch.float32, device=dev)
        normalize = ctx.norm_on and g_pos is not None
        gx = torch.empty(n, A, dtype=torch.float32, device=dev) if normalize else None
        gse = torch.empty(n, d, dtype=torch.float32, device=dev) if g_struct is not None else None
        g_w = torch.empty(d, dtype=torch.float32, device=dev)
        g_b = torch.empty(1, dtype=torch.float32, device=dev)
        common = _pgnn_common(prep, PS, table)
        with torch.cuda.device(dev):
            nbytes = int(lib.ctgcn_pgnn_bwd_row_workspace_bytes(n, d))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
            with _timed("pgnn_conv_bwd_row", n=n, A=A, d=d):
                check(lib.ctgcn_pgnn_conv_bwd_row_f32(*common, ptr(prep.idx), ptr(w_p), ptr(g_pos), ptr(xraw), 1 if normalize else 0,
                                                      ptr(g_struct), 0 if g_struct is None else g_struct.stride(0), ctx.p, ctx.key, ptr(gPS), 2 * d,
                                                      ptr(gd), ptr(gx), ptr(gse), d, ptr(g_w), ptr(g_b), ptr(ws), nbytes, _stream()),
                      "ctgcn_pgnn_conv_bwd_row_f32")
            del ws
            if ctx.needs_input_grad[0]:
                perm, pieces, multi_node, multi_ptr, part_rows = prep.pull()
                nbytes = int(lib.ctgcn_pgnn_bwd_pull_workspace_bytes(part_rows, d))
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
                with _timed("pgnn_conv_bwd_pull", n=n, A=A, d=d):
                    check(lib.ctgcn_pgnn_conv_bwd_pull_f32(*common, ptr(w_p), ptr(gx if normalize else g_pos), ptr(gse), d, ptr(perm), ptr(pieces),
                                                           pieces.shape[1], ptr(multi_node), ptr(multi_ptr), multi_node.numel(), part_rows,
                                                           ptr(gPS), 2 * d, ptr(ws), nbytes, _stream()), "ctgcn_pgnn_conv_bwd_pull_f32")
                del ws
            g_table = None
            if ctx.needs_input_grad[1]:
                perm, pieces, piece_ptr = prep.table_lists()
                g_table = torch.empty(table.numel(), dtype=torch.float32, device=dev)
                nbytes = int(lib.ctgcn_pgnn_table_grad_workspace_bytes(pieces.shape[1]))
                ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)
                with _timed("pgnn_table_grad", n=n, A=A):
                    check(lib.ctgcn_pgnn_table_grad_f32(n * A, table.numel(), ptr(gd), ptr(perm), ptr(pieces), pieces.shape[1], ptr(piece_ptr),
                                                        ptr(g_table), ptr(ws), nbytes, _stream()), "ctgcn_pgnn_table_grad_f32")
        have_pos = g_pos is not None
        return (gPS if ctx.needs_input_grad[0] else None, g_table, g_w if (have_pos and ctx.needs_input_grad[2]) else None,
                g_b if (have_pos and ctx.has_b and ctx.needs_input_grad[3]) else None, None, None, None, None, None, None)


def pgnn_conv(PS, dists_max, dists_argmax, w_p, b_p=None, table=None, need_pos=True, need_struct=True, epi=PGNN_EPI_NONE, p=0.0, key=0,
              piece=None):
    """(pos [n, A] or None, struct [n, out] or None) of one P-GNN layer after its product PS [n, 2 out] = P | S:
    m = relu(d'[i, a] P[dists_argmax[i, a]] + S[i]), pos = <m, w_p> + b_p, struct = mean_a m, with m formed in registers: nothing of
    n x A x out exists, in the forward or the backward.  d' = table[k] where dists_max[i, a] == pgnn_prepare(dists_max, dists_argmax).values[k]:
    build a table from that tensor, entry for entry, and from nothing else.  Its order is whatever the prepared index has: ascending
    for a pair that went through torch.unique, but 0, 1, 1/2, 1/3, ... (entry 0 present even when nothing is unreached) for a pair that
    baseline.pgnn.get_dist_max made from a DistHandle.  So a trainable distance transform runs under autograd on those few values and
    the kernel indexes its result; table None: d' = dists_max.  epi PGNN_EPI_NORM: F.normalize(pos, p=2, dim=-1).  p > 0: dropout on struct,
    entry (i, c) kept iff u01(key, i, c) >= p.  Differentiable in PS, table, w_p and b_p; an output that was not asked for costs nothing
    and sends no gradient (w_p and b_p get None without pos).  The prepared index is cached against the two dists tensors
    (pgnn_prepare).  More than PGNN_MAX_TABLE distinct values in dists_max: the composed torch formulation (table must then be None)."""
    _need_cuda(PS, dists_max, dists_argmax, w_p, b_p, table)
    if not (need_pos or need_struct):
        raise ValueError("neither pos nor struct asked for")
    if epi not in (PGNN_EPI_NONE, PGNN_EPI_NORM):
        raise ValueError("epi must be PGNN_EPI_NONE or PGNN_EPI_NORM")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout p must lie in [0, 1), got %r" % p)
    if PS.dim() != 2 or PS.shape[1] < 2 or PS.shape[1] % 2:
        raise ValueError("PS must be [n, 2 out], got %s" % (tuple(PS.shape),))
    n, d = PS.shape[0], PS.shape[1] // 2
    if not 1 <= d <= 512:
        raise ValueError("out = %d outside [1, 512]" % d)
    w_p = w_p.reshape(-1)
    if w_p.numel() != d or (b_p is not None and b_p.numel() != 1):
        raise ValueError("w_p must have %d entries and b_p one" % d)
    if any(t is not None and t.dtype != torch.float32 for t in (PS, w_p, b_p, table)):
        raise TypeError("fp32 features and weights expected")
    if any(t is not None and t.device != PS.device for t in (dists_max, dists_argmax, w_p, b_p, table)):
        raise ValueError("every operand must be on one device")
    key = int(key) & (2 ** 64 - 1)
    prep = pgnn_prepare(dists_max, dists_argmax, n, piece=piece)
    if prep.composed:
        if table is not None:
            raise ValueError("dists_max has %d distinct values, above PGNN_MAX_TABLE = %d: no table" % (prep.values.numel(), PGNN_MAX_TABLE))
        return pgnn_conv_composed(PS, dists_max.to(torch.float32), dists_argmax.to(torch.int64), w_p, b_p, need_pos, need_struct, epi, p, key)
    if table is None:
        table = prep.values
    table = table.reshape(-1)
    if table.numel() != prep.values.numel():
        raise ValueError("table must have %d entries (the distinct values of dists_max)" % prep.values.numel())
    if n == 0:
        return (PS.new_zeros(0, prep.A) if need_pos else None), (PS.new_zeros(0, d) if need_struct else None)
    return _PgnnConv.apply(_row_view(PS), table.contiguous(), w_p.contiguous(), None if b_p is None else b_p.reshape(-1).contiguous(), prep,
                           bool(need_pos), bool(need_struct), int(epi), p, key)


# ------------------------------------------------------------------------- decoder loss of the VGRNN baseline (ctgcn_vgrnn.hip)
VAE_NLL_TILE = 32                       # rows and columns of a tile of the dense pass (ctgcn_vae_nll_tile())


class _Coefficients(object):
    """The CSR of a GcnAdj with other values: what _gcn_conv_fwd reads of an adjacency"""

    def __init__(self, adj, val):
        self.row_ptr, self.col, self.val, self.nnz = adj.row_ptr, adj.col, val, adj.nnz
        self.long_rows, self.long_threshold, self.workspace = adj.long_rows, adj.long_threshold, adj.workspace


def adjacency_sum(adj):
    """S = the sum of the stored values of a GcnAdj in fp64, once per adjacency (one device-to-host read)"""
    s = getattr(adj, "_value_sum", None)
    if s is None:
        s = adj._value_sum = float(adj.val.double().sum())
    return s


def _vae_nll_raw(z, adj, posw_m1, want_grad):
    """(Σ_ij softplus(x_ij) + Σ_stored a_e ((posw − 1) softplus(−x_e) − x_e) as a fp64 [1] tensor, its gradient by z or None)"""
    lib = _lib.load()
    n, d = z.shape
    dev = z.device
    loss = torch.zeros(2, dtype=torch.float64, device=dev)          # an adjacency without stored entries writes no second term
    dz = torch.empty(n, d, dtype=torch.float32, device=dev) if want_grad else None
    with torch.cuda.device(dev), _timed("vae_nll", n=n, d=d, nnz=adj.nnz):
        nbytes = int(lib.ctgcn_vae_nll_workspace_bytes(n, adj.nnz))
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dev)
        check(lib.ctgcn_vae_nll_dense_f32(n, d, ptr(z), z.stride(0), ptr(dz), d, ptr(loss), ptr(ws), nbytes, _stream()),
              "ctgcn_vae_nll_dense_f32")
        for k, a in enumerate((adj, adj.transposed()) if want_grad else (adj,)):
            coef = torch.empty(a.nnz, dtype=torch.float32, device=dev)
            check(lib.ctgcn_vae_nll_entries_f32(n, a.nnz, d, ptr(a.row_ptr), ptr(a.col), ptr(a.val), ptr(z), z.stride(0), posw_m1, ptr(coef),
                                                None if k else loss[1:].data_ptr(), ptr(ws), nbytes, _stream()), "ctgcn_vae_nll_entries_f32")
            if want_grad and a.nnz:
                dz += _gcn_conv_fwd(_Coefficients(a, coef), z, None, GCN_EPI_NONE)[0]
    return loss.sum(0, keepdim=True), dz


class _VaeNll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, adj, n2_minus_s, posw_m1):
        want_grad = ctx.needs_input_grad[0]
        total, dz = _vae_nll_raw(z, adj, posw_m1, want_grad)
        scale = 1.0 / (2.0 * n2_minus_s)
        if want_grad:
            ctx.save_for_backward(dz.mul_(scale))
        return (total * scale).to(torch.float32).reshape(())

    @staticmethod
    def backward(ctx, g):
        return ctx.saved_tensors[0] * g, None, None, None


def vae_nll(z, adj):
    """The reference's VAELoss.__nll_bernoulli(z zᵀ, adj.to_dense()) (metrics.py:154-161) as a fp32 scalar, differentiable in z, with
    no [n, n] matrix: one tiled pass over z zᵀ on the fp32 matrix cores gives Σ softplus(x_ij) and its gradient, the stored entries of
    adj (a GcnAdj of the target adjacency as given: its weights count, its pattern need not be symmetric) give the rest.  Sums are kept
    in fp64 and added in a fixed order.  An adjacency whose values sum to 0 (the reference divides by zero) or to n² raises ValueError."""
    _need_cuda(z, adj.val)
    if z.dim() != 2 or z.shape[0] != adj.n:
        raise ValueError("z must be [%d, d], got %s" % (adj.n, tuple(z.shape)))
    if z.dtype != torch.float32:
        raise TypeError("fp32 embeddings expected")
    if z.device != adj.device:
        raise ValueError("z on %s but adjacency on %s" % (z.device, adj.device))
    if z.shape[1] < 1:
        raise ValueError("z needs at least one column")
    s = adjacency_sum(adj)
    n2 = float(adj.n) * float(adj.n)
    if s == 0.0:
        raise ValueError("the adjacency's values sum to 0: pos_weight = (n² − S) / S is undefined")
    if n2 - s == 0.0:
        raise ValueError("the adjacency's values sum to n²: the loss's norm n² / (2 (n² − S)) is undefined")
    return _VaeNll.apply(_row_view(z), adj, n2 - s, (n2 - s) / s - 1.0)


# ------------------------------------------------------------------------- fused gathers of the VGRNN baseline (ctgcn_vgrnn.hip)
def _transposed_gather(adj, G):
    """Âᵀ G: the plain aggregation over the transposed CSR, as gcn_conv's backward does"""
    return _gcn_conv_fwd(adj.transposed(), G, None, GCN_EPI_NONE)[0]


VGRNN_PREP_GATES, VGRNN_PREP_BLEND, VGRNN_PREP_HEADS = 0, 1, 2


def _vgrnn_prep(mode, grads, saved, extras, want_db):
    """(G, extra results, db): ctgcn_vgrnn_bwd_prep_f32, the one N x d pass of a fused gather's backward.  grads: up to three incoming
    gradients (None counts as zero), saved: the forward's saved [n, w] tensors, extras: how many [n, w] results besides G"""
    lib = _lib.load()
    n, w = saved[0].shape
    segs = (3, 1, 2)[mode]
    dev = saved[0].device
    grads = [None if g is None else _row_view(g) for g in grads] + [None] * (3 - len(grads))
    saved = list(saved) + [None] * (3 - len(saved))
    G = torch.empty(n, segs * w, dtype=torch.float32, device=dev)
    out = [torch.empty(n, w, dtype=torch.float32, device=dev) for _ in range(extras)] + [None] * (2 - extras)
    db = torch.zeros(segs * w, dtype=torch.float32, device=dev) if want_db else None
    nbytes = int(lib.ctgcn_gcn_conv_prep_workspace_bytes(n, segs * w)) if want_db else 0
    ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev) if want_db else None
    flat = []
    for t in grads + saved:
        flat += [ptr(t), 0 if t is None else t.stride(0)]
    with torch.cuda.device(dev), _timed("vgrnn_bwd_prep", n=n, d=segs * w):
        check(lib.ctgcn_vgrnn_bwd_prep_f32(mode, n, w, *flat, ptr(G), G.stride(0), ptr(out[0]), ptr(out[1]), ptr(db), ptr(ws), nbytes, _stream()),
              "ctgcn_vgrnn_bwd_prep_f32")
    return G, out[:extras], db


class _GgruGates(torch.autograd.Function):
    @staticmethod
    def forward(ctx, U, h, bias, adj):
        lib = _lib.load()
        n, H = h.shape
        z, r, q, c = (torch.empty(n, H, dtype=torch.float32, device=U.device) for _ in range(4))
        with torch.cuda.device(U.device), _timed("ggru_gates_fwd", n=n, d=3 * H, nnz=adj.nnz):
            check(lib.ctgcn_ggru_gates_fwd_f32(n, H, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(U), U.stride(0), ptr(bias), ptr(h),
                                               h.stride(0), ptr(z), ptr(r), ptr(q), ptr(c), *_gcn_long(adj, 3 * H), _stream()),
                  "ctgcn_ggru_gates_fwd_f32")
        ctx.adj = adj
        ctx.save_for_backward(z, r, h)
        return z, q, c

    @staticmethod
    def backward(ctx, dz, dq, dc):
        G, (dh,), db = _vgrnn_prep(VGRNN_PREP_GATES, (dz, dq, dc), ctx.saved_tensors, 1, ctx.needs_input_grad[2])
        dU = _transposed_gather(ctx.adj, G) if ctx.needs_input_grad[0] else None
        return dU, dh, db, None


class _GgruBlend(torch.autograd.Function):
    @staticmethod
    def forward(ctx, V, c, z, h, adj):
        lib = _lib.load()
        n, H = h.shape
        h_new, h_tilde = (torch.empty(n, H, dtype=torch.float32, device=V.device) for _ in range(2))
        with torch.cuda.device(V.device), _timed("ggru_blend_fwd", n=n, d=H, nnz=adj.nnz):
            check(lib.ctgcn_ggru_blend_fwd_f32(n, H, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(V), V.stride(0), ptr(c), c.stride(0),
                                               ptr(z), z.stride(0), ptr(h), h.stride(0), ptr(h_new), ptr(h_tilde), *_gcn_long(adj, H),
                                               _stream()), "ctgcn_ggru_blend_fwd_f32")
        ctx.adj = adj
        ctx.save_for_backward(z, h, h_tilde)
        return h_new

    @staticmethod
    def backward(ctx, dh_new):
        G, (dz, dh), _ = _vgrnn_prep(VGRNN_PREP_BLEND, (dh_new,), ctx.saved_tensors, 2, False)     # G: in front of the gather, and dc
        dV = _transposed_gather(ctx.adj, G) if ctx.needs_input_grad[0] else None
        return dV, G, dz, dh, None


class _VgrnnHeads(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, bias, noise, adj):
        lib = _lib.load()
        n, out = noise.shape
        mean, std, z = (torch.empty(n, out, dtype=torch.float32, device=S.device) for _ in range(3))
        with torch.cuda.device(S.device), _timed("vgrnn_heads_fwd", n=n, d=2 * out, nnz=adj.nnz):
            check(lib.ctgcn_vgrnn_heads_fwd_f32(n, out, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(S), S.stride(0), ptr(bias), ptr(noise),
                                                noise.stride(0), ptr(mean), ptr(std), ptr(z), *_gcn_long(adj, 2 * out), _stream()),
                  "ctgcn_vgrnn_heads_fwd_f32")
        ctx.adj = adj
        ctx.save_for_backward(std, noise)
        return mean, std, z

    @staticmethod
    def backward(ctx, dmean, dstd, dz):
        # softplus' = σ(pre) = 1 − exp(−std); above the threshold std = pre and the factor rounds to 1
        G, _, db = _vgrnn_prep(VGRNN_PREP_HEADS, (dmean, dstd, dz), ctx.saved_tensors, 0, ctx.needs_input_grad[1])
        return (_transposed_gather(ctx.adj, G) if ctx.needs_input_grad[0] else None), db, None, None


def _check_rows(adj, width, **tensors):
    """fp32 [adj.n, width] CUDA operands on the adjacency's device, as row views; None passes"""
    out = []
    for name, (t, w) in tensors.items():
        if t is None:
            out.append(None)
            continue
        if t.dim() != 2 or tuple(t.shape) != (adj.n, w):
            raise ValueError("%s must be [%d, %d], got %s" % (name, adj.n, w, tuple(t.shape)))
        if t.dtype != torch.float32:
            raise TypeError("fp32 %s expected" % name)
        if t.device != adj.device:
            raise ValueError("%s on %s but adjacency on %s" % (name, t.device, adj.device))
        out.append(_row_view(t))
    return out


def _check_bias(bias, width, device):
    if bias is None:
        return None
    if bias.dtype != torch.float32 or tuple(bias.shape) != (width,) or bias.device != device:
        raise ValueError("bias must be fp32 [%d] on %s" % (width, device))
    return bias.contiguous()


def ggru_gates(U, h, adj, bias=None):
    """(z, q, c) of a graph-GRU step's first pass (reference baseline/vgrnn.py:384-386) from one gather of width 3 H:
    [g_z | g_r | g_c] = Â U + bias, z = σ(g_z), q = σ(g_r) ∘ h, c = g_c, with U = x [W_xz | W_xr | W_xh] + h [W_hz | W_hr | 0] and the
    summed biases.  Differentiable in U, h and bias: one N x 3H pre-pass on the saved z, r and h (the gradient in front of the gather, dh,
    the bias gradient by per-block column sums), then the plain aggregation over adj.transposed()."""
    _need_cuda(U, h, adj.val, bias)
    if h.dim() != 2:
        raise ValueError("h must be [n, H]")
    H = h.shape[1]
    U, h = _check_rows(adj, H, U=(U, 3 * H), h=(h, H))
    return _GgruGates.apply(U, h, _check_bias(bias, 3 * H, adj.device), adj)


def ggru_blend(V, c, z, h, adj):
    """h' = z ∘ h + (1 − z) ∘ tanh(c + Â V) (reference baseline/vgrnn.py:386-387) from one gather of width H, V = q W_hh.
    Differentiable in V, c, z and h."""
    _need_cuda(V, c, z, h, adj.val)
    if h.dim() != 2:
        raise ValueError("h must be [n, H]")
    H = h.shape[1]
    V, c, z, h = _check_rows(adj, H, V=(V, H), c=(c, H), z=(z, H), h=(h, H))
    return _GgruBlend.apply(V, c, z, h, adj)


def vgrnn_heads(S, adj, bias, noise):
    """(mean, std, z) of the VGRNN encoder's twin heads (reference baseline/vgrnn.py:498-507) from one gather of width 2 out:
    [g_m | g_s] = Â S + bias, mean = g_m, std = F.softplus(g_s), z = mean + noise ∘ std, with S = enc [W_mean | W_std].
    Differentiable in S and bias; noise is an operand (torch.randn from torch's generator, so torch.manual_seed reproduces a run)."""
    _need_cuda(S, adj.val, bias, noise)
    if noise.dim() != 2:
        raise ValueError("noise must be [n, out]")
    out = noise.shape[1]
    S, noise = _check_rows(adj, out, S=(S, 2 * out), noise=(noise.detach(), out))
    return _VgrnnHeads.apply(S, _check_bias(bias, 2 * out, adj.device), noise, adj)


# ------------------------------------------------------------------------- row-selected passes of the DynGEM / DynAE baselines (ctgcn_dyngem.hip)
class SnapshotRows(object):
    """The T snapshots of a window as one stacked CSR on the device: row t N + v is row v of snapshot t, columns are node ids, int32
    indices and fp32 values, canonical (columns sorted, duplicates summed).  A stored zero stays stored and counts as absent wherever the
    reference tests x != 0.  Also: row_sum, the weight sum of every row in fp64 rounded once (DynGEM's divisor); transposed(), the
    stack's transpose as a GcnAdj of N rows with columns in [0, T N), built once by a stable sort; and a host copy of the CSR, whose
    row lengths size every batch's long-position list and staging area without a device read-back.  Built from scipy matrices, as
    DataLoader.get_date_adj_list(..., data_type='matrix') returns them."""
    LONG_POSITION = 2048

    def __init__(self, mats, device, long_threshold=None):
        import numpy as np
        import scipy.sparse as sp
        mats = [sp.csr_matrix(m) for m in (mats if isinstance(mats, (list, tuple)) else [mats])]
        if not mats:
            raise ValueError("at least one snapshot expected")
        n = mats[0].shape[0]
        for m in mats:
            if m.shape != (n, n):
                raise ValueError("every snapshot must be [%d, %d], got %s" % (n, n, m.shape))
        device = torch.device(device)
        if device.type != 'cuda':
            raise _lib.CtgcnHipError("ctgcn_amd runs on MI355X only: SnapshotRows on %s. There is no CPU fallback." % device)
        csr = sp.vstack(mats, format='csr')
        csr.sum_duplicates()
        csr.sort_indices()
        if csr.nnz >= 2 ** 31 or csr.shape[0] >= 2 ** 31:
            raise ValueError("more than 2^31-1 rows or stored entries")
        self.T, self.n, self.rows, self.nnz = len(mats), n, len(mats) * n, int(csr.nnz)
        self.device = device
        self.long_threshold = int(self.LONG_POSITION if long_threshold is None else long_threshold)
        if self.long_threshold < 1:
            raise ValueError("long_threshold must be >= 1")
        self.host_ptr = csr.indptr.astype(np.int64)
        self.host_col = csr.indices.astype(np.int32)
        self.host_val = csr.data.astype(np.float32)
        self.host_len = np.diff(self.host_ptr)
        row_of = np.repeat(np.arange(self.rows), self.host_len)
        sums = np.bincount(row_of, weights=self.host_val.astype(np.float64), minlength=self.rows)
        self.row_ptr = torch.from_numpy(self.host_ptr.astype(np.int32)).to(device)
        self.col = torch.from_numpy(self.host_col).to(device)
        self.val = torch.from_numpy(self.host_val).to(device)
        self.row_sum = torch.from_numpy(sums.astype(np.float32)).to(device)
        self._transposed = None
        self._ws = {}

    @classmethod
    def from_scipy(cls, mats, device, long_threshold=None):
        return cls(mats, device, long_threshold)

    def transposed(self):
        """the stack's transpose: a GcnAdj of N rows whose columns are stacked row ids, rows ascending within a column"""
        if self._transposed is None:
            counts = (self.row_ptr[1:] - self.row_ptr[:-1]).to(torch.int64)
            row = torch.repeat_interleave(torch.arange(self.rows, device=self.device), counts)
            col = self.col.to(torch.int64)
            order = torch.argsort(col, stable=True)
            row_ptr = torch.zeros(self.n + 1, dtype=torch.int64, device=self.device)
            row_ptr[1:] = torch.bincount(col, minlength=self.n).cumsum(0)
            self._transposed = GcnAdj(row_ptr.to(torch.int32), row[order].to(torch.int32), self.val[order], self.long_threshold)
        return self._transposed

    def select(self, idx):
        return idx if isinstance(idx, RowSelection) else RowSelection(self, idx)

    def snapshot(self, t):
        """snapshot t as a scipy CSR (host copy)"""
        import scipy.sparse as sp
        lo, hi = self.host_ptr[t * self.n], self.host_ptr[(t + 1) * self.n]
        return sp.csr_matrix((self.host_val[lo:hi], self.host_col[lo:hi], self.host_ptr[t * self.n:(t + 1) * self.n + 1] - lo), shape=(self.n, self.n))

    def dense(self, idx):
        """the selected rows as a dense [B, L, N] fp32 tensor (-1: a zero row), made on the device with stock torch ops: the composed
        path's input"""
        sel = self.select(idx)
        ix = sel.idx.to(torch.int64)
        B, L = ix.shape
        safe = ix.clamp(min=0).reshape(-1)
        start = self.row_ptr.to(torch.int64)[safe]
        cnt = torch.where(ix.reshape(-1) >= 0, self.row_ptr.to(torch.int64)[safe + 1] - start, torch.zeros_like(start))
        slot = torch.repeat_interleave(torch.arange(B * L, device=self.device), cnt)
        first = torch.cumsum(cnt, 0) - cnt
        e = start[slot] + (torch.arange(slot.numel(), device=self.device) - first[slot])
        out = torch.zeros(B * L, self.n, dtype=torch.float32, device=self.device)
        out[slot, self.col.to(torch.int64)[e]] = self.val[e]
        return out.view(B, L, self.n)

    def workspace(self, key, nbytes):
        ws = self._ws.get(key)
        if ws is None or ws.numel() < nbytes:
            ws = self._ws[key] = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=self.device)
        return ws


class RowSelection(object):
    """A batch of stacked row ids of a SnapshotRows: idx [B] or [B, L] as host integers (-1: an empty row), uploaded once as int32.
    From the host copy of the row lengths: the positions with more than long_threshold entries and the pieces their longest is cut into
    (the contract of ctgcn_gather.h), and ent_ptr, the running sums of the lengths.  inverted(s): per stacked row the batch positions
    whose slot s selected it, ascending, from a stable sort on the device."""

    def __init__(self, rows, idx):
        import numpy as np
        if isinstance(idx, torch.Tensor):
            idx = idx.detach().cpu().numpy()
        idx = np.asarray(idx)
        if idx.dtype.kind not in 'iu':
            raise TypeError("integer row ids expected")
        idx = idx.astype(np.int64)
        if idx.ndim == 1:
            idx = idx[:, None]
        if idx.ndim != 2 or idx.shape[1] < 1:
            raise ValueError("idx must be [B] or [B, L]")
        if idx.size and (idx.min() < -1 or idx.max() >= rows.rows):
            raise ValueError("row id outside [-1, %d)" % rows.rows)
        self.rows, self.host_idx = rows, idx
        self.B, self.L = idx.shape
        lens = np.where(idx >= 0, rows.host_len[np.maximum(idx, 0)], 0)
        self.host_len = lens.sum(1)
        self.idx = torch.from_numpy(idx.astype(np.int32)).to(rows.device)
        self.long_pos, self.pieces = None, 1
        top = int(self.host_len.max()) if self.B else 0
        if top > rows.long_threshold:
            self.long_pos = torch.from_numpy(np.nonzero(self.host_len > rows.long_threshold)[0].astype(np.int32)).to(rows.device)
            piece = GCN_PIECE_FACTOR * rows.long_threshold
            self.pieces = (top + piece - 1) // piece
        self._inv, self._ent = {}, None

    def inverted(self, s):
        hit = self._inv.get(s)
        if hit is None:
            col = self.idx[:, s].to(torch.int64)
            vals, order = torch.sort(torch.where(col >= 0, col, torch.full_like(col, self.rows.rows)), stable=True)
            inv_ptr = torch.searchsorted(vals, torch.arange(self.rows.rows + 1, device=col.device))
            hit = self._inv[s] = (inv_ptr.to(torch.int32), order.to(torch.int32))
        return hit

    def ent_ptr(self):
        """(int64 [B + 1] on the device, total) of a selection with one row per position"""
        import numpy as np
        if self._ent is None:
            run = np.zeros(self.B + 1, dtype=np.int64)
            np.cumsum(self.host_len, out=run[1:])
            self._ent = (torch.from_numpy(run).to(self.rows.device), int(run[-1]))
        return self._ent


def _rowsel_fwd(S, rows, sel, bias, relu, col_stride):
    lib = _lib.load()
    d = S.shape[1]
    Y = torch.empty(sel.B, d, dtype=torch.float32, device=S.device)
    n_long = 0 if sel.long_pos is None else sel.long_pos.numel()
    nbytes = n_long * sel.pieces * ((d + 3) // 4 * 4) * 4
    ws = rows.workspace(("rowsel", d), nbytes) if n_long else None
    with torch.cuda.device(S.device), _timed("rowsel_conv_fwd", n=sel.B, d=d, nnz=int(sel.host_len.sum())):
        check(lib.ctgcn_rowsel_conv_fwd_f32(sel.B, sel.L, d, ptr(sel.idx), ptr(rows.row_ptr), ptr(rows.col), ptr(rows.val), ptr(S), S.stride(0),
                                            col_stride, ptr(bias), 1 if relu else 0, ptr(Y), Y.stride(0), ptr(sel.long_pos), n_long,
                                            rows.long_threshold, ptr(ws), nbytes, _stream()), "ctgcn_rowsel_conv_fwd_f32")
    return Y


def _rowsel_bucket(sel, s, G):
    lib = _lib.load()
    d = G.shape[1]
    inv_ptr, inv_pos = sel.inverted(s)
    out = torch.empty(sel.rows.rows, d, dtype=torch.float32, device=G.device)
    with torch.cuda.device(G.device), _timed("rowsel_bucket", n=sel.rows.rows, d=d):
        check(lib.ctgcn_rowsel_bucket_f32(sel.rows.rows, d, ptr(inv_ptr), ptr(inv_pos), ptr(G), G.stride(0), ptr(out), out.stride(0), _stream()),
              "ctgcn_rowsel_bucket_f32")
    return out


def _stack_gather_t(rows, src, out):
    """out [N, d] = Mᵀ src for the stacked matrix M [T N, N] and src [T N, d]: the plain aggregation over rows.transposed()"""
    lib = _lib.load()
    adj = rows.transposed()
    d = src.shape[1]
    with torch.cuda.device(src.device), _timed("gcn_conv_fwd", n=adj.n, d=d, nnz=adj.nnz):
        check(lib.ctgcn_gcn_conv_fwd_f32(adj.n, d, ptr(adj.row_ptr), ptr(adj.col), ptr(adj.val), ptr(src), src.stride(0), None, ptr(out),
                                         out.stride(0), GCN_EPI_NONE, 0.0, 0, None, *_gcn_long(adj, d), _stream()), "ctgcn_gcn_conv_fwd_f32")
    return out


class _RowselConv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, S, bias, rows, sel, relu, col_stride):
        Y = _rowsel_fwd(S, rows, sel, bias, relu, col_stride)
        ctx.rows, ctx.sel, ctx.relu, ctx.col_stride, ctx.s_shape = rows, sel, relu, col_stride, tuple(S.shape)
        ctx.save_for_backward(*((Y,) if relu else ()))
        return Y

    @staticmethod
    def backward(ctx, dY):
        Y = ctx.saved_tensors[0] if ctx.relu else None
        rows, sel = ctx.rows, ctx.sel
        G, db = _gcn_conv_prep(_row_view(dY), Y, None, GCN_EPI_RELU if ctx.relu else GCN_EPI_NONE, want_db=ctx.needs_input_grad[1])
        dS = None
        if ctx.needs_input_grad[0]:
            dS = torch.zeros(ctx.s_shape, dtype=torch.float32, device=dY.device)
            apart = sel.L == 1 or ctx.col_stride >= rows.n                  # the slots' blocks of S do not overlap
            for s in range(sel.L):
                block = dS[s * ctx.col_stride:s * ctx.col_stride + rows.n]
                bucket = _rowsel_bucket(sel, s, G)
                if apart:
                    _stack_gather_t(rows, bucket, block)
                else:
                    block += _stack_gather_t(rows, bucket, torch.empty_like(block))
        return dS, db, None, None, None, None


def rowsel_conv(S, rows, idx, bias=None, relu=False, col_stride=0):
    """Y[b] = epi(bias + Σ_s Σ_{e ∈ row idx[b, s]} val[e] S[s col_stride + col[e]]): the first Linear of an MLP over the adjacency rows
    idx selects from a SnapshotRows (host integers [B] or [B, L], -1 an empty row, or a prepared RowSelection), without the dense
    [B, L N] input.  S is the transposed weight, [L N, d] with col_stride = N for DynAE, [N, d] for DynGEM.  Differentiable in S and
    bias: the pre-pass of gcn_conv, bucket sums of its result per stacked row from an inverted index, and the plain aggregation over
    the transposed stack; no atomics, repeated calls are bit-identical."""
    _need_cuda(S, bias, rows.val)
    sel = rows.select(idx)
    if sel.rows is not rows:
        raise ValueError("the selection belongs to another SnapshotRows")
    if S.dim() != 2 or S.shape[1] < 1:
        raise ValueError("S must be [rows, d]")
    if S.dtype != torch.float32:
        raise TypeError("fp32 S expected")
    if S.device != rows.device:
        raise ValueError("S on %s but the snapshots on %s" % (S.device, rows.device))
    col_stride = int(col_stride)
    if col_stride < 0 or S.shape[0] < (sel.L - 1) * col_stride + rows.n:
        raise ValueError("S needs at least (L - 1) col_stride + N = %d rows, got %d" % ((sel.L - 1) * max(col_stride, 0) + rows.n, S.shape[0]))
    if sel.L > int(_lib.load().ctgcn_rowsel_max_slots()):
        raise ValueError("at most %d rows per batch position" % int(_lib.load().ctgcn_rowsel_max_slots()))
    return _RowselConv.apply(_row_view(S), _check_bias(bias, S.shape[1], S.device), rows, sel, bool(relu), col_stride)


class _WreconLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Z, rows, sel, beta, divide, scale, relu, overwrite):
        lib = _lib.load()
        B, N = Z.shape
        dev = Z.device
        want_grad = ctx.needs_input_grad[0]
        dZ = (Z.detach() if overwrite else torch.empty(B, N, dtype=torch.float32, device=dev)) if want_grad else None
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ent_ptr, entries = sel.ent_ptr()
        nbytes = int(lib.ctgcn_wrecon_loss_workspace_bytes(B, entries))
        ws = rows.workspace("wrecon", nbytes)
        with torch.cuda.device(dev), _timed("wrecon_loss", n=B, d=N, nnz=entries):
            check(lib.ctgcn_wrecon_loss_f32(B, N, ptr(Z), Z.stride(0), ptr(sel.idx), ptr(ent_ptr), entries, ptr(rows.row_ptr), ptr(rows.col),
                                            ptr(rows.val), beta, ptr(rows.row_sum) if divide else None, scale, 1 if relu else 0, ptr(dZ),
                                            0 if dZ is None else dZ.stride(0), ptr(loss), ptr(ws), nbytes, _stream()), "ctgcn_wrecon_loss_f32")
        ctx.dz, ctx.overwrite = dZ, overwrite
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        # an overwriting call owns Z's memory: no second [B, N] tensor (such a graph is walked once)
        return (ctx.dz.mul_(g) if ctx.overwrite else ctx.dz * g), None, None, None, None, None, None, None


def wrecon_loss(Z, rows, tgt, beta, divide=False, scale=1.0, relu=True, overwrite=False):
    """scale Σ_b Σ_j ((p_bj − x_bj) pen_bj)² / div_b as a fp32 scalar, differentiable in Z: the reconstruction term of DynGEMLoss and
    DynGraph2VecLoss.  p = relu(Z) (relu=True: Z is the last decoder layer's pre-activation) or Z; x_b is row tgt[b] of the
    SnapshotRows (host integers [B] or a RowSelection, -1 an all-zero row); pen is beta where x != 0 and 1 elsewhere; div_b the row's
    weight sum with divide, else 1.  One sweep of Z and a correction at the stored entries: no dense target or penalty tensor.
    overwrite=True lets the gradient take Z's own memory: Z must not be read afterwards, and the backward may run once."""
    _need_cuda(Z, rows.val)
    sel = rows.select(tgt)
    if sel.rows is not rows:
        raise ValueError("the selection belongs to another SnapshotRows")
    if sel.L != 1:
        raise ValueError("one target row per batch position expected")
    if Z.dim() != 2 or tuple(Z.shape) != (sel.B, rows.n):
        raise ValueError("Z must be [%d, %d], got %s" % (sel.B, rows.n, tuple(Z.shape)))
    if Z.dtype != torch.float32:
        raise TypeError("fp32 Z expected")
    if Z.device != rows.device:
        raise ValueError("Z on %s but the snapshots on %s" % (Z.device, rows.device))
    return _WreconLoss.apply(_row_view(Z), rows, sel, float(beta), bool(divide), float(scale), bool(relu), bool(overwrite))


# ------------------------------------------------------------------------- an LSTM layer of any width (ctgcn_lstmcell.hip): DynRNN, DynAERNN
def _lstm_cell_fwd(gi_t, gh, bias, c_prev, h, c, gates):
    lib = _lib.load()
    B, H = c.shape
    ld = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    with torch.cuda.device(c.device), _timed("lstm_cell_fwd", n=B, d=H):
        check(lib.ctgcn_lstm_cell_fwd_f32(B, H, ptr(gi_t), ld(gi_t), ptr(gh), ld(gh), ptr(bias), ptr(c_prev), ld(c_prev), ptr(h), ld(h), ptr(c),
                                          ld(c), ptr(gates), ld(gates), _stream()), "ctgcn_lstm_cell_fwd_f32")


def _lstm_cell_bwd(gates, c, c_prev, dh_out, dh_rec, dc_next, dgates, dc_prev):
    lib = _lib.load()
    B, H = c.shape
    ld = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    with torch.cuda.device(c.device), _timed("lstm_cell_bwd", n=B, d=H):
        check(lib.ctgcn_lstm_cell_bwd_f32(B, H, ptr(gates), ld(gates), ptr(c), ld(c), ptr(c_prev), ld(c_prev), ptr(dh_out), ld(dh_out),
                                          ptr(dh_rec), ld(dh_rec), ptr(dc_next), ld(dc_next), ptr(dgates), ld(dgates), ptr(dc_prev),
                                          ld(dc_prev), _stream()), "ctgcn_lstm_cell_bwd_f32")


def _time_major(t):
    """a [B, L, D] tensor as a contiguous [L, B, D] one: a view where the memory already is (what lstm_layer returns), else a copy"""
    tm = t.transpose(0, 1)
    return tm if tm.is_contiguous() else tm.contiguous()


class _LstmLayer(torch.autograd.Function):
    """Every per-step tensor is time-major, [L, B, .]: a step is a contiguous [B, .] block for the GEMMs, and the steps >= 1 of dgates
    and the steps < L - 1 of h are contiguous too, so dW_hh is one GEMM over them without a copy."""

    @staticmethod
    def forward(ctx, x, gi, w_ih, w_hh, b_ih, b_hh, last_only, train):
        H = w_hh.shape[1]
        dev = w_hh.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        own = gi is None
        if own:
            xt = _time_major(x)
            L, B = xt.shape[:2]
            x2d = xt.reshape(L * B, -1)
            git = (torch.mm(x2d, w_ih.t()) if b_ih is None else torch.addmm(b_ih, x2d, w_ih.t())).view(L, B, 4 * H)
        else:
            xt = None
            git = (gi if gi.stride(2) == 1 else gi.contiguous()).transpose(0, 1)
            L, B = git.shape[:2]
        gh = new(B, 4 * H) if L > 1 else None
        w_hh_t = w_hh.t()
        if train:
            # the activated gates take the memory of a gi made here (a step's kernel reads and writes each element once)
            gates = git if own else new(L, B, 4 * H)
            c_all = new(L, B, H)
            h_all = new(L - 1 if last_only else L, B, H)
            h_last = new(B, H) if last_only else h_all[L - 1]
            for t in range(L):
                if t:
                    torch.mm(h_all[t - 1], w_hh_t, out=gh)
                _lstm_cell_fwd(git[t], gh if t else None, b_hh, c_all[t - 1] if t else None, h_last if t == L - 1 else h_all[t], c_all[t], gates[t])
            ctx.save_for_backward(xt, w_ih, w_hh, gates, c_all, h_all)
            ctx.own, ctx.last_only, ctx.has_bias = own, last_only, (b_ih is not None, b_hh is not None)
        else:
            c2 = new(2, B, H)
            h_all = new(2 if last_only else L, B, H)
            for t in range(L):
                h_t = h_all[t & 1] if last_only else h_all[t]
                if t:
                    torch.mm(h_all[(t - 1) & 1] if last_only else h_all[t - 1], w_hh_t, out=gh)
                _lstm_cell_fwd(git[t], gh if t else None, b_hh, c2[(t - 1) & 1] if t else None, h_t, c2[t & 1], None)
            h_last = h_all[(L - 1) & 1] if last_only else None
        return h_last if last_only else h_all.transpose(0, 1)

    @staticmethod
    def backward(ctx, dout):
        xt, w_ih, w_hh, gates, c_all, h_all = ctx.saved_tensors
        L, B, H4 = gates.shape
        H = H4 // 4
        dev = gates.device
        if dout.dtype != torch.float32 or dout.stride(-1) != 1:
            dout = dout.to(torch.float32).contiguous()
        dgates = torch.empty(L, B, H4, dtype=torch.float32, device=dev)
        dc = torch.empty(B, H, dtype=torch.float32, device=dev) if L > 1 else None
        dh_rec = torch.empty(B, H, dtype=torch.float32, device=dev) if L > 1 else None
        for t in range(L - 1, -1, -1):
            last = t == L - 1
            dh_out = (dout if last else None) if ctx.last_only else dout[:, t]
            # dc is read as dc_next and written as dc_prev by the same thread
            _lstm_cell_bwd(gates[t], c_all[t], c_all[t - 1] if t else None, dh_out, None if last else dh_rec, None if last else dc, dgates[t],
                           dc if t else None)
            if t:
                torch.mm(dgates[t], w_hh, out=dh_rec)
        need = ctx.needs_input_grad
        dg2 = dgates.view(L * B, H4)
        dx = dgi = dw_ih = dw_hh = db_ih = db_hh = None
        if need[3]:
            dw_hh = torch.mm(dgates[1:].reshape((L - 1) * B, H4).t(), h_all[:L - 1].reshape((L - 1) * B, H)) if L > 1 else torch.zeros_like(w_hh)
        if (ctx.has_bias[0] and need[4]) or (ctx.has_bias[1] and need[5]):
            db = dg2.sum(0)
            db_ih = db if ctx.has_bias[0] and need[4] else None
            db_hh = db if ctx.has_bias[1] and need[5] else None
        if ctx.own:
            x2d = xt.reshape(L * B, -1)
            if need[2]:
                dw_ih = torch.mm(dg2.t(), x2d)
            if need[0]:
                dx = torch.mm(dg2, w_ih).view(L, B, -1).transpose(0, 1)
        elif need[1]:
            dgi = dgates.transpose(0, 1)
        return dx, dgi, dw_ih, dw_hh, db_ih, db_hh, None, None


def lstm_layer(x, weight_ih, weight_hh, bias_ih=None, bias_hh=None, last_only=False, gi=None):
    """One batch_first nn.LSTM layer of any hidden width H, zero initial state: h_seq [B, L, H], or with last_only only h_{L-1} [B, H].
    x [B, L, in] is dense; or gi [B, L, 4 H] is the input projection made elsewhere (ops.rowsel_conv over adjacency rows, with bias_ih
    folded by its maker; x, weight_ih and bias_ih are then None).  The parameters are those of the nn.LSTM (gate order i, f, g, o);
    either bias may be None.  One library GEMM makes gi for all steps, one per step >= 1 makes h_{t-1} W_hhᵀ, and one
    ctgcn_lstm_cell_fwd_f32 pass per step does the rest; the backward is one ctgcn_lstm_cell_bwd_f32 pass and one dgates_t W_hh GEMM per
    step, then one GEMM each for dW_hh (over the stacked steps >= 1), dW_ih and dx, and one column sum for both bias gradients.  With
    last_only the steps before the last get no gradient from above and no [B, L, H] zero tensor is made; h_{L-1} is a tensor of its own
    which the backward never reads.  Without grad no gates are kept and c alternates between two buffers.  h_seq is a [B, L, H] view of
    [L, B, H] memory, which a following lstm_layer takes as it is."""
    _need_cuda(x, gi, weight_ih, weight_hh, bias_ih, bias_hh)
    if (x is None) == (gi is None):
        raise ValueError("exactly one of x and gi expected")
    if gi is not None and (weight_ih is not None or bias_ih is not None):
        raise ValueError("with gi, weight_ih and bias_ih belong to whoever made it")
    for t in (x, gi, weight_ih, weight_hh, bias_ih, bias_hh):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("fp32 tensors expected, got %s" % t.dtype)
    if weight_hh.dim() != 2 or weight_hh.shape[0] != 4 * weight_hh.shape[1] or weight_hh.shape[1] < 1:
        raise ValueError("weight_hh must be [4 H, H]")
    H = weight_hh.shape[1]
    seq = x if gi is None else gi
    if seq.dim() != 3 or seq.shape[1] < 1:
        raise ValueError("%s must be [B, L, %s] with L >= 1" % (("x", "in") if gi is None else ("gi", "4 H")))
    if gi is None:
        if weight_ih is None or weight_ih.dim() != 2 or tuple(weight_ih.shape) != (4 * H, x.shape[2]):
            raise ValueError("weight_ih must be [%d, %d]" % (4 * H, x.shape[2]))
    elif gi.shape[2] != 4 * H:
        raise ValueError("gi must be [B, L, %d], got %s" % (4 * H, tuple(gi.shape)))
    for b in (bias_ih, bias_hh):
        if b is not None and tuple(b.shape) != (4 * H,):
            raise ValueError("a bias must be [%d]" % (4 * H))
    for t in (seq, weight_ih, bias_ih, bias_hh):
        if t is not None and t.device != weight_hh.device:
            raise ValueError("tensors on %s and %s" % (t.device, weight_hh.device))
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, gi, weight_ih, weight_hh, bias_ih, bias_hh))
    bias_hh = None if bias_hh is None else (bias_hh if bias_hh.is_contiguous() else bias_hh.contiguous())
    return _LstmLayer.apply(x, gi, None if weight_ih is None else _row_view(weight_ih), _row_view(weight_hh), bias_ih, bias_hh, bool(last_only),
                            train)


# ------------------------------------------------------------------------- a GRU layer of any width (ctgcn_grucell.hip): rnn_reduce_norm
def rnn_cell_enabled():
    """CTGCN_RNN_CELL=0 sends the GRUs of widths other than 128 and the LSTMs the width-128 kernels do not take back to the PyTorch-ROCm
    modules (layers.rnn_over_rows) for A/B measurement; default: library GEMMs plus one fused HIP cell pass per step."""
    return _os.environ.get("CTGCN_RNN_CELL", "1") != "0"


def rnn_cell_ok(rnn, seq):
    """What ops.gru_layer / ops.lstm_layer run for layers.rnn_reduce_norm: an fp32 CUDA sequence through a single-layer, unidirectional,
    batch_first nn.GRU of any hidden size other than 128 (that one has kernels of its own, gru_fused_ok) or nn.LSTM without projection."""
    if not (seq.is_cuda and seq.dtype == torch.float32 and seq.dim() == 3 and rnn_cell_enabled()):
        return False
    if not isinstance(rnn, (torch.nn.GRU, torch.nn.LSTM)) or rnn.num_layers != 1 or rnn.bidirectional or not rnn.batch_first:
        return False
    if rnn.weight_hh_l0.dtype != torch.float32 or not rnn.weight_hh_l0.is_cuda:
        return False
    return rnn.hidden_size != 128 if isinstance(rnn, torch.nn.GRU) else getattr(rnn, "proj_size", 0) == 0


def _gru_cell_fwd(gi_t, gh, b_hh, h_prev, h, gates, q, acc=None, acc_init=False):
    lib = _lib.load()
    B, H = h.shape
    ld = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    with torch.cuda.device(h.device), _timed("gru_cell_fwd", n=B, d=H):
        check(lib.ctgcn_gru_cell_fwd_f32(B, H, ptr(gi_t), ld(gi_t), ptr(gh), ld(gh), ptr(b_hh), ptr(h_prev), ld(h_prev), ptr(h), ld(h), ptr(gates),
                                         ld(gates), ptr(q), ld(q), ptr(acc), ld(acc), int(bool(acc_init)), _stream()), "ctgcn_gru_cell_fwd_f32")


def _gru_cell_bwd(gates, q, h_prev, dh_out, dh_rec, dgi, dgh, dh_prev):
    lib = _lib.load()
    B, H = q.shape
    ld = lambda t: 0 if t is None else t.stride(0)  # noqa: E731
    with torch.cuda.device(q.device), _timed("gru_cell_bwd", n=B, d=H):
        check(lib.ctgcn_gru_cell_bwd_f32(B, H, ptr(gates), ld(gates), ptr(q), ld(q), ptr(h_prev), ld(h_prev), ptr(dh_out), ld(dh_out),
                                         ptr(dh_rec), ld(dh_rec), ptr(dgi), ld(dgi), ptr(dgh), ld(dgh), ptr(dh_prev), ld(dh_prev), _stream()),
              "ctgcn_gru_cell_bwd_f32")


class _GruLayer(torch.autograd.Function):
    """Every per-step tensor is time-major, [L, B, .], as in _LstmLayer: a step is a contiguous [B, .] block for the GEMMs, and the steps
    >= 1 of dgh and the steps < L - 1 of h are contiguous too, so dW_hh is one GEMM over them without a copy."""

    @staticmethod
    def forward(ctx, x, gi, w_ih, w_hh, b_ih, b_hh, reduce_sum, train):
        H = w_hh.shape[1]
        dev = w_hh.device
        new = lambda *shape: torch.empty(*shape, dtype=torch.float32, device=dev)  # noqa: E731
        own = gi is None
        if own:
            xt = _time_major(x)
            L, B = xt.shape[:2]
            x2d = xt.reshape(L * B, -1)
            with _timed("gru_layer_gemm", n=L * B, d=3 * H):
                git = (torch.mm(x2d, w_ih.t()) if b_ih is None else torch.addmm(b_ih, x2d, w_ih.t())).view(L, B, 3 * H)
        else:
            xt = None
            git = (gi if gi.stride(2) == 1 else gi.contiguous()).transpose(0, 1)
            L, B = git.shape[:2]
        gh = new(B, 3 * H) if L > 1 else None
        w_hh_t = w_hh.t()
        acc = new(B, H) if reduce_sum else None
        if train:
            # the activated gates take the memory of a gi made here (a step's kernel reads and writes each element once)
            gates = git if own else new(L, B, 3 * H)
            q_all = new(L, B, H)
            h_all = new(L - 1 if reduce_sum else L, B, H)              # the backward reads h_t as step t + 1's h_prev: never h_{L-1}
            h_last = new(B, H) if reduce_sum else h_all[L - 1]
            for t in range(L):
                if t:
                    with _timed("gru_layer_gemm", n=B, d=3 * H):
                        torch.mm(h_all[t - 1], w_hh_t, out=gh)
                _gru_cell_fwd(git[t], gh if t else None, b_hh, h_all[t - 1] if t else None, h_last if t == L - 1 else h_all[t], gates[t],
                              q_all[t], acc, t == 0)
            ctx.save_for_backward(xt, w_ih, w_hh, gates, q_all, h_all)
            ctx.own, ctx.reduce_sum, ctx.has_bias = own, reduce_sum, (b_ih is not None, b_hh is not None)
        else:
            h_all = new(2 if reduce_sum else L, B, H)
            for t in range(L):
                h_t, h_p = (h_all[t & 1], h_all[(t - 1) & 1]) if reduce_sum else (h_all[t], h_all[t - 1])
                if t:
                    with _timed("gru_layer_gemm", n=B, d=3 * H):
                        torch.mm(h_p, w_hh_t, out=gh)
                _gru_cell_fwd(git[t], gh if t else None, b_hh, h_p if t else None, h_t, None, None, acc, t == 0)
        return acc if reduce_sum else h_all.transpose(0, 1)

    @staticmethod
    def backward(ctx, dout):
        xt, w_ih, w_hh, gates, q_all, h_all = ctx.saved_tensors
        L, B, H3 = gates.shape
        H = H3 // 3
        dev = gates.device
        if dout.dtype != torch.float32 or dout.stride(-1) != 1 or dout.stride(0) < H:           # an expanded gradient has stride 0
            dout = dout.to(torch.float32).contiguous()
        dgi = torch.empty(L, B, H3, dtype=torch.float32, device=dev)
        dgh = torch.empty(L, B, H3, dtype=torch.float32, device=dev)
        dh_rec = torch.empty(B, H, dtype=torch.float32, device=dev) if L > 1 else None
        for t in range(L - 1, -1, -1):
            # dh_rec is read as the complete dh of this step and takes the direct part dh z of dh_prev, written by the same thread;
            # the GEMM then adds dgh_t W_hh to it
            _gru_cell_bwd(gates[t], q_all[t], h_all[t - 1] if t else None, dout if ctx.reduce_sum else dout[:, t], None if t == L - 1 else dh_rec,
                          dgi[t], dgh[t], dh_rec if t else None)
            if t:
                with _timed("gru_layer_gemm", n=B, d=H):
                    dh_rec.addmm_(dgh[t], w_hh)
        need = ctx.needs_input_grad
        dgi2 = dgi.view(L * B, H3)
        dx = dgi_out = dw_ih = dw_hh = db_ih = db_hh = None
        if ctx.has_bias[0] and need[4]:
            db_ih = dgi2.sum(0)
        if ctx.has_bias[1] and need[5]:
            db_hh = dgh.view(L * B, H3).sum(0)                         # differs from db_ih in the n block: da_n r
        with _timed("gru_layer_gemm", n=L * B, d=H3):
            if need[3]:
                dw_hh = torch.mm(dgh[1:].reshape((L - 1) * B, H3).t(), h_all[:L - 1].reshape((L - 1) * B, H)) if L > 1 else torch.zeros_like(w_hh)
            if ctx.own:
                x2d = xt.reshape(L * B, -1)
                if need[2]:
                    dw_ih = torch.mm(dgi2.t(), x2d)
                if need[0]:
                    dx = torch.mm(dgi2, w_ih).view(L, B, -1).transpose(0, 1)
            elif need[1]:
                dgi_out = dgi.transpose(0, 1)
        return dx, dgi_out, dw_ih, dw_hh, db_ih, db_hh, None, None


def gru_layer(x, weight_ih, weight_hh, bias_ih=None, bias_hh=None, reduce_sum=False, gi=None):
    """One batch_first nn.GRU layer of any hidden width H, zero initial state: h_seq [B, L, H], or with reduce_sum the sum of h over the
    steps [B, H].  x [B, L, in] is dense; or gi [B, L, 3 H] is the input projection made elsewhere (bias_ih folded by its maker; x,
    weight_ih and bias_ih are then None).  The parameters are those of the nn.GRU (gate order r, z, n); either bias may be None.
    Differentiable in every tensor argument.  One library GEMM makes gi for all steps, one per step >= 1 makes h_{t-1} W_hhᵀ, and one
    ctgcn_gru_cell_fwd_f32 pass per step does the rest (with reduce_sum it also keeps the running sum); the backward is one
    ctgcn_gru_cell_bwd_f32 pass and one dgh_t W_hh GEMM per step, then one GEMM each for dW_hh (over the stacked steps >= 1), dW_ih and
    dx, and the column sums of dgi (db_ih) and dgh (db_hh: they differ in the n block).
    A training call keeps 5 H floats per (row, step) besides x: the activated gates r, z, n (in the memory of gi), q = h_{t-1} W_hnᵀ +
    b_hn and h; its backward holds another 6 H (dgi and dgh) while it runs.  Without grad nothing per step is kept: h alternates between
    two buffers with reduce_sum (else it is the output), and gi is the only [rows, L, 3 H] buffer.  Rows go through in equal chunks of
    at most _GI_MAX_ELEMS / (3 H L) rows, so that buffer never exceeds _GI_MAX_ELEMS elements; rows are independent sequences, so the
    chunks are exact.  h_seq of an unchunked call is a [B, L, H] view of [L, B, H] memory, which a following layer takes as it is."""
    _need_cuda(x, gi, weight_ih, weight_hh, bias_ih, bias_hh)
    if (x is None) == (gi is None):
        raise ValueError("exactly one of x and gi expected")
    if gi is not None and (weight_ih is not None or bias_ih is not None):
        raise ValueError("with gi, weight_ih and bias_ih belong to whoever made it")
    for t in (x, gi, weight_ih, weight_hh, bias_ih, bias_hh):
        if t is not None and t.dtype != torch.float32:
            raise TypeError("fp32 tensors expected, got %s" % t.dtype)
    if weight_hh.dim() != 2 or weight_hh.shape[0] != 3 * weight_hh.shape[1] or weight_hh.shape[1] < 1:
        raise ValueError("weight_hh must be [3 H, H]")
    H = weight_hh.shape[1]
    seq = x if gi is None else gi
    if seq.dim() != 3 or seq.shape[1] < 1:
        raise ValueError("%s must be [B, L, %s] with L >= 1" % (("x", "in") if gi is None else ("gi", "3 H")))
    if gi is None:
        if weight_ih is None or weight_ih.dim() != 2 or tuple(weight_ih.shape) != (3 * H, x.shape[2]):
            raise ValueError("weight_ih must be [%d, %d]" % (3 * H, x.shape[2]))
    elif gi.shape[2] != 3 * H:
        raise ValueError("gi must be [B, L, %d], got %s" % (3 * H, tuple(gi.shape)))
    for b in (bias_ih, bias_hh):
        if b is not None and tuple(b.shape) != (3 * H,):
            raise ValueError("a bias must be [%d]" % (3 * H))
    for t in (seq, weight_ih, bias_ih, bias_hh):
        if t is not None and t.device != weight_hh.device:
            raise ValueError("tensors on %s and %s" % (t.device, weight_hh.device))
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, gi, weight_ih, weight_hh, bias_ih, bias_hh))
    bias_hh = None if bias_hh is None else (bias_hh if bias_hh.is_contiguous() else bias_hh.contiguous())
    w_ih, w_hh = None if weight_ih is None else _row_view(weight_ih), _row_view(weight_hh)
    rows, L = seq.shape[:2]
    run = lambda part: _GruLayer.apply(part if gi is None else None, None if gi is None else part, w_ih, w_hh, bias_ih, bias_hh,  # noqa: E731
                                       bool(reduce_sum), train)
    max_rows = max(1, _GI_MAX_ELEMS // (3 * H * L))
    if rows <= max_rows:
        return run(seq)
    chunk = -(-rows // -(-rows // max_rows))
    return torch.cat([run(seq[lo:lo + chunk]) for lo in range(0, rows, chunk)], 0)


# ------------------------------------------------------------------------------------- fp64 blocks (ctgcn_timers.hip)
def _f64_block(t, what):
    if t.dtype != torch.float64 or t.dim() != 2:
        raise TypeError("%s must be a 2-D fp64 tensor, got %s %s" % (what, t.dtype, tuple(t.shape)))
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


def _f64_out(out, rows, cols, like, what):
    if out is None:
        return torch.empty(rows, cols, dtype=torch.float64, device=like.device)
    if out.dtype != torch.float64 or tuple(out.shape) != (rows, cols) or out.stride(1) != 1 or out.stride(0) < cols or out.device != like.device:
        raise ValueError("%s must be a [%d, %d] fp64 tensor with unit column stride on %s" % (what, rows, cols, like.device))
    return out


def _stored(t):
    """t, or one zero of its kind for a matrix that stores nothing (an empty tensor has no address, and the entries are never read)"""
    return t if t is None or t.numel() else t.new_zeros(1)


def spmm_csr_f64(row_ptr, col, val, x, out=None, accumulate=False):
    """Y = A·X (or Y += A·X into out) in fp64 on [n, b] blocks; x and out may be column slices of wider buffers."""
    _need_cuda(row_ptr, col, val, x, out)
    lib = _lib.load()
    x = _f64_block(x, "x")
    if val.dtype != torch.float64:
        raise TypeError("fp64 values expected")
    n, b = row_ptr.numel() - 1, x.shape[1]
    if out is None:
        accumulate = False
    out = _f64_out(out, n, b, x, "out")
    with torch.cuda.device(x.device):
        check(lib.ctgcn_spmm_csr_f64(n, b, ptr(_i32(row_ptr)), ptr(_stored(_i32(col))), ptr(_stored(val.contiguous())), ptr(x), x.stride(0), ptr(out), out.stride(0),
                                     1 if accumulate else 0, _stream()), "ctgcn_spmm_csr_f64")
    return out


def tsgemm_tn(x, y):
    """G [b1, b2] = xᵀ·y over the n rows of two tall fp64 blocks (b1, b2 <= 512); fixed summation order."""
    _need_cuda(x, y)
    lib = _lib.load()
    x, y = _f64_block(x, "x"), _f64_block(y, "y")
    if x.shape[0] != y.shape[0]:
        raise ValueError("x and y must have the same rows")
    n, b1, b2 = x.shape[0], x.shape[1], y.shape[1]
    G = torch.empty(b1, b2, dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        nb = lib.ctgcn_tsgemm_tn_workspace_bytes(n, b1, b2)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=x.device)
        check(lib.ctgcn_tsgemm_tn_f64(n, b1, b2, ptr(x), x.stride(0), ptr(y), y.stride(0), ptr(G), ptr(ws), nb, _stream()), "ctgcn_tsgemm_tn_f64")
    return G


def tsgemm_nn(x, c, out=None, colsq=False):
    """Y [n, b2] = x [n, b1]·c [b1, b2] in fp64 (b1 <= 1024, b2 <= 512); with colsq also the column sums of squares of Y: (Y, colsq)."""
    _need_cuda(x, c, out)
    lib = _lib.load()
    x, c = _f64_block(x, "x"), _f64_block(c, "c")
    if c.shape[0] != x.shape[1]:
        raise ValueError("c must have x's columns as rows")
    n, b1, b2 = x.shape[0], x.shape[1], c.shape[1]
    out = _f64_out(out, n, b2, x, "out")
    sq = torch.empty(b2, dtype=torch.float64, device=x.device) if colsq else None
    with torch.cuda.device(x.device):
        nb = lib.ctgcn_tsgemm_nn_workspace_bytes(n, b2) if colsq else 0
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=x.device) if colsq else None
        check(lib.ctgcn_tsgemm_nn_f64(n, b1, b2, ptr(x), x.stride(0), ptr(c), c.stride(0), ptr(out), out.stride(0), ptr(sq), ptr(ws), nb,
                                      _stream()), "ctgcn_tsgemm_nn_f64")
    return (out, sq) if colsq else out


def timers_obj(row_ptr, col, s, U, V, s_old=None):
    """Device double[2] over the stored entries (r, c, s) of a CSR matrix, d = ⟨U_r, V_c⟩: (Σ s², Σ s·d), or with s_old (values on the
    same pattern) (Σ (s_old + s − d)² − (s_old − d)², Σ s·d)."""
    _need_cuda(row_ptr, col, s, U, V, s_old)
    lib = _lib.load()
    U, V = _f64_block(U, "U"), _f64_block(V, "V")
    n, k = row_ptr.numel() - 1, U.shape[1]
    if U.shape[0] != n or V.shape[1] != k:
        raise ValueError("U must be [n, k] and V [., k]")
    for t in (s, s_old):
        if t is not None and (t.dtype != torch.float64 or t.numel() != col.numel()):
            raise TypeError("one fp64 value per stored entry expected")
    out = torch.zeros(2, dtype=torch.float64, device=U.device)
    with torch.cuda.device(U.device):
        nb = lib.ctgcn_timers_obj_workspace_bytes(n, k)
        ws = torch.empty(max(nb, 8), dtype=torch.uint8, device=U.device)
        check(lib.ctgcn_timers_obj_f64(n, k, ptr(_i32(row_ptr)), ptr(_stored(_i32(col))), ptr(_stored(s.contiguous())),
                                       ptr(None if s_old is None else _stored(s_old.contiguous())),
                                       ptr(U), U.stride(0), ptr(V), V.stride(0), ptr(out), ptr(ws), nb, _stream()), "ctgcn_timers_obj_f64")
    return out


SYM_TOPK_DROP = 1e-7        # a direction of A·Q whose norm is below this fraction of the largest leaves the block


def _chol_inverse_t(G):
    """L⁻ᵀ of G = L Lᵀ (host, numpy), or None when G is not safely positive definite"""
    import numpy as np
    try:
        L = np.linalg.cholesky((G + G.T) / 2)
    except np.linalg.LinAlgError:
        return None
    d = np.diag(L)
    if not np.all(np.isfinite(d)) or d.min() <= SYM_TOPK_DROP * d.max():
        return None
    return np.linalg.inv(L).T


def _orthonormalise(Z, out_buf):
    """CholeskyQR2 of the tall block Z into the leading columns of out_buf; returns the view.  Two passes of G = ZᵀZ = L Lᵀ (b x b,
    on the host), Z ← Z L⁻ᵀ.  When the first G is not safely positive definite (A·Q has lost rank: an operator of rank below the block
    width) the first pass uses G = V D Vᵀ instead and keeps the directions with √(D / D_max) above SYM_TOPK_DROP, so the block narrows
    to the operator's numerical rank; an all-zero Z gives width 0."""
    import numpy as np
    dev = Z.device
    G = tsgemm_tn(Z, Z).cpu().numpy()
    C = _chol_inverse_t(G)
    if C is None:
        D, Vv = np.linalg.eigh((G + G.T) / 2)
        keep = D > (SYM_TOPK_DROP ** 2) * max(D.max(), 0.0)
        if not keep.any():
            return out_buf[:, :0]
        C = Vv[:, keep] / np.sqrt(D[keep])
    Q1 = tsgemm_nn(Z, torch.from_numpy(np.ascontiguousarray(C)).to(dev))
    C2 = _chol_inverse_t(tsgemm_tn(Q1, Q1).cpu().numpy())
    if C2 is None:
        raise RuntimeError("sym_topk: the second CholeskyQR pass met a Gram matrix that is not positive definite")
    return tsgemm_nn(Q1, torch.from_numpy(np.ascontiguousarray(C2)).to(dev), out=out_buf[:, :C2.shape[0]])


def sym_topk(apply, n, k, tol=1e-12, max_iter=5000, seed=0, device=None, _deficient_ok=False):
    """The k eigenpairs of largest magnitude of a symmetric operator given as a callable on [n, b] fp64 device blocks (apply(Q) -> A·Q;
    Q may be a column slice of a wider buffer): (w [k], X [n, k]) on the device, sorted by |w| descending, X orthonormal.

    Block subspace iteration with Rayleigh–Ritz on a block of min(n, 2 k + 8) columns: Z = A·Q, H = QᵀZ, H = S Θ Sᵀ on the host, and
    the residuals ‖A x − w x‖₂ of the k wanted Ritz pairs as the column norms of [Z | Q]·[S; −S Θ] (one ctgcn_tsgemm_nn_f64 with its
    sums of squares); then Q ← CholeskyQR2(Z).  It stops when every wanted pair has ‖A x − w x‖₂ <= tol·|w₁| and raises a RuntimeError
    naming the achieved residual after max_iter iterations: unconverged pairs are never returned.  Only b x b matrices and k-vectors
    cross to the host inside the loop.  The start block is a seeded host generator's normal draws, so a seed gives the same block on
    every run and device.  An operator of rank r < k has no k pairs this iteration can reach: RuntimeError.
    sym_topk.last holds (iterations, largest residual) of the latest call."""
    import numpy as np
    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.CtgcnHipError("ctgcn_amd runs on MI355X only: sym_topk on %s; there is no CPU fallback." % device)
    n, k = int(n), int(k)
    if k < 1 or k > n:
        raise ValueError("need 1 <= k <= n, got k=%d n=%d" % (k, n))
    b = min(n, 2 * k + 8)
    if b > 512:
        raise ValueError("sym_topk: block width %d above 512 (k <= 252)" % b)
    gen = torch.Generator().manual_seed(int(seed))
    start = torch.randn(n, b, generator=gen, dtype=torch.float64).to(device)
    W = torch.empty(n, 2 * b, dtype=torch.float64, device=device)          # [Z | Q], so that one product gives the residual block
    Qbuf = torch.empty(n, b, dtype=torch.float64, device=device)
    Q = _orthonormalise(start, Qbuf)
    del start
    res_max = float("inf")
    for it in range(1, int(max_iter) + 1):
        bw = Q.shape[1]
        kk = min(k, bw)
        if bw < k and not _deficient_ok:
            raise RuntimeError("sym_topk: the operator has numerical rank %d, below the %d pairs asked for" % (bw, k))
        if bw == 0:
            break
        Zv, Qv = W[:, :bw], W[:, bw:2 * bw]
        Qv.copy_(Q)
        Zv.copy_(apply(Qv))
        H = tsgemm_tn(Qv, Zv).cpu().numpy()
        theta, S = np.linalg.eigh((H + H.T) / 2)
        order = np.argsort(-np.abs(theta), kind="stable")[:kk]
        theta, S = theta[order], np.ascontiguousarray(S[:, order])
        C = torch.from_numpy(np.concatenate((S, -S * theta[None, :]), axis=0)).to(device)
        _, sq = tsgemm_nn(W[:, :2 * bw], C, colsq=True)
        res_max = float(np.sqrt(sq.cpu().numpy().max()))
        if res_max <= tol * abs(theta[0]):
            X = torch.zeros(n, k, dtype=torch.float64, device=device)
            tsgemm_nn(Qv, torch.from_numpy(S).to(device), out=X[:, :kk])
            w = torch.zeros(k, dtype=torch.float64, device=device)
            w[:kk] = torch.from_numpy(theta).to(device)
            sym_topk.last = (it, res_max)
            return w, X
        Q = _orthonormalise(Zv, Qbuf)
    else:
        raise RuntimeError("sym_topk: residual %.3e after %d iterations, above tol·|w1| = %.3e" % (res_max, max_iter, tol * abs(theta[0])))
    sym_topk.last = (it, 0.0)          # a zero operator (only with _deficient_ok): zero pairs
    return torch.zeros(k, dtype=torch.float64, device=device), torch.zeros(n, k, dtype=torch.float64, device=device)


sym_topk.last = (0, 0.0)


# ------------------------------------------------------------------------------------ top-k link ranking (ctgcn_topk.hip)
TOPK_TILE = 32                          # query rows of a wave and candidate columns of a tile
TOPK_MAX_CHUNKS = 256
_TOPK_WAVES = 1024                      # waves the default col_chunks aims at: four a CU on 256 CUs


def topk_max_k():
    return int(_lib.load().ctgcn_topk_max_k())


def topk_max_d():
    return int(_lib.load().ctgcn_topk_max_d())


def _topk_exclusion(exclude, n, dev):
    """(row_ptr, col) of the exclusion pattern; its shape, device and ascending columns are checked once per GcnAdj"""
    if not isinstance(exclude, GcnAdj):
        raise TypeError("exclude must be an ops.GcnAdj, got %s" % type(exclude).__name__)
    if exclude.n != n:
        raise ValueError("exclude has %d rows, E has %d" % (exclude.n, n))
    if exclude.device != dev:
        raise ValueError("exclude is on %s, E on %s" % (exclude.device, dev))
    if not getattr(exclude, "_topk_checked", False):
        if exclude.nnz:
            col = exclude.col.to(torch.int64)
            if int(col.min()) < 0 or int(col.max()) >= n:
                raise ValueError("exclude has a column outside [0, %d)" % n)
            key = exclude._rows() * n + col
            if exclude.nnz > 1 and not bool((key[1:] > key[:-1]).all()):
                raise ValueError("exclude's columns must ascend within every row (sorted, no duplicates)")
        exclude._topk_checked = True
    return exclude.row_ptr, exclude.col


def topk_scores(E, k, rows=None, row_bias=None, col_bias=None, exclude_self=False, upper_only=False, exclude=None, col_chunks=None):
    """The k best admissible candidates of every query row by s(i, j) = E[q] · E[j] (+ col_bias[j]) (+ row_bias[i]), q = rows[i] or i:
    (score float32 [m, k], index int32 [m, k]), each row by score descending and index ascending among equal scores, unused slots
    -inf / -1.  The score is one ascending fp32 fmaf chain on the matrix cores and the two adds, in that order; the [m, n] matrix is
    never stored.  exclude_self drops j == q, upper_only j <= q, exclude (a GcnAdj, only its pattern is read) the stored entries of
    row q.  col_chunks cuts the candidates into that many column ranges swept by different blocks (None: enough to fill the device);
    the result does not depend on it.  No autograd."""
    _need_cuda(E, rows, row_bias, col_bias)
    if E.dtype != torch.float32:
        raise TypeError("E must be float32, got %s" % E.dtype)
    if E.dim() != 2:
        raise ValueError("E must be [n, d]")
    n, d = E.shape
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1, got %d" % k)
    if k > topk_max_k():
        raise ValueError("k = %d above ctgcn_topk_max_k() = %d" % (k, topk_max_k()))
    if d < 1 or d > topk_max_d():
        raise ValueError("d = %d outside [1, ctgcn_topk_max_d() = %d]" % (d, topk_max_d()))
    if n >= 2 ** 31:
        raise ValueError("n = %d: at most 2^31 - 1 candidates" % n)
    dev = E.device
    E = E.detach()
    if n and (E.stride(1) != 1 or E.stride(0) < d):
        E = E.contiguous()
    if rows is not None:
        if rows.dtype not in (torch.int32, torch.int64):
            raise TypeError("rows must be int32 or int64, got %s" % rows.dtype)
        if rows.dim() != 1 or rows.device != dev:
            raise ValueError("rows must be a vector on E's device")
        if rows.numel() and (int(rows.min()) < 0 or int(rows.max()) >= n):
            raise ValueError("rows has an entry outside [0, %d)" % n)
        rows = _i32(rows)
        m = rows.numel()
    else:
        m = n
    for name, b, length in (("row_bias", row_bias, m), ("col_bias", col_bias, n)):
        if b is None:
            continue
        if b.dtype != torch.float32:
            raise TypeError("%s must be float32, got %s" % (name, b.dtype))
        if b.dim() != 1 or b.numel() != length or b.device != dev:
            raise ValueError("%s must be a vector of %d entries on E's device" % (name, length))
    row_bias = None if row_bias is None else row_bias.detach().contiguous()
    col_bias = None if col_bias is None else col_bias.detach().contiguous()
    ex_ptr, ex_col = (None, None) if exclude is None else _topk_exclusion(exclude, n, dev)
    tiles = (n + TOPK_TILE - 1) // TOPK_TILE
    if col_chunks is None:
        row_tiles = max(1, (m + TOPK_TILE - 1) // TOPK_TILE)
        col_chunks = max(1, min((_TOPK_WAVES + row_tiles - 1) // row_tiles, tiles, 64))
    col_chunks = int(col_chunks)
    if col_chunks < 1 or col_chunks > TOPK_MAX_CHUNKS:
        raise ValueError("col_chunks = %d outside [1, %d]" % (col_chunks, TOPK_MAX_CHUNKS))
    flags = (_lib.TOPK_NO_SELF if exclude_self else 0) | (_lib.TOPK_UPPER if upper_only else 0)
    score = torch.empty(m, k, dtype=torch.float32, device=dev)
    index = torch.empty(m, k, dtype=torch.int32, device=dev)
    if m == 0:
        return score, index
    lib = _lib.load()
    with torch.cuda.device(dev), _timed("topk_scores", m=m, n=n, d=d, k=k, col_chunks=col_chunks):
        nbytes = int(lib.ctgcn_topk_workspace_bytes(m, n, k, col_chunks))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev) if nbytes else None
        check(lib.ctgcn_topk_scores_f32(m, n, d, k, ptr(E), E.stride(0) if n else d, ptr(rows), ptr(row_bias), ptr(col_bias), ptr(ex_ptr),
                                        ptr(ex_col), flags, col_chunks, ptr(score), ptr(index), ptr(ws), nbytes, _stream()),
              "ctgcn_topk_scores_f32")
    return score, index
