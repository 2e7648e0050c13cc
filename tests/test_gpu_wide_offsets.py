"""Every strided entry point of include/ctgcn_hip.h with one operand laid out across the 2^31-element and 4 GiB offsets
(tests/_wide_ref.py): a tiny logical matrix whose rows are 2^27 + 256 floats apart, 2^31 floats into a 24 GiB allocation.  A kernel
that forms row * ld, or a byte offset, in 32 bits reads or writes a wrong place that is still inside the allocation, so a regression
shows as a wrong number.  For every (entry point, wide operand, layout):

  * the result equals a float64 host computation on the small logical data, at the tolerance of the op's own test file;
  * it is bit-identical to the call on a dense operand of the same alignment class (the kernels are deterministic);
  * a wide OUTPUT leaves the 256 floats before and after each of its rows untouched.

TABLE is the contract: tests/test_wide_offsets_host.py fails when include/ctgcn_hip.h has a function with a stride parameter that
TABLE does not list, or TABLE names something the header does not have.  A row that is not driven yet says so (`deferred`)."""
import functools

import numpy as np
import pytest
import torch

import _wide_ref as W
from conftest import check_close, close_scaled

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = W.MAX_ROWS                # 33 rows: a second 32-row tile, a third 16-row tile
BOTH = ("aligned", "odd")
ALIGNED = ("aligned",)        # entry points that refuse rows that are not 16-byte (or 8-byte) aligned


def _row(wide, drive="ctypes", dense=None, deferred=None):
    """wide: {stride parameter: layouts}; dense: {stride parameter: why it is never made wide}; drive: how the case calls the kernel"""
    return {"wide": wide, "dense": dense or {}, "drive": drive, "deferred": deferred}


def _todo(why, *params):
    """a row that is listed and not driven yet: every stride parameter named, one line of reason"""
    return _row({k: BOTH for k in params}, deferred=why)


_GAT = "not driven yet: needs the float64 mirror of the attention backward (R, csum, B, ksum) or of GATConv's form on raw CSR operands"
_EVAL = "not driven yet: needs the chunked class tables of evaluation._ovr as fixture, with E wide (float64 model: tests/_logreg_ref.py)"

TABLE = {
    # ------------------------------------------------------------------------------------------------ core path
    "ctgcn_transpose_bias_f32": _row({"ldw": BOTH, "ldo": BOTH}),
    "ctgcn_spmm_csr_f32": _row({"ldx": BOTH, "ldy": BOTH}, drive="ops.spmm_csr"),
    "ctgcn_core_aggregate_f32": _row({"ldx": BOTH}),
    "ctgcn_core_aggregate_split_f32": _row({"ldx": ALIGNED}),
    "ctgcn_core_aggregate_bwd_f32": _row({"lddx": BOTH}),
    "ctgcn_gru_seq_f32": _row({"ld_out": ALIGNED}),
    "ctgcn_layernorm_bwd_f32": _row({"ld_dy": ALIGNED}),
    "ctgcn_gru_layer_f32": _row({"ldx": ALIGNED, "ld_out": ALIGNED, "ld_row": ALIGNED, "step_offsets": ALIGNED}),
    "ctgcn_gru_layer_presplit_f32": _row({"ld_out": ALIGNED}),
    "ctgcn_gru_input_proj_f32": _row({"ldx": ALIGNED}, drive="ops._project"),
    "ctgcn_gru_input_grad_f32": _row({"ldx": ALIGNED}, drive="ops._project_grad"),
    "ctgcn_gru_weight_grad_f32": _row({"ldg01": BOTH, "ldg2": BOTH, "ldx": BOTH}, drive="ops._weight_grad"),
    "ctgcn_gru_bwd_in_f32": _row({"ldx": ALIGNED}),          # an ldx that is no multiple of 4 is refused by contract
    "ctgcn_linear_f32": _row({"ldx": BOTH, "ldw": BOTH, "ldy": BOTH}),
    "ctgcn_split_rows_f32": _row({"ldx": BOTH}),
    "ctgcn_pack_weight_f32": _row({"ldw": BOTH}),
    "ctgcn_linear_packed_f32": _row({"ldy": BOTH}),
    "ctgcn_linear_presplit_f32": _row({"ldw": BOTH, "ldy": BOTH}),
    # ------------------------------------------------------------------------------------------------ gather family
    "ctgcn_gcn_layer_fwd_f32": _row({"lds": BOTH, "ldy": BOTH}),
    "ctgcn_gcn_layer_bwd_f32": _row({"lddy": BOTH, "ldy": BOTH, "ldds": BOTH}),
    "ctgcn_gcn_conv_fwd_f32": _row({"lds": BOTH, "ldy": BOTH}),
    "ctgcn_gcn_conv_prep_f32": _row({"lddy": BOTH, "ldy": BOTH, "ldg": BOTH}),
    "ctgcn_tg_conv_fwd_f32": _row({"lds": BOTH, "ldt": BOTH, "ldy": BOTH}),
    "ctgcn_tg_conv_prep_f32": _row({"lddy": BOTH, "ldy": BOTH, "ldg": BOTH}),
    "ctgcn_pool_conv_fwd_f32": _row({"lds": BOTH, "ldt": BOTH, "ldy": BOTH, "ldsave": BOTH}),
    "ctgcn_pool_conv_prep_f32": _row({"lddy": BOTH, "ldy": BOTH, "ldg": BOTH}),
    "ctgcn_pool_max_fwd_f32": _row({"lds": BOTH, "ldy": BOTH, "ldarg": BOTH}),
    "ctgcn_pool_max_bwd_f32": _row({"lddy": BOTH, "ldarg": BOTH, "ldds": BOTH}),
    "ctgcn_bn_stats_f32": _row({"ldx": BOTH}),
    "ctgcn_bn_apply_f32": _row({"ldx": BOTH, "ldy": BOTH}),
    "ctgcn_bn_bwd_f32": _row({"ldx": BOTH, "lddy": BOTH, "lddx": BOTH}),
    # ------------------------------------------------------------------------------------- GRU / LSTM cell row strides
    "ctgcn_gru_cell_fwd_f32": _row({k: BOTH for k in ("ldgi", "ldgh", "ldhp", "ldh", "ldg", "ldq", "ldacc")}),
    "ctgcn_gru_cell_bwd_f32": _row({k: BOTH for k in ("ldg", "ldq", "ldhp", "lddo", "lddr", "lddgi", "lddgh", "lddp")}),
    "ctgcn_lstm_cell_fwd_f32": _row({k: BOTH for k in ("ldgi", "ldgh", "ldcp", "ldh", "ldc", "ldg")}),
    "ctgcn_lstm_cell_bwd_f32": _row({k: BOTH for k in ("ldg", "ldc", "ldcp", "lddo", "lddr", "lddn", "lddg", "lddp")}),
    # ------------------------------------------------------------------------------------- row-selected passes (DynGEM)
    "ctgcn_rowsel_conv_fwd_f32": _row({"lds": BOTH, "col_stride": ALIGNED, "ldy": BOTH}),
    "ctgcn_rowsel_bucket_f32": _row({"ldg": BOTH, "ldout": BOTH}),
    "ctgcn_gat_fwd_f32": _row({"lds": BOTH, "ldout": BOTH, "ldy": BOTH}),
    "ctgcn_gat_bwd_prep_f32": _row({"lddy": BOTH, "ldy": BOTH, "ldg": BOTH}),
    "ctgcn_gat_da_f32": _row({"lds": BOTH}),
    "ctgcn_tgat_fwd_f32": _row({"lds": BOTH, "ldout": BOTH, "ldy": BOTH}),
    "ctgcn_ggru_gates_fwd_f32": _row({"ldu": BOTH, "ldh": BOTH}),
    "ctgcn_ggru_blend_fwd_f32": _row({"ldv": BOTH, "ldc": BOTH, "ldz": BOTH, "ldh": BOTH}),
    "ctgcn_vgrnn_heads_fwd_f32": _row({"lds": BOTH, "ldnoise": BOTH}),
    "ctgcn_vgrnn_bwd_prep_f32": _row({k: BOTH for k in ("ldg0", "ldg1", "ldg2", "lds0", "lds1", "lds2", "ldG")}),
    # ------------------------------------------------------------------------- evaluation passes over an embedding E
    "ctgcn_lp_grad_f32": _row({"lde": BOTH}, drive="evaluation._logreg"),
    "ctgcn_lp_hess_f32": _row({"lde": BOTH}, drive="evaluation._logreg"),
    "ctgcn_lp_scores_f32": _row({"lde": BOTH}, drive="evaluation._logreg"),
    "ctgcn_cls_head_fwd_f32": _row({"lde": BOTH}, drive="ops.cls_head_forward"),
    "ctgcn_cls_head_bwd_f32": _row({"lde": BOTH, "ldde": BOTH}, drive="ops.cls_head_backward"),
    "ctgcn_sim_gram_f32": _row({"lde": BOTH}),
    "ctgcn_ridge_gram_f32": _row({"ldx": BOTH}),
    "ctgcn_ridge_sse_f32": _row({"ldx": BOTH}),
    "ctgcn_sim_gram_f64": _row({"lde": ALIGNED}),
    "ctgcn_ridge_gram_f64": _row({"ldx": ALIGNED}),
    "ctgcn_ridge_sse_f64": _row({"ldx": ALIGNED}),
    # ------------------------------------------- the fp64 TIMERS passes (8-byte elements: the aligned layout, 32 rows)
    "ctgcn_spmm_csr_f64": _row({"ldx": ALIGNED, "ldy": ALIGNED}),
    "ctgcn_tsgemm_tn_f64": _row({"ldx": ALIGNED, "ldy": ALIGNED}),
    "ctgcn_tsgemm_nn_f64": _row({"ldx": ALIGNED, "ldc": ALIGNED, "ldy": ALIGNED}),
    "ctgcn_timers_obj_f64": _row({"ldu": ALIGNED, "ldv": ALIGNED}),
    # ------------------------------------------------------------------------------------------ listed, not driven yet
    "ctgcn_transpose_bias_group_f32": _todo("not driven yet: grouped call (descriptor table + host pointer arrays); same kernel body as ctgcn_transpose_bias_f32", "ldw", "ldo"),
    "ctgcn_linear_packed_group_f32": _todo("not driven yet: grouped call over whole 128-row panels: a wide y needs 128 rows, the layouts hold 33", "ldy"),
    "ctgcn_negsampling_loss_fwd_bwd_f32": _todo("not driven yet: needs the exact sampler model of tests/_sampling_ref.py to build its index arrays", "lde", "ldg"),
    "ctgcn_reconstruction_loss_fwd_bwd_f32": _todo("not driven yet: needs the epoch-loss fixture of tests/test_gpu_epoch_loss.py", "lds", "lde", "ldds", "ldde"),
    "ctgcn_write_embedding_tsv": _todo("not driven: a HOST function on a host pointer (no device addressing); a wide view would need a 16 GiB host mapping", "ld"),
    "ctgcn_nc_grad_f32": _todo(_EVAL, "lde"),
    "ctgcn_nc_hess_f32": _todo(_EVAL, "lde"),
    "ctgcn_nc_predict_f32": _todo(_EVAL, "lde"),
    "ctgcn_ec_grad_f32": _todo(_EVAL, "lde"),
    "ctgcn_ec_hess_f32": _todo(_EVAL, "lde"),
    "ctgcn_ec_predict_f32": _todo(_EVAL, "lde"),
    "ctgcn_gat_bwd_row_f32": _todo(_GAT, "lds", "ldg", "ldr"),
    "ctgcn_gat_bwd_col_f32": _todo(_GAT, "ldg", "lds", "ldds", "ldb"),
    "ctgcn_tgat_bwd_row_f32": _todo(_GAT, "lds", "ldg", "ldy", "ldr"),
    "ctgcn_tgat_bwd_col_f32": _todo(_GAT, "ldg", "lds", "ldds", "ldb"),
    "ctgcn_pgnn_conv_fwd_f32": _todo("not driven yet: needs the anchor tables of ops.pgnn_prepare as fixture", "ldps", "ldstruct"),
    "ctgcn_pgnn_conv_bwd_row_f32": _todo("not driven yet: needs the anchor tables of ops.pgnn_prepare as fixture", "ldps", "ldgs", "ldg", "ldgse"),
    "ctgcn_pgnn_conv_bwd_pull_f32": _todo("not driven yet: needs the pull pieces of ops.pgnn_prepare as fixture", "ldps", "ldgse", "ldg"),
    "ctgcn_vae_nll_dense_f32": _todo("not driven yet: needs the tiled loss model of tests/_vgrnn_ref.py (decomposed_nll)", "ldz", "lddz"),
    "ctgcn_vae_nll_entries_f32": _todo("not driven yet: needs the tiled loss model of tests/_vgrnn_ref.py (decomposed_nll)", "ldz"),
    "ctgcn_wrecon_loss_f32": _todo("not driven yet: needs ops.SnapshotRows as fixture", "ldz", "lddz"),
}


def cases():
    out = []
    for fn, row in TABLE.items():
        if row["deferred"]:
            continue
        for param, layouts in row["wide"].items():
            for layout in layouts:
                out.append((fn, param, layout))
    return out


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture(scope="module")
def arena():
    total = torch.cuda.get_device_properties(0).total_memory
    if total < 64 * (1 << 30):
        pytest.skip("the wide-stride arena needs a device with at least 64 GiB (this one has %.0f GiB)" % (total / 2 ** 30))
    torch.cuda.reset_peak_memory_stats()
    a = W.WideArena(DEV)
    yield a
    a.release()


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
    """a case that left the device in an error state ends the module: nothing more is launched on it"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device error before this test, stopping: %s" % e, returncode=3)
    yield


def _lib():
    from ctgcn_amd import _lib as L
    return L.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ck(rc, what):
    from ctgcn_amd import _lib as L
    L.check(rc, what)


def _p(t):
    return None if t is None else t.data_ptr()


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + 1000 * len(shape) + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def _ints(*shape, seed=0, lo=-4, hi=5):
    """small integers as fp32: with weights that are multiples of 1/4 every partial sum is exact, whatever the order of a long row's terms"""
    g = torch.Generator().manual_seed(seed + 77 * len(shape) + sum(shape))
    return torch.randint(lo, hi, shape, generator=g).float().to(DEV)


def _run_case(arena, layout, wide, ins, outs, call, ref, compare, bitwise=True):
    """ins / outs: name -> small dense device tensor (outs: their initial contents, None = sentinel-filled float [shape given as tuple]).
    `wide` names the one operand that goes to the arena.  call(t) runs the kernel on the dict of tensors.  ref: name -> float64.
    compare(name, got, ref64) asserts the tolerance."""
    def fresh_outs():
        return {k: (torch.full(v, W.SENTINEL, device=DEV) if isinstance(v, tuple) else v.clone()) for k, v in outs.items()}

    # the dense call, with the operand in question in the layout's alignment class
    t, o = dict(ins), fresh_outs()
    if wide in t:
        t[wide] = W.dense_twin(t[wide], layout)
    else:
        o[wide] = W.dense_twin(o[wide], layout)
    call({**t, **o})
    dense = {k: v.clone() for k, v in o.items()}
    # the wide call
    t, o = dict(ins), fresh_outs()
    if wide in t:
        t[wide] = arena.put(layout, t[wide])
    else:
        n, d = o[wide].shape
        init = None if isinstance(outs[wide], tuple) else outs[wide]
        dt = None if init is None or init.dtype == torch.float32 else init.dtype               # int32 outputs: same 4-byte elements
        o[wide] = arena.out(layout, n, d, dtype=dt, fill=init if dt is None else init.contiguous().view(torch.float32))
    call({**t, **o})
    torch.cuda.synchronize()
    if wide in outs:
        assert arena.guards_intact(layout, n, d, dtype=dt), "%s: the kernel wrote outside the rows of its wide output" % wide
        o[wide] = arena.read(layout, n, d, dtype=dt)
    for k in outs:
        if k in ref:
            compare(k, o[k], ref[k])
        if bitwise:
            assert torch.equal(o[k], dense[k]), "%s: wide and dense calls differ by %g" % (k, float((o[k].double() - dense[k].double()).abs().max()))


def _exact(name, got, ref64):
    assert torch.equal(got.double().cpu(), ref64.cpu()), name


def _scaled(rtol=1e-5, atol_scale=2e-6):
    return lambda name, got, ref64: close_scaled(got.cpu().numpy(), ref64.cpu().numpy(), rtol=rtol, atol_scale=atol_scale)


def _floor(floor):
    """tests/test_gpu_dyngem_ops.py::held without its yardstick: |err| <= floor max|ref| (the inputs here sum exactly in fp32)"""
    def compare(name, got, ref64):
        top = float(ref64.abs().max())
        assert top > 0 and float((got.double().cpu() - ref64).abs().max()) <= floor * top, name
    return compare


def _widths(layout):
    return (128, 50)          # 128 and a width that is no multiple of 4


# ------------------------------------------------------------------------------------------ transpose, SpMM, aggregation
def _drive_transpose_bias(arena, param, layout):
    """tests/test_gpu_kernels.py::test_linear_of_identity_is_transposed_weight_plus_bias: exact (data movement and one add)"""
    lib = _lib()
    for width in _widths(layout):
        n, d = (width + 2, N) if param == "ldw" else (N, width)         # the wide operand has 33 rows: w is [d, n], out [n, d]
        w, bias = _rand(d, n, seed=1), _rand(d, seed=2)

        def call(t):
            _ck(lib.ctgcn_transpose_bias_f32(n, d, _p(t["w"]), t["w"].stride(0), _p(bias), _p(t["out"]), t["out"].stride(0), _stream()), "transpose_bias")

        ref = {"out": (w.double().t() + bias.double()).float().double()}   # one fp32 add: the rounded float64 sum is the same number
        _run_case(arena, layout, "w" if param == "ldw" else "out", {"w": w}, {"out": (n, d)}, call, ref, _exact)


@functools.lru_cache(maxsize=None)
def _graph():
    """33 nodes, 3 nested slots; row 0 is a hub of 9 000 entries (two pieces of <= 8 192), rows 1.. have a handful.  Entries sorted by
    (row, slot, col); every node is some entry's column, so every row of a wide X is gathered."""
    rng = np.random.default_rng(7)
    K, rows = 3, []
    for r in range(N):
        m = 9000 if r == 0 else int(rng.integers(0, 7))
        slot = np.sort(rng.integers(0, K, m))
        col = rng.integers(0, N, m)
        if r == 0:
            col[:N] = np.arange(N)
        order = np.lexsort((col, slot))
        rows.append((slot[order], col[order], rng.integers(1, 9, m) * 0.25))
    row_ptr = np.concatenate([[0], np.cumsum([len(s) for s, _, _ in rows])]).astype(np.int32)
    slot = np.concatenate([s for s, _, _ in rows]).astype(np.uint8)
    col = np.concatenate([c for _, c, _ in rows]).astype(np.int32)
    val = np.concatenate([v for _, _, v in rows]).astype(np.float32)
    A = np.zeros((K, N, N))
    for r in range(N):
        lo, hi = row_ptr[r], row_ptr[r + 1]
        np.add.at(A, (slot[lo:hi], r, col[lo:hi]), val[lo:hi].astype(np.float64))
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return {"K": K, "row_ptr": dev(row_ptr), "col": dev(col), "val": dev(val), "slot": dev(slot), "A": torch.from_numpy(A),
            "long_rows": torch.tensor([0], dtype=torch.int32, device=DEV), "threshold": 64}


def _hub_ws(lib, g, slots, d):
    nbytes = int(lib.ctgcn_hub_workspace_bytes(1, 2, slots, d))
    assert nbytes > 0
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV), nbytes


def _agg_ref(g, x):
    """res_j = res_{j-1} + A_j x with res_{-1} = x (self loop) and A_j = the entries tagged <= j (nested); H[:, j] = relu(res_j), float64"""
    x64 = x.double().cpu()
    acc, cum, out = x64.clone(), torch.zeros_like(x64), []
    for j in range(g["K"]):
        cum = cum + g["A"][j] @ x64
        acc = acc + cum
        out.append(torch.relu(acc))
    return torch.stack(out, 1)


def _drive_core_aggregate(arena, param, layout):
    """tests/test_gpu_kernels.py::_agg_case: close_scaled at rtol 1e-5; hub row in two pieces + the fixed-order final pass"""
    from ctgcn_amd import _lib as L
    lib, g = _lib(), _graph()
    flags = L.F_SELF_LOOP | L.F_RELU | L.F_NESTED
    for d in _widths(layout):
        x = _ints(N, d, seed=3)
        ws, ws_bytes = _hub_ws(lib, g, g["K"], d)

        def call(t):
            _ck(lib.ctgcn_core_aggregate_f32(N, d, g["K"], _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(g["slot"]), _p(t["X"]), t["X"].stride(0),
                                             _p(t["H"]), flags, _p(g["long_rows"]), 1, g["threshold"], 2, _p(ws), ws_bytes, _stream()), "core_aggregate")

        ref = {"H": _agg_ref(g, x).reshape(N, g["K"] * d)}
        _run_case(arena, layout, "X", {"X": x}, {"H": (N, g["K"] * d)}, call, ref, _scaled())


def _decode_planes(ws, rows, d):
    """planes as ctgcn_core_aggregate_split_f32 / ctgcn_split_rows_f32 lay them out: fp16 plane 1 [rows, kp] | plane 2 | fp32 row scales"""
    kp = -(-d // 64) * 64
    half = ws[: rows * kp * 4].view(torch.float16).view(2, rows, kp)
    scale = ws[rows * kp * 4: rows * kp * 4 + rows * 4].view(torch.float32)
    return ((half[0].double() + half[1].double()) * scale.double()[:, None])[:, :d]


def _drive_core_aggregate_split(arena, param, layout):
    """the aggregation whose output leaves as fp16x2 planes + row scales (22 bits: inside close_scaled's rtol 1e-5 of the fp32 form)"""
    from ctgcn_amd import _lib as L
    lib, g = _lib(), _graph()
    flags, d, K = L.F_SELF_LOOP | L.F_RELU | L.F_NESTED, 128, _graph()["K"]
    x = _ints(N, d, seed=4)
    hub, hub_bytes = _hub_ws(lib, g, K, d)
    nbytes = int(lib.ctgcn_core_aggregate_split_workspace_bytes(N, d, K, 1, 1))

    def call(t):
        _ck(lib.ctgcn_core_aggregate_split_f32(N, d, K, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(g["slot"]), _p(t["X"]), t["X"].stride(0), flags,
                                               _p(g["long_rows"]), 1, g["threshold"], 1, None, None, None, 0, None, 2, _p(hub), hub_bytes,
                                               _p(t["ws"]), nbytes, _stream()), "core_aggregate_split")

    def compare(name, got, ref64):
        close_scaled(_decode_planes(got, N * K, d).cpu().numpy(), ref64.numpy())

    _run_case(arena, layout, "X", {"X": x}, {"ws": torch.zeros(nbytes, dtype=torch.uint8, device=DEV)}, call,
              {"ws": _agg_ref(g, x).reshape(N * K, d)}, compare)


def _drive_core_aggregate_bwd(arena, param, layout):
    """tests/test_gpu_kernels.py::_agg_case backward: close_scaled(rtol 2e-5, atol_scale 4e-6)"""
    from ctgcn_amd import _lib as L
    lib, g = _lib(), _graph()
    flags, K = L.F_SELF_LOOP | L.F_NESTED, _graph()["K"]
    for d in _widths(layout):
        Z, S0 = _rand(N, K, d, seed=5), _rand(N, d, seed=6)
        ws, ws_bytes = _hub_ws(lib, g, 1, d)

        def call(t):
            _ck(lib.ctgcn_core_aggregate_bwd_f32(N, d, K, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(g["slot"]), _p(Z), _p(S0), _p(t["dX"]),
                                                 t["dX"].stride(0), flags, _p(g["long_rows"]), 1, g["threshold"], 2, _p(ws), ws_bytes, _stream()),
                "core_aggregate_bwd")

        ref = S0.double().cpu() + sum(g["A"][j] @ Z[:, j].double().cpu() for j in range(K))
        _run_case(arena, layout, "dX", {}, {"dX": (N, d)}, call, {"dX": ref}, _scaled(2e-5, 4e-6))


def _drive_spmm(arena, param, layout):
    """tests/test_gpu_kernels.py::test_spmm_csr_matches_torch_sparse_and_accumulates: close_scaled defaults; Y += A X reads Y too"""
    from ctgcn_amd import ops
    g = _graph()
    A = g["A"].sum(0)
    for d in _widths(layout):
        x, y0 = _ints(N, d, seed=7), _ints(N, d, seed=8)

        def call(t):
            ops.spmm_csr(g["row_ptr"], g["col"], g["val"], t["X"], out=t["Y"], accumulate=True)

        ref = {"Y": y0.double().cpu() + A @ x.double().cpu()}
        _run_case(arena, layout, "X" if param == "ldx" else "Y", {"X": x}, {"Y": y0}, call, ref, _scaled())


# ------------------------------------------------------------------------------------------------------------ GRU path
def _gru_ref64(gi, w_hh, b_hn):
    """h sequence [rows, steps, 128] of the recurrence on gate pre-activations gi [rows, steps, 384] (order r, z, n), float64"""
    gi, w, b = gi.double().cpu(), w_hh.double().cpu(), b_hn.double().cpu()
    h = torch.zeros(gi.shape[0], 128, dtype=torch.float64)
    out = []
    for t in range(gi.shape[1]):
        gh = h @ w.t()
        r = torch.sigmoid(gi[:, t, :128] + gh[:, :128])
        z = torch.sigmoid(gi[:, t, 128:256] + gh[:, 128:256])
        n = torch.tanh(gi[:, t, 256:] + r * (gh[:, 256:] + b))
        h = (1 - z) * n + z * h
        out.append(h)
    return torch.stack(out, 1)


def _ln64(x, gamma, beta, eps=1e-5):
    return torch.nn.functional.layer_norm(x, (128,), gamma.double().cpu(), beta.double().cpu(), eps)


def _gru_params(seed):
    s = 1.0 / np.sqrt(128)
    return {"w_ih": _rand(384, 128, seed=seed, scale=s), "w_hh": _rand(384, 128, seed=seed + 1, scale=s), "bias_gi": _rand(384, seed=seed + 2, scale=0.1),
            "b_hn": _rand(128, seed=seed + 3, scale=0.1), "gamma": _rand(128, seed=seed + 4, scale=0.3) + 1.0, "beta": _rand(128, seed=seed + 5, scale=0.2)}


def _gru_close(name, got, ref64):
    """tests/test_gpu_gru.py::test_fused_gru_matches_torch: rtol 1e-4, atol 1e-5"""
    check_close(got.cpu().numpy(), ref64.numpy(), 1e-4, 1e-5, what="wide " + name)


def _drive_gru_seq(arena, param, layout):
    lib, p, steps = _lib(), _gru_params(10), 3
    gi = _rand(N, steps, 384, seed=11)
    ref = {"out": _ln64(_gru_ref64(gi, p["w_hh"], p["b_hn"]).sum(1), p["gamma"], p["beta"])}
    for mode in (0, 1, 2):                                   # fp32 MFMA, bf16x3 and fp16x2 recurrence kernels

        def call(t):
            _ck(lib.ctgcn_gru_seq_f32(N, steps, 128, _p(gi), _p(p["w_hh"]), _p(p["b_hn"]), _p(p["gamma"]), _p(p["beta"]), 1e-5, 1, _p(t["out"]),
                                      t["out"].stride(0), None, mode, 0, None, None, None, _stream()), "gru_seq")

        _run_case(arena, layout, "out", {}, {"out": (N, 128)}, call, ref, _gru_close)


def _drive_gru_layer(arena, param, layout):
    lib, p = _lib(), _gru_params(20)
    ld = W.LAYOUTS[layout][1]

    def gi_of(x):
        return x.double().cpu() @ p["w_ih"].double().cpu().t() + p["bias_gi"].double().cpu()

    def layer(rows, steps, x, ldx, reduce_sum, out, ld_out, offs=None, ld_row=0):
        _ck(lib.ctgcn_gru_layer_f32(rows, steps, 128, 128, _p(x), ldx, _p(p["w_ih"]), _p(p["w_hh"]), _p(p["bias_gi"]), _p(p["b_hn"]), _p(p["gamma"]),
                                    _p(p["beta"]), 1e-5, 1 if reduce_sum else 0, _p(out), ld_out, None, _p(offs), ld_row, _stream()), "gru_layer")

    if param == "ldx":                                       # x [rows, steps, 128] as 33 row-steps, ldx floats apart
        for rows, steps in ((N, 1), (11, 3)):
            x = _rand(rows * steps, 128, seed=21)
            hs = _gru_ref64(gi_of(x).view(rows, steps, 384), p["w_hh"], p["b_hn"])
            for reduce_sum in (True, False):
                ref = {"out": _ln64(hs.sum(1), p["gamma"], p["beta"]) if reduce_sum else _ln64(hs, p["gamma"], p["beta"]).reshape(rows, steps * 128)}

                def call(t):
                    layer(rows, steps, t["x"], t["x"].stride(0), reduce_sum, t["out"], 0)

                _run_case(arena, layout, "x", {"x": x}, {"out": (rows, 128 if reduce_sum else steps * 128)}, call, ref, _gru_close)
    elif param == "ld_out":
        steps = 3
        x = _rand(N * steps, 128, seed=22)
        ref = {"out": _ln64(_gru_ref64(gi_of(x).view(N, steps, 384), p["w_hh"], p["b_hn"]).sum(1), p["gamma"], p["beta"])}

        def call(t):
            layer(N, steps, x, 128, True, t["out"], t["out"].stride(0))

        _run_case(arena, layout, "out", {}, {"out": (N, 128)}, call, ref, _gru_close)
    elif param == "ld_row":                                  # step t of sequence r at base + r ld_row + step_offsets[t]: rows 2^27 apart
        steps = 3
        x = _rand(N, steps * 160, seed=23)                   # step t in columns [160 t, 160 t + 128)
        xs = x.view(N, steps, 160)[:, :, :128]
        ref = {"out": _ln64(_gru_ref64(gi_of(xs.reshape(N * steps, 128)).view(N, steps, 384), p["w_hh"], p["b_hn"]), p["gamma"], p["beta"]).reshape(N, steps * 128)}
        offs = torch.tensor([160 * t for t in range(steps)], dtype=torch.int64, device=DEV)

        def call(t):
            layer(N, steps, t["x"], 128, False, t["out"], 0, offs, t["x"].stride(0))

        _run_case(arena, layout, "x", {"x": x}, {"out": (N, steps * 128)}, call, ref, _gru_close)
    else:                                                    # step_offsets: the steps of a sequence 2^31 and 2^32 floats apart, rows dense
        rows, steps, at = 8, 3, (0, 16, 32)
        x = _rand(N, rows * 128, seed=24)                    # wide row `at[t]` holds step t of all 8 sequences
        xs = torch.stack([x[a].view(rows, 128) for a in at], 1)
        ref = {"out": _ln64(_gru_ref64(gi_of(xs.reshape(rows * steps, 128)).view(rows, steps, 384), p["w_hh"], p["b_hn"]), p["gamma"], p["beta"]).reshape(rows, steps * 128)}

        def call(t):
            offs = torch.tensor([a * t["x"].stride(0) for a in at], dtype=torch.int64, device=DEV)
            layer(rows, steps, t["x"], 128, False, t["out"], 0, offs, 128)

        _run_case(arena, layout, "x", {"x": x}, {"out": (rows, steps * 128)}, call, ref, _gru_close)


def _drive_gru_layer_presplit(arena, param, layout):
    """the layer kernel on fp16x2 planes + row scales (the layout ctgcn_core_aggregate_split_f32 and ctgcn_split_rows_f32 share), out rows wide"""
    lib, p, steps = _lib(), _gru_params(25), 3
    x = _rand(N * steps, 128, seed=26)
    nbytes = int(lib.ctgcn_core_aggregate_split_workspace_bytes(N, 128, steps, 1, 0))          # whole tiles: the kernel stages 16 sequences at a time
    planes = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _ck(lib.ctgcn_split_rows_f32(N * steps, 128, _p(x), 128, _p(planes), nbytes, _stream()), "split_rows")
    gi = x.double().cpu() @ p["w_ih"].double().cpu().t() + p["bias_gi"].double().cpu()
    ref = {"out": _ln64(_gru_ref64(gi.view(N, steps, 384), p["w_hh"], p["b_hn"]).sum(1), p["gamma"], p["beta"])}

    def call(t):
        _ck(lib.ctgcn_gru_layer_presplit_f32(N, steps, 128, _p(planes), _p(p["w_ih"]), _p(p["w_hh"]), _p(p["bias_gi"]), _p(p["b_hn"]), _p(p["gamma"]), _p(p["beta"]),
                                             1e-5, _p(t["out"]), t["out"].stride(0), None, None, _stream()), "gru_layer_presplit")

    _run_case(arena, layout, "out", {}, {"out": (N, 128)}, call, ref, _gru_close)


def _drive_layernorm_bwd(arena, param, layout):
    """tests/test_gpu_gru.py::test_layernorm_backward_kernel_matches_autograd and its three bounds"""
    lib, steps = _lib(), 3
    h, dy, gamma = _rand(N, steps, 128, seed=30, scale=0.7), _rand(N, 128, seed=31), _rand(128, seed=32)
    x64 = h.double().cpu().sum(1).requires_grad_(True)
    g64, b64 = gamma.double().cpu().requires_grad_(True), torch.zeros(128, dtype=torch.float64, requires_grad=True)
    torch.nn.functional.layer_norm(x64, (128,), g64, b64, 1e-5).backward(dy.double().cpu())

    def call(t):
        _ck(lib.ctgcn_layernorm_bwd_f32(N, steps, 128, _p(h), _p(t["dy"]), t["dy"].stride(0), _p(gamma), 1e-5, _p(t["dx"]), _p(t["part"]), 40, None, _stream()),
            "layernorm_bwd")

    def compare(name, got, ref64):
        if name == "dx":
            assert (got.double().cpu() - ref64).abs().max().item() <= 2e-5 * ref64.abs().max().item() + 1e-6
        else:
            sums = got.double().cpu().sum(0)
            assert (sums[:128] - g64.grad).abs().max().item() <= 1e-5 * g64.grad.abs().max().item() + 1e-5
            assert (sums[128:] - b64.grad).abs().max().item() <= 1e-5 * b64.grad.abs().max().item() + 1e-5

    _run_case(arena, layout, "dy", {"dy": dy}, {"dx": (N, 128), "part": (40, 256)}, call, {"dx": x64.grad, "part": None}, compare)


def _split_close(x, w):
    """tests/test_gpu_gru.py::test_split_bf16_projection_is_fp32_accurate: no worse than twice a plain fp32 GEMM's error, or 2e-7 of the scale"""
    def compare(name, got, ref64):
        err_split = (got.double().cpu() - ref64).abs().max().item()
        err_fp32 = ((x.cpu() @ w.cpu()).double() - ref64).abs().max().item()
        assert err_split <= max(2.0 * err_fp32, 2e-7 * ref64.abs().max().item()), (name, err_split, err_fp32)
    return compare


def _drive_gru_input_proj(arena, param, layout, monkeypatch):
    from ctgcn_amd import ops
    x = torch.relu(_rand(N, 128, seed=40)) * 4.0
    w = (torch.rand(384, 128, generator=torch.Generator().manual_seed(41)) - 0.5).to(DEV) * 0.18
    ref = {"gi": x.double().cpu() @ w.double().cpu().t()}
    for mode in ("f16x2", "bf16x3"):
        monkeypatch.setenv("CTGCN_GRU_SPLIT", mode)
        monkeypatch.setenv("CTGCN_FP32_MFMA_ONLY", "0")
        assert ops.forward_split_mode() == (2 if mode == "f16x2" else 1)

        def call(t):
            assert ops._project(t["x"], w, None, t["gi"]) is False

        _run_case(arena, layout, "x", {"x": x}, {"gi": (N, 384)}, call, ref, _split_close(x, w.t()))


def _drive_gru_input_grad(arena, param, layout):
    """tests/test_gpu_gru.py::test_split_bf16_input_gradient_is_fp32_accurate"""
    from ctgcn_amd import ops
    g = _rand(N, 384, seed=42) * torch.rand(N, 1, generator=torch.Generator().manual_seed(43)).to(DEV) * 3.0
    w = (torch.rand(384, 128, generator=torch.Generator().manual_seed(44)) - 0.5).to(DEV) * 0.18
    assert ops.split_mfma_enabled()

    def call(t):
        ops._project_grad(g, w, t["dx"])

    _run_case(arena, layout, "dx", {}, {"dx": (N, 128)}, call, {"dx": g.double().cpu() @ w.double().cpu()}, _split_close(g, w))


GRU_BWD_IN_CASE = dict(rows=11, steps=3, mask_bits=[0b101], seed=90)      # audited by tests/test_gru_bwd_ref_host.py


def _drive_gru_bwd_in(arena, param, layout):
    """tests/test_gpu_gru_bwd_direct.py's exact tier: 11 sequences of 3 steps = 33 row-steps of fp32 x, one per wide row, under a row plan;
    d_gi and x are NaN at the steps that are not fresh, dx keeps its prefill there.  Bit for bit the float64 model."""
    import _gru_bwd_ref as M
    lib = _lib()
    rows, steps, bits = GRU_BWD_IN_CASE["rows"], GRU_BWD_IN_CASE["steps"], GRU_BWD_IN_CASE["mask_bits"]
    assert rows * steps == N
    t, want = M.exact_case(audit=False, **GRU_BWD_IN_CASE)
    fresh = M.fresh_matrix(bits, rows, steps)
    x = torch.from_numpy(np.where(fresh[:, :, None], t["x"], np.nan).reshape(N, 128)).float().to(DEV)
    dgi, w_ih = torch.from_numpy(want["d_gi"]).float().to(DEV), torch.from_numpy(t["w_ih"]).float().to(DEV)
    tm = torch.from_numpy(M.pack_masks(bits, steps).view(np.int32)).to(DEV)
    assert lib.ctgcn_gru_bwd_blocks(rows) == 1

    def call(v):
        _ck(lib.ctgcn_gru_bwd_in_f32(rows, steps, 128, _p(dgi), _p(w_ih), _p(tm), None, 0, 0, _p(v["x"]), v["x"].stride(0), _p(v["dx"]), None, None,
                                     None, 0, _p(v["dw"]), _p(v["dbi"]), 1, 0, _stream()), "ctgcn_gru_bwd_in_f32")

    ref = {"dx": torch.from_numpy(np.nan_to_num(want["dx"], nan=W.SENTINEL).reshape(N, 128)), "dw": torch.from_numpy(want["dW_ih"]),
           "dbi": torch.from_numpy(want["db_ih"][None])}
    _run_case(arena, layout, "x", {"x": x}, {"dx": (N, 128), "dw": (384, 128), "dbi": (1, 384)}, call, ref, _exact)


# ------------------------------------------------------------------------------------------------------- the split GEMM
def _gemm_close(x, w, b):
    """tests/test_gpu_gemm.py: error over sum |x_k w_k| no worse than twice the fp32 library GEMM's, or 2e-7"""
    def compare(name, got, ref64):
        scale = (x.double().abs() @ w.double().abs().t()).cpu() + 1e-30
        err_split = ((got.double().cpu() - ref64).abs() / scale).max().item()
        err_lib = ((torch.addmm(b, x, w.t()).double().cpu() - ref64).abs() / scale).max().item()
        assert err_split <= max(2 * err_lib, 2e-7), (name, err_split, err_lib)
    return compare


def _gemm_operands(param, k):
    rows, n_out = (N, 24) if param != "ldw" else (40, N)                 # the wide operand has 33 rows
    x, w, b = _rand(rows, k, seed=50), _rand(n_out, k, seed=51, scale=0.1), _rand(n_out, seed=52, scale=0.1)
    return rows, n_out, x, w, b, {"y": x.double().cpu() @ w.double().cpu().t() + b.double().cpu()}


def _drive_linear(arena, param, layout):
    lib = _lib()
    for k in _widths(layout):
        rows, n_out, x, w, b, ref = _gemm_operands(param, k)
        nbytes = int(lib.ctgcn_linear_workspace_bytes(rows, n_out, k))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

        def call(t):
            _ck(lib.ctgcn_linear_f32(rows, n_out, k, _p(t["x"]), t["x"].stride(0), _p(t["w"]), t["w"].stride(0), _p(b), 0, _p(t["y"]), t["y"].stride(0),
                                     _p(ws), nbytes, _stream()), "linear")

        _run_case(arena, layout, {"ldx": "x", "ldw": "w", "ldy": "y"}[param], {"x": x, "w": w}, {"y": (rows, n_out)}, call, ref, _gemm_close(x, w, b))


def _drive_packed(fn):
    """ctgcn_split_rows_f32 -> ctgcn_pack_weight_f32 -> ctgcn_linear_packed_f32, one of the three with its strided operand wide"""
    def drive(arena, param, layout):
        lib = _lib()
        for k in _widths(layout):
            rows, n_out, x, w, b, ref = _gemm_operands(param, k)
            pb, wb = int(lib.ctgcn_split_planes_bytes(rows, k)), int(lib.ctgcn_pack_weight_bytes(n_out, k))
            planes, packed = torch.empty(pb, dtype=torch.uint8, device=DEV), torch.empty(wb, dtype=torch.uint8, device=DEV)

            def call(t):
                _ck(lib.ctgcn_split_rows_f32(rows, k, _p(t["x"]), t["x"].stride(0), _p(planes), pb, _stream()), "split_rows")
                _ck(lib.ctgcn_pack_weight_f32(n_out, k, _p(t["w"]), t["w"].stride(0), _p(packed), wb, _stream()), "pack_weight")
                _ck(lib.ctgcn_linear_packed_f32(rows, n_out, k, _p(planes), _p(packed), _p(b), 0, _p(t["y"]), t["y"].stride(0), _stream()), "linear_packed")

            _run_case(arena, layout, {"ldx": "x", "ldw": "w", "ldy": "y"}[param], {"x": x, "w": w}, {"y": (rows, n_out)}, call, ref, _gemm_close(x, w, b))
    return drive


def _drive_linear_presplit(arena, param, layout):
    """the GEMM on the planes ctgcn_core_aggregate_split_f32 wrote into the shared workspace: y = H w^T + b (one slot: 33 operand rows)"""
    from ctgcn_amd import _lib as L
    lib, g = _lib(), _graph()
    flags, d = L.F_SELF_LOOP | L.F_RELU | L.F_NESTED, 64
    n_out = N if param == "ldw" else 24
    x, w, b = _ints(N, d, seed=60), _rand(n_out, d, seed=61, scale=0.1), _rand(n_out, seed=62, scale=0.1)
    H = torch.relu(x.double().cpu() + g["A"].sum(0) @ x.double().cpu())          # K = 1 without slot tags: every entry belongs to the one matrix
    nbytes = int(lib.ctgcn_core_aggregate_split_workspace_bytes(N, d, 1, n_out, 0))
    ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    _ck(lib.ctgcn_core_aggregate_split_f32(N, d, 1, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), None, _p(x), d, flags, None, 0, 0, n_out,
                                           None, None, None, 0, None, 1, None, 0, _p(ws), nbytes, _stream()), "core_aggregate_split")

    def call(t):
        _ck(lib.ctgcn_linear_presplit_f32(N, n_out, d, _p(t["w"]), t["w"].stride(0), _p(b), _p(t["y"]), t["y"].stride(0), _p(ws), nbytes, _stream()),
            "linear_presplit")

    ref = {"y": H @ w.double().cpu().t() + b.double().cpu()}
    _run_case(arena, layout, "w" if param == "ldw" else "y", {"w": w}, {"y": (N, n_out)}, call, ref, _gemm_close(H.float().to(DEV), w, b))


# ------------------------------------------------------------------------------------------------- the gather family
def _csr():
    """the graph above as one matrix (slot tags dropped): row 0 is the long row of every gather kernel (threshold 64: 36 pieces)"""
    g = _graph()
    return g, g["A"].sum(0)


def _long(g, d, item=4):
    pieces = -(-9000 // (4 * g["threshold"]))
    nbytes = pieces * (-(-d // 4) * 4) * item
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    return (_p(g["long_rows"]), 1, g["threshold"], _p(ws), nbytes), ws


def _pick(param, names):
    """the operand a stride parameter belongs to"""
    return names[param]


def _f64(t):
    return t.double().cpu()


def _drive_gcn_layer_fwd(arena, param, layout):
    """tests/test_gpu_gcn_layer.py: close_scaled; eval-mode RReLU (slope 11/48)"""
    lib = _lib()
    g, A = _csr()
    for d in _widths(layout):
        S = _ints(N, d, seed=80)
        long, _ws = _long(g, d)

        def call(t):
            _ck(lib.ctgcn_gcn_layer_fwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["S"]), t["S"].stride(0), _p(t["Y"]), t["Y"].stride(0), 1,
                                            None, None, *long, _stream()), "gcn_layer_fwd")

        y = A @ _f64(S)
        _run_case(arena, layout, _pick(param, {"lds": "S", "ldy": "Y"}), {"S": S}, {"Y": (N, d)}, call, {"Y": torch.where(y >= 0, y, y * 11 / 48)}, _scaled())


def _drive_gcn_layer_bwd(arena, param, layout):
    lib = _lib()
    g, A = _csr()
    for d in _widths(layout):
        dY, Y = _ints(N, d, seed=81), _ints(N, d, seed=82) * 48.0            # dY * 11/48 of multiples of 48: exact
        dY = dY * 48.0
        long, _ws = _long(g, d)

        def call(t):
            _ck(lib.ctgcn_gcn_layer_bwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["dY"]), t["dY"].stride(0), _p(t["Y"]), t["Y"].stride(0), 1,
                                            _p(t["dS"]), t["dS"].stride(0), *long, _stream()), "gcn_layer_bwd")

        ref = A @ (_f64(dY) * torch.where(_f64(Y) > 0, 1.0, 11 / 48))
        _run_case(arena, layout, _pick(param, {"lddy": "dY", "ldy": "Y", "ldds": "dS"}), {"dY": dY, "Y": Y}, {"dS": (N, d)}, call, {"dS": ref}, _scaled())


def _conv_fwd(kind):
    """Y = relu(A S [+ self_scale T] + bias): ctgcn_gcn_conv_fwd_f32 / ctgcn_tg_conv_fwd_f32 (epi 1, no dropout); tests/test_gpu_gcn_conv.py,
    tests/test_gpu_tg_ops.py: close_scaled"""
    def drive(arena, param, layout):
        lib = _lib()
        g, A = _csr()
        for d in _widths(layout):
            S, T, bias = _ints(N, d, seed=83), _ints(N, d, seed=84), _ints(d, seed=85)
            long, _ws = _long(g, d)

            def call(t):
                if kind == "gcn":
                    _ck(lib.ctgcn_gcn_conv_fwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["S"]), t["S"].stride(0), _p(bias), _p(t["Y"]),
                                                   t["Y"].stride(0), 1, 0.0, 0, None, *long, _stream()), "gcn_conv_fwd")
                else:
                    _ck(lib.ctgcn_tg_conv_fwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["S"]), t["S"].stride(0), _p(t["T"]), t["T"].stride(0),
                                                  0.5, _p(bias), _p(t["Y"]), t["Y"].stride(0), 1, 0.0, 0, *long, _stream()), "tg_conv_fwd")

            ref = A @ _f64(S) + _f64(bias) + (0.5 * _f64(T) if kind == "tg" else 0.0)
            _run_case(arena, layout, _pick(param, {"lds": "S", "ldt": "T", "ldy": "Y"}), {"S": S, "T": T}, {"Y": (N, d)}, call, {"Y": torch.relu(ref)}, _scaled())
    return drive


def _conv_prep(kind):
    """the backward's N x d pass of the ReLU epilogue, with the bias gradient: G = dY where the forward's output was positive"""
    def drive(arena, param, layout):
        lib = _lib()
        for d in _widths(layout):
            dY, Y, bias = _rand(N, d, seed=86), _rand(N, d, seed=87), _rand(d, seed=88)
            nbytes = int((lib.ctgcn_gcn_conv_prep_workspace_bytes if kind == "gcn" else lib.ctgcn_tg_prep_workspace_bytes)(N, d))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

            def call(t):
                if kind == "gcn":
                    _ck(lib.ctgcn_gcn_conv_prep_f32(N, d, _p(t["dY"]), t["dY"].stride(0), _p(t["Y"]), t["Y"].stride(0), None, 1, 0.0, _p(t["G"]), t["G"].stride(0),
                                                    _p(t["db"]), _p(ws), nbytes, _stream()), "gcn_conv_prep")
                else:
                    _ck(lib.ctgcn_tg_conv_prep_f32(N, d, _p(t["dY"]), t["dY"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(bias), 1, 0.0, 0, _p(t["G"]),
                                                   t["G"].stride(0), _p(t["db"]), _p(ws), nbytes, _stream()), "tg_conv_prep")

            G = torch.where(_f64(Y) + (_f64(bias) if kind == "tg" else 0.0) > 0, _f64(dY), 0.0)
            _run_case(arena, layout, _pick(param, {"lddy": "dY", "ldy": "Y", "ldg": "G"}), {"dY": dY, "Y": Y}, {"G": (N, d), "db": (1, d)}, call,
                      {"G": G, "db": G.sum(0, keepdim=True)}, _scaled())
    return drive


def _drive_pool_conv_fwd(arena, param, layout):
    """tests/test_gpu_pool_conv.py: close_scaled.  ReLU, the row's L2 normalisation, dropout: with p > 0 Ysave receives the normalised rows"""
    import _gcrn_ref as R
    lib = _lib()
    g, A = _csr()
    p, key = (0.25, 2 ** 60 + 99) if param == "ldsave" else (0.0, 0)
    for d in _widths(layout):
        S, T, bias = _ints(N, d, seed=89), _ints(N, d, seed=90), _ints(d, seed=91)
        long, _ws = _long(g, d)

        def call(t):
            _ck(lib.ctgcn_pool_conv_fwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["S"]), t["S"].stride(0), _p(t["T"]), t["T"].stride(0), 0.5,
                                            _p(bias), _p(t["Y"]), t["Y"].stride(0), 1, p, key, _p(t["norm"]), _p(t["save"]) if p else None,
                                            t["save"].stride(0) if p else 0, *long, _stream()), "pool_conv_fwd")

        x = torch.relu(A @ _f64(S) + 0.5 * _f64(T) + _f64(bias))
        norm = x.norm(dim=1, keepdim=True)
        rows = x / norm.clamp_min(1e-12)
        ref = {"norm": norm.t(), "Y": rows}
        outs = {"Y": (N, d), "norm": (1, N)}
        if p:
            keep = torch.from_numpy(np.asarray(R.keep_mask(key, N, d, p))).double()
            ref = {"norm": norm.t(), "save": rows, "Y": rows * keep / (1.0 - p)}
            outs["save"] = (N, d)
        _run_case(arena, layout, _pick(param, {"lds": "S", "ldt": "T", "ldy": "Y", "ldsave": "save"}), {"S": S, "T": T}, outs, call, ref, _scaled())


def _drive_pool_conv_prep(arena, param, layout):
    lib = _lib()
    for d in _widths(layout):
        dY = _rand(N, d, seed=92)
        x = torch.relu(_rand(N, d, seed=93))
        norm = x.norm(dim=1)
        Y = x / norm[:, None]
        nbytes = int(lib.ctgcn_pool_prep_workspace_bytes(N, d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

        def call(t):
            _ck(lib.ctgcn_pool_conv_prep_f32(N, d, _p(t["dY"]), t["dY"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(norm), 0.0, 0, _p(t["G"]), t["G"].stride(0),
                                             _p(t["db"]), _p(ws), nbytes, _stream()), "pool_conv_prep")

        y64, g64 = _f64(Y), _f64(dY)
        G = torch.where(y64 > 0, (g64 - y64 * (y64 * g64).sum(1, keepdim=True)) / _f64(norm)[:, None], 0.0)
        _run_case(arena, layout, _pick(param, {"lddy": "dY", "ldy": "Y", "ldg": "G"}), {"dY": dY, "Y": Y}, {"G": (N, d), "db": (1, d)}, call,
                  {"G": G, "db": G.sum(0, keepdim=True)}, _scaled())


def _drive_pool_max_fwd(arena, param, layout):
    """tests/test_gpu_pool_max.py: the maximum and its (lowest) column exactly"""
    lib = _lib()
    g, _A = _csr()
    rp, col = g["row_ptr"].cpu().numpy(), g["col"].cpu().numpy()
    for d in _widths(layout):
        S = _rand(N, d, seed=94)
        long, _ws = _long(g, d, item=8)
        s64 = S.cpu().numpy().astype(np.float64)
        Y, arg = np.zeros((N, d)), np.full((N, d), -1, np.int32)
        for r in range(N):
            cols = np.unique(col[rp[r]:rp[r + 1]])
            if len(cols):
                best = s64[cols].argmax(0)                        # first maximum: the lowest column among equal values
                arg[r], Y[r] = cols[best], s64[cols[best], np.arange(d)]

        def call(t):
            _ck(lib.ctgcn_pool_max_fwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(t["S"]), t["S"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(t["arg"]),
                                           t["arg"].stride(0), *long, _stream()), "pool_max_fwd")

        def compare(name, got, ref64):
            assert torch.equal(got.cpu().double(), ref64), name

        _run_case(arena, layout, _pick(param, {"lds": "S", "ldy": "Y", "ldarg": "arg"}), {"S": S},
                  {"Y": (N, d), "arg": torch.full((N, d), -7, dtype=torch.int32, device=DEV)}, call,
                  {"Y": torch.from_numpy(Y), "arg": torch.from_numpy(arg).double()}, compare)


def _drive_pool_max_bwd(arena, param, layout):
    lib = _lib()
    g, _A = _csr()
    rp, col = g["row_ptr"].cpu().numpy(), g["col"].cpu().numpy()
    for d in _widths(layout):
        dY = _ints(N, d, seed=95)
        arg = torch.randint(0, N, (N, d), generator=torch.Generator().manual_seed(96), dtype=torch.int32).to(DEV)
        long, _ws = _long(g, d)
        a, gy = arg.cpu().numpy(), dY.cpu().numpy().astype(np.float64)
        ref = np.zeros((N, d))
        for j in range(N):
            i = col[rp[j]:rp[j + 1]]
            ref[j] = ((a[i] == j) * gy[i]).sum(0)

        def call(t):
            _ck(lib.ctgcn_pool_max_bwd_f32(N, d, _p(g["row_ptr"]), _p(g["col"]), _p(t["dY"]), t["dY"].stride(0), _p(t["arg"]), t["arg"].stride(0), _p(t["dS"]),
                                           t["dS"].stride(0), *long, _stream()), "pool_max_bwd")

        _run_case(arena, layout, _pick(param, {"lddy": "dY", "ldarg": "arg", "ldds": "dS"}), {"dY": dY, "arg": arg}, {"dS": (N, d)}, call,
                  {"dS": torch.from_numpy(ref)}, _scaled())


def _bn_inputs(d):
    x = _rand(N, d, seed=97) * torch.linspace(0.5, 3.0, d, device=DEV) + torch.linspace(-2.0, 2.0, d, device=DEV)
    w = _rand(d, seed=98) + 1.5 * torch.sign(_rand(d, seed=99))
    return x, w, _rand(d, seed=100), _rand(N, d, seed=101)


def _bn_used(terms=0.0):
    """tests/test_gpu_batch_norm_act.py::used: close_scaled's tolerance, its absolute part also covering the terms that cancel in dx"""
    def compare(name, got, ref64):
        got, ref = got.double().cpu().numpy(), ref64.numpy()
        tol = 1e-5 * np.abs(ref) + 2e-6 * max(1.0, float(np.abs(ref).max(initial=0.0)), terms if name == "dx" else 0.0)
        assert (np.abs(got - ref) <= tol).all(), (name, float((np.abs(got - ref) / tol).max()))
    return compare


def _drive_bn_stats(arena, param, layout):
    lib = _lib()
    for d in _widths(layout):
        x = _bn_inputs(d)[0]
        nbytes = int(lib.ctgcn_bn_stats_workspace_bytes(N, d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

        def call(t):
            _ck(lib.ctgcn_bn_stats_f32(N, d, _p(t["x"]), t["x"].stride(0), 1e-5, _p(t["mean"]), _p(t["var"]), _p(t["rstd"]), _p(ws), nbytes, _stream()), "bn_stats")

        x64 = _f64(x)
        var = x64.var(0, unbiased=False, keepdim=True)
        _run_case(arena, layout, "x", {"x": x}, {"mean": (1, d), "var": (1, d), "rstd": (1, d)}, call,
                  {"mean": x64.mean(0, keepdim=True), "var": var, "rstd": (var + 1e-5).rsqrt()}, _bn_used())


def _drive_bn_apply(arena, param, layout):
    lib = _lib()
    for d in _widths(layout):
        x, w, b, _ = _bn_inputs(d)
        mean, rstd = x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()

        def call(t):
            _ck(lib.ctgcn_bn_apply_f32(N, d, _p(t["x"]), t["x"].stride(0), _p(mean), _p(rstd), _p(w), _p(b), 1, 0.0, 0, _p(t["y"]), t["y"].stride(0), _stream()), "bn_apply")

        ref = torch.relu((_f64(x) - _f64(mean)) * _f64(rstd) * _f64(w) + _f64(b))
        _run_case(arena, layout, _pick(param, {"ldx": "x", "ldy": "y"}), {"x": x}, {"y": (N, d)}, call, {"y": ref}, _bn_used())


def _drive_bn_bwd(arena, param, layout):
    lib = _lib()
    for d in _widths(layout):
        x, w, b, dy = _bn_inputs(d)
        mean, rstd = x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()
        nbytes = int(lib.ctgcn_bn_bwd_workspace_bytes(N, d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

        def call(t):
            _ck(lib.ctgcn_bn_bwd_f32(N, d, _p(t["x"]), t["x"].stride(0), _p(t["dy"]), t["dy"].stride(0), _p(mean), _p(rstd), _p(w), _p(b), 1, 0.0, 0, 1,
                                     _p(t["dx"]), t["dx"].stride(0), _p(t["dw"]), _p(t["db"]), _p(ws), nbytes, _stream()), "bn_bwd")

        xh = (_f64(x) - _f64(mean)) * _f64(rstd)
        gy = torch.where(xh * _f64(w) + _f64(b) > 0, _f64(dy), 0.0)
        db, dw = gy.sum(0, keepdim=True), (gy * xh).sum(0, keepdim=True)
        dx = _f64(w) * _f64(rstd) * (gy - db / N - xh * dw / N)
        terms = float((_f64(w).abs() * _f64(rstd)).max() * _f64(dy).abs().max())
        _run_case(arena, layout, _pick(param, {"ldx": "x", "lddy": "dy", "lddx": "dx"}), {"x": x, "dy": dy}, {"dx": (N, d), "dw": (1, d), "db": (1, d)}, call,
                  {"dx": dx, "dw": dw, "db": db}, _bn_used(terms))


# ------------------------------------------------------------------------------------------- GRU / LSTM cell passes
def _cell_share(ref32, floor):
    """tests/test_gpu_gru_cell.py, tests/test_gpu_lstm_cell.py: error <= max(4 x yardstick, floor) max|ref|, the yardstick being the float32
    evaluation of the same dense definition; floor 2e-6 for outputs, 1e-5 for gradients"""
    import _dynrnn_ref as D

    def compare(name, got, ref64):
        assert D.dense_share("wide " + name, got.cpu(), ref64, ref32[name], floor) <= 1.0, name
    return compare


def _cell_case(arena, param, layout, names, ins, out_shapes, call, dense_def, floor, init=None):
    """dense_def(tensors) -> {output: tensor} evaluates the step's definition in the dtype of its inputs"""
    ref64 = dense_def({k: v.double().cpu() for k, v in ins.items()})
    ref32 = dense_def({k: v.float().cpu() for k, v in ins.items()})
    outs = {k: (init[k] if init and k in init else shape) for k, shape in out_shapes.items()}
    _run_case(arena, layout, names[param], ins, outs, call, ref64, _cell_share(ref32, floor))


def _drive_gru_cell_fwd(arena, param, layout):
    import _gru_ref as G
    lib = _lib()
    for H in _widths(layout):
        ins = {"gi": _rand(N, 3 * H, seed=110), "gh": _rand(N, 3 * H, seed=111), "hp": _rand(N, H, seed=112), "b": _rand(3 * H, seed=113, scale=0.1)}
        acc0 = _rand(N, H, seed=114)

        def call(t):
            _ck(lib.ctgcn_gru_cell_fwd_f32(N, H, _p(t["gi"]), t["gi"].stride(0), _p(t["gh"]), t["gh"].stride(0), _p(t["b"]), _p(t["hp"]), t["hp"].stride(0),
                                           _p(t["h"]), t["h"].stride(0), _p(t["gates"]), t["gates"].stride(0), _p(t["q"]), t["q"].stride(0), _p(t["acc"]),
                                           t["acc"].stride(0), 0, _stream()), "gru_cell_fwd")

        def dense_def(t):
            h, gates, q = G.cell_fwd(t["gi"], t["gh"], t["b"], t["hp"])
            return {"h": h, "gates": gates, "q": q, "acc": acc0.cpu().to(h.dtype) + h}

        _cell_case(arena, param, layout, {"ldgi": "gi", "ldgh": "gh", "ldhp": "hp", "ldh": "h", "ldg": "gates", "ldq": "q", "ldacc": "acc"}, ins,
                   {"h": (N, H), "gates": (N, 3 * H), "q": (N, H), "acc": (N, H)}, call, dense_def, 2e-6, init={"acc": acc0})


def _drive_gru_cell_bwd(arena, param, layout):
    import _gru_ref as G
    lib = _lib()
    for H in _widths(layout):
        ins = {"gates": torch.sigmoid(_rand(N, 3 * H, seed=120)), "q": _rand(N, H, seed=121), "hp": _rand(N, H, seed=122), "do": _rand(N, H, seed=123),
               "dr": _rand(N, H, seed=124)}

        def call(t):
            _ck(lib.ctgcn_gru_cell_bwd_f32(N, H, _p(t["gates"]), t["gates"].stride(0), _p(t["q"]), t["q"].stride(0), _p(t["hp"]), t["hp"].stride(0),
                                           _p(t["do"]), t["do"].stride(0), _p(t["dr"]), t["dr"].stride(0), _p(t["dgi"]), t["dgi"].stride(0), _p(t["dgh"]),
                                           t["dgh"].stride(0), _p(t["dp"]), t["dp"].stride(0), _stream()), "gru_cell_bwd")

        def dense_def(t):
            dgi, dgh, dp = G.cell_bwd(t["gates"], t["q"], t["hp"], t["do"], t["dr"])
            return {"dgi": dgi, "dgh": dgh, "dp": dp}

        _cell_case(arena, param, layout, {"ldg": "gates", "ldq": "q", "ldhp": "hp", "lddo": "do", "lddr": "dr", "lddgi": "dgi", "lddgh": "dgh", "lddp": "dp"},
                   ins, {"dgi": (N, 3 * H), "dgh": (N, 3 * H), "dp": (N, H)}, call, dense_def, 1e-5)


def _drive_lstm_cell_fwd(arena, param, layout):
    import _dynrnn_ref as D
    lib = _lib()
    for H in _widths(layout):
        ins = {"gi": _rand(N, 4 * H, seed=130), "gh": _rand(N, 4 * H, seed=131), "cp": _rand(N, H, seed=132), "b": _rand(4 * H, seed=133, scale=0.1)}

        def call(t):
            _ck(lib.ctgcn_lstm_cell_fwd_f32(N, H, _p(t["gi"]), t["gi"].stride(0), _p(t["gh"]), t["gh"].stride(0), _p(t["b"]), _p(t["cp"]), t["cp"].stride(0),
                                            _p(t["h"]), t["h"].stride(0), _p(t["c"]), t["c"].stride(0), _p(t["gates"]), t["gates"].stride(0), _stream()),
                "lstm_cell_fwd")

        def dense_def(t):
            h, c, gates = D.cell_fwd(t["gi"], t["gh"], t["b"], t["cp"])
            return {"h": h, "c": c, "gates": gates}

        _cell_case(arena, param, layout, {"ldgi": "gi", "ldgh": "gh", "ldcp": "cp", "ldh": "h", "ldc": "c", "ldg": "gates"}, ins,
                   {"h": (N, H), "c": (N, H), "gates": (N, 4 * H)}, call, dense_def, 2e-6)


def _drive_lstm_cell_bwd(arena, param, layout):
    import _dynrnn_ref as D
    lib = _lib()
    for H in _widths(layout):
        ins = {"gates": torch.sigmoid(_rand(N, 4 * H, seed=140)), "c": _rand(N, H, seed=141), "cp": _rand(N, H, seed=142), "do": _rand(N, H, seed=143),
               "dr": _rand(N, H, seed=144), "dn": _rand(N, H, seed=145)}

        def call(t):
            _ck(lib.ctgcn_lstm_cell_bwd_f32(N, H, _p(t["gates"]), t["gates"].stride(0), _p(t["c"]), t["c"].stride(0), _p(t["cp"]), t["cp"].stride(0),
                                            _p(t["do"]), t["do"].stride(0), _p(t["dr"]), t["dr"].stride(0), _p(t["dn"]), t["dn"].stride(0), _p(t["dg"]),
                                            t["dg"].stride(0), _p(t["dp"]), t["dp"].stride(0), _stream()), "lstm_cell_bwd")

        def dense_def(t):
            dg, dp = D.cell_bwd(t["gates"], t["c"], t["cp"], t["do"], t["dr"], t["dn"])
            return {"dg": dg, "dp": dp}

        _cell_case(arena, param, layout, {"ldg": "gates", "ldc": "c", "ldcp": "cp", "lddo": "do", "lddr": "dr", "lddn": "dn", "lddg": "dg", "lddp": "dp"},
                   ins, {"dg": (N, 4 * H), "dp": (N, H)}, call, dense_def, 1e-5)


# ------------------------------------------------------------------------------------------- row-selected passes
@functools.lru_cache(maxsize=None)
def _stack(ncols):
    """a stacked CSR of 33 rows over `ncols` node ids; row 0 has 9 000 entries (positions that select it are long: threshold 64)"""
    rng = np.random.default_rng(11)
    lens = [9000] + [int(rng.integers(0, 6)) for _ in range(N - 1)]
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    col = np.concatenate([np.sort(rng.integers(0, ncols, m)) for m in lens]).astype(np.int32)
    val = (rng.integers(1, 9, rp[-1]) * 0.25).astype(np.float32)
    A = np.zeros((N, ncols))
    for r in range(N):
        np.add.at(A[r], col[rp[r]:rp[r + 1]], val[rp[r]:rp[r + 1]].astype(np.float64))
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return dev(rp), dev(col), dev(val), torch.from_numpy(A), np.asarray(lens)


def _drive_rowsel_conv(arena, param, layout):
    """tests/test_gpu_dyngem_ops.py: Y[b] = relu(bias + sum_s sum_{e in row idx[b][s]} val[e] S[s col_stride + col[e]]), floor 2e-6.
    lds: S rows 2^27 apart, slot 1 reaching row 32.  col_stride: dense S rows, the SLOTS 2^31 and 2^32 floats apart."""
    lib = _lib()
    assert lib.ctgcn_rowsel_max_slots() >= 3
    for d in _widths(layout) if param != "col_stride" else (128,):
        slots, ncols = (3, 8) if param == "col_stride" else (2, 16)
        rp, col, val, A, lens = _stack(ncols)
        idx = np.array([[(7 * b + 3 * s) % N if (b + s) % 5 else -1 for s in range(slots)] for b in range(N)], np.int32)
        idx[1, 0] = 0                                                       # the long row, in both kinds of slot
        idx[2, slots - 1] = 0
        entries = np.array([sum(lens[i] for i in row if i >= 0) for row in idx])
        long_pos = torch.from_numpy(np.flatnonzero(entries > 64).astype(np.int32)).to(DEV)
        pieces = -(-int(entries.max()) // 256)
        nbytes = len(long_pos) * pieces * (-(-d // 4) * 4) * 4
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        idx_d, bias = torch.from_numpy(idx).to(DEV), _ints(d, seed=150)
        if param == "col_stride":
            S = _ints(N, ncols * d, seed=151)                               # wide row 16 s holds slot s: node c in columns [c d, (c + 1) d)
            src = lambda s, c: S[16 * s, c * d:(c + 1) * d]
        else:
            S = _ints(N, d, seed=152)                                       # row 17 s + c
            src = lambda s, c: S[17 * s + c]
        Sm = np.stack([np.stack([src(s_, c).double().cpu().numpy() for c in range(ncols)]) for s_ in range(slots)])      # [slots, ncols, d]
        ref = np.zeros((N, d))
        for b in range(N):
            for s_ in range(slots):
                if idx[b, s_] >= 0:
                    ref[b] += A[idx[b, s_]].numpy() @ Sm[s_]
        ref = torch.relu(torch.from_numpy(ref) + bias.double().cpu())

        def call(t):
            lds, stride = (d, 16 * t["S"].stride(0) // d) if param == "col_stride" else (t["S"].stride(0), 17)
            assert param != "col_stride" or (16 * t["S"].stride(0)) % d == 0
            _ck(lib.ctgcn_rowsel_conv_fwd_f32(N, slots, d, _p(idx_d), _p(rp), _p(col), _p(val), _p(t["S"]), lds, stride, _p(bias), 1, _p(t["Y"]),
                                              t["Y"].stride(0), _p(long_pos), len(long_pos), 64, _p(ws), nbytes, _stream()), "rowsel_conv_fwd")

        _run_case(arena, layout, "Y" if param == "ldy" else "S", {"S": S}, {"Y": (N, d)}, call, {"Y": ref}, _floor(2e-6))


def _drive_rowsel_bucket(arena, param, layout):
    """out[r] = sum of G[inv_pos[k]] over the positions of row r, in order; a row without positions is zeros"""
    lib = _lib()
    rng = np.random.default_rng(12)
    lens = rng.integers(0, 5, N)
    lens[3] = 0
    inv_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    inv_pos = np.concatenate([np.sort(rng.choice(N, m, replace=False)) for m in lens]).astype(np.int32)
    inv_pos[:2] = (0, 32)
    ptr_d, pos_d = torch.from_numpy(inv_ptr).to(DEV), torch.from_numpy(inv_pos).to(DEV)
    for d in _widths(layout):
        G = _ints(N, d, seed=153)
        g64 = G.double().cpu().numpy()
        ref = np.stack([g64[inv_pos[inv_ptr[r]:inv_ptr[r + 1]]].sum(0) for r in range(N)])

        def call(t):
            _ck(lib.ctgcn_rowsel_bucket_f32(N, d, _p(ptr_d), _p(pos_d), _p(t["G"]), t["G"].stride(0), _p(t["out"]), t["out"].stride(0), _stream()), "rowsel_bucket")

        _run_case(arena, layout, "G" if param == "ldg" else "out", {"G": G}, {"out": (N, d)}, call, {"out": torch.from_numpy(ref)}, _floor(2e-6))


# --------------------------------------------------------------------------------- evaluation passes over an embedding E
def _nan64(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=DEV)


def _drive_sim_gram(arena, param, layout, f64=False):
    """tests/test_gpu_sim_shapes.py: E[rows] E[rows]^T exactly symmetric and within d 2^-52 (|E||E|^T) of float64; unordered rows, one repeat"""
    lib = _lib()
    N = N64 if f64 else W.MAX_ROWS
    fn = lib.ctgcn_sim_gram_f64 if f64 else lib.ctgcn_sim_gram_f32
    rows = np.random.default_rng(13).permutation(N).astype(np.int64)
    rows[-1] = rows[0]
    rows_d = torch.from_numpy(rows).to(DEV)
    for d in _widths(layout):
        E = _rand64(N, d, seed=160) if f64 else _rand(N, d, seed=160)
        E64 = E.double().cpu().numpy()[rows]

        def call(t):
            _ck(fn(N, d, _p(t["E"]), t["E"].stride(0), _p(rows_d), _p(t["out"]), _stream()), "sim_gram")

        def compare(name, got, ref64):
            assert torch.equal(got, got.T)
            bound = d * 2.0 ** -52 * (np.abs(E64) @ np.abs(E64).T)
            assert float((np.abs(got.cpu().numpy() - ref64.numpy()) / bound).max()) <= 1.0

        _run_case(arena, layout, "E", {"E": E}, {"out": _nan64(N, N)}, call, {"out": torch.from_numpy(E64 @ E64.T)}, compare)


def _ridge_case(d, f64=False):
    rng = np.random.default_rng(14 + d)
    F, T, P = 5, 2, 3
    n = N64 if f64 else N
    X = _rand64(n, d, seed=161) if f64 else _rand(n, d, seed=161)
    Y = torch.from_numpy(rng.standard_normal((n, T))).to(DEV)
    Wt = torch.from_numpy(rng.standard_normal((F, P, d + 1)) * (0.5 / np.sqrt(d))).to(DEV)
    return F, T, P, X, Y, Wt, np.array([1, 0, 1], np.int32)


def _drive_ridge_gram(arena, param, layout, f64=False):
    """tests/test_gpu_cent_shapes.py::test_ridge_gram_against_long_double: within rows_f 2^-52 (|Z_f|^T |Z_f|) per entry; 33 rows in 5 folds"""
    import _central_ref as R
    lib = _lib()
    N = N64 if f64 else 33
    fn = lib.ctgcn_ridge_gram_f64 if f64 else lib.ctgcn_ridge_gram_f32
    for d in _widths(layout):
        F, T, _P, X, Y, _W, _tgt = _ridge_case(d, f64)
        nb = int(lib.ctgcn_ridge_gram_workspace_bytes(d, T, F))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        folds = R.fold_grams(X.cpu().numpy(), Y.cpu().numpy(), F)

        def call(t):
            _ck(fn(N, d, T, F, _p(t["X"]), t["X"].stride(0), _p(Y), _p(t["gram"]), _p(ws), nb, _stream()), "ridge_gram")

        def compare(name, got, ref64):
            got = got.cpu().numpy().reshape(F, d + 1, d + 1 + T)
            for f, (want, absg, rows) in enumerate(folds):
                assert got[f, d, d] == rows
                assert float((np.abs(got[f] - want) / (rows * 2.0 ** -52 * absg)).max()) <= 1.0, f

        _run_case(arena, layout, "X", {"X": X}, {"gram": _nan64(F, (d + 1) * (d + 1 + T))}, call, {"gram": None}, compare)


def _drive_ridge_sse(arena, param, layout, f64=False):
    """tests/test_gpu_cent_shapes.py::test_ridge_sse_against_long_double: the long-double mirror within its running-error bound"""
    import _central_ref as R
    lib = _lib()
    N = N64 if f64 else 33
    fn = lib.ctgcn_ridge_sse_f64 if f64 else lib.ctgcn_ridge_sse_f32
    for d in _widths(layout):
        F, T, P, X, Y, W, tgt = _ridge_case(d, f64)
        nb = int(lib.ctgcn_ridge_sse_workspace_bytes(P, F))
        ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
        tgt_d = torch.from_numpy(tgt).to(DEV)
        rows_max = -(-N // F)
        want, bound = R.fold_sse(X.cpu().numpy(), Y.cpu().numpy(), W.cpu().numpy(), tgt, F, 1 + -(-(-(-rows_max // 16)) // 32) + 4 + 128)

        def call(t):
            _ck(fn(N, d, T, F, P, _p(t["X"]), t["X"].stride(0), _p(Y), _p(W), _p(tgt_d), _p(t["sse"]), _p(ws), nb, _stream()), "ridge_sse")

        def compare(name, got, ref64):
            assert float((np.abs(got.cpu().numpy() - want) / bound).max()) <= 1.0

        _run_case(arena, layout, "X", {"X": X}, {"sse": _nan64(F, P)}, call, {"sse": None}, compare)


# --------------------------------------------------------------------------------------------------- attention passes
def _gat_tol(ref32):
    """tests/test_gpu_gat_conv.py: the larger of close_scaled's tolerance and 4 x the largest error of the float32 mirror"""
    def compare(name, got, ref64):
        want, g = ref64.numpy(), got.double().cpu().numpy()
        tol = np.maximum(1e-5 * np.abs(want) + 2e-6 * max(1.0, float(np.abs(want).max(initial=0.0))), 4 * np.abs(ref32[name].double().numpy() - want).max(initial=0.0))
        assert (np.abs(g - want) <= tol).all(), (name, float((np.abs(g - want) / tol).max()))
    return compare


def _gat_entries():
    g = _graph()
    rp = g["row_ptr"].cpu().numpy()
    rows = torch.from_numpy(np.repeat(np.arange(N), np.diff(rp)).astype(np.int64))
    return g, rows, g["col"].cpu().long()


def _drive_gat_fwd(arena, param, layout):
    import _gat_ref as A
    lib = _lib()
    g, rows, cols = _gat_entries()
    heads = 2
    for d in _widths(layout):
        S = _rand(N, d, seed=170, scale=0.5)
        a_src, a_dst = _rand(heads, d // heads, seed=171, scale=0.3), _rand(heads, d // heads, seed=172, scale=0.3)
        floats = int(lib.ctgcn_gat_piece_floats(d, heads))
        nbytes = 36 * floats * 4
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

        def mirror(dt):
            s, a, b = S.cpu().to(dt), a_src.cpu().to(dt), a_dst.cpu().to(dt)
            Y, m, Z = A.attention(s, a, b, rows, cols, heads)
            sh = s.reshape(N, heads, d // heads)
            return {"out": torch.nn.functional.elu(Y), "Y": Y, "u": (sh * a).sum(-1), "v": (sh * b).sum(-1), "m": m, "Z": Z}

        def call(t):
            _ck(lib.ctgcn_gat_fwd_f32(N, d, heads, _p(g["row_ptr"]), _p(g["col"]), _p(t["S"]), t["S"].stride(0), _p(a_src), _p(a_dst), A.ALPHA, 1, 0.0, 0, 0.0, 0,
                                      _p(t["out"]), t["out"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(t["u"]), _p(t["v"]), _p(t["m"]), _p(t["Z"]),
                                      _p(g["long_rows"]), 1, g["threshold"], _p(ws), nbytes, _stream()), "gat_fwd")

        outs = {"out": (N, d), "Y": (N, d), "u": (N, heads), "v": (N, heads), "m": (N, heads), "Z": (N, heads)}
        _run_case(arena, layout, _pick(param, {"lds": "S", "ldout": "out", "ldy": "Y"}), {"S": S}, outs, call, mirror(torch.float64), _gat_tol(mirror(torch.float32)))


def _drive_gat_bwd_prep(arena, param, layout):
    lib = _lib()
    heads = 2
    for d in _widths(layout):
        dY, Y = _rand(N, d, seed=173), _rand(N, d, seed=174)
        u, m, Z = _rand(N, heads, seed=175), _rand(N, heads, seed=176), _rand(N, heads, seed=177).abs() + 0.5
        Z[5] = 0.0                                                          # a row without entries: 1 / Z is written as 0

        def mirror(dt):
            gy, y = dY.cpu().to(dt), Y.cpu().to(dt)
            G = gy * torch.where(y > 0, torch.ones_like(y), torch.exp(y))
            D = (G * y).reshape(N, heads, d // heads).sum(-1)
            z = Z.cpu().to(dt)
            pack = torch.stack([u.cpu().to(dt), m.cpu().to(dt), torch.where(z > 0, 1 / torch.where(z > 0, z, torch.ones_like(z)), torch.zeros_like(z)), D], -1)
            return {"G": G, "pack": pack.reshape(N, heads * 4)}

        def call(t):
            _ck(lib.ctgcn_gat_bwd_prep_f32(N, d, heads, _p(t["dY"]), t["dY"].stride(0), _p(t["Y"]), t["Y"].stride(0), 1, 0.0, 0, _p(u), _p(m), _p(Z), _p(t["G"]),
                                           t["G"].stride(0), _p(t["pack"]), _stream()), "gat_bwd_prep")

        _run_case(arena, layout, _pick(param, {"lddy": "dY", "ldy": "Y", "ldg": "G"}), {"dY": dY, "Y": Y}, {"G": (N, d), "pack": (N, heads * 4)}, call,
                  mirror(torch.float64), _gat_tol(mirror(torch.float32)))


def _drive_gat_da(arena, param, layout):
    lib = _lib()
    heads = 2
    for d in _widths(layout):
        S, du, dv = _rand(N, d, seed=178), _rand(N, heads, seed=179), _rand(N, heads, seed=180)
        nbytes = int(lib.ctgcn_gat_da_workspace_bytes(N, d))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

        def mirror(dt):
            sh = S.cpu().to(dt).reshape(N, heads, d // heads)
            return {"da_src": (du.cpu().to(dt)[:, :, None] * sh).sum(0), "da_dst": (dv.cpu().to(dt)[:, :, None] * sh).sum(0)}

        def call(t):
            _ck(lib.ctgcn_gat_da_f32(N, d, heads, _p(t["S"]), t["S"].stride(0), _p(du), _p(dv), _p(t["da_src"]), _p(t["da_dst"]), _p(ws), nbytes, _stream()), "gat_da")

        _run_case(arena, layout, "S", {"S": S}, {"da_src": (heads, d // heads), "da_dst": (heads, d // heads)}, call, mirror(torch.float64),
                  _gat_tol(mirror(torch.float32)))


def _drive_tgat_fwd(arena, param, layout):
    """GATConv's form (tests/_tg_ref.py::attention): a_tgt on the row's own features, a_src on the gathered ones; out = relu(Y + bias)"""
    import _tg_ref as TG
    lib = _lib()
    g, rows, cols = _gat_entries()
    heads = 2
    for d in _widths(layout):
        S, bias = _rand(N, d, seed=181, scale=0.5), _rand(d, seed=182, scale=0.1)
        a_tgt, a_src = _rand(heads, d // heads, seed=183, scale=0.3), _rand(heads, d // heads, seed=184, scale=0.3)
        nbytes = 36 * int(lib.ctgcn_gat_piece_floats(d, heads)) * 4
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)

        def mirror(dt):
            Y = TG.attention(S.cpu().to(dt), a_src.cpu().to(dt), a_tgt.cpu().to(dt), cols, rows, heads, 0.2)
            return {"Y": Y, "out": torch.relu(Y + bias.cpu().to(dt))}

        def call(t):
            _ck(lib.ctgcn_tgat_fwd_f32(N, d, heads, _p(g["row_ptr"]), _p(g["col"]), _p(t["S"]), t["S"].stride(0), _p(a_tgt), _p(a_src), 0.2, _p(bias), 1, 0.0, 0,
                                       _p(t["out"]), t["out"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(t["u"]), _p(t["v"]), _p(t["m"]), _p(t["Z"]),
                                       _p(g["long_rows"]), 1, g["threshold"], _p(ws), nbytes, _stream()), "tgat_fwd")

        outs = {"out": (N, d), "Y": (N, d), "u": (N, heads), "v": (N, heads), "m": (N, heads), "Z": (N, heads)}
        _run_case(arena, layout, _pick(param, {"lds": "S", "ldout": "out", "ldy": "Y"}), {"S": S}, outs, call, mirror(torch.float64), _gat_tol(mirror(torch.float32)))


# ------------------------------------------------------------------------------------------------ VGRNN fused gathers
def _vg_long(g, width):
    return _long(g, width)


def _drive_ggru_gates(arena, param, layout):
    """tests/test_gpu_vgrnn_ops.py: max(4 x the stock fp32 error, 2e-6) max|ref| for results"""
    lib = _lib()
    g, A = _csr()
    for hid in _widths(layout):
        ins = {"U": _ints(N, 3 * hid, seed=190) / 1024.0, "h": _rand(N, hid, seed=191), "b": _rand(3 * hid, seed=192, scale=0.1)}
        long, _ws = _vg_long(g, 3 * hid)

        def call(t):
            _ck(lib.ctgcn_ggru_gates_fwd_f32(N, hid, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["U"]), t["U"].stride(0), _p(t["b"]), _p(t["h"]),
                                             t["h"].stride(0), _p(t["z"]), _p(t["r"]), _p(t["q"]), _p(t["c"]), *long, _stream()), "ggru_gates")

        def dense_def(t):
            gz, gr, gc = (A.to(t["U"].dtype) @ t["U"] + t["b"]).chunk(3, dim=1)
            r = torch.sigmoid(gr)
            return {"z": torch.sigmoid(gz), "r": r, "q": r * t["h"], "c": gc}

        _cell_case(arena, param, layout, {"ldu": "U", "ldh": "h"}, ins, {k: (N, hid) for k in "zrqc"}, call, dense_def, 2e-6)


def _drive_ggru_blend(arena, param, layout):
    lib = _lib()
    g, A = _csr()
    for hid in _widths(layout):
        ins = {"V": _ints(N, hid, seed=193) / 1024.0, "c": _rand(N, hid, seed=194), "z": torch.sigmoid(_rand(N, hid, seed=195)), "h": _rand(N, hid, seed=196)}
        long, _ws = _vg_long(g, hid)

        def call(t):
            _ck(lib.ctgcn_ggru_blend_fwd_f32(N, hid, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["V"]), t["V"].stride(0), _p(t["c"]), t["c"].stride(0),
                                             _p(t["z"]), t["z"].stride(0), _p(t["h"]), t["h"].stride(0), _p(t["h_new"]), _p(t["h_tilde"]), *long, _stream()),
                "ggru_blend")

        def dense_def(t):
            ht = torch.tanh(t["c"] + A.to(t["V"].dtype) @ t["V"])
            return {"h_new": t["z"] * t["h"] + (1 - t["z"]) * ht, "h_tilde": ht}

        _cell_case(arena, param, layout, {"ldv": "V", "ldc": "c", "ldz": "z", "ldh": "h"}, ins, {"h_new": (N, hid), "h_tilde": (N, hid)}, call, dense_def, 2e-6)


def _drive_vgrnn_heads(arena, param, layout):
    lib = _lib()
    g, A = _csr()
    for out in _widths(layout):
        ins = {"S": _ints(N, 2 * out, seed=197) / 1024.0, "noise": _rand(N, out, seed=198), "b": _rand(2 * out, seed=199, scale=0.1)}
        long, _ws = _vg_long(g, 2 * out)

        def call(t):
            _ck(lib.ctgcn_vgrnn_heads_fwd_f32(N, out, _p(g["row_ptr"]), _p(g["col"]), _p(g["val"]), _p(t["S"]), t["S"].stride(0), _p(t["b"]), _p(t["noise"]),
                                              t["noise"].stride(0), _p(t["mean"]), _p(t["std"]), _p(t["z"]), *long, _stream()), "vgrnn_heads")

        def dense_def(t):
            gm, gs = (A.to(t["S"].dtype) @ t["S"] + t["b"]).chunk(2, dim=1)
            std = torch.nn.functional.softplus(gs)
            return {"mean": gm, "std": std, "z": gm + t["noise"] * std}

        _cell_case(arena, param, layout, {"lds": "S", "ldnoise": "noise"}, ins, {k: (N, out) for k in ("mean", "std", "z")}, call, dense_def, 2e-6)


def _drive_vgrnn_bwd_prep(arena, param, layout):
    """mode 0 (gates): G = [dz z (1 - z) | dq h r (1 - r) | dc], x0 = dq r, db = the column sums of G; floor 1e-5 (gradients)"""
    lib = _lib()
    for w in _widths(layout):
        ins = {"g0": _rand(N, w, seed=200), "g1": _rand(N, w, seed=201), "g2": _rand(N, w, seed=202), "s0": torch.sigmoid(_rand(N, w, seed=203)),
               "s1": torch.sigmoid(_rand(N, w, seed=204)), "s2": _rand(N, w, seed=205)}
        nbytes = int(lib.ctgcn_gcn_conv_prep_workspace_bytes(N, 3 * w))
        ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=DEV)

        def call(t):
            _ck(lib.ctgcn_vgrnn_bwd_prep_f32(0, N, w, _p(t["g0"]), t["g0"].stride(0), _p(t["g1"]), t["g1"].stride(0), _p(t["g2"]), t["g2"].stride(0),
                                             _p(t["s0"]), t["s0"].stride(0), _p(t["s1"]), t["s1"].stride(0), _p(t["s2"]), t["s2"].stride(0), _p(t["G"]),
                                             t["G"].stride(0), _p(t["x0"]), None, _p(t["db"]), _p(ws), nbytes, _stream()), "vgrnn_bwd_prep")

        def dense_def(t):
            dz, dq, dc, z, r, h = (t[k] for k in ("g0", "g1", "g2", "s0", "s1", "s2"))
            G = torch.cat([dz * z * (1 - z), dq * h * r * (1 - r), dc], 1)
            return {"G": G, "x0": dq * r, "db": G.sum(0, keepdim=True)}

        _cell_case(arena, param, layout, {"ldg0": "g0", "ldg1": "g1", "ldg2": "g2", "lds0": "s0", "lds1": "s1", "lds2": "s2", "ldG": "G"}, ins,
                   {"G": (N, 3 * w), "x0": (N, w), "db": (1, 3 * w)}, call, dense_def, 1e-5)


# ------------------------------------------------------------------------------------------- the fp64 TIMERS passes
N64 = W.MAX_ROWS_F64          # 32 rows of doubles: the byte positions of the fp32 view's rows 0..31 (tests/_wide_ref.py)


@functools.lru_cache(maxsize=None)
def _csr64():
    import scipy.sparse as sp
    rng = np.random.RandomState(21)
    A = sp.random(N64, N64, density=0.2, random_state=rng, data_rvs=lambda k: rng.randn(k)).tolil()
    A[0, :] = rng.randn(N64)                                   # every row of a wide X is gathered
    A = A.tocsr()
    A.sort_indices()
    dev = lambda a: torch.from_numpy(a).to(DEV)
    return A, dev(A.indptr.astype(np.int32)), dev(A.indices.astype(np.int32)), dev(A.data.astype(np.float64))


def _rand64(*shape, seed=0):
    return torch.from_numpy(np.random.RandomState(seed).randn(*shape)).to(DEV)


def _bounded(bound):
    """tests/test_gpu_timers_ops.py: |got - long-double reference| <= the summation bound, entry by entry"""
    def compare(name, got, ref64):
        assert (np.abs(got.cpu().numpy().astype(np.longdouble) - ref64) <= bound).all(), name
    return compare


def _drive_spmm_f64(arena, param, layout):
    import _timers_ref as T
    lib = _lib()
    A, rp, col, val = _csr64()
    for b in (16, 5):
        X, Y0 = _rand64(N64, b, seed=22), _rand64(N64, b, seed=23)
        LD = np.longdouble
        mag = np.abs(A) @ np.abs(X.cpu().numpy())
        ref = Y0.cpu().numpy().astype(LD) + A.astype(LD) @ X.cpu().numpy().astype(LD)
        m = int(np.diff(A.indptr).max())

        def call(t):
            _ck(lib.ctgcn_spmm_csr_f64(N64, b, _p(rp), _p(col), _p(val), _p(t["X"]), t["X"].stride(0), _p(t["Y"]), t["Y"].stride(0), 1, _stream()), "spmm_f64")

        _run_case(arena, layout, "X" if param == "ldx" else "Y", {"X": X}, {"Y": Y0}, call, {"Y": ref},
                  _bounded((m + 1) * T.U53 * (mag + np.abs(Y0.cpu().numpy()))))


def _drive_tsgemm_tn(arena, param, layout):
    import _timers_ref as T
    lib = _lib()
    for b1, b2 in ((16, 7), (5, 16)):
        X, Y = _rand64(N64, b1, seed=24), _rand64(N64, b2, seed=25)
        nb = int(lib.ctgcn_tsgemm_tn_workspace_bytes(N64, b1, b2))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        x, y = X.cpu().numpy(), Y.cpu().numpy()

        def call(t):
            _ck(lib.ctgcn_tsgemm_tn_f64(N64, b1, b2, _p(t["X"]), t["X"].stride(0), _p(t["Y"]), t["Y"].stride(0), _p(t["G"]), _p(ws), nb, _stream()), "tsgemm_tn")

        _run_case(arena, layout, "X" if param == "ldx" else "Y", {"X": X, "Y": Y}, {"G": torch.full((b1, b2), float("nan"), dtype=torch.float64, device=DEV)},
                  call, {"G": x.astype(np.longdouble).T @ y.astype(np.longdouble)}, _bounded(N64 * T.U53 * (np.abs(x).T @ np.abs(y))))


def _drive_tsgemm_nn(arena, param, layout):
    import _timers_ref as T
    lib = _lib()
    for b1, b2 in ((16, 7), (5, 16)):
        rows = N64 if param != "ldc" else 40                      # C is [b1, b2]: wide, it is the operand with 32 rows
        b1 = b1 if param != "ldc" else N64
        X, C = _rand64(rows, b1, seed=26), _rand64(b1, b2, seed=27)
        nb = int(lib.ctgcn_tsgemm_nn_workspace_bytes(rows, b2))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        x, c = X.cpu().numpy(), C.cpu().numpy()

        def call(t):
            _ck(lib.ctgcn_tsgemm_nn_f64(rows, b1, b2, _p(t["X"]), t["X"].stride(0), _p(t["C"]), t["C"].stride(0), _p(t["Y"]), t["Y"].stride(0), None, _p(ws), nb,
                                        _stream()), "tsgemm_nn")

        _run_case(arena, layout, {"ldx": "X", "ldc": "C", "ldy": "Y"}[param], {"X": X, "C": C},
                  {"Y": torch.full((rows, b2), float("nan"), dtype=torch.float64, device=DEV)}, call,
                  {"Y": x.astype(np.longdouble) @ c.astype(np.longdouble)}, _bounded(b1 * T.U53 * (np.abs(x) @ np.abs(c))))


def _drive_timers_obj(arena, param, layout):
    import _timers_ref as T
    lib = _lib()
    A, rp, col, val = _csr64()
    LD = np.longdouble
    for k in (16, 5):
        U, V = _rand64(N64, k, seed=28), _rand64(N64, k, seed=29)
        old = _rand64(A.nnz, seed=30)
        nb = int(lib.ctgcn_timers_obj_workspace_bytes(N64, k))
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device=DEV)
        u, v, o = U.cpu().numpy(), V.cpu().numpy(), old.cpu().numpy()
        for s_old in (None, old):
            ref = T.obj_sums(A.astype(LD), u.astype(LD), v.astype(LD), None if s_old is None else o.astype(LD), as_float=False)
            bound = T.obj_bound(A, u, v, None if s_old is None else o)

            def call(t):
                _ck(lib.ctgcn_timers_obj_f64(N64, k, _p(rp), _p(col), _p(val), _p(s_old), _p(t["U"]), t["U"].stride(0), _p(t["V"]), t["V"].stride(0), _p(t["out"]),
                                             _p(ws), nb, _stream()), "timers_obj")

            _run_case(arena, layout, "U" if param == "ldu" else "V", {"U": U, "V": V}, {"out": torch.full((1, 2), float("nan"), dtype=torch.float64, device=DEV)},
                      call, {"out": np.array([[ref[0], ref[1]]], dtype=LD)}, _bounded(np.array([[bound[0], bound[1]]])))


def _drive_lp(which):
    """tests/test_gpu_logreg_shapes.py::test_link_prediction_passes and its bounds (1e-6 / 1e-6 / 1e-5 of the error scales, 1e-4 for scores),
    through ctgcn_amd.evaluation._logreg, which passes E.stride(0) on: four models, one per edge measure, 100 edges over the 33 rows of E"""
    def drive(arena, param, layout):
        import _logreg_ref as R
        from ctgcn_amd.evaluation import _logreg
        gen = torch.Generator().manual_seed(31)
        for d in _widths(layout):
            E = _rand(N, d, seed=210)
            edges = torch.stack([torch.randint(0, N, (100,), generator=gen), torch.randint(0, N, (100,), generator=gen), (torch.rand(100, generator=gen) < 0.3).long()], 1)
            edges[0], edges[1] = torch.tensor([0, 32, 1]), torch.tensor([32, 16, 0])
            Wt = (torch.randn(4, d + 1, generator=gen, dtype=torch.float64) * 0.2).to(DEV)
            es = _logreg.EdgeSet(edges.to(DEV), N)
            En, Wn, ed = E.double().cpu().numpy(), Wt.cpu().numpy(), edges.numpy()
            a, b, y = En[ed[:, 0]], En[ed[:, 1]], ed[:, 2]
            sw = np.where(y > 0, es.w_pos, es.w_neg)
            refs = [R.loss_grad_hess(R.features(meas, a, b), y, es.w_neg, es.w_pos, Wn[m]) + R.error_scales(R.features(meas, a, b), sw)
                    for m, meas in enumerate(R.MEASURES)]

            def call(t):
                if which == "grad":
                    loss, grad = _logreg.loss_grad(t["E"], es, R.MEASURES, Wt)
                    t["out"].copy_(torch.cat([loss[:, None], grad], 1))
                elif which == "hess":
                    t["out"].copy_(_logreg.hessian(t["E"], es, R.MEASURES, Wt).reshape(4, -1))
                else:
                    t["out"].copy_(_logreg.scores(t["E"], es, R.MEASURES, Wt).double())

            def compare(name, got, ref64):
                g = got.cpu().numpy()
                for m, (L, G, H, zz, scale, scale2) in enumerate(refs):
                    if which == "grad":
                        assert abs(g[m, 0] - L) <= 1e-6 * scale and np.abs(g[m, 1:] - G).max() <= 1e-6 * scale, m
                    elif which == "hess":
                        assert np.abs(g[m].reshape(d + 1, d + 1) - H).max() <= 1e-5 * scale2, m
                    else:
                        assert np.abs(g[m] - zz).max() <= 1e-4, m

            width = {"grad": d + 2, "hess": (d + 1) * (d + 1), "scores": 100}[which]
            _run_case(arena, layout, "E", {"E": E}, {"out": _nan64(4, width)}, call, {"out": None}, compare)
    return drive


# ------------------------------------------------------------------------------------------- supervised classifier head
def _cls_parity(ref32):
    """tests/test_gpu_supervised_kernels.py::_parity: |got - ref| <= max(1.5 x |torch fp32 - ref|_max, 8 x 2^-24 max|ref|)"""
    def compare(name, got, ref64):
        ref, t32 = ref64.double().cpu().numpy(), ref32[name].double().cpu().numpy()
        tol = max(1.5 * float(np.abs(t32 - ref).max(initial=0.0)), 8.0 * 2.0 ** -24 * float(np.abs(ref).max(initial=0.0)))
        assert float(np.abs(got.double().cpu().numpy() - ref).max(initial=0.0)) <= tol, name
    return compare


def _cls_fixture(d, mode):
    from ctgcn_amd import ops
    gen = torch.Generator().manual_seed(41 + d + mode)
    a, b = torch.randint(0, N, (60,), generator=gen), torch.randint(0, N, (60,), generator=gen)
    a[:3], b[:3] = torch.tensor([32, 16, 0]), torch.tensor([0, 32, 31])
    idx = a.to(DEV) if mode == 0 else torch.stack([a, b]).to(DEV)
    Wc = ((torch.rand(4, d, generator=gen) * 2 - 1) / np.sqrt(d)).to(DEV)
    bias = ((torch.rand(4, generator=gen) * 2 - 1) * 0.1).to(DEV)
    return idx, Wc, bias, ops.cls_items(idx, mode, N)


def _cls_pre(E, idx, Wc, bias, mode, dt):
    E = E.to(dt)
    f = E[idx] if mode == 0 else E[idx[0]] * E[idx[1]]
    return torch.nn.functional.linear(f, Wc.to(dt), bias.to(dt)), f


def _drive_cls_head_fwd(arena, param, layout):
    from ctgcn_amd import ops
    for d in _widths(layout):
        for mode in (0, 1):                                                 # node items, Hadamard pair items
            E = _rand(N, d, seed=220)
            idx, Wc, bias, items = _cls_fixture(d, mode)

            def call(t):
                t["out"].copy_(ops.cls_head_forward(t["E"], items, Wc, bias, 1))

            def mirror(dt):
                return {"out": torch.nn.functional.selu(_cls_pre(E, idx, Wc, bias, mode, dt)[0])}

            _run_case(arena, layout, "E", {"E": E}, {"out": (60, 4)}, call, mirror(torch.float64), _cls_parity(mirror(torch.float32)))


def _drive_cls_head_bwd(arena, param, layout):
    from ctgcn_amd import ops
    for d in _widths(layout):
        for mode in (0, 1):
            E, dl = _rand(N, d, seed=221), _rand(60, 4, seed=222)
            idx, Wc, bias, items = _cls_fixture(d, mode)

            def call(t):
                _dE, dW, db = ops.cls_head_backward(t["E"], items, Wc, dl, dE=t["dE"])
                t["dW"].copy_(dW)
                t["db"].copy_(db[None])

            def mirror(dt):
                e = E.detach().clone().to(dt).requires_grad_(True)             # a leaf of its own: E itself goes to the kernel
                pre, f = _cls_pre(e, idx, Wc, bias, mode, dt)
                (dE,) = torch.autograd.grad((pre * dl.to(dt)).sum(), e)
                return {"dE": dE.detach(), "dW": (dl.to(dt).t() @ f).detach(), "db": dl.to(dt).sum(0, keepdim=True)}

            _run_case(arena, layout, "E" if param == "lde" else "dE", {"E": E}, {"dE": (N, d), "dW": (4, d), "db": (1, 4)}, call, mirror(torch.float64),
                      _cls_parity(mirror(torch.float32)))


# --------------------------------------------------------------------------------------------------------- weight gradient
def _dw_operands(rows, steps, shift):
    dgi, dghn = _rand(rows, 384, seed=70, scale=0.5), _rand(rows, 128, seed=71, scale=0.5)
    x = torch.tanh(_rand(rows, 128, seed=72))
    xs = x.clone()
    if shift:
        xs = torch.zeros_like(x)
        xs.view(rows // steps, steps, 128)[:, 1:] = x.view(rows // steps, steps, 128)[:, :-1]
    G = torch.cat([dgi[:, :256], dghn], 1)
    return dgi[:, :256].contiguous(), dghn, x, G, xs


def _drive_weight_grad(arena, param, layout):
    """the kernel's buffer descriptors span at most 2 GiB per block: a 2^27-float stride is refused, not read wrong"""
    from ctgcn_amd import _lib as L, ops
    g01, g2, x, _, _ = _dw_operands(N - 1, 4, True)
    t = {"ldg01": g01, "ldg2": g2, "ldx": x}
    name = {"ldg01": "g01", "ldg2": "g2", "ldx": "x"}[param]
    t[param] = arena.put(layout, t[param])
    part = torch.zeros(8, 384, 128, device=DEV)
    with pytest.raises(L.CtgcnHipError, match=r"code -4.*gru_weight_grad: %s with ld=" % name):
        ops._weight_grad(part, t["ldg01"], t["ldg2"], t["ldx"], 4, True, False)
    torch.cuda.synchronize()
    assert not part.any()                                    # refused before any launch


def dw_max_ld(rows, n_pairs, shift_x):
    """Largest leading dimension ctgcn_gru_weight_grad_f32 can address, from the kernel's arithmetic: block pair p stages the 32-row chunks
    [p per, (p + 1) per); its descriptor starts at its first row (one row earlier for the shifted x) and covers min(bytes to the end of the
    last data row + the 128-byte tail of 32 columns, 0x7fffffff); offsets are 32-bit, so rows past the end must stay below 2^32 to read 0."""
    nchunks = -(-rows // 32)
    per = -(-nchunks // n_pairs)
    nblk = -(-nchunks // per)
    sh = 1 if shift_x else 0
    data = pad = 0
    for p in range(nblk):
        lo, hi = p * per * 32, min((p + 1) * per, nchunks) * 32
        first = lo - (sh if lo >= sh else 0)
        data = max(data, min(hi, rows) - 1 - sh - first)
        pad = max(pad, hi - 1 - sh - first)
    lim = (0x7fffffff - 128) // 4 // data if data > 0 else None
    if pad > data:
        lim = min(lim, (2 ** 32 - 128) // 4 // pad) if lim else (2 ** 32 - 128) // 4 // pad
    return lim


@pytest.mark.parametrize("shift", [False, True])
@pytest.mark.parametrize("wide", ["g01", "g2", "x"])
def test_weight_gradient_just_below_the_descriptor_bound(arena, wide, shift):
    """64 rows, 8 block pairs: a block's 32 rows span a little under 2 GiB, the operand about 4 GiB.  The float64 weight gradient at the
    tolerance of tests/test_gpu_gru.py::test_split_bf16_weight_gradient_is_fp32_accurate."""
    from ctgcn_amd import ops
    rows, steps = 64, 4
    ld = dw_max_ld(rows, 8, shift and wide == "x")
    assert 31 * ld * 4 + 128 <= 0x7fffffff < 31 * (ld + 1) * 4 + 128 and 63 * ld * 4 > 2 ** 32
    g01, g2, x, G, xs = _dw_operands(rows, steps, shift)
    t = {"g01": g01, "g2": g2, "x": x}
    base = W.LAYOUTS["aligned"][0]
    d = t[wide].shape[1]
    for r in range(rows):
        arena.buf[base + r * ld: base + r * ld + d].copy_(t[wide][r])
    t[wide] = torch.as_strided(arena.buf, (rows, d), (ld, 1), base)
    ref = G.double().cpu().t() @ xs.double().cpu()
    part = torch.full((8, 384, 128), float("nan"), device=DEV)
    ops._weight_grad(part, t["g01"], t["g2"], t["x"], steps, shift, False)
    out = part.sum(0)
    err_split = (out.cpu().double() - ref).abs().max().item()
    err_fp32 = ((G.t() @ xs).double().cpu() - ref).abs().max().item()
    print("  weight gradient, %s wide (ld %d), shift %d: |err| %.3e, fp32 GEMM %.3e" % (wide, ld, shift, err_split, err_fp32))
    assert err_split <= max(2.0 * err_fp32, 3e-7 * ref.abs().max().item()), (err_split, err_fp32)
    dense = torch.full((8, 384, 128), float("nan"), device=DEV)
    ops._weight_grad(dense, g01, g2, x, steps, shift, False)
    assert torch.equal(part, dense)                          # deterministic: the stride changes no arithmetic


# ------------------------------------------------------------------------------------------------------------- the test
DRIVERS = {
    "ctgcn_transpose_bias_f32": _drive_transpose_bias,
    "ctgcn_spmm_csr_f32": _drive_spmm,
    "ctgcn_core_aggregate_f32": _drive_core_aggregate,
    "ctgcn_core_aggregate_split_f32": _drive_core_aggregate_split,
    "ctgcn_core_aggregate_bwd_f32": _drive_core_aggregate_bwd,
    "ctgcn_gru_seq_f32": _drive_gru_seq,
    "ctgcn_layernorm_bwd_f32": _drive_layernorm_bwd,
    "ctgcn_gru_layer_f32": _drive_gru_layer,
    "ctgcn_gru_layer_presplit_f32": _drive_gru_layer_presplit,
    "ctgcn_gru_input_proj_f32": _drive_gru_input_proj,
    "ctgcn_gru_input_grad_f32": _drive_gru_input_grad,
    "ctgcn_gru_weight_grad_f32": _drive_weight_grad,
    "ctgcn_gru_bwd_in_f32": _drive_gru_bwd_in,
    "ctgcn_linear_f32": _drive_linear,
    "ctgcn_split_rows_f32": _drive_packed("split_rows"),
    "ctgcn_pack_weight_f32": _drive_packed("pack_weight"),
    "ctgcn_linear_packed_f32": _drive_packed("linear_packed"),
    "ctgcn_linear_presplit_f32": _drive_linear_presplit,
    "ctgcn_gcn_layer_fwd_f32": _drive_gcn_layer_fwd,
    "ctgcn_gcn_layer_bwd_f32": _drive_gcn_layer_bwd,
    "ctgcn_gcn_conv_fwd_f32": _conv_fwd("gcn"),
    "ctgcn_gcn_conv_prep_f32": _conv_prep("gcn"),
    "ctgcn_tg_conv_fwd_f32": _conv_fwd("tg"),
    "ctgcn_tg_conv_prep_f32": _conv_prep("tg"),
    "ctgcn_pool_conv_fwd_f32": _drive_pool_conv_fwd,
    "ctgcn_pool_conv_prep_f32": _drive_pool_conv_prep,
    "ctgcn_pool_max_fwd_f32": _drive_pool_max_fwd,
    "ctgcn_pool_max_bwd_f32": _drive_pool_max_bwd,
    "ctgcn_bn_stats_f32": _drive_bn_stats,
    "ctgcn_bn_apply_f32": _drive_bn_apply,
    "ctgcn_bn_bwd_f32": _drive_bn_bwd,
    "ctgcn_gru_cell_fwd_f32": _drive_gru_cell_fwd,
    "ctgcn_gru_cell_bwd_f32": _drive_gru_cell_bwd,
    "ctgcn_lstm_cell_fwd_f32": _drive_lstm_cell_fwd,
    "ctgcn_lstm_cell_bwd_f32": _drive_lstm_cell_bwd,
    "ctgcn_rowsel_conv_fwd_f32": _drive_rowsel_conv,
    "ctgcn_rowsel_bucket_f32": _drive_rowsel_bucket,
    "ctgcn_gat_fwd_f32": _drive_gat_fwd,
    "ctgcn_gat_bwd_prep_f32": _drive_gat_bwd_prep,
    "ctgcn_gat_da_f32": _drive_gat_da,
    "ctgcn_tgat_fwd_f32": _drive_tgat_fwd,
    "ctgcn_ggru_gates_fwd_f32": _drive_ggru_gates,
    "ctgcn_ggru_blend_fwd_f32": _drive_ggru_blend,
    "ctgcn_vgrnn_heads_fwd_f32": _drive_vgrnn_heads,
    "ctgcn_vgrnn_bwd_prep_f32": _drive_vgrnn_bwd_prep,
    "ctgcn_spmm_csr_f64": _drive_spmm_f64,
    "ctgcn_tsgemm_tn_f64": _drive_tsgemm_tn,
    "ctgcn_tsgemm_nn_f64": _drive_tsgemm_nn,
    "ctgcn_timers_obj_f64": _drive_timers_obj,
    "ctgcn_lp_grad_f32": _drive_lp("grad"),
    "ctgcn_lp_hess_f32": _drive_lp("hess"),
    "ctgcn_lp_scores_f32": _drive_lp("scores"),
    "ctgcn_cls_head_fwd_f32": _drive_cls_head_fwd,
    "ctgcn_cls_head_bwd_f32": _drive_cls_head_bwd,
    "ctgcn_sim_gram_f32": _drive_sim_gram,
    "ctgcn_ridge_gram_f32": _drive_ridge_gram,
    "ctgcn_ridge_sse_f32": _drive_ridge_sse,
    "ctgcn_sim_gram_f64": functools.partial(_drive_sim_gram, f64=True),
    "ctgcn_ridge_gram_f64": functools.partial(_drive_ridge_gram, f64=True),
    "ctgcn_ridge_sse_f64": functools.partial(_drive_ridge_sse, f64=True),
}


@pytest.mark.parametrize("fn,param,layout", cases(), ids=lambda v: str(v).replace("ctgcn_", ""))
def test_wide_operand(arena, fn, param, layout, monkeypatch):
    drive = DRIVERS[fn]
    code = getattr(drive, "func", drive).__code__
    if "monkeypatch" in code.co_varnames[: code.co_argcount]:
        drive(arena, param, layout, monkeypatch)
    else:
        drive(arena, param, layout)


def test_peak_device_memory_stays_under_32_gib(arena):
    """runs last in the module: the arena (24 GiB + 64 MiB) plus every case's small tensors"""
    peak = torch.cuda.max_memory_allocated()
    print("  peak device memory of the wide-offset module: %.2f GiB" % (peak / 2 ** 30))
    assert peak < 32 * (1 << 30)
