"""The CoreDiffusion aggregation kernels (agg_fwd_kernel, agg_bwd_kernel, agg_bwd_prep_kernel, the hub kernels, agg_hub_final_kernel) against
the float64 model of _agg_ref.py, at forced row lengths, slot layouts and every launch branch (_agg_cases.py).

Every case runs two tiers.  exact: inputs whose partial sums are all exact in fp32 (the host test checks the 2^24 condition) — the kernels
must equal the model bit for bit, H, Z, S0 and dX.  rounded: normal inputs, |error| <= gamma_k T per element, from the inputs alone.
Both repeat every call (bit-identical) and run the backward on the MODEL's H, so that the relu mask is the test's and not a near-tie's."""
import numpy as np
import pytest
import torch

import _agg_cases as C
import _agg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
worst = {}                                  # worst used fraction of the rounded tier, per result


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)


def _x_tensor(case, x):
    if not case.strided:
        return _t(x)
    buf = torch.full((case.n, case.d + 5), float("nan"), device=DEV)       # columns 1..d: odd row stride, base 4 bytes off 16
    buf[:, 1:case.d + 1] = _t(x)
    return buf[:, 1:case.d + 1]


def _prep(H, dH, nested, relu, with_s0):
    from ctgcn_amd import _lib
    lib = _lib.load()
    n, K, d = dH.shape
    flags = (_lib.F_NESTED if nested else 0) | (_lib.F_RELU if relu else 0) | (_lib.F_SELF_LOOP if with_s0 else 0)
    Z = torch.full_like(dH, float("nan"))
    S0 = torch.full((n, d), float("nan"), device=dH.device) if with_s0 else None
    _lib.check(lib.ctgcn_core_aggregate_bwd_prep_f32(n, d, K, _lib.ptr(dH), _lib.ptr(H), _lib.ptr(Z), _lib.ptr(S0), flags,
                                                     torch.cuda.current_stream().cuda_stream), "ctgcn_core_aggregate_bwd_prep_f32")
    return Z, S0


def _compare(case, tier, name, got, res):
    got = got.detach().cpu().numpy()
    assert np.isfinite(got).all(), (case, tier, name)
    if tier == "exact":
        assert torch.equal(torch.from_numpy(got), torch.from_numpy(res.value.astype(np.float32))), \
            "%s %s: %d of %d elements differ from the model" % (case, name, (got != res.value).sum(), got.size)
    else:
        used = res.used(got, case.K)
        worst[name] = max(worst.get(name, 0.0), used)
        print("  [bound] %-50s %-3s %.3f of gamma T" % (case, name, used))
        assert used <= 1.0, "%s %s: %.3f x the bound" % (case, name, used)


def _run(case, autograd=False):
    from ctgcn_amd import CoreAdj, ops
    old = CoreAdj.LONG_ROW
    try:
        if case.long_row is not None:
            CoreAdj.LONG_ROW = case.long_row
        for tier in ("exact", "rounded"):
            mats, x, dH, model = (C.exact_inputs(case) if tier == "exact" else C.rounded_inputs(case))[:4]
            adj = CoreAdj.from_matrices([m.astype(np.float32) for m in mats], self_loop=case.self_loop, device=DEV)
            assert (adj.K, adj.n, adj.nested) == (case.K, case.n, model["nested"])
            if case.symmetric is not None:
                assert adj.symmetric == case.symmetric
            # which path runs, through what the API exposes
            hubs, hubs_t = adj.long_rows(), adj.long_rows(transposed=True)
            count = lambda t: 0 if t is None else t.numel()
            if case.long_row is None and not case.expect:
                assert hubs is None and hubs_t is None
            for key, got in (("hubs", count(hubs)), ("hubs_t", count(hubs_t)), ("split", adj.hub_split()), ("split_t", adj.hub_split(True))):
                if key in case.expect:
                    assert got == case.expect[key], (case, key, got)
            xt, dHt = _x_tensor(case, x), _t(dH)
            H = ops._aggregate_fwd(adj, xt, case.relu)
            assert torch.equal(ops._aggregate_fwd(adj, xt, case.relu), H), "forward not repeatable"
            _compare(case, tier, "H", H, model["H"])
            Hm = _t(model["H"].value)                      # the model's H rounded to fp32: its sign pattern is the mask
            Z, S0 = _prep(Hm, dHt, adj.nested, case.relu, adj.self_loop)
            _compare(case, tier, "Z", Z, model["Z"])
            if adj.self_loop:
                _compare(case, tier, "S0", S0, model["S0"])
            dX = ops._aggregate_bwd(adj, Hm, dHt, case.relu)
            assert torch.equal(ops._aggregate_bwd(adj, Hm, dHt, case.relu), dX), "backward not repeatable"
            _compare(case, tier, "dX", dX, model["dX"])
            if autograd and tier == "exact":               # end to end: the kernels' own H (bit-equal to the model's) is the mask
                xg = _x_tensor(case, x).clone().requires_grad_(True)
                Hg = ops.core_aggregate(xg, adj, relu=case.relu)
                (Hg * dHt).sum().backward()
                _compare(case, tier, "H", Hg, model["H"])
                _compare(case, tier, "dX", xg.grad, model["dX"])
    finally:
        CoreAdj.LONG_ROW = old


def _ids(group):
    return dict(argvalues=C.cases(group), ids=[c.id for c in C.cases(group)])


@pytest.mark.parametrize("case", **_ids("widths"))
def test_row_kernels_at_every_width(case):
    _run(case)


@pytest.mark.parametrize("case", **_ids("layouts"))
def test_row_kernels_at_every_slot_layout(case):
    _run(case)


@pytest.mark.parametrize("case", **_ids("flags"))
def test_flag_combinations_and_autograd(case):
    _run(case, autograd=True)


@pytest.mark.parametrize("case", **_ids("slots"))
def test_slot_counts(case):
    _run(case)


@pytest.mark.parametrize("case", **_ids("hub_threshold"))
def test_hub_kernels_at_low_thresholds(case):
    _run(case)


@pytest.mark.parametrize("case", **_ids("hub_groups"))
def test_hub_group_counts_and_fallback(case):
    _run(case)


@pytest.mark.parametrize("case", **_ids("hub_pieces"))
def test_hub_rows_in_pieces(case):
    from ctgcn_amd import _lib
    assert int(_lib.load().ctgcn_hub_split_entries()) == C.HUB_SPLIT_ENTRIES
    _run(case)


@pytest.mark.parametrize("d,vec4,strided", C.SPMM_CASES)
def test_spmm_csr_is_the_row_kernel_at_one_slot(d, vec4, strided):
    """ctgcn_spmm_csr_f32: K = 1, null slot pointer; accumulate off and on; out as a column slice (ldy > d) whose neighbours stay untouched"""
    from ctgcn_amd import ops
    case = C.spmm_case(d, vec4, strided)
    for tier in ("exact", "rounded"):
        mats, x, dH, model = (C.exact_inputs(case) if tier == "exact" else C.rounded_inputs(case))[:4]
        m = mats[0].tocsr()
        m.sort_indices()
        rp, col, val = (torch.from_numpy(a).to(DEV) for a in (m.indptr.astype(np.int32), m.indices.astype(np.int32), m.data.astype(np.float32)))
        xt = _x_tensor(case, x)
        y = ops.spmm_csr(rp, col, val, xt)
        H = model["H"]
        flat = R.Result(H.value[:, 0], H.T[:, 0], H.m)
        _compare(case, tier, "Y", y, flat)
        y0 = np.random.default_rng(d).integers(-8, 9, (case.n, d)) * 0.25
        for accumulate in (False, True):
            lead = 4 if vec4 else 3                        # float4: the slice keeps its 16-byte alignment, ldy = d + 8
            buf = torch.full((case.n, d + (8 if vec4 else 5)), 7.0, device=DEV)
            out = buf[:, lead:lead + d]
            out.copy_(_t(y0))
            for _ in range(2):                             # the repeat: from the same start, bit-identical
                out.copy_(_t(y0))
                got = ops.spmm_csr(rp, col, val, xt, out=out, accumulate=accumulate)
                assert got.data_ptr() == out.data_ptr()
                want = R.Result(flat.value + (y0 if accumulate else 0), flat.T + (np.abs(y0) if accumulate else 0), flat.m + 1)
                _compare(case, tier, "Y+" if accumulate else "Y", out, want)
            assert (buf[:, :lead] == 7.0).all() and (buf[:, lead + d:] == 7.0).all()


@pytest.mark.parametrize("d,K", C.PREP_CASES)
def test_bwd_prep_kernel_directly(d, K):
    """agg_bwd_prep_kernel: float4 (d = 8) and scalar (d = 5), K = 1 .. 255, nested / general, relu on / off, with and without S0; H holds
    exact +0.0 beside positive entries, and every masked entry has a non-zero gradient"""
    for nested in (True, False):
        for relu in (True, False):
            H, dH, Z, S0 = C.prep_exact(d, K, nested, relu)
            Hr, dHr = C.prep_inputs(d, K, None)
            Zr, S0r = R.backward_prep(Hr, dHr, nested, relu)
            case = "prep-d%d-K%d-%s-%s" % (d, K, "nested" if nested else "general", "relu" if relu else "linear")
            for with_s0 in (True, False):
                for tier, (h, g, z, s) in (("exact", (H, dH, Z, S0)), ("rounded", (Hr, dHr, Zr, S0r))):
                    ht, gt = _t(h), _t(g)
                    gz, gs = _prep(ht, gt, nested, relu, with_s0)
                    gz2, gs2 = _prep(ht, gt, nested, relu, with_s0)
                    assert torch.equal(gz, gz2) and (gs is None or torch.equal(gs, gs2))
                    kc = type("K", (), dict(K=K, __repr__=lambda self: case))()
                    _compare(kc, tier, "Z", gz, z)
                    if with_s0:
                        _compare(kc, tier, "S0", gs, s)
                    else:
                        assert gs is None
            if not relu:                                   # H may be null without the relu flag
                gz, _ = _prep(None, _t(dH), nested, False, False)
                assert torch.equal(gz.cpu(), torch.from_numpy(Z.value.astype(np.float32)))


def test_empty_graph_and_hub_workspace_refusals():
    """n = 0 returns before anything is launched; set_hub_pieces refuses a split above 64, a short and a misaligned workspace — with the
    error code, nothing launched, the output untouched"""
    from ctgcn_amd import _lib
    lib = _lib.load()
    n, d, K = 5, 4, 2
    rp = torch.tensor([0, 3, 3, 3, 3, 3], dtype=torch.int32, device=DEV)
    col = torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV)
    val = torch.ones(3, device=DEV)
    slot = torch.tensor([0, 1, 1], dtype=torch.uint8, device=DEV)
    long_rows = torch.zeros(1, dtype=torch.int32, device=DEV)
    x = torch.ones(n, d, device=DEV)
    H = torch.full((n, K, d), 7.0, device=DEV)
    dX = torch.full((n, d), 7.0, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    p, st = _lib.ptr, torch.cuda.current_stream().cuda_stream
    need = int(lib.ctgcn_hub_workspace_bytes(1, 2, K, d))
    assert need == 1 * 2 * K * d * 4 and int(lib.ctgcn_hub_workspace_bytes(1, 1, K, d)) == 0

    def fwd(rows, split, wsp, nbytes):
        return lib.ctgcn_core_aggregate_f32(rows, d, K, p(rp), p(col), p(val), p(slot), p(x), d, p(H), _lib.F_NESTED, p(long_rows), 1, 2,
                                            split, wsp, nbytes, st)

    def bwd(rows, split, wsp, nbytes):
        return lib.ctgcn_core_aggregate_bwd_f32(rows, d, K, p(rp), p(col), p(val), p(slot), p(H), None, p(dX), d, _lib.F_NESTED, p(long_rows), 1,
                                                2, split, wsp, nbytes, st)
    for call in (fwd, bwd):
        assert call(0, 2, p(ws), 4096) == 0                                            # no rows: OK, nothing to do
        assert call(n, 65, p(ws), 4096) == -1 and b"hub_split" in lib.ctgcn_last_error()
        assert call(n, 2, p(ws), 8) == -3                                              # CTGCN_E_WORKSPACE: too small
        assert call(n, 2, p(ws) + 4, 4092) == -3                                       # ... and not 16-byte aligned
    assert lib.ctgcn_spmm_csr_f32(0, d, p(rp), p(col), p(val), p(x), d, p(dX), d, 0, st) == 0
    assert lib.ctgcn_core_aggregate_bwd_prep_f32(0, d, K, p(x), p(x), p(x), None, 0, st) == 0
    torch.cuda.synchronize()
    assert (H == 7.0).all() and (dX == 7.0).all()


def test_worst_used_fraction_is_reported():
    """runs last in the file: the rounded tier's worst use of its bound, per result (DESIGN.md 4.3a quotes it)"""
    for name in sorted(worst):
        print("  [bound] worst over the file: %-3s %.3f of gamma T" % (name, worst[name]))
    assert all(v <= 1.0 for v in worst.values())
