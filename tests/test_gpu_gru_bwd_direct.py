"""ctgcn_gru_bwd_rec_f32 and ctgcn_gru_bwd_in_f32 called directly (ctypes), under row plans the training chain never produces.

Exact tier: dyadic inputs for which the kernels' bf16 x 2 split MFMAs are exact (tests/_gru_bwd_ref.exact_case; the conditions are
asserted on the CPU by tests/test_gru_bwd_ref_host.py over EXACT_CASES below, so the exactness does not rest on the code under test):
d_gi, dx or Z / S0 and the block sums of the four weight / bias partial tables must equal the float64 model bit for bit; what the
contract says is not written (steps that are not fresh, rows past `rows`, output rows `order` does not name, partial rows past
ctgcn_gru_bwd_blocks(rows)) must keep its NaN prefill; the input side must not read a step that is not fresh (NaN there).
Cases by path:
  grid-*      rows = 150 (10 tiles, tail of 6) under ctgcn_set_persistent_cus 1 / 2 / 3 / 7 and the default grid: 10, 5/5, 4/3/3,
              2/2/2/1/1/1/1 tiles per block — the plane-buffer parity and the unit iterator across tiles, under every mask pattern
              (first-only, top-and-zero, nested-like with f = S and f = 1, alternating, random, neighbouring tiles first-only | all ones;
              past 32 steps: low word only, bits {0, 32}, {0, 31, 32}, {0, 63}), steps 1 2 3 31 32 33 63 64
  rows-*      rows 1 15 16 17 33 150 under 3 persistent blocks with a plan
  prod-*      rows x {no plan, random} x (dh_sum | dh_seq) x (3 | 4 gates) at 3 and 33 steps, the input-side forms rotating
  garbage-*   bits at and above `steps` set in the one- and two-word masks: ignored (include/ctgcn_hip.h)
Every case runs both entry points; the input side rotates through its four instantiations (planes | fp32 x) x (dx | Z): planes with
first_row 0 / 32 inside a larger plane_rows, fp32 x with ldx 128 / 132 / 256, Z with order NULL / a permutation into a larger n,
nested 0 / 1, S0 NULL / not; accumulate 0 / 1.

Numeric tier: random values (float32 numpy GRU forward, nn.GRU default weights, x = relu(randn) 1.5, dh ~ randn) against the float64
model on the same float32 operands; weight and bias sums at the rule of tests/test_gpu_gru.py::_check_grads (1e-5 of the tensor's
largest entry, or twice the float32 numpy model's error), per-row outputs at the same rule per SEQUENCE.
Measured on an MI355X (worst |err| / max|want| of a family over its 24 cases; per sequence for the per-row outputs):
  d_gi 1.7e-6   dx 8.8e-6   Z 9.0e-6   S0 9.0e-6   (all at 150 x 8, nested-like)        — 1e-5 per sequence holds: no family has its own bound
  dW_hh 4.1e-6 (150 x 8 random)   db_hh(n) 8.6e-7   dW_ih 7.2e-6 (33 x 64 nested-like)   db_ih 2.7e-6
  saturated, three gates, z-bias +6: d_gi |err| 2.8e-6 of scale 0.83 (four gates 8.8e-8); +30: every output exactly 0 in both forms.

Refusals: return codes, and nothing written.

Run time of this file on an MI355X: 11.5 s (205 tests; most of it is the model on the host).  DESIGN.md §4.8a lists the cases by path."""
import collections
import functools
import os

import numpy as np
import pytest
import torch

import _gru_bwd_ref as M

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(bool(os.environ.get("CTGCN_BWD_ABLATE")), reason="CTGCN_BWD_ABLATE is set: the library caches it, the kernels skip work")]
DEV = "cuda:0"
H, G3 = 128, 384
PAD = 2                      # rows behind `rows` in every per-row output: must stay NaN
SENT = 12345.625             # stands in for NaN when got and want are compared (positions and values in one torch.equal)
OK, E_INVALID, E_UNSUPPORTED = 0, -1, -4

ROWS = (1, 15, 16, 17, 33, 150)
STEPS = (1, 2, 3, 31, 32, 33, 63, 64)
GRIDS = (3, 1, 2, 7, 0)      # ctgcn_set_persistent_cus (0: the device's CUs, one tile per block)
NARROW = ("ones", "first-only", "top-and-zero", "nested-like", "alternating", "random", "first-then-ones")
WIDE = ("low-word-only", "b0-32", "b0-31-32")
REC_FORMS = ((4, False), (3, False), (4, True), (3, True))                       # (gate_count, dh per step)
X_FORMS = (("planes", 0, 128), ("f32", 0, 128), ("planes", 32, 128), ("f32", 0, 132), ("f32", 0, 256))      # (x, first_row, ldx)
OUT_FORMS = (("dx", False, 0, False), ("Z", False, 0, True), ("Z", True, 1, True), ("Z", True, 0, False), ("dx", False, 0, False),
             ("Z", False, 1, False), ("Z", True, 1, False))                       # (output, order, nested, S0)

Case = collections.namedtuple("Case", "name rows steps mask grid gc per_step x first_row ldx out order nested s0 accumulate garbage seed")


def _masks_for(steps):
    if steps < 2:
        return (None,)
    m = (None,) + NARROW
    if steps > 32:
        m += WIDE
    if steps == 64:
        m += ("b0-63",)
    if steps in (31, 63):      # the neighbours 32 / 64 carry the full list
        m = tuple(p for p in m if p in (None, "random", "nested-like", "top-and-zero", "alternating") + WIDE)
    return m


def _build_cases():
    out, i = [], 0

    def add(prefix, rows, steps, mask, grid, k, garbage=False, rec=None):
        gc, per_step = REC_FORMS[k % 4] if rec is None else rec
        x, first_row, ldx = X_FORMS[(k // 2) % 5]
        o, order, nested, s0 = OUT_FORMS[(k // 3) % 7]
        name = "%s-%dx%d-%s-cus%d-g%d%s-%s%s-%s%s" % (prefix, rows, steps, mask or "noplan", grid, gc, "seq" if per_step else "sum",
                                                      x, ("+%d" % first_row) if x == "planes" else ("/%d" % ldx),
                                                      o + ("-perm" if order else "") + ("-nested" if nested else "") + ("-S0" if s0 else ""),
                                                      "" if k % 3 else "-acc0")
        out.append(Case(name, rows, steps, mask, grid, gc, per_step, x, first_row, ldx, o, order, nested, s0, 1 if k % 3 else 0, garbage, 100 + len(out)))

    for steps in STEPS:                                     # every mask at every step count over 10 tiles, the grids rotating
        for mask in _masks_for(steps):
            add("grid", 150, steps, mask, GRIDS[i % 5], i)
            i += 1
    nontrivial = [p for p in NARROW + WIDE + ("b0-63",) if p != "ones"]
    for j in range(12):                                     # every row count, step count and mask under 3 persistent blocks with a plan
        steps = STEPS[1:][j % 7] if j < 7 else (64, 33, 63, 64, 2)[j - 7]
        pool = [p for p in nontrivial if p in _masks_for(steps)]
        mask = pool[j % len(pool)] if j != 7 else "b0-63"
        add("rows", ROWS[j % 6], steps, mask, 3, i)
        i += 1
    for steps in (3, 33):                                   # the full product over the small axes
        for rows in ROWS:
            for mask in (None, "random"):
                for f, rec in enumerate(REC_FORMS):
                    add("prod", rows, steps, mask, 3 if (rows + f) % 2 else 0, i, rec=rec)
                    i += 1
    for steps, rows in ((3, 33), (31, 150), (2, 17), (33, 33), (63, 17)):       # bits at and above `steps` are ignored
        add("garbage", rows, steps, "random", 3, i, garbage=True)
        i += 1
    return out


EXACT_CASES = _build_cases()


def exact_model(c, audit):
    """(inputs, want, mask bits) of an exact case"""
    bits = None if c.mask is None else M.make_masks(c.mask, c.rows, c.steps, seed=c.seed)
    n_out = c.rows + 7 if c.order else c.rows
    order = np.random.default_rng(c.seed).permutation(n_out)[: c.rows].astype(np.int32) if c.order else None
    t, want = M.exact_case(c.rows, c.steps, bits, c.gc, c.per_step, seed=c.seed, negatives=c.x == "f32", order=order, nested=c.nested,
                           self_loop=c.s0, zout=c.out == "Z", n_out=n_out, audit=audit)
    t["order"], t["n_out"] = order, n_out
    return t, want, bits


# ------------------------------------------------------------------------------------------------------------ fixtures
@pytest.fixture
def persistent_cus():
    """ctgcn_set_persistent_cus(n): the persistent kernels run n blocks that walk all tiles; back to the device's CUs afterwards"""
    from ctgcn_amd import _lib
    lib = _lib.load()
    try:
        yield lambda n: lib.ctgcn_set_persistent_cus(int(n))
    finally:
        lib.ctgcn_set_persistent_cus(0)


@pytest.fixture(autouse=True)
def _stop_after_a_device_fault():
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


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEV)


def _mask_dev(bits, steps, garbage_seed=None):
    return None if bits is None else torch.from_numpy(M.pack_masks(bits, steps, garbage_seed=garbage_seed).view(np.int32)).to(DEV)


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _eq(got, want64, what):
    """bit for bit, NaN positions included"""
    g = torch.nan_to_num(got.double().cpu(), nan=SENT)
    w = torch.nan_to_num(torch.from_numpy(np.asarray(want64, dtype=np.float64)), nan=SENT)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    if not torch.equal(g, w):
        bad = (g != w).nonzero()
        raise AssertionError("%s: %d of %d entries differ from the exact model; first at %s: got %r, want %r"
                             % (what, len(bad), g.numel(), bad[0].tolist(), float(g[tuple(bad[0])]), float(w[tuple(bad[0])])))


def _tables(blocks, n_partial, width, accumulate):
    """partial tables of n_partial rows: NaN, the first `blocks` rows zero if the call accumulates"""
    t = [_nan(n_partial, G3, H), _nan(n_partial, width)]
    if accumulate:
        for a in t:
            a[:blocks] = 0
    return t


def run_rec(lib, rows, steps, gc, gates, hseq, dh_sum, dh_seq, w_hh, tm, accumulate, tables=None, expect=OK):
    """one call on NaN-prefilled outputs; returns (d_gi [rows + PAD, steps, 384], dW partials, db_hn partials, blocks)"""
    blocks = lib.ctgcn_gru_bwd_blocks(rows)
    dgi = _nan(rows + PAD, steps, G3)
    dw, dbn = tables if tables is not None else _tables(blocks, blocks + 2, H, accumulate)
    rc = lib.ctgcn_gru_bwd_rec_f32(rows, steps, H, _p(gates), gc, _p(hseq), _p(dh_sum), _p(dh_seq), _p(w_hh), _p(tm), _p(dgi), _p(dw), _p(dbn),
                                   dw.shape[0], accumulate, _stream())
    assert rc == expect, (rc, lib.ctgcn_last_error())
    torch.cuda.synchronize()
    return dgi, dw, dbn, blocks


def run_inp(lib, rows, steps, dgi, w_ih, tm, planes, plane_rows, first_row, x, ldx, zout, n_out, s0, order, nested, accumulate, tables=None):
    blocks = lib.ctgcn_gru_bwd_blocks(rows)
    dx = None if zout else _nan(rows + PAD, steps, H)
    Z = _nan(n_out + PAD, steps, H) if zout else None
    S0 = _nan(n_out + PAD, H) if zout and s0 else None
    dw, dbi = tables if tables is not None else _tables(blocks, blocks + 2, G3, accumulate)
    rc = lib.ctgcn_gru_bwd_in_f32(rows, steps, H, _p(dgi), _p(w_ih), _p(tm), _p(planes), plane_rows, first_row, _p(x), ldx, _p(dx), _p(Z), _p(S0),
                                  _p(order), nested, _p(dw), _p(dbi), dw.shape[0], accumulate, _stream())
    assert rc == OK, (rc, lib.ctgcn_last_error())
    torch.cuda.synchronize()
    return dx, Z, S0, dw, dbi, blocks


def _x_operands(c, x, fresh, exact):
    """the x operand of the input side in the case's form, NaN at the row-steps that are not fresh (and in the padding columns of a wide
    ldx, and in every plane row outside the call's sequences); returns (planes, plane_rows, x tensor, ldx, the float32 values the kernel decodes)"""
    rows, steps = c.rows, c.steps
    if c.x == "planes":
        plane_rows = (c.first_row + rows) * steps + 5
        buf, dec = M.build_planes(x, plane_rows, c.first_row, exact=exact, seed=c.seed)
        buf = M.poison_planes(buf, plane_rows, c.first_row, fresh)
        return torch.from_numpy(buf).to(DEV), plane_rows, None, 0, dec
    xs = np.full((rows * steps, c.ldx), M.NAN, dtype=np.float32)
    xs[:, :H] = np.where(fresh.reshape(-1, 1), x.reshape(rows * steps, H), M.NAN)
    return None, 0, torch.from_numpy(xs).to(DEV), c.ldx, np.asarray(x, dtype=np.float32)


def _check_tables(dw, db, blocks, accumulate, what):
    assert torch.isnan(dw[blocks:]).all() and torch.isnan(db[blocks:]).all(), "%s: partial rows at and past ctgcn_gru_bwd_blocks(rows) were written" % what
    assert torch.isfinite(dw[:blocks]).all() and torch.isfinite(db[:blocks]).all(), "%s: accumulate = %d left a NaN in the block rows" % (what, accumulate)


# ---------------------------------------------------------------------------------------------------------- the exact tier
@pytest.mark.parametrize("c", EXACT_CASES, ids=lambda c: c.name)
def test_exact_case_equals_the_float64_model_bit_for_bit(c, persistent_cus):
    lib = _lib()
    t, want, bits = exact_model(c, audit=False)
    rows, steps = c.rows, c.steps
    fresh = M.fresh_matrix(bits, rows, steps)
    tm = _mask_dev(bits, steps, c.seed if c.garbage else None)
    if c.garbage:
        assert all(int(w) >> (steps % 32) for w in M.pack_masks(bits, steps, garbage_seed=c.seed)[(1 if steps > 32 else 0)::(2 if steps > 32 else 1)])
    persistent_cus(c.grid)
    ntiles = (rows + 15) // 16
    assert lib.ctgcn_gru_bwd_blocks(rows) == (min(ntiles, c.grid) if c.grid else ntiles)
    gates, hseq, w_hh, w_ih = _dev(t["gates_used"]), _dev(t["hseq"]), _dev(t["w_hh"]), _dev(t["w_ih"])
    dh_sum, dh_seq = (None, _dev(t["dh_seq"])) if c.per_step else (_dev(t["dh_sum"]), None)
    runs = [run_rec(lib, rows, steps, c.gc, gates, hseq, dh_sum, dh_seq, w_hh, tm, c.accumulate) for _ in range(2)]
    dgi, dw, dbn, blocks = runs[0]
    assert all(_same_bits(a, b) for a, b in zip(runs[0][:3], runs[1][:3])), "gru_bwd_rec: two calls differ"
    _eq(dgi[:rows], want["d_gi"], "d_gi")
    assert torch.isnan(dgi[rows:]).all(), "d_gi rows past `rows` were written"
    _check_tables(dw, dbn, blocks, c.accumulate, "gru_bwd_rec")
    _eq(dw[:blocks].sum(0), want["dW_hh"], "dW_hh")
    _eq(dbn[:blocks].sum(0), want["db_hn"], "db_hn")

    # the input side on the MODEL's d_gi (NaN at the steps that are not fresh), x NaN there too
    planes, plane_rows, x, ldx, _ = _x_operands(c, t["x"], fresh, exact=True)
    order = _dev(t["order"], torch.int32) if c.order else None
    dgi_in = _dev(want["d_gi"])
    runs = [run_inp(lib, rows, steps, dgi_in, w_ih, tm, planes, plane_rows, c.first_row, x, ldx, c.out == "Z", t["n_out"], c.s0, order, c.nested,
                    c.accumulate) for _ in range(2)]
    dx, Z, S0, dw, dbi, blocks = runs[0]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert (a is None and b is None) or _same_bits(a, b), "gru_bwd_in: two calls differ"
    if c.out == "Z":
        _eq(Z[: t["n_out"]], want["Z"], "Z")
        assert torch.isnan(Z[t["n_out"]:]).all()
        if c.s0:
            _eq(S0[: t["n_out"]], want["S0"], "S0")
            assert torch.isnan(S0[t["n_out"]:]).all()
    else:
        _eq(dx[:rows], want["dx"], "dx")
        assert torch.isnan(dx[rows:]).all(), "dx rows past `rows` were written"
    _check_tables(dw, dbi, blocks, c.accumulate, "gru_bwd_in")
    _eq(dw[:blocks].sum(0), want["dW_ih"], "dW_ih")
    _eq(dbi[:blocks].sum(0), want["db_ih"], "db_ih")


@pytest.mark.parametrize("rows,steps,grid", [(150, 3, 3), (33, 32, 0), (150, 33, 2), (17, 64, 3)])
def test_explicit_all_ones_plan_is_bit_identical_to_no_plan_and_accumulation_doubles(rows, steps, grid, persistent_cus):
    """every output of both entry points: tile_mask of all ones against NULL; and with accumulate = 1 on zeroed tables two calls leave
    exactly twice one call's partials (the exact tier's sums are exact in any order)"""
    lib = _lib()
    c = Case("ones", rows, steps, "ones", grid, 4, False, "f32", 0, 128, "Z", False, 1, True, 1, False, 7)
    t, want, bits = exact_model(c, audit=False)
    persistent_cus(grid)
    gates, hseq, w_hh, w_ih, dh = _dev(t["gates_used"]), _dev(t["hseq"]), _dev(t["w_hh"]), _dev(t["w_ih"]), _dev(t["dh_sum"])
    x = _dev(t["x"].reshape(rows * steps, H))
    tm = _mask_dev(bits, steps)
    a = run_rec(lib, rows, steps, 4, gates, hseq, dh, None, w_hh, tm, 0)
    b = run_rec(lib, rows, steps, 4, gates, hseq, dh, None, w_hh, None, 0)
    assert all(_same_bits(u, v) for u, v in zip(a[:3], b[:3]))
    _eq(a[0][:rows], want["d_gi"], "d_gi")
    ai = run_inp(lib, rows, steps, a[0], w_ih, tm, None, 0, 0, x, H, True, rows, True, None, 1, 0)
    bi = run_inp(lib, rows, steps, a[0], w_ih, None, None, 0, 0, x, H, True, rows, True, None, 1, 0)
    assert all(_same_bits(u, v) for u, v in zip(ai[1:5], bi[1:5]))
    _eq(ai[1][:rows], want["Z"], "Z")
    # accumulate = 1
    blocks = a[3]
    tabs = _tables(blocks, blocks + 2, H, 1)
    for _ in range(2):
        run_rec(lib, rows, steps, 4, gates, hseq, dh, None, w_hh, tm, 1, tables=tabs)
    assert torch.equal(tabs[0][:blocks], 2 * a[1][:blocks]) and torch.equal(tabs[1][:blocks], 2 * a[2][:blocks])
    assert torch.isnan(tabs[0][blocks:]).all() and torch.isnan(tabs[1][blocks:]).all()
    tabs = _tables(blocks, blocks + 2, G3, 1)
    for _ in range(2):
        run_inp(lib, rows, steps, a[0], w_ih, tm, None, 0, 0, x, H, True, rows, True, None, 1, 1, tables=tabs)
    assert torch.equal(tabs[0][:blocks], 2 * ai[3][:blocks]) and torch.equal(tabs[1][:blocks], 2 * ai[4][:blocks])
    assert torch.isnan(tabs[0][blocks:]).all() and torch.isnan(tabs[1][blocks:]).all()


# -------------------------------------------------------------------------------------------------------- the numeric tier
@functools.lru_cache(maxsize=None)
def _numeric_inputs(rows, steps, mask, z_bias=0.0):
    """float32 operands: x = relu(randn) 1.5 (a step that is not fresh repeats the row before it), nn.GRU's default weights, gates and
    hseq of the float32 numpy forward, dh ~ randn"""
    torch.manual_seed(31 * rows + steps)
    rnn = torch.nn.GRU(H, H, 1, batch_first=True)
    w_ih, w_hh, b_ih, b_hh = (p.detach().numpy().copy() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0))
    b_ih[H:2 * H] += z_bias
    bits = None if mask is None else M.make_masks(mask, rows, steps, seed=steps)
    fresh = M.fresh_matrix(bits, rows, steps)
    x = (torch.relu(torch.randn(rows, steps, H)) * 1.5).numpy()
    src = np.maximum.accumulate(np.where(fresh, np.arange(steps)[None, :], 0), 1)
    x = np.take_along_axis(x, src[:, :, None], 1)
    gates, hseq = M.forward(x, w_ih, w_hh, b_ih, b_hh, dtype=np.float32)
    return {"x": x, "w_ih": w_ih, "w_hh": w_hh, "gates": gates, "hseq": hseq, "bits": bits, "fresh": fresh,
            "dh_sum": torch.randn(rows, H).numpy(), "dh_seq": torch.randn(rows, steps, H).numpy()}


WORST = collections.defaultdict(float)         # family -> worst |err| / max|want| seen in this process (printed per case)


def _tensor_rule(what, family, got, want64, want32, bound=1e-5):
    """_check_grads of tests/test_gpu_gru.py"""
    a, b, c = got.double().cpu().numpy(), want64, want32.astype(np.float64)
    scale = max(1e-30, float(np.abs(b).max()))
    err, err32 = float(np.abs(a - b).max()) / scale, float(np.abs(c - b).max()) / scale
    WORST[family] = max(WORST[family], err)
    print("  [tol] %s %-6s |err| / max|want| %.3e  fp32 numpy %.3e  (limit %.1e; family worst %.3e)" % (what, family, err, err32, max(bound, 2 * err32), WORST[family]))
    assert err <= max(bound, 2.0 * err32), (what, family, err, err32)


def _sequence_rule(what, family, got, want64, want32, bound=1e-5):
    """the same rule per sequence (leading axis): the largest error over a sequence's written steps and columns against that sequence's own
    largest entry; entries the model leaves unwritten (NaN) must be NaN"""
    a, b, c = got.double().cpu().numpy(), want64, want32.astype(np.float64)
    assert np.array_equal(np.isnan(a), np.isnan(b)), "%s %s: written where the model does not write, or the reverse" % (what, family)
    n = a.shape[0]
    a, b, c = (np.nan_to_num(v).reshape(n, -1) for v in (a, b, c))
    scale = np.maximum(1e-30, np.abs(b).max(1))
    err, err32 = np.abs(a - b).max(1) / scale, np.abs(c - b).max(1) / scale
    live = np.abs(b).max(1) > 0
    share = float(err[live].max()) if live.any() else 0.0
    over = err / np.maximum(bound, 2 * err32)
    WORST[family] = max(WORST[family], share)
    print("  [tol] %s %-6s per sequence: worst |err| / max|want_seq| %.3e  (fp32 numpy there %.3e; worst err / limit %.3f; family worst %.3e)"
          % (what, family, share, float(err32[live][err[live].argmax()]) if live.any() else 0.0, float(over.max()), WORST[family]))
    assert (err <= np.maximum(bound, 2.0 * err32)).all(), (what, family, share, float(over.max()))


def _numeric_rec(lib, t, rows, steps, gc, per_step, tm):
    gates = t["gates"] if gc == 4 else t["gates"][:, :, [0, 1, 3]]
    kw = {"dh_seq": t["dh_seq"]} if per_step else {"dh_sum": t["dh_sum"]}
    want64 = M.rec(gates, gc, t["hseq"], t["w_hh"], t["bits"], steps, **kw)
    want32 = M.rec(gates, gc, t["hseq"], t["w_hh"], t["bits"], steps, dtype=np.float32, **kw)
    runs = [run_rec(lib, rows, steps, gc, _dev(gates), _dev(t["hseq"]), None if per_step else _dev(t["dh_sum"]), _dev(t["dh_seq"]) if per_step else None,
                    _dev(t["w_hh"]), tm, 0) for _ in range(2)]
    assert all(_same_bits(a, b) for a, b in zip(runs[0][:3], runs[1][:3])), "gru_bwd_rec: two calls differ"
    return runs[0], want64, want32


@pytest.mark.parametrize("xform", ["planes-Z", "f32-dx"])
@pytest.mark.parametrize("grid", [0, 3])
@pytest.mark.parametrize("mask", ["random", "nested-like"])
@pytest.mark.parametrize("rows,steps", [(150, 8), (150, 33), (33, 64)])
def test_random_values_against_the_float64_model(rows, steps, mask, grid, xform, persistent_cus):
    """planes-Z: three gates, dh_sum, Z / S0 with a row map (the CoreDiffusion chain's forms); f32-dx: four gates, dh per step, dx"""
    lib = _lib()
    t = _numeric_inputs(rows, steps, mask)
    planes_form = xform == "planes-Z"
    gc, per_step = (3, False) if planes_form else (4, True)
    what = "%dx%d %s cus%d %s" % (rows, steps, mask, grid, xform)
    persistent_cus(grid)
    tm = _mask_dev(t["bits"], steps)
    (dgi, dw, dbn, blocks), want64, want32 = _numeric_rec(lib, t, rows, steps, gc, per_step, tm)
    assert torch.isnan(dgi[rows:]).all() and torch.isnan(dw[blocks:]).all() and torch.isnan(dbn[blocks:]).all()
    _sequence_rule(what, "d_gi", dgi[:rows], want64[0], want32[0])
    _tensor_rule(what, "dW_hh", dw[:blocks].sum(0), want64[1], want32[1])
    _tensor_rule(what, "db_hn", dbn[:blocks].sum(0), want64[2], want32[2])
    # the input side consumes the kernel's own float32 d_gi, and so does the model
    c = Case(what, rows, steps, mask, grid, gc, per_step, "planes" if planes_form else "f32", 16 if planes_form else 0, 128 if planes_form else 132,
             "Z" if planes_form else "dx", planes_form, 1 if mask == "nested-like" else 0, True, 0, False, rows + steps)
    planes, plane_rows, x, ldx, xdec = _x_operands(c, t["x"], t["fresh"], exact=False)
    n_out = rows + 7 if planes_form else rows
    order = np.random.default_rng(5).permutation(n_out)[:rows].astype(np.int32) if planes_form else None
    dgi_np = dgi[:rows].cpu().numpy()
    kw = dict(order=order, nested=c.nested, self_loop=True, zout=planes_form, n_out=n_out)
    w64 = M.inp(dgi_np, t["w_ih"], t["bits"], xdec, steps, **kw)
    w32 = M.inp(dgi_np, t["w_ih"], t["bits"], xdec, steps, dtype=np.float32, **kw)
    runs = [run_inp(lib, rows, steps, dgi, _dev(t["w_ih"]), tm, planes, plane_rows, c.first_row, x, ldx, planes_form, n_out, True,
                    _dev(order, torch.int32), c.nested, 0) for _ in range(2)]
    dx, Z, S0, dw, dbi, blocks = runs[0]
    for a, b in zip(runs[0][:5], runs[1][:5]):
        assert (a is None and b is None) or _same_bits(a, b), "gru_bwd_in: two calls differ"
    if planes_form:
        _sequence_rule(what, "Z", Z[:n_out], w64["Z"], w32["Z"])
        _sequence_rule(what, "S0", S0[:n_out], w64["S0"], w32["S0"])
        assert torch.isnan(Z[n_out:]).all() and torch.isnan(S0[n_out:]).all()
    else:
        _sequence_rule(what, "dx", dx[:rows], w64["dx"], w32["dx"])
        assert torch.isnan(dx[rows:]).all()
    assert torch.isnan(dw[blocks:]).all() and torch.isnan(dbi[blocks:]).all()
    _tensor_rule(what, "dW_ih", dw[:blocks].sum(0), w64["dW"], w32["dW"])
    _tensor_rule(what, "db_ih", dbi[:blocks].sum(0), w64["db"], w32["db"])


@pytest.mark.parametrize("z_bias", [6.0, 30.0])
def test_saturated_update_gate_in_the_three_gate_form(z_bias):
    """z-bias + 6 / + 30 (z = 0.9975 / exactly 1.0f): n rebuilt from h_t, h_{t-1}, z must stay finite and no worse than the four-gate call
    on the same inputs (the path that stores n), at the rule of test_fused_training_with_saturated_update_gate: relative to the tensor's
    largest entry, with the absolute floor of 1e-7"""
    lib = _lib()
    rows, steps = 150, 8
    t = _numeric_inputs(rows, steps, "random", z_bias)
    tm = _mask_dev(t["bits"], steps)
    (g3, dw3, db3, blocks), _, _ = _numeric_rec(lib, t, rows, steps, 3, False, tm)
    (g4, dw4, db4, _), want, _ = _numeric_rec(lib, t, rows, steps, 4, False, tm)
    for name, a3, a4, w in (("d_gi", g3[:rows], g4[:rows], want[0]), ("dW_hh", dw3[:blocks].sum(0), dw4[:blocks].sum(0), want[1]),
                            ("db_hn", db3[:blocks].sum(0), db4[:blocks].sum(0), want[2])):
        a3, a4 = a3.double().cpu().numpy(), a4.double().cpu().numpy()
        assert np.array_equal(np.isnan(a3), np.isnan(w)) and np.isfinite(a3[~np.isnan(w)]).all(), name
        a3, a4, w = np.nan_to_num(a3), np.nan_to_num(a4), np.nan_to_num(w)
        scale, e_new, e_old = float(np.abs(w).max()), float(np.abs(a3 - w).max()), float(np.abs(a4 - w).max())
        print("  [tol] z-bias %+.0f %-6s three gates |err| %.3e  four gates %.3e  scale %.3e" % (z_bias, name, e_new, e_old, scale))
        assert e_new <= max(1e-4 * scale, 3.0 * e_old) + 1e-7, (name, e_new, e_old, scale)


# ---------------------------------------------------------------------------------------------------------------- refusals
def _refusal_operands():
    rows, steps = 20, 4
    f = lambda *s: torch.zeros(*s, device=DEV)
    blocks = _lib().ctgcn_gru_bwd_blocks(rows)
    ins = {"gates": f(rows, steps, 4, H), "h_seq": f(rows, steps, H), "dh_sum": f(rows, H), "dh_seq": f(rows, steps, H), "w": f(G3, H),
           "d_gi_in": f(rows, steps, G3), "x": f(rows * steps, 256), "planes": torch.zeros((40 * steps) * (4 * H + 4) + 64, dtype=torch.uint8, device=DEV)}
    outs = {"d_gi": _nan(rows, steps, G3), "dw": _nan(blocks, G3, H), "dbn": _nan(blocks, H), "dbi": _nan(blocks, G3), "dx": _nan(rows, steps, H),
            "Z": _nan(rows, steps, H), "S0": _nan(rows, H)}
    return rows, steps, blocks, ins, outs


def _rec_args(base, i, o, **kw):
    rows, steps, blocks = base
    a = dict(rows=rows, steps=steps, hidden=H, gates=_p(i["gates"]), gate_count=4, h_seq=_p(i["h_seq"]), dh_sum=_p(i["dh_sum"]), dh_seq=None,
             w_hh=_p(i["w"]), tile_mask=None, d_gi=_p(o["d_gi"]), dw=_p(o["dw"]), dbn=_p(o["dbn"]), n_partial=blocks, accumulate=0)
    a.update(kw)
    return list(a.values()) + [_stream()]


def _in_args(base, i, o, **kw):
    rows, steps, blocks = base
    a = dict(rows=rows, steps=steps, hidden=H, d_gi=_p(i["d_gi_in"]), w_ih=_p(i["w"]), tile_mask=None, x_planes=None, plane_rows=0, first_row=0,
             x=_p(i["x"]), ldx=128, dx=_p(o["dx"]), Z=None, S0=None, order=None, nested=0, dw=_p(o["dw"]), dbi=_p(o["dbi"]), n_partial=blocks,
             accumulate=0)
    a.update(kw)
    return list(a.values()) + [_stream()]


def test_refusals_return_the_error_and_write_nothing():
    lib = _lib()
    rows, steps, blocks, i, o = _refusal_operands()
    base = (rows, steps, blocks)
    off = lambda t: _p(t, 4)
    planes = dict(x=None, ldx=0, x_planes=_p(i["planes"]), plane_rows=40 * steps, first_row=16)
    rec_bad = [("hidden 64", E_UNSUPPORTED, dict(hidden=64)), ("steps 0", E_INVALID, dict(steps=0)), ("steps 65", E_INVALID, dict(steps=65)),
               ("gate_count 2", E_INVALID, dict(gate_count=2)), ("dh_sum and dh_seq", E_INVALID, dict(dh_seq=_p(i["dh_seq"]))),
               ("neither dh", E_INVALID, dict(dh_sum=None)), ("n_partial", E_INVALID, dict(n_partial=blocks - 1))]
    rec_bad += [("%s 4 bytes off" % k, E_INVALID, {k: off(t)}) for k, t in (("gates", i["gates"]), ("h_seq", i["h_seq"]), ("dh_sum", i["dh_sum"]),
                                                                          ("d_gi", o["d_gi"]), ("dw", o["dw"]), ("dbn", o["dbn"]))]
    rec_bad.append(("dh_seq 4 bytes off", E_INVALID, dict(dh_sum=None, dh_seq=off(i["dh_seq"]))))
    for what, code, kw in rec_bad:
        assert lib.ctgcn_gru_bwd_rec_f32(*_rec_args(base, i, o, **kw)) == code, ("gru_bwd_rec", what, lib.ctgcn_last_error())
    in_bad = [("hidden 64", E_UNSUPPORTED, dict(hidden=64)), ("steps 0", E_INVALID, dict(steps=0)), ("steps 65", E_INVALID, dict(steps=65)),
              ("x and planes", E_INVALID, dict(planes, x=_p(i["x"]), ldx=128)), ("neither x", E_INVALID, dict(x=None)),
              ("dx and Z", E_INVALID, dict(Z=_p(o["Z"]))), ("neither dx nor Z", E_INVALID, dict(dx=None)),
              ("ldx 124", E_INVALID, dict(ldx=124)), ("ldx 130", E_INVALID, dict(ldx=130)),
              ("first_row 8", E_INVALID, dict(planes, first_row=8)),
              ("plane_rows one short", E_INVALID, dict(planes, plane_rows=(16 + rows) * steps - 1)),
              ("n_partial", E_INVALID, dict(n_partial=blocks - 1)),
              ("planes 4 bytes off", E_INVALID, dict(planes, x_planes=off(i["planes"]))),
              ("Z 4 bytes off", E_INVALID, dict(dx=None, Z=off(o["Z"]))), ("S0 4 bytes off", E_INVALID, dict(dx=None, Z=_p(o["Z"]), S0=off(o["S0"])))]
    in_bad += [("%s 4 bytes off" % k, E_INVALID, {k: off(t)}) for k, t in (("d_gi", i["d_gi_in"]), ("x", i["x"]), ("dx", o["dx"]), ("dw", o["dw"]),
                                                                         ("dbi", o["dbi"]))]
    for what, code, kw in in_bad:
        assert lib.ctgcn_gru_bwd_in_f32(*_in_args(base, i, o, **kw)) == code, ("gru_bwd_in", what, lib.ctgcn_last_error())
    # the complement: the same operands are accepted once nothing is wrong (planes with exactly enough rows), checked last
    assert blocks == 2 and lib.ctgcn_gru_bwd_blocks(0) == 1
    assert lib.ctgcn_gru_bwd_rec_f32(*_rec_args(base, i, o, rows=0)) == OK           # rows = 0: fine, and nothing is written
    assert lib.ctgcn_gru_bwd_in_f32(*_in_args(base, i, o, rows=0)) == OK
    assert lib.ctgcn_gru_bwd_in_f32(*_in_args(base, i, o, **dict(planes, rows=0, plane_rows=16 * steps))) == OK
    torch.cuda.synchronize()
    for k, t in o.items():
        assert torch.isnan(t).all(), "%s was written by a refused call" % k
    assert lib.ctgcn_gru_bwd_in_f32(*_in_args(base, i, o, **dict(planes, plane_rows=(16 + rows) * steps))) == OK
    torch.cuda.synchronize()
    assert torch.isfinite(o["dx"]).all()
