"""The float64 model of the fused GRU backward (tests/_gru_bwd_ref.py) pinned on the CPU: against float64 torch autograd of nn.GRU(128, 128)
without a plan and under a plan whose repeated steps really repeat x; its Z / S0 epilogue against a direct evaluation of the suffix sums;
and the exactness conditions of every exact case tests/test_gpu_gru_bwd_direct.py runs (the GPU test's bit-for-bit claim rests on this
file, not on the kernels)."""
import numpy as np
import pytest
import torch

import _gru_bwd_ref as M
import test_gpu_gru_bwd_direct as T
import test_gpu_wide_offsets as WT

H = 128


def _close(name, got, want, rtol=1e-12):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    err = float(np.abs(got - want).max()) / max(1e-300, float(np.abs(want).max()))
    assert err <= rtol, (name, err)


def _autograd(rows, steps, mask_bits, per_step, seed):
    """float64 nn.GRU; x of a step that is not fresh IS the row of the fresh step before it (one shared leaf per group)"""
    torch.manual_seed(seed)
    rnn = torch.nn.GRU(H, H, 1, batch_first=True).double()
    fresh = M.fresh_matrix(mask_bits, rows, steps)
    src = np.maximum.accumulate(np.where(fresh, np.arange(steps)[None, :], 0), 1)
    leaf = (torch.relu(torch.randn(rows, steps, H, dtype=torch.float64)) * 1.5).requires_grad_(True)
    x = torch.gather(leaf, 1, torch.from_numpy(src)[:, :, None].expand(rows, steps, H))
    G = torch.randn((rows, steps, H) if per_step else (rows, H), dtype=torch.float64)
    h = rnn(x)[0]
    ((h if per_step else h.sum(1)) * G).sum().backward()
    p = {k: v.detach().numpy() for k, v in rnn.named_parameters()}
    g = {k: v.grad.numpy() for k, v in rnn.named_parameters()}
    return p, g, x.detach().numpy(), leaf.grad.numpy(), G.numpy(), fresh


@pytest.mark.parametrize("gate_count", [4, 3])
@pytest.mark.parametrize("per_step", [False, True])
@pytest.mark.parametrize("pattern", [None, "random", "nested-like", "first-only"])
def test_the_model_reproduces_float64_autograd(pattern, per_step, gate_count):
    rows, steps = 37, 6
    bits = None if pattern is None else M.make_masks(pattern, rows, steps, seed=3)
    p, g, x, dleaf, G, fresh = _autograd(rows, steps, bits, per_step, 11)
    gates, hseq = M.forward(x, p["weight_ih_l0"], p["weight_hh_l0"], p["bias_ih_l0"], p["bias_hh_l0"])
    gates = gates if gate_count == 4 else gates[:, :, [0, 1, 3]]
    kw = {"dh_seq": G} if per_step else {"dh_sum": G}
    d_gi, dW_hh, dbn = M.rec(gates, gate_count, hseq, p["weight_hh_l0"], bits, steps, **kw)
    assert np.array_equal(np.isnan(d_gi).any(2), ~fresh) and np.array_equal(np.isnan(d_gi).all(2), ~fresh)
    out = M.inp(d_gi, p["weight_ih_l0"], bits, x, steps)
    rtol = 1e-12
    _close("dW_hh", dW_hh, g["weight_hh_l0"], rtol)
    _close("db_hh(n)", dbn, g["bias_hh_l0"][2 * H:], rtol)
    _close("dW_ih", out["dW"], g["weight_ih_l0"], rtol)
    _close("db_ih", out["db"], g["bias_ih_l0"], rtol)
    _close("db_hh(r, z) = db_ih(r, z)", out["db"][:2 * H], g["bias_hh_l0"][:2 * H], rtol)
    # dx at a fresh step carries its whole repeat group: the gradient of the shared row
    assert np.array_equal(np.isnan(out["dx"]).all(2), ~fresh)
    _close("dx", np.nan_to_num(out["dx"]), dleaf, rtol)
    assert not dleaf[~fresh].any()


@pytest.mark.parametrize("nested", [0, 1])
@pytest.mark.parametrize("pattern", [None, "random", "top-and-zero"])
def test_the_epilogue_equals_the_suffix_sums_over_an_explicit_dx(pattern, nested):
    rows, steps, n_out = 21, 7, 30
    rng = np.random.default_rng(5)
    bits = None if pattern is None else M.make_masks(pattern, rows, steps, seed=1)
    fresh = M.fresh_matrix(bits, rows, steps)
    d_gi, w, x = rng.standard_normal((rows, steps, 384)), rng.standard_normal((384, H)), rng.standard_normal((rows, steps, H))
    order = rng.permutation(n_out)[:rows]
    out = M.inp(d_gi, w, bits, x, steps, order=order, nested=nested, self_loop=True, zout=True, n_out=n_out)
    dx = np.where(fresh[:, :, None], d_gi @ w, 0.0) * (x > 0)                      # [rows, steps, 128], the ReLU mask applied
    for p in range(rows):
        G = [dx[p, t:].sum(0) for t in range(steps)]
        for t in range(steps):
            if not fresh[p, t]:
                assert np.isnan(out["Z"][order[p], t]).all()
                continue
            want = sum(G[i] for i in range(t, steps) if fresh[p, i]) if nested else G[t]
            _close("Z", out["Z"][order[p], t], want, 1e-13)
        _close("S0", out["S0"][order[p]], G[0], 1e-13)
    rest = np.setdiff1d(np.arange(n_out), order)
    assert np.isnan(out["Z"][rest]).all() and np.isnan(out["S0"][rest]).all()
    assert M.inp(d_gi, w, bits, x, steps, zout=True)["S0"] is None


def test_the_mask_helpers():
    for steps in (2, 3, 31, 32, 33, 63, 64):
        for pat in M.PATTERNS:
            if (pat in ("low-word-only", "b0-32", "b0-31-32") and steps <= 32) or (pat == "b0-63" and steps != 64):
                continue
            bits = M.make_masks(pat, 150, steps, seed=steps)
            assert len(bits) == 10 and all(m & 1 and m >> steps == 0 for m in bits), (pat, steps)
            words = M.pack_masks(bits, steps)
            assert words.dtype == np.uint32 and len(words) == (20 if steps > 32 else 10)
            back = [int(words[2 * i]) | (int(words[2 * i + 1]) << 32) for i in range(10)] if steps > 32 else [int(w) for w in words]
            assert back == bits
    assert M.make_masks("first-only", 40, 33) == [1, 1, 1] and M.make_masks("b0-31-32", 16, 40) == [1 | 1 << 31 | 1 << 32]
    assert M.make_masks("first-then-ones", 40, 64) == [1, 2 ** 64 - 1, 1]
    nl = M.make_masks("nested-like", 150, 64)
    assert 1 in nl and 2 ** 64 - 1 in nl and all(m == 1 | ((2 ** 64 - 1) >> f << f) for m, f in zip(nl, (64, 1, 2, 63, 32, 32, 33)))
    g = M.pack_masks([5, 1], 3, garbage_seed=1)
    assert [int(w) & 7 for w in g] == [5, 1] and all(int(w) >> 3 for w in g)
    g = M.pack_masks([5, 1 | 1 << 32], 33, garbage_seed=1)
    assert [int(w) for w in g[0::2]] == [5, 1] and [int(w) & 1 for w in g[1::2]] == [0, 1] and all(int(w) >> 1 for w in g[1::2])
    assert M.pack_masks(None, 3) is None


def test_the_bf16_split_and_the_plane_builder():
    v = np.array([1.0, 1.00390625, 257.0, 65535.0, 1 + 2.0 ** -9 + 2.0 ** -18, -0.3], dtype=np.float32)
    hi, lo = M.split2(v)
    assert hi.tolist()[:3] == [1.0, 1.0, 256.0] and lo.tolist()[:3] == [0.0, 0.00390625, 1.0]
    assert (hi + lo)[3] == 65535.0 and (hi.astype(np.float64) + lo)[4] == 1 + 2.0 ** -9       # 16 bits survive, more do not
    rng = np.random.default_rng(2)
    x = np.maximum(rng.standard_normal((5, 3, H)), 0).astype(np.float32)
    buf, dec = M.build_planes(x, 40, first_row=2)
    assert buf.dtype == np.uint8 and buf.size == 40 * (4 * H + 4)
    half, sc = buf[: 40 * 4 * H].view(np.float16).reshape(2, 40, H), buf[40 * 4 * H:].view(np.float32)
    assert np.isnan(half[:, :6]).all() and np.isnan(half[:, 21:]).all() and np.isnan(sc[:6]).all() and np.isnan(sc[21:]).all()
    assert np.array_equal((half[0, 6:21].astype(np.float32) + half[1, 6:21].astype(np.float32)) * sc[6:21, None], dec.reshape(15, H))
    assert np.abs(dec - x).max() <= 2.0 ** -20 * np.abs(x).max()
    xi = rng.integers(0, 4, (5, 3, H)).astype(np.float32)
    buf, dec = M.build_planes(xi, 15, exact=True)
    assert np.array_equal(dec, xi) and not buf[15 * 2 * H: 15 * 4 * H].any()
    fresh = np.ones((5, 3), dtype=bool)
    fresh[1, 2] = False
    poisoned = M.poison_planes(buf, 15, 0, fresh)
    assert np.isnan(poisoned[: 15 * 4 * H].view(np.float16).reshape(2, 15, H)[:, 5]).all() and np.isnan(poisoned[15 * 4 * H:].view(np.float32)[5])
    assert np.array_equal(np.delete(poisoned[: 15 * 2 * H].view(np.float16).reshape(15, H), 5, 0), np.delete(buf[: 15 * 2 * H].view(np.float16).reshape(15, H), 5, 0))


def test_the_audit_notices_inputs_that_are_not_exact():
    A = M.Audit()
    with pytest.raises(AssertionError, match="16 significant bits"):
        A.plane("v", np.array([1 + 2.0 ** -9 + 2.0 ** -18]))
    with pytest.raises(AssertionError, match="no float32"):
        A.f32("v", np.array([1.0 + 2.0 ** -30]))
    with pytest.raises(AssertionError, match="lo·lo"):
        A.product("p", np.array([[257.0]]), np.array([[257.0]]))
    A.terms("s", np.array([2.0 ** 20]), 2.0 ** -4)
    with pytest.raises(AssertionError, match="partial sum"):
        A.finish()
    t = M.exact_inputs(20, 4, 0)
    with pytest.raises(AssertionError):                     # a weight with 17 significant bits
        M.rec(t["gates"], 4, t["hseq"], t["w_hh"] * (1 + 2.0 ** -16), None, 4, dh_sum=t["dh_sum"], audit=M.Audit())


def test_the_case_list_covers_every_value_of_every_axis():
    cases = T.EXACT_CASES
    assert len({c.name for c in cases}) == len(cases)
    planned = [c for c in cases if c.grid == 3 and c.mask not in (None, "ones")]
    for group in (cases, planned):
        assert {c.rows for c in group} == set(T.ROWS)
        assert {c.steps for c in group} >= set(T.STEPS) - ({1} if group is planned else set())
        assert {c.mask for c in group} >= set(M.PATTERNS) - {"ones"}
        assert {(c.gc, c.per_step) for c in group} == set(T.REC_FORMS)
        assert {(c.x, c.out == "Z") for c in group} == {("planes", False), ("planes", True), ("f32", False), ("f32", True)}
        assert {c.first_row for c in group if c.x == "planes"} == {0, 32} and {c.ldx for c in group if c.x == "f32"} == {128, 132, 256}
        assert {(c.out, c.order, c.nested, c.s0) for c in group} == set(T.OUT_FORMS)
        assert {c.order for c in group} == {False, True} and {c.nested for c in group} == {0, 1} and {c.s0 for c in group} == {False, True}
        assert {c.accumulate for c in group} == {0, 1}
    assert {c.grid for c in cases if c.rows == 150} == {0, 1, 2, 3, 7}
    assert {(c.rows, c.mask, c.gc, c.per_step, c.steps) for c in cases if c.name.startswith("prod")} == \
        {(r, m, g, p, s) for r in T.ROWS for m in (None, "random") for g, p in T.REC_FORMS for s in (3, 33)}
    # pairs: every mask with every grid family member at 150 rows somewhere, every step count with a plan and without
    assert {c.steps for c in cases if c.mask is None} == set(T.STEPS) and {c.steps for c in cases if c.mask == "random"} == set(T.STEPS) - {1}
    assert any(c.garbage and c.steps < 32 for c in cases)


@pytest.mark.parametrize("c", T.EXACT_CASES, ids=lambda c: c.name)
def test_every_exact_case_of_the_gpu_file_passes_the_audit(c):
    """planes hi + lo exact, no lo·lo term, every intermediate a float32, every order-free sum below 2^24 granules"""
    t, want, bits = T.exact_model(c, audit=True)
    fresh = M.fresh_matrix(bits, c.rows, c.steps)
    assert np.array_equal(np.isnan(want["d_gi"]).all(2), ~fresh)
    for k, v in want.items():
        if v is not None:
            w = np.nan_to_num(v)
            assert np.array_equal(w.astype(np.float32).astype(np.float64), w), k
    assert np.abs(np.nan_to_num(want["d_gi"])).max() > 0 or c.rows * c.steps < 4
    if c.steps > 1:
        assert np.abs(want["dW_hh"]).max() > 0 and np.abs(want["dW_ih"]).max() > 0


def test_the_wide_offset_fixture_passes_the_audit():
    """tests/test_gpu_wide_offsets.py drives ctgcn_gru_bwd_in_f32's ldx with an exact case of its own: 33 row-steps, a plan with a repeat"""
    t, want = M.exact_case(**WT.GRU_BWD_IN_CASE)
    assert WT.GRU_BWD_IN_CASE["rows"] * WT.GRU_BWD_IN_CASE["steps"] == WT.N and np.isnan(want["dx"][:, 1]).all() and np.isfinite(want["dx"][:, [0, 2]]).all()
    assert np.abs(want["dW_ih"]).max() > 0
