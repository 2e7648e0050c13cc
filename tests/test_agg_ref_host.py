"""Pins the float64 aggregation model (_agg_ref.py) on the host: against the C oracle, against float64 autograd of the layers.py
expression, and the exact tier's 2^24 condition for every case of test_gpu_agg_shapes.py (_agg_cases.py)."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _agg_cases as C
import _agg_ref as R


def _small_lists():
    rng = np.random.default_rng(7)
    n = 41
    base = sp.random(n, n, density=0.2, random_state=1, format="csr")
    base.data = rng.uniform(0.2, 1.0, base.nnz) * rng.choice([-1.0, 1.0], base.nnz)
    base.setdiag(0)
    base.eliminate_zeros()
    up = sp.triu(base + base.T, 1).tocoo()
    level = rng.integers(0, 3, up.nnz)                         # one level per undirected edge: A_0 ⊆ A_1 ⊆ A_2, symmetric
    nested = []
    for j in range(3):
        keep = level >= 2 - j
        half = sp.coo_matrix((up.data[keep], (up.row[keep], up.col[keep])), shape=(n, n))
        nested.append((half + half.T).tocsr())
    general = []
    for j in range(4):
        m = sp.random(n, n, density=0.1, random_state=10 + j, format="csr")
        m.data = rng.standard_normal(m.nnz)
        general.append(m)
    return {"nested-selfloop": (nested, True), "general-asymmetric": (general, False), "K1": ([general[0]], False)}


def _f32(a):
    return np.asarray(a, np.float32).astype(np.float64)


@pytest.mark.parametrize("name", ["nested-selfloop", "general-asymmetric", "K1"])
@pytest.mark.parametrize("relu", [True, False])
def test_model_equals_float64_autograd(name, relu):
    """layers.py:41-48: res_j = res_{j-1} + A_j x, relu, stacked [N, K, d] — in float64 torch, gradients by autograd"""
    mats, self_loop = _small_lists()[name]
    assert R.is_nested(mats) == (name != "general-asymmetric")
    rng = np.random.default_rng(3)
    n, K, d = mats[0].shape[0], len(mats), 6
    x, dH = rng.standard_normal((n, d)), rng.standard_normal((n, K, d))
    xt = torch.from_numpy(x).requires_grad_(True)
    res, hs = None, []
    for j, m in enumerate(mats):
        a = torch.from_numpy(m.toarray() + (np.eye(n) if j == 0 and self_loop else 0.0))
        res = a @ xt if res is None else res + a @ xt
        hs.append(torch.relu(res) if relu else res)
    Ht = torch.stack(hs, 1)
    (Ht * torch.from_numpy(dH)).sum().backward()
    H, pre = R.forward(mats, x, self_loop, relu)
    dX = R.backward(mats, x, dH, self_loop, relu)
    np.testing.assert_allclose(H.value, Ht.detach().numpy(), rtol=0, atol=1e-13 * max(1.0, H.T.max()))
    np.testing.assert_allclose(dX.value, xt.grad.numpy(), rtol=0, atol=1e-13 * max(1.0, dX.T.max()))
    # Z and S0 give the same dX through the stored form: dX[r] = S0[r] + sum_e val_e Z[col_e, slot_e] over the transposed entries
    for nested in ([True, False] if R.is_nested(mats) else [False]):
        Z, S0 = R.backward_prep(H.value, dH, nested, relu)
        got = S0.value.copy() if self_loop else np.zeros((n, d))
        for j, m in enumerate(mats):
            prev = mats[j - 1] if (nested and j) else None
            new = (m - prev).tocsr() if prev is not None else sp.csr_matrix(m)      # nested storage: the entries first present in A_j
            got += new.T @ Z.value[:, j]
        np.testing.assert_allclose(got, dX.value, rtol=0, atol=1e-12 * max(1.0, dX.T.max()))
    assert (H.T >= np.abs(pre.value) - 1e-12).all() and (dX.T >= np.abs(dX.value) - 1e-12).all()


@pytest.mark.parametrize("name", ["nested-selfloop", "general-asymmetric", "K1"])
def test_model_against_the_c_oracle(name):
    """the oracle computes in fp32 (one SpMM per matrix, then the cumulative sums): it must sit inside the same gamma T bound"""
    from oracle import oracle as O
    mats, self_loop = _small_lists()[name]
    mats = [sp.csr_matrix((_f32(m.data), m.indices, m.indptr), shape=m.shape) for m in mats]
    rng = np.random.default_rng(5)
    n, K, d = mats[0].shape[0], len(mats), 9
    x, dH = _f32(rng.standard_normal((n, d))), _f32(rng.standard_normal((n, K, d)))
    ref_list = [(m + sp.identity(n)).tocsr() if (j == 0 and self_loop) else m for j, m in enumerate(mats)]
    H, pre = R.forward(mats, x, self_loop, True)
    # the oracle sums every A_j x afresh: its term count is that of the general form
    H.m = np.sum([np.diff(m.indptr) for m in ref_list], axis=0)[:, None]
    got = O.core_aggregate(ref_list, x.astype(np.float32))
    used = H.used(got, K)
    print("  [bound] oracle forward %-20s %.3f of gamma T" % (name, used))
    assert used <= 1.0
    # backward: the oracle masks with ITS fp32 pre-activations; compare where the two masks agree (they do, away from fp32 near-ties)
    _, opre = O.core_aggregate(ref_list, x.astype(np.float32), return_pre=True)
    assert ((opre > 0) == (pre.value > 0)).all(), "an fp32 near-tie in the fixture: pick another seed"
    dX = R.backward(mats, x, dH, self_loop, True)
    dX.m = np.sum([np.asarray((m != 0).sum(axis=0)).reshape(-1) for m in ref_list], axis=0)[:, None]
    used = dX.used(O.core_aggregate_bwd(ref_list, x.astype(np.float32), dH.astype(np.float32)), K)
    print("  [bound] oracle backward %-19s %.3f of gamma T" % (name, used))
    assert used <= 1.0


def test_exact_inputs_of_a_case_hit_the_mask():
    """exact zeros among the pre-activations are what the exact tier is for"""
    case = C.cases("flags")[0]
    mats, x, dH, model, level = C.exact_inputs(case)
    pre = model["pre"].value
    assert (pre == 0).mean() > 0.01 and (pre > 0).any() and (pre < 0).any()


@pytest.mark.parametrize("group", sorted(C.GROUPS))
def test_exact_tier_condition_holds_for_every_gpu_case(group):
    """every term mass of every modelled intermediate below 2^24 granules (exact_model asserts it per level), the model's nestedness is
    the case's unless the layout makes a general list nested by accident, the forced row lengths are there"""
    for case in C.cases(group):
        mats, x, dH, model, level = C.exact_inputs(case)
        assert model["granules"] < 2.0 ** 24, case.id
        assert model["nested"] or not case.nested, case.id
        for r in (model["H"], model["Z"], model["S0"], model["dX"]):
            assert np.array_equal(r.value.astype(np.float32).astype(np.float64), r.value), case.id
        print("  [exact] %-52s level %d, %.3g granules" % (case.id, level, model["granules"]))


def test_forced_rows_hold_their_lengths_and_layouts():
    for L in (8, 16, 32, 64):
        st = C.forced_rows(L, 7, "at4L")
        assert list(st.lengths()[:12]) == C.row_lengths(L) and list(st.lengths()[12:24]) == C.row_lengths(L)
        row = st.slots[st.rows == 11]                                   # 3 L + 2 entries: changes exactly at entry 4 and entry L
        assert list(np.flatnonzero(np.diff(row)) + 1) == [4, L]
        assert st.slots[st.rows == 23].min() == 1                       # variant B: slot 0 empty
        assert set(C.forced_rows(L, 7, "last").slots) == {6} and set(C.forced_rows(L, 7, "trail").slots[:200]) <= {0, 1}
        each = C.forced_rows(L, 7, "each")
        assert list(each.slots[each.rows == 9][:8]) == [0, 1, 2, 3, 4, 5, 6, 6]
    sym = C.symmetric_rows(16, 7, "s036")
    m = sym.matrices(np.arange(1, sym.edge.max() + 2), True)[-1]
    assert abs(m - m.T).sum() == 0 and list(sym.lengths()[:12]) == C.row_lengths(16)


def test_piece_rows_put_slot_boundaries_on_and_inside_pieces():
    st = C.piece_rows(64, 16385, 8193)
    lens, lens_t = st.lengths(), st.lengths(True)
    assert (lens[0], lens[1], lens_t[2], lens_t[3]) == (16385, 8193, 16385, 8193) and lens[2:].max() <= 5
    row = st.slots[st.rows == 0]
    plen = 5504                                                         # ceil(ceil(16385 / 3) / 64) * 64
    assert list(np.flatnonzero(np.diff(row)) + 1) == [plen, plen + plen // 2]
    assert list(np.flatnonzero(np.diff(st.slots[st.rows == 1])) + 1) == [4160, 4160 + 2080]     # two pieces of a split of three


def test_prep_inputs_are_exact():
    for d, K in C.PREP_CASES:
        for nested in (True, False):
            H, dH, Z, S0 = C.prep_exact(d, K, nested, True)
            assert (H == 0).any() and (dH[H == 0] != 0).all()
