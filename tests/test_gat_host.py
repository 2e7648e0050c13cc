"""Host checks of the GAT baseline: the torch mirror (tests/_gat_ref.py) against the reference's recorded results
(tests/golden/gat_uci.npz), the new C entry points' argument checks, the host models of the two dropout draws, and the modules'
interface.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _gat_ref as A
import _gcrn_ref as R
from conftest import check_sampled_tensor, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_gat_da_workspace_bytes", "ctgcn_gat_da_f32", "ctgcn_gat_piece_floats", "ctgcn_gat_fwd_f32", "ctgcn_gat_bwd_prep_f32", "ctgcn_gat_bwd_row_f32", "ctgcn_gat_bwd_col_f32")
_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def mirror_run(case, dtype):
    if (case, dtype) not in _runs:
        g = A.fixture()
        model = A.build(case, A.GatMirror)
        seeded_parameters(model, int(g["seed"]))
        model = model.to(dtype).train()
        x, adj = A.features(case, dtype), A.adjacency(dtype)
        _runs[case, dtype] = A.adam_losses(model, lambda: model(x, adj), A.surrogate_weights(case, dtype))
    losses, (outs, grads) = _runs[case, dtype]
    return losses, outs, grads


@pytest.mark.parametrize("case", A.CASES)
def test_mirror_float64_matches_the_reference(case):
    g = A.fixture()
    losses, outs, grads = mirror_run(case, torch.float64)
    for t in range(A.T):
        check_sampled_tensor(g, "%s_out_t%d" % (case, t), outs[t].numpy(), 0.0, 1e-9)
    for k in g[case + "_keys"]:
        check_sampled_tensor(g, "%s_grad_%s" % (case, k), grads[str(k)].numpy(), 0.0, 1e-9)
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 1e-9 * np.abs(g[case + "_losses"]).max()


@pytest.mark.parametrize("case", A.CASES)
def test_mirror_float32_is_within_twice_the_reference_s_own_float32_error(case):
    g = A.fixture()
    losses, outs, grads = mirror_run(case, torch.float32)

    def worst(got, key):
        ref, pick, top = stored(g, key)
        got = got.double().numpy().reshape(-1)
        return np.abs((got if pick is None else got[pick]) - ref).max() / top

    for t in range(A.T):
        assert worst(outs[t], "%s_out_t%d" % (case, t)) <= 2 * g[case + "_yard_out"][t], (case, t)
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        assert worst(grads[str(k)], "%s_grad_%s" % (case, k)) <= 2 * yard, (case, str(k))
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 2 * float(g[case + "_yard_losses"]) * np.abs(g[case + "_losses"]).max()


def test_fixture_is_the_setup_the_tests_describe():
    lens = [np.diff(R.row_normalized_csr(t).indptr) for t in range(A.T)]
    assert [int(v.sum()) for v in lens] == [5441, 19929, 6677]
    assert min(int(v.min()) for v in lens) == 1 and max(int(v.max()) for v in lens) == 199
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "gat_uci.npz")) < 1000000


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert lib.ctgcn_gat_piece_floats(18, 3) == 2 * 20 + 4 and lib.ctgcn_gat_piece_floats(0, 1) == 0


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch
    nan, inf = float("nan"), float("inf")

    def fwd(n=4, d=8, heads=2, rp=p, col=p, S=p, lds=8, asrc=p, adst=p, alpha=0.2, epi=2, pa=0.0, pf=0.0, out=p, ldo=8, Y=p, ldy=8, u=p, v=p,
            m=p, Z=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_gat_fwd_f32(n, d, heads, rp, col, S, lds, asrc, adst, alpha, epi, pa, 1, pf, 2, out, ldo, Y, ldy, u, v, m, Z, lr, nl, thr,
                                     ws, wsb, None)

    def prep(n=4, d=8, heads=2, dY=p, lddy=8, Y=p, ldy=8, epi=2, pf=0.0, u=p, m=p, Z=p, G=p, ldg=8, pack=p):
        return lib.ctgcn_gat_bwd_prep_f32(n, d, heads, dY, lddy, Y, ldy, epi, pf, 2, u, m, Z, G, ldg, pack, None)

    def row(n=4, d=8, heads=2, rp=p, col=p, S=p, lds=8, G=p, ldg=8, v=p, pack=p, alpha=0.2, pa=0.0, R_=p, ldr=8, cs=p, du=p, lr=None, nl=0, thr=8,
            ws=None, wsb=0):
        return lib.ctgcn_gat_bwd_row_f32(n, d, heads, rp, col, S, lds, G, ldg, v, pack, alpha, pa, 1, R_, ldr, cs, du, lr, nl, thr, ws, wsb, None)

    def colp(n=4, d=8, heads=2, rp=p, col=p, G=p, ldg=8, S=p, lds=8, v=p, pack=p, asrc=p, adst=p, alpha=0.2, pa=0.0, du=p, dS=p, ldds=8, B=p,
             ldb=8, ks=p, dv=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_gat_bwd_col_f32(n, d, heads, rp, col, G, ldg, S, lds, v, pack, asrc, adst, alpha, pa, 1, du, dS, ldds, B, ldb, ks, dv,
                                         lr, nl, thr, ws, wsb, None)

    def da(n=4, d=8, heads=2, S=p, lds=8, du=p, dv=p, das=p, dad=p, ws=p, wsb=1 << 20):
        return lib.ctgcn_gat_da_f32(n, d, heads, S, lds, du, dv, das, dad, ws, wsb, None)

    assert da(n=-1) == INVALID and da(n=2 ** 31) == INVALID and da(d=0) == INVALID and da(heads=0) == INVALID and da(d=9, lds=9) == INVALID
    assert da(lds=7) == INVALID and da(S=None) == INVALID and da(du=None) == INVALID and da(das=None) == INVALID and da(dad=None) == INVALID
    assert da(du=None, das=None, dv=None, dad=None) == INVALID
    assert da(ws=None) == WORKSPACE and da(wsb=63) == WORKSPACE          # one block of d = 8 holds 2 * 8 floats
    assert b"gat_da" in lib.ctgcn_last_error()
    assert lib.ctgcn_gat_da_workspace_bytes(64, 8) == 64 and lib.ctgcn_gat_da_workspace_bytes(65, 6) == 128
    assert lib.ctgcn_gat_da_workspace_bytes(-1, 8) == 0
    for call in (fwd, prep, row, colp):
        assert call(n=-1) == INVALID and call(n=2 ** 31) == INVALID
        assert call(d=0) == INVALID and call(heads=0) == INVALID and call(d=9, heads=2, **{k: 9 for k in _lds(call)}) == INVALID
        for ld in _lds(call):
            assert call(**{ld: 7}) == INVALID, (call.__name__, ld)
        assert call(n=0) == 0
    for call in (fwd, row, colp):
        assert call(alpha=nan) == INVALID and call(alpha=inf) == INVALID
        assert call(pa=1.0) == INVALID and call(pa=-0.1) == INVALID and call(pa=nan) == INVALID
        assert call(rp=None) == INVALID and call(col=None) == INVALID and call(S=None) == INVALID
        assert call(nl=1, lr=None) == INVALID and call(nl=5, lr=p) == INVALID
        assert call(nl=1, lr=p, thr=0, ws=p, wsb=1 << 20) == INVALID
        assert call(nl=1, lr=p, ws=None, wsb=0) == WORKSPACE
        assert call(nl=1, lr=p, ws=p, wsb=16 * 4) == WORKSPACE          # one piece of d = 8, heads = 2 holds 2 * 8 + 4 floats
        assert call(nl=1, lr=p, ws=ctypes.c_void_p(68), wsb=1 << 20) == WORKSPACE
    for call in (fwd, prep):
        assert call(pf=1.0) == INVALID and call(pf=nan) == INVALID
        assert call(epi=3) == INVALID and call(epi=-1) == INVALID
        assert call(Y=None) == INVALID
    assert fwd(asrc=None) == INVALID and fwd(adst=None) == INVALID and fwd(out=None) == INVALID
    assert fwd(u=None) == INVALID and fwd(v=None) == INVALID and fwd(m=None) == INVALID and fwd(Z=None) == INVALID
    assert b"gat_fwd" in lib.ctgcn_last_error()
    assert prep(dY=None) == INVALID and prep(G=None) == INVALID and prep(pack=None) == INVALID and prep(pack=ctypes.c_void_p(68)) == INVALID
    assert prep(u=None) == INVALID and prep(m=None) == INVALID and prep(Z=None) == INVALID
    assert b"gat_bwd_prep" in lib.ctgcn_last_error()
    assert row(G=None) == INVALID and row(v=None) == INVALID and row(pack=None) == INVALID and row(R_=None) == INVALID
    assert row(cs=None) == INVALID and row(du=None) == INVALID
    assert b"gat_bwd_row" in lib.ctgcn_last_error()
    assert colp(G=None) == INVALID and colp(v=None) == INVALID and colp(pack=None) == INVALID and colp(B=None) == INVALID
    assert colp(ks=None) == INVALID and colp(dv=None) == INVALID and colp(asrc=None) == INVALID and colp(adst=None) == INVALID
    assert colp(du=None) == INVALID and colp(dS=None) == INVALID          # du and dS go together
    assert b"gat_bwd_col" in lib.ctgcn_last_error()


def _lds(call):
    import inspect
    return [k for k in inspect.signature(call).parameters if k.startswith("ld")]


def test_host_draw_models_agree_with_u01_on_hand_computed_triples():
    """u01(k, i, j) = (mix64(mix64(k) ^ mix64(i * 0x100000001b3 + j)) >> 11) / 2^53 in wrapping uint64 arithmetic, written out here in
    Python integers; the attention draw of head h is the one of key + h on the (row, column) pair, the feature draw is keyed on
    (row, feature column)"""
    M = (1 << 64) - 1

    def mix(z):
        z = (z + 0x9e3779b97f4a7c15) & M
        z = ((z ^ (z >> 30)) * 0xbf58476d1ce4e5b9) & M
        z = ((z ^ (z >> 27)) * 0x94d049bb133111eb) & M
        return z ^ (z >> 31)

    def by_hand(k, i, j):
        return (mix(mix(k & M) ^ mix((i * 0x100000001b3 + j) & M)) >> 11) / 9007199254740992.0

    rows, cols = np.array([0, 3, 66, 1898]), np.array([5, 3, 0, 1897])
    for key in (0, 12345, 2 ** 61 + 7, M - 1):                   # M - 1: key + h wraps
        for p in (0.5, 0.1):
            keep = A.att_keep(key, rows, cols, 3, p)
            assert keep.shape == (4, 3)
            for e in range(4):
                for h in range(3):
                    want = by_hand(key + h, int(rows[e]), int(cols[e]))
                    assert float(R.u01((key + h) & M, np.uint64(rows[e]), np.uint64(cols[e]))) == want
                    assert bool(keep[e, h]) == (want >= p)
    feat = A.feat_keep(77, 5, 7, 0.5)
    assert feat.shape == (5, 7) and all(bool(feat[i, c]) == (by_hand(77, i, c) >= 0.5) for i in range(5) for c in range(7))
    # the draw is keyed on the pair, not on the entry's position: the transposed order gives the same mask
    order = np.argsort(cols, kind="stable")
    assert np.array_equal(A.att_keep(9, rows[order], cols[order], 2, 0.5), A.att_keep(9, rows, cols, 2, 0.5)[order])
    masks = A.model_keep(100, 2, rows, cols, 3, 4, 0.5)
    assert np.array_equal(masks["att0"].numpy(), A.att_keep(100 + 8192, rows, cols, 3, 0.5))
    assert np.array_equal(masks["att1"].numpy(), A.att_keep(100 + 8192 + 2048, rows, cols, 1, 0.5))
    assert np.array_equal(masks["feat"].numpy(), A.feat_keep(100 + 2 ** 40 + 2, A.N, 12, 0.5))


def test_unshifted_softmax_breaks_where_the_shifted_one_does_not():
    """float32, logits below fp32 exp's underflow and above its overflow: the reference's form gives NaN, the shifted one float64's"""
    rows, cols = torch.tensor([0, 0, 1, 1, 2]), torch.tensor([0, 1, 0, 1, 2])
    S = torch.tensor([[130.0, 1.0], [125.0, 2.0], [-3000.0, 3.0]])            # rows 0, 1: l = -260 .. -250; row 2: l = +1200
    a = torch.tensor([[1.0, 0.0]])
    bad, _, _ = A.attention(S, a, a, rows, cols, 1, shifted=False)
    good, _, _ = A.attention(S, a, a, rows, cols, 1)
    want, _, _ = A.attention(S.double(), a.double(), a.double(), rows, cols, 1)
    assert bool(torch.isnan(bad).all())                                      # 0 / 0 twice, inf / inf
    assert bool(torch.isfinite(good).all()) and float((good.double() - want).abs().max()) <= 1e-6 * float(want.abs().max())


@pytest.mark.parametrize("case", A.CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(case):
    import ctgcn_amd
    g = A.fixture()
    model = A.build(case, ctgcn_amd.GAT)
    assert model.method_name == "GAT"
    sd = model.state_dict()
    assert sorted(sd) == [str(k) for k in g[case + "_keys"]]
    for k, shape in zip(g[case + "_keys"], g[case + "_shapes"]):
        assert ",".join(str(s) for s in sd[str(k)].shape) == str(shape), k
    mirror = A.build(case, A.GatMirror)
    mirror.load_state_dict(sd)            # strict: same keys and shapes both ways
    model.load_state_dict(mirror.state_dict())


def test_constructor_initialiser_and_exports():
    import ctgcn_amd
    from ctgcn_amd import GAT, SpGraphAttentionLayer, embedding
    from ctgcn_amd.baseline import GAT as G2, SpGraphAttentionLayer as L2
    assert G2 is GAT and L2 is SpGraphAttentionLayer and "GAT" in ctgcn_amd.__all__ and "SpGraphAttentionLayer" in ctgcn_amd.__all__
    m = GAT(30, 500, 128, dropout=0.5, alpha=0.2, head_num=1, learning_type="S-edge")
    assert sorted(m.state_dict()) == ["attention_0.W", "attention_0.a", "out_att.W", "out_att.a"]
    assert tuple(m.attention_0.a.shape) == (1, 1000) and tuple(m.out_att.W.shape) == (500, 128) and m.out_att.concat is False
    assert repr(m.attention_0) == "SpGraphAttentionLayer (30 -> 500)"
    # xavier_normal_ with gain 1.414: std = gain * sqrt(2 / (fan_in + fan_out)); 64 000 draws: the sample's is within 2 %
    W = GAT(400, 160, 8, head_num=1).attention_0.W.detach()
    assert abs(float(W.std()) / (1.414 * np.sqrt(2.0 / 560)) - 1) < 0.02
    with pytest.raises(AssertionError):
        GAT(8, 4, 2, learning_type="U-own")
    with pytest.raises(ValueError, match="head_num"):
        GAT(8, 1, 2, head_num=2049)
    assert "GAT" in embedding._SUPPORTED and "GAT" not in embedding._S_MODELS and "GCN" not in embedding._SUPPORTED


def test_cpu_tensors_raise():
    from ctgcn_amd import GAT, SpGraphAttentionLayer, ops
    from ctgcn_amd._lib import CtgcnHipError
    eye = torch.eye(8).to_sparse()
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        GAT(8, 4, 2, head_num=2)(eye, eye)
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        GAT(8, 4, 2, head_num=2)([torch.zeros(8, 8)], [eye])
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        SpGraphAttentionLayer(8, 4, 0.5, 0.2)(torch.zeros(8, 8), eye)

    class Adj(object):                                          # stands in for a GcnAdj: gat_conv refuses before it reads one
        val = torch.zeros(0)

    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.gat_conv(torch.zeros(8, 4), torch.zeros(2, 2), torch.zeros(2, 2), Adj(), 2)
