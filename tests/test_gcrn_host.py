"""Host checks of the GCN / GCRN baselines: the torch mirror (tests/_gcrn_ref.py) against the reference's recorded results
(tests/golden/gcrn_uci.npz), the new C entry points' argument checks, the host model of the dropout draw, and the modules' interface.
No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _gcrn_ref as R
from conftest import check_sampled_tensor, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_gcn_conv_fwd_f32", "ctgcn_gcn_conv_prep_rows", "ctgcn_gcn_conv_prep_workspace_bytes", "ctgcn_gcn_conv_prep_f32")
_runs = {}


def stored(g, key):
    """(reference values float64, index into the flattened tensor or None, largest magnitude of the tensor) of a put_tensor record"""
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def mirror_run(case, dtype):
    """(losses, outputs, gradients) of the mirror on the fixture's setup, computed once per (case, dtype)"""
    if (case, dtype) not in _runs:
        g = R.fixture()
        model = R.build(case, R.GcnMirror, R.GcrnMirror)
        seeded_parameters(model, int(g["seed"]))
        model = model.to(dtype).train()
        x, adj = R.features(case, dtype), R.adjacency(dtype)
        _runs[case, dtype] = R.adam_losses(model, lambda: model(x, adj), R.surrogate_weights(case, dtype))
    losses, (outs, grads) = _runs[case, dtype]
    return losses, outs, grads


@pytest.mark.parametrize("case", R.CASES)
def test_mirror_float64_matches_the_reference(case):
    g = R.fixture()
    losses, outs, grads = mirror_run(case, torch.float64)
    for t in range(R.T):
        check_sampled_tensor(g, "%s_out_t%d" % (case, t), outs[t].numpy(), 1e-9, 1e-9)
    for k in g[case + "_keys"]:
        check_sampled_tensor(g, "%s_grad_%s" % (case, k), grads[str(k)].numpy(), 1e-9, 1e-9)
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 1e-9 * np.abs(g[case + "_losses"]).max()


@pytest.mark.parametrize("case", R.CASES)
def test_mirror_float32_is_within_twice_the_reference_s_own_float32_error(case):
    g = R.fixture()
    losses, outs, grads = mirror_run(case, torch.float32)

    def worst(got, key):
        ref, pick, top = stored(g, key)
        got = got.double().numpy().reshape(-1)
        return np.abs((got if pick is None else got[pick]) - ref).max() / top

    for t in range(R.T):
        assert worst(outs[t], "%s_out_t%d" % (case, t)) <= 2 * g[case + "_yard_out"][t], (case, t)
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        assert worst(grads[str(k)], "%s_grad_%s" % (case, k)) <= 2 * yard, (case, str(k))
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 2 * float(g[case + "_yard_losses"]) * np.abs(g[case + "_losses"]).max()


def test_fixture_stays_clear_of_the_normalisation_clamp():
    assert float(R.fixture()["min_row_norm"]) > 0.1


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def fwd(n=4, d=8, rp=p, col=p, val=p, S=p, lds=8, b=p, Y=p, ldy=8, epi=2, pr=0.0, key=1, norm=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_gcn_conv_fwd_f32(n, d, rp, col, val, S, lds, b, Y, ldy, epi, pr, key, norm, lr, nl, thr, ws, wsb, None)

    def prep(n=4, d=8, dY=p, lddy=8, Y=p, ldy=8, norm=p, epi=2, pr=0.0, G=p, ldg=8, db=None, ws=None, wsb=0):
        return lib.ctgcn_gcn_conv_prep_f32(n, d, dY, lddy, Y, ldy, norm, epi, pr, G, ldg, db, ws, wsb, None)

    for call in (fwd, prep):
        assert call(n=-1) == INVALID
        assert call(n=2 ** 31) == INVALID
        assert call(d=0) == INVALID
        assert call(epi=3) == INVALID and call(epi=-1) == INVALID
        assert call(pr=1.0) == INVALID and call(pr=-0.1) == INVALID and call(pr=float("nan")) == INVALID
        assert call(Y=None) == INVALID
        assert call(ldy=7) == INVALID
        assert call(norm=None, epi=2) == INVALID
        assert call(n=0) == 0
    assert fwd(rp=None) == INVALID and fwd(col=None) == INVALID and fwd(val=None) == INVALID
    assert fwd(S=None) == INVALID and fwd(lds=7) == INVALID
    assert fwd(nl=1, lr=None) == INVALID
    assert fwd(nl=5, lr=p) == INVALID                           # more long rows than rows
    assert fwd(nl=1, lr=p, thr=0, ws=p, wsb=1 << 20) == INVALID
    assert fwd(nl=1, lr=p, ws=None, wsb=0) == WORKSPACE
    assert fwd(nl=1, lr=p, ws=p, wsb=16) == WORKSPACE           # one piece of a row of width 8 needs 32 bytes
    assert b"gcn_conv_fwd" in lib.ctgcn_last_error()
    assert prep(dY=None) == INVALID and prep(G=None) == INVALID and prep(lddy=7) == INVALID and prep(ldg=7) == INVALID
    assert prep(epi=1, Y=None) == INVALID and prep(epi=1, G=None) == INVALID
    rows = lib.ctgcn_gcn_conv_prep_rows()
    assert rows == 64
    assert lib.ctgcn_gcn_conv_prep_workspace_bytes(rows, 8) == 32 and lib.ctgcn_gcn_conv_prep_workspace_bytes(rows + 1, 6) == 64
    assert lib.ctgcn_gcn_conv_prep_workspace_bytes(-1, 8) == 0
    assert prep(db=p, ws=None, wsb=0) == WORKSPACE
    assert prep(db=p, ws=p, wsb=16) == WORKSPACE                # one block of width 8 needs 32 bytes
    assert prep(db=p, ws=ctypes.c_void_p(68), wsb=1 << 20) == WORKSPACE      # not 16-byte aligned
    assert b"gcn_conv_prep" in lib.ctgcn_last_error()
    assert prep(epi=0, Y=None, G=None, norm=None, db=None) == 0                  # G = dY and no bias gradient: nothing to launch


@pytest.mark.parametrize("p,bound", [(0.5, 0.027), (0.1, 0.016)])
def test_host_dropout_model_keeps_its_share(p, bound):
    """67 x 128 draws: the keep share lies within 5 binomial standard deviations of 1 - p"""
    n, d = 67, 128
    sd5 = min(bound, 5 * np.sqrt(p * (1 - p) / (n * d)))            # bound: the same figure rounded to three decimals; the smaller holds
    masks = []
    for key in (1, 7, 12345):
        keep = R.keep_mask(key, n, d, p)
        assert keep.shape == (n, d) and abs(keep.mean() - (1 - p)) <= sd5, (key, keep.mean())
        masks.append(keep)
    assert (masks[0] != masks[1]).any() and (masks[1] != masks[2]).any()
    # a larger p drops a superset: one draw per entry, compared with p
    assert not (R.keep_mask(1, n, d, 0.5) & ~R.keep_mask(1, n, d, 0.1)).any()
    assert R.keep_mask(1, n, d, 0.0).all()


def test_host_draw_is_splitmix64():
    # splitmix64's first outputs from state 0 (Vigna's reference implementation): mix64(k * golden) walks the same sequence
    assert int(R.mix64(np.uint64(0))) == 0xe220a8397b1dcdaf
    assert int(R.mix64(np.uint64(0x9e3779b97f4a7c15))) == 0x6e789e6aa1b965f4
    u = R.u01(3, np.arange(5, dtype=np.uint64), np.uint64(2))
    assert u.dtype == np.float64 and ((u >= 0) & (u < 1)).all() and len(set(u.tolist())) == 5


@pytest.mark.parametrize("case", R.CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(case):
    import ctgcn_amd
    g = R.fixture()
    model = R.build(case, ctgcn_amd.GCN, ctgcn_amd.GCRN)
    assert model.method_name == R.CASES[case][0]
    sd = model.state_dict()
    assert sorted(sd) == [str(k) for k in g[case + "_keys"]]
    for k, shape in zip(g[case + "_keys"], g[case + "_shapes"]):
        assert ",".join(str(s) for s in sd[str(k)].shape) == str(shape), k
    mirror = R.build(case, R.GcnMirror, R.GcrnMirror)
    mirror.load_state_dict(sd)            # strict: same keys and shapes both ways
    model.load_state_dict(mirror.state_dict())


def test_constructors_keep_the_reference_s_arguments():
    from ctgcn_amd import GCN, GCRN, GraphConvolution
    from ctgcn_amd.baseline import GCN as G2, GCRN as R2
    assert G2 is GCN and R2 is GCRN
    m = GCRN(30, 7, 20, 16, feature_pre=False, layer_num=3, dropout=0.25, bias=False, duration=2, rnn_type='LSTM')
    assert isinstance(m.rnn, torch.nn.LSTM) and len(m.gcn_list) == 2 and m.gcn_list[0].dropout == 0.25
    assert sorted(m.state_dict()) == sorted(["gcn_list.%d.gc%d.weight" % (t, k) for t in range(2) for k in (1, 2)]
                                            + ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "norm.weight", "norm.bias"])
    assert GraphConvolution(5, 3, bias=False).bias is None and repr(GraphConvolution(5, 3)) == "GraphConvolution (5 -> 3)"
    with pytest.raises(AssertionError):
        GCRN(30, 0, 20, 16, rnn_type='RNN')


def test_initialisation_follows_the_reset_parameters_rule():
    from ctgcn_amd import GCN
    model = GCN(400, 50, 30)
    for name, p in model.named_parameters():
        out_dim = 50 if name.startswith("gc1") else 30
        bound = 1.0 / np.sqrt(out_dim)                            # weight and bias alike: 1 / sqrt(weight.size(1))
        top = float(p.detach().abs().max())
        assert (0.5 if p.dim() > 1 else 0.2) * bound < top <= bound, name


def test_dropout_key_comes_from_the_default_generator():
    from ctgcn_amd.baseline.gcn import GCN, draw_key
    model, plain = GCN(8, 4, 2, dropout=0.5), GCN(8, 4, 2, dropout=0.0)
    torch.manual_seed(5)
    a = draw_key(model)
    torch.manual_seed(5)
    assert draw_key(model) == a and 0 <= a < 2 ** 62
    assert draw_key(model) != a
    state = torch.random.get_rng_state()
    assert draw_key(model.eval()) == 0 and draw_key(plain) == 0
    assert torch.equal(state, torch.random.get_rng_state())      # no draw where nothing is dropped


def test_trainers_accept_gcrn_and_not_gcn():
    from ctgcn_amd import embedding
    assert "GCRN" in embedding._SUPPORTED and "GCRN" not in embedding._S_MODELS
    assert "GCN" not in embedding._SUPPORTED


def test_cpu_tensors_raise():
    from ctgcn_amd import GCN, GCRN, ops
    from ctgcn_amd._lib import CtgcnHipError
    eye = torch.eye(8).to_sparse()
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        GCN(8, 4, 2)(eye, eye)
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        GCN(8, 4, 2)([torch.zeros(8, 8)], [eye])
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        GCRN(8, 0, 4, 2, duration=1)([eye], [eye])

    class Adj(object):                                          # stands in for a GcnAdj: gcn_conv refuses before it reads one
        val = torch.zeros(0)

    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.gcn_conv(torch.zeros(8, 4), Adj())
