"""Host checks of the EvolveGCN baseline: the torch mirror (tests/_egcn_ref.py) against the reference's recorded results
(tests/golden/egcn_uci.npz), the new C entry points' argument checks, and the module's interface.  No GPU needed."""
import ctypes
import os
import tempfile

import numpy as np
import pytest
import torch

import _egcn_ref as E
from conftest import check_sampled_tensor, load_golden, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_gcn_normalize_workspace_bytes", "ctgcn_gcn_normalize_f32", "ctgcn_gcn_layer_fwd_f32", "ctgcn_gcn_layer_bwd_f32")
_runs = {}


def stored(g, key):
    """(reference values float64, index into the flattened tensor or None, largest magnitude of the tensor) of a put_tensor record"""
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def mirror_run(case, dtype):
    """(losses, outputs, gradients) of the mirror on the fixture's setup, computed once per (case, dtype)"""
    if (case, dtype) not in _runs:
        g = E.fixture()
        model = E.EgcnMirror(E.input_dim(case, g), E.HID, E.OUT, E.egcn_type(case))
        seeded_parameters(model, int(g["seed"]))
        model = model.to(dtype)
        x = E.features(case, g, dtype)
        adj = [E.sparse_tensor(E.normalized_csr(g, t), dtype) for t in range(E.T)]        # the loader's float32 values in both runs
        losses, (outs, grads) = E.adam_losses(model, lambda: model(x, adj), E.surrogate_weights(dtype))
        _runs[case, dtype] = (losses, outs, grads)
    return _runs[case, dtype]


@pytest.mark.parametrize("case", E.CASES)
def test_mirror_float64_matches_the_reference(case):
    g = E.fixture()
    losses, outs, grads = mirror_run(case, torch.float64)
    for t in range(E.T):
        check_sampled_tensor(g, "%s_out_t%d" % (case, t), outs[t].numpy(), 1e-9, 1e-9)
    for k in g[case + "_keys"]:
        check_sampled_tensor(g, "%s_grad_%s" % (case, k), grads[str(k)].numpy(), 1e-9, 1e-9)
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 1e-9 * np.abs(g[case + "_losses"]).max()


@pytest.mark.parametrize("case", E.CASES)
def test_mirror_float32_is_within_twice_the_reference_s_own_float32_error(case):
    g = E.fixture()
    losses, outs, grads = mirror_run(case, torch.float32)

    def worst(got, key):
        ref, pick, top = stored(g, key)
        got = got.double().numpy().reshape(-1)
        return np.abs((got if pick is None else got[pick]) - ref).max() / top

    for t in range(E.T):
        assert worst(outs[t], "%s_out_t%d" % (case, t)) <= 2 * g[case + "_yard_out"][t], (case, t)
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        if stored(g, "%s_grad_%s" % (case, k))[2] == 0:       # EGCNO's unused scorer
            assert float(grads[str(k)].abs().max()) == 0
            continue
        assert worst(grads[str(k)], "%s_grad_%s" % (case, k)) <= 2 * yard, (case, str(k))
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 2 * float(g[case + "_yard_losses"]) * np.abs(g[case + "_losses"]).max()


def test_fixture_meets_the_top_k_gap_condition():
    g = E.fixture()
    assert float(g["min_gap"]) >= 1e-5


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_gcn.hip" for s in build.SRCS)


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch
    assert lib.ctgcn_gcn_normalize_f32(-1, p, p, p, 0, p, p, p, 1 << 20, None) == INVALID
    assert lib.ctgcn_gcn_normalize_f32(4, p, p, p, 2, p, p, p, 1 << 20, None) == INVALID
    assert lib.ctgcn_gcn_normalize_f32(4, None, p, p, 0, p, p, p, 1 << 20, None) == INVALID
    assert lib.ctgcn_gcn_normalize_f32(4, p, p, p, 0, p, None, p, 1 << 20, None) == INVALID
    assert lib.ctgcn_gcn_normalize_f32(4, p, p, p, 0, p, p, p, 8, None) == WORKSPACE
    assert b"gcn_normalize" in lib.ctgcn_last_error()
    assert lib.ctgcn_gcn_normalize_workspace_bytes(10) == 80

    def fwd(n=4, d=8, rp=p, col=p, val=p, S=p, lds=8, Y=p, ldy=8, act=1, sv=None, so=None, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_gcn_layer_fwd_f32(n, d, rp, col, val, S, lds, Y, ldy, act, sv, so, lr, nl, thr, ws, wsb, None)

    def bwd(n=4, d=8, rp=p, col=p, val=p, dY=p, lddy=8, Y=p, ldy=8, act=1, dS=p, ldds=8, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_gcn_layer_bwd_f32(n, d, rp, col, val, dY, lddy, Y, ldy, act, dS, ldds, lr, nl, thr, ws, wsb, None)

    for call in (fwd, bwd):
        assert call(n=-1) == INVALID
        assert call(d=0) == INVALID
        assert call(act=2) == INVALID
        assert call(rp=None) == INVALID
        assert call(val=None) == INVALID
        assert call(ldy=4) == INVALID
        assert call(nl=1, lr=None) == INVALID
        assert call(nl=5, lr=p) == INVALID                       # more long rows than rows
        assert call(nl=1, lr=p, thr=0, ws=p, wsb=1 << 20) == INVALID
        assert call(nl=1, lr=p, ws=None, wsb=0) == WORKSPACE
        assert call(nl=1, lr=p, ws=p, wsb=16) == WORKSPACE       # one piece of a row of width 8 needs 32 bytes
    assert fwd(S=None) == INVALID and fwd(Y=None) == INVALID and fwd(lds=7) == INVALID
    assert fwd(sv=p, so=None) == INVALID and fwd(sv=None, so=p) == INVALID
    assert bwd(dY=None) == INVALID and bwd(dS=None) == INVALID and bwd(Y=None, act=1) == INVALID and bwd(ldds=7) == INVALID
    assert b"gcn_layer_bwd" in lib.ctgcn_last_error()
    assert fwd(n=0) == 0 and bwd(n=0) == 0


@pytest.mark.parametrize("case", E.CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(case):
    from ctgcn_amd import EvolveGCN
    g = E.fixture()
    model = EvolveGCN(E.input_dim(case, g), E.HID, E.OUT, E.egcn_type(case))
    assert model.method_name == "EvolveGCN"
    sd = model.state_dict()
    assert sorted(sd) == [str(k) for k in g[case + "_keys"]]
    for k, shape in zip(g[case + "_keys"], g[case + "_shapes"]):
        assert ",".join(str(s) for s in sd[str(k)].shape) == str(shape), k
    mirror = E.EgcnMirror(E.input_dim(case, g), E.HID, E.OUT, E.egcn_type(case))
    mirror.load_state_dict(sd)            # strict: same keys and shapes both ways
    model.load_state_dict(mirror.state_dict())


def test_initialisation_follows_the_reset_param_rules():
    from ctgcn_amd import EvolveGCN
    model = EvolveGCN(40, 16, 8)
    for name, p in model.named_parameters():
        fan = p.shape[0] if name.endswith("scorer") else p.shape[1]
        bound = 1.0 / np.sqrt(fan)
        top = float(p.detach().abs().max())
        assert 0.5 * bound < top <= bound, name


def test_masks_and_cpu_tensors_raise():
    from ctgcn_amd import EvolveGCN, ops
    from ctgcn_amd._lib import CtgcnHipError
    model = EvolveGCN(24, 16, 16)
    x = [torch.zeros(8, 24)]
    with pytest.raises(NotImplementedError):
        model(x, [None], nodes_mask_list=[torch.zeros(8, 1)])
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        model(x, [torch.eye(8).to_sparse()])
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.GcnAdj(torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.gcn_normalize(torch.zeros(9, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    with pytest.raises(AssertionError):
        EvolveGCN(24, 16, 16, egcn_type="EGCN")


def test_trainers_accept_the_method_and_still_refuse_others():
    from ctgcn_amd import embedding
    assert "EvolveGCN" in embedding._SUPPORTED and "GCN" not in embedding._SUPPORTED
    assert "EvolveGCN" not in embedding._S_MODELS


def test_unnormalised_date_adjacency_is_unchanged():
    import scipy.sparse as sp
    from ctgcn_amd.helper import DataLoader
    from ctgcn_amd._lib import CtgcnHipError
    snaps = load_golden("uci_snapshots.npz")
    names = [str(s) for s in snaps["node_names"]]
    with tempfile.TemporaryDirectory() as tmp:
        for t in range(2):
            with open(os.path.join(tmp, "%d.csv" % t), "w") as fp:
                fp.write("from_id\tto_id\tweight\n")
                for s, o, w in zip(snaps["t%d_src" % t], snaps["t%d_dst" % t], snaps["t%d_w" % t]):
                    fp.write("%s\t%s\t%s\n" % (names[s], names[o], repr(float(w))))
        loader = DataLoader(names, 2, has_cuda=False)
        for add_eye in (False, True):
            mats = loader.get_date_adj_list(tmp, 0, 2, add_eye=add_eye, data_type="matrix")
            tens = loader.get_date_adj_list(tmp, 0, 2, add_eye=add_eye)
            for t in range(2):
                want = E.snapshot_csr(t, with_eye=add_eye)
                assert sp.isspmatrix_coo(mats[t]) and abs(mats[t].tocsr() - want).sum() == 0
                assert tens[t].is_sparse and tens[t].dtype == torch.float32 and tens[t].device.type == "cpu"
                assert np.array_equal(tens[t]._indices().numpy(), np.vstack((mats[t].row, mats[t].col)))
                assert np.array_equal(tens[t]._values().numpy(), mats[t].data.astype(np.float32))
        with pytest.raises(CtgcnHipError, match="no CPU fallback"):
            loader.get_date_adj_list(tmp, 0, 2, normalize=True, add_eye=True)
