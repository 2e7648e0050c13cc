"""Host checks of the PyG-variant baselines (TgGCN, TgGAT, TgSAGE, TgGIN): the new C entry points' declarations and argument checks,
the modules' interface, state_dict keys and initialisers, the trainers' gates, and the stock-torch mirror (tests/_tg_ref.py) against
dense-matrix forms of the same formulas in float64.  No GPU needed."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch

import _tg_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_tg_keys", "ctgcn_tg_csr_count", "ctgcn_tg_csr_emit", "ctgcn_tg_conv_fwd_f32", "ctgcn_tg_prep_workspace_bytes",
               "ctgcn_tg_conv_prep_f32", "ctgcn_tgat_fwd_f32", "ctgcn_tgat_bwd_row_f32", "ctgcn_tgat_bwd_col_f32")


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_tg.hip" for s in build.SRCS)
    assert lib.ctgcn_tg_prep_workspace_bytes(64, 8) == 32 and lib.ctgcn_tg_prep_workspace_bytes(65, 6) == 64
    assert lib.ctgcn_tg_prep_workspace_bytes(-1, 8) == 0 and lib.ctgcn_tg_prep_workspace_bytes(4, 0) == 0


def _lds(call):
    return [k for k in inspect.signature(call).parameters if k.startswith("ld")]


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch
    nan, inf = float("nan"), float("inf")

    def conv(n=4, d=8, rp=p, col=p, val=p, S=p, lds=8, T=p, ldt=8, b=p, Y=p, ldy=8, epi=1, pd=0.0, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_tg_conv_fwd_f32(n, d, rp, col, val, S, lds, T, ldt, 1.0, b, Y, ldy, epi, pd, 1, lr, nl, thr, ws, wsb, None)

    def prep(n=4, d=8, dY=p, lddy=8, Y=p, ldy=8, b=None, epi=1, pd=0.0, G_=p, ldg=8, db=None, ws=None, wsb=0):
        return lib.ctgcn_tg_conv_prep_f32(n, d, dY, lddy, Y, ldy, b, epi, pd, 1, G_, ldg, db, ws, wsb, None)

    def fwd(n=4, d=8, heads=2, rp=p, col=p, S=p, lds=8, at=p, asrc=p, slope=0.2, b=p, epi=1, pd=0.0, out=p, ldout=8, Y=p, ldy=8, u=p, v=p, m=p,
            Z=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_tgat_fwd_f32(n, d, heads, rp, col, S, lds, at, asrc, slope, b, epi, pd, 1, out, ldout, Y, ldy, u, v, m, Z, lr, nl, thr, ws,
                                      wsb, None)

    def row(n=4, d=8, heads=2, rp=p, col=p, S=p, lds=8, G_=p, ldg=8, Y=p, ldy=8, v=p, pack=p, slope=0.2, R_=p, ldr=8, cs=p, du=p, lr=None, nl=0,
            thr=8, ws=None, wsb=0):
        return lib.ctgcn_tgat_bwd_row_f32(n, d, heads, rp, col, S, lds, G_, ldg, Y, ldy, v, pack, slope, R_, ldr, cs, du, lr, nl, thr, ws, wsb, None)

    def colp(n=4, d=8, heads=2, rp=p, col=p, G_=p, ldg=8, S=p, lds=8, v=p, pack=p, at=p, asrc=p, slope=0.2, du=p, dS=p, ldds=8, B=p, ldb=8,
             ks=p, dv=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_tgat_bwd_col_f32(n, d, heads, rp, col, G_, ldg, S, lds, v, pack, at, asrc, slope, du, dS, ldds, B, ldb, ks, dv, lr, nl,
                                          thr, ws, wsb, None)

    for call in (conv, prep, fwd, row, colp):
        assert call(n=-1) == INVALID and call(n=2 ** 31) == INVALID and call(d=0) == INVALID, call.__name__
        for ld in _lds(call):
            assert call(**{ld: 7}) == INVALID, (call.__name__, ld)
        assert call(n=0) == 0
    for call in (fwd, row, colp):
        assert call(heads=0) == INVALID and call(d=9, heads=2, **{k: 9 for k in _lds(call)}) == INVALID
        assert call(slope=nan) == INVALID and call(slope=inf) == INVALID
    for call in (conv, fwd, row, colp):
        assert call(rp=None) == INVALID and call(col=None) == INVALID and call(S=None) == INVALID
        assert call(nl=1, lr=None) == INVALID and call(nl=5, lr=p) == INVALID
        assert call(nl=1, lr=p, thr=0, ws=p, wsb=1 << 20) == INVALID
        assert call(nl=1, lr=p, ws=None, wsb=0) == WORKSPACE
        assert call(nl=1, lr=p, ws=p, wsb=4 * 4) == WORKSPACE
        assert call(nl=1, lr=p, ws=ctypes.c_void_p(68), wsb=1 << 20) == WORKSPACE
    for call in (conv, prep, fwd):
        assert call(pd=1.0) == INVALID and call(pd=-0.1) == INVALID and call(pd=nan) == INVALID
        assert call(epi=2) == INVALID and call(epi=-1) == INVALID
        assert call(Y=None) == INVALID
    assert conv(val=None) == INVALID
    assert b"tg_conv_fwd" in lib.ctgcn_last_error()
    assert prep(dY=None) == INVALID and prep(G_=None) == INVALID and prep(epi=0) == INVALID           # epi 0 without db: nothing to compute
    assert prep(db=p, ws=None) == WORKSPACE and prep(db=p, ws=p, wsb=31) == WORKSPACE and prep(db=p, ws=ctypes.c_void_p(68), wsb=64) == WORKSPACE
    assert b"tg_conv_prep" in lib.ctgcn_last_error()
    assert fwd(at=None) == INVALID and fwd(asrc=None) == INVALID and fwd(out=None) == INVALID
    assert fwd(u=None) == INVALID and fwd(v=None) == INVALID and fwd(m=None) == INVALID and fwd(Z=None) == INVALID
    assert b"tgat_fwd" in lib.ctgcn_last_error()
    assert row(Y=None) == INVALID and row(G_=None) == INVALID and row(v=None) == INVALID and row(pack=None) == INVALID and row(R_=None) == INVALID
    assert row(cs=None) == INVALID and row(du=None) == INVALID and row(pack=ctypes.c_void_p(68)) == INVALID
    assert b"tgat_bwd_row" in lib.ctgcn_last_error()
    assert colp(G_=None) == INVALID and colp(v=None) == INVALID and colp(pack=None) == INVALID and colp(B=None) == INVALID
    assert colp(ks=None) == INVALID and colp(dv=None) == INVALID and colp(at=None) == INVALID and colp(asrc=None) == INVALID
    assert colp(du=None) == INVALID and colp(dS=None) == INVALID          # du and dS go together
    assert b"tgat_bwd_col" in lib.ctgcn_last_error()
    # the reference-form entry points still refuse the new epilogue value
    assert lib.ctgcn_gat_fwd_f32(4, 8, 2, p, p, p, 8, p, p, 0.2, 3, 0.0, 1, 0.0, 2, p, 8, p, 8, p, p, p, p, None, 0, 8, None, 0, None) == INVALID

    def keys(E=4, n=4, src=p, dst=p, k=p, flag=p):
        return lib.ctgcn_tg_keys(E, n, src, dst, k, flag, None)

    def count(E=4, n=4, k=p, raw=p, at=p, nl=p):
        return lib.ctgcn_tg_csr_count(E, n, k, raw, at, nl, None)

    def emit(E=4, n=4, k=p, raw=p, at=p, nl=p, lp=p, col=p, mean=p, cl=p, vl=p):
        return lib.ctgcn_tg_csr_emit(E, n, k, raw, at, nl, lp, col, mean, cl, vl, None)

    for call in (keys, count, emit):
        assert call(E=-1) == INVALID and call(n=-1) == INVALID and call(n=2 ** 31) == INVALID
        assert call(E=2 ** 31 - 4) == INVALID and call(E=2 ** 31 - 3, n=3) == INVALID          # E >= 2^31 - n
        assert call(k=None) == INVALID
    assert keys(src=None) == INVALID and keys(dst=None) == INVALID and keys(flag=None) == INVALID and keys(E=0) == 0
    assert count(raw=None) == INVALID and count(at=None) == INVALID and count(nl=None) == INVALID
    assert emit(raw=None) == INVALID and emit(lp=None) == INVALID and emit(col=None) == INVALID and emit(mean=None) == INVALID
    assert emit(cl=None) == INVALID and emit(vl=None) == INVALID and emit(E=0, n=0) == 0
    assert b"tg_csr_emit" in lib.ctgcn_last_error()


def _expected_keys(kind, feature_pre, layer_num, bias):
    keys = []
    if feature_pre:
        keys += ["linear_pre.weight"] + (["linear_pre.bias"] if bias else [])
    for name in ["conv_first"] + ["conv_hidden.%d" % i for i in range(layer_num - 2)] + ["conv_out"]:
        if kind == "TgGCN":
            keys += [name + ".weight"] + ([name + ".bias"] if bias else [])
        elif kind == "TgGAT":
            keys += [name + ".att_l", name + ".att_r", name + ".lin_l.weight", name + ".lin_r.weight"] + ([name + ".bias"] if bias else [])
        elif kind == "TgSAGE":
            keys += [name + ".lin_l.weight", name + ".lin_r.weight"] + ([name + ".lin_l.bias"] if bias else [])
        else:
            twin = name.replace("conv_hidden.", "conv_hidden_nn.") if "hidden" in name else name + "_nn"
            keys += [name + ".eps", name + ".nn.weight", twin + ".weight"] + ([name + ".nn.bias", twin + ".bias"] if bias else [])
    return sorted(keys)


@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("layer_num", [2, 3])
@pytest.mark.parametrize("feature_pre", [True, False])
@pytest.mark.parametrize("kind", G.KINDS)
def test_constructor_attributes_and_state_dict_keys(kind, feature_pre, layer_num, bias):
    import ctgcn_amd
    cls = getattr(ctgcn_amd, kind)
    m = cls(30, 12, 10, 6, feature_pre=feature_pre, layer_num=layer_num, dropout=0.25, bias=bias, unused_keyword=1)
    assert m.method_name == kind
    assert (m.input_dim, m.feature_dim, m.hidden_dim, m.output_dim) == (30, 12, 10, 6)
    assert (m.feature_pre, m.layer_num, m.dropout, m.bias) == (feature_pre, layer_num, 0.25, bias)
    assert hasattr(m, "linear_pre") == feature_pre and len(m.conv_hidden) == layer_num - 2
    sd = m.state_dict()
    assert sorted(sd) == _expected_keys(kind, feature_pre, layer_num, bias)
    first_in = 12 if feature_pre else 30
    shapes = {"TgGCN": ("conv_first.weight", (first_in, 10)), "TgGAT": ("conv_first.lin_l.weight", (10, first_in)),
              "TgSAGE": ("conv_first.lin_r.weight", (10, first_in)), "TgGIN": ("conv_first.nn.weight", (10, first_in))}
    key, shape = shapes[kind]
    assert tuple(sd[key].shape) == shape
    if kind == "TgGAT":
        assert tuple(sd["conv_out.att_l"].shape) == (1, 1, 6) and m.conv_first.lin_l.weight is m.conv_first.lin_r.weight
    if kind == "TgGIN":
        assert tuple(sd["conv_out.eps"].shape) == (1,) and float(sd["conv_out.eps"]) == 0.0
        assert m.conv_first.nn is m.conv_first_nn and "conv_first.eps" not in dict(m.named_parameters())
    mirror = G.TgMirror(kind, 30, 12, 10, 6, feature_pre=feature_pre, layer_num=layer_num, bias=bias)
    mirror.load_state_dict(sd)            # strict: same keys and shapes both ways
    m.load_state_dict(mirror.state_dict())


def test_defaults_exports_and_initialisers():
    import ctgcn_amd
    from ctgcn_amd import baseline, embedding
    names = ("TgGCN", "TgGAT", "TgSAGE", "TgGIN", "TgGCNConv", "TgGATConv", "TgSAGEConv", "TgGINConv")
    for name in names:
        assert getattr(baseline, name) is getattr(ctgcn_amd, name) and name in ctgcn_amd.__all__
    sig = inspect.signature(ctgcn_amd.TgGIN.__init__).parameters
    assert sig["dropout"].default is True and sig["feature_pre"].default is True and sig["layer_num"].default == 2
    assert inspect.signature(ctgcn_amd.TgSAGE.__init__).parameters["dropout"].default == 0.5
    for kind in G.KINDS:
        assert kind in embedding._SUPPORTED and kind not in embedding._S_MODELS
    assert "GCN" not in embedding._SUPPORTED
    torch.manual_seed(5)

    def top(t):
        return float(t.detach().abs().max())

    gcn = ctgcn_amd.TgGCNConv(300, 200)
    bound = math.sqrt(6.0 / 500)
    assert 0.99 * bound < top(gcn.weight) <= bound and top(gcn.bias) == 0.0
    gat = ctgcn_amd.TgGATConv(300, 200)
    assert 0.99 * bound < top(gat.lin_l.weight) <= bound
    ab = math.sqrt(6.0 / 201)            # glorot over the last two sizes of [1, 1, out]
    for att in (gat.att_l, gat.att_r):
        assert 0.9 * ab < top(att) <= ab
    assert top(gat.bias) == 0.0
    sage = ctgcn_amd.TgSAGEConv(300, 200)
    lb = 1.0 / math.sqrt(300)            # nn.Linear's own reset
    for t in (sage.lin_l.weight, sage.lin_l.bias, sage.lin_r.weight):
        assert 0.9 * lb < top(t) <= lb
    with pytest.raises(TypeError, match="Linear"):
        ctgcn_amd.TgGINConv(torch.nn.Sequential(torch.nn.Linear(4, 4)))


@pytest.mark.parametrize("kind", G.KINDS)
def test_cpu_tensors_raise(kind):
    import ctgcn_amd
    from ctgcn_amd import ops
    from ctgcn_amd._lib import CtgcnHipError
    model = getattr(ctgcn_amd, kind)(6, 4, 4, 2, dropout=0.0)
    ei, _ = G.small_graph()
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        model(torch.zeros(6, 6), ei)
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        model([torch.eye(6).to_sparse()], [ei])
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.TgGraph(ei, 6)

    class Adj(object):                                          # stands in for a GcnAdj: the ops refuse before they read one
        val = torch.zeros(0)

    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.tg_conv(torch.zeros(6, 4), Adj())
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        ops.tgat_conv(torch.zeros(6, 4), torch.zeros(1, 4), torch.zeros(1, 4), Adj())


@pytest.mark.parametrize("kind", G.KINDS)
def test_trainers_accept_the_names_and_gate_what_they_cannot_run(kind, tmp_path):
    import ctgcn_amd
    from ctgcn_amd import embedding

    class Foreign(torch.nn.Module):
        method_name = kind

    class Loss(ctgcn_amd.NegativeSamplingLoss):
        def __init__(self):
            torch.nn.Module.__init__(self)

    class Cls(ctgcn_amd.ClassificationLoss):
        def __init__(self):
            torch.nn.Module.__init__(self)

    model = getattr(ctgcn_amd, kind)(6, 4, 4, 2)
    for trainer_cls, loss in ((embedding.UnsupervisedEmbedding, Loss()), (embedding.SupervisedEmbedding, Cls())):
        trainer = object.__new__(trainer_cls)
        trainer.loss = loss
        assert trainer._check_model(model) == kind
        with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline." + kind):
            trainer._check_model(Foreign())
    with pytest.raises(ValueError, match=kind + " needs edge_list"):
        embedding._check_edge_list(kind, None, 3)
    with pytest.raises(ValueError, match=kind + " needs edge_list"):
        embedding._check_edge_list(kind, [None, None], 3)
    with pytest.raises(ValueError, match="a VGRNN needs edge_list: one \\[2, E\\] index tensor \\(or prepared adjacency\\) per snapshot"):
        embedding._check_edge_list("VGRNN", None, 3)
    embedding._check_edge_list("GAT", None, 3)
    seen = {}

    class Probe(torch.nn.Module):
        method_name = kind

        def forward(self, x, second):
            seen["second"] = second
            return x

    assert embedding.model_forward(Probe(), "x", None, None, 6, "cpu", edge_list="edges") == "x" and seen["second"] == "edges"


# ------------------------------------------------------------------------------------------------ the mirror against itself
def _small_inputs():
    ei, n = G.small_graph()
    rng = np.random.default_rng(3)
    t = lambda *shape: torch.from_numpy(rng.uniform(-1.0, 1.0, shape))
    return ei, n, t


def test_edge_wise_mirror_equals_the_dense_matrix_formulas():
    ei, n, t = _small_inputs()
    x = t(n, 5)
    cases = {
        "gcn": (G.gcn_conv, G.dense_gcn, (x, t(5, 3), t(3), ei)),
        "gat": (G.gat_conv, G.dense_gat, (x, t(3, 5), t(1, 1, 3), t(1, 1, 3), t(3), ei)),
        "sage": (G.sage_conv, G.dense_sage, (x, t(3, 5), t(3), t(3, 5), ei)),
        "gin": (G.gin_conv, G.dense_gin, (x, t(3, 5), t(3), 0.25, ei)),
    }
    for name, (edge_wise, dense, args) in cases.items():
        got, want = edge_wise(*args), dense(*args)
        assert got.dtype == torch.float64 and float((got - want).abs().max()) <= 1e-14 * float(want.abs().max()), name


def test_gat_and_gcn_share_one_pattern_with_one_loop_per_node():
    ei, n, _ = _small_inputs()
    src, tgt = G.looped_edges(ei, n)
    s2, t2, w = G.gcn_norm(ei, n, torch.float64)
    assert torch.equal(src, s2) and torch.equal(tgt, t2)
    pairs = list(zip(src.tolist(), tgt.tolist()))
    assert all(pairs.count((v, v)) == 1 for v in range(n)) and pairs.count((0, 1)) == 2
    assert len(pairs) == ei.shape[1] - 3 + n                      # three input loops leave, one per node enters
    host = G.host_graph(ei.numpy(), n)
    row_ptr, col, val = host["looped"]
    assert list(np.diff(row_ptr)) == [2, 4, 1, 1, 3, 1] and list(col[row_ptr[1]:row_ptr[2]]) == [0, 0, 1, 4]
    A = torch.zeros(n, n, dtype=torch.float64).index_put_((tgt, src), w, accumulate=True)
    B = np.zeros((n, n))
    np.add.at(B, (np.repeat(np.arange(n), np.diff(row_ptr)), col), val)
    assert np.abs(A.numpy() - B).max() <= 1e-15
    raw_ptr, rcol, mean = host["raw"]
    assert list(np.diff(raw_ptr)) == [1, 3, 2, 1, 2, 0] and list(mean[raw_ptr[1]:raw_ptr[2]]) == [1 / 3] * 3
