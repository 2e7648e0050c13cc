"""Host checks of the VGRNN baseline: the torch mirror (tests/_vgrnn_ref.py) against the reference's recorded results
(tests/golden/vgrnn_uci.npz), the decomposed decoder loss against the dense one, the new C entry points' argument checks, and the
module's interface and refusals.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _vgrnn_ref as V
from conftest import check_sampled_tensor, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_vae_nll_tile", "ctgcn_vae_nll_workspace_bytes", "ctgcn_vae_nll_dense_f32", "ctgcn_vae_nll_entries_f32",
               "ctgcn_vgrnn_bwd_prep_f32", "ctgcn_ggru_gates_fwd_f32", "ctgcn_ggru_blend_fwd_f32", "ctgcn_vgrnn_heads_fwd_f32")
KEYS = sorted(["%s.%s" % (m, p) for m in ("phi_x.0", "phi_z.0", "enc", "enc_mean", "enc_std", "prior.0", "prior_mean.0", "prior_std.0")
               for p in ("weight", "bias")]
              + ["rnn.weight_%s.0.%s" % (g, p) for g in ("xz", "hz", "xr", "hr", "xh", "hh") for p in ("weight", "bias")])
_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def mirror_run(dtype):
    if dtype not in _runs:
        g = V.fixture()
        model = V.build(V.VgrnnMirror)
        seeded_parameters(model, int(g["seed"]))
        model = model.to(dtype).train()
        x, edges, adj, noise = V.identity_features(dtype), V.edge_lists(), V.target_adjacency(dtype), V.noise(dtype)

        def forward_loss():
            emb, h, data = model(x, edges, None, noise)
            return emb, h, V.vae_loss(data, adj)

        _runs[dtype] = V.adam_run(model, forward_loss)
    losses, (outs, h, grads) = _runs[dtype]
    return losses, outs, h, grads


def test_mirror_float64_matches_the_reference():
    g = V.fixture()
    losses, outs, h, grads = mirror_run(torch.float64)
    assert sorted(grads) == KEYS == [str(k) for k in g["keys"]] and len(KEYS) == 28
    for k, shape in zip(g["keys"], g["shapes"]):
        assert ",".join(str(s) for s in grads[str(k)].shape) == str(shape)
    for t in range(V.T):
        check_sampled_tensor(g, "out_t%d" % t, outs[t].numpy(), 1e-9, 1e-9)
    check_sampled_tensor(g, "h", h.numpy(), 1e-9, 1e-9)
    for k in g["keys"]:
        check_sampled_tensor(g, "grad_%s" % k, grads[str(k)].numpy(), 1e-9, 1e-9)
    assert np.abs(np.asarray(losses) - g["losses"]).max() <= 1e-9 * np.abs(g["losses"]).max()


def test_mirror_float32_is_within_twice_the_reference_s_own_float32_error():
    g = V.fixture()
    losses, outs, h, grads = mirror_run(torch.float32)

    def worst(got, key):
        ref, pick, top = stored(g, key)
        got = got.double().numpy().reshape(-1)
        return np.abs((got if pick is None else got[pick]) - ref).max() / top

    for t in range(V.T):
        assert worst(outs[t], "out_t%d" % t) <= 2 * g["yard_out"][t], t
    assert worst(h, "h") <= 2 * float(g["yard_h"])
    for k, yard in zip(g["keys"], g["yard_grad"]):
        assert worst(grads[str(k)], "grad_%s" % k) <= max(2 * yard, 1e-6), str(k)
    assert np.abs(np.asarray(losses) - g["losses"]).max() <= max(2 * float(g["yard_losses"]), 2e-7) * np.abs(g["losses"]).max()


def small_case(n=37, d=5, seed=3):
    gen = torch.Generator().manual_seed(seed)
    z = torch.randn(n, d, generator=gen, dtype=torch.float64)
    rows, cols = torch.randint(0, n, (90,), generator=gen), torch.randint(0, n, (90,), generator=gen)       # asymmetric, with duplicates
    rows, cols = torch.cat([rows, torch.arange(4)]), torch.cat([cols, torch.arange(4)])                     # and stored diagonal entries
    w = torch.rand(rows.numel(), generator=gen, dtype=torch.float64) + 0.5
    return z, torch.sparse_coo_tensor(torch.stack((rows, cols)), w, (n, n)).coalesce()


def test_decomposed_loss_equals_the_dense_one_in_float64():
    z, target = small_case()
    z.requires_grad_(True)
    dense = V.dense_nll(z @ z.t(), target.to_dense())
    dec = V.decomposed_nll(z, target)
    assert abs(float(dense) - float(dec)) <= 1e-13 * abs(float(dense))
    g1, = torch.autograd.grad(dense, z)
    g2, = torch.autograd.grad(dec, z)
    assert float((g1 - g2).abs().max()) <= 1e-13 * float(g1.abs().max())


def test_two_layers_match_the_six_convolution_form():
    """rnn_layer_num 2 cannot be pinned to the reference (its in-place h_out[i] fails in autograd): the mirror's stacked cell against
    the six convolutions written out by hand, layer 1 fed layer 0's new state"""
    torch.manual_seed(5)
    n, hid = 23, 6
    edges = torch.randint(0, n, (2, 70))
    adj = V.normalized_adjacency(edges, n)
    rnn = V.GruMirror(2 * hid, hid, 2).double()
    for p in rnn.parameters():
        p.data.normal_(0, 0.3)
    x, h = torch.randn(n, 2 * hid, dtype=torch.float64), torch.randn(2, n, hid, dtype=torch.float64)
    got = rnn(x, adj, h)
    dense = adj.to_dense()
    inp = x
    for i in range(2):
        conv = lambda m, v: dense @ (v @ m[i].weight) + m[i].bias  # noqa: E731
        z = torch.sigmoid(conv(rnn.weight_xz, inp) + conv(rnn.weight_hz, h[i]))
        r = torch.sigmoid(conv(rnn.weight_xr, inp) + conv(rnn.weight_hr, h[i]))
        cand = torch.tanh(conv(rnn.weight_xh, inp) + conv(rnn.weight_hh, r * h[i]))
        inp = z * h[i] + (1 - z) * cand
        assert float((got[i] - inp).abs().max()) <= 1e-12
    # a listed (i, i) ends up as 3 before the normalisation, every other listed entry as its count
    raw = V.normalized_adjacency(torch.tensor([[0, 0, 1], [0, 1, 0]]), 2)
    deg = torch.tensor([4.0, 3.0], dtype=torch.float64)                  # row 0: (0,0) + (0,1) + loop 2; row 1: (1,0) + loop 2
    want = torch.tensor([[3.0, 1.0], [1.0, 2.0]], dtype=torch.float64) / torch.sqrt(deg[:, None] * deg[None, :])
    assert float((raw.to_dense() - want).abs().max()) <= 1e-15


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_vgrnn.hip" for s in build.SRCS)
    assert lib.ctgcn_vae_nll_tile() == 32


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def dense(n=40, d=8, Z=p, ldz=8, dZ=p, lddz=8, loss=p, ws=p, wsb=1 << 10):
        return lib.ctgcn_vae_nll_dense_f32(n, d, Z, ldz, dZ, lddz, loss, ws, wsb, None)

    def entries(n=40, nnz=100, d=8, rp=p, col=p, val=p, Z=p, ldz=8, pw=3.0, coef=p, loss=p, ws=p, wsb=1 << 10):
        return lib.ctgcn_vae_nll_entries_f32(n, nnz, d, rp, col, val, Z, ldz, pw, coef, loss, ws, wsb, None)

    for call in (dense, entries):
        assert call(n=-1) == INVALID and call(n=2 ** 31) == INVALID and call(d=0) == INVALID
        assert call(Z=None) == INVALID and call(ldz=7) == INVALID
        assert call(ws=None, wsb=0) == WORKSPACE and call(ws=ctypes.c_void_p(68)) == WORKSPACE
        assert call(n=0) == 0
    assert dense(loss=None) == INVALID and dense(lddz=7) == INVALID
    assert dense(n=65, wsb=16) == WORKSPACE                      # three row tiles need 24 bytes
    assert b"vae_nll_dense" in lib.ctgcn_last_error()
    assert entries(nnz=-1) == INVALID and entries(rp=None) == INVALID and entries(col=None) == INVALID and entries(val=None) == INVALID
    assert entries(coef=None) == INVALID and entries(nnz=0) == 0
    assert entries(nnz=33, wsb=16) == WORKSPACE                  # three blocks of 16 entries need 24 bytes
    assert b"vae_nll_entries" in lib.ctgcn_last_error()
    assert lib.ctgcn_vae_nll_workspace_bytes(65, 0) == 24 and lib.ctgcn_vae_nll_workspace_bytes(1, 33) == 24
    assert lib.ctgcn_vae_nll_workspace_bytes(-1, 0) == 0


def test_fused_gathers_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE = -1, -3
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def gates(n=4, w=8, rp=p, col=p, val=p, src=p, ld=24, b=p, h=p, ldh=8, o=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_ggru_gates_fwd_f32(n, w, rp, col, val, src, ld, b, h, ldh, o, o, o, o, lr, nl, thr, ws, wsb, None)

    def blend(n=4, w=8, rp=p, col=p, val=p, src=p, ld=8, b=p, h=p, ldh=8, o=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_ggru_blend_fwd_f32(n, w, rp, col, val, src, ld, b, 8, b, 8, h, ldh, o, o, lr, nl, thr, ws, wsb, None)

    def heads(n=4, w=8, rp=p, col=p, val=p, src=p, ld=16, b=p, h=p, ldh=8, o=p, lr=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_vgrnn_heads_fwd_f32(n, w, rp, col, val, src, ld, b, h, ldh, o, o, o, lr, nl, thr, ws, wsb, None)

    for call, segs in ((gates, 3), (blend, 1), (heads, 2)):
        assert call(n=-1) == INVALID and call(n=2 ** 31) == INVALID and call(w=0) == INVALID
        assert call(rp=None) == INVALID and call(col=None) == INVALID and call(val=None) == INVALID
        assert call(src=None) == INVALID and call(h=None) == INVALID and call(o=None) == INVALID
        assert call(ld=8 * segs - 1) == INVALID and call(ldh=7) == INVALID
        assert call(nl=1, lr=None) == INVALID and call(nl=5, lr=p) == INVALID
        assert call(nl=1, lr=p, thr=0, ws=p, wsb=1 << 20) == INVALID
        assert call(nl=1, lr=p, ws=None, wsb=0) == WORKSPACE
        assert call(nl=1, lr=p, ws=p, wsb=32 * segs - 16) == WORKSPACE        # one piece of a row of width 8 segs needs 32 segs bytes
        assert call(n=0) == 0
    assert blend(b=None) == INVALID
    assert b"ggru_blend_fwd" in lib.ctgcn_last_error()

    def prep(mode=0, n=4, w=8, g0=p, g1=p, g2=p, ldg=8, s0=p, s1=p, s2=p, lds=8, G=p, ldG=24, x0=p, x1=p, db=None, ws=None, wsb=0):
        return lib.ctgcn_vgrnn_bwd_prep_f32(mode, n, w, g0, ldg, g1, ldg, g2, ldg, s0, lds, s1, lds, s2, lds, G, ldG, x0, x1, db, ws, wsb, None)

    assert prep(mode=3) == INVALID and prep(mode=-1) == INVALID
    for mode, segs in ((0, 3), (1, 1), (2, 2)):
        assert prep(mode, n=-1) == INVALID and prep(mode, n=2 ** 31) == INVALID and prep(mode, w=0) == INVALID
        assert prep(mode, s0=None) == INVALID and prep(mode, s1=None) == INVALID and prep(mode, G=None) == INVALID
        assert prep(mode, ldg=7) == INVALID and prep(mode, lds=7) == INVALID and prep(mode, ldG=8 * segs - 1) == INVALID
        assert prep(mode, n=0) == 0
    assert prep(0, s2=None) == INVALID and prep(0, x0=None) == INVALID
    assert prep(1, g0=None) == INVALID and prep(1, x1=None) == INVALID and prep(1, s2=None) == INVALID
    assert prep(0, db=p, ws=None, wsb=0) == WORKSPACE and prep(2, db=p, ws=p, wsb=32) == WORKSPACE      # one block of width 16 needs 64 bytes
    assert prep(0, db=p, ws=ctypes.c_void_p(68), wsb=1 << 20) == WORKSPACE
    assert b"vgrnn_bwd_prep" in lib.ctgcn_last_error()


def test_interface_and_refusals():
    import ctgcn_amd
    from ctgcn_amd import _lib, baseline, embedding, metrics, ops
    for name in ("VGRNN", "GCNConv", "graph_gru_gcn", "InnerProductDecoder"):
        assert name in ctgcn_amd.__all__ and getattr(ctgcn_amd, name) is getattr(baseline, name)
    assert "VAELoss" in ctgcn_amd.__all__ and "VAEClassificationLoss" in ctgcn_amd.__all__
    assert "VGRNN" in embedding._SUPPORTED and "VGRNN" not in embedding._S_MODELS and "GCN" not in embedding._SUPPORTED
    model = ctgcn_amd.VGRNN(12, 6, 4, 1)
    assert model.method_name == "VGRNN" and sorted(model.state_dict()) == KEYS
    assert tuple(model.enc.weight.shape) == (12, 6) and tuple(model.rnn.weight_xz[0].weight.shape) == (12, 6)
    assert float(model.enc.bias.abs().max()) == 0.0              # zero bias, glorot weight
    assert float(model.enc.weight.abs().max()) <= np.sqrt(6.0 / 18) + 1e-7
    mirror = V.VgrnnMirror(12, 6, 4, 1)
    mirror.load_state_dict(model.state_dict())                   # checkpoints move both ways
    model.load_state_dict(mirror.state_dict())
    two = ctgcn_amd.VGRNN(12, 6, 4, 2)
    assert len(two.state_dict()) == 40 and tuple(two.rnn.weight_xz[1].weight.shape) == (6, 6)
    model.reset_parameters(0.1)
    for kind in ("SAGE", "GIN"):
        with pytest.raises(NotImplementedError, match=kind):
            ctgcn_amd.VGRNN(12, 6, 4, 1, conv_type=kind)
    # CPU tensors
    x = [torch.eye(12)]
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        model(x, [torch.zeros(2, 3, dtype=torch.int64)])
    z, target = small_case()
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        metrics.VAELoss()([[z], [z], [z], [z], [baseline.LazyInnerProduct(z.float())], [target.float()]])
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.vae_nll(z.float(), type("A", (), {"val": z, "n": z.shape[0]})())
    # S = 0: the dense form refuses on the host; the kernel path refuses the same way (tests/test_gpu_vgrnn.py)
    empty = torch.sparse_coo_tensor(torch.zeros(2, 0, dtype=torch.int64), torch.zeros(0), (5, 5))
    zz = torch.zeros(5, 5)
    with pytest.raises(ValueError, match="sum to 0"):
        metrics.VAELoss()([[zz], [zz + 1], [zz], [zz + 1], [zz], [empty]])
    # the trainers: a foreign module that carries the name, the wrong loss, a missing edge_list
    class Foreign(torch.nn.Module):
        method_name = "VGRNN"

    def trainer(m, loss):
        t = object.__new__(embedding.UnsupervisedEmbedding)
        t.loss = loss
        return t

    with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline.VGRNN"):
        trainer(None, metrics.VAELoss())._check_model(Foreign())
    with pytest.raises(ValueError, match="VAELoss"):
        trainer(None, metrics.NegativeSamplingLoss.__new__(metrics.NegativeSamplingLoss))._check_model(model)
    assert trainer(None, metrics.VAELoss())._check_model(model) == "VGRNN"
    with pytest.raises(ValueError, match="edge_list"):
        embedding._check_edge_list("VGRNN", None, 3)
    with pytest.raises(ValueError, match="edge_list"):
        embedding._check_edge_list("VGRNN", [1, 2], 3)
    embedding._check_edge_list("GCN", None, 3)
    sup = object.__new__(embedding.SupervisedEmbedding)
    sup.loss = metrics.VAEClassificationLoss(3)
    assert sup._check_model(model) == "VGRNN"
    sup.loss = metrics.ClassificationLoss(3)
    with pytest.raises(ValueError, match="VAEClassificationLoss"):
        sup._check_model(model)


def test_dense_vae_loss_matches_the_mirror_on_the_host():
    """metrics.VAELoss on dense logits is stock torch ops: any device"""
    from ctgcn_amd import metrics
    z, target = small_case()
    mean, std = z[:, :2], z[:, 2:4].abs() + 0.1
    data = [[mean], [std], [mean * 0.5], [std + 0.2], [z @ z.t()]]
    got = metrics.VAELoss()(data + [[target]])
    want = V.vae_loss(data, [target])
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
