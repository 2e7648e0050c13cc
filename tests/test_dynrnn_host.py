"""Host checks of the DynRNN / DynAERNN baselines: the torch mirror (tests/_dynrnn_ref.py) against the reference's recorded results
(tests/golden/dynrnn_uci.npz), the modules' state_dict keys and checkpoints, the new C entry points' declarations and argument checks,
and the interface and its refusals.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _dynrnn_ref as R
from conftest import check_sampled_tensor, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_lstm_cell_fwd_f32", "ctgcn_lstm_cell_bwd_f32")
LSTM_PARAMS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
KEYS = {
    "dynrnn": sorted("%s.layer_list.%d.%s" % (m, i, p) for m in ("encoder", "decoder") for i in range(3) for p in LSTM_PARAMS),
    "dynaernn": sorted(["ae_encoder.layer_list.%d.layer_list.%d.%s" % (t, i, p) for t in range(3) for i in range(3) for p in ("weight", "bias")]
                       + ["rnn_encoder.layer_list.%d.%s" % (i, p) for i in range(2) for p in LSTM_PARAMS]
                       + ["decoder.layer_list.%d.%s" % (i, p) for i in range(3) for p in ("weight", "bias")]),
}
_runs = {}


def mirror_run(method, dtype):
    if (method, dtype) not in _runs:
        import _dyngem_ref as D
        g = R.fixture()
        csr = D.stacked(R.window())
        idx, tgt = R.batch_rows(g)
        x_pre, x_cur = D.dense_rows(csr, idx, dtype), D.dense_rows(csr, tgt, dtype)[:, 0]
        model = R.mirror(method)
        seeded_parameters(model, int(g["seed"]))
        model.to(dtype)
        _runs[(method, dtype)] = D.adam_run(model, lambda: R.model_loss(model, x_pre, x_cur))
    losses, (hx, pred, grads) = _runs[(method, dtype)]
    return losses, hx, pred, grads


def project_model(method, bias=True):
    import ctgcn_amd
    if method == "dynrnn":
        return ctgcn_amd.DynRNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, n_units=R.UNITS, bias=bias, ae_units=[], rnn_units=[])
    return ctgcn_amd.DynAERNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, n_units=[], ae_units=R.UNITS, rnn_units=R.RNN_UNITS, bias=bias)


@pytest.mark.parametrize("method", R.METHODS)
def test_mirror_float64_matches_the_reference(method):
    g = R.fixture()
    losses, hx, pred, grads = mirror_run(method, torch.float64)
    assert sorted(grads) == KEYS[method] == [str(k) for k in g[method + "_keys"]]
    for k, shape in zip(g[method + "_keys"], g[method + "_shapes"]):
        assert ",".join(str(s) for s in grads[str(k)].shape) == str(shape)
    check_sampled_tensor(g, method + "_hx", hx.numpy(), 1e-9, 1e-9)
    check_sampled_tensor(g, method + "_pred", pred.numpy(), 1e-9, 1e-9)
    for k in g[method + "_keys"]:
        check_sampled_tensor(g, "%s_grad_%s" % (method, k), grads[str(k)].numpy(), 1e-9, 1e-9)
    assert np.abs(np.asarray(losses) - g[method + "_losses"]).max() <= 1e-9 * np.abs(g[method + "_losses"]).max()


@pytest.mark.parametrize("method", R.METHODS)
def test_mirror_float32_is_within_the_rule(method):
    """the GPU tests' rule, max(4 x the stored yardstick, floor), holds for the mirror's own float32 run on the CPU"""
    g = R.fixture()
    losses, hx, pred, grads = mirror_run(method, torch.float32)
    assert R.share_used(g, method + "_hx", hx, g[method + "_yard_hx"], 2e-6) <= 1.0
    assert R.share_used(g, method + "_pred", pred, g[method + "_yard_pred"], 2e-6) <= 1.0
    for k, yard in zip(g[method + "_keys"], g[method + "_yard_grad"]):
        assert R.share_used(g, "%s_grad_%s" % (method, k), grads[str(k)], yard, 1e-5) <= 1.0, str(k)
    ref = g[method + "_losses"]
    assert np.abs(np.asarray(losses) - ref).max() <= max(4 * float(g[method + "_yard_losses"]), 2e-6) * np.abs(ref).max()


def test_the_recipe_s_seed_condition_is_recorded():
    g = R.fixture()
    assert int(g["stored_targets"]) >= R.BATCH // 4
    assert len(g["saturated"]) == 8 and g["saturated"].max() <= 0.01              # 6 LSTM layers of DynRNN, 2 of DynAERNN
    assert len(g["active"]) == 12 and g["active"].min() >= 0.2 and g["active"].max() <= 0.8
    graph = g["graph"]
    assert set(graph.tolist()) == {0, 1} and len(graph) == R.BATCH                # both training positions of a node occur
    assert len(R.window()) == 5 and R.LOOK_BACK == 3


def test_the_cell_equations_of_the_mirror_are_those_of_nn_lstm():
    """lstm_dense and cell_bwd against torch's own LSTM and autograd, in float64"""
    gen = torch.Generator().manual_seed(5)
    B, L, I, H = 5, 4, 3, 6
    rnn = torch.nn.LSTM(I, H, batch_first=True).double()
    x = torch.randn(B, L, I, generator=gen, dtype=torch.float64, requires_grad=True)
    want, _ = rnn(x)
    got = R.lstm_dense(x, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)
    assert float((got - want).detach().abs().max()) <= 1e-14
    gi =(torch.randn(B, 4 * H, generator=gen, dtype=torch.float64)).requires_grad_(True)
    c_prev = torch.randn(B, H, generator=gen, dtype=torch.float64, requires_grad=True)
    dh, dc_next = torch.randn(B, H, generator=gen, dtype=torch.float64), torch.randn(B, H, generator=gen, dtype=torch.float64)
    h, c, gates = R.cell_fwd(gi, None, None, c_prev)
    dz, dcp = torch.autograd.grad((h * dh).sum() + (c * dc_next).sum(), (gi, c_prev))
    dgates, dc_prev = R.cell_bwd(gates.detach(), c.detach(), c_prev.detach(), dh, None, dc_next)
    assert float((dgates - dz).abs().max()) <= 1e-14 and float((dc_prev - dcp).abs().max()) <= 1e-14


@pytest.mark.parametrize("method", R.METHODS)
def test_state_dict_keys_shapes_and_checkpoints(method):
    g = R.fixture()
    model = project_model(method)
    state = model.state_dict()
    assert sorted(state) == KEYS[method] == [str(k) for k in g[method + "_keys"]]
    for k, shape in zip(g[method + "_keys"], g[method + "_shapes"]):
        assert ",".join(str(s) for s in state[str(k)].shape) == str(shape), str(k)
    assert model.method_name == {"dynrnn": "DynRNN", "dynaernn": "DynAERNN"}[method] and model.look_back == R.LOOK_BACK
    # checkpoints move both ways between the model and the mirror
    mirror = R.mirror(method)
    seeded_parameters(mirror, 3)
    model.load_state_dict(mirror.state_dict())
    assert all(torch.equal(v, mirror.state_dict()[k]) for k, v in model.state_dict().items())
    seeded_parameters(model, 4)
    mirror.load_state_dict(model.state_dict())
    assert all(torch.equal(v, model.state_dict()[k]) for k, v in mirror.state_dict().items())
    # and between the model's LSTM stack and a stack of nn.LSTM as the reference builds it
    stack = model.encoder if method == "dynrnn" else model.rnn_encoder
    dims = [R.N] + R.UNITS + [R.OUT] if method == "dynrnn" else [R.OUT] + R.RNN_UNITS + [R.OUT]
    plain = torch.nn.ModuleList([torch.nn.LSTM(a, b, bias=True, batch_first=True) for a, b in zip(dims[:-1], dims[1:])])
    plain.load_state_dict({k[len("layer_list."):]: v for k, v in stack.state_dict().items()})
    stack.load_state_dict({"layer_list." + k: v for k, v in plain.state_dict().items()})
    assert all(isinstance(m, torch.nn.LSTM) and m.batch_first for m in stack.layer_list)
    # bias=False drops exactly the bias keys
    assert sorted(project_model(method, bias=False).state_dict()) == [k for k in KEYS[method] if "bias" not in k]
    assert sorted(R.mirror(method, bias=False).state_dict()) == [k for k in KEYS[method] if "bias" not in k]


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_lstmcell.hip" for s in build.SRCS)


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID = -1
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def fwd(B=4, H=8, gi=p, ldgi=32, gh=p, ldgh=32, bias=p, cp=p, ldcp=8, h=p, ldh=8, c=p, ldc=8, gates=p, ldg=32):
        return lib.ctgcn_lstm_cell_fwd_f32(B, H, gi, ldgi, gh, ldgh, bias, cp, ldcp, h, ldh, c, ldc, gates, ldg, None)

    assert fwd(B=-1) == INVALID and fwd(B=2 ** 31) == INVALID and fwd(H=0) == INVALID and fwd(H=2 ** 29) == INVALID
    for name in ("ldgi", "ldgh", "ldg"):
        assert fwd(**{name: 31}) == INVALID, name
    for name in ("ldcp", "ldh", "ldc"):
        assert fwd(**{name: 7}) == INVALID, name
    for name in ("gi", "h", "c"):
        assert fwd(**{name: None}) == INVALID, name
    assert b"lstm_cell_fwd" in lib.ctgcn_last_error()
    assert fwd(B=0) == 0 and fwd(B=0, gi=None, h=None, c=None) == 0
    assert fwd(B=0, ldgi=31) == INVALID                               # sizes are checked before the empty call returns

    def bwd(B=4, H=8, gates=p, ldg=32, c=p, ldc=8, cp=p, ldcp=8, do=p, lddo=8, dr=p, lddr=8, dn=p, lddn=8, dg=p, lddg=32, dp=p, lddp=8):
        return lib.ctgcn_lstm_cell_bwd_f32(B, H, gates, ldg, c, ldc, cp, ldcp, do, lddo, dr, lddr, dn, lddn, dg, lddg, dp, lddp, None)

    assert bwd(B=-1) == INVALID and bwd(B=2 ** 31) == INVALID and bwd(H=0) == INVALID and bwd(H=2 ** 29) == INVALID
    for name in ("ldg", "lddg"):
        assert bwd(**{name: 31}) == INVALID, name
    for name in ("ldc", "ldcp", "lddo", "lddr", "lddn", "lddp"):
        assert bwd(**{name: 7}) == INVALID, name
    for name in ("gates", "c", "dg"):
        assert bwd(**{name: None}) == INVALID, name
    assert b"lstm_cell_bwd" in lib.ctgcn_last_error()
    assert bwd(B=0) == 0 and bwd(B=0, gates=None, c=None, dg=None) == 0


def tiny_window():
    a = sp.csr_matrix(np.array([[0, 1, 0, 2, 0], [1, 0, 3, 0, 0], [0, 3, 0, 0, 0], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.float64))
    return [a, a.T.tocsr(), a, a]


def test_interface_and_refusals(tmp_path):
    import ctgcn_amd
    from ctgcn_amd import _lib, baseline, ops
    from ctgcn_amd.baseline import dynae, dynaernn, dynrnn
    for name in ("DynRNN", "DynAERNN", "MLLSTM", "MTMLP"):
        assert name in ctgcn_amd.__all__ and getattr(ctgcn_amd, name) is getattr(baseline, name)
    assert dynaernn.MLP is dynae.MLP and dynaernn.MLLSTM is dynrnn.MLLSTM
    rnn = ctgcn_amd.DynRNN(5, 2, look_back=3, n_units=[3])
    aernn = ctgcn_amd.DynAERNN(5, 2, look_back=3, ae_units=[4], rnn_units=[3])
    assert isinstance(rnn.decoder, ctgcn_amd.MLLSTM) and rnn.decoder.layer_list[-1].hidden_size == 5      # the last decoder layer is N wide
    assert isinstance(aernn.ae_encoder, ctgcn_amd.MTMLP) and len(aernn.ae_encoder.layer_list) == 3 and isinstance(aernn.decoder, dynae.MLP)
    assert tuple(rnn.encoder.first_transposed().shape) == (5, 12) and [tuple(t.shape) for t in aernn.first_transposed()] == [(5, 4)] * 3
    # CPU tensors
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        rnn(torch.zeros(2, 3, 5))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        aernn(torch.zeros(2, 3, 5))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.lstm_layer(torch.zeros(2, 3, 5), torch.zeros(8, 5), torch.zeros(8, 2))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.lstm_layer(None, None, torch.zeros(8, 2), gi=torch.zeros(2, 3, 8))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ctgcn_amd.BatchPredictor(list("abcde"), 4).predict(rnn, tiny_window()[:3])
    # a window of another length than look_back
    with pytest.raises(ValueError, match="look_back 3"):
        aernn(torch.zeros(2, 4, 5))
    with pytest.raises(ValueError, match="look_back 3"):
        aernn.ae_encoder(torch.zeros(2, 2, 5))
    # the trainer: has_cuda=False, a foreign module
    (tmp_path / "origin").mkdir()
    nodes = list("abcde")
    args = (str(tmp_path), "origin", "emb", nodes)
    gen, pred = ctgcn_amd.BatchGenerator(nodes, 4, 3, 5.0), ctgcn_amd.BatchPredictor(nodes, 4)
    for model in (rnn, aernn):
        with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
            ctgcn_amd.DynamicEmbedding(*args, model, ctgcn_amd.DynGraph2VecLoss(5.0, 0., 0.), gen, pred, has_cuda=False)

    class Foreign(torch.nn.Module):
        method_name = "DynRNN"

    with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline.DynGEM"):
        ctgcn_amd.DynamicEmbedding(*args, Foreign(), ctgcn_amd.DynGraph2VecLoss(5.0, 0., 0.), gen, pred, has_cuda=True)
    # the generator's batches have look_back 3 columns and two training positions per node
    batch = next(ctgcn_amd.BatchGenerator(nodes, 4, 3, 5.0, shuffle=False).generate(tiny_window()))
    assert batch.host_idx.tolist() == [[0, 5, 10], [1, 6, 11], [2, 7, 12], [3, 8, 13]] and batch.host_tgt.tolist() == [15, 16, 17, 18]
