"""The GIN / GraphSAGE modules and their stock-torch mirrors against the reference's recorded results (tests/golden/gin_sage_uci.npz),
on the host: the mirrors in float64 reproduce the reference's float64 outputs, gradients and losses to 1e-12, and the modules have
the reference's state_dict keys and shapes, so checkpoints move both ways.  No kernel runs here.

Gradients that are zero in exact arithmetic (a Linear bias in front of a BatchNorm, which removes it again) are rounding noise of
1e-15 to 1e-11 in both programs and cannot agree relative to themselves: a bias gradient is held to 1e-12 of the larger of its own
magnitude and its Linear's weight gradient's, which the same row gradients produce.

The running buffers are held to 1e-12 as well, with one reasoned exception.  Adam moves such a bias by lr g / (|g| + 1e-8), at most
lr |g| / 1e-8 for these |g| far below 1e-8, and the shift goes straight into the running mean of the BatchNorm behind it (and nowhere
else: the BatchNorm removes it from its output).  With sum and average pooling the mirror's noise is the reference's bit for bit and
nothing differs.  With max pooling the mirror's backward adds in another order than the reference's loop over the nodes, so the two
noises differ; at worst each program moves the bias its own way on both steps that precede a later forward, so those running means
are held to 4 lr max|g| / 1e-8, |g| the larger of the two programs' first-step gradients of the bias in front (1e-6 to 1e-8 here)."""
import numpy as np
import pytest
import torch

import _gin_sage_ref as G
from conftest import seeded_parameters

_runs = {}


def mirror_run(case):
    if case not in _runs:
        g = G.fixture()
        model = G.build(case, G.GinMirror, G.SageMirror)
        seeded_parameters(model, int(g["seed"]))
        model = model.double().train()
        x, adj = G.features(case, torch.float64), G.adjacency(torch.float64)
        losses, (outs, grads) = G.adam_losses(model, lambda: model(x, adj), G.surrogate_weights(torch.float64))
        _runs[case] = (losses, outs, grads, G.buffers(model))
    return _runs[case]


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def error(g, key, got):
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    return float(np.abs((got if pick is None else got[pick]) - ref).max(initial=0.0)), top


@pytest.mark.parametrize("case", G.CASES)
def test_the_float64_mirror_reproduces_the_reference(case):
    g = G.fixture()
    losses, outs, grads, bufs = mirror_run(case)
    for t in range(G.T):
        err, top = error(g, "%s_out_t%d" % (case, t), outs[t])
        assert err <= 1e-12 * top, ("out", t, err, top)
    assert np.abs(np.asarray(losses) - g[case + "_losses"]).max() <= 1e-12 * np.abs(g[case + "_losses"]).max()
    keys = [str(k) for k in g[case + "_keys"]]
    assert sorted(grads) == keys
    for k in keys:
        err, top = error(g, "%s_grad_%s" % (case, k), grads[k])
        if k.endswith(".bias") and k[:-4] + "weight" in keys:
            top = max(top, float(g["%s_grad_%sweight__maxabs" % (case, k[:-4])]))
        assert err <= 1e-12 * top, (k, err, top)
    names = [str(k) for k in g[case + "_buffer_keys"]]
    assert sorted(bufs) == names
    kwargs = G.CASES[case][2]
    for k in names:
        ref = g["%s_buffer_%s" % (case, k)]
        top = float(np.abs(ref).max())
        tol = 1e-12 * top
        if k.endswith("running_mean") and kwargs.get("neighbor_pooling_type") == "max":
            noise = max(float(grads[bias_in_front(k, keys)].abs().max()), float(g["%s_grad_%s__maxabs" % (case, bias_in_front(k, keys))]))
            assert noise < 1e-10, (k, noise)                        # far below Adam's 1e-8: the bound's premise
            tol += 4 * G.LR * noise / 1e-8
        assert np.abs(bufs[k].double().numpy() - ref).max() <= tol, (k, tol)
        if k.endswith("num_batches_tracked"):
            assert int(bufs[k]) == int(ref) == G.T * G.ADAM_STEPS


def bias_in_front(buffer_key, keys):
    """the Linear bias whose output the BatchNorm of `buffer_key` normalises: mlps.l.linears.k for mlps.l.batch_norms.k, the MLP's last
    Linear for batch_norms.l"""
    part = buffer_key.split(".")
    if part[0] == "mlps":
        return "mlps.%s.linears.%s.bias" % (part[1], part[3])
    last = [k for k in keys if k.startswith("mlps.%s.linear" % part[1]) and k.endswith(".bias")]
    return sorted(last)[-1]


@pytest.mark.parametrize("case", G.CASES)
def test_state_dict_keys_and_shapes_are_the_reference_s(case):
    import ctgcn_amd
    g = G.fixture()
    want = {str(k): tuple(int(s) for s in str(shape).split(",") if s) for k, shape in zip(g[case + "_state_keys"], g[case + "_state_shapes"])}
    for cls_pair in ((ctgcn_amd.GIN, ctgcn_amd.SAGE), (G.GinMirror, G.SageMirror)):
        model = G.build(case, *cls_pair)
        assert {k: tuple(v.shape) for k, v in model.state_dict().items()} == want
    model = G.build(case, ctgcn_amd.GIN, ctgcn_amd.SAGE)
    assert sorted(k for k, _ in model.named_parameters()) == [str(k) for k in g[case + "_keys"]]
    assert model.method_name == G.CASES[case][0]
    # a state dict of the golden's keys and shapes loads strictly
    state = {k: torch.full(shape, 0.25, dtype=torch.int64 if k.endswith("num_batches_tracked") else torch.float32) for k, shape in want.items()}
    model.load_state_dict(state, strict=True)
    assert all(float(v.double().mean()) == (0.0 if k.endswith("num_batches_tracked") else 0.25) for k, v in model.state_dict().items())


def test_constructor_arguments_and_defaults():
    import ctgcn_amd
    from ctgcn_amd.baseline.gin import MLP
    from ctgcn_amd.baseline.sage import Aggregator, SAGE_Layer
    gin = ctgcn_amd.GIN(30, 20, 16, 2, 2, False)
    assert (gin.neighbor_pooling_type, gin.dropout, gin.bias, gin.learn_eps) == ("sum", 0.5, True, False)
    assert tuple(gin.eps.shape) == (2,) and float(gin.eps.detach().abs().sum()) == 0.0
    assert ctgcn_amd.GIN(30, 20, 16, 2, 2, True, "sum").learn_eps            # constructs; the reference's forward raises UnboundLocalError
    assert sorted(MLP(4, 5, 6, 1).state_dict()) == ["linear.bias", "linear.weight"]
    assert sorted(MLP(4, 5, 6, 3, bias=False).state_dict())[-2:] == ["linears.1.weight", "linears.2.weight"]
    with pytest.raises(ValueError):
        MLP(4, 5, 6, 0)
    with pytest.raises(AssertionError):
        ctgcn_amd.GIN(30, 20, 16, 2, 2, False, "min")
    sage = ctgcn_amd.SAGE(30, 20, 16, None)
    assert (sage.pooling_type, sage.dropout, sage.bias, sage.num_sample, sage.sage1.gcn) == ("sum", 0.5, True, None, False)
    assert tuple(sage.sage1.linear.weight.shape) == (20, 40) and tuple(ctgcn_amd.SAGE(30, 20, 16, None, gcn=True).sage2.linear.weight.shape) == (16, 20)
    assert Aggregator().num_sample is None and Aggregator().pooling_type == "sum"
    for make in (lambda: ctgcn_amd.SAGE(30, 20, 16, num_sample=2), lambda: ctgcn_amd.SAGE(30, 20, 16), lambda: SAGE_Layer(4, 4),
                 lambda: Aggregator(num_sample=2)):
        with pytest.raises(NotImplementedError, match="random.sample"):
            make()


def test_the_trainers_accept_both_models():
    from ctgcn_amd import embedding
    assert "GIN" in embedding._SUPPORTED and "SAGE" in embedding._SUPPORTED


def test_the_mirror_s_maximum_sends_a_tie_s_gradient_to_the_first_entry():
    h = torch.tensor([[1.0, 5.0], [1.0, 2.0], [0.5, 5.0], [-3.0, -4.0]], dtype=torch.float64, requires_grad=True)
    rows, cols = torch.tensor([0, 0, 0, 2, 3, 3]), torch.tensor([0, 1, 2, 3, 0, 2])
    out = G.pool_max(h, rows, cols)
    assert out.tolist() == [[1.0, 5.0], [0.0, 0.0], [-3.0, -4.0], [1.0, 5.0]]
    (out * torch.tensor([[1.0, 10.0], [0.0, 0.0], [100.0, 1000.0], [7.0, 70.0]], dtype=torch.float64)).sum().backward()
    assert h.grad.tolist() == [[8.0, 80.0], [0.0, 0.0], [0.0, 0.0], [100.0, 1000.0]]
