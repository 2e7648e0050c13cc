"""CTGCN-C on one-hot features with the first Linear stored by input row (ops.to_gather_layout) and its rows gathered by the first
CoreDiffusion aggregation, bias added in registers (CTGCN.gather_operand), against CTGCN_LINEAR_GATHER=0 — the materialised
Linear(I) = W^T + b of ctgcn_transpose_bias_f32: outputs and every parameter gradient torch.equal, on the plain, the small-window, the
sharded and the hipGraph paths."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

N, T = 300, 3


def _dev():
    return torch.device("cuda", 0)


_WINDOW = {}


def _window():
    """adjacency lists and one-hot features of the window, built once"""
    if not _WINDOW:
        from ctgcn_amd.helper import core_adj_from_scipy
        from ctgcn_amd.synth import dynamic_graph
        dev = _dev()
        graphs = dynamic_graph(N, 8, T, seed=9)
        eye = torch.arange(N, device=dev).repeat(2, 1)
        _WINDOW.update(graphs=graphs, adj=[core_adj_from_scipy(g, 4, dev)[0] for g in graphs],
                       xs=[torch.sparse_coo_tensor(eye, torch.ones(N, device=dev), (N, N)) for _ in range(T)])
    return _WINDOW["graphs"], _WINDOW["adj"], _WINDOW["xs"]


def _pair(hid, bias=True):
    """two copies of one seeded CTGCN-C: the gather forward re-lays its weights in place, so each switch position gets its own"""
    import ctgcn_amd
    torch.manual_seed(hid)
    model = ctgcn_amd.CTGCN(N, hid, 128, 1, 2, T, bias=bias).to(_dev())
    return model, copy.deepcopy(model)


def _gathered(model):
    from ctgcn_amd import ops
    return [ops.in_gather_layout(m.linear.weight) for m in model.mlp_list]


# (CTGCN_GROUP, CTGCN_GROUP_HEAD, does the forward gather?) — the grouped launches of small windows read a materialised Linear(I)
PATHS = {"per-snapshot": ("0", None, True), "grouped-tail": ("1", "0", None), "grouped": ("1", None, False)}


@pytest.mark.parametrize("path", sorted(PATHS))
@pytest.mark.parametrize("hid", [128, 500])
def test_inference_forward_is_bit_identical_with_the_switch_off_and_on(hid, path, monkeypatch):
    group, head, gathers = PATHS[path]
    if gathers is None:
        gathers = hid != 128         # a 500-wide first layer in front of the grouped 128-wide ones gathers; at 128 every layer is grouped
    monkeypatch.setenv("CTGCN_GROUP", group)
    if head is not None:
        monkeypatch.setenv("CTGCN_GROUP_HEAD", head)
    _, adj, xs = _window()
    off, on = _pair(hid)
    off.eval(), on.eval()
    want_w = [m.linear.weight.detach().clone() for m in on.mlp_list]
    with torch.no_grad():
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        want = off(xs, adj)
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "1")
        got = on(xs, adj)
        again = on(xs, adj)
    assert torch.isfinite(want).all() and torch.equal(got, want) and torch.equal(again, want)
    assert _gathered(off) == [False] * T and _gathered(on) == [gathers] * T
    for m, w in zip(on.mlp_list, want_w):                  # same parameter, same shape, same values
        assert tuple(m.linear.weight.shape) == (hid, N) and torch.equal(m.linear.weight, w)
    # a re-laid weight on the path that still wants the matrix: the same bits from the row-major add
    with torch.no_grad():
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        assert torch.equal(on(xs, adj), want)


def test_a_linear_without_bias_is_gathered_as_it_is(monkeypatch):
    monkeypatch.setenv("CTGCN_GROUP", "0")
    _, adj, xs = _window()
    off, on = _pair(128, bias=False)
    off.eval(), on.eval()
    with torch.no_grad():
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        want = off(xs, adj)
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "1")
        got = on(xs, adj)
    assert torch.equal(got, want) and _gathered(on) == [True] * T


@pytest.mark.parametrize("hid", [128, 500])
def test_one_training_step_gives_the_same_gradients_and_the_same_update(hid, monkeypatch):
    _, adj, xs = _window()
    off, on = _pair(hid)
    off.train(), on.train()
    outs, opts = [], []
    for model, flag in ((off, "0"), (on, "1")):
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", flag)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        out = model(xs, adj)
        out.square().mean().backward()
        outs.append(out.detach())
        opts.append(opt)
    assert torch.equal(outs[0], outs[1])
    assert _gathered(off) == [False] * T and _gathered(on) == [True] * T
    named_off, named_on = dict(off.named_parameters()), dict(on.named_parameters())
    compared = 0
    for name, p in named_off.items():
        q = named_on[name]
        assert (p.grad is None) == (q.grad is None), name
        if p.grad is not None:
            assert p.grad.shape == q.grad.shape and torch.equal(p.grad, q.grad), name          # by value, whatever the strides
            compared += 1
    assert compared >= 10 * T + 6
    for t in range(T):
        g = named_on["mlp_list.%d.linear.weight" % t].grad
        assert float(g.abs().max()) > 0 and float(named_on["mlp_list.%d.linear.bias" % t].grad.abs().max()) > 0
    for opt in opts:
        opt.step()
    for name, p in named_off.items():
        assert torch.equal(p.detach(), named_on[name].detach()), name
    assert _gathered(on) == [True] * T                      # the optimizer's update keeps the layout


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("hid", [128, 500])
def test_sharded_forward_equals_the_plain_one(hid, world, monkeypatch):
    from _loopback import LoopbackDist
    from ctgcn_amd import snapshot_parallel as spp
    graphs, adj, xs = _window()
    off, on = _pair(hid)
    off.eval(), on.eval()
    with torch.no_grad():
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        want = off(xs, adj).clone()
    monkeypatch.setenv("CTGCN_LINEAR_GATHER", "1")
    loop = LoopbackDist(world)
    monkeypatch.setattr(spp, "dist", loop)
    models = [copy.deepcopy(on) for _ in range(world)]

    def body(rank):
        m = models[rank]
        plan = spp.shard_ctgcn(m, N, costs=[g.nnz for g in graphs], group=loop.group.WORLD, gather_output=True)
        mine = plan.assignment[rank]
        with torch.no_grad():
            got = m([xs[t] if t in mine else None for t in range(T)], [adj[t] if t in mine else None for t in range(T)])
        return bool(torch.equal(got, want)), [g for t, g in enumerate(_gathered(m)) if t in mine]
    for same, gathered in loop.run(body):
        assert same and all(gathered)


@pytest.mark.parametrize("hid", [128, 500])
def test_hipgraph_replay_equals_the_plain_forward(hid, monkeypatch):
    from ctgcn_amd.graph_capture import GraphedInference
    monkeypatch.setenv("CTGCN_GROUP", "0")                   # the per-snapshot launches: the path that gathers
    _, adj, xs = _window()
    off, on = _pair(hid)
    off.eval(), on.eval()
    with torch.no_grad():
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        want = off(xs, adj).clone()
    monkeypatch.setenv("CTGCN_LINEAR_GATHER", "1")
    runner = GraphedInference(on, xs, adj)                    # the warm-up forwards re-lay the weights, the capture gathers
    assert _gathered(on) == [True] * T
    assert torch.equal(runner(), want)
    with torch.no_grad():                                     # a replay sees an in-place weight update
        for m in list(on.mlp_list) + list(off.mlp_list):
            m.linear.bias.add_(0.25)
        monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
        want2 = off(xs, adj).clone()
    assert not torch.equal(want2, want) and torch.equal(runner(), want2)


def test_other_consumers_of_a_relaid_weight_keep_their_bits():
    """ops.linear_of_identity (forward and gradients) and a dense-feature call on the same Linear, before and after the re-layout"""
    from ctgcn_amd import MLP, ops
    torch.manual_seed(3)
    mlp = MLP(N, 64, 96, 1, activate_type='L').to(_dev())
    lin = mlp.linear
    dense = torch.randn(40, N, device=_dev())
    want = ops.linear_of_identity(lin.weight, lin.bias)
    want.square().sum().backward()
    gw, gb = lin.weight.grad.clone(), lin.bias.grad.clone()
    with torch.no_grad():
        want_dense = mlp(dense)
    lin.weight.grad = lin.bias.grad = None
    ops.to_gather_layout(lin.weight)
    assert ops.in_gather_layout(lin.weight)
    got = ops.linear_of_identity(lin.weight, lin.bias)
    got.square().sum().backward()
    assert torch.equal(got, want) and torch.equal(lin.weight.grad, gw) and torch.equal(lin.bias.grad, gb)
    with torch.no_grad():
        bare = ops.linear_of_identity(lin.weight, None)
        assert torch.equal(bare, lin.weight.t()) and bare.data_ptr() != lin.weight.data_ptr()      # a copy, never the parameter's memory
        assert torch.equal(mlp(dense), want_dense)
