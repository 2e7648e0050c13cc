"""ops.TgGraph, ops.tg_conv and ops.tgat_conv (ctgcn_tg.hip, the PyG-form passes of ctgcn_gat.hip) on the GPU.

TgGraph against a numpy host model: patterns exactly, looped values within one float32 ulp of the fp64 formula, mean values exactly.
The two ops against the float64 stock-torch mirror (tests/_tg_ref.py): outputs and every gradient.  Tolerance per tensor (the rule of
tests/test_gpu_gcrn.py and test_gpu_gat.py): 4 x the mirror's own float32-vs-float64 error, measured here on the CPU on the same
inputs, over the tensor's largest magnitude, with a floor of 2e-6 max|ref| for outputs and 1e-5 max|ref| for gradients."""
import numpy as np
import pytest
import torch

import _tg_ref as G

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HUB_N, HUB = 70, 3
_graphs = {}


def edge_index(name):
    """numpy int64 [2, E]"""
    if name in _graphs:
        return _graphs[name]
    if name == "one":
        ei, n = np.zeros((2, 0), dtype=np.int64), 1
    elif name == "small":
        ei, n = G.SMALL_EDGES.copy(), G.SMALL_N
    elif name == "hub":
        # node 3 with 300 incoming pairs from 69 possible sources: distinct, repeated and its own loop; node 69 isolated (an empty row
        # as given, a row of its loop alone once looped); node 68 with one incoming pair; the rest a sparse ring
        rng = np.random.default_rng(11)
        ring = np.array([v for v in range(68) if (v + 1) % 68 != HUB])
        src = np.concatenate((rng.integers(0, 69, 299), [HUB], ring, [5]))
        tgt = np.concatenate((np.full(300, HUB), (ring + 1) % 68, [68]))
        perm = rng.permutation(src.size)
        ei, n = np.vstack((src[perm], tgt[perm])).astype(np.int64), HUB_N
    else:
        ei, n = G.uci_edges(0).numpy(), G.N
    _graphs[name] = (ei, n)
    return _graphs[name]


def tg_graph(name, long_threshold=None):
    from ctgcn_amd import ops
    ei, n = edge_index(name)
    return ops.TgGraph(torch.from_numpy(ei).to(DEV), n, long_threshold=long_threshold)


@pytest.mark.parametrize("name", ["one", "small", "hub", "uci"])
def test_tg_graph_matches_the_host_model(name):
    ei, n = edge_index(name)
    g, g2 = tg_graph(name), tg_graph(name)
    host = G.host_graph(ei, n)
    row_ptr, col, val = host["looped"]
    assert np.array_equal(g.looped.row_ptr.cpu().numpy(), row_ptr) and np.array_equal(g.looped.col.cpu().numpy(), col)
    got, want = g.looped.val.cpu().numpy(), val.astype(np.float32)
    assert got.dtype == np.float32 and (np.abs(got.astype(np.float64) - want) <= np.spacing(want)).all()
    raw_ptr, rcol, mean = host["raw"]
    for adj in (g.mean, g.sum):
        assert np.array_equal(adj.row_ptr.cpu().numpy(), raw_ptr) and np.array_equal(adj.col.cpu().numpy(), rcol)
    assert g.mean.row_ptr is g.sum.row_ptr and g.mean.col is g.sum.col
    assert np.array_equal(g.mean.val.cpu().numpy(), mean.astype(np.float32))
    assert np.array_equal(g.sum.val.cpu().numpy(), np.ones(ei.shape[1], dtype=np.float32))
    for a, b in ((g.looped, g2.looped), (g.mean, g2.mean)):                      # two builds: bit-identical
        assert torch.equal(a.row_ptr, b.row_ptr) and torch.equal(a.col, b.col) and torch.equal(a.val, b.val)
    if name == "one":
        assert g.looped.row_ptr.tolist() == [0, 1] and g.looped.col.tolist() == [0] and g.looped.val.tolist() == [1.0] and g.mean.nnz == 0
    if name == "hub":
        assert int(np.diff(raw_ptr)[HUB]) == 300 and int(np.diff(raw_ptr)[69]) == 0 and int(np.diff(row_ptr)[69]) == 1
        assert len(set(rcol[raw_ptr[HUB]:raw_ptr[HUB + 1]])) < 300


def test_tg_graph_refuses_bad_input():
    from ctgcn_amd import ops
    ei = torch.tensor([[0, 1, 2], [1, 2, 6]], device=DEV)
    for bad in (ei, ei.flip(0), torch.tensor([[0, -1], [1, 1]], device=DEV)):
        with pytest.raises(ValueError, match="outside"):
            ops.TgGraph(bad, 6).looped
    ops.TgGraph(ei, 7).mean
    with pytest.raises(ValueError):
        ops.TgGraph(ei, 2 ** 31)
    with pytest.raises(ValueError):
        ops.TgGraph(ei.to(torch.int32), 7)
    with pytest.raises(ValueError):
        ops.TgGraph(ei[0], 7)


# ------------------------------------------------------------------------------------------------ comparison with the mirror
def entries(adj):
    """(src, tgt, val) of a GcnAdj on the CPU: val as the kernels read it (float32), widened"""
    rows = torch.repeat_interleave(torch.arange(adj.n), (adj.row_ptr[1:] - adj.row_ptr[:-1]).cpu().long())
    return adj.col.cpu().long(), rows, adj.val.cpu().double()


def compare(name, got, run_mirror, floors):
    """run_mirror(dtype) -> list of tensors; got: the same list from the GPU.  Prints the share of the tolerance every tensor uses."""
    want, yard = run_mirror(torch.float64), run_mirror(torch.float32)
    over = {}
    for k, (g, w, y, floor) in enumerate(zip(got, want, yard, floors)):
        top = float(w.abs().max())
        if top == 0.0:
            assert float(g.abs().max()) == 0.0, (name, k)
            continue
        own = float((y.double() - w).abs().max()) / top
        err = float((g.cpu().double() - w).abs().max()) / top
        used = err / max(4 * own, floor)
        print("  [tol] %-40s tensor %d |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (name, k, err, used, own, floor))
        if not used <= 1.0:
            over[k] = round(used, 3)
    assert not over, "%s: share of the tolerance used %s" % (name, over)


def inputs(n, d, layout, seed):
    """(leaf, S): S [n, d] a view of the float32 leaf: the leaf itself, a strided column slice, or a base 4 bytes off 16-byte alignment"""
    rng = np.random.default_rng(seed)
    if layout == "slice":
        leaf = torch.from_numpy(rng.uniform(-1, 1, (n, d + 3)).astype(np.float32)).to(DEV).requires_grad_()
        return leaf, leaf[:, 1:1 + d]
    if layout == "misaligned":
        leaf = torch.from_numpy(rng.uniform(-1, 1, n * d + 1).astype(np.float32)).to(DEV).requires_grad_()
        return leaf, leaf[1:].view(n, d)
    leaf = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(DEV).requires_grad_()
    return leaf, leaf


def view_of(leaf64, d, layout, n):
    return leaf64[:, 1:1 + d] if layout == "slice" else leaf64[1:].view(n, d) if layout == "misaligned" else leaf64


TG_CASES = [
    # graph, adjacency, d, T, epi, p, bias, long_threshold, layout
    ("small", "mean", 4, "none", 0, 0.0, False, None, "plain"),
    ("small", "sum", 6, "same", 1, 0.0, True, None, "plain"),
    ("small", "looped", 4, "other", 1, 0.5, True, None, "plain"),
    ("hub", "mean", 132, "pair", 1, 0.5, True, 16, "plain"),
    ("hub", "mean", 4, "pair", 0, 0.0, True, None, "plain"),
    ("hub", "sum", 6, "other", 1, 0.5, False, 16, "slice"),
    ("hub", "sum", 4, "same", 1, 0.0, True, 16, "misaligned"),
    ("hub", "mean", 132, "none", 1, 0.5, True, None, "plain"),
    ("hub", "looped", 6, "pair", 1, 0.0, True, 16, "plain"),
]


@pytest.mark.parametrize("case", TG_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_tg_conv_matches_the_mirror(case):
    from ctgcn_amd import ops
    graph, which, d, tmode, epi, p, with_bias, thr, layout = case
    adj = getattr(tg_graph(graph, thr), which)
    n = adj.n
    if thr and graph == "hub" and which != "looped":
        assert adj.long_rows is not None and adj.pieces == 5                     # 300 entries in pieces of 64
    key, scale = 0x1234567 + d, 1.0 if tmode in ("none", "pair") else 1.75
    if tmode == "pair":
        leaf, Z = inputs(n, 2 * d, "plain", d)
        S, T = Z[:, :d], Z[:, d:]
        leaves = [leaf]
    else:
        leaf, S = inputs(n, d, layout, d)
        leaves = [leaf]
        T = None
        if tmode == "same":
            T = S
        elif tmode == "other":
            tleaf, T = inputs(n, d, "plain", d + 100)
            leaves.append(tleaf)
    bias = torch.from_numpy(np.random.default_rng(5).uniform(-0.5, 0.5, d).astype(np.float32)).to(DEV).requires_grad_() if with_bias else None
    if bias is not None:
        leaves.append(bias)
    C = torch.from_numpy(np.random.default_rng(6).uniform(-1, 1, (n, d)).astype(np.float32)).to(DEV)

    def gpu():
        for t in leaves:
            t.grad = None
        out = ops.tg_conv(S, adj, T, scale, bias, epi, p, key)
        (out * C).sum().backward()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    got, again = gpu(), gpu()
    assert all(torch.equal(a, b) for a, b in zip(got, again))                    # repeated forward and backward: bit-identical
    keep = ops.dropout_keep_mask(key, n, d, p, DEV).cpu() if (epi and p > 0) else None
    if keep is not None:
        assert 0.3 < float(keep.double().mean()) < 0.7
    src, tgt, val = entries(adj)

    def mirror(dtype):
        ls = [t.detach().cpu().to(dtype).requires_grad_() for t in leaves]
        if tmode == "pair":
            s, tm = ls[0][:, :d], ls[0][:, d:]
        else:
            s = view_of(ls[0], d, layout, n)
            tm = None if tmode == "none" else s if tmode == "same" else ls[1]
        y = G.tg_conv(s, tm, scale, ls[-1] if with_bias else None, src, tgt, val.to(dtype))
        if epi:
            y = G.relu_dropout(y, keep, p)
        (y * C.cpu().to(dtype)).sum().backward()
        return [y.detach()] + [t.grad for t in ls]

    compare("tg_conv " + "-".join(str(v) for v in case), got, mirror, [2e-6] + [1e-5] * len(leaves))


TGAT_CASES = [
    # graph, adjacency, d, heads, epi, p, bias, long_threshold, layout
    ("small", "looped", 4, 1, 0, 0.0, False, None, "plain"),
    ("small", "looped", 6, 1, 1, 0.0, True, None, "plain"),
    ("small", "mean", 4, 1, 1, 0.0, True, None, "plain"),             # node 5's row is empty: epi(bias), no gradient to S
    ("hub", "looped", 132, 1, 1, 0.5, True, 16, "plain"),
    ("hub", "looped", 8, 2, 1, 0.0, True, None, "plain"),
    ("hub", "mean", 8, 2, 0, 0.0, False, 16, "plain"),
    ("hub", "looped", 6, 1, 1, 0.5, True, 16, "slice"),
    ("hub", "looped", 4, 1, 0, 0.0, True, None, "misaligned"),
]


@pytest.mark.parametrize("case", TGAT_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_tgat_conv_matches_the_mirror(case):
    from ctgcn_amd import ops
    graph, which, d, heads, epi, p, with_bias, thr, layout = case
    adj = getattr(tg_graph(graph, thr), which)
    n, F_ = adj.n, d // heads
    key = 0x7654321 + d
    leaf, S = inputs(n, d, layout, 20 + d)
    rng = np.random.default_rng(21)
    a_tgt, a_src = (torch.from_numpy(rng.uniform(-1, 1, (heads, F_)).astype(np.float32)).to(DEV).requires_grad_() for _ in range(2))
    leaves = [leaf, a_tgt, a_src]
    bias = torch.from_numpy(rng.uniform(-0.5, 0.5, d).astype(np.float32)).to(DEV).requires_grad_() if with_bias else None
    if bias is not None:
        leaves.append(bias)
    C = torch.from_numpy(rng.uniform(-1, 1, (n, d)).astype(np.float32)).to(DEV)

    def gpu():
        for t in leaves:
            t.grad = None
        out = ops.tgat_conv(S, a_tgt, a_src, adj, heads, 0.2, bias, epi, p, key)
        (out * C).sum().backward()
        return [out.detach().clone()] + [t.grad.detach().clone() for t in leaves]

    got, again = gpu(), gpu()
    assert all(torch.equal(a, b) for a, b in zip(got, again))
    keep = ops.dropout_keep_mask(key, n, d, p, DEV).cpu() if (epi and p > 0) else None
    src, tgt, _ = entries(adj)

    def mirror(dtype):
        ls = [t.detach().cpu().to(dtype).requires_grad_() for t in leaves]
        y = G.attention(view_of(ls[0], d, layout, n), ls[2], ls[1], src, tgt, heads, 0.2)
        if with_bias:
            y = y + ls[3]
        if epi:
            y = G.relu_dropout(y, keep, p)
        (y * C.cpu().to(dtype)).sum().backward()
        return [y.detach()] + [t.grad for t in ls]

    compare("tgat_conv " + "-".join(str(v) for v in case), got, mirror, [2e-6] + [1e-5] * len(leaves))
    if which == "mean" and graph == "small" and with_bias:
        want = torch.relu(bias.detach()) if epi else bias.detach()
        assert torch.equal(got[0][5], want) and float(got[1].view(n, -1)[5].abs().max()) == 0.0


def test_tgat_conv_logits_of_200_stay_finite():
    from ctgcn_amd import ops
    adj = tg_graph("hub").looped
    n = adj.n
    rng = np.random.default_rng(31)
    S = torch.from_numpy(rng.uniform(-1, 1, (n, 4)).astype(np.float32)).to(DEV)
    S[:, 0] = torch.from_numpy(rng.choice([-100.0, 100.0], n).astype(np.float32)).to(DEV)       # z = u + v in {-200, 0, 200}
    S.requires_grad_()
    a = torch.tensor([[1.0, 0.0, 0.0, 0.0]], device=DEV, requires_grad=True)
    a2 = a.detach().clone().requires_grad_()
    out = ops.tgat_conv(S, a, a2, adj, 1, 1.0)                                                   # slope 1: l = z itself
    out.sum().backward()
    for t in (out, S.grad, a.grad, a2.grad):
        assert bool(torch.isfinite(t).all())
    src, tgt, _ = entries(adj)
    want = G.attention(S.detach().cpu().double(), a2.detach().cpu().double(), a.detach().cpu().double(), src, tgt, 1, 1.0)
    assert float((out.detach().cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())


def test_only_the_gradients_asked_for_are_computed():
    from ctgcn_amd import ops
    g = tg_graph("hub")
    n, d = g.looped.n, 8                                                         # the build: not part of what is counted below
    seen = []
    S = torch.rand(n, d, device=DEV)
    bias = torch.zeros(d, device=DEV, requires_grad=True)
    a = torch.rand(1, d, device=DEV)
    ops.set_launch_timer(lambda name, *_: seen.append(name))
    try:
        ops.tg_conv(S, g.mean, S, 1.0, bias, ops.TG_EPI_RELU).sum().backward()
        assert seen == ["tg_conv_fwd", "tg_conv_prep"] and bias.grad is not None
        del seen[:]
        ops.tgat_conv(S, a, a.clone(), g.looped, 1, 0.2, bias, ops.TG_EPI_RELU).sum().backward()
        assert seen == ["tgat_fwd", "tg_conv_prep"]
        del seen[:]
        a_tgt = a.clone().requires_grad_()
        ops.tgat_conv(S, a_tgt, a.clone(), g.looped, 1, 0.2, None, ops.TG_EPI_NONE).sum().backward()
        assert seen == ["tgat_fwd", "gat_bwd_prep", "tgat_bwd_row", "gat_da"] and a_tgt.grad is not None     # no pass over the transpose
        del seen[:]
        S2 = S.clone().requires_grad_()
        ops.tg_conv(S2, g.sum, None, 1.0, None, ops.TG_EPI_NONE).sum().backward()
        assert seen == ["tg_conv_fwd", "gcn_conv_fwd"]                                                       # no pre-pass without an epilogue
    finally:
        ops.set_launch_timer(None)


def test_ops_refuse_what_they_cannot_run():
    from ctgcn_amd import ops
    adj = tg_graph("small").mean
    S = torch.zeros(6, 4, device=DEV)
    a = torch.zeros(1, 4, device=DEV)
    with pytest.raises(ValueError, match="epi"):
        ops.tg_conv(S, adj, epi=2)
    with pytest.raises(ValueError, match="epi"):
        ops.tgat_conv(S, a, a, adj, epi=3)
    with pytest.raises(ValueError, match="dropout p"):
        ops.tg_conv(S, adj, epi=1, p=1.0)
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.tgat_conv(S, a, a, adj, heads=3)
    with pytest.raises(ValueError, match="S must be"):
        ops.tg_conv(torch.zeros(5, 4, device=DEV), adj)
    with pytest.raises(TypeError):
        ops.tg_conv(S.double(), adj)
