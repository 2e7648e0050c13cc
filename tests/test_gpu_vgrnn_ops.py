"""The VGRNN baseline's fused gathers on the GPU (ops.ggru_gates, ops.ggru_blend, ops.vgrnn_heads; ctgcn_vgrnn.hip): forward and every
gradient against the same expressions in float64 with a dense matrix, at the widths at which the row kernel takes another path
(5: scalar rows, 8 lanes a row; 12: scalar, 16 lanes; 16: float4, 4 lanes; 128: float4, 32 lanes; 130: scalar, 64 lanes and more than one
chunk a lane), with and without rows cut into pieces (long_threshold 4), on a matrix with rows without entries, on contiguous operands
and on views with a row stride above the width.

There is no recorded yardstick for a single op, so the same expression in stock fp32 torch ops on the same GPU is measured against the
float64 result too; the op may use 4 x that error (the project's margin for fp32 yardsticks) with the fixture rule's floors: 2e-6
max|ref| for results, 1e-5 max|ref| for gradients."""
import pytest
import torch
from torch.nn import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N = 70
WIDTHS = [5, 12, 16, 128, 130]
_graphs = {}


def graph(long_threshold):
    """(GcnAdj, dense float64 matrix): asymmetric, weighted, row 0 and column 3 of 40 entries, the last ten rows empty"""
    from ctgcn_amd import ops
    if long_threshold not in _graphs:
        gen = torch.Generator().manual_seed(11)
        rows = torch.cat([torch.randint(0, N - 10, (200,), generator=gen), torch.zeros(40, dtype=torch.int64), torch.arange(40)])
        cols = torch.cat([torch.randint(0, N, (200,), generator=gen), torch.arange(40), torch.full((40,), 3)])
        vals = torch.rand(rows.numel(), generator=gen) * 0.4 + 0.05
        t = torch.sparse_coo_tensor(torch.stack((rows, cols)), vals, (N, N)).coalesce()
        adj = ops.GcnAdj.from_sparse_tensor(t, DEV, long_threshold=long_threshold, check_symmetric=False)
        assert (adj.long_rows is not None) == bool(long_threshold)
        if long_threshold:
            assert adj.transposed().long_rows is not None
        _graphs[long_threshold] = (adj, t.to_dense().double())
    return _graphs[long_threshold]


def operands(shapes, seed, scale=1.0):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=gen) * scale for s in shapes]


def place(t, view):
    """t on the GPU as a leaf: contiguous, or rows of a wider buffer at an odd offset (a row stride above the width, no float4 alignment)"""
    if not view:
        return t.to(DEV).requires_grad_(True)
    buf = torch.zeros(t.shape[0], t.shape[1] + 7, device=DEV)
    buf[:, 3:3 + t.shape[1]] = t.to(DEV)
    return buf.requires_grad_(True)


def taken(t, leaf, view):
    """the operand an op reads: the leaf, or its view"""
    return leaf[:, 3:3 + t.shape[1]] if view else leaf


def leaf_grad(t, leaf, view):
    return taken(t, leaf.grad, view).double().cpu()


def check(what, fn_ref, fn_op, inputs, weights, diff, view):
    """fn_ref(A, *inputs) in float64 / float32, fn_op(*inputs) on the GPU; results weighted by `weights` into one scalar for the gradients
    of inputs[k], k in diff"""
    def run_ref(dtype, device):
        ins = [t.to(device=device, dtype=dtype).requires_grad_(k in diff) for k, t in enumerate(inputs)]
        outs = fn_ref(dtype, device, *ins)
        sum((o * w.to(device=device, dtype=dtype)).sum() for o, w in zip(outs, weights)).backward()
        return [o.detach().double().cpu() for o in outs], [ins[k].grad.double().cpu() for k in diff]

    want, want_g = run_ref(torch.float64, "cpu")
    yard, yard_g = run_ref(torch.float32, DEV)
    leaves = [place(t, view and t.dim() == 2) if k in diff else t.to(DEV) for k, t in enumerate(inputs)]
    outs = fn_op(*[taken(t, l, view and t.dim() == 2) if k in diff else l for k, (t, l) in enumerate(zip(inputs, leaves))])
    sum((o * w.to(DEV)).sum() for o, w in zip(outs, weights)).backward()
    got = [o.detach().double().cpu() for o in outs]
    got_g = [leaf_grad(inputs[k], leaves[k], view and inputs[k].dim() == 2) for k in diff]
    over = {}
    for kind, floor, triples in (("out", 2e-6, zip(got, yard, want)), ("grad", 1e-5, zip(got_g, yard_g, want_g))):
        for k, (g, y, w) in enumerate(triples):
            top = float(w.abs().max())
            err, yerr = float((g - w).abs().max()) / top, float((y - w).abs().max()) / top
            print("  [tol] %-34s %s %d  op %.3e  stock fp32 %.3e  allowed %.3e" % (what, kind, k, err, yerr, max(4 * yerr, floor)))
            if not err <= max(4 * yerr, floor):
                over["%s%d" % (kind, k)] = (err, yerr)
    assert not over, (what, over)
    return outs, [l.grad.clone() for k, l in enumerate(leaves) if k in diff]


def dense(A, dtype, device):
    return A.to(device=device, dtype=dtype)


@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "views"])
@pytest.mark.parametrize("long_threshold", [None, 4], ids=["rows", "pieces"])
@pytest.mark.parametrize("H", WIDTHS)
def test_ggru_gates(H, long_threshold, view):
    from ctgcn_amd import ops
    adj, A = graph(long_threshold)
    U, h, bias = operands([(N, 3 * H), (N, H), (3 * H,)], 100 + H)
    weights = operands([(N, H)] * 3, 200 + H)

    def ref(dtype, device, U, h, bias):
        G = dense(A, dtype, device) @ U + bias
        return torch.sigmoid(G[:, :H]), torch.sigmoid(G[:, H:2 * H]) * h, G[:, 2 * H:]

    check("gates H%d" % H, ref, lambda U, h, bias: ops.ggru_gates(U, h, adj, bias), [U, h, bias], weights, (0, 1, 2), view)


@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "views"])
@pytest.mark.parametrize("long_threshold", [None, 4], ids=["rows", "pieces"])
@pytest.mark.parametrize("H", WIDTHS)
def test_ggru_blend(H, long_threshold, view):
    from ctgcn_amd import ops
    adj, A = graph(long_threshold)
    V, c, z, h = operands([(N, H)] * 4, 300 + H)
    z = torch.sigmoid(z)
    weights = operands([(N, H)], 400 + H)

    def ref(dtype, device, V, c, z, h):
        ht = torch.tanh(c + dense(A, dtype, device) @ V)
        return (z * h + (1 - z) * ht,)

    check("blend H%d" % H, ref, lambda V, c, z, h: (ops.ggru_blend(V, c, z, h, adj),), [V, c, z, h], weights, (0, 1, 2, 3), view)


@pytest.mark.parametrize("view", [False, True], ids=["contiguous", "views"])
@pytest.mark.parametrize("long_threshold", [None, 4], ids=["rows", "pieces"])
@pytest.mark.parametrize("out", WIDTHS)
def test_vgrnn_heads(out, long_threshold, view):
    """bias column out + 0 lifts that standard deviation's pre-activation above F.softplus's threshold of 20"""
    from ctgcn_amd import ops
    adj, A = graph(long_threshold)
    S, bias, noise = operands([(N, 2 * out), (2 * out,), (N, out)], 500 + out)
    bias[out] = 25.0
    weights = operands([(N, out)] * 3, 600 + out)

    def ref(dtype, device, S, bias, noise):
        G = dense(A, dtype, device) @ S + bias
        mean, std = G[:, :out], F.softplus(G[:, out:])
        return mean, std, mean + noise * std

    outs, _ = check("heads out%d" % out, ref, lambda S, bias, noise: ops.vgrnn_heads(S, adj, bias, noise), [S, bias, noise], weights, (0, 1), view)
    assert bool((outs[1][N - 10:, 0] == 25.0).all())              # an empty row holds the bias alone: the pass-through branch above 20


def test_the_ops_are_bit_identical_when_repeated_and_take_no_bias():
    from ctgcn_amd import ops
    adj, A = graph(4)
    H = 16
    U, h, S, noise, V, c, z = (t.to(DEV) for t in operands([(N, 3 * H), (N, H), (N, 2 * H), (N, H), (N, H), (N, H), (N, H)], 9))

    def once():
        Ug, hg, Sg, Vg = (t.clone().requires_grad_(True) for t in (U, h, S, V))
        zz, q, cc = ops.ggru_gates(Ug, hg, adj)
        hn = ops.ggru_blend(Vg, cc, zz, hg, adj)
        mean, std, zs = ops.vgrnn_heads(Sg, adj, None, noise)
        (hn.sum() + (q * c).sum() + (zs * z).sum() + std.sum()).backward()
        return [t.detach().clone() for t in (zz, q, cc, hn, mean, std, zs, Ug.grad, hg.grad, Sg.grad, Vg.grad)]

    a, b = once(), once()
    assert all(torch.equal(x, y) for x, y in zip(a, b))
    G = A.float().to(DEV) @ U
    assert float((a[2] - G[:, 2 * H:]).abs().max()) <= 1e-5 * float(G.abs().max())      # no bias: c is the plain aggregation
    with pytest.raises(ValueError):
        ops.ggru_gates(U[:, :H], h, adj)
    with pytest.raises(TypeError):
        ops.vgrnn_heads(S.double(), adj, None, noise)
