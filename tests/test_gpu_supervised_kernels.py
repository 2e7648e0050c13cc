"""Kernels of the supervised classifier head (ctgcn_supervised.hip through ctgcn_amd.ops): head forward, loss pass and pull backward
of the three modes against float64 torch autograd of the reference's expression on the same fp32 inputs.

Tolerance (the parity rule of tests/test_gpu_configs.py): the error against float64 may be at most 1.5 x the error of torch's own fp32
evaluation of the same expression on the same inputs, with a floor of 8 units of 2^-24 of the largest magnitude in the compared array
(at these sizes the fp32 evaluation can be exact by luck)."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_NODES, N_USED, T = 200, 150, 3           # nodes N_USED.. carry no item
NODE, HADAMARD, DOT = 0, 1, 2
E_INVALID, E_UNSUPPORTED = -1, -4

#        mode      items  d    C   act  hub
CASES = [(NODE, 1, 8, 2, 0, False), (NODE, 31, 20, 3, 1, False), (NODE, 32, 128, 7, 0, False), (NODE, 33, 256, 32, 1, False),
         (NODE, 1057, 128, 4, 0, True),
         (HADAMARD, 1, 20, 3, 1, False), (HADAMARD, 31, 128, 2, 0, False), (HADAMARD, 32, 256, 7, 1, False),
         (HADAMARD, 33, 8, 32, 0, False), (HADAMARD, 1057, 128, 3, 1, True), (HADAMARD, 70001, 20, 3, 0, False),
         (DOT, 1, 8, 0, 0, False), (DOT, 31, 256, 0, 0, False), (DOT, 32, 20, 0, 0, False), (DOT, 33, 128, 0, 0, False),
         (DOT, 1057, 128, 0, 0, True)]
IDS = ["%s-i%d-d%d-C%d-%s%s" % (("node", "had", "dot")[m], i, d, C, "LN"[a], "-hub" if h else "") for m, i, d, C, a, h in CASES]


def _parity(got, ref64, torch32, what):
    """|got - ref| <= max(1.5 x |torch fp32 - ref|_max, 8 x 2^-24 x max|ref|); prints the used fraction (conftest.check_close's habit)."""
    got, ref, t32 = (x.detach().double().cpu().numpy() for x in (got, ref64, torch32))
    scale = float(np.abs(ref).max(initial=0.0))
    tol = max(1.5 * float(np.abs(t32 - ref).max(initial=0.0)), 8.0 * 2.0 ** -24 * scale)
    err = float(np.abs(got - ref).max(initial=0.0))
    print("  [tol] %-40s max |err| %.3e = %.3f of the tolerance %.3e (torch fp32 err %.3e, scale %.3e)"
          % (what, err, err / tol if tol else 0.0, tol, float(np.abs(t32 - ref).max(initial=0.0)), scale))
    assert err <= tol, "%s: max |err| %.3e above the tolerance %.3e" % (what, err, tol)


def _inputs(mode, items, d, C, hub, seed=11):
    from ctgcn_amd import ops
    g = torch.Generator().manual_seed(seed + 1000 * mode + items + d)
    E3 = torch.randn(N_NODES, T, d, generator=g).to(DEV)
    E = E3.transpose(0, 1)[1]                              # a strided [N, d] view of [N, T, d]: lde = T * d
    assert E.stride(0) == T * d and E.stride(1) == 1
    a = torch.randint(0, N_USED, (items,), generator=g)
    b = torch.randint(0, N_USED, (items,), generator=g)
    k = min(5, items)
    if hub:                                                # node 7 takes part in 2 * CLS_PULL_PIECE + 5 incidences
        want = 2 * ops.CLS_PULL_PIECE + 5
        b[b == 7] = 8
        a[a == 7] = 9
    b[:k] = a[:k]                                          # five pairs with from == to
    if hub:
        a[10:10 + want] = 7
        assert int((a == 7).sum() + (0 if mode == NODE else (b == 7).sum())) == want
    idx = a.to(DEV) if mode == NODE else torch.stack([a, b]).to(DEV)
    W = ((torch.rand(max(C, 1), d, generator=g) * 2 - 1) / np.sqrt(d)).to(DEV)
    bias = ((torch.rand(max(C, 1), generator=g) * 2 - 1) * 0.1).to(DEV)
    y = torch.randint(0, max(C, 2), (items,), generator=g).to(DEV)
    return E3, E, idx, W, bias, y


def _features(E, idx, mode):
    return E[idx] if mode == NODE else E[idx[0]] * E[idx[1]]


def _head_ref(E, idx, W, bias, mode, act, dtype):
    """the reference's expression (models.py:78-82, :105-113) in `dtype`: (logits, pre-activation)"""
    E, W, bias = E.to(dtype), W.to(dtype), bias.to(dtype)
    f = _features(E, idx, mode)
    if mode == DOT:
        z = torch.sum(f, dim=1)
        return z, z
    pre = F.linear(f, W, bias)
    return (F.selu(pre) if act else pre), pre


@pytest.mark.parametrize("mode,items,d,C,act,hub", CASES, ids=IDS)
def test_head_forward(mode, items, d, C, act, hub):
    from ctgcn_amd import ops
    E3, E, idx, W, bias, _ = _inputs(mode, items, d, C, hub)
    it = ops.cls_items(idx, mode, N_NODES)
    got = ops.cls_head_forward(E, it, W, bias, act)
    ref, _ = _head_ref(E, idx, W, bias, mode, act, torch.float64)
    t32, _ = _head_ref(E, idx, W, bias, mode, act, torch.float32)
    assert got.shape == ref.shape and got.dtype == torch.float32
    _parity(got, ref, t32, "logits")
    assert torch.equal(got, ops.cls_head_forward(E, it, W, bias, act))                      # bit-identical on a second call
    assert torch.equal(got, ops.cls_head_forward(E.contiguous(), it, W, bias, act))         # the layout of E does not change a bit


def _gapped_logits(items, C, seed):
    """fp32 logits whose float64 top-two gap (|z| for C == 0) is at least 1e-5 on every row"""
    g = torch.Generator().manual_seed(seed)
    if C == 0:
        z = torch.randn(items, generator=g) * 3
        z[z.abs() < 1e-3] = 0.5
        return z.to(DEV)
    z = torch.randn(items, C, generator=g) * 2
    top = z.topk(2, dim=1)
    close = (top.values[:, 0] - top.values[:, 1]) < 1e-3
    z[close, top.indices[close, 0]] += 1.0
    return z.to(DEV)


def _loss_ref(z, y, C, act, dtype):
    """(loss, prob, dlogits) in `dtype`; act: z are activated logits and dlogits carries SELU' written from the output"""
    z = z.detach().to(dtype).requires_grad_(True)
    if C == 0:
        loss = F.binary_cross_entropy_with_logits(z, y.to(dtype))
        prob = torch.sigmoid(z)
    else:
        loss = F.cross_entropy(z, y)
        prob = torch.softmax(z, dim=1)
    dl, = torch.autograd.grad(loss, z)
    if act:
        alpha, scale = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
        dl = dl * torch.where(z > 0, torch.full_like(z, scale), z + scale * alpha)
    return loss.detach(), prob.detach(), dl.detach()


@pytest.mark.parametrize("items,C,act", [(1, 2, 0), (31, 3, 1), (32, 7, 0), (33, 32, 1), (1057, 4, 0), (1, 0, 0), (33, 0, 0), (1057, 0, 0),
                                         (300000, 4, 1)])
def test_loss_pass(items, C, act):
    from ctgcn_amd import ops
    z = _gapped_logits(items, C, seed=5 + items + C)
    g = torch.Generator().manual_seed(99 + items)
    y = torch.randint(0, max(C, 2), (items,), generator=g).to(DEV)
    z64 = z.double()
    if C == 0:
        assert float(z64.abs().min()) >= 1e-5
        want_correct = int(((z64 > 0).long() == y).sum())
    else:
        top = z64.topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= 1e-5
        want_correct = int((z64.argmax(1) == y).sum())
    loss, correct, prob, dl = ops.cls_loss(z, y, dot=C == 0, act=act)
    assert int(correct) == want_correct
    r64, r32 = _loss_ref(z, y, C, act, torch.float64), _loss_ref(z, y, C, act, torch.float32)
    _parity(loss, r64[0].reshape(1), r32[0].reshape(1), "loss")
    _parity(prob, r64[1], r32[1], "probabilities")
    _parity(dl, r64[2], r32[2], "dlogits")
    again = ops.cls_loss(z, y, dot=C == 0, act=act)
    assert all(torch.equal(p, q) for p, q in zip((loss, correct, prob, dl), again))
    only = ops.cls_loss(z, y, dot=C == 0, act=act, want_prob=False, want_grad=False)
    assert only[2] is None and only[3] is None and torch.equal(only[0], loss) and torch.equal(only[1], correct)


def test_loss_pass_ties():
    """two equal maxima in a row: the first wins, as torch.max does; z == 0 predicts class 0"""
    from ctgcn_amd import ops
    z = torch.tensor([[0.5, 2.0, 2.0, -1.0], [3.0, 1.0, 3.0, 0.0], [0.0, 0.0, 0.0, 0.0], [1.0, 2.0, 3.0, 4.0]], device=DEV)
    for y, want in (([1, 0, 0, 3], 4), ([2, 2, 1, 3], 1)):
        y = torch.tensor(y, device=DEV)
        assert int(ops.cls_loss(z, y)[1]) == want == int((z.max(1)[1] == y).sum())
    zd = torch.tensor([0.0, 1.0, -1.0, 0.0], device=DEV)
    assert int(ops.cls_loss(zd, torch.tensor([0, 1, 0, 1], device=DEV), dot=True)[1]) == 3


@pytest.mark.parametrize("mode,items,d,C,act,hub", CASES, ids=IDS)
def test_head_backward(mode, items, d, C, act, hub):
    from ctgcn_amd import ops
    E3, E, idx, W, bias, y = _inputs(mode, items, d, C, hub)
    it = ops.cls_items(idx, mode, N_NODES)
    g = torch.Generator().manual_seed(3 + items)
    dl = (torch.randn((items,) if mode == DOT else (items, C), generator=g) / items).to(DEV)

    def ref(dtype):
        Ed = E.detach().to(dtype).requires_grad_(True)
        Wd, bd = W.detach().to(dtype).requires_grad_(True), bias.detach().to(dtype).requires_grad_(True)
        f = _features(Ed, idx, mode)
        pre = torch.sum(f, dim=1) if mode == DOT else F.linear(f, Wd, bd)
        wrt = [Ed] if mode == DOT else [Ed, Wd, bd]
        return torch.autograd.grad((pre * dl.to(dtype)).sum(), wrt)

    r64, r32 = ref(torch.float64), ref(torch.float32)
    buf = torch.full((N_NODES, T, d), float("nan"), device=DEV)
    dE_view = buf.transpose(0, 1)[1]
    dE, dW, db = ops.cls_head_backward(E, it, None if mode == DOT else W, dl, dE=dE_view)
    assert dE.data_ptr() == dE_view.data_ptr()
    assert torch.isnan(buf[:, 0]).all() and torch.isnan(buf[:, 2]).all()          # nothing written outside the [N, d] view
    touched = torch.zeros(N_NODES, dtype=torch.bool, device=DEV)
    touched[idx.reshape(-1)] = True
    assert not touched[N_USED:].any() and bool((dE[~touched] == 0).all())           # rows of untouched nodes: exactly zero
    _parity(dE, r64[0], r32[0], "dE")
    if mode == DOT:
        assert dW is None and db is None
    else:
        _parity(dW, r64[1], r32[1], "dW")
        _parity(db, r64[2], r32[2], "db")
    dE2, dW2, db2 = ops.cls_head_backward(E, it, None if mode == DOT else W, dl)
    assert torch.equal(dE2, dE) and (mode == DOT or (torch.equal(dW2, dW) and torch.equal(db2, db)))
    if hub:
        inc = it.incidence
        assert inc.n_hubs == 1 and int(inc.hub_node[0]) == 7 and inc.hub_pieces == 3


@pytest.mark.parametrize("mode,act", [(NODE, 1), (HADAMARD, 0), (DOT, 0)])
def test_autograd_wrappers(mode, act):
    """ops.cls_head + ops.cls_loss_autograd against the same expression in stock torch ops, end to end through autograd"""
    from ctgcn_amd import ops
    items, d, C = 257, 128, 0 if mode == DOT else 4
    E3, E, idx, W, bias, y = _inputs(mode, items, d, C, False)

    def run(fused, dtype):
        E3d = E3.detach().to(dtype).requires_grad_(True)
        Ed = E3d.transpose(0, 1)[1]
        Wd, bd = W.detach().to(dtype).requires_grad_(True), bias.detach().to(dtype).requires_grad_(True)
        if fused:
            z = ops.cls_head(Ed, idx, None if mode == DOT else Wd, None if mode == DOT else bd, mode, act)
            loss, correct, prob = ops.cls_loss_autograd(z, y, dot=mode == DOT)
        else:
            z, _ = _head_ref(Ed, idx, Wd, bd, mode, act, dtype)
            loss = F.binary_cross_entropy_with_logits(z, y.to(dtype)) if mode == DOT else F.cross_entropy(z, y)
        loss.backward()
        return [loss.detach().reshape(1), E3d.grad] + ([] if mode == DOT else [Wd.grad, bd.grad])

    got, r64, r32 = run(True, torch.float32), run(False, torch.float64), run(False, torch.float32)
    for name, a, b, c in zip(("loss", "dE", "dW", "db"), got, r64, r32):
        _parity(a, b, c, name)


def test_bad_arguments_return_codes():
    """d = 257 and C = 33 are CTGCN_E_UNSUPPORTED, an index outside [0, n_nodes) is CTGCN_E_INVALID from the host check: no launch"""
    from ctgcn_amd import _lib, ops
    from ctgcn_amd._lib import ptr
    lib = _lib.load()
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    E = torch.zeros(4, 257, device=DEV)
    W = torch.zeros(33, 257, device=DEV)
    a = torch.tensor([0, 1, 2], device=DEV)
    out = torch.zeros(3, 33, device=DEV)
    assert lib.ctgcn_cls_head_fwd_f32(NODE, 0, 3, 257, 4, ptr(a), None, 4, ptr(E), 257, ptr(W), None, ptr(out), st) == E_UNSUPPORTED
    assert lib.ctgcn_cls_head_fwd_f32(NODE, 0, 3, 256, 33, ptr(a), None, 4, ptr(E), 257, ptr(W), None, ptr(out), st) == E_UNSUPPORTED
    assert b"n_class" in lib.ctgcn_last_error()
    assert lib.ctgcn_cls_head_fwd_f32(HADAMARD, 0, 3, 256, 4, ptr(a), None, 4, ptr(E), 257, ptr(W), None, ptr(out), st) == E_INVALID
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=DEV)
    loss = torch.zeros(1, dtype=torch.float64, device=DEV)
    cnt = torch.zeros(1, dtype=torch.int64, device=DEV)
    assert lib.ctgcn_cls_loss_f32(NODE, 0, 3, 33, ptr(out), ptr(a), ptr(loss), ptr(cnt), None, None, ptr(ws), ws.numel(), st) == E_UNSUPPORTED
    assert lib.ctgcn_cls_head_bwd_f32(NODE, 3, 257, 4, ptr(a), None, 4, ptr(E), 257, ptr(W), ptr(out), 0, None, None, None, None, None, 0,
                                      None, None, 0, None, 0, None, None, ptr(ws), ws.numel(), st) == E_UNSUPPORTED
    bad = torch.tensor([0, -1, 2], device=DEV)
    assert lib.ctgcn_cls_check_items(NODE, 3, ptr(bad), None, 4, st) == E_INVALID
    assert lib.ctgcn_cls_check_items(DOT, 3, ptr(a), ptr(torch.tensor([0, 4, 2], device=DEV)), 4, st) == E_INVALID
    assert lib.ctgcn_cls_check_items(DOT, 3, ptr(a), ptr(a), 4, st) == 0
    with pytest.raises(_lib.CtgcnHipError, match="outside"):
        ops.cls_items(bad, NODE, 4)
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0
