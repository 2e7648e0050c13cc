"""ops.pool_conv (ctgcn_pool.hip) against float64 scipy: Y = epi(Â S + self_scale T + b) with and without the self term, with T and S
as the two halves of one buffer, with and without the ReLU / L2-normalisation / dropout epilogue and the bias, at every dispatch
boundary (scalar and float4 rows, every lane-group width, rows around each width, long rows in pieces); the backward's pre-pass
(G and the bias gradient); the draws against the host model; and the op under autograd against stock float64 autograd.  The matrices
are test_gpu_gcn_conv.py's (not symmetric).  Tolerance: conftest.close_scaled's, as for ops.gcn_conv; every output is repeated and
compared bit for bit."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _egcn_ref as E
import _gcrn_ref as R
from _gcn_graphs import DEV, DIMS, N, WIDTHS, dense, gcn_adj
from conftest import close_scaled
from test_gpu_gcn_conv import directed_graph, f64, graph, tolerance

pytestmark = pytest.mark.gpu
NONE, NORM = 0, 1
EPS = 1e-12
KEY = 2 ** 61 + 777
SCALE = 0.75
DEAD = (3, 4)                            # rows whose self term is so negative that nothing passes the ReLU


def used(got, ref, what):
    """prints the share of close_scaled's tolerance the worst entry uses"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    share = float((np.abs(got - ref) / tolerance(ref)).max(initial=0.0)) if ref.size else 0.0
    print("  [tol] %-40s %.3f of the tolerance" % (what, share))
    close_scaled(got, ref)


def operands(d, mode, strided=False):
    """(S, T, scale): mode 'none' no self term; 'self' a separate T with rows DEAD at -50; 'halves' T and S the halves of one buffer"""
    if mode == "halves":
        Z = torch.from_numpy(dense((N, 2 * d), d + 20)).to(DEV)
        return Z[:, d:], Z[:, :d], SCALE
    S = torch.from_numpy(dense((N, d), d)).to(DEV)
    if mode == "none":
        return S, None, 1.0
    t = dense((N, d), d + 21)
    t[list(DEAD)] = -50.0
    return S, torch.from_numpy(t).to(DEV), SCALE


def reference(m, S, T, scale, bias, epi):
    """(Y, norm) in float64"""
    pre = np.zeros((N, (T if S is None else S).shape[1])) if S is None else m @ f64(S)
    if T is not None:
        pre = pre + scale * f64(T)
    if bias is not None:
        pre = pre + f64(bias)
    if epi == NONE:
        return pre, None
    r = np.maximum(pre, 0.0)
    norm = np.sqrt((r * r).sum(axis=1))
    return r / np.maximum(norm, EPS)[:, None], norm


def prep_reference(dY, Y, norm, keep=None, p=0.0):
    """(G, db) in float64 from the kernel's own normalised rows and norms"""
    g = f64(dY) if keep is None else np.where(keep, f64(dY) / (1.0 - p), 0.0)
    y, nrm = f64(Y), f64(norm)
    ok = nrm >= EPS
    G = np.where(y > 0, (g - y * np.where(ok, (y * g).sum(axis=1), 0.0)[:, None]) / np.where(ok, nrm, EPS)[:, None], 0.0)
    return G, G.sum(axis=0)


def check_forward(m, adj, S, T, scale, bias, epi, what):
    from ctgcn_amd import ops
    Y, norm, save = ops._pool_conv_fwd(adj, S, T, scale, bias, epi)
    ref, ref_norm = reference(m, S, T, scale, bias, epi)
    used(f64(Y), ref, what)
    assert save is Y and (norm is None) == (epi == NONE)
    if epi == NORM:
        used(f64(norm), ref_norm, what + " norm")
    Y2, norm2, _ = ops._pool_conv_fwd(adj, S, T, scale, bias, epi)
    assert torch.equal(Y, Y2) and (norm is None or torch.equal(norm, norm2))
    return Y, norm


def check_prep(dY, Y, norm, p=0.0, key=0, what="prep"):
    from ctgcn_amd import ops
    n, d = dY.shape
    G, db = ops._pool_conv_prep(dY, Y, norm, p, key, want_db=True)
    ref, ref_db = prep_reference(dY, Y, norm, R.keep_mask(key, n, d, p) if p > 0 else None, p)
    used(f64(G), ref, what + " G")
    used(f64(db), ref_db, what + " db")
    G2, db2 = ops._pool_conv_prep(dY, Y, norm, p, key, want_db=True)
    G3, none = ops._pool_conv_prep(dY, Y, norm, p, key, want_db=False)
    assert torch.equal(G, G2) and torch.equal(db, db2) and none is None and torch.equal(G, G3)
    return G


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("epi", [NONE, NORM], ids=["none", "norm"])
@pytest.mark.parametrize("d", DIMS)
def test_forward_and_pre_pass_at_every_lane_group_width(d, epi, with_bias):
    bias = torch.from_numpy(dense((d,), d + 1)).to(DEV) if with_bias else None
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
    for width in WIDTHS:
        m = graph(width)
        adj = gcn_adj(m)
        assert adj.long_rows is None
        for mode in ("none", "self", "halves"):
            S, T, scale = operands(d, mode)
            assert mode != "halves" or (S.stride(0) == T.stride(0) == 2 * d and S.data_ptr() == T.data_ptr() + 4 * d)
            Y, norm = check_forward(m, adj, S, T, scale, bias, epi, "d %d width %d %s" % (d, width, mode))
            if mode == "none" and not with_bias:                 # the empty row: exactly 0, and so are its norm and its gradient
                assert not Y[0].any() and (epi == NONE or float(norm[0]) == 0.0)
            if epi == NORM:
                G = check_prep(dY, Y, norm, what="d %d width %d %s" % (d, width, mode))
                if mode == "self":                               # nothing passed the ReLU: Y = 0, norm = 0, G = 0
                    rows = torch.tensor(DEAD, device=DEV)
                    assert not Y[rows].any() and not norm[rows].any() and not G[rows].any()
                if mode == "none" and not with_bias:
                    assert not G[0].any()


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("epi", [NONE, NORM], ids=["none", "norm"])
@pytest.mark.parametrize("d", DIMS)
def test_long_rows_of_a_directed_matrix_and_of_its_transpose(d, epi, with_bias):
    """long_threshold 8: rows of 9 entries and more go to the piece kernels, forward over the matrix and backward over its transpose"""
    from ctgcn_amd import ops
    m = directed_graph()
    adj, plain = gcn_adj(m, long_threshold=8), gcn_adj(m)
    rows = np.diff(m.indptr)
    assert adj.long_rows is not None and adj.transposed().long_rows is not None and adj.pieces > 1
    bias = torch.from_numpy(dense((d,), d + 1)).to(DEV) if with_bias else None
    short = torch.from_numpy(rows <= 8).to(DEV)
    for mode in ("none", "self", "halves"):
        S, T, scale = operands(d, mode)
        Y, norm = check_forward(m, adj, S, T, scale, bias, epi, "pieces d %d %s" % (d, mode))
        assert torch.equal(Y[short], ops._pool_conv_fwd(plain, S, T, scale, bias, epi)[0][short])
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
    G = check_prep(dY, Y, norm, what="pieces d %d" % d) if epi == NORM else dY
    dS, _ = ops._gcn_conv_fwd(adj.transposed(), G, None, ops.GCN_EPI_NONE)
    used(f64(dS), m.T @ f64(G), "pieces d %d dS" % d)
    assert torch.equal(dS, ops._gcn_conv_fwd(adj.transposed(), G, None, ops.GCN_EPI_NONE)[0])


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("d", [10, 24, 130, 132])
def test_dropout_follows_the_host_model(d, p, long_threshold):
    from ctgcn_amd import ops
    m = graph(64)
    adj = gcn_adj(m, long_threshold)
    S, T, scale = operands(d, "self")
    bias = torch.from_numpy(dense((d,), d + 1)).to(DEV)
    plain, norm0, _ = ops._pool_conv_fwd(adj, S, T, scale, bias, NORM)
    assert torch.equal(plain, ops._pool_conv_fwd(adj, S, T, scale, bias, NORM, 0.0, KEY)[0])
    masks = []
    for key in (KEY, KEY + 1):
        Y, norm, save = ops._pool_conv_fwd(adj, S, T, scale, bias, NORM, p, key)
        keep = R.keep_mask(key, N, d, p)
        assert torch.equal(save, plain) and torch.equal(norm, norm0) and save is not Y     # what the backward reads: the rows before dropout
        y = f64(Y)
        assert not y[~keep].any() and np.array_equal(y != 0, keep & (f64(plain) > 0))
        used(y, np.where(keep, f64(plain) / (1.0 - p), 0.0), "dropout d %d p %g" % (d, p))
        Y2, _, save2 = ops._pool_conv_fwd(adj, S, T, scale, bias, NORM, p, key)
        assert torch.equal(Y, Y2) and torch.equal(save, save2)
        masks.append(keep)
    assert (masks[0] != masks[1]).mean() > 0.5 * 2 * p * (1 - p)
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
    check_prep(dY, save, norm, p, KEY + 1, "dropout d %d p %g" % (d, p))


@pytest.mark.parametrize("d", [1, 10, 24, 130, 132, 260])
def test_pre_pass_over_several_blocks(d):
    """199 rows: three full pre-pass blocks and one of 7 rows; 260 columns: two passes of the 64 float4 lanes"""
    n = 199
    rng = np.random.default_rng(d)
    dY = torch.from_numpy(dense((n, d), d + 3)).to(DEV)
    y = np.abs(dense((n, d), d + 4))
    y[rng.random((n, d)) < 0.3] = 0.0
    norm = rng.uniform(0.2, 3.0, n).astype(np.float32)
    norm[[0, 64, 198]] = [0.0, 5e-13, 9.9e-13]                  # below the clamp, in three different blocks
    y[[0, 64, 198]] = 0.0                                       # a norm that small means nothing passed the ReLU
    Y, nrm = torch.from_numpy(y).to(DEV), torch.from_numpy(norm).to(DEV)
    for p in (0.0, 0.5, 0.1):
        check_prep(dY, Y, nrm, p, KEY, "blocks d %d p %g" % (d, p))


@pytest.mark.parametrize("epi", [NONE, NORM], ids=["none", "norm"])
def test_padded_rows_at_an_unaligned_base_take_the_scalar_path(epi):
    from ctgcn_amd import ops
    d, ld = 24, 27

    def strided(seed):
        buf = torch.zeros(N * ld + 1, device=DEV)
        view = buf[1:].as_strided((N, d), (ld, 1))
        view.copy_(torch.from_numpy(dense((N, d), seed)))
        assert view.data_ptr() % 16 == 4
        return view

    bias = torch.from_numpy(dense((d,), 9)).to(DEV)
    for long_threshold in (None, 8):
        m = directed_graph()
        adj = gcn_adj(m, long_threshold)
        S, T = strided(5), strided(6)
        Y, norm = check_forward(m, adj, S, T, SCALE, bias, epi, "unaligned")
        aligned = ops._pool_conv_fwd(adj, S.contiguous(), T.contiguous(), SCALE, bias, epi)[0]
        close_scaled(f64(Y), f64(aligned))
        if epi == NORM:
            check_prep(strided(7), Y, norm, what="unaligned")


def test_the_epilogue_alone_and_argument_checks():
    from ctgcn_amd import ops
    d = 24
    pre = torch.from_numpy(dense((N, d), 3)).to(DEV)
    bias = torch.from_numpy(dense((d,), 4)).to(DEV)
    Y = ops.pool_conv(None, None, T=pre, bias=bias, epi=ops.POOL_EPI_NORM)
    used(f64(Y), reference(None, None, pre, 1.0, bias, NORM)[0], "epilogue alone")
    assert torch.equal(Y, ops.pool_conv(None, None, T=pre, bias=bias, epi=ops.POOL_EPI_NORM))
    adj = gcn_adj(graph(32))
    S = torch.from_numpy(dense((N, d), 5)).to(DEV)
    for bad in (lambda: ops.pool_conv(S, None), lambda: ops.pool_conv(None, None), lambda: ops.pool_conv(S[:-1], adj),
                lambda: ops.pool_conv(S, adj, T=S[:, :-1]), lambda: ops.pool_conv(S, adj, epi=2), lambda: ops.pool_conv(S, adj, epi=1, p=1.0),
                lambda: ops.pool_conv(S, adj, bias=bias[:-1])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.pool_conv(S.double(), adj)


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("mode", ["none", "self", "same", "halves"])
@pytest.mark.parametrize("epi,p", [(NONE, 0.0), (NORM, 0.0), (NORM, 0.5)], ids=["none", "norm", "dropout"])
def test_autograd_function_matches_stock_autograd(epi, p, mode, long_threshold):
    """mode 'same': T is S itself (GIN with a learnt eps), self_scale a tensor that takes a gradient; 'halves': one buffer's gradient"""
    from ctgcn_amd import ops
    m = directed_graph()
    adj = gcn_adj(m, long_threshold)
    d = 24
    C = torch.from_numpy(dense((N, d), 13)).to(DEV)
    b = torch.from_numpy(dense((d,), 12)).to(DEV).requires_grad_()
    scale = torch.tensor(SCALE, device=DEV, requires_grad=True) if mode in ("self", "same") else 1.0
    if mode == "halves":
        leaf = torch.from_numpy(dense((N, 2 * d), 11)).to(DEV).requires_grad_()
        Z = leaf * 1.0
        S, T = Z[:, d:], Z[:, :d]
    else:
        leaf = torch.from_numpy(dense((N, d), 11)).to(DEV).requires_grad_()
        S = leaf
        T = None if mode == "none" else S if mode == "same" else torch.from_numpy(dense((N, d), 14)).to(DEV).requires_grad_()
    Y = ops.pool_conv(S, adj, T=T, self_scale=scale, bias=b, epi=epi, p=p, key=KEY)
    (Y * C).sum().backward()

    leaf64, b64 = leaf.detach().cpu().double().requires_grad_(), b.detach().cpu().double().requires_grad_()
    scale64 = torch.tensor(SCALE, dtype=torch.float64, requires_grad=True)
    A = E.sparse_tensor(m, torch.float64)
    if mode == "halves":
        S64, T64 = leaf64[:, d:], leaf64[:, :d]
    else:
        S64 = leaf64
        T64 = None if mode == "none" else S64 if mode == "same" else T.detach().cpu().double().requires_grad_()
    pre = torch.sparse.mm(A, S64) + b64
    if T64 is not None:
        pre = pre + (scale64 if mode in ("self", "same") else 1.0) * T64
    Y64 = pre
    if epi == NORM:
        Y64 = F.normalize(F.relu(pre), p=2)
        if p > 0:
            Y64 = Y64 * torch.from_numpy(R.keep_mask(KEY, N, d, p)).double() / (1.0 - p)
    (Y64 * C.cpu().double()).sum().backward()
    what = "autograd %s %s" % (mode, "pieces" if long_threshold else "rows")
    used(f64(Y), Y64.detach().numpy(), what + " Y")
    used(f64(leaf.grad), leaf64.grad.numpy(), what + " d leaf")
    used(f64(b.grad), b64.grad.numpy(), what + " db")
    if mode == "self":
        used(f64(T.grad), T64.grad.numpy(), what + " dT")
    if mode in ("self", "same"):
        used(f64(scale.grad), scale64.grad.numpy(), what + " d self_scale")
    # repeated: bit-identical
    grads = [leaf.grad.clone(), b.grad.clone()]
    leaf.grad = b.grad = None
    if mode == "halves":
        Z = leaf * 1.0
        S, T = Z[:, d:], Z[:, :d]
    Y2 = ops.pool_conv(S, adj, T=T, self_scale=scale, bias=b, epi=epi, p=p, key=KEY)
    (Y2 * C).sum().backward()
    assert torch.equal(Y, Y2) and torch.equal(leaf.grad, grads[0]) and torch.equal(b.grad, grads[1])
