"""The GCN / GCRN kernels of ctgcn_gcn.hip against float64 scipy: the aggregation with its bias and epilogues (none, ReLU + dropout,
L2 row normalisation) at every dispatch boundary (scalar and float4 rows, every lane-group width, rows around each width, long rows
in pieces), the backward's pre-pass (G and the bias gradient), the aggregation over the transposed CSR, and ops.gcn_conv under
autograd.  The matrices are not symmetric: the graphs of _gcn_graphs.py with their rows scaled."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _egcn_ref as E
import _gcrn_ref as R
from _gcn_graphs import DEV, DIMS, N, WIDTHS, dense, gcn_adj, symmetric_graph
from conftest import close_scaled

pytestmark = pytest.mark.gpu
N2 = 199                                 # the pre-pass takes 64 rows per block: four blocks, the last of 7 rows
NONE, RELU, L2NORM = 0, 1, 2
EPIS = {"none": NONE, "relu": RELU, "l2norm": L2NORM}
EPS = 1e-12
KEY = 2 ** 61 + 12345
_graphs = {}


def row_scaled(m, seed):
    """diag(r) m with random positive r, values exact in float32: same pattern, no longer symmetric"""
    r = np.random.default_rng(seed).uniform(0.5, 1.5, m.shape[0])
    out = (sp.diags(r) @ m).tocsr()
    out.sort_indices()
    out.data = out.data.astype(np.float32).astype(np.float64)
    return out


def graph(width):
    if width not in _graphs:
        m = row_scaled(symmetric_graph(width), 7 + width)
        assert abs(m - m.T).sum() > 1 and list(np.diff(m.indptr)[:2]) == [0, 1]
        _graphs[width] = m
    return _graphs[width]


def directed_graph():
    """graph(64) with the strictly-lower-triangular entries of every third row removed: the rows and the columns have different
    lengths, so the matrix and its transpose have different long rows"""
    if "directed" not in _graphs:
        m = graph(64).tolil()
        for i in range(0, N, 3):
            for j in [j for j in m.rows[i] if j < i]:
                m[i, j] = 0.0
        m = m.tocsr()
        m.eliminate_zeros()
        m.sort_indices()
        _graphs["directed"] = m
    return _graphs["directed"]


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def pre_activation(m, S, bias):
    pre = m @ f64(S)
    return pre if bias is None else pre + f64(bias)


def epilogue(pre, epi):
    """(Y, norm) in float64"""
    if epi == RELU:
        return np.maximum(pre, 0.0), None
    if epi == L2NORM:
        norm = np.sqrt((pre * pre).sum(axis=1))
        return pre / np.maximum(norm, EPS)[:, None], norm
    return pre, None


def tolerance(ref):
    """close_scaled's per-entry tolerance"""
    return 1e-5 * np.abs(ref) + 2e-6 * max(1.0, float(np.abs(ref).max(initial=0.0)))


def check_forward(m, adj, d, epi, with_bias, S=None, out=None):
    from ctgcn_amd import ops
    n = m.shape[0]
    S = torch.from_numpy(dense((n, d), d)).to(DEV) if S is None else S
    bias = torch.from_numpy(dense((d,), d + 1)).to(DEV) if with_bias else None
    Y, norm = ops._gcn_conv_fwd(adj, S, bias, epi, out=out)
    ref, ref_norm = epilogue(pre_activation(m, S, bias), epi)
    close_scaled(f64(Y), ref)
    assert (norm is None) == (epi != L2NORM)
    if epi == L2NORM:
        close_scaled(f64(norm), ref_norm)
    Y1 = Y.clone()
    Y2, norm2 = ops._gcn_conv_fwd(adj, S, bias, epi, out=out)
    assert torch.equal(Y1, Y2) and (norm is None or torch.equal(norm, norm2))
    return Y, norm, bias


def prep_reference(dY, Y, norm, epi, p):
    """(G, db) in float64"""
    dY = f64(dY)
    if epi == NONE:
        G = dY
    elif epi == RELU:
        G = np.where(f64(Y) > 0, dY / (1.0 - p), 0.0)
    else:
        y, nrm = f64(Y), f64(norm)
        ok = nrm >= EPS
        G = np.where(ok[:, None], (dY - y * (y * dY).sum(axis=1, keepdims=True)) / np.where(ok, nrm, 1.0)[:, None], dY / EPS)
    return G, G.sum(axis=0)


def check_prep(dY, Y, norm, epi, p=0.0, clamped=()):
    """the pre-pass against float64; rows in `clamped` (norm below the clamp: G = dY / 1e-12, twelve orders above the rest) are held
    to the tolerance on their own, and the bias gradient is compared over the other rows"""
    from ctgcn_amd import ops
    G, db = ops._gcn_conv_prep(dY, Y, norm, epi, p, want_db=True)
    ref, _ = prep_reference(dY, Y, norm, epi, p)
    rest = np.setdiff1d(np.arange(dY.shape[0]), np.asarray(clamped, dtype=np.int64))
    if epi == NONE:
        assert G is dY                                          # nothing is written
    else:
        close_scaled(f64(G)[rest], ref[rest])
        for r in clamped:
            close_scaled(f64(G)[r], f64(dY)[r] / EPS)
    if len(clamped) == 0:
        close_scaled(f64(db), ref.sum(axis=0))
    G2, db2 = ops._gcn_conv_prep(dY, Y, norm, epi, p, want_db=True)
    assert torch.equal(G, G2) and torch.equal(db, db2)
    G3, none = ops._gcn_conv_prep(dY, Y, norm, epi, p, want_db=False)
    assert none is None and torch.equal(G, G3)
    return G, db


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
@pytest.mark.parametrize("d", DIMS)
def test_forward_and_pre_pass_at_every_lane_group_width(d, epi, with_bias):
    for width in WIDTHS:
        m = graph(width)
        adj = gcn_adj(m)
        assert adj.long_rows is None and not adj.symmetric
        Y, norm, bias = check_forward(m, adj, d, epi, with_bias)
        # the empty row: exactly the bias (its epilogue), or exactly 0 without one
        want0, _ = epilogue(f64(bias)[None, :] if with_bias else np.zeros((1, d)), epi)
        if epi == L2NORM and with_bias:
            close_scaled(f64(Y[0]), want0[0])
        else:
            assert np.array_equal(f64(Y[0]), want0[0])
        if epi == L2NORM and not with_bias:
            assert float(norm[0]) == 0.0
        if d > 1:
            assert bool((Y > 0).any()) and (epi == RELU or bool((Y < 0).any()))
        dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
        clamped = (0,) if (epi == L2NORM and not with_bias) else ()           # the empty row without a bias: norm 0, G = dY / 1e-12
        G, _ = check_prep(dY, Y, norm, epi, clamped=clamped)
        if width == 64:                                         # the transposed aggregation, here without long rows
            from ctgcn_amd import ops
            if clamped:
                G = G.clone()
                G[0] = 0                                        # column 0 is empty, but 0 * 1e12-sized values would swamp the tolerance's scale
            dS, _ = ops._gcn_conv_fwd(adj.transposed(), G, None, NONE)
            close_scaled(f64(dS), m.T @ f64(G))


@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
@pytest.mark.parametrize("d", [1, 10, 24, 130, 132, 260])
def test_pre_pass_over_several_blocks(d, epi):
    """199 rows: three full pre-pass blocks and one of 7 rows; 260 columns: two passes of the 64 float4 lanes"""
    rng = np.random.default_rng(d)
    dY = torch.from_numpy(dense((N2, d), d + 3)).to(DEV)
    y = dense((N2, d), d + 4)
    y[rng.random((N2, d)) < 0.3] = 0.0                        # dropped or non-positive entries
    norm = rng.uniform(0.2, 3.0, N2).astype(np.float32)
    Y, nrm = torch.from_numpy(y).to(DEV), torch.from_numpy(norm).to(DEV)
    for p in ((0.0, 0.5, 0.1) if epi == RELU else (0.0,)):
        check_prep(dY, Y, nrm if epi == L2NORM else None, epi, p)
    if epi == L2NORM:
        norm[[0, 64, 198]] = [0.0, 5e-13, 9.9e-13]             # below the clamp, in three different blocks
        check_prep(dY, Y, torch.from_numpy(norm).to(DEV), epi, clamped=(0, 64, 198))


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("d", [10, 24, 130, 132])
def test_dropout_follows_the_host_model(d, p, long_threshold):
    from ctgcn_amd import ops
    m = graph(64)
    adj = gcn_adj(m, long_threshold)
    S = torch.from_numpy(dense((N, d), d)).to(DEV)
    bias = torch.from_numpy(dense((d,), d + 1)).to(DEV)
    pre = pre_activation(m, S, bias)
    tol = tolerance(pre)
    sure_pos, sure_neg = pre > tol, pre < -tol
    assert sure_pos.mean() > 0.3 and sure_neg.mean() > 0.3
    masks = []
    for key in (KEY, KEY + 1):
        Y, _ = ops._gcn_conv_fwd(adj, S, bias, RELU, p, key)
        y = f64(Y)
        keep = R.keep_mask(key, N, d, p)
        assert np.array_equal((y != 0)[sure_pos], keep[sure_pos]) and not y[sure_neg].any() and (y >= 0).all()
        want = np.where(keep & (pre > 0), pre / (1.0 - p), 0.0)
        sure = sure_pos | sure_neg
        close_scaled(y[sure], want[sure])
        assert np.all(np.abs(y[~sure]) <= 2 * tol[~sure] / (1.0 - p))
        assert torch.equal(Y, ops._gcn_conv_fwd(adj, S, bias, RELU, p, key)[0])
        masks.append((y != 0)[sure_pos])
    assert (masks[0] != masks[1]).mean() > 0.5 * 2 * p * (1 - p)            # two keys: independent masks differ in 2 p (1 - p) of the entries
    plain, _ = ops._gcn_conv_fwd(adj, S, bias, RELU)
    assert torch.equal(plain, ops._gcn_conv_fwd(adj, S, bias, RELU, 0.0, KEY)[0])
    # what the backward recovers from Y alone: kept and positive exactly where Y > 0
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
    check_prep(dY, Y, None, RELU, p)


@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
@pytest.mark.parametrize("d", DIMS)
def test_long_rows_of_a_directed_matrix_and_of_its_transpose(d, epi, with_bias):
    """long_threshold 8: rows of 9 entries and more go to the piece kernels, forward over the matrix and backward over its transpose"""
    from ctgcn_amd import ops
    m = directed_graph()
    adj = gcn_adj(m, long_threshold=8)
    adj_t = adj.transposed()
    rows, cols = np.diff(m.indptr), np.diff(m.T.tocsr().indptr)
    assert adj_t is not adj and adj_t.transposed() is adj and adj.transposed() is adj_t
    assert sorted(adj.long_rows.cpu().tolist()) == np.nonzero(rows > 8)[0].tolist() != []
    assert sorted(adj_t.long_rows.cpu().tolist()) == np.nonzero(cols > 8)[0].tolist() != []
    assert adj.long_rows.cpu().tolist() != adj_t.long_rows.cpu().tolist() and adj_t.long_threshold == 8
    assert abs(sp.csr_matrix(adj_t.to_sparse_tensor().cpu().to_dense().numpy().astype(np.float64)) - m.T).sum() == 0
    Y, norm, _ = check_forward(m, adj, d, epi, with_bias)
    short = torch.from_numpy(rows <= 8).to(DEV)
    assert torch.equal(Y[short], check_forward(m, gcn_adj(m), d, epi, with_bias)[0][short])
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV)
    G, _ = ops._gcn_conv_prep(dY, Y, norm, epi)
    if epi == L2NORM and not with_bias:
        G = G.clone()
        G[torch.from_numpy(rows == 0).to(DEV)] = 0            # the clamped rows (test above) would swamp the tolerance's scale
    dS, _ = ops._gcn_conv_fwd(adj_t, G, None, NONE)
    close_scaled(f64(dS), m.T @ f64(G))
    assert torch.equal(dS, ops._gcn_conv_fwd(adj_t, G, None, NONE)[0])


def test_a_symmetric_matrix_is_its_own_transpose():
    from ctgcn_amd import ops
    m = symmetric_graph(16)
    assert ops.GcnAdj.from_scipy(m, DEV, check_symmetric=True).transposed().symmetric
    adj = ops.GcnAdj.from_scipy(m, DEV, check_symmetric=True)
    assert adj.transposed() is adj
    with pytest.raises(ValueError, match="symmetric"):
        ops.GcnAdj.from_scipy(graph(16), DEV, check_symmetric=True)


@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
def test_padded_rows_at_an_unaligned_base_take_the_scalar_path(epi):
    d, ld = 24, 27

    def strided(seed):
        buf = torch.zeros(N * ld + 1, device=DEV)
        view = buf[1:].as_strided((N, d), (ld, 1))
        view.copy_(torch.from_numpy(dense((N, d), seed)))
        assert view.data_ptr() % 16 == 4
        return view

    for long_threshold in (None, 8):
        m = directed_graph()
        adj = gcn_adj(m, long_threshold)
        out = strided(6)
        Y, norm, _ = check_forward(m, adj, d, epi, True, S=strided(5), out=out)
        assert Y is out
        aligned, _, _ = check_forward(m, adj, d, epi, True, S=strided(5).contiguous())
        close_scaled(f64(Y), f64(aligned))
        check_prep(strided(7), Y, norm, epi)


def test_out_writes_one_slot_of_a_sequence_buffer():
    from ctgcn_amd import ops
    m = graph(32)
    adj = gcn_adj(m)
    for d in (24, 27):
        S = torch.from_numpy(dense((N, d), 3)).to(DEV)
        bias = torch.from_numpy(dense((d,), 4)).to(DEV)
        want = ops.gcn_conv(S, adj, bias, ops.GCN_EPI_L2NORM)
        buf = torch.full((N, 3, d), 7.0, device=DEV)
        got = ops.gcn_conv(S, adj, bias, ops.GCN_EPI_L2NORM, out=buf[:, 1, :])
        assert got.data_ptr() == buf[:, 1, :].data_ptr() and torch.equal(buf[:, 1, :], want)
        assert bool((buf[:, 0, :] == 7.0).all()) and bool((buf[:, 2, :] == 7.0).all())
    with pytest.raises(RuntimeError, match="inference"):
        ops.gcn_conv(S.clone().requires_grad_(), adj, bias, out=buf[:, 1, :])
    with pytest.raises(ValueError):
        ops.gcn_conv(S, adj, bias, out=buf[:, :, 0])
    with pytest.raises(ValueError):
        ops.gcn_conv(S[:-1], adj)
    with pytest.raises(ValueError):
        ops.gcn_conv(S, adj, epi=3)
    with pytest.raises(ValueError):
        ops.gcn_conv(S, adj, epi=ops.GCN_EPI_RELU, p=1.0)
    with pytest.raises(ValueError):
        ops.gcn_conv(S, adj, bias[:-1])
    with pytest.raises(TypeError):
        ops.gcn_conv(S.double(), adj)


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("epi,p", [(NONE, 0.0), (RELU, 0.0), (RELU, 0.5), (L2NORM, 0.0)], ids=["none", "relu", "dropout", "l2norm"])
def test_autograd_function_matches_stock_autograd(epi, p, long_threshold):
    from ctgcn_amd import ops
    from torch.nn import functional as F
    m = directed_graph()
    adj = gcn_adj(m, long_threshold)
    d = 24
    S = torch.from_numpy(dense((N, d), 11)).to(DEV).requires_grad_()
    b = torch.from_numpy(dense((d,), 12)).to(DEV).requires_grad_()
    C = torch.from_numpy(dense((N, d), 13)).to(DEV)
    Y = ops.gcn_conv(S, adj, b, epi, p, KEY)
    (Y * C).sum().backward()
    S64, b64 = S.detach().cpu().double().requires_grad_(), b.detach().cpu().double().requires_grad_()
    pre = torch.sparse.mm(E.sparse_tensor(m, torch.float64), S64) + b64
    if epi == RELU:
        keep = (Y.detach().cpu() > 0).double()                  # the dropout mask, recovered from the output
        Y64 = F.relu(pre) * keep / (1.0 - p)
        if p > 0:
            sure = f64(pre) > tolerance(f64(pre))
            assert np.array_equal(keep.numpy().astype(bool)[sure], R.keep_mask(KEY, N, d, p)[sure])
    elif epi == L2NORM:
        Y64 = F.normalize(pre, p=2)
    else:
        Y64 = pre
    (Y64 * C.cpu().double()).sum().backward()
    close_scaled(f64(Y), Y64.detach().numpy())
    close_scaled(f64(S.grad), S64.grad.numpy())
    close_scaled(f64(b.grad), b64.grad.numpy())
    # only the gradients that are asked for
    S2 = S.detach().clone().requires_grad_()
    (ops.gcn_conv(S2, adj, b.detach(), epi, p, KEY) * C).sum().backward()
    assert torch.equal(S2.grad, S.grad)
    b2 = b.detach().clone().requires_grad_()
    (ops.gcn_conv(S.detach(), adj, b2, epi, p, KEY) * C).sum().backward()
    assert torch.equal(b2.grad, b.grad)
    S3 = S.detach().clone().requires_grad_()
    (ops.gcn_conv(S3, adj, None, NONE) * C).sum().backward()     # no bias, no epilogue: dS = Â^T C
    close_scaled(f64(S3.grad), m.T @ f64(C))
