"""Kernels of ctgcn_gcn.hip against float64 scipy: the fused GCN step forward and backward at every dispatch boundary (scalar and
float4 rows, every lane-group width, rows around each width, long rows in one and in several pieces), and the normalisation against
the reference's recorded values."""
import json
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _egcn_ref as E
from _gcn_graphs import DEV, DIMS, N, WIDTHS, dense, gcn_adj, symmetric_graph
from conftest import close_scaled

pytestmark = pytest.mark.gpu
SLOPE = np.float32((1.0 / 8.0 + 1.0 / 3.0) / 2.0).astype(np.float64)


def graph(width):
    """the symmetric graph of that width with float32 values: the layer takes it as it is"""
    return symmetric_graph(width, float32_values=True)


def act_of(pre, act):
    return np.where(pre >= 0, pre, pre * SLOPE) if act else pre


def check_forward(m, adj, d, act, score, S=None):
    from ctgcn_amd import ops
    S = torch.from_numpy(dense((N, d), d)).to(DEV) if S is None else S
    p = torch.from_numpy(dense((d,), d + 1)).to(DEV) if score else None
    Y, sc = ops._gcn_fwd(adj, S, act, p)
    ref = act_of(m @ S.cpu().numpy().astype(np.float64), act)
    close_scaled(Y.cpu().numpy(), ref)
    assert (sc is None) == (not score)
    if score:
        close_scaled(sc.cpu().numpy(), ref @ p.cpu().numpy().astype(np.float64))
    Y2, sc2 = ops._gcn_fwd(adj, S, act, p)
    assert torch.equal(Y, Y2) and (sc is None or torch.equal(sc, sc2))
    return Y


def check_backward(m, adj, d, act, Y, dY=None):
    from ctgcn_amd import ops
    dY = torch.from_numpy(dense((N, d), d + 2)).to(DEV) if dY is None else dY
    dS = ops._gcn_bwd(adj, dY, Y if act else None, act)
    y = Y.cpu().numpy().astype(np.float64)
    g = dY.cpu().numpy().astype(np.float64) * (np.where(y > 0, 1.0, SLOPE) if act else 1.0)
    close_scaled(dS.cpu().numpy(), m.T @ g)
    assert torch.equal(dS, ops._gcn_bwd(adj, dY, Y if act else None, act))


@pytest.mark.parametrize("score", [False, True], ids=["plain", "score"])
@pytest.mark.parametrize("act", [0, 1], ids=["identity", "rrelu"])
@pytest.mark.parametrize("d", DIMS)
def test_layer_at_every_lane_group_width(d, act, score):
    for width in WIDTHS:
        m = graph(width)
        adj = gcn_adj(m)
        assert adj.long_rows is None
        Y = check_forward(m, adj, d, act, score)
        assert float(Y[0].abs().max()) == 0                      # the empty row: exactly 0, and the slope in the backward
        if d > 1:
            assert bool((Y > 0).any()) and bool((Y < 0).any())
        if not score:
            check_backward(m, adj, d, act, Y)


@pytest.mark.parametrize("score", [False, True], ids=["plain", "score"])
@pytest.mark.parametrize("act", [0, 1], ids=["identity", "rrelu"])
@pytest.mark.parametrize("d", DIMS)
def test_long_rows_in_pieces(d, act, score):
    """long_threshold 8: rows of 8 entries stay with their lane group, rows of 9 go to the piece kernels (one piece up to 32 entries);
    the row of 65 entries is cut into three pieces, those of 63 and 64 into two"""
    m = graph(64)
    adj = gcn_adj(m, long_threshold=8)
    lens = np.diff(m.indptr)
    assert sorted(adj.long_rows.cpu().tolist()) == sorted(np.nonzero(lens > 8)[0].tolist()) and 5 not in adj.long_rows.cpu().tolist()
    assert lens[4] == 65 and adj.pieces == 3
    Y = check_forward(m, adj, d, act, score)
    short = torch.from_numpy(lens <= 8).to(DEV)
    assert torch.equal(Y[short], check_forward(m, gcn_adj(m), d, act, score)[short])
    if not score:
        check_backward(m, adj, d, act, Y)


def test_fewer_pieces_than_a_row_asks_for():
    """a workspace of one piece per row: the pieces grow, the sums stay right"""
    from ctgcn_amd import ops
    m = graph(64)
    adj = gcn_adj(m, long_threshold=8)
    adj.pieces = 1
    check_backward(m, adj, 24, 1, check_forward(m, adj, 24, 1, True))


@pytest.mark.parametrize("act", [0, 1], ids=["identity", "rrelu"])
def test_padded_rows_at_an_unaligned_base_take_the_scalar_path(act):
    d, ld = 24, 27

    def strided(seed):
        buf = torch.zeros(N * ld + 1, device=DEV)
        view = buf[1:].as_strided((N, d), (ld, 1))
        view.copy_(torch.from_numpy(dense((N, d), seed)))
        assert view.data_ptr() % 16 == 4
        return view

    for long_threshold in (None, 8):
        m = graph(64)
        adj = gcn_adj(m, long_threshold)
        Y = check_forward(m, adj, d, act, True, S=strided(5))
        Ypad = strided(6)
        Ypad.copy_(Y)
        check_backward(m, adj, d, act, Ypad, dY=strided(7))


@pytest.mark.parametrize("score", [False, True], ids=["plain", "score"])
@pytest.mark.parametrize("long_threshold", [None, 8])
def test_autograd_function_matches_stock_autograd(long_threshold, score):
    from ctgcn_amd import ops
    from torch.nn import functional as F
    m = graph(64)
    adj = gcn_adj(m, long_threshold)
    d = 24
    S = torch.from_numpy(dense((N, d), 11)).to(DEV).requires_grad_()
    C = torch.from_numpy(dense((N, d), 12)).to(DEV)
    p = torch.from_numpy(dense((d,), 13)).to(DEV) if score else None
    res = ops.gcn_layer(S, adj, 1, p)
    Y = res[0] if score else res
    assert (not score) or (not res[1].requires_grad)
    (Y * C).sum().backward()
    S64 = S.detach().cpu().double().requires_grad_()
    Y64 = F.rrelu(torch.sparse.mm(E.sparse_tensor(m, torch.float64), S64))
    (Y64 * C.cpu().double()).sum().backward()
    close_scaled(Y.detach().cpu().numpy(), Y64.detach().numpy())
    close_scaled(S.grad.cpu().numpy(), S64.grad.numpy())
    if score:
        close_scaled(res[1].cpu().numpy(), (Y64.detach() @ p.cpu().double()).numpy())
    with pytest.raises(ValueError):
        ops.gcn_layer(S[:-1], adj, 1)
    with pytest.raises(ValueError):
        ops.gcn_layer(S, adj, 2)


# ------------------------------------------------------------------------------------------------ normalisation
@pytest.mark.parametrize("row_norm", [False, True], ids=["sym", "row"])
def test_normalisation_matches_the_reference_within_one_ulp(row_norm):
    from ctgcn_amd import ops
    g = E.fixture()
    shares = []
    for t in range(E.T):
        m = E.snapshot_csr(t)
        adj = gcn_adj(m)
        got = ops.gcn_normalize(adj.row_ptr, adj.col, adj.val, row_norm).cpu().numpy()
        ref = g["norm%d_t%d" % (int(row_norm), t)]
        assert got.dtype == ref.dtype == np.float32 and got.shape == ref.shape
        print("  snapshot %d row_norm %d: %.4f of %d values bit-identical" % (t, row_norm, float((got == ref).mean()), ref.size))
        shares.append({"snapshot": t, "values": int(ref.size), "bit_identical": int((got == ref).sum())})
        assert np.all(np.abs(got.astype(np.float64) - ref.astype(np.float64)) <= np.spacing(np.abs(ref)).astype(np.float64))
    out_dir = os.environ.get("CTGCN_PARITY_OUT")             # a measuring run keeps the shares (profiles/egcn_parity_errors.json)
    if out_dir:
        with open(os.path.join(out_dir, "egcn_norm_bits_row_norm%d.json" % int(row_norm)), "w") as fp:
            json.dump(shares, fp)


def test_normalisation_of_a_zero_row_and_of_a_negative_row_sum():
    from ctgcn_amd import ops
    m = sp.csr_matrix(np.array([[2.0, 1.0, 0, 0], [1.0, 1.0, 0, 2.0], [0, 0, 0, 0], [0, 2.0, 0, 2.0]]))
    adj = gcn_adj(m)
    for row_norm in (False, True):
        got = ops.gcn_normalize(adj.row_ptr, adj.col, adj.val, row_norm).cpu().numpy()
        r = np.array([3.0, 4.0, 1.0, 4.0]) ** (-1.0 if row_norm else -0.5)
        ref = (sp.diags(r) @ m @ (sp.identity(4) if row_norm else sp.diags(r))).tocsr()
        ref.sort_indices()
        want = ref.data.astype(np.float32)
        assert np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(np.abs(want)).astype(np.float64))
    cancel = sp.csr_matrix(np.array([[1.0, -1.0], [-1.0, 3.0]]))          # a stored row whose sum is zero scales to zeros
    a = gcn_adj(cancel)
    got = ops.gcn_normalize(a.row_ptr, a.col, a.val, False).cpu().numpy()
    assert np.array_equal(got[:3], np.zeros(3, np.float32)) and got[3] == np.float32(1.5)
    neg = gcn_adj(sp.csr_matrix(np.array([[1.0, -3.0], [-3.0, 5.0]])))
    for row_norm in (False, True):
        with pytest.raises(ValueError, match="negative"):
            ops.gcn_normalize(neg.row_ptr, neg.col, neg.val, row_norm)
