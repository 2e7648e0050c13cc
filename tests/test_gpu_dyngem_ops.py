"""ops.rowsel_conv and ops.wrecon_loss (ctgcn_dyngem.hip) on the GPU against the float64 mirror (tests/_dyngem_ref.py: the dense
definition, dense adjacency rows and the reference's penalty expression), at every size at which the kernels take another path.

The rule is the project's for fp32 kernels: the same dense expression in stock fp32 torch ops on the same GPU is measured against the
float64 mirror too, and the kernel may use max(4 x that error, 2e-6) of the largest reference magnitude for outputs and losses, with
a 1e-5 floor for gradients.

Gather: widths on both sides of every lane-width boundary of launch_rows (chunk counts 4/5, 8/9, 16/17, 32/33) in the float4 form, and
in the scalar form both by a width that is no multiple of 4 and by a misaligned view; 1 and 3 rows per position; duplicates, -1 and an
all -1 position, empty CSR rows, 70 positions (more than one block at every lane width).  Long positions with a small long_threshold (the
smallest from 4 up that has a position exactly on it and one just over it): the first is not long, the second is one piece, and the
longest position (45 entries and more) is cut into the maximum number of pieces.
Loss: N around the 4-wide quads and the 256-thread sweep (1, 3, 4, 255, 256, 257, 1030); ldz > N; ReLU on and off; divisor on and off;
beta 1; a row with no stored entry, one with every entry stored, a stored zero, tgt -1; dZ aliasing Z; B = 1; the loss under no_grad
against the loss of the gradient call, bit for bit."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _dyngem_ref as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N_G, T_G, B_G = 97, 3, 70
_cache = {}


def window(n=N_G, T=T_G, seed=0):
    """row v of snapshot t stores (7 v + 3 t) mod 12 entries (so some rows are empty), row 2 of snapshot 0 stores 45; weights in [0.5, 2)"""
    key = ("window", n, T, seed)
    if key not in _cache:
        rng = np.random.default_rng(seed)
        mats = []
        for t in range(T):
            r, c, w = [], [], []
            for v in range(n):
                k = 45 if (t == 0 and v == 2) else (7 * v + 3 * t) % 12
                cols = rng.choice(n, size=min(k, n), replace=False)
                r += [v] * len(cols)
                c += cols.tolist()
                w += (rng.random(len(cols)) * 1.5 + 0.5).tolist()
            mats.append(sp.csr_matrix((np.asarray(w), (np.asarray(r), np.asarray(c))), shape=(n, n)))
        _cache[key] = mats
    return _cache[key]


def rows_of(mats, long_threshold=None):
    from ctgcn_amd import ops
    key = ("rows", id(mats), long_threshold)
    if key not in _cache:
        _cache[key] = ops.SnapshotRows(mats, DEV, long_threshold=long_threshold)
    return _cache[key]


def positions(L, B=B_G, n=N_G, T=T_G):
    """[B, L] stacked row ids: slot s reads snapshot s; with duplicates, single -1 entries and an all -1 position"""
    rng = np.random.default_rng(100 + L)
    node = rng.integers(0, n, size=B)
    node[:3] = 2                                                      # the longest row, three times
    node[3:6] = node[6:9]                                             # more duplicates
    idx = np.stack([(s % T) * n + node for s in range(L)], axis=1).astype(np.int64)
    idx[10, 0] = -1
    idx[11, :] = -1
    if L > 1:
        idx[12, L - 1] = -1
    return idx[:B]


def dense_x(mats, idx):
    key = ("dense", id(mats), idx.tobytes(), idx.shape)
    if key not in _cache:
        _cache[key] = D.dense_rows(D.stacked(mats), idx, torch.float64)
    return _cache[key]


def operand(shape, seed, misaligned=False):
    """fp32 CUDA tensor; misaligned: a view whose base is 4 bytes past a 16-byte boundary"""
    gen = torch.Generator().manual_seed(seed)
    t = torch.randn(*shape, generator=gen) / np.sqrt(shape[-1])
    if not misaligned:
        return t.to(DEV)
    flat = torch.zeros(t.numel() + 1, device=DEV)
    view = flat[1:].view(*shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def gather_case(mats, idx, d, col_stride, relu, misaligned, long_threshold=None):
    """(kernel results, float64 mirror, stock fp32 on the GPU), each (Y, dS, dbias)"""
    from ctgcn_amd import ops
    rows = rows_of(mats, long_threshold)
    n, L = mats[0].shape[0], idx.shape[1]
    S0 = operand(((L - 1) * col_stride + n, d), 7 + d, misaligned)
    bias0 = operand((d,), 11 + d)
    C = operand((idx.shape[0], d), 13 + d)
    x64 = dense_x(mats, idx)

    def run(fn, S, bias, Cw):
        S, bias = S.detach().requires_grad_(True), bias.detach().requires_grad_(True)      # the same storage: a misaligned view stays one
        Y = fn(S, bias)
        gS, gb = torch.autograd.grad((Y * Cw).sum(), (S, bias))
        return Y.detach(), gS.detach(), gb.detach()

    def kernel(S, bias):
        return ops.rowsel_conv(S, rows, idx, bias, relu=relu, col_stride=col_stride)

    got = run(kernel, S0, bias0, C)
    again = run(kernel, S0, bias0, C)
    assert all(torch.equal(a, b) for a, b in zip(got, again))        # no atomics: a second call is bit-identical
    ref = run(lambda S, b: D.rowsel_conv(S, x64, b, relu, col_stride), S0.double().cpu(), bias0.double().cpu(), C.double().cpu())
    x32 = x64.float().to(DEV)
    yard = run(lambda S, b: D.rowsel_conv(S, x32, b, relu, col_stride), S0, bias0, C)
    return got, ref, yard, rows


def held(what, got, ref, yard, floors=(2e-6, 1e-5, 1e-5)):
    for name, g, r, y, floor in zip(("Y", "dS", "dbias"), got, ref, yard, floors):
        top = float(r.abs().max())
        assert top > 0, (what, name)
        err = float((g.double().cpu() - r).abs().max()) / top
        ye = float((y.double().cpu() - r).abs().max()) / top
        print("  [tol] %-34s %-5s kernel %.3e  stock fp32 %.3e  allowed %.3e" % (what, name, err, ye, max(4 * ye, floor)))
        assert err <= max(4 * ye, floor), (what, name, err, ye)


WIDTHS = [(16, False), (20, False), (32, False), (36, False), (64, False), (68, False), (128, False), (132, False),        # float4: chunks d / 4
          (5, False), (9, False), (17, False), (33, False),                                                               # scalar: chunks d
          (4, True), (8, True), (16, True), (32, True)]                                                                   # scalar by misalignment


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("d,misaligned", WIDTHS)
def test_gather_forward_and_backward_at_the_lane_width_boundaries(d, misaligned, L):
    mats = window()
    idx = positions(L)
    got, ref, yard, rows = gather_case(mats, idx, d, N_G if L > 1 else 0, relu=True, misaligned=misaligned)
    assert rows.select(idx).long_pos is None
    assert tuple(got[0].shape) == (B_G, d) and torch.equal(got[0][11], got[0][11].clamp(min=0))
    held("d%d%s L%d" % (d, " misaligned" if misaligned else "", L), got, ref, yard)


@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("d", [20, 7])
def test_gather_long_positions_and_pieces(d, L):
    mats = window()
    idx = positions(L)
    lens = rows_of(mats).select(idx).host_len
    # the smallest threshold from 4 up with a position exactly on it (not long) and one just over it (long, one piece)
    thr = next(c for c in range(4, 15) if (lens == c).any() and (lens == c + 1).any())
    rows = rows_of(mats, thr)
    sel = rows.select(idx)
    top = int(lens.max())                                             # row 2 of snapshot 0 and what the other slots add to it
    assert top >= 45 and sel.long_pos is not None and sel.pieces == -(-top // (4 * thr)) and sel.pieces >= 2
    assert set(sel.long_pos.tolist()) == set(np.nonzero(lens > thr)[0].tolist())
    got, ref, yard, _ = gather_case(mats, idx, d, N_G if L > 1 else 0, relu=False, misaligned=False, long_threshold=thr)
    held("long thr%d d%d L%d" % (thr, d, L), got, ref, yard)
    plain = gather_case(mats, idx, d, N_G if L > 1 else 0, relu=False, misaligned=False)[0]
    for a, b in zip(got, plain):                                      # pieces change the order of a long position's sum, nothing else
        assert float((a - b).abs().max()) <= 1e-5 * float(b.abs().max())


def test_gather_single_position_shared_block_and_refusals():
    from ctgcn_amd import ops
    mats = window()
    idx = np.array([[2]], dtype=np.int64)
    got, ref, yard, rows = gather_case(mats, idx, 12, 0, relu=True, misaligned=False)
    held("B1", got, ref, yard)
    # slots sharing one block of S (col_stride 0): the blocks' gradients add
    idx3 = positions(3)
    got, ref, yard, _ = gather_case(mats, idx3, 8, 0, relu=False, misaligned=False)
    held("col_stride 0 L3", got, ref, yard)
    S = torch.zeros(N_G, 8, device=DEV)
    with pytest.raises(ValueError, match="row id outside"):
        ops.rowsel_conv(S, rows, np.array([T_G * N_G]))
    with pytest.raises(ValueError, match="rows"):
        ops.rowsel_conv(S, rows, idx3, col_stride=N_G)               # S too short for three blocks
    with pytest.raises(TypeError):
        ops.rowsel_conv(S.double(), rows, idx)
    with pytest.raises(TypeError):
        ops.rowsel_conv(S, rows, np.array([0.5]))


def test_bucket_sums_and_the_transposed_stack():
    from ctgcn_amd import ops
    mats = window()
    rows = rows_of(mats)
    idx = positions(3)
    sel = rows.select(idx)
    G = operand((B_G, 20), 3)
    for s in range(3):
        got = ops._rowsel_bucket(sel, s, G)
        want = D.bucket(G.double().cpu(), idx[:, s], rows.rows)
        assert tuple(got.shape) == (T_G * N_G, 20)
        assert float((got.double().cpu() - want).abs().max()) <= 1e-6 * float(want.abs().max())
        assert torch.equal(got, ops._rowsel_bucket(sel, s, G))
    t = rows.transposed()
    stack = D.stacked(mats).tocsc()
    assert t.n == N_G and np.array_equal(t.row_ptr.cpu().numpy(), stack.indptr) and np.array_equal(t.col.cpu().numpy(), stack.indices)
    assert np.allclose(rows.row_sum.cpu().numpy(), np.asarray(D.stacked(mats).sum(axis=1)).reshape(-1), rtol=1e-7)
    dense = rows.dense(idx)
    assert torch.equal(dense.cpu(), dense_x(mats, idx).float())


# ------------------------------------------------------------------------------------------------ the loss
def loss_window(n):
    """2 snapshots of n nodes: row 0 stores every entry, row 1 none, row 2 a zero among its entries; the rest about 5 % full"""
    key = ("loss_window", n)
    if key not in _cache:
        rng = np.random.default_rng(n)
        mats = []
        for t in range(2):
            dense = (rng.random((n, n)) < 0.05) * (rng.integers(1, 4, size=(n, n)).astype(np.float64))
            if t == 0:
                dense[0, :] = rng.integers(1, 4, size=n)
                dense[1 % n, :] = 0 if n > 1 else dense[0, :]
            m = sp.csr_matrix(dense)
            if t == 0 and n > 2:                                      # a stored zero in row 2
                m = m.tolil()
                m[2, 0] = 7.0
                m = m.tocsr()
                m.data[m.indptr[2]] = 0.0
            mats.append(m)
        _cache[key] = mats
    return _cache[key]


def loss_case(n, relu, divide, beta, view, overwrite, tgt=None, scale=0.25):
    from ctgcn_amd import ops
    mats = loss_window(n)
    rows = rows_of(mats)
    if tgt is None:
        tgt = np.array([0, n, -1, 1 % n, 2 % n, n + (3 % n), 0, 2 % n, n + n - 1], dtype=np.int64)
        if divide:                                                    # a zero divisor gives inf / nan, as in the reference: not compared
            sums = np.asarray(D.stacked(mats).sum(axis=1)).reshape(-1)
            tgt = np.array([r for r in tgt if r >= 0 and sums[r] > 0], dtype=np.int64)
    B = len(tgt)
    Z0 = operand((B, n), 50 + n)
    x64 = D.dense_rows(D.stacked(mats), tgt, torch.float64)[:, 0]
    div64 = x64.sum(1) if divide else None

    def reference(dtype, device):
        z = Z0.to(device=device, dtype=dtype).requires_grad_(True)
        x = x64.to(device=device, dtype=dtype)
        loss = D.wrecon_loss(z, x, beta, None if div64 is None else div64.to(device=device, dtype=dtype), scale, relu)
        g, = torch.autograd.grad(loss, z)
        return float(loss.detach()), g.detach().double().cpu()

    def buffer():
        if view:                                                      # rows of a wider buffer: ldz = n + 4 > n
            z = torch.zeros(B, n + 4, device=DEV)[:, :n]
            z.copy_(Z0)
            return z
        return Z0.clone()

    with torch.no_grad():
        alone = ops.wrecon_loss(buffer(), rows, tgt, beta, divide=divide, scale=scale, relu=relu)
    z = buffer().requires_grad_(True)
    loss = ops.wrecon_loss(z, rows, tgt, beta, divide=divide, scale=scale, relu=relu, overwrite=overwrite)
    grad = torch.autograd.grad(loss, z)[0].detach()
    # dZ took Z's memory, or Z is as it was
    assert torch.equal(z.detach(), grad) if overwrite else torch.equal(z.detach(), Z0)
    assert loss.dtype == torch.float32 and loss.dim() == 0 and torch.equal(loss.detach(), alone)        # bit for bit
    ref_loss, ref_grad = reference(torch.float64, "cpu")
    yard_loss, yard_grad = reference(torch.float32, DEV)
    what = "n%d relu%d div%d beta%g view%d alias%d B%d" % (n, relu, divide, beta, view, overwrite, B)
    err_l, yl = abs(float(loss.detach()) - ref_loss) / abs(ref_loss), abs(yard_loss - ref_loss) / abs(ref_loss)
    top = float(ref_grad.abs().max())
    err_g, yg = float((grad.double().cpu() - ref_grad).abs().max()) / top, float((yard_grad - ref_grad).abs().max()) / top
    print("  [tol] %-44s loss %.3e (stock %.3e, allowed %.3e)  grad %.3e (stock %.3e, allowed %.3e)"
          % (what, err_l, yl, max(4 * yl, 2e-6), err_g, yg, max(4 * yg, 1e-5)))
    assert err_l <= max(4 * yl, 2e-6) and err_g <= max(4 * yg, 1e-5), what
    return grad, ref_grad


COMBOS = [(True, False, 5.0, False, False), (False, True, 1.0, True, False), (True, True, 3.0, False, True), (False, False, 2.0, True, True)]


@pytest.mark.parametrize("relu,divide,beta,view,overwrite", COMBOS, ids=["relu", "div-beta1-view", "relu-div-alias", "view-alias"])
@pytest.mark.parametrize("n", [1, 3, 4, 255, 256, 257, 1030])
def test_wrecon_loss_and_gradient(n, relu, divide, beta, view, overwrite):
    grad, ref_grad = loss_case(n, relu, divide, beta, view, overwrite)
    if relu:                                                          # the gradient is exactly zero where the ReLU was inactive
        assert torch.equal(grad.cpu() == 0, ref_grad == 0)


def test_wrecon_loss_single_row_empty_targets_and_refusals():
    from ctgcn_amd import ops
    loss_case(257, True, True, 4.0, False, False, tgt=np.array([0], dtype=np.int64))          # B = 1, every entry stored
    loss_case(257, True, False, 4.0, False, True, tgt=np.array([-1], dtype=np.int64))         # B = 1, no target row at all
    loss_case(256, False, False, 4.0, True, False, tgt=np.array([1, -1, 1, 257], dtype=np.int64))      # only rows without entries
    rows = rows_of(loss_window(256))
    with torch.no_grad():
        nan = ops.wrecon_loss(torch.ones(2, 256, device=DEV), rows, np.array([1, 0]), 2.0, divide=True)   # row 1 sums to 0
    assert not bool(torch.isfinite(nan))
    with pytest.raises(ValueError, match="Z must be"):
        ops.wrecon_loss(torch.ones(2, 255, device=DEV), rows, np.array([1, 0]), 2.0)
    with pytest.raises(ValueError, match="one target row"):
        ops.wrecon_loss(torch.ones(2, 256, device=DEV), rows, np.array([[1, 0], [0, 1]]), 2.0)
    with pytest.raises(TypeError):
        ops.wrecon_loss(torch.ones(2, 256, device=DEV).double(), rows, np.array([1, 0]), 2.0)
