"""The fp64 TIMERS kernels (ctgcn_timers.hip) against the numpy mirror of tests/_timers_ref.py at their dispatch boundaries, ops.sym_topk
on the golden matrices, and TRIP / Obj / RefineBound fed the golden's inputs.

Boundaries, from the tile sizes in ctgcn_timers.hip:
  spmm      a row takes LPR lanes with 4 LPR >= b, LPR in {1, 2, 4, 8, 16, 32, 64}: b = 4|5, 8|9, 16|17, 32|33, 64|65, 128|129; past
            256 columns a second walk of the row: 256|257.  256 / LPR rows a block: n = 63, 64, 65 and 300 cross blocks for every LPR.
  tsgemm    64 x 64 output tiles (widths 64|65), LDS stages of 16 rows (n = 15, 16, 17) or 16 columns of X (b1 = 15, 16, 17); tsgemm_tn
            takes one run up to 512 rows and partials above (n = 512|513, 1100: three runs); tsgemm_nn has 64-row blocks (n = 255,
            257: partial last block) and sums one column partial per block.
  obj       LPR = the power of two >= min(k, 64) lanes a row: k = 1, 4, 16|17, 64|70 (70: a second lap of the lanes); 256 / LPR row
            groups a block and 4 rows a group before a second block: n = 300 gives more than one block for every k.

Tolerance of every sum: m·2⁻⁵³·Σ|terms| with m the number of summed terms, computed from the inputs: the worst case of any summation
order.  Nothing is measured.  The kernels' sums are compared with the same sums in extended precision (numpy longdouble, whose own
rounding of 2⁻⁶⁴ a term is far inside that), the passes fed the golden's inputs with the reference's fp64 results at twice the bound
(both sides carry it)."""
import importlib

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _timers_ref as T
from conftest import load_golden
from ctgcn_amd import ops

pytestmark = pytest.mark.gpu
TM = importlib.import_module("ctgcn_amd.baseline.timers")
DEV = "cuda"
LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def csr_dev(A):
    A = sp.csr_matrix(A)
    return dev(A.indptr.astype(np.int32)), dev(A.indices.astype(np.int32)), dev(A.data.astype(np.float64))


def graph(n, seed, long_row=True):
    """n x n CSR with about 6 entries a row, row 0 empty when n > 1, and with long_row and n >= 300 a row of more than 256 entries"""
    rng = np.random.RandomState(seed)
    A = sp.random(n, n, density=min(1.0, 6.0 / n), random_state=rng, data_rvs=lambda k: rng.randn(k)).tolil()
    if n > 1:
        A[0, :] = 0
    if long_row and n >= 300:
        A[5, :280] = rng.randn(280)
    A = A.tocsr()
    A.eliminate_zeros()
    return A


@pytest.fixture(scope="module")
def gold():
    return load_golden("timers_synth.npz")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_spmm_f64_boundaries(n):
    A = graph(n, n)
    if n == 300:
        assert np.diff(A.indptr).max() > 256 and np.diff(A.indptr).min() == 0
    rp, col, val = csr_dev(A)
    Al = A.toarray().astype(LD)
    rng = np.random.RandomState(n + 1)
    for b in (1, 3, 4, 5, 8, 9, 16, 17, 32, 33, 40, 64, 65, 72, 128, 129, 256, 257):
        for pad in (0, 3):                                    # ld > b: column slices of wider buffers
            X, Y0 = rng.randn(n, b + pad), rng.randn(n, b + pad)
            ref = Al @ X[:, :b].astype(LD)
            mag, m = abs(A) @ np.abs(X[:, :b]), np.diff(A.indptr)[:, None]
            bound = (m + 1) * T.U53 * (mag + np.abs(Y0[:, :b]))          # accumulate: one more term
            Xd = dev(X)
            got = ops.spmm_csr_f64(rp, col, val, Xd[:, :b])
            assert (np.abs(got.cpu().numpy() - ref) <= m * T.U53 * mag).all(), (n, b, pad)
            buf = dev(Y0)
            out = ops.spmm_csr_f64(rp, col, val, Xd[:, :b], out=buf[:, :b], accumulate=True)
            assert out.data_ptr() == buf.data_ptr()
            assert (np.abs(buf.cpu().numpy()[:, :b] - (Y0[:, :b].astype(LD) + ref)) <= bound).all(), (n, b, pad, "accumulate")
            assert (buf.cpu().numpy()[:, b:] == Y0[:, b:]).all()              # nothing past the block's columns
            again = ops.spmm_csr_f64(rp, col, val, Xd[:, :b])
            assert torch.equal(got, again)
            ops.spmm_csr_f64(rp, col, val, Xd[:, :b], out=buf[:, :b])          # plain store over old contents
            assert torch.equal(buf[:, :b], got)


WIDTHS = [(1, 1), (4, 15), (15, 4), (16, 17), (17, 16), (40, 72), (72, 40), (64, 65), (1, 72)]


@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 255, 257, 512, 513, 1100])
def test_tsgemm_tn_boundaries(n):
    rng = np.random.RandomState(n)
    for b1, b2 in WIDTHS:
        X, Y = rng.randn(n, b1 + 2), rng.randn(n, b2 + 1)
        Xd, Yd = dev(X)[:, :b1], dev(Y)[:, 1:]
        got = ops.tsgemm_tn(Xd, Yd)
        ref = X[:, :b1].T.astype(LD) @ Y[:, 1:].astype(LD)
        bound = n * T.U53 * (np.abs(X[:, :b1]).T @ np.abs(Y[:, 1:]))
        assert got.shape == (b1, b2) and (np.abs(got.cpu().numpy() - ref) <= bound).all(), (n, b1, b2)
        assert torch.equal(got, ops.tsgemm_tn(Xd, Yd))
    X = dev(rng.randn(n, 40))
    G = ops.tsgemm_tn(X, X).cpu().numpy()                      # the Gram of one block with itself
    assert (G == G.T).all()


@pytest.mark.parametrize("n", [1, 3, 15, 16, 17, 255, 257, 513, 1100])
def test_tsgemm_nn_boundaries(n):
    rng = np.random.RandomState(n + 7)
    for b1, b2 in WIDTHS + [(144, 32)]:
        X, C = rng.randn(n, b1 + 2), rng.randn(b1, b2 + 3)
        Xd, Cd = dev(X)[:, 2:], dev(C)[:, :b2]
        Xh, Ch = X[:, 2:], C[:, :b2]
        ref = Xh.astype(LD) @ Ch.astype(LD)
        mag = np.abs(Xh) @ np.abs(Ch)
        buf = torch.full((n, b2 + 2), 7.0, dtype=torch.float64, device=DEV)
        got, sq = ops.tsgemm_nn(Xd, Cd, out=buf[:, :b2], colsq=True)
        assert (np.abs(got.cpu().numpy() - ref) <= b1 * T.U53 * mag).all(), (n, b1, b2)
        assert (buf[:, b2:] == 7.0).all()
        # Σ_r y²: each y within b1·2⁻⁵³ of its terms' magnitude, squared and summed over n rows
        assert (np.abs(sq.cpu().numpy() - (ref * ref).sum(axis=0)) <= (n + 2 * b1 + 2) * T.U53 * (mag * mag).sum(axis=0)).all(), (n, b1, b2)
        plain = ops.tsgemm_nn(Xd, Cd)
        got2, sq2 = ops.tsgemm_nn(Xd, Cd, colsq=True)
        assert torch.equal(plain, got2) and torch.equal(got2, got) and torch.equal(sq, sq2)


@pytest.mark.parametrize("k", [1, 4, 16, 17, 64, 70])
def test_timers_obj_boundaries(k):
    rng = np.random.RandomState(k)
    for n, A in ((300, graph(300, 11)), (1, sp.csr_matrix(np.array([[2.5]]))), (65, sp.csr_matrix((65, 65))), (64, graph(64, 5))):
        rp, col, val = csr_dev(A)
        U, V = rng.randn(n, k + 1), rng.randn(n, k + 2)
        Uh, Vh = U[:, :k], V[:, 2:]
        Ud, Vd = dev(U)[:, :k], dev(V)[:, 2:]
        old = rng.randn(A.nnz)
        for s_old in (None, old):
            got = ops.timers_obj(rp, col, val, Ud, Vd, s_old=None if s_old is None else dev(s_old))
            ref = T.obj_sums(sp.csr_matrix(A).astype(LD), Uh.astype(LD), Vh.astype(LD), None if s_old is None else s_old.astype(LD), as_float=False)
            bound = T.obj_bound(A, Uh, Vh, s_old)
            g = got.cpu().numpy()
            assert abs(g[0] - ref[0]) <= bound[0] and abs(g[1] - ref[1]) <= bound[1], (k, n, s_old is None, g, ref, bound)
            if A.nnz == 0:
                assert g[0] == 0.0 and g[1] == 0.0
            assert torch.equal(got, ops.timers_obj(rp, col, val, Ud, Vd, s_old=None if s_old is None else dev(s_old)))


def _residuals(A, w, X):
    return np.linalg.norm(A @ X - X * w, axis=0)


def test_sym_topk_on_the_golden_matrices(gold):
    n, K = int(gold["n"]), int(gold["K"])
    snaps = [T.get_csr(gold, "snap%d" % i) for i in range(2)]
    A = TM.DeviceCsr(snaps[0], DEV)
    w, X = ops.sym_topk(A.matmul, n, K, tol=T.TOL)
    its = ops.sym_topk.last[0]
    w2, X2 = ops.sym_topk(A.matmul, n, K, tol=T.TOL)
    assert torch.equal(w, w2) and torch.equal(X, X2) and ops.sym_topk.last[0] == its          # same seed, same start block, same run
    w3, _ = ops.sym_topk(A.matmul, n, K, tol=T.TOL, seed=5)
    w, X = w.cpu().numpy(), X.cpu().numpy()
    w1 = abs(w[0])
    assert (np.abs(w)[:-1] >= np.abs(w)[1:]).all()
    sigma = gold["u_sigma"][0][::-1]
    # a symmetric operator's eigenvalue error is bounded by the residual norm; plus the reference's own spread
    assert (np.abs(np.abs(w) - sigma) <= T.TOL * w1 + float(gold["spread_sigma"])).all()
    assert (np.abs(w3.cpu().numpy() - w) <= 2 * T.TOL * w1).all()
    # the residuals, recomputed in numpy (whose own rounding is n·2⁻⁵³·|w1|)
    assert (_residuals(snaps[0], w, X) <= T.TOL * w1 + n * T.U53 * w1).all()
    assert np.abs(X.T @ X - np.eye(K)).max() <= 64 * n * T.U53
    # the bound operator of step 1 at 2 K pairs
    d = T.delta(snaps[0], snaps[1])
    apply, trace_change = TM.bound_operator(snaps[0], d, DEV)
    assert trace_change == gold["u_trace_change"][1]
    wb, Xb = ops.sym_topk(apply, n, 2 * K, tol=T.TOL, _deficient_ok=True)
    wb, Xb = wb.cpu().numpy(), Xb.cpu().numpy()
    M = T.bound_dense(snaps[0], d)
    wb1 = abs(wb[0])
    assert (_residuals(M, wb, Xb) <= T.TOL * wb1 + n * T.U53 * wb1).all()
    kept = np.sort(wb[wb >= 0])[::-1]
    want = gold["u_kept1"]                                       # LAPACK on the dense operator: n·2⁻⁵³·|w1| of its own
    assert len(kept) == len(want) and (np.abs(kept - want) <= T.TOL * wb1 + n * T.U53 * wb1).all()
    print("  sym_topk iterations: adjacency %d, bound operator %d" % (its, ops.sym_topk.last[0]))


def test_sym_topk_failure_modes_and_rank_deficiency():
    rng = np.random.RandomState(0)
    B = rng.randn(50, 5)
    M = dev(B @ B.T)
    apply = lambda q: ops.tsgemm_nn(M, q)                        # noqa: E731
    w, X = ops.sym_topk(apply, 50, 3)
    ev = np.linalg.eigvalsh(B @ B.T)[::-1]
    assert (np.abs(w.cpu().numpy() - ev[:3]) <= T.TOL * ev[0] + 50 * T.U53 * ev[0]).all()
    with pytest.raises(RuntimeError, match="rank 5"):
        ops.sym_topk(apply, 50, 8)
    w, X = ops.sym_topk(apply, 50, 8, _deficient_ok=True)
    assert (w[5:] == 0).all() and (X[:, 5:] == 0).all() and (np.abs(w.cpu().numpy()[:5] - ev[:5]) <= T.TOL * ev[0] + 50 * T.U53 * ev[0]).all()
    A = TM.DeviceCsr(graph(300, 2) + graph(300, 2).T, DEV)
    with pytest.raises(RuntimeError, match=r"residual \d\.\d+e[-+]\d+ after 3 iterations"):
        ops.sym_topk(A.matmul, 300, 8, max_iter=3)


def test_obj_trip_and_refinebound_on_the_golden_inputs(gold):
    n, K = int(gold["n"]), int(gold["K"])
    snaps = [T.get_csr(gold, "snap%d" % i) for i in range(T.STEPS + 1)]
    restart = gold["u_restart"]
    for i in range(T.STEPS + 1):
        U, s, V = gold["u_U%d" % i], gold["u_S%d" % i], gold["u_V%d" % i]
        Uc, Vc = U * np.sqrt(s), V * np.sqrt(s)
        got = TM.Obj(snaps[i], dev(Uc), dev(Vc))
        assert abs(got - gold["u_loss"][i]) <= 2 * T.obj_total_bound(snaps[i], Uc, Vc), i
        if i == 0:
            continue
        U0, s0, V0 = gold["u_U%d" % (i - 1)], gold["u_S%d" % (i - 1)], gold["u_V%d" % (i - 1)]
        d = T.delta(snaps[i - 1], snaps[i])
        nU, nS, nV = TM.TRIP(dev(U0), dev(s0), dev(V0), d)
        tag = "u_trip_" if restart[i] else "u_"
        cols, sv = T.trip_bound(U0, s0, V0, d)
        assert (np.abs(nU.cpu().numpy() - gold[tag + "U%d" % i]) <= 2 * cols).all(), i
        assert (np.abs(nV.cpu().numpy() - gold[tag + "V%d" % i]) <= 2 * cols).all(), i
        assert (np.abs(torch.diagonal(nS).cpu().numpy() - gold[tag + "S%d" % i]) <= 2 * sv).all(), i
        nU2, nS2, nV2 = TM.TRIP(dev(U0), torch.diag(dev(s0)), dev(V0), TM.DeviceCsr(d, DEV))          # the reference's [K, K] S
        assert torch.equal(nU, nU2) and torch.equal(nS, nS2) and torch.equal(nV, nV2)
    # Obj_SimChange against the objective of the sum, and the reference's value
    U, s, V = gold["u_U0"], gold["u_S0"], gold["u_V0"]
    Uc, Vc = U * np.sqrt(s), V * np.sqrt(s)
    d = T.delta(snaps[0], snaps[1])
    r, c, _ = T.entries(d)
    old = np.asarray(snaps[0][r, c]).ravel()
    got = TM.Obj_SimChange(snaps[0], d, dev(Uc), dev(Vc), float(gold["f_loss"][0]))
    assert abs(got - gold["f_tested_loss"][1]) <= 2 * (T.obj_bound(d, Uc, Vc, s_old=old)[0] + 4 * T.U53 * abs(got))
    # RefineBound of step 1: the summation bound of the trace plus K·tol·|w1| (and ARPACK's own n·2⁻⁵³·|w1| per eigenvalue)
    w1 = float(np.abs(np.linalg.eigvalsh(T.bound_dense(snaps[0], d))).max())
    got = TM.RefineBound(snaps[0], d, float(gold["u_loss"][0]), K, tol=T.TOL)
    tot = snaps[0] + d
    trace_bound = (tot.nnz + snaps[0].nnz) * T.U53 * float((tot.data ** 2).sum() + (snaps[0].data ** 2).sum())
    assert abs(got - gold["u_tested_bound"][1]) <= trace_bound + K * (T.TOL + 2 * n * T.U53) * w1 + 4 * T.U53 * abs(got)
    assert got == TM.RefineBound(snaps[0], d, float(gold["u_loss"][0]), K, tol=T.TOL)
