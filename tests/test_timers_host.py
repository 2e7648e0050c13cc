"""TIMERS host logic (no GPU): the new C ABI entries and their argument checks, the interface refusals, and the numpy mirror of
tests/_timers_ref.py (Obj, TRIP, the bound operator, the subspace solver, the whole loop) against what the reference's functions gave
(tests/golden/timers_synth.npz, written by tests/golden/make_golden_timers.py)."""
import importlib
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _timers_ref as T
import ctgcn_amd
from ctgcn_amd import _lib, baseline, build, ops

TM = importlib.import_module("ctgcn_amd.baseline.timers")      # (baseline.timers is the function of that name, as in the reference)
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "timers_synth.npz"))
NEW = ("ctgcn_spmm_csr_f64", "ctgcn_tsgemm_tn_workspace_bytes", "ctgcn_tsgemm_tn_f64", "ctgcn_tsgemm_nn_workspace_bytes",
       "ctgcn_tsgemm_nn_f64", "ctgcn_timers_obj_workspace_bytes", "ctgcn_timers_obj_f64")


def _snaps(prefix):
    return [T.get_csr(GOLD, prefix + "snap%d" % i) for i in range(T.STEPS + 1)]


def test_timers_symbols_exports_and_abi():
    assert _lib.ABI_VERSION == 31 and _lib.load().ctgcn_abi_version() == 31
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctgcn_hip.h")).read()
    lib = _lib.load()
    for name in NEW:
        assert name in _lib.SIGNATURES and name + "(" in header and hasattr(lib, name), name
    assert any(os.path.basename(s) == "ctgcn_timers.hip" for s in build.SRCS)
    for name in ("TIMERS", "timers", "timers_embedding"):
        assert name in ctgcn_amd.__all__ and getattr(ctgcn_amd, name) is getattr(baseline, name) is getattr(TM, name)
    for name in ("get_sp_delta_adj_mat", "Obj", "Obj_SimChange", "RefineBound", "TRIP"):
        assert callable(getattr(TM, name))
    for name in ("spmm_csr_f64", "tsgemm_tn", "tsgemm_nn", "timers_obj", "sym_topk"):
        assert callable(getattr(ops, name))


def test_timers_entries_check_arguments_before_any_launch():
    lib = _lib.load()
    q = 1     # never dereferenced: every call below fails its argument check first, or is the empty call
    INV, WS, UNS = -1, -3, -4
    # spmm: sizes, leading dimensions, null pointers, the empty call
    assert lib.ctgcn_spmm_csr_f64(-1, 4, q, q, q, q, 4, q, 4, 0, None) == INV
    assert b"spmm_csr_f64" in lib.ctgcn_last_error()
    assert lib.ctgcn_spmm_csr_f64(1 << 31, 4, q, q, q, q, 4, q, 4, 0, None) == INV
    assert lib.ctgcn_spmm_csr_f64(10, 0, q, q, q, q, 4, q, 4, 0, None) == INV
    assert lib.ctgcn_spmm_csr_f64(10, 4, q, q, q, q, 3, q, 4, 0, None) == INV            # ldx < b
    assert lib.ctgcn_spmm_csr_f64(10, 4, q, q, q, q, 4, q, 3, 0, None) == INV            # ldy < b
    for hole in range(5):
        p = [q] * 5
        p[hole] = None
        assert lib.ctgcn_spmm_csr_f64(10, 4, p[0], p[1], p[2], p[3], 4, p[4], 4, 0, None) == INV
    assert lib.ctgcn_spmm_csr_f64(0, 4, None, None, None, None, 4, None, 4, 0, None) == 0
    # tsgemm_tn
    assert lib.ctgcn_tsgemm_tn_f64(-1, 4, 4, q, 4, q, 4, q, q, 1 << 30, None) == INV
    assert lib.ctgcn_tsgemm_tn_f64(10, 0, 4, q, 4, q, 4, q, q, 1 << 30, None) == INV
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 0, q, 4, q, 4, q, q, 1 << 30, None) == INV
    assert lib.ctgcn_tsgemm_tn_f64(10, 513, 4, q, 513, q, 4, q, q, 1 << 30, None) == UNS
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 513, q, 4, q, 513, q, q, 1 << 30, None) == UNS
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 4, q, 3, q, 4, q, q, 1 << 30, None) == INV     # ldx < b1
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 4, q, 4, q, 3, q, q, 1 << 30, None) == INV     # ldy < b2
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 4, None, 4, q, 4, q, q, 1 << 30, None) == INV
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 4, q, 4, None, 4, q, q, 1 << 30, None) == INV
    assert lib.ctgcn_tsgemm_tn_f64(10, 4, 4, q, 4, q, 4, None, q, 1 << 30, None) == INV
    need = lib.ctgcn_tsgemm_tn_workspace_bytes(2000, 40, 72)
    assert need > 0 and need % (8 * 40 * 72) == 0 and lib.ctgcn_tsgemm_tn_workspace_bytes(512, 40, 72) == 0
    assert lib.ctgcn_tsgemm_tn_f64(2000, 40, 72, q, 40, q, 72, q, q, need - 1, None) == WS
    assert lib.ctgcn_tsgemm_tn_f64(2000, 40, 72, q, 40, q, 72, q, None, need, None) == WS
    assert lib.ctgcn_tsgemm_tn_f64(0, 4, 4, None, 4, None, 4, None, None, 0, None) == 0
    # tsgemm_nn
    assert lib.ctgcn_tsgemm_nn_f64(-1, 4, 4, q, 4, q, 4, q, 4, None, None, 0, None) == INV
    assert lib.ctgcn_tsgemm_nn_f64(10, 0, 4, q, 4, q, 4, q, 4, None, None, 0, None) == INV
    assert lib.ctgcn_tsgemm_nn_f64(10, 1025, 4, q, 1025, q, 4, q, 4, None, None, 0, None) == UNS
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 513, q, 4, q, 513, q, 513, None, None, 0, None) == UNS
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, q, 3, q, 4, q, 4, None, None, 0, None) == INV      # ldx < b1
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, q, 4, q, 3, q, 4, None, None, 0, None) == INV      # ldc < b2
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, q, 4, q, 4, q, 3, None, None, 0, None) == INV      # ldy < b2
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, None, 4, q, 4, q, 4, None, None, 0, None) == INV
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, q, 4, None, 4, q, 4, None, None, 0, None) == INV
    assert lib.ctgcn_tsgemm_nn_f64(10, 4, 4, q, 4, q, 4, None, 4, None, None, 0, None) == INV
    need = lib.ctgcn_tsgemm_nn_workspace_bytes(130, 40)
    assert need == 8 * 3 * 40
    assert lib.ctgcn_tsgemm_nn_f64(130, 4, 40, q, 4, q, 40, q, 40, q, q, need - 1, None) == WS   # colsq asked for
    assert lib.ctgcn_tsgemm_nn_f64(0, 4, 4, None, 4, None, 4, None, 4, None, None, 0, None) == 0
    # timers_obj
    assert lib.ctgcn_timers_obj_f64(-1, 4, q, q, q, None, q, 4, q, 4, q, q, 1 << 20, None) == INV
    assert lib.ctgcn_timers_obj_f64(10, 0, q, q, q, None, q, 4, q, 4, q, q, 1 << 20, None) == INV
    assert lib.ctgcn_timers_obj_f64(10, 4, q, q, q, None, q, 3, q, 4, q, q, 1 << 20, None) == INV     # ldu < k
    assert lib.ctgcn_timers_obj_f64(10, 4, q, q, q, None, q, 4, q, 3, q, q, 1 << 20, None) == INV     # ldv < k
    for hole in range(6):
        p = [q] * 6
        p[hole] = None
        assert lib.ctgcn_timers_obj_f64(10, 4, p[0], p[1], p[2], None, p[3], 4, p[4], 4, p[5], q, 1 << 20, None) == INV
    need = lib.ctgcn_timers_obj_workspace_bytes(300, 16)
    assert need >= 16 and need % 16 == 0
    assert lib.ctgcn_timers_obj_f64(300, 16, q, q, q, None, q, 16, q, 16, q, q, need - 1, None) == WS
    assert lib.ctgcn_timers_obj_f64(300, 16, q, q, q, None, q, 16, q, 16, q, None, need, None) == WS
    assert b"timers_obj_f64" in lib.ctgcn_last_error()
    assert lib.ctgcn_timers_obj_f64(0, 4, None, None, None, None, None, 4, None, 4, None, None, 0, None) == 0


def test_timers_interface_refusals():
    x = torch.zeros(4, 3, dtype=torch.float64)
    rp, col, val = torch.zeros(5, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0, dtype=torch.float64)
    for call in (lambda: ops.spmm_csr_f64(rp, col, val, x), lambda: ops.tsgemm_tn(x, x), lambda: ops.tsgemm_nn(x, torch.zeros(3, 3, dtype=torch.float64)),
                 lambda: ops.timers_obj(rp, col, val, x, x), lambda: ops.sym_topk(lambda q: q, 4, 1, device="cpu"),
                 lambda: TM.Obj(sp.identity(4, format="csr"), x, x), lambda: TM.TRIP(x, torch.ones(3, dtype=torch.float64), x, sp.identity(4, format="csr")),
                 lambda: TM.RefineBound(sp.identity(4), sp.identity(4), 1.0, 1, device="cpu"),
                 lambda: TM.TIMERS(1, device="cpu").fit_first(sp.identity(4, format="csr"))):
        with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
            call()
    A = sp.csr_matrix(np.triu(np.ones((40, 40)), 1))
    with pytest.raises(ValueError, match="symmetric"):
        TM.TIMERS(4).fit_first(A)
    S = A + A.T
    with pytest.raises(ValueError, match="2 K"):
        TM.TIMERS(20).fit_first(S)           # n = 40 < 2·20 + 2
    with pytest.raises(ValueError, match="non-negative"):
        TM.bound_eigen_sum(np.array([-3.0, -1.0]), 2)
    with pytest.raises(ValueError, match="1 <= k <= n"):
        ops.sym_topk(lambda q: q, 4, 5, device="cuda")


def test_get_sp_delta_adj_mat_matches_the_snapshot_difference(tmp_path):
    snaps = _snaps("tiny_")
    names = ["v%d" % i for i in range(T.TINY_N)]
    cur = sp.triu(snaps[1]).tocoo()
    path = tmp_path / "s1.csv"
    with open(path, "w") as fh:
        fh.write("from_id\tto_id\tweight\n")
        for r, c, w in zip(cur.row, cur.col, cur.data):
            fh.write("%s\t%s\t%g\n" % (names[r], names[c], w))
    for nodes in (names, dict(zip(names, range(len(names))))):
        d = TM.get_sp_delta_adj_mat(snaps[0], str(path), nodes, sep='\t')
        want = T.delta(snaps[0], snaps[1])
        assert sp.issparse(d) and (d != want).nnz == 0 and (d.data != 0).all() and d.nnz == want.nnz


@pytest.mark.parametrize("prefix", ["", "tiny_"])
def test_mirror_obj_and_trip_reproduce_the_reference(prefix):
    snaps, restart = _snaps(prefix), GOLD[prefix + "u_restart"]
    for i in range(T.STEPS + 1):
        U, s, V = GOLD[prefix + "u_U%d" % i], GOLD[prefix + "u_S%d" % i], GOLD[prefix + "u_V%d" % i]
        Uc, Vc = U * np.sqrt(s), V * np.sqrt(s)
        got, want = T.Obj(snaps[i], Uc, Vc), GOLD[prefix + "u_loss"][i]
        assert abs(got - want) <= 2 * T.obj_total_bound(snaps[i], Uc, Vc), (i, got, want)
        if i == 0:
            continue
        U0, s0, V0 = GOLD[prefix + "u_U%d" % (i - 1)], GOLD[prefix + "u_S%d" % (i - 1)], GOLD[prefix + "u_V%d" % (i - 1)]
        d = T.delta(snaps[i - 1], snaps[i])
        nU, nS, nV = T.TRIP(U0, s0, V0, d)
        tag = "u_trip_" if restart[i] else "u_"
        wU, wS, wV = GOLD[prefix + tag + "U%d" % i], GOLD[prefix + tag + "S%d" % i], GOLD[prefix + tag + "V%d" % i]
        cols, sv = T.trip_bound(U0, s0, V0, d)
        assert (np.abs(nU - wU) <= 2 * cols).all() and (np.abs(nV - wV) <= 2 * cols).all(), (i, np.abs(nU - wU).max(), cols.max())
        assert (np.abs(np.diag(nS) - wS) <= 2 * sv).all(), i


def test_mirror_simchange_is_the_objective_of_the_sum():
    snaps = _snaps("tiny_")
    U, s, V = GOLD["tiny_u_U0"], GOLD["tiny_u_S0"], GOLD["tiny_u_V0"]
    Uc, Vc = U * np.sqrt(s), V * np.sqrt(s)
    d = T.delta(snaps[0], snaps[1])
    got = T.Obj_SimChange(snaps[0], d, Uc, Vc, T.Obj(snaps[0], Uc, Vc))
    r, c, _ = T.entries(d)
    old = np.asarray(snaps[0][r, c]).ravel()
    tol = 2 * (T.obj_total_bound(snaps[0], Uc, Vc) + T.obj_total_bound(snaps[1], Uc, Vc) + T.obj_bound(d, Uc, Vc, s_old=old)[0])
    assert abs(got - T.Obj(snaps[1], Uc, Vc)) <= tol
    assert abs(got - GOLD["tiny_f_tested_loss"][1]) <= tol + T.SPREAD_MAX * got


@pytest.mark.parametrize("prefix", ["", "tiny_"])
def test_mirror_bound_operator_and_solver_reproduce_the_reference(prefix):
    snaps = _snaps(prefix)
    n, K = int(GOLD[prefix + "n"]), int(GOLD[prefix + "K"])
    # the solver on the first snapshot: |w| are the reference's singular values
    w, X, its = T.sym_topk(lambda x: snaps[0] @ x, n, K)
    sigma = GOLD[prefix + "u_sigma"][0][::-1]
    assert its > 1 and (np.abs(np.abs(w) - sigma) <= T.TOL * sigma[0] + GOLD[prefix + "spread_sigma"] + n * T.U53 * sigma[0]).all()
    assert (np.linalg.norm(snaps[0] @ X - X * w, axis=0) <= T.TOL * abs(w[0]) + n * T.U53 * abs(w[0])).all()
    # the bound of step 1: operator against its dense form, eigenvalues against LAPACK, the bound against the reference's RefineBound
    d = T.delta(snaps[0], snaps[1])
    apply, trace_change = T.bound_operator(snaps[0], d)
    M = T.bound_dense(snaps[0], d)
    x = np.random.RandomState(3).randn(n, 5)
    assert np.abs(apply(x) - M @ x).max() <= 4 * n * T.U53 * (np.abs(M) @ np.abs(x)).max() + 1e-300
    assert trace_change == GOLD[prefix + "u_trace_change"][1]
    w = T.sym_topk(apply, n, min(2 * K, n))[0]
    s, kept = T.eigen_sum(w, K)
    want = GOLD[prefix + "u_kept1"]
    w1 = np.abs(w).max()
    assert len(kept) == len(want) and (np.abs(kept - want) <= T.TOL * w1 + n * T.U53 * w1).all()
    bound = GOLD[prefix + "u_loss"][0] + trace_change - s
    # (the reference's eigs runs ARPACK to machine precision: n·2⁻⁵³·|w1| per eigenvalue)
    assert abs(bound - GOLD[prefix + "u_tested_bound"][1]) <= K * (T.TOL + 2 * n * T.U53) * w1 + 4 * T.U53 * abs(bound)


@pytest.mark.parametrize("update", [True, False])
def test_mirror_loop_reproduces_the_reference_run(update):
    m = "tiny_u_" if update else "tiny_f_"
    rec = T.run_mirror(_snaps("tiny_"), T.TINY_K, T.THETA, update)
    assert (rec["restart"] == GOLD[m + "restart"]).all()
    allow = 1000 * T.TOL / float(GOLD["tiny_g_min"])
    for key in ("loss", "bound", "tested_loss", "tested_bound"):
        assert (np.abs(rec[key] - GOLD[m + key]) <= allow * np.abs(GOLD[m + key])).all(), key
    rc = GOLD[m + "pick_rc"]
    for i, (Uc, Vc) in enumerate(rec["cur"]):
        got = (Uc[rc[i, :, 0]] * Vc[rc[i, :, 1]]).sum(axis=1)
        assert (np.abs(got - GOLD[m + "pick"][i]) <= allow * GOLD[m + "sigma"][i].max()).all(), i
