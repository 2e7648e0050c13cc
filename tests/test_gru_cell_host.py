"""Host checks of the any-width GRU cell passes: the dense mirror (tests/_gru_ref.py) against nn.GRU and autograd in float64, the new C
entry points' declarations and argument checks, and the dispatch predicate and refusals of ops.gru_layer.  No GPU needed."""
import ctypes
import os

import pytest
import torch

import _gru_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_gru_cell_fwd_f32", "ctgcn_gru_cell_bwd_f32")


@pytest.mark.parametrize("bias", [True, False])
def test_the_cell_equations_of_the_mirror_are_those_of_nn_gru(bias):
    gen = torch.Generator().manual_seed(5)
    B, L, I, H = 5, 4, 3, 6
    rnn = torch.nn.GRU(I, H, batch_first=True, bias=bias).double()
    x = torch.randn(B, L, I, generator=gen, dtype=torch.float64)
    b_ih, b_hh = (rnn.bias_ih_l0, rnn.bias_hh_l0) if bias else (None, None)
    want = rnn(x)[0]
    got = G.gru_dense(x, rnn.weight_ih_l0, rnn.weight_hh_l0, b_ih, b_hh)
    assert float((got - want).detach().abs().max()) <= 1e-14
    assert float((G.gru_dense(x, rnn.weight_ih_l0, rnn.weight_hh_l0, b_ih, b_hh, reduce_sum=True) - want.sum(1)).detach().abs().max()) <= 1e-14
    gi = x @ rnn.weight_ih_l0.t() + (b_ih if bias else 0)
    assert float((G.gru_dense(None, None, rnn.weight_hh_l0, None, b_hh, gi=gi) - want).detach().abs().max()) <= 1e-14


def test_the_backward_of_the_mirror_is_autograd_of_its_forward():
    gen = torch.Generator().manual_seed(6)
    B, H = 5, 6
    rand = lambda *s: torch.randn(*s, generator=gen, dtype=torch.float64)  # noqa: E731
    gi, gh, h_prev = rand(B, 3 * H).requires_grad_(True), rand(B, 3 * H).requires_grad_(True), rand(B, H).requires_grad_(True)
    b_hh, dh_out, dh_rec = rand(3 * H), rand(B, H), rand(B, H)
    h, gates, q = G.cell_fwd(gi, gh, b_hh, h_prev)
    dgi, dgh, dhp = torch.autograd.grad((h * (dh_out + dh_rec)).sum(), (gi, gh, h_prev))
    got = G.cell_bwd(gates.detach(), q.detach(), h_prev.detach(), dh_out, dh_rec)
    for a, b in zip(got, (dgi, dgh, dhp)):
        assert float((a - b).abs().max()) <= 1e-14
    # step 0: no recurrent term, h_prev = 0
    h, gates, q = G.cell_fwd(gi, None, b_hh, None)
    (dgi,) = torch.autograd.grad((h * dh_out).sum(), (gi,))
    assert float((G.cell_bwd(gates.detach(), q.detach(), None, dh_out, None)[0] - dgi).abs().max()) <= 1e-14


def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_grucell.hip" for s in build.SRCS)


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID = -1
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def fwd(B=4, H=8, gi=p, ldgi=24, gh=p, ldgh=24, b_hh=p, hp=p, ldhp=8, h=p, ldh=8, gates=p, ldg=24, q=p, ldq=8, acc=p, ldacc=8, init=0):
        return lib.ctgcn_gru_cell_fwd_f32(B, H, gi, ldgi, gh, ldgh, b_hh, hp, ldhp, h, ldh, gates, ldg, q, ldq, acc, ldacc, init, None)

    assert fwd(B=-1) == INVALID and fwd(B=2 ** 31) == INVALID and fwd(H=0) == INVALID and fwd(H=2 ** 29) == INVALID
    for name in ("ldgi", "ldgh", "ldg"):
        assert fwd(**{name: 23}) == INVALID, name
    for name in ("ldhp", "ldh", "ldq", "ldacc"):
        assert fwd(**{name: 7}) == INVALID, name
    for name in ("gi", "h", "gates", "q"):                            # gates and q come together
        assert fwd(**{name: None}) == INVALID, name
    assert b"gru_cell_fwd" in lib.ctgcn_last_error()
    assert fwd(B=0) == 0 and fwd(B=0, gi=None, h=None) == 0
    assert fwd(B=0, ldgi=23) == INVALID                               # sizes are checked before the empty call returns

    def bwd(B=4, H=8, gates=p, ldg=24, q=p, ldq=8, hp=p, ldhp=8, do=p, lddo=8, dr=p, lddr=8, dgi=p, lddgi=24, dgh=p, lddgh=24, dp=p, lddp=8):
        return lib.ctgcn_gru_cell_bwd_f32(B, H, gates, ldg, q, ldq, hp, ldhp, do, lddo, dr, lddr, dgi, lddgi, dgh, lddgh, dp, lddp, None)

    assert bwd(B=-1) == INVALID and bwd(B=2 ** 31) == INVALID and bwd(H=0) == INVALID and bwd(H=2 ** 29) == INVALID
    for name in ("ldg", "lddgi", "lddgh"):
        assert bwd(**{name: 23}) == INVALID, name
    for name in ("ldq", "ldhp", "lddo", "lddr", "lddp"):
        assert bwd(**{name: 7}) == INVALID, name
    for name in ("gates", "q", "dgi"):
        assert bwd(**{name: None}) == INVALID, name
    assert b"gru_cell_bwd" in lib.ctgcn_last_error()
    assert bwd(B=0) == 0 and bwd(B=0, gates=None, q=None, dgi=None) == 0


def test_gru_layer_refuses_cpu_tensors_and_the_predicate_reads_the_module():
    from ctgcn_amd import _lib, ops
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.gru_layer(torch.zeros(2, 3, 5), torch.zeros(6, 5), torch.zeros(6, 2))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.gru_layer(None, None, torch.zeros(6, 2), gi=torch.zeros(2, 3, 6))
    cpu = torch.zeros(2, 3, 4)
    assert not ops.rnn_cell_ok(torch.nn.GRU(4, 64, batch_first=True), cpu)          # a CPU sequence never takes the cell path
