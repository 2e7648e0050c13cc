"""ops.batch_norm_act (ctgcn_pool.hip) against float64 F.batch_norm + relu: the statistics (several statistics blocks with a partial
last one, a column with a mean five orders above its spread), the apply pass with and without the ReLU, dropout against the host
model of the draw, eval mode with given statistics, and dx, dw, db against float64 autograd.  Scalar and float4 rows, one to five
passes of the backward's 64 lanes.  Tolerance: conftest.close_scaled's (1e-5 relative plus 2e-6 of the tensor's largest magnitude):
outputs and gradients are O(1) sums of at most 1000 fp32 terms.  dx with batch statistics is the exception: w rstd (g - mean(g) -
x_hat mean(g x_hat)) is a difference of terms of size A = max|w rstd| max|dy| that cancel (with 2 rows almost entirely: x_hat is +-1),
and each term carries a few fp32 ulps of A, so its absolute part is 2e-6 of the larger of the tensor's magnitude and A, with A
computed in float64.  Every output is repeated and compared bit for bit."""
import numpy as np
import pytest
import torch
from torch.nn import functional as F

import _gcrn_ref as R
from _gcn_graphs import DEV, dense

pytestmark = pytest.mark.gpu
EPS = 1e-5
KEY = 2 ** 60 + 4242
NS = (2, 67, 199, 1000)                  # 1000 rows: seven statistics blocks of 128 and one of 104; sixteen backward blocks of 64, the last of 40
DS = (1, 10, 24, 130, 132, 260)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


def used(got, ref, what, terms=0.0):
    """close_scaled's tolerance, its absolute part also covering `terms`, the size of the terms that cancel in ref; prints the share used"""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    tol = 1e-5 * np.abs(ref) + 2e-6 * max(1.0, float(np.abs(ref).max(initial=0.0)), terms)
    share = float((np.abs(got - ref) / tol).max(initial=0.0))
    print("  [tol] %-40s %.3f of the tolerance" % (what, share))
    assert share <= 1.0, what


def dx_terms(x, w, C):
    """A = max|w rstd| max|dy| in float64"""
    return float((np.abs(f64(w)) / np.sqrt(f64(x).var(axis=0) + EPS)).max() * np.abs(f64(C)).max())


def inputs(n, d, seed=0):
    """x with a column-dependent scale and offset.  Two rows are kept at least half a unit apart: a column whose spread is far below
    its magnitude loses its digits in x - mean in any fp32 program, which test_a_large_mean_does_not_cost_the_variance is about"""
    base = dense((n, d), 100 * n + d + seed)
    if n == 2:
        base[1] = base[0] + np.where(base[1] >= 0, 1, -1).astype(np.float32) * (np.float32(0.5) + np.float32(0.5) * np.abs(base[1]))
    x = base * np.linspace(0.5, 3.0, d, dtype=np.float32) + np.linspace(-2.0, 2.0, d, dtype=np.float32)
    w = dense((d,), d + 1) + np.float32(1.5) * np.sign(dense((d,), d + 3))        # both signs, away from 0
    b = dense((d,), d + 2)
    return torch.from_numpy(x).to(DEV), torch.from_numpy(w).to(DEV), torch.from_numpy(b).to(DEV)


def stock(x, w, b, relu, mean=None, var=None, keep=None, p=0.0):
    """float64 F.batch_norm (+ relu, + the keep mask) on the CPU, with leaves to differentiate"""
    x64, w64, b64 = (t.detach().cpu().double().requires_grad_() for t in (x, w, b))
    if mean is None:
        y = F.batch_norm(x64, None, None, w64, b64, True, 0.1, EPS)
    else:
        y = F.batch_norm(x64, mean.cpu().double(), var.cpu().double(), w64, b64, False, 0.1, EPS)
    if relu:
        y = F.relu(y)
    if keep is not None:
        y = y * torch.from_numpy(keep).double() / (1.0 - p)
    return y, (x64, w64, b64)


@pytest.mark.parametrize("relu", [False, True], ids=["plain", "relu"])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_training_mode_forward_and_backward(n, d, relu):
    from ctgcn_amd import ops
    x, w, b = inputs(n, d)
    C = torch.from_numpy(dense((n, d), n + d + 7)).to(DEV)
    leaves = [t.clone().requires_grad_() for t in (x, w, b)]
    y, mean, var = ops.batch_norm_act(*leaves, relu=relu, eps=EPS)
    (y * C).sum().backward()
    want, leaves64 = stock(x, w, b, relu)
    (want * C.cpu().double()).sum().backward()
    what = "n %d d %d" % (n, d)
    used(f64(mean), f64(x).mean(axis=0), what + " mean")
    used(f64(var), f64(x).var(axis=0), what + " var")
    used(f64(y), want.detach().numpy(), what + " y")
    for name, got, ref in zip(("dx", "dw", "db"), leaves, leaves64):
        used(f64(got.grad), ref.grad.numpy(), what + " " + name, dx_terms(x, w, C) if name == "dx" else 0.0)
    assert not mean.requires_grad and not var.requires_grad
    again = [t.clone().requires_grad_() for t in (x, w, b)]
    y2, mean2, var2 = ops.batch_norm_act(*again, relu=relu, eps=EPS)
    (y2 * C).sum().backward()
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(var, var2)
    assert all(torch.equal(a.grad, c.grad) for a, c in zip(leaves, again))


@pytest.mark.parametrize("n", [1, 67])
def test_eval_mode_uses_the_given_statistics(n):
    from ctgcn_amd import ops
    d = 24
    x, w, b = inputs(n, d)
    mean = torch.from_numpy(dense((d,), 5)).to(DEV)
    var = torch.from_numpy(np.abs(dense((d,), 6)) + np.float32(0.1)).to(DEV)
    C = torch.from_numpy(dense((n, d), 7)).to(DEV)
    for relu in (False, True):
        leaves = [t.clone().requires_grad_() for t in (x, w, b)]
        y, m, v = ops.batch_norm_act(*leaves, mean, var, relu=relu, eps=EPS)
        (y * C).sum().backward()
        assert torch.equal(m, mean) and torch.equal(v, var)
        want, leaves64 = stock(x, w, b, relu, mean, var)
        (want * C.cpu().double()).sum().backward()
        used(f64(y), want.detach().numpy(), "eval n %d y" % n)
        for name, got, ref in zip(("dx", "dw", "db"), leaves, leaves64):
            used(f64(got.grad), ref.grad.numpy(), "eval n %d %s" % (n, name))
        assert torch.equal(y, ops.batch_norm_act(x, w, b, mean, var, relu=relu, eps=EPS)[0])


def test_a_single_row_in_training_mode_raises_torch_s_error():
    from ctgcn_amd import ops
    x, w, b = inputs(1, 10)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        ops.batch_norm_act(x, w, b)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        F.batch_norm(x, None, None, w, b, True)
    for bad in (lambda: ops.batch_norm_act(x, w[:-1], b), lambda: ops.batch_norm_act(x, w, b, w, None), lambda: ops.batch_norm_act(x, w, b, p=1.0),
                lambda: ops.batch_norm_act(x[0], w, b)):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        ops.batch_norm_act(x.double(), w, b)


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("d", [10, 24, 130, 132])
def test_dropout_follows_the_host_model(d, p):
    from ctgcn_amd import ops
    n = 199
    x, w, b = inputs(n, d)
    C = torch.from_numpy(dense((n, d), d + 9)).to(DEV)
    plain = ops.batch_norm_act(x, w, b, relu=True, eps=EPS)[0]
    assert torch.equal(plain, ops.batch_norm_act(x, w, b, relu=True, p=0.0, key=KEY, eps=EPS)[0])
    masks = []
    for key in (KEY, KEY + 1):
        keep = R.keep_mask(key, n, d, p)
        leaves = [t.clone().requires_grad_() for t in (x, w, b)]
        y = ops.batch_norm_act(*leaves, relu=True, p=p, key=key, eps=EPS)[0]
        (y * C).sum().backward()
        assert np.array_equal(f64(y) != 0, keep & (f64(plain) > 0))
        want, leaves64 = stock(x, w, b, True, keep=keep, p=p)
        (want * C.cpu().double()).sum().backward()
        used(f64(y), want.detach().numpy(), "dropout d %d p %g y" % (d, p))
        for name, got, ref in zip(("dx", "dw", "db"), leaves, leaves64):
            used(f64(got.grad), ref.grad.numpy(), "dropout d %d p %g %s" % (d, p, name), dx_terms(x, w, C) / (1.0 - p) if name == "dx" else 0.0)
        again = [t.clone().requires_grad_() for t in (x, w, b)]
        y2 = ops.batch_norm_act(*again, relu=True, p=p, key=key, eps=EPS)[0]
        (y2 * C).sum().backward()
        assert torch.equal(y, y2) and all(torch.equal(a.grad, c.grad) for a, c in zip(leaves, again))
        masks.append(keep)
    assert (masks[0] != masks[1]).mean() > 0.5 * 2 * p * (1 - p)


@pytest.mark.parametrize("n", [199, 1000])
def test_a_large_mean_does_not_cost_the_variance(n):
    """column 3 holds 1e4 + U(-0.1, 0.1): E[x^2] - mean^2 in fp32 loses every digit of its variance (1e8 against 3e-3).  The variance is
    compared with the float64 variance of the same fp32 inputs; the tolerance is 4 x the error of torch's CPU fp32 F.batch_norm on this
    input (its running_var from zero with momentum 1, brought back to the biased form), computed here."""
    from ctgcn_amd import ops
    d = 10
    x, w, b = inputs(n, d)
    rng = np.random.default_rng(n)
    col = (1e4 + rng.uniform(-0.1, 0.1, n)).astype(np.float32)
    x[:, 3] = torch.from_numpy(col).to(DEV)
    exact = col.astype(np.float64).var()
    run_var = torch.zeros(d)
    F.batch_norm(x.cpu(), torch.zeros(d), run_var, None, None, True, 1.0, EPS)
    stock_err = abs(float(run_var[3]) * (n - 1) / n - exact)
    _, mean, var = ops.batch_norm_act(x, w, b, eps=EPS)
    err = abs(float(var[3]) - exact)
    naive = abs(float((col * col).mean() - col.mean() ** 2) - exact)
    print("  [tol] large mean n %d: |var - exact| %.3e = %.3f of 4 x torch's %.3e (exact %.3e; the one-pass fp32 formula is off by %.3e)" % (
        n, err, err / (4 * stock_err) if stock_err else float("inf") if err else 0.0, stock_err, exact, naive))
    assert err <= 4 * stock_err
    assert abs(float(mean[3]) - col.astype(np.float64).mean()) <= 1e4 * 2.0 ** -23        # within an fp32 ulp of 1e4
    assert naive > 100 * max(err, 1e-12)                                                  # what the test is for
    used(f64(var)[np.arange(d) != 3], f64(x).var(axis=0)[np.arange(d) != 3], "large mean n %d other columns" % n)
