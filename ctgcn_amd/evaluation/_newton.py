"""Batched Newton's method with Armijo backtracking for many strictly convex objectives at once: the solver of _logreg.py and _ovr.py.

The caller owns the objective and the Hessians (kernels, scaling, regulariser); this module owns the iteration: the per-model active
mask, the fp64 Cholesky solve with its damping fallback, the line search with both acceptance rules, the iteration counts and the
stall exit.  Nothing here needs a GPU: it runs wherever the callbacks' tensors live.
"""
import torch

LINE_SEARCH_STEPS = 40


def _solve_spd(H, g):
    """-H⁻¹ g of every system by Cholesky; a numerically singular system (saturated fits) is damped by 1e-10 · max|diag|."""
    L, info = torch.linalg.cholesky_ex(H)
    if bool((info > 0).any()):
        damp = (info > 0).to(torch.float64) * 1e-10 * H.diagonal(dim1=1, dim2=2).abs().amax(1).clamp_min(1e-30)
        H = H + damp[:, None, None] * torch.eye(H.shape[1], dtype=torch.float64, device=H.device)
        L = torch.linalg.cholesky(H)
    return -torch.cholesky_solve(g.unsqueeze(2), L).squeeze(2)


def minimize(theta, objective, hessians, tol, max_iter, fitted=None):
    """Newton iterations from theta (double[M, D]) until max|∇f| <= tol for every model, max_iter, or no descent is left.

    objective(theta, live) -> (f double[M], g double[M, D]) in the scaling tol refers to, with g zero for a model that is not fitted;
        only the values of the models in `live` (bool[M]; None: all) are used.
    hessians(theta, active) yields (m0, m1, H): the regularised Hessians (double[m1 - m0, D, D], SPD) of the models m0..m1-1, in any
        chunks; every active model must be covered, and the step of an inactive one is discarded.
    fitted: bool[M], the models to iterate on (None: all).

    Returns (theta, iterations list[M], max|∇f| list[M])."""
    M = theta.shape[0]
    dev = theta.device
    f, g = objective(theta, None)
    iters = torch.zeros(M, dtype=torch.int64, device=dev)
    for _ in range(max_iter):
        gmax = g.abs().amax(1)
        active = gmax > tol
        if fitted is not None:
            active = active & fitted
        if not bool(active.any()):
            break
        iters += active.to(torch.int64)
        p = torch.zeros_like(theta)
        for m0, m1, H in hessians(theta, active):
            p[m0:m1] = _solve_spd(H, g[m0:m1])
        p[~active] = 0
        slope = (g * p).sum(1)
        t = torch.ones(M, dtype=torch.float64, device=dev)
        done = ~active
        for _ls in range(LINE_SEARCH_STEPS):
            trial = torch.where(done[:, None], theta, theta + t[:, None] * p)
            f_new, g_new = objective(trial, ~done)
            armijo = f_new <= f + 1e-4 * t * slope
            # near the optimum the decrease of f sinks below its rounding floor (fp32 z per row) while ∇f is still accurate to
            # ~1e-9: there, a step that lowers max|∇f| is progress
            ok = (armijo | (g_new.abs().amax(1) < gmax)) & ~done
            theta = torch.where(ok[:, None], trial, theta)
            f = torch.where(ok, f_new, f)
            g = torch.where(ok[:, None], g_new, g)
            done = done | ok
            if bool(done.all()):
                break
            t = torch.where(done, t, 0.5 * t)
        if not bool(done.all()):
            break                              # no descent left for some model: stop and report
    return theta, iters.tolist(), g.abs().amax(1).tolist()
