"""Epoch-fused loss kernels (ctgcn_epoch.hip) against the per-batch sampler and float64 autograd of the reference's formulas
(metrics.py:38-66 negative sampling, metrics.py:111-123 reconstruction), batch by batch."""
import numpy as np
import pytest
import torch

import _sampling_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pairs(n, num, seed):
    """pair CSR whose rows have degree 0, 1..num and > num; returns (WalkPairs, degrees)"""
    from ctgcn_amd.walks import WalkPairs
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, size=n)
    deg = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, num + 1, size=n), rng.integers(num + 1, 4 * num, size=n)))
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n, size=int(row_ptr[-1]))
    return WalkPairs(torch.from_numpy(row_ptr.astype(np.int32)).to(DEV), torch.from_numpy(col.astype(np.int32)).to(DEV)), deg


def _setup(n=1000, num=5, bs=96, T=2, seed=0, empty_batch=True):
    """a negative-sampling loss over T snapshots with a tiny negative table (negatives collide across batches), an epoch order whose
    batch 1 holds only degree-0 nodes (n_b = 0) and whose last batch is partial, and per-(snapshot, batch) seeds"""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    rng = np.random.default_rng(seed)
    pairs, degs = [], []
    for t in range(T):
        p, d = _pairs(n, num, seed * 10 + t)
        pairs.append(p)
        degs.append(d)
    tables = [torch.from_numpy(rng.integers(0, 12, size=num + 2).astype(np.int32)) for _ in range(T)]
    loss = NegativeSamplingLoss(pairs, tables, neg_num=num, Q=3.5)
    order = rng.permutation(n)
    if empty_batch:
        zero = np.flatnonzero(np.all([d == 0 for d in degs], axis=0))
        assert len(zero) >= bs
        rest = np.setdiff1d(order, zero[:bs], assume_unique=False)
        rest = rest[rng.permutation(len(rest))]
        order = np.concatenate([rest[:bs], zero[:bs], rest[bs:]])
    assert n % bs != 0
    B = -(-n // bs)
    seeds = [[int(x) for x in rng.integers(0, 2 ** 63, size=B)] for _ in range(T)]
    return loss, torch.from_numpy(order).to(DEV), seeds, B


def test_batched_sampler_matches_single_batch_draws():
    loss, perm, seeds, B = _setup()
    bs = 96
    for t in range(2):
        total, offsets, boff, node, pos, neg = loss.batched_sample_indices(t, perm, bs, seeds[t])
        boff = boff.cpu()
        assert int(boff[-1]) == total and int(offsets[-1]) == total and total > 0
        assert neg.shape == (B, 5)
        empty = 0
        for b in range(B):
            batch = perm[b * bs:(b + 1) * bs]
            cnt, nd, ps, ng = loss.sample_indices(t, batch, seed=seeds[t][b])
            lo, hi = int(boff[b]), int(boff[b + 1])
            assert hi - lo == cnt
            if cnt:
                assert torch.equal(node[lo:hi], nd) and torch.equal(pos[lo:hi], ps)
            else:
                empty += 1
            if cnt:
                assert torch.equal(ng, neg[b])
            else:                                                  # the negatives are drawn even when n_b = 0: they depend on the seed only
                _, _, _, ng_alone = loss.sample_indices(t, perm[:bs], seed=seeds[t][b])
                assert torch.equal(neg[b], ng_alone)
        assert empty >= 1
        assert len(torch.unique(neg)) < neg.numel()                # collisions across batches


def _neg_reference(loss, E64, perm, bs, seeds, Q):
    """float64 autograd of metrics.py:38-66 per batch (draws from the single-batch sampler): per-batch losses [T, B] and d(Σ)/dE"""
    T = len(E64)
    leaves = [e.detach().clone().requires_grad_(True) for e in E64]
    B = -(-perm.numel() // bs)
    losses = torch.zeros(T, B, dtype=torch.float64)
    total = 0
    bce = torch.nn.BCEWithLogitsLoss()
    for t in range(T):
        e = leaves[t]
        for b in range(B):
            cnt, nd, ps, ng = loss.sample_indices(t, perm[b * bs:(b + 1) * bs], seed=seeds[t][b])
            if cnt == 0:
                continue
            pos_score = torch.sum(e[nd] * e[ps], dim=1)
            neg_score = torch.sum(e[nd].matmul(e[ng].t()), dim=1)
            lb = bce(pos_score, torch.ones_like(pos_score)) + Q * bce(neg_score, torch.zeros_like(neg_score))
            losses[t, b] = lb.detach().cpu()
            total = total + lb
    total.backward()
    return losses, [e.grad for e in leaves]


def _close(got, want, rtol=1e-5):
    got, want = got.double().cpu(), want.double().cpu()
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= rtol * scale, "max|err| %.3e > %.1e x max|want| %.3e" % (err, rtol, scale)


@pytest.mark.parametrize("layout", ["strided", "list"])
def test_negsampling_loss_matches_float64_autograd(layout):
    loss, perm, seeds, B = _setup()
    n, T, d, bs = 1000, 2, 128, 96
    torch.manual_seed(1)
    base = (0.3 * torch.randn(n, T, d)).to(DEV)
    if layout == "strided":
        E = base.transpose(0, 1)                                   # [T, N, d] view of [N, T, d]: read in place
        G = torch.zeros_like(E)
        assert G.stride() == E.stride()
        E64 = [E[t].double() for t in range(T)]
    else:
        E = [base[:, t].contiguous() for t in range(T)]
        G = [torch.zeros_like(e) for e in E]
        E64 = [e.double() for e in E]
    got = loss.epoch_loss(E, perm, bs, seeds, G)
    want_l, want_g = _neg_reference(loss, E64, perm, bs, seeds, 3.5)
    assert (want_l == 0).any(dim=1).all()                          # the n_b = 0 batch contributes nothing
    _close(got, want_l)
    for t in range(T):
        _close(G[t], want_g[t])


def test_negsampling_loss_accumulates_and_is_deterministic():
    loss, perm, seeds, B = _setup(n=3000, num=8, bs=512, T=1, seed=3, empty_batch=False)
    torch.manual_seed(2)
    E = (0.3 * torch.randn(3000, 64)).to(DEV)
    prior = torch.randn(3000, 64, device=DEV)
    runs = []
    for _ in range(2):
        G = prior.clone()
        l = loss.epoch_loss(E, perm, 512, seeds, G)
        runs.append((l, G))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])     # bit-identical dE
    G0 = torch.zeros_like(E)
    loss.epoch_loss(E, perm, 512, seeds, G0)
    _close(runs[0][1] - prior, G0, rtol=1e-6)                                            # accumulated, not overwritten


def _recon_reference(E64, S64, perm, bs):
    T = len(E64)
    le = [e.detach().clone().requires_grad_(True) for e in E64]
    ls = [s.detach().clone().requires_grad_(True) for s in S64]
    B = -(-perm.numel() // bs)
    losses = torch.zeros(T, B, dtype=torch.float64)
    total = 0
    for t in range(T):
        for b in range(B):
            idx = perm[b * bs:(b + 1) * bs]
            lb = torch.nn.functional.mse_loss(ls[t][idx], le[t][idx])
            losses[t, b] = lb.detach().cpu()
            total = total + lb
    total.backward()
    return losses, [e.grad for e in le], [s.grad for s in ls]


def test_reconstruction_loss_matches_float64_autograd_and_is_deterministic():
    from ctgcn_amd.metrics import ReconstructionLoss
    n, T, d, bs = 1000, 3, 128, 96
    torch.manual_seed(4)
    base = torch.randn(n, T, d, device=DEV)
    E = base.transpose(0, 1)                                       # CTGCN-S embeddings: strided view
    S = [torch.randn(n, d, device=DEV) for _ in range(T)]         # structure list
    perm = torch.randperm(n).to(DEV)
    want_l, want_ge, want_gs = _recon_reference([E[t].double() for t in range(T)], [s.double() for s in S], perm, bs)
    runs = []
    for _ in range(2):
        GE, GS = torch.zeros_like(E), [torch.zeros_like(s) for s in S]
        l = ReconstructionLoss().epoch_loss(E, S, perm, bs, GE, GS)
        runs.append((l, GE, GS))
    l, GE, GS = runs[0]
    _close(l, want_l)
    for t in range(T):
        _close(GE[t], want_ge[t])
        _close(GS[t], want_gs[t])
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(runs[0][2], runs[1][2]))


def test_reconstruction_loss_forward_matches_float64():
    from ctgcn_amd.metrics import ReconstructionLoss
    torch.manual_seed(5)
    n, T, d = 500, 2, 32
    E = torch.randn(T, n, d, device=DEV)
    S = [torch.randn(n, d, device=DEV) for _ in range(T)]
    batch = torch.randperm(n, device=DEV)[:77]
    for idx in (batch, None):
        got = ReconstructionLoss()([E, S, idx])
        want = sum(((S[t].double() - E[t].double()) if idx is None else (S[t][idx].double() - E[t][idx].double())).pow(2).mean()
                   for t in range(T))
        assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())
    got = ReconstructionLoss()([E[0], S[0], None])                # 2-D inputs: one snapshot
    want = (S[0].double() - E[0].double()).pow(2).mean()
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())


# ------------------------------------------------------------------------------------------------------------------------------
# Shapes the epoch runs and the earlier tests do not: every d class of the column loops, lde > d, accumulation onto a prior, and one
# epoch long enough for the tile-scan carry and for long segmented runs.  The draws come from the host model (tests/_sampling_ref.py),
# so a sampler bug cannot hide in a reference that shares it.
PAD = 3                                                            # list layout: rows of a [N, d + PAD] buffer, so lde = d + PAD > d


def _model_sampler(loss, perm, bs, seeds):
    """sample_indices(t, batch b, seed) with the signature _neg_reference uses, answered by the host model"""
    perm_h = perm.cpu().numpy()
    num = int(loss.neg_sample_num)
    cache = {}

    def draws(t):
        if t not in cache:
            pairs, table = loss._device_inputs(t, perm.device)
            node, pos, _, boff = R.pos_draws(perm_h, bs, seeds[t], pairs.row_ptr.cpu().numpy(), pairs.col.cpu().numpy(), num)
            neg = np.stack([R.neg_draws(s, table.cpu().numpy(), num) for s in seeds[t]])
            cache[t] = (torch.from_numpy(node).to(perm.device), torch.from_numpy(pos).to(perm.device), boff,
                        torch.from_numpy(neg).to(perm.device))
        return cache[t]

    def sample_indices(t, batch, seed):
        node, pos, boff, neg = draws(t)
        b = seeds[t].index(seed)
        assert seeds[t].count(seed) == 1
        lo, hi = int(boff[b]), int(boff[b + 1])
        return hi - lo, node[lo:hi], pos[lo:hi], neg[b]

    return sample_indices


class _ModelDrawn(object):
    """what _neg_reference needs of a loss, with the draws taken from the host model"""

    def __init__(self, loss, perm, bs, seeds):
        self.sample_indices = _model_sampler(loss, perm, bs, seeds)


def _report_close(got, want, what, rtol=1e-5):
    got, want = got.double().cpu(), want.double().cpu()
    scale, err = want.abs().max().item(), (got - want).abs().max().item()
    print("  [epoch-loss] %-44s max|err| %.3e = %.3e x max|want| %.3e" % (what, err, err / max(scale, 1e-300), scale))
    _close(got, want, rtol)


def _shaped(n, T, d, layout, seed, scale):
    """T matrices [n, d] with lde > d in both layouts: 'strided' = the [T, N, d] view of [N, T, d] (lde = T d), 'list' = the first d
    columns of [N, d + PAD] buffers.  Returns (what epoch_loss takes, the per-snapshot views, the buffers)"""
    g = torch.Generator().manual_seed(seed)
    if layout == "strided":
        buf = (scale * torch.randn(n, T, d, generator=g)).to(DEV)
        arg = buf.transpose(0, 1)
        return arg, [arg[t] for t in range(T)], [buf]
    bufs = [(scale * torch.randn(n, d + PAD, generator=g)).to(DEV) for _ in range(T)]
    views = [b[:, :d] for b in bufs]
    return views, views, bufs


@pytest.mark.parametrize("layout", ["strided", "list"])
@pytest.mark.parametrize("d", [1, 37, 63, 65, 100, 500, 512])
def test_negsampling_loss_shapes_match_float64_on_model_draws(d, layout):
    loss, perm, seeds, B = _setup()
    n, T, bs = 1000, 2, 96
    E, Ev, _ = _shaped(n, T, d, layout, 100 + d, 0.3)
    G, Gv, Gbuf = _shaped(n, T, d, layout, 200 + d, 0.02)          # a non-zero prior of the gradients' own size: the kernels accumulate
    prior = [g.double() for g in Gv]
    before = [b.clone() for b in Gbuf]
    assert all(e.stride(0) > d for e in Ev) and all(g.stride(0) > d for g in Gv)
    got = loss.epoch_loss(E, perm, bs, seeds, G)
    want_l, want_g = _neg_reference(_ModelDrawn(loss, perm, bs, seeds), [e.double() for e in Ev], perm, bs, seeds, 3.5)
    assert (want_l == 0).any(dim=1).all() and (want_l != 0).any(dim=1).all()
    _report_close(got, want_l, "neg d=%d %s loss" % (d, layout))
    for t in range(T):
        _report_close(Gv[t].double() - prior[t], want_g[t], "neg d=%d %s dE[%d]" % (d, layout, t))
    if layout == "list":                                           # the padding columns beyond d are not the kernels' to write
        assert all(torch.equal(b[:, d:], b0[:, d:]) for b, b0 in zip(Gbuf, before))


def test_negsampling_loss_refuses_d_513_and_writes_nothing():
    from ctgcn_amd._lib import CtgcnHipError
    loss, perm, seeds, B = _setup()
    E, _, _ = _shaped(1000, 2, 513, "list", 7, 0.3)
    G, _, Gbuf = _shaped(1000, 2, 513, "list", 8, 0.02)
    before = [b.clone() for b in Gbuf]
    with pytest.raises(CtgcnHipError, match=r"code -4\)"):           # CTGCN_E_UNSUPPORTED
        loss.epoch_loss(E, perm, 96, seeds, G)
    torch.cuda.synchronize()
    assert all(torch.equal(b, b0) for b, b0 in zip(Gbuf, before))


@pytest.mark.parametrize("layout", ["strided", "list"])
@pytest.mark.parametrize("d", [1, 37, 63, 65, 100, 500, 512, 513])
def test_reconstruction_loss_shapes_match_float64(d, layout):
    """the reconstruction kernel strides its lanes over d: no cap at 512"""
    from ctgcn_amd.metrics import ReconstructionLoss
    n, T, bs = 1000, 2, 96
    E, Ev, _ = _shaped(n, T, d, layout, 300 + d, 1.0)
    S, Sv, _ = _shaped(n, T, d, "list", 400 + d, 1.0)
    GE, GEv, GEbuf = _shaped(n, T, d, layout, 500 + d, 0.02 / d)     # priors of the gradients' own size, 2 (s - e) / (|b| d): the sum is
    GS, GSv, GSbuf = _shaped(n, T, d, "list", 600 + d, 0.02 / d)     # rounded to fp32 at ITS magnitude, which a large prior would dominate
    pe, ps = [g.double() for g in GEv], [g.double() for g in GSv]
    before = [b.clone() for b in GEbuf + GSbuf]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(d)).to(DEV)
    want_l, want_ge, want_gs = _recon_reference([e.double() for e in Ev], [s.double() for s in Sv], perm, bs)
    got = ReconstructionLoss().epoch_loss(E, S, perm, bs, GE, GS)
    _report_close(got, want_l, "recon d=%d %s loss" % (d, layout))
    for t in range(T):
        _report_close(GEv[t].double() - pe[t], want_ge[t], "recon d=%d %s dE[%d]" % (d, layout, t))
        _report_close(GSv[t].double() - ps[t], want_gs[t], "recon d=%d %s dS[%d]" % (d, layout, t))
    for b, b0 in zip(GEbuf + GSbuf, before):
        if b.dim() == 2:                                           # [N, d + PAD] buffers: the padding is not the kernel's to write
            assert torch.equal(b[:, d:], b0[:, d:])


def test_negsampling_loss_600k_positions_match_float64_and_are_deterministic():
    """N = P = 600 000 at batch 2 048: 293 batches and 293 scan tiles (the tile-sum scan carries into a second chunk of 256), and a
    64-entry negative table over 8 nodes, so single nodes collect dS from hundreds of batches in one segmented run."""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    n, bs, d, num = 600000, 2048, 32, 8
    rng = np.random.default_rng(77)
    pairs, _ = _pairs(n, num, 78)
    table = torch.from_numpy(rng.integers(0, n, size=8)[rng.integers(0, 8, size=64)].astype(np.int32))
    loss = NegativeSamplingLoss([pairs], [table], neg_num=num, Q=3.5)
    perm = torch.from_numpy(rng.permutation(n)).to(DEV)
    B = -(-n // bs)
    assert B == 293 and n % bs != 0
    seeds = [[int(x) for x in rng.integers(0, 2 ** 64, size=B, dtype=np.uint64)]]
    E = (0.3 * torch.randn(n, d, generator=torch.Generator().manual_seed(79))).to(DEV)
    runs = []
    for _ in range(2):
        G = torch.zeros_like(E)
        runs.append((loss.epoch_loss(E, perm, bs, seeds, G), G))
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    drawn = _ModelDrawn(loss, perm, bs, seeds)
    negs = torch.stack([drawn.sample_indices(0, None, s)[3] for s in seeds[0]])
    assert torch.bincount(negs.view(-1)).max().item() > 200        # one node is a negative hundreds of times over
    want_l, want_g = _neg_reference(drawn, [E.double()], perm, bs, seeds, 3.5)
    _report_close(runs[0][0], want_l, "neg 600k loss")
    _report_close(runs[0][1], want_g[0], "neg 600k dE")
