"""The kernels of ctgcn_gat.hip (ops.gat_conv) against the float64 mirror of tests/_gat_ref.py: the forward with its row maximum m,
row sum Z and the three epilogues at every dispatch boundary (scalar and float4 lanes, every lane-group width, rows around each
width, head boundaries inside a float4, two and more passes of the lanes, long rows in pieces), logits beyond fp32 exp's range, both
dropouts against the host models of their draws, and the backward over the CSR and its transpose under autograd.  The graphs are
those of test_gpu_gcn_conv.py (rebuilt here from _gcn_graphs.py): not symmetric, and a directed one whose transpose has other long
rows; only their pattern is read.

Tolerance: the larger of conftest.close_scaled's (1e-5 |ref| + 2e-6 max(1, max|ref|)) and 4 x the largest error of the float32 mirror
against the float64 mirror on the same inputs; computed here on the CPU from the mirror alone."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _gat_ref as A
from _gcn_graphs import DEV, N, WIDTHS, dense, gcn_adj, symmetric_graph

pytestmark = pytest.mark.gpu
NONE, ELU, ELU_DROP = 0, 1, 2
EPIS = {"none": NONE, "elu": ELU, "elu_drop": ELU_DROP}
SHAPES = [(1, 1), (1, 6), (2, 3), (3, 6), (1, 12), (2, 12), (8, 16), (1, 130), (1, 132), (4, 33), (1, 500)]
KEY, FKEY = 2 ** 61 + 12345, 2 ** 60 + 99
_graphs = {}


def row_scaled(m, seed):
    r = np.random.default_rng(seed).uniform(0.5, 1.5, m.shape[0])
    out = (sp.diags(r) @ m).tocsr()
    out.sort_indices()
    out.data = out.data.astype(np.float32).astype(np.float64)
    return out


def graph(width):
    """symmetric_graph(width) with its rows scaled, as test_gpu_gcn_conv.py's: rows of 0, 1, width - 1, width, width + 1, 8, 9 entries"""
    if width not in _graphs:
        m = row_scaled(symmetric_graph(width), 7 + width)
        assert list(np.diff(m.indptr)[:7]) == [0, 1, width - 1, width, width + 1, 8, 9]
        _graphs[width] = m
    return _graphs[width]


def directed_graph():
    """graph(64) without the strictly-lower-triangular entries of every third row: rows and columns have different lengths"""
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


def inputs(heads, F, seed=0, scale=1.0):
    d = heads * F
    S = torch.from_numpy(dense((N, d), 100 + d + seed))
    a_src = torch.from_numpy(dense((heads, F), 200 + d + seed)) * scale
    a_dst = torch.from_numpy(dense((heads, F), 300 + d + seed)) * scale
    C = torch.from_numpy(dense((N, d), 400 + d + seed))
    return S, a_src, a_dst, C


def mirror(m, S, a_src, a_dst, heads, epi, C=None, dtype=torch.float64, keep_att=None, p_att=0.0, keep_feat=None, p_feat=0.0, shifted=True):
    """dict of float64 numpy arrays: out, m, Z and, with C, the gradients of sum(out * C)"""
    rows, cols = A.entries(m)
    S, a_src, a_dst = (t.detach().cpu().to(dtype).requires_grad_(C is not None) for t in (S, a_src, a_dst))
    Y, mx, Z = A.attention(S, a_src, a_dst, rows, cols, heads, A.ALPHA, keep_att, p_att, shifted)
    out = A.epilogue(Y, epi, keep_feat, p_feat)
    res = {"out": out, "m": mx, "Z": Z}
    if C is not None:
        (out * C.cpu().to(dtype)).sum().backward()
        res.update(dS=S.grad, da_src=a_src.grad, da_dst=a_dst.grad)
    return {k: v.detach().double().numpy() for k, v in res.items()}


def references(*args, **kw):
    return mirror(*args, dtype=torch.float64, **kw), mirror(*args, dtype=torch.float32, **kw)


def check(got, ref, what):
    """got against ref = (float64 mirror, float32 mirror), one key at a time; prints the share of the tolerance used"""
    r64, r32 = ref
    for k, g in got.items():
        g = g.detach().cpu().double().numpy()
        want = r64[k]
        tol = np.maximum(1e-5 * np.abs(want) + 2e-6 * max(1.0, float(np.abs(want).max(initial=0.0))), 4 * np.abs(r32[k] - want).max(initial=0.0))
        used = float((np.abs(g - want) / tol).max(initial=0.0))
        print("  [tol] %-46s max |err| %.3e  = %.3f of the tolerance" % ("%s %s" % (what, k), float(np.abs(g - want).max(initial=0.0)), used))
        assert np.isfinite(g).all() and used <= 1.0, "%s %s: %.2f x the tolerance" % (what, k, used)


def forward(adj, S, a_src, a_dst, heads, epi=NONE, p_att=0.0, key=0, p_feat=0.0, fkey=0):
    from ctgcn_amd import ops
    out, _, _, _, m, Z = ops._gat_fwd(adj, S, a_src, a_dst, heads, A.ALPHA, epi, p_att, key, p_feat, fkey)
    return {"out": out, "m": m, "Z": Z}


def backward(adj, S, a_src, a_dst, heads, epi, C, needs=(True, True, True), **kw):
    from ctgcn_amd import ops
    leaves = [t.detach().clone().requires_grad_(need) for t, need in zip((S, a_src, a_dst), needs)]
    out = ops.gat_conv(leaves[0], leaves[1], leaves[2], adj, heads, A.ALPHA, epi, **kw)
    (out * C).sum().backward()
    res = {"out": out.detach()}
    res.update({k: t.grad for k, t, need in zip(("dS", "da_src", "da_dst"), leaves, needs) if need})
    return res


def gpu(*tensors):
    return [t.to(DEV) for t in tensors]


@pytest.mark.parametrize("heads,F", SHAPES)
def test_forward_m_Z_and_epilogues_at_every_lane_group_width(heads, F):
    S, a_src, a_dst, _ = inputs(heads, F)
    Sg, asg, adg = gpu(S, a_src, a_dst)
    for width in WIDTHS:
        m = graph(width)
        adj = gcn_adj(m)
        assert adj.long_rows is None
        for name, epi in EPIS.items():
            ref = references(m, S, a_src, a_dst, heads, epi)
            got = forward(adj, Sg, asg, adg, heads, epi)
            check(got, ref, "%dx%d w%d %s" % (heads, F, width, name))
            assert not got["out"][0].any() and float(got["Z"][0].abs().max()) == 0.0          # the empty row: exact zeros
            assert bool((got["Z"][1:] >= 1.0).all())                                          # the row maximum contributes exp(0)
            again = forward(adj, Sg, asg, adg, heads, epi)
            assert all(torch.equal(got[k], again[k]) for k in got)
        if heads * F > 1:
            assert bool((got["out"] < 0).any()) and bool((got["out"] > 0).any())


def test_logits_beyond_the_range_of_fp32_exp():
    """a scaled so that one row's logits all lie below -120 (fp32 exp underflows: 0 / 0) and another's reach above +500 (overflow:
    inf / inf).  The mirror's unshifted float32 variant, the reference's arithmetic, gives NaN on those rows, here on the CPU; the
    kernels' shifted form gives float64's result."""
    heads, F = 2, 12
    m = graph(16)
    S, a_src, a_dst, _ = inputs(heads, F)
    rows, cols = A.entries(m)
    lo, hi = 5, 6                                                # rows of 8 and 9 entries
    S[lo], S[hi] = 0.0, 0.0
    S[lo, 0], S[lo, F] = 140.0, 140.0                            # u_lo = 140 a_src[h, 0]: z > 0, l = -z
    S[hi, 0], S[hi, F] = -2700.0, -2700.0                        # z < 0, l = -alpha z
    a_src[:, 0], a_dst[:, 0] = 1.0, 0.0
    unshifted = mirror(m, S, a_src, a_dst, heads, NONE, dtype=torch.float32, shifted=False)
    assert np.isnan(unshifted["out"][lo]).all() and np.isnan(unshifted["out"][hi]).all()
    ref = references(m, S, a_src, a_dst, heads, NONE)
    assert (ref[0]["m"][lo] < -120).all() and (ref[0]["m"][hi] > 500).all()
    got = forward(gcn_adj(m), *gpu(S, a_src, a_dst), heads)
    assert bool(torch.isfinite(got["out"]).all())
    check(got, ref, "extreme logits")


@pytest.mark.parametrize("heads,F", [(1, 6), (2, 12), (4, 33), (1, 132), (1, 500)])
def test_long_rows_of_a_directed_matrix_and_of_its_transpose(heads, F):
    """long_threshold 8: rows of 9 entries and more go to the piece kernels, in the forward and the row pass over the matrix, in the
    column pass over its transpose, whose long rows are others; short rows are bit-identical to the run without a long-row list"""
    from ctgcn_amd import ops
    m = directed_graph()
    adj, plain = gcn_adj(m, long_threshold=8), gcn_adj(m)
    adj_t, plain_t = adj.transposed(), plain.transposed()
    rows, colsn = np.diff(m.indptr), np.diff(m.T.tocsr().indptr)
    assert sorted(adj.long_rows.cpu().tolist()) == np.nonzero(rows > 8)[0].tolist() != []
    assert sorted(adj_t.long_rows.cpu().tolist()) == np.nonzero(colsn > 8)[0].tolist() != [] and plain.long_rows is None
    assert adj.long_rows.cpu().tolist() != adj_t.long_rows.cpu().tolist()
    S, a_src, a_dst, C = inputs(heads, F)
    Sg, asg, adg, Cg = gpu(S, a_src, a_dst, C)
    short = torch.from_numpy(rows <= 8).to(DEV)
    short_t = torch.from_numpy(colsn <= 8).to(DEV)
    for name, epi in EPIS.items():
        ref = references(m, S, a_src, a_dst, heads, epi, C)
        got = forward(adj, Sg, asg, adg, heads, epi)
        want = forward(plain, Sg, asg, adg, heads, epi)
        assert all(torch.equal(got[k][short], want[k][short]) for k in got)
        check(got, ref, "pieces fwd " + name)
        check(backward(adj, Sg, asg, adg, heads, epi, Cg), ref, "pieces bwd " + name)
    # the two backward passes on their own: du over the matrix, dv over the transpose
    _, Y, u, v, mx, Z = ops._gat_fwd(adj, Sg, asg, adg, heads, A.ALPHA, NONE)
    G, pack = ops._gat_bwd_prep(Cg, Y, u, mx, Z, heads, NONE)
    du, du_plain = (ops._gat_bwd_row(a, Sg, G, v, pack, heads, A.ALPHA) for a in (adj, plain))
    assert torch.equal(du[short], du_plain[short]) and torch.equal(du, ops._gat_bwd_row(adj, Sg, G, v, pack, heads, A.ALPHA))
    (_, dv), (_, dv_plain) = (ops._gat_bwd_col(a, Sg, G, v, pack, asg, adg, heads, A.ALPHA) for a in (adj_t, plain_t))
    assert torch.equal(dv[short_t], dv_plain[short_t])
    dS, dv2 = ops._gat_bwd_col(adj_t, Sg, G, v, pack, asg, adg, heads, A.ALPHA, du=du)
    assert torch.equal(dv, dv2)                                   # dv does not depend on whether dS is asked for
    ref = references(m, S, a_src, a_dst, heads, NONE, C)
    check({"dS": dS}, ref, "pieces passes")
    S3 = S.reshape(N, heads, F).double()
    check({"da_src": (du.cpu().double()[:, :, None] * S3).sum(0), "da_dst": (dv.cpu().double()[:, :, None] * S3).sum(0)}, ref, "pieces du dv")


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("heads,F", [(1, 6), (2, 12), (4, 33), (1, 132)])
def test_attention_dropout_follows_the_host_model_forward_and_backward(heads, F, p, long_threshold):
    m = directed_graph()
    adj = gcn_adj(m, long_threshold)
    rows, cols = A.entries(m)
    S, a_src, a_dst, C = inputs(heads, F)
    Sg, asg, adg, Cg = gpu(S, a_src, a_dst, C)
    masks = []
    for key in (KEY, KEY + 4096):
        keep = torch.from_numpy(A.att_keep(key, rows.numpy(), cols.numpy(), heads, p))
        masks.append(keep)
        ref = references(m, S, a_src, a_dst, heads, ELU, C, keep_att=keep, p_att=p)
        got = backward(adj, Sg, asg, adg, heads, ELU, Cg, p_att=p, key=key)
        # the backward under the same key: its column pass runs over the transposed CSR and regenerates the draw from (i, j)
        check(got, ref, "attention dropout p %g" % p)
        again = backward(adj, Sg, asg, adg, heads, ELU, Cg, p_att=p, key=key)
        assert all(torch.equal(got[k], again[k]) for k in got)
    differ = float((masks[0] != masks[1]).double().mean())
    assert abs(differ - 2 * p * (1 - p)) < 5 * np.sqrt(0.25 / masks[0].numel()) + 0.02, differ
    plain = backward(adj, Sg, asg, adg, heads, ELU, Cg)
    zero = backward(adj, Sg, asg, adg, heads, ELU, Cg, p_att=0.0, key=KEY)
    assert all(torch.equal(plain[k], zero[k]) for k in plain)
    dropped = backward(adj, Sg, asg, adg, heads, ELU, Cg, p_att=p, key=KEY)
    assert not torch.equal(plain["out"], dropped["out"])


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("heads,F", [(1, 6), (2, 12), (4, 33), (1, 132)])
def test_feature_dropout_follows_the_host_model(heads, F, p, long_threshold):
    m = directed_graph()
    adj = gcn_adj(m, long_threshold)
    S, a_src, a_dst, C = inputs(heads, F)
    Sg, asg, adg, Cg = gpu(S, a_src, a_dst, C)
    d = heads * F
    keep = A.feat_keep(FKEY, N, d, p)
    ref = references(m, S, a_src, a_dst, heads, ELU_DROP, C, keep_feat=torch.from_numpy(keep), p_feat=p)
    got = backward(adj, Sg, asg, adg, heads, ELU_DROP, Cg, p_feat=p, fkey=FKEY)
    check(got, ref, "feature dropout p %g" % p)
    out = got["out"].cpu().numpy()
    elu = mirror(m, S, a_src, a_dst, heads, ELU)["out"]
    sure = np.abs(elu) > 1e-4                                    # an ELU output of (nearly) 0 is not a dropped entry
    assert np.array_equal((out != 0)[sure], keep[sure])           # kept exactly where the host model keeps, negative ELU outputs included
    assert (elu[sure & keep] < 0).any() and (out[sure & keep & (elu < 0)] < 0).all()
    plain = backward(adj, Sg, asg, adg, heads, ELU, Cg)
    zero = backward(adj, Sg, asg, adg, heads, ELU_DROP, Cg, p_feat=0.0, fkey=FKEY)
    assert all(torch.equal(plain[k], zero[k]) for k in plain)     # p_feat = 0 draws nothing


@pytest.mark.parametrize("long_threshold", [None, 8], ids=["rows", "pieces"])
@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
@pytest.mark.parametrize("heads,F", SHAPES)
def test_autograd_function_matches_the_mirror_s_autograd(heads, F, epi, long_threshold):
    m = directed_graph()
    adj = gcn_adj(m, long_threshold)
    S, a_src, a_dst, C = inputs(heads, F, seed=1)
    Sg, asg, adg, Cg = gpu(S, a_src, a_dst, C)
    kw = dict(p_feat=0.5, fkey=FKEY) if epi == ELU_DROP else {}
    keep = torch.from_numpy(A.feat_keep(FKEY, N, heads * F, 0.5)) if epi == ELU_DROP else None
    ref = references(m, S, a_src, a_dst, heads, epi, C, keep_feat=keep, p_feat=0.5 if epi == ELU_DROP else 0.0)
    got = backward(adj, Sg, asg, adg, heads, epi, Cg, **kw)
    check(got, ref, "autograd %dx%d" % (heads, F))
    assert not got["dS"][0].any() and not got["out"][0].any()     # row 0 and column 0 are empty: exact zeros both ways
    again = backward(adj, Sg, asg, adg, heads, epi, Cg, **kw)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # only the gradients that are asked for, bit-identical
    for needs in ((True, False, False), (False, True, False), (False, False, True), (False, True, True)):
        part = backward(adj, Sg, asg, adg, heads, epi, Cg, needs=needs, **kw)
        assert sorted(part) == sorted(["out"] + [k for k, need in zip(("dS", "da_src", "da_dst"), needs) if need])
        assert all(torch.equal(part[k], got[k]) for k in part), needs


@pytest.mark.parametrize("epi", list(EPIS.values()), ids=list(EPIS))
def test_padded_rows_at_an_unaligned_base_take_the_scalar_path(epi):
    heads, F, ld = 2, 12, 27
    d = heads * F
    S, a_src, a_dst, C = inputs(heads, F)
    buf = torch.zeros(N * ld + 1, device=DEV)
    view = buf[1:].as_strided((N, d), (ld, 1))
    view.copy_(S)
    assert view.data_ptr() % 16 == 4
    asg, adg, Cg = gpu(a_src, a_dst, C)
    for long_threshold in (None, 8):
        m = directed_graph()
        adj = gcn_adj(m, long_threshold)
        ref = references(m, S, a_src, a_dst, heads, epi, C)
        got = backward(adj, view, asg, adg, heads, epi, Cg)
        check(got, ref, "strided")
        aligned = backward(adj, S.to(DEV), asg, adg, heads, epi, Cg)
        check(got, tuple({k: v.cpu().double().numpy() for k, v in aligned.items()} for _ in range(2)), "strided vs aligned")
        fw = forward(adj, view, asg, adg, heads, epi)
        check(fw, ref, "strided fwd")


@pytest.mark.parametrize("heads,F", [(1, 1), (3, 6), (2, 12), (1, 130), (8, 16)])
def test_attention_vector_gradients_over_several_blocks(heads, F):
    """600 rows: nine full blocks of the column sums' 64 rows and one of 24, in up to three strips of 64 columns; rows padded to a
    stride of d + 3"""
    from ctgcn_amd import ops
    n, d = 600, heads * F
    S = torch.from_numpy(dense((n, d + 3), d))[:, :d]
    du, dv = torch.from_numpy(dense((n, heads), d + 1)), torch.from_numpy(dense((n, heads), d + 2))
    Sg, dug, dvg = torch.from_numpy(dense((n, d + 3), d)).to(DEV)[:, :d], du.to(DEV), dv.to(DEV)
    assert Sg.stride(0) == d + 3 and torch.equal(Sg.cpu(), S)
    got = dict(zip(("da_src", "da_dst"), ops._gat_da(Sg, dug, dvg, heads)))
    ref = tuple({"da_src": (a.to(t)[:, :, None] * S.to(t).reshape(n, heads, F)).sum(0).double().numpy(),
                 "da_dst": (b.to(t)[:, :, None] * S.to(t).reshape(n, heads, F)).sum(0).double().numpy()}
                for t, a, b in ((torch.float64, du, dv), (torch.float32, du, dv)))
    check(got, ref, "da %dx%d" % (heads, F))
    again = ops._gat_da(Sg, dug, dvg, heads)
    assert torch.equal(got["da_src"], again[0]) and torch.equal(got["da_dst"], again[1])
    only_src, none = ops._gat_da(Sg, dug, None, heads)
    assert none is None and torch.equal(only_src, got["da_src"])
    none, only_dst = ops._gat_da(Sg, None, dvg, heads)
    assert none is None and torch.equal(only_dst, got["da_dst"])


def test_input_checks():
    from ctgcn_amd import ops
    m = graph(8)
    adj = gcn_adj(m)
    S, a_src, a_dst, _ = gpu(*inputs(2, 12))
    with pytest.raises(ValueError):
        ops.gat_conv(S[:-1], a_src, a_dst, adj, 2)
    with pytest.raises(ValueError):
        ops.gat_conv(S, a_src, a_dst, adj, 5)
    with pytest.raises(ValueError):
        ops.gat_conv(S, a_src[:, :-1], a_dst, adj, 2)
    with pytest.raises(ValueError):
        ops.gat_conv(S, a_src, a_dst, adj, 2, epi=3)
    with pytest.raises(ValueError):
        ops.gat_conv(S, a_src, a_dst, adj, 2, p_att=1.0)
    with pytest.raises(ValueError):
        ops.gat_conv(S, a_src, a_dst, adj, 2, alpha=float("nan"))
    with pytest.raises(TypeError):
        ops.gat_conv(S.double(), a_src, a_dst, adj, 2)
    # stored entries count even when their value is 0: only the pattern is read
    zeroed = ops.GcnAdj(adj.row_ptr, adj.col, torch.zeros_like(adj.val))
    assert torch.equal(ops.gat_conv(S, a_src, a_dst, zeroed, 2), ops.gat_conv(S, a_src, a_dst, adj, 2))
