"""The walk corpus, the positive / negative draws and the epoch offset scan (ctgcn_walks.hip, ctgcn_epoch.hip) against the host
model tests/_sampling_ref.py.  The counter RNG is integer arithmetic plus exact conversions and every draw one IEEE multiply and
a compare, so every assertion here is EQUALITY; test_sampling_ref_host.py ties the model to things outside this project."""
import numpy as np
import pytest
import torch

import _sampling_ref as R
from conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a).astype(dtype))).to(DEV)


def _corpus(row_ptr, col, val, L, W, weighted, seed, per_round=10):
    from ctgcn_amd.walks import random_walk_corpus
    pairs, freq = random_walk_corpus(_dev(row_ptr, np.int32), _dev(col, np.int32), _dev(val, np.float32), walk_length=L, walk_time=W,
                                     weighted=weighted, seed=seed, walks_per_round=per_round)
    return pairs.row_ptr.cpu().numpy(), pairs.col.cpu().numpy(), freq.cpu().numpy()


def _model(row_ptr, col, val, L, W, weighted, seed):
    cumw = R.row_cumsum(row_ptr, np.asarray(val, dtype=np.float32))
    _, _, freq, prp, pc = R.walks(row_ptr, col, cumw, L, W, seed, weighted)
    return prp, pc, freq


def _same(got, want, what):
    for g, w, name in zip(got, want, ("pair row_ptr", "pair col", "freq")):
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differs from the host model" % (what, name)


def _uci():
    from ctgcn_amd.utils import symmetric_csr_from_rows
    snaps = load_golden("uci_snapshots.npz")
    adj = symmetric_csr_from_rows(snaps["t6_src"], snaps["t6_dst"], snaps["t6_w"], len(snaps["node_names"])).tocsr()
    adj.sort_indices()
    return adj.indptr.astype(np.int64), adj.indices.astype(np.int64), adj.data.astype(np.float32)


def _hub_graph(seed=21):
    """~20 000 nodes, out-degrees ~ a power law, integer weights 1..99; NOT symmetric.  Row 0 is a hub of >= 5 000 entries; nodes
    n-40..n-1 have no out-edges (the last 20 of them no in-edges either: isolated); node 1's only neighbour is the dead end n-40;
    every row r = 3 (mod 7) of degree >= 4 has leading and trailing weight 0.  Nodes 10 000..17 999 are spokes whose only neighbour is
    the hub, so the hub row is drawn from ~10^5 times: a weighted draw lands exactly on a prefix sum with probability ~ deg / 2**24,
    and only a long row drawn often has such ties at all (they are what tells `cumw > target` from `cumw >= target`)."""
    rng = np.random.default_rng(seed)
    n = 20000
    deg = np.minimum((2.0 / rng.random(n) ** 0.8).astype(np.int64), 400)
    deg[0] = 8000
    deg[10000:18000] = 1
    deg[n - 40:] = 0
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n - 20, size=len(src))
    dst[(src >= 10000) & (src < 18000)] = 0
    keep = src != 1
    keys = np.unique(np.concatenate([src[keep] * n + dst[keep], [1 * n + (n - 40)]]))
    src, col = keys // n, keys % n
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(src, minlength=n), out=row_ptr[1:])
    val = rng.integers(1, 100, size=len(col)).astype(np.float32)
    d = np.diff(row_ptr)
    zr = np.flatnonzero((np.arange(n) % 7 == 3) & (d >= 4))
    val[row_ptr[zr]] = 0
    val[row_ptr[zr + 1] - 1] = 0
    assert d[0] >= 5000 and len(zr) > 100 and d[1] == 1 and col[row_ptr[1]] == n - 40 and d[n - 40] == 0
    assert not np.isin(np.arange(n - 20, n), col).any()
    assert d.max() * 99 < 2 ** 24                                          # the documented exact domain of the fp32 prefix sums
    return row_ptr, col, val


@pytest.mark.parametrize("weighted", [True, False])
def test_uci_corpus_equals_model_for_every_round_size(weighted):
    """walk_time 10 cut into rounds of 10, 3, 1 and 7 walks: the corpus must not depend on the cut (first_walk offset) and must be
    the model's, which knows no rounds"""
    row_ptr, col, val = _uci()
    want = _model(row_ptr, col, val, 5, 10, weighted, 1)
    assert want[0][-1] > 5000 and want[2].sum() > 0
    runs = []
    for per_round in (10, 3, 1, 7):
        got = _corpus(row_ptr, col, val, 5, 10, weighted, 1, per_round)
        _same(got, want, "walks_per_round=%d" % per_round)
        runs.append(got)
    for other in runs[1:]:
        _same(other, runs[0], "round sizes among themselves")


@pytest.mark.parametrize("weighted", [True, False])
def test_hub_graph_corpus_equals_model(weighted):
    row_ptr, col, val = _hub_graph()
    want = _model(row_ptr, col, val, 5, 10, weighted, 0xDEADBEEFCAFEF00D)     # a seed with the top bit set
    for per_round in (10, 3):
        _same(_corpus(row_ptr, col, val, 5, 10, weighted, 0xDEADBEEFCAFEF00D, per_round), want, "hub graph, walks_per_round=%d" % per_round)
    n = len(row_ptr) - 1
    if weighted:                                                           # the weights matter on this graph (UCI's are all 1)
        assert not np.array_equal(_model(row_ptr, col, val, 5, 10, False, 0xDEADBEEFCAFEF00D)[2], want[2])
    assert np.all(want[2][n - 20:] == 0) and np.all(np.diff(want[0])[n - 20:] == 0)      # isolated nodes
    assert want[0][2] - want[0][1] >= 1                                                 # node 1 pairs with its dead-end neighbour


def test_row_cumsum_kernel_is_bit_identical_to_sequential_float32():
    from ctgcn_amd import _lib, ops
    from ctgcn_amd._lib import check, ptr
    row_ptr, col, val = _hub_graph()
    for v in (val, (val * np.float32(0.37) + np.float32(0.013)).astype(np.float32)):     # exact integers; fractions (order matters)
        rp, vv = _dev(row_ptr, np.int32), _dev(v, np.float32)
        out = torch.full_like(vv, float("nan"))
        with torch.cuda.device(DEV):
            check(_lib.load().ctgcn_row_cumsum_f32(len(row_ptr) - 1, ptr(rp), ptr(vv), ptr(out), ops._stream()), "ctgcn_row_cumsum_f32")
        assert np.array_equal(out.cpu().numpy().view(np.uint32), R.row_cumsum(row_ptr, v).view(np.uint32))


@pytest.mark.parametrize("L,W", [(1, 10), (31, 2), (5, 1)])
@pytest.mark.parametrize("weighted", [True, False])
def test_walk_length_and_walk_time_limits(L, W, weighted):
    row_ptr, col, val = _uci()
    _same(_corpus(row_ptr, col, val, L, W, weighted, 7, 3), _model(row_ptr, col, val, L, W, weighted, 7), "L=%d W=%d" % (L, W))


def test_walk_length_32_is_refused():
    from ctgcn_amd._lib import CtgcnHipError
    row_ptr, col, val = _uci()
    with pytest.raises(CtgcnHipError, match=r"code -1\)"):                   # CTGCN_E_INVALID
        _corpus(row_ptr, col, val, 32, 1, True, 7)


@pytest.mark.parametrize("weighted", [True, False])
@pytest.mark.parametrize("n", [1, 50])
def test_single_node_and_edgeless_graphs(n, weighted):
    row_ptr, col, val = np.zeros(n + 1, dtype=np.int64), np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.float32)
    got = _corpus(row_ptr, col, val, 5, 10, weighted, 3, 3)
    _same(got, _model(row_ptr, col, val, 5, 10, weighted, 3), "edgeless n=%d" % n)
    assert got[0].tolist() == [0] * (n + 1) and got[1].size == 0 and not got[2].any()


# ---------------------------------------------------------------------------------------------------------------- draws
def _pair_mix(n, num, seed, hubs=0):
    """the degree mix of test_gpu_epoch_loss._pairs (0, 1..num, num+1..4num-1), plus `hubs` rows of degree 5 000"""
    rng = np.random.default_rng(seed)
    kind = rng.integers(0, 3, size=n)
    deg = np.where(kind == 0, 0, np.where(kind == 1, rng.integers(1, num + 1, size=n), rng.integers(num + 1, 4 * num, size=n)))
    if hubs:
        deg[rng.choice(n, size=hubs, replace=False)] = 5000
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=row_ptr[1:])
    col = rng.integers(0, n, size=int(row_ptr[-1]))
    return row_ptr, col


def _loss(row_ptr, col, table, num):
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import WalkPairs
    return NegativeSamplingLoss([WalkPairs(_dev(row_ptr, np.int32), _dev(col, np.int32))], [_dev(table, np.int32)], neg_num=num, Q=3.5)


def _seeds(rng, B):
    s = [int(x) for x in rng.integers(0, 2 ** 64, size=B, dtype=np.uint64)]
    if B:
        s[0] = 2 ** 64 - 1
    if B > 1:
        s[-1] = 2 ** 63
    return s


def _eq(t, a):
    return t.dtype == torch.int64 and t.shape == a.shape and np.array_equal(t.cpu().numpy(), a)


@pytest.mark.parametrize("n,num,bs,hubs,table_len", [
    (1000, 5, 96, 0, 7),            # the epoch-loss tests' shape: partial last batch, colliding negatives
    (700, 5, 1, 0, 5),              # one position per batch; table_len == num (every draw is a permutation of the table)
    (4097, 20, 2048, 6, 300),       # rows of degree 5 000 against num 20; the last batch holds ONE position
    (2048, 8, 2048, 0, 64),         # exactly one full batch
])
def test_batched_draws_equal_model(n, num, bs, hubs, table_len):
    rng = np.random.default_rng(n + num)
    row_ptr, col = _pair_mix(n, num, n, hubs)
    table = rng.integers(0, n, size=table_len)
    perm = rng.permutation(n)
    B = -(-n // bs)
    seeds = _seeds(rng, B)
    assert max(seeds) >= 2 ** 63
    total, offsets, boff, node, pos, neg = _loss(row_ptr, col, table, num).batched_sample_indices(0, _dev(perm, np.int64), bs, seeds)
    w_node, w_pos, w_off, w_boff = R.pos_draws(perm, bs, seeds, row_ptr, col, num)
    assert total == w_off[-1] and total > 0
    assert _eq(offsets, w_off), "offsets"
    assert _eq(boff, w_boff), "batch offsets"
    assert _eq(node, w_node), "node indices"
    assert _eq(pos, w_pos), "positive draws"
    assert _eq(neg, np.stack([R.neg_draws(s, table, num) for s in seeds])), "negative draws"
    if hubs:
        assert n % bs == 1 and (np.diff(row_ptr) == 5000).sum() == hubs


@pytest.mark.parametrize("seed", [0, 12345, 2 ** 63, 2 ** 64 - 1])
def test_single_batch_draws_equal_model(seed):
    num, n = 20, 3000
    rng = np.random.default_rng(5)
    row_ptr, col = _pair_mix(n, num, 6, hubs=3)
    hub = np.flatnonzero(np.diff(row_ptr) == 5000)
    batch = np.concatenate([hub, rng.choice(np.setdiff1d(np.arange(n), hub), size=297, replace=False)])[rng.permutation(300)]
    for table in (rng.integers(0, n, size=1000), rng.integers(0, n, size=num)):        # a long table; table_len == num
        cnt, node, pos, neg = _loss(row_ptr, col, table, num).sample_indices(0, _dev(batch, np.int64), seed=seed)
        w_node, w_pos, w_off, _ = R.pos_draws(batch, len(batch), [seed], row_ptr, col, num)
        assert cnt == w_off[-1] and _eq(node, w_node) and _eq(pos, w_pos)
        assert _eq(neg, R.neg_draws(seed, table, num))


def test_table_shorter_than_num_is_refused():
    from ctgcn_amd._lib import CtgcnHipError
    row_ptr, col = _pair_mix(500, 5, 1)
    loss = _loss(row_ptr, col, np.arange(4), 5)
    perm = _dev(np.arange(500), np.int64)
    with pytest.raises(CtgcnHipError, match=r"code -1\)"):
        loss.sample_indices(0, perm[:96], seed=1)
    with pytest.raises(CtgcnHipError, match=r"code -1\)"):
        loss.batched_sample_indices(0, perm, 96, list(range(6)))


def test_no_positions():
    row_ptr, col = _pair_mix(500, 5, 1)
    total, offsets, boff, node, pos, neg = _loss(row_ptr, col, np.arange(9), 5).batched_sample_indices(0, _dev(np.zeros(0), np.int64), 96, [])
    assert total == 0 and node is None and pos is None and tuple(neg.shape) == (0, 5)
    assert offsets.tolist() == [0] and boff.tolist() == [0]


@pytest.mark.parametrize("P", [2047, 2048, 2049, 524288, 524289, 1200000])
def test_offset_scan_equals_cumsum(P):
    """ctgcn_neg_sampling_offsets_batched alone (nothing consumes the offsets).  One scan tile is 2 048 positions and the tile sums
    are scanned 256 at a time: 524 288 positions fill one such chunk exactly, 524 289 need the carry into a second one."""
    from ctgcn_amd import _lib, ops
    from ctgcn_amd._lib import check, ptr
    num, n, bs = 8, 5000, 2048
    rng = np.random.default_rng(P)
    row_ptr, _ = _pair_mix(n, num, 2)
    perm = rng.integers(0, n, size=P)
    lib = _lib.load()
    B = -(-P // bs)
    d_perm, d_rp = _dev(perm, np.int64), _dev(row_ptr, np.int32)
    offsets = torch.full((P + 1,), -1, dtype=torch.int64, device=DEV)
    boff = torch.full((B + 1,), -1, dtype=torch.int64, device=DEV)
    with torch.cuda.device(DEV):
        ws = torch.empty(lib.ctgcn_epoch_scan_workspace_bytes(P), dtype=torch.uint8, device=DEV)
        check(lib.ctgcn_neg_sampling_offsets_batched(P, ptr(d_perm), ptr(d_rp), num, bs, ptr(offsets), ptr(boff), ptr(ws), ws.numel(),
                                                     ops._stream()), "ctgcn_neg_sampling_offsets_batched")
    want = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(np.minimum(np.diff(row_ptr)[perm], num), out=want[1:])
    assert want[-1] > 3 * P
    assert _eq(offsets, want), "offsets"
    assert _eq(boff, want[np.minimum(np.arange(B + 1) * bs, P)]), "batch offsets"
