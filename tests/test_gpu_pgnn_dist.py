"""ops.pgnn_anchor_dist (ctgcn_pgnn.hip) against the host model of the pass (_pgnn_ref.host_dist, which tests/test_pgnn_host.py pins to
the reference's recorded dist_max / dist_argmax): exact equality of the levels, the bits of dist_max, the positions and the node ids,
twice over (the results do not depend on the order of execution), on graphs chosen for what can go wrong: a 300-node path (levels
past 255), a star whose hub has more entries than any long-row threshold, two components plus isolated nodes with a set that misses
one component (unreached: 0 and position 0), a CSR with self-loops and repeated entries, n = 1, 2, 65, and the three UCI snapshots
against the recorded results of the reference itself.  Cutoffs -1, 1, 2; 1, 33 and 100 anchor sets; sets of 1 and n / 2 members; one
set that lists a member twice."""
import numpy as np
import pytest
import torch

import _pgnn_ref as P

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def csr(n, pairs, symmetric=True):
    """(indptr, indices) in the order given (no sorting, no merging of repeats)"""
    pairs = list(pairs)
    if symmetric:
        pairs = pairs + [(b, a) for a, b in pairs]
    rows = np.asarray([a for a, _ in pairs], dtype=np.int64)
    cols = np.asarray([b for _, b in pairs], dtype=np.int64)
    order = np.argsort(rows, kind="stable")
    indptr = np.zeros(n + 1, dtype=np.int64)
    indptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return indptr.astype(np.int32), cols[order].astype(np.int32)


def graphs():
    rng = np.random.default_rng(3)
    out = {"path300": csr(300, [(i, i + 1) for i in range(299)]),
           "star3000": csr(3001, [(0, i) for i in range(1, 3001)]),
           "n1": csr(1, []), "n2": csr(2, [(0, 1)]),
           "n65": csr(65, [(int(a), int(b)) for a, b in rng.integers(0, 65, (90, 2))])}
    # nodes 0..19 a ring, 20..39 a tree, 40..47 isolated
    out["components"] = csr(48, [(i, (i + 1) % 20) for i in range(20)] + [(20 + (i - 1) // 2, 20 + i) for i in range(1, 20)])
    # self-loops, the same pair several times, and one direction stored twice
    out["loops"] = csr(30, [(i, i) for i in range(0, 30, 3)] + [(i, i + 1) for i in range(29)] * 2 + [(3, 17), (3, 17), (8, 25)])
    return out


def anchor_sets(name, n, A):
    rng = np.random.default_rng(1000 + n + A)
    sets = []
    for a in range(A):
        size = 1 if a % 2 else max(1, n // 2)
        sets.append(rng.choice(n, size=size, replace=False).astype(np.int64))
    if name == "components":
        sets[0] = np.arange(20, 30, dtype=np.int64)              # the tree alone: the ring and the isolated nodes stay unreached
    sets[-1] = np.concatenate((sets[-1][-1:], sets[-1], sets[-1][:1]))          # a member at two positions: the smaller one counts
    return sets


def run(indptr, indices, sets, cutoff):
    from ctgcn_amd import ops
    rp, col = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    first = ops.pgnn_anchor_dist((rp, col), sets, cutoff, node_ids=True)
    again = ops.pgnn_anchor_dist((rp, col), [torch.from_numpy(s).to(DEV) for s in sets], cutoff, node_ids=True)
    assert all(torch.equal(a, b) for a, b in zip(first, again))
    assert ops.pgnn_anchor_dist((rp, col), sets, cutoff)[3] is None
    return [t.cpu().numpy() for t in first]


@pytest.mark.parametrize("name", list(graphs()))
def test_levels_distances_positions_and_node_ids_equal_the_host_model(name):
    indptr, indices = graphs()[name]
    n = len(indptr) - 1
    seen_unreached = False
    for A in (1, 33, 100):
        sets = anchor_sets(name, n, A)
        for cutoff in (-1, 1, 2):
            level, dist, pos, node = run(indptr, indices, sets, cutoff)
            want = P.host_dist(indptr, indices, sets, cutoff)
            assert level.dtype == np.int32 and dist.dtype == np.float32 and pos.dtype == np.int32 and node.dtype == np.int32
            assert np.array_equal(level, want[0]), (name, A, cutoff)
            assert np.array_equal(dist.view(np.uint32), want[1].view(np.uint32)), (name, A, cutoff)
            assert np.array_equal(pos, want[2]) and np.array_equal(node, want[3]), (name, A, cutoff)
            assert level.max() <= (cutoff if cutoff > 0 else n)
            unreached = level < 0
            assert not dist[unreached].any() and not pos[unreached].any()
            seen_unreached |= bool(unreached.any())
            if name == "components" and cutoff < 0:
                assert (level[:20, 0] == -1).all() and (level[40:, 0] == -1).all() and (level[20:40, 0] >= 0).all()
    if name in ("components", "star3000", "path300"):
        assert seen_unreached


def test_a_path_s_far_end_is_299_hops_away():
    """levels are 32-bit: nothing wraps at 255"""
    indptr, indices = graphs()["path300"]
    level, dist, pos, node = run(indptr, indices, [np.asarray([0]), np.asarray([299, 0, 299])], -1)
    assert np.array_equal(level[:, 0], np.arange(300)) and level[299, 0] == 299 and dist[299, 0] == np.float32(1) / np.float32(300)
    assert np.array_equal(level[:, 1], np.minimum(np.arange(300), 299 - np.arange(300)))
    assert pos[149, 1] == 1 and pos[150, 1] == 0 and node[149, 1] == 0 and node[150, 1] == 299    # node 299 sits at positions 0 and 2


@pytest.mark.parametrize("cutoff", P.CUTOFFS)
def test_the_uci_snapshots_equal_the_reference_s_recorded_results(cutoff):
    from ctgcn_amd import ops
    from ctgcn_amd.baseline import get_dist_max, precompute_dist_data
    g = P.fixture()
    sets = P.anchor_sets(g)
    edges = []
    for t in range(P.T):
        indptr, indices = P.pattern(t)
        level, dist, pos, node = run(indptr.astype(np.int32), indices.astype(np.int32), sets, cutoff)
        want_level, want_dist, want_pos = P.recorded_dist(g, t, cutoff)
        assert np.array_equal(level, want_level) and np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
        assert np.array_equal(pos.astype(np.int64), want_pos)
        coo = P.G.raw_csr(t).tocoo()
        keep = coo.row < coo.col                                  # one direction, as an edge list has it
        edges.append(torch.from_numpy(np.vstack((coo.row[keep], coo.col[keep])).astype(np.int64)).to(DEV))
    # the module's own route: handles from the edge lists, plain float32 / int64 tensors out, the prepared index registered on the way
    handles = precompute_dist_data(edges, P.N, cutoff)
    dms, das = get_dist_max(sets, handles, DEV)
    for t in range(P.T):
        _, want_dist, want_pos = P.recorded_dist(g, t, cutoff)
        assert dms[t].dtype == torch.float32 and das[t].dtype == torch.int64
        assert np.array_equal(dms[t].cpu().numpy().view(np.uint32), want_dist.view(np.uint32)) and np.array_equal(das[t].cpu().numpy(), want_pos)
        prep = ops.pgnn_prepare(dms[t], das[t])
        values, inverse = torch.unique(dms[t], return_inverse=True)
        assert torch.equal(prep.values[prep.lvl.long()], dms[t]) and prep.values.numel() == values.numel() + (0 if bool((dms[t] == 0).any()) else 1)
    single = get_dist_max(sets, handles[0], DEV, node_ids=True)
    members = [np.asarray(s) for s in sets]
    want_pos = P.recorded_dist(g, 0, cutoff)[2]
    assert torch.equal(single[0], dms[0])
    assert all(np.array_equal(single[1][:, a].cpu().numpy(), members[a][want_pos[:, a]]) for a in range(len(sets)))


def test_bad_anchor_sets_are_refused():
    from ctgcn_amd import _lib, ops
    indptr, indices = graphs()["n65"]
    rp, col = torch.from_numpy(indptr).to(DEV), torch.from_numpy(indices).to(DEV)
    for bad in ([np.asarray([65])], [np.asarray([3]), np.asarray([-1])]):
        with pytest.raises(_lib.CtgcnHipError, match="member outside"):
            ops.pgnn_anchor_dist((rp, col), bad, -1)
    with pytest.raises(ValueError):
        ops.pgnn_anchor_dist((rp, col), [], -1)
    level, dist, pos, node = ops.pgnn_anchor_dist((rp, col), [np.asarray([], dtype=np.int64), np.asarray([5])], -1, node_ids=True)
    assert (level[:, 0] == -1).all() and not dist[:, 0].any() and not pos[:, 0].any() and not node[:, 0].any()       # an empty set reaches nothing
