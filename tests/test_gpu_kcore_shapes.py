"""ops.kcore at every dispatch boundary of its two algorithms, against closed-form core numbers (tests/_kcore_ref.py; its Python
Batagelj-Zaversnik peel where a graph is cut and the closed form is lost).  Every comparison is np.array_equal on the whole core
array plus the returned maximum.

What each group reaches (ctgcn_amd/csrc/ctgcn_hip.hip):
  bipartite classes  kcore_hindex_kernel's list-length classes at their edges — one lane up to KH_TINY = 16 entries, a 16-lane group up
                     to KC_LONG = 48, a wave with the LDS cache up to KH_CACHE = 1024 — and kcore_hindex_hub_kernel above that: one and
                     two laps of its 2 048-entry gather and 1 024-entry marking loops (1 025, 2 048 | 2 049), the bin ownership
                     W = ceil(B / 256) at 5 | 6 (1 280 | 1 281), the clip of the estimate at KH_BINS = 8 192 (8 191, 8 192, 8 193) and
                     the grid-stride over hubs (K_{1025,1025}: 2 050 active hubs on 1 024 blocks).  K_{a,b} puts a vertices of degree b
                     and b of degree a at core min(a, b), so one side crosses an edge while the other stays in a chosen class.
  cliques, K_5 + leaves  the same edges with lists whose every entry (K_m, K_{1024,1024}), or whose first | last four entries, decide the
                     core number: the large side of a K_{3,b} keeps its core number when an entry of its list is lost.
  vertex counts      n against KH_CHUNK = 1 024 vertices a block, and the word | byte paths of the flag read (v0 + 3 < n).
  sweep batches      the host loop queues 48 sweeps, then batches of 32; a path needs about one sweep per two hops, and in-place
                     updates make the exact count run-dependent, so the lengths straddle 48 and 80 sweeps instead of naming one.
  caps               the peel (0 < cap <= 16) and the capped h-index (cap >= 17) on one graph with cores 1, 20 and 39; the peel's
                     16-lane pass | wave pass at KC_LONG.
  peel queue         kcore_level_kernel's LDS queue (KC_QCAP = 8 192), its linked spill stack and the refill; blocks capped at 2 048
                     (chunk > 1 024).
  forced algorithms  CTGCN_KCORE=peel | hindex is read once per process: one fresh child per mode (tests/_kcore_worker.py) runs the
                     peel past its first BATCH = 16 levels and the h-index at caps <= 16."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _kcore_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _kcore(csr, cap=-1):
    from ctgcn_amd import ops
    csr = sp.csr_matrix(csr)
    assert csr.has_sorted_indices
    d = torch.device("cuda:0")
    core, mx = ops.kcore(torch.from_numpy(csr.indptr.astype(np.int32)).to(d), torch.from_numpy(csr.indices.astype(np.int32)).to(d),
                         level_cap=cap)
    return core.cpu().numpy(), mx


def _check(csr, want, cap=-1, what=""):
    want = np.asarray(want, dtype=np.int32) if cap < 0 else np.minimum(np.asarray(want, dtype=np.int32), cap)
    core, mx = _kcore(csr, cap)
    assert core.dtype == np.int32
    bad = np.flatnonzero(core != want)
    assert np.array_equal(core, want), (what, cap, len(bad), bad[:8], core[bad[:8]], want[bad[:8]])
    assert mx == int(want.max(initial=0)), (what, cap, mx)


# ------------------------------------------------------------------------------------------ h-index classes, uncapped
BIPARTITE = ([(3, b) for b in (16, 17, 48, 49)] + [(a, b) for a in (3, 20, 50) for b in (1024, 1025, 2048, 2049)]
             + [(3, b) for b in (1280, 1281, 8191, 8192, 8193)] + [(1025, 1025)])


@pytest.mark.parametrize("a,b", BIPARTITE)
def test_hindex_bipartite_classes(a, b):
    csr, core = R.bipartite(a, b)
    _check(csr, core, what="K_{%d,%d}" % (a, b))
    if csr.nnz < 500000:                                        # and with the two sides mixed inside every block's range
        csr, core = R.union([(csr, core)], seed=a * 10000 + b)
        _check(csr, core, what="K_{%d,%d} permuted" % (a, b))


@pytest.mark.parametrize("m", [17, 18, 49, 50, 2050])
def test_hindex_cliques(m):
    """degree = core: every entry of the list is needed, so one dropped at a class edge (16 | 17, 48 | 49 entries) or between the
    hub kernel's gather laps (K_2050: 2 049 entries, 2 050 hubs) shows.  The large side of a K_{3,b} would not notice."""
    _check(*R.clique(m), what="K_%d" % m)


@pytest.mark.parametrize("clique_last", [True, False], ids=["needed-entries-last", "needed-entries-first"])
@pytest.mark.parametrize("deg", [16, 17, 48, 49, 1024, 1025, 2048, 2049, 8192, 8193])
def test_hindex_hub_whose_core_hangs_on_four_entries(deg, clique_last):
    """K_5 with deg - 4 leaves on one of its vertices: that vertex stays at 4 only while its four clique entries are read and
    counted, at the start or at the end of a list of every class length"""
    _check(*R.clique_with_pendants(5, deg - 4, clique_last), what="K_5 + %d leaves" % (deg - 4))


def test_hindex_full_cache_every_entry_needed():
    """K_{1024,1024}: lists of exactly KH_CACHE entries with degree = core (K_{1025,1025} is the same on the hub side of that edge)"""
    _check(*R.bipartite(1024, 1024), what="K_{1024,1024}")


def test_hindex_mixed_union():
    csr, core = R.union(R.mixed_parts(), seed=3)
    assert csr.shape[0] == 1100
    _check(csr, core, what="mixed")


# ------------------------------------------------------------------------------------------ vertex count
@pytest.mark.parametrize("n", [1, 2, 3, 5, 1023, 1024, 1025, 1027, 2049])
def test_hindex_vertex_counts(n):
    if n <= 1100:
        csr = R.cut(R.union(R.mixed_parts(), seed=3)[0], n)
        core = R.core_numbers(csr.indptr, csr.indices)
    else:
        csr, core = R.union(R.mixed_parts(n - 1100), seed=4)    # padded with isolated vertices, under the permutation
    assert csr.shape[0] == n
    if n >= 1023:
        assert core[-4:].any()                                  # the last flag word / bytes belong to vertices with edges
    _check(csr, core, what="n=%d" % n)
    if n <= 17:                                                 # the cut above has no edge left: the same cut of the unpermuted union is K_n
        csr = R.cut(R.union(R.mixed_parts())[0], n)
        assert csr.nnz == n * (n - 1)
        _check(csr, np.full(n, n - 1), what="K_n, n=%d" % n)


def test_hindex_edgeless_and_single_edge():
    _check(*R.isolated(1025), what="edgeless")
    _check(*R.path(2), what="one edge")


# ------------------------------------------------------------------------------------------ sweep batches
@pytest.mark.parametrize("lengths", [range(80, 121), range(150, 181)], ids=["first-batch-48", "second-batch-80"])
def test_hindex_paths_across_the_sweep_batches(lengths):
    for n in lengths:
        _check(*R.path(n), what="path %d" % n)


# ------------------------------------------------------------------------------------------ caps
@pytest.mark.parametrize("cap", [1, 2, 15, 16, 17, 39, 60])
def test_caps_peel_and_capped_hindex(cap):
    csr, core = R.caps_graph()
    assert int(core.max()) == 39
    _check(csr, core, cap=cap, what="caps graph")


@pytest.mark.parametrize("b", [48, 49])
def test_peel_group_and_wave_pass(b):
    _check(*R.bipartite(5, b), cap=8, what="K_{5,%d}" % b)
    _check(*R.union([R.bipartite(5, b), R.path(9)], seed=b), cap=8, what="K_{5,%d} + path" % b)


@pytest.mark.parametrize("u_last", [True, False], ids=["last-entry", "first-entry"])
@pytest.mark.parametrize("entries", [16, 17, 48, 49, 64, 65, 129])
def test_peel_relaxes_every_entry_of_a_list(entries, u_last):
    """a vertex removed at level 1 whose first | last entry is a neighbour without slack (tests/_kcore_ref.py: broom): it comes out
    one level too high if the 16-lane pass (up to KC_LONG = 48 entries) or the wave pass (64 lanes a lap) skips that entry.
    K_{5,b} cannot show this: there the long lists are walked when their neighbours are gone."""
    _check(*R.broom(entries - 1, u_last), cap=8, what="broom %d" % entries)


# ------------------------------------------------------------------------------------------ peel queue
PEEL_PATH = 50001


def test_peel_queue_spill_and_refill_on_a_long_path():
    """vertices in id order: the blocks of the two ends chase about 25 000 vertices each, one push per round — the queue passes
    KC_QCAP = 8 192 three times, each time through the spill stack and a refill"""
    _check(*R.path(PEEL_PATH), cap=2, what="path")


def test_peel_star_forest():
    hubs, leaves = 40, 20000
    h = np.repeat(np.arange(hubs), leaves)
    l = hubs + np.arange(hubs * leaves)
    n = hubs + hubs * leaves
    csr = sp.coo_matrix((np.ones(2 * len(h), dtype=np.float32), (np.concatenate([h, l]), np.concatenate([l, h]))), shape=(n, n)).tocsr()
    csr.sort_indices()
    _check(csr, np.ones(n, dtype=np.int32), cap=2, what="star forest")


def test_peel_block_cap_perfect_matching():
    """2 097 157 vertices: blocks stop at 2 048, so chunk = 1 025 > 1 024, and every vertex is claimed in the scan"""
    csr, core = R.union([R.matching(1048577), R.isolated(3)])
    assert csr.shape[0] == 2 * 1048577 + 3 and -(-csr.shape[0] // 2048) > 1024
    _check(csr, core, cap=2, what="matching")


# ------------------------------------------------------------------------------------------ forced algorithms
def _child(mode, out):
    env = dict(os.environ, CTGCN_KCORE=mode)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_kcore_worker.py"), mode, str(out)], env=env,
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, (mode, res.stdout[-1000:], res.stderr[-2000:])
    return np.load(str(out))


def test_forced_algorithms_give_the_same_integers(tmp_path):
    csr, core = R.caps_graph()
    got = _child("peel", tmp_path / "peel.npz")                 # three rounds of BATCH = 16 levels; the spill path uncapped
    assert np.array_equal(got["caps_core"], core) and int(got["caps_max"]) == 39
    assert np.array_equal(got["path_core"], np.ones(PEEL_PATH, dtype=np.int32)) and int(got["path_max"]) == 1
    got = _child("hindex", tmp_path / "hindex.npz")             # the sweeps at caps the default routes to the peel
    for cap in (1, 2, 16):
        assert np.array_equal(got["caps_core_%d" % cap], np.minimum(core, cap)), cap
        assert int(got["caps_max_%d" % cap]) == cap
