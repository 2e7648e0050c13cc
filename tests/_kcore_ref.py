"""Exact host models of the nested k-core ingest (ctgcn_amd/core_adj.py: CoreAdj.from_graph) and the graph families whose core
numbers are known in closed form.  Plain numpy / Python: nothing here touches the library under test.

  core_numbers      Batagelj-Zaversnik bucket peel (the algorithm behind networkx.core_number); stored diagonal entries are ignored,
                    as kcore_init_kernel and kcore_hindex_init_kernel ignore them.
  edge_levels_ref   level(e) = min(core[row], core[col]) and its histogram, binned at min(level, hist_len - 1).
  slot_reorder_ref  per row, a STABLE sort by table[min(level, len(table) - 1)].
  builders          (scipy CSR with sorted indices and unit weights, int32 core numbers): K_{a,b} -> min(a, b), K_m -> m - 1,
                    path -> 1 (a single vertex: 0), cycle -> 2, star -> 1, isolated -> 0, a clique with pendant leaves on one vertex,
                    and disjoint unions of these under a seeded vertex permutation (a component's core numbers do not depend on
                    the others)."""
import numpy as np
import scipy.sparse as sp


# ------------------------------------------------------------------------------------------ models
def core_numbers(indptr, indices):
    """int32[n] core numbers of the simple undirected graph whose symmetric CSR structure is (indptr, indices)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    n = len(indptr) - 1
    if n == 0:
        return np.zeros(0, dtype=np.int32)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    off = indices != rows
    deg = np.bincount(rows[off], minlength=n).astype(np.int64)
    md = int(deg.max(initial=0))
    start = np.zeros(md + 2, dtype=np.int64)                    # start[d]: first position of the degree-d bucket in vert
    np.cumsum(np.bincount(deg, minlength=md + 1), out=start[1:])
    vert = np.argsort(deg, kind="stable")
    pos = np.empty(n, dtype=np.int64)
    pos[vert] = np.arange(n)
    deg, vert, pos, start = deg.tolist(), vert.tolist(), pos.tolist(), start[:-1].tolist()
    ip, ix = indptr.tolist(), indices.tolist()
    for i in range(n):
        v = vert[i]
        dv = deg[v]
        for e in range(ip[v], ip[v + 1]):
            u = ix[e]
            if u != v and deg[u] > dv:
                du, pu = deg[u], pos[u]
                pw = start[du]                                  # swap u with the first vertex of its bucket, then shrink the bucket
                w = vert[pw]
                if w != u:
                    vert[pu], vert[pw] = w, u
                    pos[u], pos[w] = pw, pu
                start[du] += 1
                deg[u] = du - 1
    return np.asarray(deg, dtype=np.int32)


def edge_levels_ref(indptr, indices, val, core, hist_len):
    """(level int32[nnz], count int64[hist_len], wsum longdouble[hist_len]); val may be None (wsum is then all zero)."""
    indptr = np.asarray(indptr, dtype=np.int64)
    indices = np.asarray(indices, dtype=np.int64)
    core = np.asarray(core, dtype=np.int64)
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    level = np.minimum(core[rows], core[indices])
    bins = np.minimum(level, hist_len - 1)
    count = np.bincount(bins, minlength=hist_len).astype(np.int64)
    wsum = np.zeros(hist_len, dtype=np.longdouble)
    if val is not None and len(bins):
        order = np.argsort(bins, kind="stable")
        w = np.asarray(val)[order].astype(np.longdouble)
        first = np.flatnonzero(np.r_[True, np.diff(bins[order]) != 0])
        wsum[bins[order][first]] = np.add.reduceat(w, first)
    return level.astype(np.int32), count, wsum


def slot_reorder_ref(indptr, col, val, level, table):
    """(col_out, val_out, slot_out uint8): every row's entries stably sorted by their slot"""
    indptr = np.asarray(indptr, dtype=np.int64)
    col, val, table = np.asarray(col), np.asarray(val), np.asarray(table)
    slot = table[np.minimum(np.asarray(level, dtype=np.int64), len(table) - 1)].astype(np.uint8)
    col_out, val_out, slot_out = np.empty_like(col), np.empty_like(val), np.empty_like(slot)
    for r in range(len(indptr) - 1):
        s, e = indptr[r], indptr[r + 1]
        o = s + np.argsort(slot[s:e], kind="stable")
        col_out[s:e], val_out[s:e], slot_out[s:e] = col[o], val[o], slot[o]
    return col_out, val_out, slot_out


# ---------------------------------------------------------------------------------------- builders
def _csr(indptr, indices, n):
    indices = np.asarray(indices, dtype=np.int32)
    return sp.csr_matrix((np.ones(len(indices), dtype=np.float32), indices, np.asarray(indptr, dtype=np.int32)), shape=(n, n))


def _from_pairs(a, b, n):
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    m = sp.coo_matrix((np.ones(2 * len(a), dtype=np.float32), (np.concatenate([a, b]), np.concatenate([b, a]))), shape=(n, n)).tocsr()
    m.sort_indices()
    return m


def bipartite(a, b):
    """K_{a,b}: vertices 0 .. a-1 (degree b) against a .. a+b-1 (degree a); core min(a, b)"""
    n = a + b
    indptr = np.concatenate([np.arange(a + 1, dtype=np.int64) * b, a * b + np.arange(1, b + 1, dtype=np.int64) * a])
    indices = np.concatenate([np.tile(np.arange(a, n, dtype=np.int32), a), np.tile(np.arange(a, dtype=np.int32), b)])
    return _csr(indptr, indices, n), np.full(n, min(a, b), dtype=np.int32)


def clique(m):
    """K_m: core m - 1"""
    full = np.tile(np.arange(m, dtype=np.int32), m).reshape(m, m)
    indices = full[~np.eye(m, dtype=bool)]
    return _csr(np.arange(m + 1, dtype=np.int64) * (m - 1), indices, m), np.full(m, m - 1, dtype=np.int32)


def path(n):
    """vertices 0 - 1 - ... - n-1 in id order; core 1 (a single vertex: 0)"""
    a = np.arange(n - 1)
    return _from_pairs(a, a + 1, n), np.full(n, 1 if n > 1 else 0, dtype=np.int32)


def cycle(n):
    """n >= 3 vertices; core 2"""
    assert n >= 3
    a = np.arange(n)
    return _from_pairs(a, (a + 1) % n, n), np.full(n, 2, dtype=np.int32)


def star(leaves):
    """hub 0 and `leaves` >= 1 leaves; core 1"""
    assert leaves >= 1
    return _from_pairs(np.zeros(leaves, dtype=np.int64), 1 + np.arange(leaves), leaves + 1), np.full(leaves + 1, 1, dtype=np.int32)


def clique_with_pendants(m, leaves, clique_last=True):
    """K_m with `leaves` degree-1 vertices hung on ONE of its vertices (the hub, a list of m - 1 + leaves entries of which exactly
    the m - 1 clique entries decide its core number): core m - 1 on the clique, 1 on the leaves.  clique_last: the leaves take the
    ids 0 .. leaves-1, so the entries that matter close the hub's list; else they open it."""
    assert m >= 3 and leaves >= 1
    n = m + leaves
    cl = (leaves if clique_last else 0) + np.arange(m)
    lf = (0 if clique_last else m) + np.arange(leaves)
    i, j = np.triu_indices(m, 1)
    core = np.ones(n, dtype=np.int32)
    core[cl] = m - 1
    return _from_pairs(np.concatenate([cl[i], np.full(leaves, cl[0])]), np.concatenate([cl[j], lf]), n), core


def broom(leaves, u_last=True, c=5, m=12):
    """A vertex v with `leaves` degree-1 neighbours and one more, u; u also touches c vertices of a K_m (m > c + 1).  Cores: leaves
    and v 1, u c, the clique m - 1.  u has no slack: it reaches c only if v's removal at level 1 is counted — v's list has
    leaves + 1 entries and u closes it (u_last) or opens it."""
    assert leaves >= 1 and m > c + 1 >= 2
    n = leaves + m + 2
    if u_last:
        lf, v, cl, u = np.arange(leaves), leaves, leaves + 1 + np.arange(m), leaves + m + 1
    else:
        u, v, lf, cl = 0, 1, 2 + np.arange(leaves), 2 + leaves + np.arange(m)
    i, j = np.triu_indices(m, 1)
    a = np.concatenate([cl[i], np.full(leaves, v), [v], np.full(c, u)])
    b = np.concatenate([cl[j], lf, [u], cl[:c]])
    core = np.ones(n, dtype=np.int32)
    core[cl], core[u] = m - 1, c
    return _from_pairs(a, b, n), core


def isolated(n):
    return sp.csr_matrix((n, n), dtype=np.float32), np.zeros(n, dtype=np.int32)


def matching(pairs):
    """perfect matching v <-> v + pairs; core 1"""
    a = np.arange(pairs, dtype=np.int32)
    return _csr(np.arange(2 * pairs + 1, dtype=np.int64), np.concatenate([a + pairs, a]), 2 * pairs), np.full(2 * pairs, 1, dtype=np.int32)


def union(parts, seed=None):
    """Disjoint union of (csr, core) pairs; with a seed, the vertices are renumbered by a seeded permutation, so that consecutive
    ids (a block's range) mix the families."""
    mats, cores = [p[0] for p in parts], [p[1] for p in parts]
    m = sp.block_diag(mats, format="csr", dtype=np.float32) if len(mats) > 1 else sp.csr_matrix(mats[0])
    core = np.concatenate(cores).astype(np.int32)
    if seed is not None:
        perm = np.random.default_rng(seed).permutation(m.shape[0])         # new id p holds old vertex perm[p]
        m = m[perm][:, perm].tocsr()
        core = core[perm]
    m.sort_indices()
    return m, core


def cut(csr, n):
    """the subgraph induced by the first n vertices (its core numbers are no closed form: use core_numbers)"""
    m = sp.csr_matrix(csr)[:n][:, :n].tocsr()
    m.sort_indices()
    return m


def with_weights(csr, lo=1, hi=8):
    """symmetric integer weights lo .. hi that depend on the unordered pair only"""
    coo = sp.csr_matrix(csr).tocoo()
    w = lo + (coo.row.astype(np.int64) * coo.col + coo.row + coo.col) % (hi - lo + 1)
    m = sp.csr_matrix((w.astype(np.float32), (coo.row, coo.col)), shape=coo.shape)
    m.sort_indices()
    return m


# the graph of the cap tests and of the end-to-end ingest test: levels 1, 20 and 39 only
CAPS_PATH = 300


def caps_graph():
    return union([clique(40), bipartite(20, 1030), path(CAPS_PATH)], seed=20)


def mixed_parts(extra_isolated=0):
    """a clique (short lists), a cycle and a star whose hub has a long list, and isolated vertices: 1 100 vertices before the extra"""
    return [clique(17), cycle(500), star(400), isolated(182 + extra_isolated)]
