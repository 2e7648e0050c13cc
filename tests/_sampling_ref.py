"""Host model of the walk / sampler draws (ctgcn_rng.h, ctgcn_walks.hip, ctgcn_epoch.hip): plain numpy, written from the
formulas, never calling the library.  Everything here is integer arithmetic, one exact uint64 -> float64 conversion, one exact
scaling by 2**-53 and then a single IEEE multiply and a compare per draw, so the kernels are held to EQUALITY with it.

  mix64 / u01          splitmix64 finaliser and the counter RNG  u01(a, b, c) = (mix(mix(a) ^ mix(b*0x100000001b3 + c)) >> 11) * 2**-53
  row_cumsum           per-row sequential float32 prefix sums of the edge weights
  walks                the whole corpus of one snapshot: walks, frequency counts, symmetric zero-diagonal 0/1 pair CSR
  pos_draws            the positives of every position of an epoch (selection sampling, order preserving) and their offsets
  neg_draws            `num` distinct positions of the negative table by rejection

The model has no notion of rounds (walks_per_round), scan tiles or batches-per-launch: that is the point.
"""
import numpy as np

U64 = np.uint64
_GOLDEN = U64(0x9E3779B97F4A7C15)
_M1 = U64(0xBF58476D1CE4E5B9)
_M2 = U64(0x94D049BB133111EB)
_FNV = U64(0x100000001B3)
_NODE_MUL = U64(1000003)
_NEG_XOR = U64(0xABCDEF)
_NEG_KEY = U64(0x5EED)


def _u64(x):
    """uint64 array of x (python ints >= 2**63 included); always at least 1-d so that the arithmetic wraps silently."""
    if isinstance(x, np.ndarray):
        return np.atleast_1d(x if x.dtype == np.uint64 else x.astype(np.uint64))
    if isinstance(x, (list, tuple)):
        return np.array([int(v) & 0xFFFFFFFFFFFFFFFF for v in x], dtype=np.uint64)
    return np.array([int(x) & 0xFFFFFFFFFFFFFFFF], dtype=np.uint64)


def mix64(z):
    z = _u64(z) + _GOLDEN
    z = (z ^ (z >> U64(30))) * _M1
    z = (z ^ (z >> U64(27))) * _M2
    return z ^ (z >> U64(31))


def u01(a, b, c):
    """float64 in [0, 1): 53 random bits scaled by 2**-53 (both steps exact)."""
    a, b, c = _u64(a), _u64(b), _u64(c)
    bits = mix64(mix64(a) ^ mix64(b * _FNV + c)) >> U64(11)
    return bits.astype(np.float64) * 2.0 ** -53


def row_cumsum(row_ptr, val):
    """cumw[e] = val[s] + ... + val[e] summed left to right in float32, per row [s, row_ptr[r + 1])."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    val = np.asarray(val, dtype=np.float32)
    out = np.empty_like(val)
    for r in np.flatnonzero(np.diff(row_ptr) > 0):
        s, e = row_ptr[r], row_ptr[r + 1]
        np.cumsum(val[s:e], dtype=np.float32, out=out[s:e])
    return out


def walks(row_ptr, col, cumw, walk_length, walk_time, seed, weighted):
    """One walker per (node, it), it = 0..walk_time-1, of walk_length steps (walk_length + 1 nodes) unless it meets an empty row.
    The step that fills walk[len] draws u = u01(seed, node*1000003 + it, len).
      unweighted: the edge s + min(int(u*(e - s)), e - s - 1);
      weighted:   the first edge with cumw > float32(u * float64(cumw[e - 1])), found by the lo/hi bisection over [s, e - 1] that falls
                  through to e - 1.
    Returns (walk int32[n*walk_time, walk_length + 1] padded with -1, length[n*walk_time], freq int64[n], pair_row_ptr int64[n + 1],
    pair_col int64[nnz]): every i < j of a walk with different endpoints counts 1 for each endpoint; the pair CSR is the symmetric,
    de-duplicated 0/1 matrix of those pairs with sorted rows."""
    row_ptr = np.asarray(row_ptr, dtype=np.int64)
    col = np.asarray(col, dtype=np.int64)
    n = len(row_ptr) - 1
    wl = int(walk_length) + 1
    node = np.repeat(np.arange(n, dtype=np.int64), walk_time)
    it = np.tile(np.arange(walk_time, dtype=np.int64), n)
    key = node.astype(np.uint64) * _NODE_MUL + it.astype(np.uint64)
    walk = np.full((n * walk_time, wl), -1, dtype=np.int64)
    walk[:, 0] = node
    length = np.ones(n * walk_time, dtype=np.int64)
    alive = np.arange(n * walk_time)
    for ln in range(1, wl):
        cur = walk[alive, ln - 1]
        s, e = row_ptr[cur], row_ptr[cur + 1]
        go = e > s                                                        # an empty row ends the walk for good
        alive, s, e = alive[go], s[go], e[go]
        if alive.size == 0:
            break
        u = u01(seed, key[alive], ln)
        if weighted:
            target = (u * cumw[e - 1].astype(np.float64)).astype(np.float32)
            lo, hi = s.copy(), e - 1
            while True:
                act = lo < hi
                if not act.any():
                    break
                mid = (lo + hi) >> 1
                up = cumw[mid] > target
                hi = np.where(act & up, mid, hi)
                lo = np.where(act & ~up, mid + 1, lo)
            pick = lo
        else:
            pick = s + np.minimum((u * (e - s).astype(np.float64)).astype(np.int64), e - s - 1)
        walk[alive, ln] = col[pick]
        length[alive] = ln + 1
    freq = np.zeros(n, dtype=np.int64)
    keys = []
    for i in range(wl):
        for j in range(i + 1, wl):
            a, b = walk[:, i], walk[:, j]
            ok = (j < length) & (a != b)
            a, b = a[ok], b[ok]
            freq += np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
            keys.append(a * n + b)
            keys.append(b * n + a)
    keys = np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)
    pair_row_ptr = np.zeros(n + 1, dtype=np.int64)
    if n:
        np.cumsum(np.bincount(keys // n, minlength=n), out=pair_row_ptr[1:])
        pair_col = keys % n
    else:
        pair_col = keys
    return walk.astype(np.int32), length, freq, pair_row_ptr, pair_col


def pos_draws(perm, batch_size, seeds, pair_row_ptr, pair_col, num):
    """Position p of the epoch order (node v = perm[p], batch p // batch_size, local index p % batch_size) takes all of v's pair
    partners if there are at most `num`, else `num` of them by selection sampling in row order: partner k is taken when
    u01(seeds[batch], local, k) * float64(deg - k) < float64(still needed).
    Returns (node int64[S], pos int64[S], offsets int64[P + 1], batch_offsets int64[B + 1])."""
    perm = np.asarray(perm, dtype=np.int64)
    pair_row_ptr = np.asarray(pair_row_ptr, dtype=np.int64)
    pair_col = np.asarray(pair_col, dtype=np.int64)
    seeds = _u64(list(seeds)) if len(seeds) else np.zeros(0, dtype=np.uint64)
    P, bs = len(perm), int(batch_size)
    B = -(-P // bs)
    p = np.arange(P, dtype=np.int64)
    s = pair_row_ptr[perm]
    deg = pair_row_ptr[perm + 1] - s
    take = np.minimum(deg, num)
    offsets = np.zeros(P + 1, dtype=np.int64)
    np.cumsum(take, out=offsets[1:])
    batch_offsets = offsets[np.minimum(np.arange(B + 1, dtype=np.int64) * bs, P)]
    base = np.zeros(P + 1, dtype=np.int64)                                # candidate slots: every partner of every position
    np.cumsum(deg, out=base[1:])
    taken = np.zeros(base[-1], dtype=bool)
    short = deg <= num
    taken[np.repeat(short, deg)] = True
    act = np.flatnonzero(~short)
    need = np.full(act.size, num, dtype=np.int64)
    seed_p, local = seeds[p // bs], (p % bs).astype(np.uint64)
    k = 0
    while act.size:
        u = u01(seed_p[act], local[act], k)
        hit = u * (deg[act] - k).astype(np.float64) < need.astype(np.float64)
        taken[base[act[hit]] + k] = True
        need = need - hit
        k += 1
        go = (need > 0) & (deg[act] > k)
        act, need = act[go], need[go]
    owner = np.repeat(p, deg)
    slot = np.arange(base[-1], dtype=np.int64) - base[owner]
    node = perm[owner][taken]
    pos = pair_col[s[owner] + slot][taken]
    assert len(node) == offsets[-1], "selection sampling fell short: the model itself is wrong"
    return node, pos, offsets, batch_offsets


def neg_draws(seed, table, num):
    """`num` distinct POSITIONS of the table (equal node ids at different positions may repeat): try t = 0, 1, ... draws position
    min(int(u01(seed ^ 0xabcdef, 0x5eed, t) * float64(len(table))), len(table) - 1) and is rejected when that position is taken."""
    table = np.asarray(table, dtype=np.int64)
    n = len(table)
    assert n >= num
    key = _u64(seed) ^ _NEG_XOR
    got, t0 = [], 0
    while len(got) < num:
        chunk = 4 * num + 16
        u = u01(key, _NEG_KEY, np.arange(t0, t0 + chunk, dtype=np.uint64))
        for q in np.minimum((u * float(n)).astype(np.int64), n - 1).tolist():
            if q not in got:
                got.append(q)
                if len(got) == num:
                    break
        t0 += chunk
    return table[np.array(got, dtype=np.int64)]
