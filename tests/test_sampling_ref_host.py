"""The host model of the walk / sampler draws (tests/_sampling_ref.py) against things that are neither the model nor the kernels:
a Python-int splitmix64, the reference's own random_walk outputs on a graph where its walks are deterministic, the defining
properties of selection sampling, and exact rational pick probabilities.  No GPU."""
import numpy as np

import _sampling_ref as R
from conftest import load_golden, csr_from

M64 = 2 ** 64 - 1


def _mix_int(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _u01_int(a, b, c):
    bits = _mix_int(_mix_int(a) ^ _mix_int((b * 0x100000001B3 + c) & M64)) >> 11
    return bits / 9007199254740992                                          # int / int: correctly rounded, and bits < 2**53 is exact


def test_u01_equals_python_int_arithmetic():
    rng = np.random.default_rng(11)
    n = 100000
    a, b, c = (rng.integers(0, 2 ** 64, size=n, dtype=np.uint64) for _ in range(3))
    a[:4] = [0, M64, 2 ** 63, 1]                                            # wrap-around and sign-bit keys
    b[:4] = [M64, M64, 0, 2 ** 63]
    c[:4] = [M64, 0, 2 ** 63, M64]
    got = R.u01(a, b, c)
    want = np.array([_u01_int(int(x), int(y), int(z)) for x, y, z in zip(a, b, c)], dtype=np.float64)
    assert got.dtype == np.float64 and np.array_equal(got, want)
    assert got.min() >= 0.0 and got.max() < 1.0
    assert np.array_equal(R.mix64(a), np.array([_mix_int(int(x)) for x in a], dtype=np.uint64))
    # scalars, python ints >= 2**63 and broadcasting take the same path
    assert R.u01(2 ** 64 - 1, 5, 7)[0] == _u01_int(2 ** 64 - 1, 5, 7)
    assert np.array_equal(R.u01(3, np.arange(5), 2), np.array([_u01_int(3, k, 2) for k in range(5)]))


def test_row_cumsum_is_the_sequential_float32_sum():
    rng = np.random.default_rng(12)
    deg = np.concatenate([[0, 1, 0, 700], rng.integers(0, 9, size=50)])
    row_ptr = np.concatenate([[0], np.cumsum(deg)])
    val = rng.random(row_ptr[-1]).astype(np.float32) * 3
    got = R.row_cumsum(row_ptr, val)
    want = np.empty_like(val)
    for r in range(len(deg)):
        acc = np.float32(0)
        for e in range(row_ptr[r], row_ptr[r + 1]):
            acc = np.float32(acc + val[e])
            want[e] = acc
    assert got.dtype == np.float32 and np.array_equal(got, want)


def test_model_reproduces_the_reference_corpus_on_the_perfect_matching():
    """every draw on a perfect matching has one outcome, so the reference's files are the model's output whatever the seed"""
    from ctgcn_amd.walks import negative_table
    g = load_golden("negloss.npz")
    n = len(g["match_adj_indptr"]) - 1
    L, W = [int(x) for x in g["match_LW"]]
    adj = csr_from(g, "match_adj", n)
    adj.sort_indices()
    want = csr_from(g, "match_pairs", n)
    want.sort_indices()
    cumw = R.row_cumsum(adj.indptr, adj.data.astype(np.float32))
    for weighted in (True, False):
        for seed in (5, 2 ** 64 - 3):
            walk, length, freq, prp, pc = R.walks(adj.indptr, adj.indices, cumw, L, W, seed, weighted)
            matched = np.repeat(np.diff(adj.indptr) > 0, W)                  # the graph also has unmatched (isolated) nodes
            assert walk.shape == (n * W, L + 1) and np.all(length == np.where(matched, L + 1, 1))
            assert np.array_equal(prp, want.indptr) and np.array_equal(pc, want.indices)
            assert np.array_equal(negative_table(freq), g["match_neg"])


def test_walks_follow_edges_stop_at_dead_ends_and_count_pairs():
    """structure of the model's walks on a small directed graph with a dead end, checked against a brute-force recount"""
    # 0 -> {1, 2}, 1 -> {3}, 2 -> {0, 1, 3}, 3 -> {} (dead end), 4 -> {3} (only neighbour is a dead end), 5 isolated
    row_ptr = np.array([0, 2, 3, 6, 6, 7, 7])
    col = np.array([1, 2, 3, 0, 1, 3, 3])
    val = np.array([1, 3, 2, 0, 5, 0, 4], dtype=np.float32)                  # row 2: leading and trailing weight 0 -> always picks 1
    cumw = R.row_cumsum(row_ptr, val)
    n, L, W = 6, 4, 50
    for weighted in (True, False):
        walk, length, freq, prp, pc = R.walks(row_ptr, col, cumw, L, W, 9, weighted)
        cnt = np.zeros(n, dtype=np.int64)
        pairs = set()
        for w, ln in zip(walk, length):
            assert np.all(w[ln:] == -1) and np.all(w[:ln] >= 0)
            for a, b in zip(w[:ln - 1], w[1:ln]):
                assert b in col[row_ptr[a]:row_ptr[a + 1]]
                if weighted and a == 2:
                    assert b == 1
            assert ln == L + 1 or row_ptr[w[ln - 1]] == row_ptr[w[ln - 1] + 1]
            for i in range(ln):
                for j in range(i + 1, ln):
                    if w[i] != w[j]:
                        cnt[w[i]] += 1
                        cnt[w[j]] += 1
                        pairs.add((int(w[i]), int(w[j])))
                        pairs.add((int(w[j]), int(w[i])))
        assert np.array_equal(freq, cnt)
        assert sorted(pairs) == [(r, int(c)) for r in range(n) for c in pc[prp[r]:prp[r + 1]]]
        assert length[5 * W:].max() == 1 and length[4 * W:5 * W].max() == 2 and freq[5] == 0
        if not weighted:                                                    # the unweighted walker does use the zero-weight edges
            assert any(w[i] == 2 and w[i + 1] in (0, 3) for w, ln in zip(walk, length) for i in range(ln - 1))


def test_selection_sampling_takes_min_deg_num_distinct_partners_in_row_order():
    rng = np.random.default_rng(13)
    n, num = 400, 6
    deg = rng.integers(0, 20, size=n)
    row_ptr = np.concatenate([[0], np.cumsum(deg)])
    col = np.concatenate([np.sort(rng.choice(1000, size=d, replace=False)) for d in deg]).astype(np.int64)
    perm = rng.permutation(n)
    bs = 96
    seeds = [int(x) for x in rng.integers(0, 2 ** 64, size=-(-n // bs), dtype=np.uint64)]
    node, pos, off, boff = R.pos_draws(perm, bs, seeds, row_ptr, col, num)
    assert off[0] == 0 and off[-1] == len(node) == len(pos)
    assert np.array_equal(boff, off[np.minimum(np.arange(len(seeds) + 1) * bs, n)])
    saw_long = 0
    for p, v in enumerate(perm):
        got = pos[off[p]:off[p + 1]]
        row = col[row_ptr[v]:row_ptr[v + 1]]
        assert len(got) == min(deg[v], num) and np.all(node[off[p]:off[p + 1]] == v)
        assert np.all(np.diff(got) > 0) and np.all(np.isin(got, row))          # distinct, in row order (rows ascend here)
        if deg[v] <= num:
            assert np.array_equal(got, row)
        else:
            saw_long += 1
    assert saw_long > 100


def test_selection_sampling_is_uniform_within_five_sigma():
    """deg 17, num 5, 20 000 locals of one batch: every partner's inclusion count is binomial(20 000, 5/17)"""
    deg, num, m = 17, 5, 20000
    row_ptr = np.array([0, deg])
    col = np.arange(100, 100 + deg)
    _, pos, off, _ = R.pos_draws(np.zeros(m, dtype=np.int64), m, [0x1234ABCD5678EF01], row_ptr, col, num)
    assert len(pos) == m * num and np.all(np.diff(off) == num)
    counts = np.bincount(pos - 100, minlength=deg)
    p = num / deg
    sigma = np.sqrt(m * p * (1 - p))
    z = np.abs(counts - m * p) / sigma
    print("  worst inclusion count at %.2f sigma" % z.max())
    assert z.max() < 5.0


def test_neg_draws_are_distinct_table_positions():
    table = np.array([7, 7, 7, 3, 3, 9, 1, 7])
    for seed in (0, 1, 2 ** 63 + 5, 2 ** 64 - 1):
        full = R.neg_draws(seed, table, len(table))                         # table_len == num: a permutation of the positions
        assert sorted(full.tolist()) == sorted(table.tolist())
        assert np.array_equal(R.neg_draws(seed, table, 3), full[:3])         # the try sequence does not depend on num
    big = np.arange(1000)
    d = np.array([R.neg_draws(s, big, 20) for s in range(300)])
    assert all(len(set(r)) == 20 for r in d.tolist())
    counts = np.bincount(d.ravel(), minlength=1000)                          # 6000 draws over 1000 slots: mean 6, sd 2.4
    assert counts.max() <= 6 + 6 * 2.5 and counts.min() >= 0 and abs(d.mean() - 499.5) < 5 * 288.7 / np.sqrt(6000)


def test_integer_weights_give_exact_pick_probabilities():
    """the weighted pick takes edge k when cumw[k-1] <= target < cumw[k]: its probability is (cumw[k] - cumw[k-1]) / cumw[-1].
    For integer weights with row sums below 2**24 every fp32 prefix sum is exact, so that is w_k / sum(w) exactly."""
    rng = np.random.default_rng(14)
    w = rng.integers(1, 100, size=200000)
    assert w.sum() < 2 ** 24
    cumw = R.row_cumsum([0, len(w)], w.astype(np.float32))
    assert np.array_equal(cumw.astype(np.int64), np.cumsum(w))
    inc = np.diff(np.concatenate([[0.0], cumw.astype(np.float64)]))
    err = np.abs(inc / float(cumw[-1]) - w / w.sum()).max()
    print("  integer weights: max |p_implied - w/sum(w)| = %g" % err)
    assert err == 0.0


def test_fractional_weights_on_a_long_row_stay_within_fp32_rounding():
    """documented limit (walks.random_walk_corpus): on a 200 000-entry row of fractional weights the fp32 prefix sums round some
    increments to zero — those edges are never picked — while the error of every pick probability stays at fp32 rounding of the
    row sum: each stored prefix is one rounding (<= 2**-24 relative to the running sum) away from prefix + w_k."""
    rng = np.random.default_rng(15)
    w = rng.random(200000).astype(np.float32)
    cumw = R.row_cumsum([0, len(w)], w)
    inc = np.diff(np.concatenate([[0.0], cumw.astype(np.float64)]))
    exact = w.astype(np.float64)
    err = np.abs(inc / float(cumw[-1]) - exact / exact.sum()).max()
    lost = int((inc == 0).sum())
    print("  fractional weights: %d of %d edges have probability 0, max |p_implied - w/sum(w)| = %.3g = %.2f x 2**-24"
          % (lost, len(w), err, err * 2 ** 24))
    assert np.all(inc >= 0) and err <= 2.0 ** -23
