"""Shared by tests/golden/make_golden_lp.py and the link-prediction tests: the fixture's embedding, rebuilt bit for bit from the
UCI snapshot edges (tests/golden/uci_snapshots.npz), and the compact encoding of the split arrays."""
import hashlib

import numpy as np
import scipy.sparse as sp


def _splitmix64(z):
    z = z + np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def embedding(src, dst, n, d, seed):
    """float32 [n, d] with link signal: two hops of (A + I) over integer weights in {-2..2} (splitmix64 of seed and entry), all in
    int64, then one correctly rounded float32 division by the row sum of (A + I)^2.  Exact on every IEEE machine."""
    a = sp.coo_matrix((np.ones(len(src), np.int64), (np.asarray(src), np.asarray(dst))), shape=(n, n)).tocsr()
    a = ((a + a.T) > 0).astype(np.int64) + sp.eye(n, dtype=np.int64, format="csr")
    idx = np.arange(n * d, dtype=np.uint64) + np.uint64(seed) * np.uint64(1 << 32)
    g = (_splitmix64(idx) % np.uint64(5)).astype(np.int64).reshape(n, d) - 2
    y = a @ (a @ g)
    c = a @ (a @ np.ones(n, np.int64))
    return y.astype(np.float32) / c.astype(np.float32)[:, None]


def digest(emb):
    return hashlib.sha256(np.ascontiguousarray(emb, dtype=np.float32).tobytes()).hexdigest()


def encode_rows(rows, n):
    """[k, 2] node pairs -> uint32 deltas of the sorted keys u * n + v (row order is not kept: no fit or AUC depends on it)."""
    key = np.sort(np.asarray(rows, np.int64)[:, 0] * n + np.asarray(rows, np.int64)[:, 1])
    return np.diff(key, prepend=0).astype(np.uint32)


def decode_split(gold, t, part, n):
    """int64 [2k, 3] split: the k positives (label 1), then the k negatives (label 0), as the reference lays them out."""
    out = []
    for name, label in (("pos", 1), ("neg", 0)):
        key = np.cumsum(gold["split_%d_%s_%s" % (t, part, name)].astype(np.int64))
        out.append(np.stack([key // n, key % n, np.full(len(key), label)], 1))
    return np.concatenate(out)


def month_embedding(snapshots, t, n, d=128, seed=20261015):
    """The fixture's embedding of month t from tests/golden/uci_snapshots.npz."""
    return embedding(snapshots["t%d_src" % t], snapshots["t%d_dst" % t], n, d, seed + t)
