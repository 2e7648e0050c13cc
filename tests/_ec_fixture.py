"""Shared by tests/golden/make_golden_edgecls.py and the edge-classification tests: the fixture's per-month edge labels, rebuilt from
the UCI snapshot edges (tests/golden/uci_snapshots.npz), and the split encoding of edge_classification_uci.npz."""
import numpy as np


def month_edge_labels(snapshots, t):
    """(u, v, label) of the edges of month t: the unique unordered pairs {u, v} of the month's rows with u < v (self-loops dropped),
    sorted by the key u·n + v.  label = (3·rank) // m (0..2), rank by (deg[u]·deg[v], key) with deg the degree in that simple
    symmetric graph: tertiles of the degree product."""
    n = len(snapshots["node_names"])
    src, dst = np.asarray(snapshots["t%d_src" % t], np.int64), np.asarray(snapshots["t%d_dst" % t], np.int64)
    keep = src != dst
    lo, hi = np.minimum(src, dst)[keep], np.maximum(src, dst)[keep]
    key = np.unique(lo * n + hi)
    u, v = key // n, key % n
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    order = np.lexsort((key, deg[u] * deg[v]))
    label = np.empty(len(key), np.int64)
    label[order] = (3 * np.arange(len(key))) // len(key)
    return u, v, label


def encode_split(rows, u, v, n):
    """[k, 3] rows (from, to, label) of a split file -> uint16 positions in the month's edge list (u, v), in file order."""
    rows = np.asarray(rows, np.int64)
    pos = np.searchsorted(u * n + v, rows[:, 0] * n + rows[:, 1])
    assert np.array_equal(u[pos], rows[:, 0]) and np.array_equal(v[pos], rows[:, 1]) and len(u) < 65536
    return pos.astype(np.uint16)


def split_rows(gold, r, t, part):
    """int64 [k, 3] (from index, to index, label) rows of the reference's <date>_<part>.csv of repetition r, month t, in file order."""
    pos = gold["split_%d_%d_%s" % (r, t, part)].astype(np.int64)
    return np.stack([gold["labels_%d_%s" % (t, c)].astype(np.int64)[pos] for c in ("from", "to", "label")], 1)
