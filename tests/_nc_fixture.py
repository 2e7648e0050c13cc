"""Shared by tests/golden/make_golden_nodecls.py and the node-classification tests: the fixture's per-month labels, rebuilt from the
UCI snapshot edges (tests/golden/uci_snapshots.npz), and the split encoding of node_classification_uci.npz."""
import numpy as np


def month_labels(snapshots, t):
    """(node index, label) of the nodes active in month t, by node index: label = quartile (0..3) of the node's degree rank, degree
    counted over the month's edge rows, ties broken by node index."""
    src, dst = np.asarray(snapshots["t%d_src" % t], np.int64), np.asarray(snapshots["t%d_dst" % t], np.int64)
    nodes, deg = np.unique(np.concatenate([src, dst]), return_counts=True)
    order = np.lexsort((nodes, deg))
    label = np.empty(len(nodes), np.int64)
    label[order] = (4 * np.arange(len(nodes))) // len(nodes)
    return nodes, label


def split_rows(gold, r, t, part):
    """int64 [n, 2] (node index, label) rows of the reference's <date>_<part>.csv of repetition r, month t, in file order."""
    key = "split_%d_%d_%s" % (r, t, part)
    return np.stack([gold[key + "_node"].astype(np.int64), gold[key + "_label"].astype(np.int64)], 1)
