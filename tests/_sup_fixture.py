"""Shared by tests/golden/make_golden_supervised.py and the supervised-trainer tests: the fixture's inputs, rebuilt from the UCI
snapshot edges (tests/golden/uci_snapshots.npz), and the decoding of supervised_uci.npz.

Window: the 3 months of uci_core_adj.npz's w4_* window (months 4, 5, 6; n = 1899).  Labels: _nc_fixture.month_labels and
_ec_fixture.month_edge_labels with their rows permuted by numpy's PCG64 under the fixture's label seed, so that every split
(taken in file order) holds every class."""
import numpy as np

import _ec_fixture
import _nc_fixture

MONTHS = (4, 5, 6)
N_NODES = 1899
RATIOS = (0.5, 0.3, 0.2)
EPOCHS, LR = 3, 1e-3
R_NODE, R_PAIR = 1e-4, 2e-4                  # the forward rule: rtol 1e-4 on embeddings (test_gpu_models.TOL), once per factor
CALLS = (("train", 0), ("train", 1), ("val", 1), ("train", 2), ("val", 2), ("test", 3))      # the loss calls of a 3-epoch run, in order
#        case            learning type  model      mode rule  classes
CASES = {"node_c": ("S-node", "CTGCN-C", R_NODE, 4), "node_s": ("S-node", "CTGCN-S", R_NODE, 4),
         "link_st": ("S-link-st", "CTGCN-C", R_PAIR, 2), "link_dy": ("S-link-dy", "CTGCN-C", R_PAIR, 2),
         "edge_cgcn": ("S-edge", "CGCN-C", R_PAIR, 3), "edge_ctgcn": ("S-edge", "CTGCN-C", R_PAIR, 3)}
MODEL_SEED = {"CTGCN-C": 21, "CTGCN-S": 22, "CGCN-C": 23}
CLS_SEED = 31
CLS_ACT = {"S-node": "N", "S-edge": "L"}     # both activations of the single-Linear head


def node_label_rows(snapshots, t, seed):
    """int64 [rows, 2] (node index, label) of month t in the fixture's file order"""
    nodes, label = _nc_fixture.month_labels(snapshots, t)
    rows = np.stack([nodes, label], 1).astype(np.int64)
    return rows[np.random.default_rng(seed * 100 + t).permutation(len(rows))]


def edge_label_rows(snapshots, t, seed):
    """int64 [rows, 3] (from index, to index, label) of month t in the fixture's file order"""
    u, v, label = _ec_fixture.month_edge_labels(snapshots, t)
    rows = np.stack([u, v, label], 1).astype(np.int64)
    return rows[np.random.default_rng(seed * 100 + 50 + t).permutation(len(rows))]


def edge_list(snapshots, t):
    """int64 [2, E]: both directions of month t's distinct pairs, sorted by u·n + v (what the reference derives from its date adjacency)"""
    src, dst = np.asarray(snapshots["t%d_src" % t], np.int64), np.asarray(snapshots["t%d_dst" % t], np.int64)
    key = np.unique(np.concatenate([src * N_NODES + dst, dst * N_NODES + src]))
    return np.stack([key // N_NODES, key % N_NODES])


def stored_splits(gold, case):
    """(idx_train, label_train, idx_val, label_val, idx_test, label_test) of a link case as numpy arrays per scored snapshot:
    idx int64 [2, n], labels float32 (1 then 0): the reference's own draws"""
    out = []
    for part in ("train", "val", "test"):
        idx, lab = [], []
        for s in range(int(gold[case + "_snapshots"])):
            e = gold["%s_split_%s_%d" % (case, part, s)].astype(np.int64)
            idx.append(e)
            lab.append(np.concatenate([np.ones(e.shape[1] // 2, np.float32), np.zeros(e.shape[1] // 2, np.float32)]))
        out += [idx, lab]
    return tuple(out)
