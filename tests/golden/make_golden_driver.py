#!/usr/bin/env python3
"""Generate tests/golden/driver_uci.json by RUNNING the reference's train.get_input_data and its window loop's arithmetic.

Like its siblings this script runs only where the reference tree is: it imports the reference in-process, on the CPU, and stores what
it returns as data, no source text.  Shims of its own (reference files untouched): np.int = int (the reference's method tables and
degree features use the removed alias), nx.to_scipy_sparse_matrix (removed from networkx; the k-core files are written through it)
as to_scipy_sparse_array in a csr_matrix, np.random.normal taking float(loc) (helper.py:131 passes a 1x1 np.matrix as loc, which
numpy no longer broadcasts to a 1-D size; make_golden.py's shim 3), and an empty stand-in for torch_geometric, which baseline/pgnn.py imports by name alone;
get_input_data imports no other baseline.
Re-run:  python tests/golden/make_golden_driver.py

Setup: the 7 UCI snapshots of uci_snapshots.npz (n = 1899) written as the reference's edge files, the reference's own k-core files for
them, and for each of the 16 GNN methods its section of uci_config.json with base_path set to that dataset.  Per method, on the window
(idx 4, time_length 3), from what get_input_data returns:
  input_dim
  adj_none          adj_list is None
  adj               per snapshot [stored entries, float64 sum of the values]; for the core-based methods one such pair per k-core matrix
  edge_shapes       per snapshot the shape of edge_list[t]
  x_kind, x_shape   'sparse' / 'dense' (a list: shape of every entry) or 'stacked-sparse' / 'stacked-dense' (one tensor: its shape)
  dist_shapes       PGNN only: the shape of every entry of node_dist_list (approximate as configured)
Schedules: for every case of SCHEDULES the (idx, time_length) sequence of the reference's loop (train.py:253-271), taken by running
gnn_embedding itself with get_input_data replaced by a recorder that ends the window there.
"""
import json
import os
import shutil
import sys
import tempfile
import types
import warnings

import networkx as nx
import numpy as np
import scipy.sparse as sp
import torch

warnings.filterwarnings("ignore")
np.int = int
if not hasattr(nx, "to_scipy_sparse_matrix"):
    nx.to_scipy_sparse_matrix = lambda *a, **k: sp.csr_matrix(nx.to_scipy_sparse_array(*a, **k))
_normal = np.random.normal
np.random.normal = lambda loc=0.0, scale=1.0, size=None: _normal(float(loc), scale, size)
REF = "/root/reference"
sys.path.insert(0, REF)
sys.modules.setdefault("torch_geometric", types.ModuleType("torch_geometric"))
import train as ref_train  # noqa: E402
from preprocessing.structure_generation import StructureInfoGenerator  # noqa: E402
from utils import get_supported_gnn_methods  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
WINDOW = (4, 3)
# (max_time_num, start_idx, end_idx, duration, learning_type)
SCHEDULES = [(7, 0, -1, 3, "U-neg"), (7, 0, -1, 3, "S-link-dy"), (7, -3, -1, 1, "U-neg"), (7, 0, -1, 7, "U-neg"), (7, 0, -1, 2, "S-link-st"),
             (7, 0, -1, 2, "S-link-dy"), (7, 2, 5, 3, "U-own"), (7, 1, -2, 2, "S-link-dy"), (7, 0, -1, 7, "S-link-dy")]


def write_dataset(base):
    snaps = np.load(os.path.join(OUT, "uci_snapshots.npz"))
    names = [str(x) for x in snaps["node_names"]]
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "nodes_set"))
    with open(os.path.join(base, "nodes_set", "nodes.csv"), "w") as fp:
        fp.write("\n".join(names) + "\n")
    for t, f in enumerate(str(f) for f in snaps["files"]):
        with open(os.path.join(base, "1.format", f), "w") as fp:
            fp.write("from_id\tto_id\tweight\n")
            for s, d, w in zip(snaps["t%d_src" % t], snaps["t%d_dst" % t], snaps["t%d_w" % t]):
                fp.write("%s\t%s\t%d\n" % (names[s], names[d], int(w)))
    return len(snaps["files"])


def entry_stats(t):
    """stored entries as the reference holds them (not coalesced) and the float64 sum of their values"""
    return [int(t._values().numel()), float(t._values().double().sum())]


def describe_x(x_list):
    if isinstance(x_list, torch.Tensor):
        return ("stacked-sparse" if x_list.is_sparse else "stacked-dense"), list(x_list.shape)
    kinds = {("sparse" if x.is_sparse else "dense") for x in x_list}
    assert len(kinds) == 1
    return kinds.pop(), [list(x.shape) for x in x_list]


def record_method(method, config, base):
    args = dict(config["embedding"][method])
    args["base_path"] = base
    args["has_cuda"] = False
    loader = ref_train.get_data_loader(args)
    input_dim, adj_list, x_list, edge_list, node_dist_list = ref_train.get_input_data(method, WINDOW[0], WINDOW[1], loader, args)
    rec = {"input_dim": int(input_dim), "adj_none": adj_list is None, "edge_shapes": [list(e.shape) for e in edge_list]}
    if adj_list is not None:
        rec["adj"] = [[entry_stats(m) for m in a] if isinstance(a, list) else entry_stats(a) for a in adj_list]
    rec["x_kind"], rec["x_shape"] = describe_x(x_list)
    if node_dist_list is not None:
        rec["dist_shapes"] = [list(np.asarray(d).shape) for d in node_dist_list]
    return rec


def record_schedule(case, base_root):
    """the loop's (idx, time_length) sequence: gnn_embedding itself, with every stage below the loop header replaced by a no-op"""
    max_time_num, start_idx, end_idx, duration, learning_type = case
    base = tempfile.mkdtemp(dir=base_root)
    os.makedirs(os.path.join(base, "origin"))
    for t in range(max_time_num):
        open(os.path.join(base, "origin", "%02d.csv" % t), "w").close()
    with open(os.path.join(base, "nodes.csv"), "w") as fp:
        fp.write("a\nb\n")
    seen = []
    args = dict(base_path=base, origin_folder="origin", embed_folder="emb", model_folder="model", model_file="m", node_file="nodes.csv",
                start_idx=start_idx, end_idx=end_idx, duration=duration, has_cuda=False, learning_type=learning_type, epoch=1, lr=1e-3,
                batch_size=2, load_model=False, shuffle=False, export=False, record_time=False, weight_decay=0.0, train_ratio=0.5,
                val_ratio=0.3, test_ratio=0.2)
    orig = ref_train.get_input_data
    ref_train.get_input_data = lambda m, idx, tl, dl, a: (seen.append([int(idx), int(tl)]), (0, None, [], [], None))[1]
    orig_model, orig_loss = ref_train.get_gnn_model, ref_train.get_loss
    orig_unsup, orig_sup = ref_train.UnsupervisedEmbedding, ref_train.SupervisedEmbedding

    class _Trainer(object):
        def __init__(self, *a, **k):
            pass

        def learn_embedding(self, *a, **k):
            return 0.0

    ref_train.get_gnn_model = lambda *a, **k: None
    ref_train.get_loss = lambda method, idx, tl, dl, a: None if a["learning_type"].startswith("U") else (None, None, None, None)
    ref_train.UnsupervisedEmbedding = ref_train.SupervisedEmbedding = _Trainer
    raised = None
    try:
        ref_train.gnn_embedding("GCN", args)
    except AssertionError:
        raised = "AssertionError"
    finally:
        ref_train.get_input_data, ref_train.get_gnn_model, ref_train.get_loss = orig, orig_model, orig_loss
        ref_train.UnsupervisedEmbedding, ref_train.SupervisedEmbedding = orig_unsup, orig_sup
    return {"max_time_num": max_time_num, "start_idx": start_idx, "end_idx": end_idx, "duration": duration, "learning_type": learning_type,
            "windows": seen, "raises": raised}


def main():
    torch.set_num_threads(8)
    with open(os.path.join(OUT, "uci_config.json")) as fp:
        config = json.load(fp)
    base = tempfile.mkdtemp()
    out = {"window": list(WINDOW), "methods": {}, "schedules": []}
    try:
        out["max_time_num"] = write_dataset(base)
        StructureInfoGenerator(base, "1.format", "CTGCN/ctgcn_cores", "nodes_set/nodes.csv").get_kcore_graph_all_time(sep="\t", worker=-1)
        for method in get_supported_gnn_methods():
            np.random.seed(1)
            out["methods"][method] = record_method(method, config, base)
            print(method, json.dumps(out["methods"][method])[:200], flush=True)
        for case in SCHEDULES + [(7, 0, -1, 1, "S-link-dy")]:
            out["schedules"].append(record_schedule(case, base))
            print(out["schedules"][-1], flush=True)
    finally:
        shutil.rmtree(base, ignore_errors=True)
    out["method_tables"] = {name: list(getattr(sys.modules["utils"], name)()) for name in
                            ("get_static_gnn_methods", "get_dynamic_gnn_methods", "get_core_based_methods", "get_supported_gnn_methods",
                             "get_supported_methods")}
    path = os.path.join(OUT, "driver_uci.json")
    with open(path, "w") as fp:
        json.dump(out, fp, indent=1, sort_keys=True)
        fp.write("\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
