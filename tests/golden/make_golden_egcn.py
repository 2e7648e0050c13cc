"""Golden data of the EvolveGCN baseline: tests/golden/egcn_uci.npz.  Runs only where the reference tree is; imports the reference
in-process (baseline/egcn.py by file path, since its package __init__ pulls in libraries that need not be installed) and stores data
only: inputs that are not closed-form, expected outputs, and the reference's own float32-vs-float64 error as the yardstick.

Setup: the first 3 UCI snapshots (n = 1899) through the reference's get_sp_adj_mat -> + eye -> get_normalized_adj(row_norm=False);
EvolveGCN(24, 16, 16) as EGCNH and EGCNO on formula features, EGCNH on one-hot degree features; parameters from
conftest.seeded_parameters; surrogate loss sum_t sum(out_t * C_t); 3 Adam steps at lr 1e-3.

Seed condition (so that no comparison hinges on a coin flip in top-k): the first parameter seed for which, at every layer, snapshot
and Adam step of every case, each consecutive pair among the top k + 1 float64 scores is at least 1e-5 max|score| apart or belongs to
two nodes with identical input rows.  The smallest gap seen is stored."""
import importlib.util
import os
import sys
import tempfile

import numpy as np
import scipy.sparse as sp
import torch

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REF)
import utils as ref_utils  # noqa: E402
sys.path.insert(0, os.path.dirname(OUT))
import _egcn_ref as E  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_egcn", os.path.join(REF, "baseline", "egcn.py"))
ref_egcn = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref_egcn)

GAP = 1e-5


def put_tensor(d, key, g, full_below=6000):
    """make_golden.put_tensor's form (checksums, the full tensor when small, else 256 sampled entries), kept in float64"""
    g = g.detach().numpy().astype(np.float64)
    d[key + "__sum"] = np.float64(g.sum())
    d[key + "__abssum"] = np.float64(np.abs(g).sum())
    d[key + "__maxabs"] = np.float64(np.abs(g).max())            # the yardsticks are errors over the tensor's largest magnitude
    if g.size <= full_below:
        d[key] = g
    else:
        flat = g.reshape(-1)
        pick = np.linspace(0, flat.size - 1, 256).astype(np.int64)
        d[key + "__pick"] = pick
        d[key + "__vals"] = flat[pick]


def reference_adjacency(d):
    snaps = np.load(os.path.join(OUT, "uci_snapshots.npz"))
    names = [str(s) for s in snaps["node_names"]]
    mats = []
    with tempfile.TemporaryDirectory() as tmp:
        for t in range(E.T):
            path = os.path.join(tmp, "%d.csv" % t)
            with open(path, "w") as fp:
                fp.write("from_id\tto_id\tweight\n")
                for s, o, w in zip(snaps["t%d_src" % t], snaps["t%d_dst" % t], snaps["t%d_w" % t]):
                    fp.write("%s\t%s\t%s\n" % (names[s], names[o], repr(float(w)) if w != int(w) else str(int(w))))
            a = ref_utils.get_sp_adj_mat(path, names, sep="\t") + sp.eye(E.N)
            mine = E.snapshot_csr(t)
            for rn in (0, 1):
                m = sp.csr_matrix(ref_utils.get_normalized_adj(a, row_norm=bool(rn)))
                m.sort_indices()
                assert np.array_equal(m.indptr, mine.indptr) and np.array_equal(m.indices, mine.indices)
                t32 = ref_utils.sparse_mx_to_torch_sparse_tensor(m.tocoo()).coalesce()       # the reference's .float()
                d["norm%d_t%d" % (rn, t)] = t32.values().numpy().copy()
                if rn == 0:
                    mats.append(m)
            if t == 0:
                deg = []
            deg.append(np.asarray((a - sp.eye(E.N)).sum(axis=1)).reshape(-1).astype(int))
    width = 1 + max(int(x.max()) for x in deg)
    d["onehot_width"] = np.int64(width)
    for t in range(E.T):
        d["onehot_deg_t%d" % t] = deg[t].astype(np.int64)
    return mats


class Watch(object):
    """records, at every TopK call, the smallest admissible gap among the top k + 1 scores"""

    def __init__(self):
        self.min_gap = np.inf
        self.ok = True

    def hook(self, module, args, output):
        x = args[0]
        x = x.to_dense() if x.is_sparse else x
        with torch.no_grad():
            s = (x.matmul(module.scorer) / module.scorer.norm()).view(-1).double()
            vals, idx = s.topk(module.k + 1)
            scale = float(s.abs().max())
            for a in range(module.k):
                gap = float(vals[a] - vals[a + 1]) / scale
                if torch.equal(x[idx[a]], x[idx[a + 1]]):
                    continue
                self.min_gap = min(self.min_gap, gap)
                if gap < GAP:
                    self.ok = False


def run_case(case, seed, dtype, mats, d, watch=None):
    g = d
    # one-hot features go in dense: the reference's to_dense() test is an isinstance on the legacy float32 sparse type, which a
    # float64 sparse tensor does not pass; a one-hot row times a matrix is a row copy either way
    x = [v.to_dense() if v.is_sparse else v for v in E.features(case, g, dtype)]
    model = ref_egcn.EvolveGCN(E.input_dim(case, g), E.HID, E.OUT, E.egcn_type(case))
    seeded_parameters(model, seed)
    model = model.to(dtype)
    if watch is not None and E.egcn_type(case) == "EGCNH":
        for layer in model.GRCU_layers:
            layer.evolve_weights.choose_topk.register_forward_hook(watch.hook)
    # both runs multiply by what the reference's loader hands over: the matrix values after its .float()
    adj = [ref_utils.sparse_mx_to_torch_sparse_tensor(m.tocoo()).to(dtype) for m in mats]
    weights = E.surrogate_weights(dtype)
    losses, (outs, grads) = E.adam_losses(model, lambda: model(x, adj), weights)
    return model, losses, outs, grads


def rel_err(a, b):
    return float((a.double() - b.double()).abs().max() / max(1e-300, float(b.double().abs().max())))


def main():
    d = {}
    mats = reference_adjacency(d)
    for seed in range(1, 200):
        watch = Watch()
        runs = {}
        for case in E.CASES:
            runs[case] = run_case(case, seed, torch.float64, mats, d, watch)
            if not watch.ok:
                break
        if watch.ok:
            break
        print("seed %d: top-k gap %.3e below %.0e" % (seed, watch.min_gap, GAP))
    else:
        raise SystemExit("no seed met the gap condition")
    print("seed %d, smallest top-k gap %.3e of max|score|" % (seed, watch.min_gap))
    d["seed"], d["min_gap"] = np.int64(seed), np.float64(watch.min_gap)
    for case in E.CASES:
        model, losses, outs, grads = runs[case]
        _, losses32, outs32, grads32 = run_case(case, seed, torch.float32, mats, d)
        d[case + "_losses"] = np.asarray(losses, dtype=np.float64)
        # the 3 losses are held like a tensor of 3 entries: largest error over the largest |loss|
        d[case + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
        for t in range(E.T):
            put_tensor(d, "%s_out_t%d" % (case, t), outs[t])
        d[case + "_yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(E.T)])
        names = sorted(grads)
        d[case + "_keys"] = np.asarray(names)
        d[case + "_shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
        for k in names:
            put_tensor(d, "%s_grad_%s" % (case, k), grads[k])
        d[case + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
        print(case, "losses", losses, "yard out", d[case + "_yard_out"], "yard grad max", d[case + "_yard_grad"].max())
    np.savez_compressed(os.path.join(OUT, "egcn_uci.npz"), **d)
    print("wrote egcn_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "egcn_uci.npz")))


if __name__ == "__main__":
    main()
