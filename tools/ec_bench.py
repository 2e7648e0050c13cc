"""Edge-classification evaluation (ctgcn_amd.evaluation.edge_classification) on two shapes: an America-Air-like window (1 190 nodes,
10 snapshots, 10 repetitions, d = 128, labels = tertiles of the degree product: 100 problems x 18 models in one solve) and config 5's
last snapshot (synthetic 1 M nodes / 8 M edges via ctgcn_amd.synth.powerlaw_edges, 5.6 M train rows, 18 models).

    python tools/ec_bench.py [--workload air-like|synthetic-1m] [--materialised] [--out profiles/ec_bench_<workload>.json]   (GPU)
    python tools/ec_bench.py --workload ... --reference [--out ...]                                                          (host CPU only)

GPU: ms per gradient pass of the pair table (the Hadamard feature formed while a tile is staged) with its share of the HBM byte bound
(two gathered rows per entry) and of the fp32 FLOP bound, the same pass with the scalar staging (the same embedding as a view that is
not 16-byte aligned), ms per Hessian pass, Newton iterations per model, seconds for the whole evaluation (fit + val/test scoring of
every problem), peak device memory.  --materialised adds the only route without the pair table: the [rows, d] fp32 product matrix
built with torch and passed to the node table as an embedding; its build time, pass times and peak memory.  --reference: the
reference's OneVsRestClassifier(LogisticRegression(lbfgs, balanced, max_iter 10000)) on the host CPU, timed for one C on one problem
(air-like) or on a deterministic subsample of SUB train rows (synthetic-1m) and extrapolated linearly to all problems, 6 C and the full
rows (by rows, the snapshots differing in size); labelled extrapolated.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"air-like": dict(nodes=1190, snapshots=10, reps=10, avg_deg=23), "synthetic-1m": dict(nodes=1_000_000, edges=8_000_000)}
HBM_BYTES_PER_S = 8.0e12         # MI355X peak HBM3E bandwidth
FP32_FLOP_PER_S = 157.3e12       # MI355X peak fp32 vector rate
D, C_LIST, K, SUB, STRENGTH = 128, [0.01, 0.1, 1, 5, 10, 20], 3, 100_000, 0.7


def tertiles(key):
    order = np.lexsort((np.arange(len(key)), key))
    lab = np.empty(len(key), np.int64)
    lab[order] = (3 * np.arange(len(key))) // len(key)
    return lab


def labelled(u, v, n):
    """(u, v, label, degree quantile per node): label = tertile of deg[u]·deg[v]."""
    u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    q = np.empty(n, np.float32)
    q[np.lexsort((np.arange(n), deg))] = np.arange(n, dtype=np.float32) / n
    return u, v, tertiles(deg[u] * deg[v]), q


def workload(name):
    """Per snapshot: (from, to, label, degree quantile)."""
    w = WORKLOADS[name]
    if name == "air-like":
        import scipy.sparse as sp
        from ctgcn_amd.synth import dynamic_graph
        out = []
        for g in dynamic_graph(w["nodes"], avg_deg=w["avg_deg"], snapshots=w["snapshots"], seed=2):
            a = sp.triu(sp.csr_matrix(g), 1).tocoo()
            out.append(labelled(a.row, a.col, w["nodes"]))
        return out
    from ctgcn_amd.synth import powerlaw_edges
    return [labelled(*powerlaw_edges(w["nodes"], w["edges"], 1), w["nodes"])]


def embedding(q, seed, dev=None):
    """Noise plus a per-node term that grows with the node's degree quantile, so that E_u ⊙ E_v carries the label."""
    g = np.random.default_rng(seed)
    x = g.standard_normal((len(q), D), dtype=np.float32) + np.float32(STRENGTH) * q[:, None]
    return torch.from_numpy(x).to(dev) if dev is not None else x


def reference(name, snaps):
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    from sklearn import preprocessing
    from ctgcn_amd.evaluation.node_classification import shuffle_split
    u, v, lab, q = snaps[-1]
    E = embedding(q, 0).astype(np.float64)
    tr, va, te = shuffle_split(len(lab), 0.7, 0.2, 0.1, np.random.RandomState(0))
    full_rows = len(tr)
    if len(tr) > SUB:
        tr = tr[:: -(-len(tr) // SUB)]
    lb = preprocessing.LabelBinarizer().fit(np.arange(K))
    t0 = time.time()
    X = E[u[tr]] * E[v[tr]]
    model = OneVsRestClassifier(LogisticRegression(C=1, solver='lbfgs', max_iter=10000, class_weight='balanced')).fit(X, lb.transform(lab[tr]))
    t_fit = (time.time() - t0) * full_rows / len(tr)
    te = te[:SUB]
    acc = float((model.predict_proba(E[u[te]] * E[v[te]]).argmax(1) == lab[te]).mean())
    reps = WORKLOADS[name].get("reps", 1)
    all_rows = reps * sum(int(np.floor(len(s[2]) * 0.7)) for s in snaps)          # the snapshots differ in size: scale by rows
    return {"extrapolated": True, "timed_rows": int(len(tr)), "train_rows": int(full_rows),
            "lbfgs_iterations": [int(e.n_iter_[0]) for e in model.estimators_], "ovr_fit_s_per_C": t_fit, "test_acc_C1": acc,
            "problems": reps * len(snaps), "train_rows_all_problems": all_rows, "evaluation_s": t_fit * len(C_LIST) * all_rows / full_rows,
            "note": "one OvR fit (3 classes, feature product included) timed at C=1 on the last snapshot, scaled linearly in rows to "
                    "every problem and by 6 C (lbfgs iterations held fixed)"}


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(reps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / reps


def gpu(name, snaps, materialised):
    import importlib
    from ctgcn_amd.evaluation import _ovr
    EC = importlib.import_module("ctgcn_amd.evaluation.edge_classification")
    dev = torch.device("cuda:0")
    torch.cuda.reset_peak_memory_stats()
    w = WORKLOADS[name]
    N = w["nodes"]
    embs = [embedding(s[3], t, dev) for t, s in enumerate(snaps)]
    reps = w.get("reps", 1)
    # the pass timings: the window's train problems (air-like) or the one snapshot's (synthetic-1m)
    rng = np.random.RandomState(0)
    E = torch.cat(embs).contiguous()
    probs = []
    for _ in range(reps):
        for t, (u, v, lab, _) in enumerate(snaps):
            tr = EC.shuffle_split(len(lab), 0.7, 0.2, 0.1, rng)[0]
            probs.append(_ovr.Problem(torch.from_numpy(u[tr] + t * N).to(dev), torch.from_numpy(lab[tr].astype(np.int32)).to(dev), K,
                                      rows2=torch.from_numpy(v[tr] + t * N).to(dev)))
    tb = _ovr.Table(E, probs, C_LIST)
    theta = (torch.randn(tb.M, D + 1, device=dev, dtype=torch.float64) * 0.05)
    grad_ms = timed(lambda: tb.loss_grad(theta), 10)
    hess_ms = timed(lambda: [tb.hessian(theta, p0, p1) for p0, p1 in tb.hess_chunks()], 3)
    rows, models = sum(tb.n), tb.max_models
    grad_bytes = rows * (2 * (D * 4 + 8) + 4)                      # each train row: two embedding rows, two indices, the label
    grad_flops = rows * (D + models * (D + 1) * 2 * 3)             # the product, then z (hi and lo parts) and the gradient
    hess_rows = int(tb.n_sub.sum())
    hess_flops = hess_rows * models * (D + 1) * (D + 2)            # upper triangle, one multiply-add each
    passes = {"grad": dict(ms=grad_ms, rows=rows, models_per_row=models, bytes=grad_bytes, flops=grad_flops,
                           hbm_bound_share=grad_bytes / HBM_BYTES_PER_S / (grad_ms * 1e-3),
                           fp32_bound_share=grad_flops / FP32_FLOP_PER_S / (grad_ms * 1e-3)),
              "hess": dict(ms=hess_ms, rows=hess_rows, models_per_row=models, flops=hess_flops,
                           fp32_bound_share=hess_flops / FP32_FLOP_PER_S / (hess_ms * 1e-3))}
    # the scalar staging: the same values behind a view whose rows start 4 bytes off 16-byte alignment
    wide = torch.empty(E.shape[0], D + 4, device=dev)
    wide[:, 1:D + 1] = E
    ts = _ovr.Table(wide[:, 1:D + 1], probs, C_LIST)
    passes["grad_scalar_staging"] = dict(ms=timed(lambda: ts.loss_grad(theta), 10))
    passes["hess_scalar_staging"] = dict(ms=timed(lambda: [ts.hessian(theta, p0, p1) for p0, p1 in ts.hess_chunks()], 3))
    del ts, wide
    out = {"problems": len(probs), "train_rows": rows, "passes": passes}
    peak_fused = torch.cuda.max_memory_allocated()
    if materialised:
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        build_ms = timed(lambda: E[tb.rows] * E[tb.rows2], 3)
        X = E[tb.rows] * E[tb.rows2]
        offs = np.concatenate([[0], np.cumsum(tb.n)])
        node = [_ovr.Problem(torch.arange(offs[i], offs[i + 1], device=dev), p.y, K) for i, p in enumerate(probs)]
        tn = _ovr.Table(X, node, C_LIST)
        out["materialised"] = dict(build_ms=build_ms, matrix_gib=X.numel() * 4 / 2 ** 30, grad_ms=timed(lambda: tn.loss_grad(theta), 10),
                                   hess_ms=timed(lambda: [tn.hessian(theta, p0, p1) for p0, p1 in tn.hess_chunks()], 3),
                                   peak_mem_over_embedding_gib=(torch.cuda.max_memory_allocated() - base) / 2 ** 30,
                                   note="train rows only; the val and test rows would need their own matrices")
        del tn, X, node
    del tb, theta
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.time()
    if name == "air-like":
        res = EC.evaluate_window(torch.stack(embs, 1), [s[:3] for s in snaps], C_LIST, rep_num=reps, seed=5)
        reports, acc = res["reports"], float(res["acc"].mean())
    else:
        u, v, lab, _ = snaps[0]
        arr = np.stack([u, v, lab], 1)
        sp = [torch.from_numpy(arr[i]).to(dev) for i in EC.shuffle_split(len(arr), 0.7, 0.2, 0.1, np.random.RandomState(0))]
        r = EC.evaluate(embs[0], sp[0], sp[1], sp[2], C_LIST, K)
        reports, acc = r["report"], r["acc"]
    torch.cuda.synchronize()
    eval_s = time.time() - t0
    its = [r.iterations for r in reports]
    out.update({"models": len(reports), "newton_iterations": {"min": min(its), "mean": float(np.mean(its)), "max": max(its)},
                "converged": all(r.converged for r in reports), "mean_test_acc": acc, "evaluation_s": eval_s,
                "peak_mem_gib": max(peak_fused, torch.cuda.max_memory_allocated()) / 2 ** 30})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="air-like", choices=sorted(WORKLOADS))
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--materialised", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    snaps = workload(args.workload)
    res = {"workload": args.workload, "nodes": WORKLOADS[args.workload]["nodes"], "snapshots": len(snaps),
           "edges_per_snapshot": [int(len(s[0])) for s in snaps], "d": D, "classes": K, "C_list": C_LIST}
    if args.reference:
        res["reference_host_cpu"] = reference(args.workload, snaps)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("ec_bench.py measures the GPU path: no GPU found (use --reference for the host-CPU reference timing)")
        res["gpu"] = gpu(args.workload, snaps, args.materialised)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
