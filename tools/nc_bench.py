"""Node-classification evaluation (ctgcn_amd.evaluation.node_classification) on two shapes: an America-Air-like window (1 190 nodes,
10 snapshots, 10 repetitions, d = 128, degree-quartile labels: 100 problems x 24 models in one solve) and config 5's last snapshot
(synthetic 1 M nodes via ctgcn_amd.synth.powerlaw_edges, ~700 k train rows, 24 models).

    python tools/nc_bench.py [--workload air-like|synthetic-1m] [--out profiles/nc_bench_<workload>.json]     (GPU)
    python tools/nc_bench.py --workload ... --reference [--out ...]                                            (host CPU only)

GPU: ms per gradient pass with its share of the HBM byte bound and of the fp32 FLOP bound, ms per Hessian pass, Newton iterations per
model, seconds for the whole evaluation (fit + val/test scoring of every problem), peak device memory.  --reference: the reference's
OneVsRestClassifier(LogisticRegression(lbfgs, balanced, max_iter 10000)) on the host CPU, timed for one C on one problem (air-like)
or on a deterministic subsample of SUB train rows (synthetic-1m) and extrapolated linearly to all problems, 6 C and the full rows;
labelled extrapolated.
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
D, C_LIST, K, SUB = 128, [0.01, 0.1, 1, 5, 10, 20], 4, 100_000


def quartiles(deg):
    order = np.lexsort((np.arange(len(deg)), deg))
    lab = np.empty(len(deg), np.int64)
    lab[order] = (4 * np.arange(len(deg))) // len(deg)
    return lab


def workload(name):
    """(labels per snapshot, embedding generator): the embedding is noise plus a planted per-class offset."""
    w = WORKLOADS[name]
    if name == "air-like":
        from ctgcn_amd.synth import dynamic_graph
        graphs = dynamic_graph(w["nodes"], avg_deg=w["avg_deg"], snapshots=w["snapshots"], seed=2)
        return [quartiles(np.asarray(g.sum(1)).ravel()) for g in graphs]
    from ctgcn_amd.synth import powerlaw_edges
    u, v = powerlaw_edges(w["nodes"], w["edges"], 1)
    return [quartiles(np.bincount(np.concatenate([u, v]), minlength=w["nodes"]))]


def embedding(lab, seed, dev=None):
    g = np.random.default_rng(seed)
    x = g.standard_normal((len(lab), D), dtype=np.float32) + 0.15 * lab[:, None].astype(np.float32)
    return torch.from_numpy(x).to(dev) if dev is not None else x


def reference(name, labels):
    from sklearn.linear_model import LogisticRegression
    from sklearn.multiclass import OneVsRestClassifier
    from sklearn import preprocessing
    from ctgcn_amd.evaluation.node_classification import shuffle_split
    lab = labels[-1]
    X = embedding(lab, 0).astype(np.float64)
    tr, va, te = shuffle_split(len(lab), 0.7, 0.2, 0.1, np.random.RandomState(0))
    full_rows = len(tr)
    if len(tr) > SUB:
        tr = tr[:: -(-len(tr) // SUB)]
    lb = preprocessing.LabelBinarizer().fit(np.arange(K))
    t0 = time.time()
    model = OneVsRestClassifier(LogisticRegression(C=1, solver='lbfgs', max_iter=10000, class_weight='balanced')).fit(X[tr], lb.transform(lab[tr]))
    t_fit = (time.time() - t0) * full_rows / len(tr)
    problems = WORKLOADS[name].get("snapshots", 1) * WORKLOADS[name].get("reps", 1)
    return {"extrapolated": True, "timed_rows": int(len(tr)), "train_rows": int(full_rows),
            "lbfgs_iterations": [int(e.n_iter_[0]) for e in model.estimators_], "ovr_fit_s_per_C": t_fit,
            "problems": problems, "evaluation_s": t_fit * len(C_LIST) * problems,
            "note": "one OvR fit (4 classes) timed at C=1, scaled linearly in rows and by 6 C x problems (lbfgs iterations held fixed)"}


def gpu(name, labels):
    import importlib
    from ctgcn_amd.evaluation import _ovr
    NC = importlib.import_module("ctgcn_amd.evaluation.node_classification")
    dev = torch.device("cuda:0")
    torch.cuda.reset_peak_memory_stats()
    w = WORKLOADS[name]
    embs = [embedding(lab, t, dev) for t, lab in enumerate(labels)]

    def timed(fn, reps):
        fn()
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(reps):
            out = fn()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1]) / reps, out

    reps = w.get("reps", 1)
    # the pass timings: the window's train problems (air-like) or the one snapshot's (synthetic-1m)
    rng = np.random.RandomState(0)
    E = torch.cat(embs).contiguous()
    N = len(labels[0])
    probs = []
    for _ in range(reps):
        for t, lab in enumerate(labels):
            tr = NC.shuffle_split(N, 0.7, 0.2, 0.1, rng)[0]
            probs.append(_ovr.Problem(torch.from_numpy(tr + t * N).to(dev), torch.from_numpy(lab[tr].astype(np.int32)).to(dev), K))
    tb = _ovr.Table(E, probs, C_LIST)
    theta = (torch.randn(tb.M, D + 1, device=dev, dtype=torch.float64) * 0.05)
    grad_ms, _ = timed(lambda: tb.loss_grad(theta), 10)
    hess_ms, _ = timed(lambda: [tb.hessian(theta, p0, p1) for p0, p1 in tb.hess_chunks()], 3)
    rows = sum(tb.n)
    models = tb.max_models
    grad_bytes = rows * (D * 4 + 8 + 4)                           # each train row gathered once: embedding row, index, label
    grad_flops = rows * models * (D + 1) * 2 * 3                   # z (hi and lo parts) and the gradient: 3 multiply-adds per (row, model, column)
    hess_rows = int(tb.n_sub.sum())
    passes = {"grad": dict(ms=grad_ms, rows=rows, models_per_row=models, bytes=grad_bytes, flops=grad_flops,
                           hbm_bound_share=grad_bytes / HBM_BYTES_PER_S / (grad_ms * 1e-3),
                           fp32_bound_share=grad_flops / FP32_FLOP_PER_S / (grad_ms * 1e-3)),
              "hess": dict(ms=hess_ms, rows=hess_rows, models_per_row=models,
                           flops=hess_rows * models * (D + 1) * (D + 2),   # upper triangle, one multiply-add each
                           fp32_bound_share=hess_rows * models * (D + 1) * (D + 2) / FP32_FLOP_PER_S / (hess_ms * 1e-3))}
    del tb, theta
    torch.cuda.synchronize()
    t0 = time.time()
    if name == "air-like":
        res = NC.evaluate_window(torch.stack(embs, 1), [(np.arange(N), lab) for lab in labels], C_LIST, rep_num=reps, seed=5)
        reports, acc = res["reports"], float(res["acc"].mean())
    else:
        ix = NC.shuffle_split(N, 0.7, 0.2, 0.1, np.random.RandomState(0))
        sp = [torch.from_numpy(np.stack([i, labels[0][i]], 1)).to(dev) for i in ix]
        r = NC.evaluate(embs[0], sp[0], sp[1], sp[2], C_LIST, K)
        reports, acc = r["report"], r["acc"]
    torch.cuda.synchronize()
    eval_s = time.time() - t0
    its = [r.iterations for r in reports]
    return {"problems": len(probs), "models": len(reports), "train_rows": rows, "passes": passes,
            "newton_iterations": {"min": min(its), "mean": float(np.mean(its)), "max": max(its)},
            "converged": all(r.converged for r in reports), "mean_test_acc": acc, "evaluation_s": eval_s,
            "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="air-like", choices=sorted(WORKLOADS))
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    labels = workload(args.workload)
    res = {"workload": args.workload, "nodes": len(labels[0]), "snapshots": len(labels), "d": D, "classes": K, "C_list": C_LIST}
    if args.reference:
        res["reference_host_cpu"] = reference(args.workload, labels)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("nc_bench.py measures the GPU path: no GPU found (use --reference for the host-CPU reference timing)")
        res["gpu"] = gpu(args.workload, labels)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
