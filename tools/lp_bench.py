"""Link-prediction evaluation of one snapshot (ctgcn_amd.evaluation) on the BASELINE shapes: config 5's last snapshot (synthetic 1 M
nodes, 8 M undirected edges) and an Enron-like snapshot (87 k nodes, 530 k edges), with a planted-signal d = 128 embedding.

    python tools/lp_bench.py [--workload synthetic-1m|enron-like] [--out profiles/lp_bench_<workload>.json]     (GPU)
    python tools/lp_bench.py --workload ... --reference [--out ...]                                              (host CPU only)

GPU: sampler ms, ms per fused pass in each mode with the bytes it must move and its share of the HBM bound, Newton iterations per
model, seconds per snapshot (splits + 16 fits + AUCs), peak device memory.  --reference: the reference's algorithm on the host CPU
(dict-checked one-at-a-time negative draws; one float64 feature matrix and one sklearn LogisticRegression(lbfgs, balanced) fit), timed
on a deterministic subsample of SUB rows and extrapolated linearly to the full split and to 4 measures x 4 C; labelled extrapolated.
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

WORKLOADS = {"synthetic-1m": dict(nodes=1_000_000, edges=8_000_000), "enron-like": dict(nodes=87_036, edges=530_284)}
HBM_BYTES_PER_S = 8.0e12         # MI355X peak HBM3E bandwidth
D, C_LIST, MEASURES, SUB = 128, [0.01, 0.1, 1, 10], ["Avg", "Had", "L1", "L2"], 100_000


def graph(w):
    from ctgcn_amd.synth import powerlaw_edges
    u, v = powerlaw_edges(w["nodes"], w["edges"], 1)
    return np.stack([u, v], 1).astype(np.int64)


def reference(w, pos):
    """Host-CPU timing of the reference's algorithm on SUB rows, extrapolated."""
    from sklearn.linear_model import LogisticRegression
    n = w["nodes"]
    rng = np.random.RandomState(0)
    edge_dict = {}
    for a, b in pos:
        edge_dict[(a, b)] = 1
        edge_dict[(b, a)] = 1
    E_rows = 2 * len(pos)
    train_num = int(np.floor((E_rows - int(E_rows * 0.2) - int(E_rows * 0.3)) * 0.5))
    t0 = time.time()
    cnt = 0
    while cnt < SUB:
        a, b = rng.choice(n), rng.choice(n)
        if a == b or (a, b) in edge_dict or (b, a) in edge_dict:
            continue
        cnt += 1
    t_neg = (time.time() - t0) * (E_rows // 2) / SUB          # negatives of all splits = E_rows / 2 in total (ratios 0.5/0.3/0.2)
    emb = np.random.RandomState(1).standard_normal((n, D))
    idx = rng.randint(0, len(pos), SUB // 2)
    rows = np.concatenate([pos[idx], rng.randint(0, n, (SUB // 2, 2))])
    y = np.r_[np.ones(SUB // 2), np.zeros(SUB // 2)]
    emb[rows[: SUB // 2, 1]] += 0.5 * emb[rows[: SUB // 2, 0]]
    t0 = time.time()
    feat = np.array([emb[a] * emb[b] for a, b in rows])
    t_feat = time.time() - t0
    t0 = time.time()
    model = LogisticRegression(C=1, solver='lbfgs', max_iter=10000, class_weight='balanced').fit(feat, y)
    t_fit = time.time() - t0
    scale = 2 * train_num / SUB
    return {"extrapolated": True, "subsample_rows": SUB, "lbfgs_iterations": int(model.n_iter_[0]),
            "neg_sampling_s": t_neg, "feature_s_per_measure": t_feat * scale, "fit_s_per_model": t_fit * scale,
            "snapshot_s": t_neg + 4 * t_feat * scale * 1.8 + 16 * t_fit * scale,
            "note": "one fit timed at C=1 on %d rows, scaled linearly in rows (lbfgs iterations held fixed); features of train+val+test "
                    "(1.8 x train rows) per measure" % SUB}


def gpu(w, pos_np):
    from ctgcn_amd.evaluation import _logreg
    import importlib
    LP = importlib.import_module("ctgcn_amd.evaluation.link_prediction")
    dev = torch.device("cuda:0")
    n = w["nodes"]
    pos = torch.from_numpy(pos_np).to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    base = torch.randn(n, D, device=dev, generator=gen)
    A = torch.sparse_coo_tensor(torch.cat([pos.t(), pos.flip(1).t()], 1), torch.ones(2 * pos.shape[0], device=dev), (n, n))
    deg = torch.sparse.sum(A, 1).to_dense().clamp_min(1)
    E = (base + 0.5 * torch.sparse.mm(A, base) / deg[:, None]).contiguous()
    del A

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

    torch.cuda.reset_peak_memory_stats()
    both = torch.stack([pos, pos.flip(1)], 1).reshape(-1, 2)
    keys = LP.membership_keys(both, n)
    tn, vn, sn = LP.split_counts(both.shape[0], 0.5, 0.3, 0.2)
    neg_ms, _ = timed(lambda: LP.sample_negatives(keys, n, tn + vn + sn, 7, dev), 3)
    split_ms, (train, val, test) = timed(lambda: LP.make_splits(pos, n, 0.5, 0.3, 0.2, seed=9), 3)
    tr = _logreg.EdgeSet(train, n)
    models = [m for m in MEASURES for _ in C_LIST]
    W = torch.randn(16, D + 1, device=dev) * 0.05
    grad_ms, _ = timed(lambda: _logreg.loss_grad(E, tr, models, W), 5)
    hs = tr.subsample(1 << 18)
    hess_ms, _ = timed(lambda: _logreg.hessian(E, hs, models, W), 5)
    score_ms, _ = timed(lambda: _logreg.scores(E, tr, models, W), 5)
    edge_bytes = 2 * D * 4 + 2 * 8 + 1
    passes = {
        "grad": dict(ms=grad_ms, rows=tr.n, bytes=tr.n * edge_bytes),
        "hess": dict(ms=hess_ms, rows=hs.n, bytes=hs.n * edge_bytes),
        "scores": dict(ms=score_ms, rows=tr.n, bytes=tr.n * (edge_bytes - 1 + 16 * 4)),
    }
    for p in passes.values():
        p["hbm_bound_share"] = p["bytes"] / HBM_BYTES_PER_S / (p["ms"] * 1e-3)
    torch.cuda.synchronize()
    t0 = time.time()
    res = LP.evaluate(E, train, val, test, C_LIST, MEASURES + ["sigmoid"])
    torch.cuda.synchronize()
    eval_s = time.time() - t0
    return {"sampler_ms": neg_ms, "splits_ms": split_ms, "train_rows": tr.n, "passes": passes,
            "newton_iterations": {"%s/C=%g" % (r.measure, r.C): r.iterations for r in res["report"]},
            "converged": all(r.converged for r in res["report"]), "auc": res["auc"], "chosen_C": res["C"],
            "evaluate_s": eval_s, "snapshot_s": eval_s + split_ms * 1e-3,
            "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1m", choices=sorted(WORKLOADS))
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    w = WORKLOADS[args.workload]
    pos = graph(w)
    res = {"workload": args.workload, "nodes": w["nodes"], "undirected_edges": int(len(pos)), "d": D}
    if args.reference:
        res["reference_host_cpu"] = reference(w, pos)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("lp_bench.py measures the GPU path: no GPU found (use --reference for the host-CPU reference timing)")
        res["gpu"] = gpu(w, pos)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
