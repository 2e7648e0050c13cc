"""Centrality-prediction evaluation (ctgcn_amd.evaluation.centrality_prediction) of one snapshot on the BASELINE shapes: the UCI
window (7 bundled months), an AS-like snapshot (config 4: 6 828 nodes, 19 500 edges), an Enron-like snapshot (87 k nodes, 530 k
edges) and config 5's last snapshot (synthetic 1 M nodes, 8 M edges), with a d = 128 float32 embedding.

    python tools/cent_bench.py [--workload uci|as-like|enron-like|synthetic-1m] [--out profiles/cent_bench_<workload>.json]   (GPU)
    python tools/cent_bench.py --workload ... --reference [--out ...]                                                         (host CPU)

GPU: ms per centrality (Brandes = closeness + betweenness, eigenvector, kcore), traversed edges per second of the Brandes pass
(sources x directed CSR entries / time), the ridge passes' bytes against the HBM bound, and whether every source ran.  synthetic-1m
runs a fixed prefix of PREFIX sources and labels the all-source figure extrapolated.  --reference: networkx's betweenness on SAMPLE
sampled sources on the host CPU (its per-source cost), scaled to all sources; labelled extrapolated.
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

WORKLOADS = {"uci": dict(nodes=1899, edges=None), "as-like": dict(nodes=6_828, edges=19_500),
             "enron-like": dict(nodes=87_036, edges=530_284), "synthetic-1m": dict(nodes=1_000_000, edges=8_000_000)}
HBM_BYTES_PER_S = 8.0e12         # MI355X peak HBM3E bandwidth
D, ALPHAS, PREFIX, SAMPLE = 128, [0.05, 0.5, 1, 2, 5, 10], 4096, 64


def graphs(name):
    """[(label, n, indptr, indices)] symmetric int32 CSRs."""
    import scipy.sparse as sp
    w = WORKLOADS[name]
    if name == "uci":
        s = np.load(os.path.join(ROOT, "tests", "golden", "uci_snapshots.npz"))
        pairs = [(str(s["files"][t]), s["t%d_src" % t], s["t%d_dst" % t]) for t in range(len(s["files"]))]
    else:
        from ctgcn_amd.synth import powerlaw_edges
        u, v = powerlaw_edges(w["nodes"], w["edges"], 1)
        pairs = [(name, u, v)]
    out = []
    for label, u, v in pairs:
        u, v = np.asarray(u, np.int64), np.asarray(v, np.int64)
        keep = u != v
        m = sp.coo_matrix((np.ones(2 * keep.sum()), (np.r_[u[keep], v[keep]], np.r_[v[keep], u[keep]])), shape=(w["nodes"],) * 2).tocsr()
        m.sum_duplicates()
        m.sort_indices()
        out.append((label, w["nodes"], m.indptr.astype(np.int32), m.indices.astype(np.int32)))
    return out


def reference(name):
    import networkx as nx
    res = []
    for label, n, indptr, indices in graphs(name):
        g = nx.Graph()
        g.add_nodes_from(range(n))
        for u in range(n):
            g.add_edges_from((u, int(x)) for x in indices[indptr[u]:indptr[u + 1]] if u < x)
        k = min(SAMPLE, n)
        t0 = time.time()
        nx.betweenness_centrality(g, k=k, seed=0)
        t = time.time() - t0
        res.append({"snapshot": label, "sampled_sources": k, "betweenness_s": t * n / k, "extrapolated": True})
    return {"networkx": nx.__version__, "snapshots": res,
            "note": "networkx betweenness_centrality(k=%d sampled sources) timed on the host CPU and scaled by n / k" % SAMPLE}


def gpu(name):
    import importlib
    CP = importlib.import_module("ctgcn_amd.evaluation.centrality_prediction")
    dev = torch.device("cuda:0")

    def timed(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3 / reps, out

    res = []
    for label, n, indptr, indices in graphs(name):
        rp, col = torch.from_numpy(indptr).to(dev), torch.from_numpy(indices).to(dev)
        nnz = int(indices.size)
        s1 = n if n <= 100_000 else PREFIX
        reps = 3 if n <= 10_000 else 1
        br_ms, (bc, r, D_) = timed(lambda: CP.brandes(rp, col, 0, s1), reps)
        all_ran = bool((r >= 1).all().item()) and r.numel() == s1
        eig_ms, (_, stop) = timed(lambda: CP.eigenvector(rp, col), reps)
        from ctgcn_amd import ops
        kc_ms, _ = timed(lambda: ops.kcore(rp, col), reps)
        gen = torch.Generator(device=dev).manual_seed(1)
        X = torch.randn(n, D, device=dev, generator=gen)
        Y = torch.rand(n, 4, device=dev, dtype=torch.float64, generator=gen)
        ridge_ms, _ = timed(lambda: CP.ridge_cv_errors(X, Y, ALPHAS, 5), reps)
        ridge_bytes = 2 * n * (D * 4 + 4 * 8)          # two passes over X (float32) and the targets
        entry = {"snapshot": label, "nodes": n, "csr_entries": nnz, "sources_run": s1, "every_source_ran": all_ran and s1 == n,
                 "brandes_ms": br_ms, "traversed_edges_per_s": s1 * nnz / (br_ms * 1e-3),
                 "eigenvector_ms": eig_ms, "eigenvector_steps": stop, "kcore_ms": kc_ms,
                 "ridge_ms": ridge_ms, "ridge_bytes": ridge_bytes, "ridge_hbm_bound_share": ridge_bytes / HBM_BYTES_PER_S / (ridge_ms * 1e-3)}
        if s1 < n:
            entry["brandes_all_sources_ms_extrapolated"] = br_ms * n / s1
        res.append(entry)
    return {"snapshots": res, "total_ms": sum(e["brandes_ms"] + e["eigenvector_ms"] + e["kcore_ms"] + e["ridge_ms"] for e in res),
            "peak_mem_gib": torch.cuda.max_memory_allocated() / 2 ** 30}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uci", choices=sorted(WORKLOADS))
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"workload": args.workload, "d": D}
    if args.reference:
        res["reference_host_cpu"] = reference(args.workload)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("cent_bench.py measures the GPU path: no GPU found (use --reference for the host-CPU reference timing)")
        res["gpu"] = gpu(args.workload)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
