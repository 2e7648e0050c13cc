"""Similarity-prediction evaluation (ctgcn_amd.evaluation.similarity_prediction) on the BASELINE shapes: the UCI window (7 bundled
months, weighted), an AS-like snapshot (config 4: 6 828 nodes, 19 500 edges) and an Enron-like snapshot (87 k nodes, 530 k edges),
alpha 0.5 and 100 steps as in config/uci.json, with a d = 128 float32 embedding.

    python tools/sim_bench.py [--workload uci|as-like|enron-like] [--out profiles/sim_bench_<workload>.json]      (GPU)
    python tools/sim_bench.py --workload ... --reference [--out ...]                                            (host CPU)

GPU, per snapshot: ms for lambda_1 (host eigsh), the series, the finish passes, the COO compaction and the predictor (Gram, the two
normalisations and the Spearman pass), and peak device memory.  The series is set against a bytes model: it gathers
iter · (nnz + m) · m · 8 bytes of panel rows, bounded by the 8.6 TB/s Infinity-Cache gather rate, and writes m² · 8 bytes to HBM
(8 TB/s).  At Enron-like size only the generator runs (m² ≈ 7.6 G values are too many for the sort) and the COO is counted, not
written.  --reference: the same algorithm with numpy / scipy (CSR x dense product, scipy.stats.spearmanr) on the host CPU; sizes
the host cannot hold are timed on a prefix of columns and labelled extrapolated.
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
             "enron-like": dict(nodes=87_036, edges=530_284)}
IC_GATHER_BYTES_PER_S = 8.6e12   # MI355X_MICROARCH: uniformly gathered rows served by the Infinity Cache
HBM_BYTES_PER_S = 8.0e12
D, ALPHA, ITERS = 128, 0.5, 100
HOST_PREFIX = 256                # columns of the series the host reference runs when n x n does not fit comfortably


def graphs(name):
    """[(label, scipy CSR float64)] symmetric, sorted, no self loops, no zeros."""
    from ctgcn_amd.utils import symmetric_csr_from_rows
    w = WORKLOADS[name]
    if name == "uci":
        s = np.load(os.path.join(ROOT, "tests", "golden", "uci_snapshots.npz"))
        rows = [(str(s["files"][t]), s["t%d_src" % t], s["t%d_dst" % t], s["t%d_w" % t]) for t in range(len(s["files"]))]
    else:
        from ctgcn_amd.synth import powerlaw_edges
        u, v = powerlaw_edges(w["nodes"], w["edges"], 1)
        rows = [(name, u, v, np.ones(len(u)))]
    out = []
    for label, u, v, x in rows:
        A = symmetric_csr_from_rows(u, v, x, w["nodes"])
        A.eliminate_zeros()
        out.append((label, A))
    return out


def reference(name):
    import scipy.sparse as sp
    import scipy.stats
    from ctgcn_amd.evaluation.similarity_prediction import host_lambda_1
    res = []
    for label, A in graphs(name):
        n = A.shape[0]
        t0 = time.time()
        lam = host_lambda_1(A)
        lam_s = time.time() - t0
        cols = n if n <= 10_000 else HOST_PREFIX
        c = ALPHA / lam
        eye = sp.eye(n, cols, format="csr").toarray()
        S = np.zeros((n, cols))
        t0 = time.time()
        for _ in range(ITERS):
            S = c * A.dot(S) + eye
        series_s = (time.time() - t0) * n / cols
        entry = {"snapshot": label, "nodes": n, "csr_entries": int(A.nnz), "lambda_s": lam_s, "series_s": series_s,
                 "series_extrapolated": cols < n}
        if cols == n:
            t0 = time.time()
            S = (S + S.T) / 2 - np.eye(n)
            S = (S - S.min()) / (S.max() - S.min())
            S[S < 1e-6] = 0
            C = sp.coo_matrix(S)
            entry["finish_coo_s"] = time.time() - t0
            keep = np.nonzero(S.sum(1) >= 1e-6)[0]
            E = np.random.default_rng(0).standard_normal((n, D))
            t0 = time.time()
            real, pred = S[np.ix_(keep, keep)], (E @ E.T)[np.ix_(keep, keep)]
            real = (real - real.min()) / (real.max() - real.min())
            pred = (pred - pred.min()) / (pred.max() - pred.min())
            scipy.stats.spearmanr((real / real.sum()).ravel(), (pred / pred.sum()).ravel())
            entry["predictor_s"] = time.time() - t0
            entry["coo_nnz"] = int(C.nnz)
        res.append(entry)
    return {"snapshots": res, "note": "numpy/scipy on the host CPU; a series marked extrapolated ran %d columns, scaled by n / %d"
            % (HOST_PREFIX, HOST_PREFIX)}


def gpu(name):
    import importlib
    SIM = importlib.import_module("ctgcn_amd.evaluation.similarity_prediction")
    from ctgcn_amd import _lib
    from ctgcn_amd._lib import check, ptr
    dev = torch.device("cuda:0")
    lib = _lib.load()
    st = torch.cuda.current_stream(dev).cuda_stream

    def timed(fn, reps=1):
        fn()
        torch.cuda.synchronize()
        t0 = time.time()
        for _ in range(reps):
            out = fn()
        torch.cuda.synchronize()
        return (time.time() - t0) * 1e3 / reps, out

    res = []
    for label, A in graphs(name):
        n = A.shape[0]
        torch.cuda.reset_peak_memory_stats(dev)
        t0 = time.time()
        lam = SIM.host_lambda_1(A)
        lam_ms = (time.time() - t0) * 1e3
        rp = torch.from_numpy(A.indptr.astype(np.int32)).to(dev)
        deg = np.diff(A.indptr)
        keep = np.nonzero(deg > 0)[0]
        m = len(keep)
        B = A[keep][:, keep].tocsr()
        B.sort_indices()
        rpb = torch.from_numpy(B.indptr.astype(np.int32)).to(dev)
        colb = torch.from_numpy(B.indices.astype(np.int32)).to(dev)
        valb = torch.from_numpy(B.data.astype(np.float64)).to(dev)
        nnz = int(B.nnz)
        panel = int(lib.ctgcn_sim_panel_cols(m, nnz))
        S = torch.empty(m, m, dtype=torch.float64, device=dev)
        nb = lib.ctgcn_sim_series_workspace_bytes(m, panel)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        c = ALPHA / lam
        reps = 3 if m <= 2_000 else 1
        series_ms, _ = timed(lambda: check(lib.ctgcn_sim_series(m, ptr(rpb), ptr(colb), ptr(valb), c, ITERS, panel, 0, m, ptr(S), ptr(ws),
                                                                 nb, st), "series"), reps)
        del ws
        gather_bytes = ITERS * (nnz + m) * m * 8
        entry = {"snapshot": label, "nodes": n, "non_isolated": m, "csr_entries": nnz, "panel_cols": panel, "panels": -(-m // panel),
                 "lambda_ms": lam_ms, "series_ms": series_ms, "series_gather_bytes": gather_bytes,
                 "series_ic_gather_bound_share": gather_bytes / IC_GATHER_BYTES_PER_S / (series_ms * 1e-3),
                 "s_write_hbm_ms_bound": m * m * 8 / HBM_BYTES_PER_S * 1e3}
        stats = torch.empty(2, dtype=torch.float64, device=dev)
        row_nnz = torch.empty(m, dtype=torch.int64, device=dev)
        nb = lib.ctgcn_sim_finish_workspace_bytes(m)
        ws = torch.empty(nb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        t0 = time.time()
        check(lib.ctgcn_sim_finish(m, int(n > m), SIM.EPS, ptr(S), ptr(stats), ptr(row_nnz), ptr(ws), nb, st), "finish")
        torch.cuda.synchronize()
        entry["finish_ms"] = (time.time() - t0) * 1e3
        smin, smax = (float(v) for v in stats.cpu().numpy())
        sim = SIM.Similarity(n, torch.from_numpy(keep).to(dev), S, row_nnz, lam, c, smin, smax)
        entry["coo_nnz"] = int(row_nnz.sum().item())
        if name != "enron-like":
            coo_ms, _ = timed(sim.coo, reps)
            entry["coo_ms"] = coo_ms
            E = torch.randn(n, D, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
            pred_ms, err = timed(lambda: SIM.prediction_error(sim, E, label), reps)
            entry["predictor_ms"] = pred_ms
            entry["spearman"] = err[1]
            entry["kept_rows"] = int(sim.kept().numel())
        entry["peak_mem_gib"] = torch.cuda.max_memory_allocated(dev) / 2 ** 30
        res.append(entry)
        del S, sim, ws
        torch.cuda.empty_cache()
    return {"snapshots": res, "series_ms_total": sum(e["series_ms"] for e in res),
            "total_ms": sum(e["lambda_ms"] + e["series_ms"] + e["finish_ms"] + e.get("coo_ms", 0) + e.get("predictor_ms", 0) for e in res)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="uci", choices=sorted(WORKLOADS))
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    res = {"workload": args.workload, "d": D, "alpha": ALPHA, "iter_num": ITERS}
    if args.reference:
        res["reference_host_cpu"] = reference(args.workload)
    else:
        if not torch.cuda.is_available():
            raise SystemExit("sim_bench.py measures the GPU path: no GPU found (use --reference for the host-CPU timing)")
        res["gpu"] = gpu(args.workload)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
