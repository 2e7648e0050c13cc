"""Top-k link ranking: the fused HIP pass (ops.topk_scores) against stock torch on the same GPU.

    python tools/topk_bench.py [--workload uci-like|enron-like|synthetic-1m|all] [--out profiles]

k = 100, d = 128, self excluded, seeded normal embeddings.  The two alternatives are timed in alternation in one process with device
events after a warm-up of every shape, and the medians are reported:
  fused   ops.topk_scores(E, k, rows, exclude_self=True): no score matrix
  torch   torch.topk(E[r0:r1] @ E.T, k) over row chunks of at most 2 GiB of scores, the self entry set to -inf
For both: the time, the peak device memory above the inputs, and 2 m n d over the time as a share of the 157.3 TFLOP/s exact-fp32
matrix peak (the pass is compute bound: reading E once is n d 4 bytes, microseconds at 8 TB/s).  For the fused pass that time is the
whole call (sweep kernel, merge kernel and two allocations), so its share is a floor on the sweep kernel's.
Writes <out>/topk_bench_<workload>.json.  Needs the GPU: there is no CPU path.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ctgcn_amd import ops  # noqa: E402

K, D = 100, 128
PEAK_FP32_MATRIX = 157.3e12
WORKLOADS = {"uci-like": (1899, None, 30), "enron-like": (87000, None, 7), "synthetic-1m": (1000000, 16384, 5)}     # n, query rows, reps
CHUNK_BYTES = 2 << 30


def torch_topk(E, rows, k):
    n = E.shape[0]
    m = n if rows is None else rows.numel()
    step = max(1, CHUNK_BYTES // (4 * n))
    score = torch.empty(m, k, dtype=torch.float32, device=E.device)
    index = torch.empty(m, k, dtype=torch.int64, device=E.device)
    for r0 in range(0, m, step):
        r1 = min(m, r0 + step)
        q = torch.arange(r0, r1, device=E.device) if rows is None else rows[r0:r1].to(torch.int64)
        s = E[q] @ E.T
        s[torch.arange(r1 - r0, device=E.device), q] = float("-inf")
        score[r0:r1], index[r0:r1] = torch.topk(s, k, dim=1)
        del s
    return score, index


def run(name, out_dir):
    n, m, reps = WORKLOADS[name]
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(20261021)
    E = torch.randn(n, D, generator=g).to(dev)
    rows = None if m is None else torch.randperm(n, generator=g)[:m].to(torch.int32).to(dev)
    m = n if m is None else m
    alts = {"fused": lambda: ops.topk_scores(E, K, rows=rows, exclude_self=True), "torch": lambda: torch_topk(E, rows, K)}
    results = {}
    for alt, fn in alts.items():            # warm-up of every shape, and the peak memory of one call
        fn()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        results[alt] = fn()
        torch.cuda.synchronize()
        results[alt + "_peak"] = torch.cuda.max_memory_allocated() - base
    times = {alt: [] for alt in alts}
    for _ in range(reps):
        for alt, fn in alts.items():
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            fn()
            end.record()
            end.synchronize()
            times[alt].append(start.elapsed_time(end))
    fi, ti = results["fused"][1].to(torch.int64), results["torch"][1]
    same_rows = float((fi == ti).all(1).double().mean())
    same_sets = float((fi.sort(1)[0] == ti.sort(1)[0]).all(1).double().mean())
    score_diff = float((results["fused"][0] - results["torch"][0]).abs().max())
    flop = 2.0 * m * n * D
    rec = {"workload": name, "device": torch.cuda.get_device_name(0), "shape": {"n": n, "query_rows": m, "d": D, "k": K},
           "reps": reps, "warmup": 2, "flop_2mnd": flop, "bound": "compute (fp32 matrix cores, 157.3 TFLOP/s peak)",
           "col_chunks_default": max(1, min((1024 + (m + 31) // 32 - 1) // ((m + 31) // 32), (n + 31) // 32, 64)),
           "agreement": {"rows_with_identical_lists": same_rows, "rows_with_identical_sets": same_sets, "max_abs_score_diff": score_diff}}
    for alt in alts:
        med = statistics.median(times[alt])
        rec[alt] = {"ms_median": med, "ms_min_max": [min(times[alt]), max(times[alt])], "peak_bytes_above_inputs": results[alt + "_peak"],
                    "tflops_2mnd_over_time": flop / (med * 1e-3) / 1e12, "share_of_fp32_matrix_peak": flop / (med * 1e-3) / PEAK_FP32_MATRIX}
    rec["speedup_fused_vs_torch"] = rec["torch"]["ms_median"] / rec["fused"]["ms_median"]
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "topk_bench_%s.json" % name)
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps({"workload": name, "fused_ms": rec["fused"]["ms_median"], "torch_ms": rec["torch"]["ms_median"],
                      "speedup": rec["speedup_fused_vs_torch"], "fused_share_of_peak": rec["fused"]["share_of_fp32_matrix_peak"],
                      "same_sets": same_sets}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=sorted(WORKLOADS) + ["all"])
    ap.add_argument("--out", default="profiles")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("topk_bench needs the GPU: nothing is measured without one")
    for w in (WORKLOADS if args.workload == "all" else [args.workload]):
        run(w, args.out)
