"""EvolveGCN (EGCN-H, hidden = embed = 128, as every reference config sets it) on three window shapes, with the GCN step
Y = rrelu(Â (X Q_t)) computed three ways:

  fused      ctgcn_amd.baseline.EvolveGCN as shipped: ops.gcn_layer (ctgcn_gcn.hip) forward and backward, the next layer's top-k
             scores from the forward's epilogue
  composed   the same module with the aggregation composed from ops.spmm_csr, F.rrelu and a torch score product; ops.spmm_csr has
             no backward, so this variant is timed in the forward only
  torch      the same module with the step in stock torch ops: torch.sparse.mm, F.rrelu, the scores from a torch product on the layer
             input, autograd for the backward

    python tools/egcn_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out profiles/egcn_bench_<workload>.json]     (GPU)

  uci-like       1 899 nodes, 7 snapshots, average degree 14, gaussian degree features [N, 1 + max degree]
  enron-like     87 000 nodes, 10 snapshots, average degree 13, gaussian degree features [N, 1 + max degree] (largest degree about 500)
  synthetic-1m   config 5's last snapshot: 1 M nodes, 8 M edges (17 M stored entries with the diagonal), one snapshot, 128-wide dense
                 features.  Degree features at that size are N x (1 + max degree), about 2 000 columns or 8 GB per snapshot and a
                 [N, 2 000] x [2 000, 128] product per layer-1 step; they fit neither here nor in the reference, which is why this
                 workload takes dense features.

Per variant: the median over REPS timed calls (after 3 warm-up calls, the variants taking turns inside every repetition) of one epoch
(forward, surrogate loss sum(out * C), backward, Adam step) and of one forward under no_grad, both between device events followed
by a synchronise; peak device memory of an epoch above what the inputs, the model and the optimizer hold; and the largest difference
of the first forward's outputs from the torch variant's, over the largest magnitude.  By-bytes traffic of the step (computed from the
shapes, see gcn_step_bytes) goes on the record beside the times, with the GCN step of the last snapshot timed alone at width 128:
the fused forward and backward against the same step composed from ops.spmm_csr and torch element-wise ops (gcn_step_ms).
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
REPS = {"uci-like": 30, "enron-like": 10, "synthetic-1m": 5}
SHAPES = {"uci-like": dict(n=1899, snapshots=7, avg_deg=14, max_degree_hint=None, features="degree"),
          "enron-like": dict(n=87000, snapshots=10, avg_deg=13, max_degree_hint=500, features="degree"),
          "synthetic-1m": dict(n=1000000, snapshots=1, avg_deg=16, max_degree_hint=None, features="dense")}


def window(name, dev):
    """(features, GcnAdj list, input width): D^-1/2 (A + I) D^-1/2 of every snapshot, scaled on the GPU"""
    import scipy.sparse as sp
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    graphs = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])
    adjs, degs = [], []
    for g in graphs:
        m = (g + sp.eye(s["n"])).tocsr()
        m.sort_indices()
        raw = ops.GcnAdj.from_scipy(m, dev)
        adjs.append(ops.GcnAdj(raw.row_ptr, raw.col, ops.gcn_normalize(raw.row_ptr, raw.col, raw.val, False)))
        degs.append(np.diff(g.indptr))
    gen = torch.Generator(device=dev).manual_seed(0)
    if s["features"] == "dense":
        width = D
        xs = [torch.randn(s["n"], width, generator=gen, device=dev) for _ in graphs]
    else:
        width = 1 + max(int(d.max()) for d in degs)
        xs = [torch.randn(s["n"], width, generator=gen, device=dev) * 1e-4 + torch.from_numpy(d.astype(np.float32)).to(dev).view(-1, 1)
              for d in degs]
    return xs, adjs, width


def composed_aggregate(self, S, adj, score_vec):
    from ctgcn_amd import ops
    Y = F.rrelu(ops.spmm_csr(adj.row_ptr, adj.col, adj.val, S))
    return Y, (None if score_vec is None else Y.matmul(score_vec))


_sparse = {}


def torch_aggregate(self, S, adj, score_vec):
    A = _sparse.get(id(adj))
    if A is None:
        A = _sparse[id(adj)] = adj.to_sparse_tensor().coalesce()
    return F.rrelu(torch.sparse.mm(A, S)), None        # no scores: the next layer's TopK takes its torch product on the layer input


def variant(model, kind):
    m = copy.deepcopy(model)
    fn = {"fused": None, "composed": composed_aggregate, "torch": torch_aggregate}[kind]
    if fn is not None:
        for unit in m.GRCU_layers:
            unit.aggregate = types.MethodType(fn, unit)
    return m


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def round_robin(fns, reps):
    """median ms per key: 3 warm-up calls each, then `reps` rounds in which the variants take turns"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [float(min(v)), float(max(v))] for k, v in times.items()}


def gcn_step_bytes(n, nnz, d):
    """bytes one GCN step moves, by the shapes: the gather reads one d-wide row per stored entry plus the CSR, every N x d pass moves
    n d 4 bytes.  fused forward: gather + write Y.  stock forward: gather + write P, read P + write Y (rrelu), read Y (scores).
    fused backward: gather of dY and Y rows + write dS.  stock backward: read Y and dY + write G (mask), gather G + write dS."""
    row, gather, csr = n * d * 4, nnz * d * 4, nnz * 8 + n * 4
    return {"fused_fwd": gather + csr + row, "stock_fwd": gather + csr + 4 * row,
            "fused_bwd": 2 * gather + csr + row, "stock_bwd": gather + csr + 4 * row}


def gcn_step_ms(adj, reps):
    """the GCN step alone on one snapshot at width D: the fused forward (with the score epilogue) and backward against the same step
    composed from ops.spmm_csr and torch element-wise ops (forward: SpMM, rrelu, score product; backward: masked copy of dY, SpMM)"""
    from ctgcn_amd import ops
    dev = adj.device
    gen = torch.Generator(device=dev).manual_seed(2)
    S, dY = (torch.randn(adj.n, D, generator=gen, device=dev) for _ in range(2))
    p = torch.randn(D, generator=gen, device=dev)
    Y = ops._gcn_fwd(adj, S, 1, None)[0]
    slope = (1.0 / 8.0 + 1.0 / 3.0) / 2.0

    def composed_fwd():
        out = F.rrelu(ops.spmm_csr(adj.row_ptr, adj.col, adj.val, S))
        return out, out.matmul(p)

    def composed_bwd():
        return ops.spmm_csr(adj.row_ptr, adj.col, adj.val, torch.where(Y > 0, dY, dY * slope))

    ms, _ = round_robin({"fused_fwd": lambda: ops._gcn_fwd(adj, S, 1, p), "composed_fwd": composed_fwd,
                         "fused_bwd": lambda: ops._gcn_bwd(adj, dY, Y, 1), "composed_bwd": composed_bwd}, reps)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "egcn_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("egcn_bench measures on the GPU; no device found")
    from ctgcn_amd import EvolveGCN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    xs, adjs, width = window(name, dev)
    n, T = xs[0].shape[0], len(xs)
    base_model = EvolveGCN(width, D, D, "EGCNH").to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    cs = [torch.randn(n, D, generator=gen, device=dev) for _ in range(T)]
    kinds = ("fused", "composed", "torch")
    models = {k: variant(base_model, k) for k in kinds}
    opts = {k: torch.optim.Adam(models[k].parameters(), lr=1e-3) for k in ("fused", "torch")}

    def epoch_of(k):
        def run():
            outs = models[k](xs, adjs)
            sum((o * c).sum() for o, c in zip(outs, cs)).backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def forward_of(k):
        def run():
            with torch.no_grad():
                models[k](xs, adjs)
        return run

    with torch.no_grad():
        first = {k: [o.clone() for o in models[k](xs, adjs)] for k in kinds}
    top = max(float(o.abs().max()) for o in first["torch"])
    agreement = {k: max(float((a - b).abs().max()) for a, b in zip(first[k], first["torch"])) / top for k in ("fused", "composed")}
    del first
    # the optimizer state exists from the first step on: take one step per trained variant before the memory baseline
    for k in opts:
        epoch_of(k)()
    peak = {}
    for k in opts:
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        epoch_of(k)()
        torch.cuda.synchronize()
        peak[k] = (torch.cuda.max_memory_allocated() - held) / 2 ** 30
    forward_ms, forward_range = round_robin({k: forward_of(k) for k in kinds}, REPS[name])
    epoch_ms, epoch_range = round_robin({k: epoch_of(k) for k in opts}, REPS[name])
    nnz = [a.nnz for a in adjs]
    step_ms = gcn_step_ms(adjs[-1], REPS[name])
    step_bytes = gcn_step_bytes(n, nnz[-1], D)
    res = {"workload": name, "device": torch.cuda.get_device_name(0), "shape": dict(SHAPES[name], input_width=width, hidden=D, embed=D,
                                                                                     stored_entries=nnz),
           "reps": REPS[name], "warmup": 3, "egcn_type": "EGCNH",
           "epoch_ms": epoch_ms, "epoch_ms_min_max": epoch_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "epoch_peak_mem_gib": peak, "first_forward_max_diff_vs_torch": agreement,
           "epoch_speedup_fused_vs_torch": epoch_ms["torch"] / epoch_ms["fused"],
           "forward_speedup_fused_vs_torch": forward_ms["torch"] / forward_ms["fused"],
           "forward_speedup_fused_vs_composed": forward_ms["composed"] / forward_ms["fused"],
           "gcn_step_bytes_last_snapshot": step_bytes, "gcn_step_ms_last_snapshot": step_ms,
           "gcn_step_gb_per_s_by_bytes": {"fused_fwd": step_bytes["fused_fwd"] / step_ms["fused_fwd"] / 1e6,
                                          "composed_fwd": step_bytes["stock_fwd"] / step_ms["composed_fwd"] / 1e6,
                                          "fused_bwd": step_bytes["fused_bwd"] / step_ms["fused_bwd"] / 1e6,
                                          "composed_bwd": step_bytes["stock_bwd"] / step_ms["composed_bwd"] / 1e6}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
