"""GAT (identity features, alpha 0.2, dropout 0.5, U-neg) on three window shapes and two layer shapes, computed two ways:

  fused   ctgcn_amd.baseline.GAT as shipped: ops.gat_conv (ctgcn_gat.hip)
  torch   the same parameters in stock torch ops: an index gather of the endpoint rows, the row-shifted softmax by scatter_reduce /
          index_add, F.dropout, F.elu, autograd (what tests/_gat_ref.py mirrors, with torch's own dropout)

    python tools/gat_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out profiles/gat_bench_<workload>.json]     (GPU)

  uci-like       1 899 nodes, 7 snapshots, average degree 14
  enron-like     87 000 nodes, 10 snapshots, average degree 13 (largest degree about 500)
  synthetic-1m   1 M nodes, 8 M edges (17 M stored entries) per snapshot, a window of 2 snapshots
  shapes         config: 1 head x 500 -> 128 (every reference config); paper: 8 heads x 64 -> 128

Per shape and variant: the median over REPS timed calls (after 3 warm-up calls, the variants taking turns inside every repetition) of
one training step in train() mode (forward with dropout, surrogate loss sum(out * C), backward, Adam step) and of one forward in
eval() mode under no_grad, both between device events followed by a synchronise, with the smallest and largest time of each; the peak
of torch's allocator above what is allocated before the call (parameters, Adam state, inputs), for one training step; and the largest
difference of the eval-mode forward from the torch variant's, over the largest magnitude.  A variant that cannot allocate is
recorded as "out of memory" instead of a time.  The column sums that give da_src and da_dst (ctgcn_gat_da_f32) are timed alone on
both layers' shapes and put beside the fused step as their share of it.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D, DROPOUT, ALPHA = 128, 0.5, 0.2
LAYERS = {"config_1x500": (1, 500), "paper_8x64": (8, 64)}
REPS = {"uci-like": 20, "enron-like": 10, "synthetic-1m": 3}
SHAPES = {"uci-like": dict(n=1899, snapshots=7, avg_deg=14, max_degree_hint=None),
          "enron-like": dict(n=87000, snapshots=10, avg_deg=13, max_degree_hint=500),
          "synthetic-1m": dict(n=1000000, snapshots=2, avg_deg=16, max_degree_hint=None)}
OOM = "out of memory"


def window(name, dev):
    """(features, GcnAdj list, (rows, cols) list): the sparse identity, and the pattern of A + I of every snapshot"""
    import scipy.sparse as sp
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    graphs = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])
    adjs, pairs = [], []
    for g in graphs:
        m = (g + sp.eye(s["n"])).tocsr()
        m.sort_indices()
        adj = ops.GcnAdj.from_scipy(m, dev)
        adjs.append(adj)
        pairs.append((adj._rows(), adj.col.to(torch.int64)))
    idx = torch.arange(s["n"], device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(s["n"], device=dev), torch.Size((s["n"], s["n"])))
    return [eye for _ in graphs], adjs, pairs


def stock_attention(S, a_src, a_dst, rows, cols, heads, p, training):
    n, d = S.shape
    Sh = S.view(n, heads, d // heads)
    u, v = (Sh * a_src).sum(-1), (Sh * a_dst).sum(-1)
    l = -F.leaky_relu(u[rows] + v[cols], ALPHA)
    m = torch.zeros(n, heads, device=S.device).scatter_reduce(0, rows[:, None].expand(-1, heads), l.detach(), "amax", include_self=False)
    e = torch.exp(l - m[rows])
    Z = torch.zeros(n, heads, device=S.device).index_add(0, rows, e)
    Y = torch.zeros_like(Sh).index_add(0, rows, F.dropout(e, p, training=training)[:, :, None] * Sh[cols])
    return (Y / Z[:, :, None]).reshape(n, d)


def stock_forward(model, pairs):
    """ctgcn_amd.GAT.forward on identity features in stock torch ops, on the module's own parameters"""
    heads = model.attentions
    hid = model.hidden_dim
    W = torch.cat([h.W for h in heads], dim=1)
    a_src = torch.cat([h.a[:, :hid] for h in heads], dim=0)
    a_dst = torch.cat([h.a[:, hid:] for h in heads], dim=0)
    o, out = model.out_att, []
    for rows, cols in pairs:
        h = F.dropout(F.elu(stock_attention(W, a_src, a_dst, rows, cols, len(heads), model.dropout, model.training)), model.dropout,
                      training=model.training)
        y = F.elu(stock_attention(h @ o.W, o.a[:, :D], o.a[:, D:], rows, cols, 1, model.dropout, model.training))
        out.append(F.log_softmax(y, dim=1))
    return out


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def round_robin(fns, reps):
    """(median, [min, max]) per key in ms, or OOM: 3 warm-up calls each, then `reps` rounds in which the variants take turns"""
    alive = dict(fns)
    for k, fn in fns.items():
        try:
            for _ in range(3):
                fn()
        except torch.cuda.OutOfMemoryError:
            del alive[k]
            torch.cuda.empty_cache()
    torch.cuda.synchronize()
    times = {k: [] for k in alive}
    for _ in range(reps):
        for k, fn in alive.items():
            times[k].append(timed(fn))
    med = {k: (float(np.median(times[k])) if k in alive else OOM) for k in fns}
    rng = {k: ([float(min(times[k])), float(max(times[k]))] if k in alive else OOM) for k in fns}
    return med, rng


def peak_above_inputs(fn):
    """bytes torch's allocator holds at the peak of one call above what it holds before it, or OOM"""
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    try:
        fn()
    except torch.cuda.OutOfMemoryError:
        torch.cuda.empty_cache()
        return OOM
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def ratio(a, b):
    return a / b if not isinstance(a, str) and not isinstance(b, str) else None


def bench_shape(name, label, xs, adjs, pairs, dev):
    import copy
    from ctgcn_amd import GAT, ops
    heads, hid = LAYERS[label]
    n, T = adjs[0].n, len(adjs)
    torch.manual_seed(0)
    models = {"fused": GAT(n, hid, D, dropout=DROPOUT, alpha=ALPHA, head_num=heads, learning_type="U-neg").to(dev)}
    models["torch"] = copy.deepcopy(models["fused"])
    gen = torch.Generator(device=dev).manual_seed(1)
    C = [torch.randn(n, D, generator=gen, device=dev) for _ in range(T)]
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def outputs(k):
        return models[k](xs, adjs) if k == "fused" else stock_forward(models[k], pairs)

    def step_of(k):
        def run():
            models[k].train()
            sum((o * c).sum() for o, c in zip(outputs(k), C)).backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def forward_of(k):
        def run():
            models[k].eval()
            with torch.no_grad():
                return outputs(k)
        return run

    for k in models:                                     # Adam's state exists before anything is measured
        try:
            step_of(k)()
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
    models["torch"].load_state_dict(models["fused"].state_dict())
    try:
        a, b = forward_of("fused")(), forward_of("torch")()
        agreement = max(float((x - y).abs().max()) / float(y.abs().max()) for x, y in zip(a, b))
        del a, b
    except torch.cuda.OutOfMemoryError:
        agreement = OOM
        torch.cuda.empty_cache()
    forward_ms, forward_range = round_robin({k: forward_of(k) for k in models}, REPS[name])
    step_ms, step_range = round_robin({k: step_of(k) for k in models}, REPS[name])
    peak = {k: peak_above_inputs(step_of(k)) for k in models}
    # the part of the fused step that da_src and da_dst take: both layers' column sums (ctgcn_gat_da_f32), every snapshot
    S1, S2 = torch.randn(n, heads * hid, device=dev), torch.randn(n, D, device=dev)
    z1, z2 = torch.randn(n, heads, device=dev), torch.randn(n, 1, device=dev)
    da_ms, _ = round_robin({"da": lambda: (ops._gat_da(S1, z1, z1, heads), ops._gat_da(S2, z2, z2, 1))}, REPS[name])
    res = {"heads": heads, "head_width": hid, "embed_dim": D,
           "step_ms": step_ms, "step_ms_min_max": step_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "step_peak_bytes_above_inputs": peak, "eval_forward_max_diff_vs_torch": agreement,
           "step_speedup_fused_vs_torch": ratio(step_ms["torch"], step_ms["fused"]),
           "forward_speedup_fused_vs_torch": ratio(forward_ms["torch"], forward_ms["fused"]),
           "fused_step_da_ms": da_ms["da"] * T, "fused_step_da_share": da_ms["da"] * T / step_ms["fused"]}
    del models, opts
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "gat_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("gat_bench measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    xs, adjs, pairs = window(name, dev)
    res = {"workload": name, "device": torch.cuda.get_device_name(0),
           "shape": dict(SHAPES[name], dropout=DROPOUT, alpha=ALPHA, features="identity", learning_type="U-neg",
                         stored_entries=[a.nnz for a in adjs], longest_row=[int((a.row_ptr[1:] - a.row_ptr[:-1]).max()) for a in adjs]),
           "reps": REPS[name], "warmup": 3, "layers": {}}
    for label in LAYERS:
        res["layers"][label] = bench_shape(name, label, xs, adjs, pairs, dev)
        print(label, json.dumps(res["layers"][label]), flush=True)
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
