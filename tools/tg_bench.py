"""TgGCN, TgGAT, TgSAGE and TgGIN (identity features, feature_dim 500, hidden 500, embedding 128, 2 layers, dropout 0.5: every reference
config's shape) on three window shapes, computed two ways on the same GPU:

  fused   ctgcn_amd.baseline.tg as shipped: ops.TgGraph, ops.gcn_conv, ops.tgat_conv, ops.tg_conv (ctgcn_tg.hip, ctgcn_gat.hip)
  torch   the same parameters in stock torch ops, edge by edge as PyG's message passing runs them: index_select of the source rows,
          index_add_ into the target rows, a scatter softmax for GATConv, F.relu, F.dropout, autograd (tests/_tg_ref.py's formulas)

    python tools/tg_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out-dir profiles]     (GPU)

writes profiles/tg_bench_<workload>.json.  Workloads and the measuring scheme are tools/gat_bench.py's: per variant the median over
REPS timed calls (after 3 warm-up calls, the variants taking turns inside every repetition), between device events followed by a
synchronise, with the smallest and largest time of each.  Quantities per model: `epoch` one training step in train() mode (forward with
dropout, surrogate loss sum(out * C), backward, Adam step); `forward` one eval-mode forward under no_grad; the peak of torch's allocator
above what is allocated before a training step.  Once per workload: the one-off ops.TgGraph build of every snapshot (what the fused
models pay on first sight of an edge index; the stock variant needs none).  A variant that cannot allocate is recorded as "out of
memory" instead of a time.
"""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from gat_bench import OOM, REPS, SHAPES, peak_above_inputs, ratio, round_robin, timed  # noqa: E402

FEAT, HID, D, DROPOUT = 500, 500, 128, 0.5
KINDS = ("TgGCN", "TgGAT", "TgSAGE", "TgGIN")


def window(name, dev):
    """(features, edge lists): the sparse identity and adj._indices() of every snapshot (both directions of an edge, no loops)"""
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    graphs = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])
    edges = []
    for g in graphs:
        coo = g.tocoo()
        edges.append(torch.from_numpy(np.vstack((coo.col, coo.row)).astype(np.int64)).to(dev))
    idx = torch.arange(s["n"], device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(s["n"], device=dev), torch.Size((s["n"], s["n"])))
    return [eye for _ in graphs], edges


def stock_conv(kind, conv, x, ei):
    import _tg_ref as G
    if kind == "TgGCN":
        return G.gcn_conv(x, conv.weight, conv.bias, ei)
    if kind == "TgGAT":
        return G.gat_conv(x, conv.lin_l.weight, conv.att_l, conv.att_r, conv.bias, ei)
    if kind == "TgSAGE":
        return G.sage_conv(x, conv.lin_l.weight, conv.lin_l.bias, conv.lin_r.weight, ei)
    return G.gin_conv(x, conv.nn.weight, conv.nn.bias, conv.eps, ei)


def stock_forward(kind, model, edges):
    """the model's forward on identity features in stock torch ops, on the module's own parameters"""
    out = []
    for ei in edges:
        x = model.linear_pre.weight.t() + model.linear_pre.bias
        for l, conv in enumerate([model.conv_first] + list(model.conv_hidden)):
            x = F.relu(stock_conv(kind, conv, x, ei))
            if l == 0 or kind != "TgGAT":
                x = F.dropout(x, model.dropout, training=model.training)
        out.append(stock_conv(kind, model.conv_out, x, ei))
    return out


def bench(kind, name, xs, edges, graphs, dev):
    import ctgcn_amd
    n, T = graphs[0].n, len(edges)
    torch.manual_seed(0)
    models = {"fused": getattr(ctgcn_amd, kind)(n, FEAT, HID, D, dropout=DROPOUT).to(dev)}
    models["torch"] = copy.deepcopy(models["fused"])
    gen = torch.Generator(device=dev).manual_seed(1)
    C = [torch.randn(n, D, generator=gen, device=dev) for _ in range(T)]
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def outputs(k):
        return models[k](xs, graphs) if k == "fused" else stock_forward(kind, models[k], edges)

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
    reps = REPS[name]
    forward_ms, forward_range = round_robin({k: forward_of(k) for k in models}, reps)
    epoch_ms, epoch_range = round_robin({k: step_of(k) for k in models}, reps)
    peak = {k: peak_above_inputs(step_of(k)) for k in models}
    res = {"epoch_ms": epoch_ms, "epoch_ms_min_max": epoch_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "epoch_peak_bytes_above_inputs": peak, "eval_forward_max_diff_vs_torch": agreement,
           "epoch_speedup_fused_vs_torch": ratio(epoch_ms.get("torch", OOM), epoch_ms.get("fused", OOM)),
           "forward_speedup_fused_vs_torch": ratio(forward_ms.get("torch", OOM), forward_ms.get("fused", OOM))}
    del models, opts
    torch.cuda.empty_cache()
    return res


def graph_build(edges, n, reps):
    """ms to turn every snapshot's edge index into its three operators (sort, count, emit, long-row lists), median of `reps` builds"""
    from ctgcn_amd import ops

    def build():
        return [(g.looped, g.mean, g.sum) for g in (ops.TgGraph(ei, n) for ei in edges)]

    for _ in range(2):
        build()
    times = sorted(timed(build) for _ in range(max(reps, 3)))
    return {"ms": times[len(times) // 2], "ms_min_max": [times[0], times[-1]], "snapshots": len(edges)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    name = args.workload
    if not torch.cuda.is_available():
        raise SystemExit("tg_bench measures on the GPU; no device found")
    from ctgcn_amd import ops
    dev = torch.device("cuda:0")
    xs, edges = window(name, dev)
    n = SHAPES[name]["n"]
    graphs = [ops.TgGraph(ei, n) for ei in edges]
    res = {"workload": name, "device": torch.cuda.get_device_name(0),
           "shape": dict(SHAPES[name], feature_dim=FEAT, hidden_dim=HID, embed_dim=D, layer_num=2, dropout=DROPOUT, features="identity",
                         edges=[int(ei.shape[1]) for ei in edges],
                         longest_row=[int((g.looped.row_ptr[1:] - g.looped.row_ptr[:-1]).max()) for g in graphs]),
           "reps": REPS[name], "warmup": 3, "graph_build": graph_build(edges, n, REPS[name]), "models": {}}
    print("graph build", json.dumps(res["graph_build"]), flush=True)
    os.makedirs(args.out_dir, exist_ok=True)
    for kind in KINDS:
        res["models"][kind] = bench(kind, name, xs, edges, graphs, dev)
        print(kind, json.dumps(res["models"][kind]), flush=True)
        with open(os.path.join(args.out_dir, "tg_bench_%s.json" % name), "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
