#!/usr/bin/env python3
"""The core-axis and the temporal RNN at embedding widths other than 128: layers.rnn_reduce_norm on the cell route (library GEMMs plus
the fused passes of ctgcn_grucell.hip / ctgcn_lstmcell.hip; ops.gru_layer, ops.lstm_layer) against the route the parent commit took,
norm(layers.rnn_over_rows(...)) through the PyTorch-ROCm modules (MIOpen), which CTGCN_RNN_CELL=0 still selects.

One run: per shape both routes are warmed up, then timed alternately, forward (no grad) and forward + backward, each repetition between
device synchronisations; medians are reported with the smallest and largest repetition.  A second pass with ops.set_launch_timer
installed sums the device time of the cell kernels and of the layer's library GEMMs (HIP events around each launch) and gives their
shares of that pass's device time.  The last entry is one CTGCN-C window at embed_dim 64 on the UCI-like workload (1 899 nodes, 7
snapshots, average degree 14), end to end, the module route selected by the environment switch.

    python tools/gru_width_bench.py [--out profiles/gru_width_bench.json] [--only NAME ...]     (GPU)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ctgcn_amd import layers, ops  # noqa: E402

# name: (rnn, rows, steps, d_in, hidden, reduce_sum, repetitions of the cell route, of the module route)
SHAPES = {
    "core 1M x 8 x 64": ("GRU", 1_000_000, 8, 64, 64, True, 5, 3),
    "core 1M x 8 x 256": ("GRU", 1_000_000, 8, 256, 256, True, 5, 3),
    "core enron-like 87000 x 5 x 64": ("GRU", 87_000, 5, 64, 64, True, 11, 5),
    "core enron-like 87000 x 5 x 256": ("GRU", 87_000, 5, 256, 256, True, 11, 5),
    "core uci-like 1899 x 8 x 64": ("GRU", 1_899, 8, 64, 64, True, 31, 31),
    "core uci-like 1899 x 8 x 256": ("GRU", 1_899, 8, 256, 256, True, 31, 31),
    "temporal 87000 x 10 x 64": ("GRU", 87_000, 10, 64, 64, False, 11, 5),
    "temporal 87000 x 10 x 256": ("GRU", 87_000, 10, 256, 256, False, 11, 5),
    "core LSTM 87000 x 5 x 64": ("LSTM", 87_000, 5, 64, 64, True, 11, 5),
}
CELL_NAMES = ("gru_cell_fwd", "gru_cell_bwd", "lstm_cell_fwd", "lstm_cell_bwd")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(samples):
    return {"median_ms": round(statistics.median(samples), 4), "min_ms": round(min(samples), 4), "max_ms": round(max(samples), 4),
            "repetitions": len(samples)}


def alternate(routes, reps):
    """routes: {name: fn}; every route warmed up twice, then timed in turn reps[name] times"""
    for fn in routes.values():
        fn()
        fn()
    samples = {k: [] for k in routes}
    for i in range(max(reps.values())):
        for k, fn in routes.items():
            if i < reps[k]:
                samples[k].append(timed(fn))
    return {k: summary(v) for k, v in samples.items()}


def shares(fn):
    """device time of one call, and of its cell kernels and layer GEMMs, from HIP events (a pass of its own: the events cost host time)"""
    seen = []
    ops.set_launch_timer(lambda name, start, end, meta: seen.append((name, start, end)))
    try:
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        end.record()
        torch.cuda.synchronize()
    finally:
        ops.set_launch_timer(None)
    total = start.elapsed_time(end)
    cell = sum(s.elapsed_time(e) for name, s, e in seen if name in CELL_NAMES)
    gemm = sum(s.elapsed_time(e) for name, s, e in seen if name == "gru_layer_gemm")
    res = {"device_ms": round(total, 4), "cell_kernels_ms": round(cell, 4), "cell_kernels_share": round(cell / total, 4),
           "cell_launches": sum(name in CELL_NAMES for name, _, _ in seen)}
    if gemm:
        res.update(library_gemms_ms=round(gemm, 4), library_gemms_share=round(gemm / total, 4))
    else:
        res["library_gemms_share"] = "not measured (ops.lstm_layer's GEMMs carry no timer)"
    return res


def layer_shape(name, dev):
    kind, rows, steps, d_in, hid, reduce_sum, reps_cell, reps_mod = SHAPES[name]
    torch.manual_seed(0)
    rnn = getattr(torch.nn, kind)(d_in, hid, 1, batch_first=True).to(dev)
    norm = torch.nn.LayerNorm(hid).to(dev)
    x = torch.relu(torch.randn(rows, steps, d_in, device=dev)).requires_grad_(True)
    assert ops.rnn_cell_ok(rnn, x)

    def cell_fwd():
        with torch.no_grad():
            return layers.rnn_reduce_norm(rnn, norm, x, reduce_sum)

    def mod_fwd():
        with torch.no_grad():
            return norm(layers.rnn_over_rows(rnn, x, reduce_sum))

    def train(route):
        def step():
            x.grad = None
            rnn.zero_grad(set_to_none=True)
            norm.zero_grad(set_to_none=True)
            out = layers.rnn_reduce_norm(rnn, norm, x, reduce_sum) if route == "cell" else norm(layers.rnn_over_rows(rnn, x, reduce_sum))
            out.square().mean().backward()
        return step

    reps = {"cell": reps_cell, "modules": reps_mod}
    res = {"rnn": kind, "rows": rows, "steps": steps, "d_in": d_in, "hidden": hid, "reduce_sum": reduce_sum,
           "forward": alternate({"cell": cell_fwd, "modules": mod_fwd}, reps),
           "forward_backward": alternate({"cell": train("cell"), "modules": train("modules")}, reps),
           "cell_route_shares": {"forward": shares(cell_fwd), "forward_backward": shares(train("cell"))}}
    with torch.no_grad():
        a, b = cell_fwd(), mod_fwd()
        res["max_abs_difference_of_the_forwards"] = float((a - b).abs().max())
        res["max_abs_output"] = float(b.abs().max())
    for part in ("forward", "forward_backward"):
        res[part]["modules_over_cell"] = round(res[part]["modules"]["median_ms"] / res[part]["cell"]["median_ms"], 3)
    return res


def window(dev):
    """one CTGCN-C window at embed_dim 64 on the UCI-like workload, inference and a training step, both routes"""
    import ctgcn_amd
    from ctgcn_amd.helper import core_adj_from_scipy
    from ctgcn_amd.synth import dynamic_graph
    n, T, max_core = 1899, 7, 8
    adj = [core_adj_from_scipy(g, max_core, dev)[0] for g in dynamic_graph(n, 14, T, seed=1)]
    torch.manual_seed(0)
    model = ctgcn_amd.CTGCN(n, 500, 64, 1, 2, T).to(dev)
    idx = torch.arange(n, device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(n, device=dev), (n, n)).coalesce()
    x = [eye] * T
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def route(value, fn):
        def run():
            os.environ["CTGCN_RNN_CELL"] = value
            try:
                return fn()
            finally:
                os.environ.pop("CTGCN_RNN_CELL", None)
        return run

    def infer():
        with torch.no_grad():
            return model(x, adj)

    def step():
        opt.zero_grad(set_to_none=True)
        model(x, adj).square().mean().backward()

    reps = {"cell": 21, "modules": 21}
    res = {"workload": "uci-like", "nodes": n, "snapshots": T, "core_matrices": [a.K for a in adj], "embed_dim": 64, "hidden_dim": 500,
           "forward": alternate({"cell": route("1", infer), "modules": route("0", infer)}, reps),
           "forward_backward": alternate({"cell": route("1", step), "modules": route("0", step)}, reps),
           "cell_route_shares": {"forward": shares(infer), "forward_backward": shares(step)}}
    for part in ("forward", "forward_backward"):
        res[part]["modules_over_cell"] = round(res[part]["modules"]["median_ms"] / res[part]["cell"]["median_ms"], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_width_bench.json"))
    ap.add_argument("--only", nargs="*", help="names of the shapes to run ('window' for the CTGCN-C window); default: all")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_width_bench needs the GPU: a timing taken elsewhere says nothing about it")
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "method": "one process; per shape both routes warmed up twice, then timed alternately between device synchronisations "
                     "(host clock); medians; shares from HIP events around each launch in a pass of their own",
           "routes": {"cell": "layers.rnn_reduce_norm: ops.gru_layer / ops.lstm_layer (library fp32 GEMMs + fused HIP cell passes), torch LayerNorm",
                      "modules": "norm(layers.rnn_over_rows(...)): nn.GRU / nn.LSTM through PyTorch-ROCm (MIOpen) in row chunks; CTGCN_RNN_CELL=0"},
           "shapes": {}}
    for name in SHAPES:
        if a.only is None or name in a.only:
            res["shapes"][name] = layer_shape(name, dev)
            print(name, json.dumps({k: res["shapes"][name][k] for k in ("forward", "forward_backward")}), flush=True)
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(a.out), exist_ok=True)
            with open(a.out, "w") as fp:                             # kept after every shape: a later shape's failure loses nothing
                json.dump(res, fp, indent=1)
    if a.only is None or "window" in a.only:
        res["ctgcn_c_window_embed_dim_64"] = window(dev)
        print("window", json.dumps({k: res["ctgcn_c_window_embed_dim_64"][k] for k in ("forward", "forward_backward")}), flush=True)
    res["cell_route_slower_at"] = sorted(
        "%s (%s)" % (name, part) for name, r in list(res["shapes"].items()) + [("CTGCN-C window", res.get("ctgcn_c_window_embed_dim_64"))]
        if r for part in ("forward", "forward_backward") if r[part]["modules_over_cell"] < 1.0)
    with open(a.out, "w") as fp:
        json.dump(res, fp, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
