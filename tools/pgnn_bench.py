"""P-GNN (identity features, feature 32, hidden 32, output 128, 2 layers, dropout 0.5: every reference config's shape) on one snapshot
of three window shapes (tools/gat_bench.py's), two comparisons:

  anchors   one anchor draw, baseline.pgnn.preselect_anchor on a DistHandle (ops.pgnn_anchor_dist, ctgcn_pgnn.hip): int(log2 N)^2 sets
            and the [N, A] distances to them, against the reference's route on the CPU where its dense [N, N] float64 matrix fits
            (uci-like only): networkx all-pairs BFS into the matrix once (`precompute`), then numpy max / argmax over the columns of
            every set per draw (`draw`).  At 87 000 nodes the matrix is 60 GB and at 1 M nodes 8 TB: recorded as "does not fit".
  index     what the layer passes need of a draw beside the distances, built once per draw on first use (ops.PgnnPrepared from the
            distance pass's levels, its transposed pull index and its table lists: two stable torch sorts over the N A items, bincount,
            repeat_interleave), timed alone with its own peak memory.  Both trainers redraw the anchors before every forward, so a
            trainer's step pays draw + index + step; `fused_step_with_draw_and_index_ms` is that sum.
  model     a training step (forward with dropout, surrogate loss sum(out * C), backward, Adam step), a forward, and one layer at
            32 -> 32 alone forward and backward:
              fused   ctgcn_amd.baseline.PGNN as shipped (ops.pgnn_conv)
              torch   the same parameters in the reference's materialising form in stock torch ops on the same GPU: the distance MLP on
                      every scalar of [N, A], the gathered [N, A, in] features, torch.cat to [N, A, 2 in], Linear, ReLU, mean, F.dropout
            with the peak of torch's allocator above what is allocated before the call.  A variant that cannot allocate is recorded
            as "out of memory" instead of a time.  The (dists_max, dists_argmax) pair is pinned, so the timed fused steps find the
            prepared index in ops.pgnn_prepare's cache: the step figures and their peak memory do NOT include the draw or the index
            build, which are the two rows above.

    python tools/pgnn_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out profiles/pgnn_bench_<workload>.json]     (GPU)

The measuring scheme is tools/gat_bench.py's: per variant the median over REPS timed calls (after 3 warm-up calls, the variants taking
turns inside every repetition), between device events followed by a synchronise, with the smallest and largest time of each.
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gat_bench import OOM, REPS, SHAPES, peak_above_inputs, ratio, round_robin  # noqa: E402

FEATURE, HID, OUT, DROPOUT = 32, 32, 128, 0.5
DENSE_LIMIT = 8 << 30            # bytes of the reference's [N, N] float64 matrix that are still built here


def snapshot(name, dev):
    """(edge_index [2, E] on the device, scipy graph) of the window's last snapshot"""
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    g = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])[-1].tocoo()
    keep = g.row < g.col
    return torch.from_numpy(np.vstack((g.row[keep], g.col[keep])).astype(np.int64)).to(dev), g


def reference_route(graph, n, sets):
    """(precompute seconds, draw seconds) of the reference's CPU route, written out: all-pairs BFS into a dense matrix, then slices"""
    import networkx as nx
    t0 = time.time()
    G = nx.Graph()
    G.add_edges_from(zip(graph.row.tolist(), graph.col.tolist()))
    G.add_nodes_from(range(n))
    dense = np.zeros((n, n))
    for u in range(n):
        for v, d in nx.single_source_shortest_path_length(G, u).items():
            dense[u, v] = 1 / (d + 1)
    t1 = time.time()
    for ids in sets:
        cols = dense[:, ids]
        np.max(cols, axis=1), np.argmax(cols, axis=1)
    return t1 - t0, time.time() - t1


def stock_layer(layer, feature, dm, da, p, training):
    d = layer.dist_compute(dm.unsqueeze(-1)).squeeze(-1)
    subset = feature[da.flatten(), :].reshape(da.shape[0], da.shape[1], feature.shape[1])
    messages = torch.cat((subset * d.unsqueeze(-1), feature.unsqueeze(1).repeat(1, da.shape[1], 1)), dim=-1)
    messages = F.relu(layer.linear_hidden(messages))
    return layer.linear_out_position(messages).squeeze(-1), F.dropout(torch.mean(messages, dim=1), p, training=training)


def stock_forward(model, dm, da):
    """ctgcn_amd.PGNN.forward on identity features in the reference's materialising form, on the module's own parameters"""
    x = model.linear_pre.weight.t() + model.linear_pre.bias
    _, x = stock_layer(model.conv_first, x, dm, da, model.dropout, model.training)
    pos, _ = stock_layer(model.conv_out, x, dm, da, 0.0, False)
    return F.normalize(pos, p=2, dim=-1)


def bench_anchors(name, edge_index, graph, dev):
    from ctgcn_amd import ops
    from ctgcn_amd.baseline.pgnn import get_random_anchorset, precompute_dist_data, preselect_anchor
    n = SHAPES[name]["n"]
    t0 = time.time()
    handle = precompute_dist_data(edge_index, n, -1)
    torch.cuda.synchronize()
    handle_s = time.time() - t0
    res = {"handle_seconds": handle_s, "stored_entries": int(handle.col.numel())}
    cut = precompute_dist_data(edge_index, n, 2)
    ms, rng = round_robin({"exact": lambda: preselect_anchor(n, handle, dev), "cutoff2": lambda: preselect_anchor(n, cut, dev)}, REPS[name])
    res.update(draw_ms=ms, draw_ms_min_max=rng)
    dm, da = preselect_anchor(n, handle, dev)
    res.update(anchor_sets=int(dm.shape[1]), unreached_share=float((dm == 0).float().mean()), distinct_values=int(torch.unique(dm).numel()),
               longest_position_list=int(torch.bincount(da.view(-1), minlength=n).max()))
    levels = ops.pgnn_prepare(dm, da).lvl - 1                       # registered by the draw

    def index_build():
        prep = ops.PgnnPrepared(dm, da, n, levels=levels)
        prep.pull()
        prep.table_lists()

    ims, irng = round_robin({"index": index_build}, REPS[name])
    res.update(index_build_ms=ims["index"], index_build_ms_min_max=irng["index"], index_build_peak_bytes=peak_above_inputs(index_build))
    if n * n * 8 <= DENSE_LIMIT:
        sets = [s.cpu().numpy() for s in get_random_anchorset(n, c=1, device=dev)]
        pre, draw = reference_route(graph, n, sets)
        res.update(reference_cpu_precompute_seconds=pre, reference_cpu_draw_ms=draw * 1e3,
                   draw_speedup_vs_reference_cpu=draw * 1e3 / ms["exact"])
    else:
        res.update(reference_cpu="does not fit: the dense [N, N] float64 matrix is %.1f GB" % (n * n * 8 / 1e9))
    return res, dm, da


def bench_model(name, dm, da, dev):
    from ctgcn_amd import PGNN
    from ctgcn_amd.baseline.pgnn import PGNN_layer
    n, A = dm.shape
    idx = torch.arange(n, device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(n, device=dev), torch.Size((n, n)))
    torch.manual_seed(0)
    models = {"fused": PGNN(n, FEATURE, HID, OUT, dropout=DROPOUT).to(dev)}
    models["torch"] = copy.deepcopy(models["fused"])
    gen = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(n, A, generator=gen, device=dev)
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def output(k):
        return models[k](eye, dm, da) if k == "fused" else stock_forward(models[k], dm, da)

    def step_of(k):
        def run():
            models[k].train()
            (output(k) * C).sum().backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def forward_of(k):
        def run():
            models[k].eval()
            with torch.no_grad():
                return output(k)
        return run

    alive = set(models)
    for k in models:                                     # Adam's state exists before anything is measured
        try:
            step_of(k)()
        except torch.cuda.OutOfMemoryError:
            alive.discard(k)
            opts[k].zero_grad(set_to_none=True)
            torch.cuda.empty_cache()
    models["torch"].load_state_dict(models["fused"].state_dict())
    agreement = OOM
    if "torch" in alive:
        try:
            a, b = forward_of("fused")(), forward_of("torch")()
            agreement = float((a - b).abs().max()) / float(b.abs().max())
            del a, b
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
    forward_ms, forward_range = round_robin({k: forward_of(k) for k in models}, REPS[name])
    step_ms, step_range = round_robin({k: step_of(k) for k in models}, REPS[name])
    peak = {k: peak_above_inputs(step_of(k)) for k in models}
    # one layer at 32 -> 32 alone, both outputs, forward and backward
    layer = PGNN_layer(HID, HID).to(dev)
    h = torch.randn(n, HID, generator=gen, device=dev, requires_grad=True)
    cp, cs = torch.randn(n, A, generator=gen, device=dev), torch.randn(n, HID, generator=gen, device=dev)

    def layer_of(k):
        def run():
            pos, st = layer(h, dm, da) if k == "fused" else stock_layer(layer, h, dm, da, 0.0, False)
            ((pos * cp).sum() + (st * cs).sum()).backward()
            layer.zero_grad(set_to_none=True)
            h.grad = None
        return run

    layer_ms, layer_range = round_robin({k: layer_of(k) for k in models}, REPS[name])
    layer_peak = {k: peak_above_inputs(layer_of(k)) for k in models}
    res = {"feature_dim": FEATURE, "hidden_dim": HID, "output_dim": OUT, "anchor_sets": int(A), "dropout": DROPOUT, "features": "identity",
           "one_materialised_tensor_bytes": {"layer1_N_A_2in": int(n) * int(A) * 2 * FEATURE * 4, "layer2_N_A_out": int(n) * int(A) * OUT * 4},
           "step_ms": step_ms, "step_ms_min_max": step_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "step_peak_bytes_above_inputs": peak, "eval_forward_max_diff_vs_torch": agreement,
           "layer_forward_backward_ms": layer_ms, "layer_forward_backward_ms_min_max": layer_range, "layer_peak_bytes_above_inputs": layer_peak,
           "step_speedup_fused_vs_torch": ratio(step_ms["torch"], step_ms["fused"]),
           "forward_speedup_fused_vs_torch": ratio(forward_ms["torch"], forward_ms["fused"]),
           "layer_speedup_fused_vs_torch": ratio(layer_ms["torch"], layer_ms["fused"])}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "pgnn_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("pgnn_bench measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    edge_index, graph = snapshot(name, dev)
    res = {"model": "PGNN", "workload": name, "device": torch.cuda.get_device_name(0), "shape": dict(SHAPES[name], snapshots_measured=1),
           "reps": REPS[name], "warmup": 3}
    res["anchors"], dm, da = bench_anchors(name, edge_index, graph, dev)
    print("anchors", json.dumps(res["anchors"]), flush=True)
    res["model_step"] = bench_model(name, dm, da, dev)
    res["fused_step_with_draw_and_index_ms"] = res["anchors"]["draw_ms"]["exact"] + res["anchors"]["index_build_ms"] + res["model_step"]["step_ms"]["fused"]
    print("model", json.dumps(res["model_step"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
