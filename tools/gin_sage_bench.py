"""GIN and GraphSAGE (identity features, hidden 500, embedding 128, dropout 0.5: every reference config's shape) on three window
shapes, with sum pooling and once with max pooling, computed two ways:

  fused   ctgcn_amd.baseline.GIN / SAGE as shipped: ops.pool_conv, ops.pool_max, ops.batch_norm_act (ctgcn_pool.hip), ops.gcn_conv
  torch   the same parameters in stock torch ops: torch.sparse.mm for sum, a gathered nnz x d tensor with scatter_reduce('amax') for
          max, nn.BatchNorm1d, F.relu, F.normalize, F.dropout, torch.cat, autograd

The reference's own forms (a dense [N, N] mask per SAGE layer, a Python loop over the nodes for max) cannot run at these sizes and are
not measured.

    python tools/gin_sage_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out-dir profiles]     (GPU)

writes profiles/gin_bench_<workload>.json and profiles/sage_bench_<workload>.json.  Workloads and the measuring scheme are
tools/gat_bench.py's: per variant the median over REPS timed calls (after 3 warm-up calls, the variants taking turns inside every
repetition), between device events followed by a synchronise, with the smallest and largest time of each.  Quantities: `epoch` one
training step in train() mode (forward with dropout, surrogate loss sum(out * C), backward, Adam step: what a fused epoch of the
trainer does around its loss); `forward` one eval-mode forward under no_grad; `forward_backward` the training step without Adam;
`layer` one SAGE layer at 500 -> 500 alone, forward and backward (SAGE), or one BatchNorm -> ReLU -> dropout step at N x 500 alone,
forward and backward (GIN); the peak of torch's allocator above what is allocated before a training step.  A variant that cannot
allocate is recorded as "out of memory" instead of a time.
"""
import argparse
import copy
import json
import os
import sys

import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gat_bench import OOM, REPS, SHAPES, peak_above_inputs, ratio, round_robin  # noqa: E402

HID, D, DROPOUT = 500, 128, 0.5


def window(name, dev):
    """(features, GcnAdj list): the sparse identity and the raw adjacency of every snapshot"""
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    graphs = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])
    adjs = []
    for g in graphs:
        m = g.tocsr()
        m.sort_indices()
        adjs.append(ops.GcnAdj.from_scipy(m, dev))
    idx = torch.arange(s["n"], device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(s["n"], device=dev), torch.Size((s["n"], s["n"])))
    return [eye for _ in graphs], adjs


def stock_max(h, rows, cols):
    return torch.zeros_like(h).scatter_reduce(0, rows[:, None].expand(-1, h.shape[1]), h[cols], "amax", include_self=False)


class StockGraph(object):
    """what the stock variant reads of one snapshot: torch sparse matrices for sum, the entry lists for max"""

    def __init__(self, adj):
        from ctgcn_amd import layers
        self.rows, self.cols = adj._rows(), adj.col.to(torch.int64)
        self.gin_sum = layers.as_pool_adj(adj, "sum", self_loop=True).to_sparse_tensor().coalesce()
        self.sage_sum = layers.as_pool_adj(adj, "pattern-sum").to_sparse_tensor().coalesce()


def stock_gin(model, graphs):
    out = []
    for g in graphs:
        h = model.linear.weight.t() + model.linear.bias
        for l in range(model.layer_num):
            pooled = stock_max(h, g.rows, g.cols) if model.neighbor_pooling_type == "max" else torch.sparse.mm(g.gin_sum, h)
            mlp = model.mlps[l]
            for k in range(mlp.layer_num - 1):
                pooled = F.relu(mlp.batch_norms[k](mlp.linears[k](pooled)))
            h = F.relu(model.batch_norms[l](mlp.linears[mlp.layer_num - 1](pooled)))
            if l < model.layer_num - 1:
                h = F.dropout(h, model.dropout, training=model.training)
        out.append(h)
    return out


def stock_sage_layer(layer, h, g):
    neigh = stock_max(h, g.rows, g.cols) if layer.pooling_type == "max" else torch.sparse.mm(g.sage_sum, h)
    return F.normalize(F.relu(layer.linear(torch.cat((h, neigh), dim=1))), p=2)


def stock_sage(model, graphs):
    out = []
    for g in graphs:
        h = stock_sage_layer(model.sage1, model.linear.weight.t() + model.linear.bias, g)
        out.append(stock_sage_layer(model.sage2, F.dropout(h, model.dropout, training=model.training), g))
    return out


def make(kind, n, pooling):
    from ctgcn_amd import GIN, SAGE
    if kind == "gin":
        return GIN(n, HID, D, 2, 2, False, neighbor_pooling_type=pooling, dropout=DROPOUT)
    return SAGE(n, HID, D, None, pooling_type=pooling, gcn=False, dropout=DROPOUT)


def layer_alone(kind, n, adjs, graphs, dev, reps):
    """the step the model is made of, alone, forward and backward: one SAGE layer 500 -> 500, or BatchNorm -> ReLU -> dropout at N x 500"""
    from ctgcn_amd import ops
    from ctgcn_amd.baseline.sage import SAGE_Layer
    x = torch.randn(n, HID, device=dev, requires_grad=True)
    C = torch.randn(n, HID, device=dev)
    if kind == "sage":
        layer = SAGE_Layer(HID, HID, None).to(dev)
        fns = {"fused": lambda: (layer(x, adjs[0], DROPOUT, 7) * C).sum().backward(),
               "torch": lambda: (F.dropout(stock_sage_layer(layer, x, graphs[0]), DROPOUT) * C).sum().backward()}
    else:
        bn = torch.nn.BatchNorm1d(HID).to(dev)
        fns = {"fused": lambda: (ops.batch_norm_act(x, bn.weight, bn.bias, relu=True, p=DROPOUT, key=7)[0] * C).sum().backward(),
               "torch": lambda: (F.dropout(F.relu(bn(x)), DROPOUT) * C).sum().backward()}
    return round_robin(fns, reps)


def bench(kind, name, pooling, xs, adjs, graphs, dev):
    n, T = adjs[0].n, len(adjs)
    torch.manual_seed(0)
    models = {"fused": make(kind, n, pooling).to(dev)}
    models["torch"] = copy.deepcopy(models["fused"])
    stock = stock_gin if kind == "gin" else stock_sage
    gen = torch.Generator(device=dev).manual_seed(1)
    C = [torch.randn(n, D, generator=gen, device=dev) for _ in range(T)]
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def outputs(k):
        return models[k](xs, adjs) if k == "fused" else stock(models[k], graphs)

    def backward_of(k, adam):
        def run():
            models[k].train()
            sum((o * c).sum() for o, c in zip(outputs(k), C)).backward()
            if adam:
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
            backward_of(k, True)()
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
    fb_ms, fb_range = round_robin({k: backward_of(k, False) for k in models}, reps)
    epoch_ms, epoch_range = round_robin({k: backward_of(k, True) for k in models}, reps)
    peak = {k: peak_above_inputs(backward_of(k, True)) for k in models}
    res = {"pooling": pooling, "hidden_dim": HID, "embed_dim": D,
           "epoch_ms": epoch_ms, "epoch_ms_min_max": epoch_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "forward_backward_ms": fb_ms, "forward_backward_ms_min_max": fb_range, "epoch_peak_bytes_above_inputs": peak,
           "eval_forward_max_diff_vs_torch": agreement,
           "epoch_speedup_fused_vs_torch": ratio(epoch_ms["torch"], epoch_ms["fused"]),
           "forward_speedup_fused_vs_torch": ratio(forward_ms["torch"], forward_ms["fused"]),
           "forward_backward_speedup_fused_vs_torch": ratio(fb_ms["torch"], fb_ms["fused"])}
    del models, opts
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles"))
    args = ap.parse_args()
    name = args.workload
    if not torch.cuda.is_available():
        raise SystemExit("gin_sage_bench measures on the GPU; no device found")
    dev = torch.device("cuda:0")
    xs, adjs = window(name, dev)
    graphs = [StockGraph(a) for a in adjs]
    os.makedirs(args.out_dir, exist_ok=True)
    for kind in ("gin", "sage"):
        res = {"model": kind.upper(), "workload": name, "device": torch.cuda.get_device_name(0),
               "shape": dict(SHAPES[name], dropout=DROPOUT, features="identity", stored_entries=[a.nnz for a in adjs],
                             longest_row=[int((a.row_ptr[1:] - a.row_ptr[:-1]).max()) for a in adjs]),
               "reps": REPS[name], "warmup": 3, "poolings": {}}
        for pooling in ("sum", "max"):
            res["poolings"][pooling] = bench(kind, name, pooling, xs, adjs, graphs, dev)
            print(kind, pooling, json.dumps(res["poolings"][pooling]), flush=True)
        ms, rng = layer_alone(kind, adjs[0].n, adjs, graphs, dev, REPS[name])
        what = "sage_layer_500_500" if kind == "sage" else "batch_norm_relu_dropout_500"
        res["layer_alone"] = {"what": what + ", forward and backward, one snapshot", "ms": ms, "ms_min_max": rng,
                              "speedup_fused_vs_torch": ratio(ms["torch"], ms["fused"])}
        print(kind, "layer alone", json.dumps(res["layer_alone"]), flush=True)
        with open(os.path.join(args.out_dir, "%s_bench_%s.json" % (kind, name)), "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
