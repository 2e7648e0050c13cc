"""VGRNN (identity features, hid 500, embed 128, 1 recurrent layer: every reference config) with VAELoss on two window shapes, computed
two ways on the same GPU and the same parameters:

  fused   ctgcn_amd.baseline.VGRNN as shipped: two gathers a graph-GRU step (ops.ggru_gates, ops.ggru_blend), one for the twin heads
          (ops.vgrnn_heads), the decoder loss without an [N, N] matrix (ops.vae_nll); all in ctgcn_vgrnn.hip
  torch   the same module with fused=False: six sparse products a step, the dense z zᵀ logits, the dense adjacency and the dense BCE

    python tools/vgrnn_bench.py --workload {uci-like,enron-like} [--out profiles/vgrnn_bench_<workload>.json]     (GPU)

  uci-like       1 899 nodes, 7 snapshots, average degree 14
  enron-like     87 000 nodes, 10 snapshots, average degree 13 (largest degree about 500)

Per variant: the median over REPS timed calls (after 3 warm-up calls, the variants taking turns inside every repetition; helpers of
tools/gat_bench.py) of one training step (forward, VAELoss, backward, Adam step), of one forward under no_grad, of one graph-GRU step
alone (forward and backward on snapshot 0) and of the decoder loss alone (forward and backward on snapshot 0's z), with the smallest
and largest time of each, and the peak of torch's allocator above what is allocated before a training step.  A variant that cannot
allocate is recorded as "out of memory" instead of a time."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gat_bench import OOM, peak_above_inputs, ratio, round_robin  # noqa: E402

HID, OUT = 500, 128
REPS = {"uci-like": 20, "enron-like": 5}
SHAPES = {"uci-like": dict(n=1899, snapshots=7, avg_deg=14, max_degree_hint=None),
          "enron-like": dict(n=87000, snapshots=10, avg_deg=13, max_degree_hint=500)}


def window(name, dev):
    """(features, [2, E] index lists, target GcnAdj list): the sparse identity and the snapshots' unit-weight symmetric patterns"""
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    edges, targets = [], []
    for g in dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"]):
        m = g.tocsr()
        m.sort_indices()
        adj = ops.GcnAdj.from_scipy(m, dev)
        targets.append(adj)
        edges.append(torch.stack((adj._rows(), adj.col.to(torch.int64))))
    idx = torch.arange(s["n"], device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(s["n"], device=dev), torch.Size((s["n"], s["n"])))
    return [eye for _ in edges], edges, targets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "vgrnn_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("vgrnn_bench measures on the GPU; no device found")
    from ctgcn_amd import VGRNN, VAELoss, metrics, ops
    from ctgcn_amd.baseline import LazyInnerProduct, gcn_conv_adjacency
    dev = torch.device("cuda:0")
    xs, edges, targets = window(name, dev)
    n, T, reps = targets[0].n, len(targets), REPS[name]
    torch.manual_seed(0)
    models = {"fused": VGRNN(n, HID, OUT, 1, fused=True).to(dev).train()}
    models["torch"] = copy.deepcopy(models["fused"])
    models["torch"].fused = False
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}
    gen = torch.Generator(device=dev).manual_seed(1)
    noise = [torch.randn(n, OUT, generator=gen, device=dev) for _ in range(T)]
    loss_fn = VAELoss()
    prepared = [gcn_conv_adjacency(e, n) for e in edges]           # built once, as in training: the window is constant

    def step_of(k):
        def run():
            _, _, data = models[k](xs, prepared, None, noise)
            loss_fn(data + [targets]).backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def forward_of(k):
        def run():
            with torch.no_grad():
                return models[k](xs, prepared, None, noise)[0]
        return run

    inp = torch.randn(n, 2 * HID, generator=gen, device=dev)
    h0 = torch.randn(1, n, HID, generator=gen, device=dev).requires_grad_(True)

    def cell_of(k):
        def run():
            out, _ = models[k].rnn(inp, prepared[0], h0, fused=(k == "fused"))
            out.sum().backward()
            models[k].zero_grad(set_to_none=True)
            h0.grad = None
        return run

    z = (torch.randn(n, OUT, generator=gen, device=dev) * 0.1).requires_grad_(True)

    def loss_of(k):
        def run():
            dec = LazyInnerProduct(z) if k == "fused" else torch.mm(z, z.t())
            metrics.VAELoss._nll_bernoulli(dec, targets[0]).backward()
            z.grad = None
        return run

    for k in models:                                               # Adam's state exists before anything is measured
        try:
            step_of(k)()
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
    models["torch"].load_state_dict(models["fused"].state_dict())
    res = {"workload": name, "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": 3,
           "shape": dict(SHAPES[name], hidden_dim=HID, embed_dim=OUT, rnn_layer_num=1, features="identity", loss="VAELoss",
                         stored_entries=[a.nnz for a in targets], longest_row=[int((a.row_ptr[1:] - a.row_ptr[:-1]).max()) for a in targets])}
    for label, make in (("forward", forward_of), ("cell_fwd_bwd", cell_of), ("nll_fwd_bwd", loss_of), ("step", step_of)):
        ms, rng = round_robin({k: make(k) for k in models}, reps)
        res[label + "_ms"], res[label + "_ms_min_max"] = ms, rng
        res[label + "_speedup_fused_vs_torch"] = ratio(ms["torch"], ms["fused"])
        print(label, json.dumps(ms), flush=True)
    res["step_peak_bytes_above_inputs"] = {k: peak_above_inputs(step_of(k)) for k in models}
    res["nll_peak_bytes_above_inputs"] = {k: peak_above_inputs(loss_of(k)) for k in models}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
