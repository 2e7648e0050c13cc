"""DynGEM and DynAE (n_units [500, 300], embed_dim 128: the reference's shipped configurations) on two window shapes and two batch
sizes, computed two ways on the same GPU and the same parameters:

  fused   the models as shipped: the first encoder layer as a row-selected gather (ops.rowsel_conv), the weighted reconstruction loss
          from one sweep of the decoder's pre-activation and a correction at the stored entries (ops.wrecon_loss); ctgcn_dyngem.hip
  torch   the trainer's fused=False path: dense adjacency rows and penalty tensors made on the GPU with stock torch ops, the reference's
          N-wide first layer and its dense loss expression

    python tools/dyngem_bench.py --workload {uci-like,synthetic-1m} [--out profiles/dyngem_bench_<workload>.json]     (GPU)

  uci-like       1 899 nodes, average degree 14; DynGEM on 1 snapshot, DynAE on 4 (look_back 3)
  synthetic-1m   1 M nodes, 8 M edges per snapshot (the largest window the other benchmarks draw from ctgcn_amd.synth); DynGEM on 1
                 snapshot, DynAE on 3 (look_back 2)

Per method, batch size (8192 as shipped, and 2048) and variant: the median over REPS timed calls (after 3 warm-up calls, the variants
taking turns inside every repetition; helpers of tools/gat_bench.py) of one training step (a generator's batch, forward, loss,
backward, Adam step) and of one prediction of the embedding (on synthetic-1m: of the first 4 batches of nodes, since the composed
path builds an [8192, 1 M] input per batch), with the smallest and largest time of each, and the peak of torch's allocator above what
is allocated before a training step.  A variant that cannot allocate is recorded as "out of memory" instead of a time."""
import argparse
import copy
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gat_bench import peak_above_inputs, ratio, round_robin  # noqa: E402

UNITS, OUT = [500, 300], 128
BATCHES = (8192, 2048)
REPS = {"uci-like": 20, "synthetic-1m": 3}
SHAPES = {"uci-like": dict(n=1899, avg_deg=14, look_back=3, max_degree_hint=None, predict_batches=None),
          "synthetic-1m": dict(n=1000000, avg_deg=16, look_back=2, max_degree_hint=None, predict_batches=4)}
PARAMS = dict(alpha=1e-5, beta=10.0, nu1=1e-4, nu2=1e-4)


class FirstNodes(object):
    """a predictor over the first `count` nodes only"""

    def __init__(self, predictor, count):
        self.predictor, self.count = predictor, count

    def predict(self, model, rows, **kw):
        full = self.predictor.node_num
        self.predictor.node_num = min(full, self.count)
        try:
            return self.predictor.predict(model, rows, **kw)
        finally:
            self.predictor.node_num = full


def bench(method, rows, batch_size, shape, reps, dev):
    import ctgcn_amd
    from ctgcn_amd import DynamicEmbedding
    n = rows.n
    nodes = list(range(n))
    torch.manual_seed(0)
    if method == "DynGEM":
        model = ctgcn_amd.DynGEM(input_dim=n, output_dim=OUT, n_units=UNITS, bias=True)
        loss_fn = ctgcn_amd.DynGEMLoss(PARAMS["alpha"], PARAMS["beta"], PARAMS["nu1"], PARAMS["nu2"])
        gen = ctgcn_amd.DynGEMBatchGenerator(nodes, batch_size, PARAMS["beta"], shuffle=True, has_cuda=True)
        pred = ctgcn_amd.DynGEMBatchPredictor(nodes, batch_size, has_cuda=True)
        start = 0
    else:
        model = ctgcn_amd.DynAE(input_dim=n, output_dim=OUT, look_back=shape["look_back"], n_units=UNITS, bias=True)
        loss_fn = ctgcn_amd.DynGraph2VecLoss(PARAMS["beta"], PARAMS["nu1"], PARAMS["nu2"])
        gen = ctgcn_amd.BatchGenerator(nodes, batch_size, shape["look_back"], PARAMS["beta"], shuffle=True, has_cuda=True)
        pred = ctgcn_amd.BatchPredictor(nodes, batch_size, has_cuda=True)
        start = rows.T - shape["look_back"]
    if shape["predict_batches"]:
        pred = FirstNodes(pred, shape["predict_batches"] * batch_size)
    models = {"fused": model.to(dev).train()}
    models["torch"] = copy.deepcopy(models["fused"])
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def step_of(k):
        def run():
            res = DynamicEmbedding.get_model_res(models[k], gen.generate(rows), fused=(k == "fused"))
            loss_fn(models[k], res).reshape(()).backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def predict_of(k):
        def run():
            return pred.predict(models[k], rows, need_pred=False, fused=(k == "fused"), start=start)[0]
        return run

    res = {}
    for label, make in (("step", step_of), ("predict", predict_of)):
        ms, rng = round_robin({k: make(k) for k in models}, reps)
        res[label + "_ms"], res[label + "_ms_min_max"] = ms, rng
        res[label + "_speedup_fused_vs_torch"] = ratio(ms["torch"], ms["fused"])
        print(method, batch_size, label, json.dumps(ms), flush=True)
    res["step_peak_bytes_above_inputs"] = {k: peak_above_inputs(step_of(k)) for k in models}
    del models, opts
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "dyngem_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("dyngem_bench measures on the GPU; no device found")
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    dev = torch.device("cuda:0")
    shape, reps = SHAPES[name], REPS[name]
    graphs = dynamic_graph(shape["n"], shape["avg_deg"], shape["look_back"] + 1, seed=3, max_degree_hint=shape["max_degree_hint"])
    windows = {"DynGEM": ops.SnapshotRows(graphs[-1:], dev), "DynAE": ops.SnapshotRows(graphs, dev)}
    res = {"workload": name, "device": torch.cuda.get_device_name(0), "reps": reps, "warmup": 3,
           "shape": dict(shape, n_units=UNITS, embed_dim=OUT, **PARAMS,
                         stored_entries={k: w.nnz for k, w in windows.items()}, longest_row={k: int(w.host_len.max()) for k, w in windows.items()}),
           "results": {}}
    for method in ("DynGEM", "DynAE"):
        for batch_size in BATCHES:
            res["results"]["%s_b%d" % (method, batch_size)] = bench(method, windows[method], batch_size, shape, reps, dev)
            os.makedirs(os.path.dirname(out_path), exist_ok=True)
            with open(out_path, "w") as fh:                          # kept after every leg: a later leg may run out of time
                json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
