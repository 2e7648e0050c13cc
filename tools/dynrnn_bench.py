"""DynRNN (n_units [500, 300]) and DynAERNN (ae_units [500, 300], rnn_units [500]), embed_dim 128, look_back 3: the reference's shipped
configurations on a UCI-like window (1 899 nodes, average degree 14, 4 snapshots), computed two ways on the same GPU and the same
parameters:

  fused   the models as shipped: first layers as row-selected gathers (ops.rowsel_conv), every LSTM layer through ops.lstm_layer
          (library fp32 GEMMs and the fused step passes of ctgcn_lstmcell.hip), the loss through ops.wrecon_loss
  torch   the trainer's fused=False path: dense [B, 3, N] adjacency rows and penalty tensors made on the GPU with stock torch ops,
          nn.LSTM (MIOpen) and nn.Linear, the reference's dense loss expression

    python tools/dynrnn_bench.py [--out profiles/dynrnn_bench_uci-like.json]     (GPU)

Per method, batch size (8192 as shipped, and 2048) and variant: the median over REPS timed calls (after 3 warm-up calls, the variants
taking turns inside every repetition; helpers of tools/gat_bench.py) of one training step (a generator's batch, forward, loss,
backward, Adam step) and of one prediction of the embedding, with the smallest and largest time of each, and the peak of torch's
allocator above what is allocated before a training step.

Where the fused step's time goes, from a separate instrumented run of REPS steps (device events around every call; the events cost
host time, so the shares are of the instrumented step, whose time is recorded too): the library GEMMs that ops.lstm_layer issues
(torch.mm / torch.addmm: for DynRNN every GEMM of the step, for DynAERNN all but those of its nn.Linear layers), the two step kernels,
and the project's other kernels (gathers, their backward, the loss)."""
import argparse
import copy
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gat_bench import peak_above_inputs, ratio, round_robin  # noqa: E402

UNITS, RNN_UNITS, OUT = [500, 300], [500], 128
BATCHES = (8192, 2048)
REPS = 20
SHAPE = dict(n=1899, avg_deg=14, look_back=3)
PARAMS = dict(beta=5.0, nu1=1e-4, nu2=1e-4)


class Timed(object):
    """device events around every call of fn while active"""

    def __init__(self, owner, name, sink):
        self.owner, self.name, self.sink, self.fn = owner, name, sink, getattr(owner, name)

    def __enter__(self):
        fn, sink = self.fn, self.sink

        def wrapped(*a, **kw):
            start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            start.record()
            out = fn(*a, **kw)
            end.record()
            sink.append((start, end))
            return out
        setattr(self.owner, self.name, wrapped)
        return self

    def __exit__(self, *exc):
        setattr(self.owner, self.name, self.fn)
        return False


def where_the_time_goes(step, reps):
    """shares of `reps` instrumented fused steps: lstm_layer's GEMMs, the step kernels, the project's other kernels"""
    from ctgcn_amd import ops
    gemm, kernels = [], []
    ops.set_launch_timer(lambda name, start, end, meta: kernels.append((name, start, end)))
    try:
        with Timed(torch, "mm", gemm), Timed(torch, "addmm", gemm):
            step()                                                    # warm with the instrumentation on
            torch.cuda.synchronize()
            del gemm[:], kernels[:]
            first, last = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            first.record()
            for _ in range(reps):
                step()
            last.record()
            torch.cuda.synchronize()
    finally:
        ops.set_launch_timer(None)
    total = first.elapsed_time(last)
    gemm_ms = sum(s.elapsed_time(e) for s, e in gemm)
    cell_ms = sum(s.elapsed_time(e) for n, s, e in kernels if n.startswith("lstm_cell"))
    other_ms = sum(s.elapsed_time(e) for n, s, e in kernels if not n.startswith("lstm_cell"))
    return {"instrumented_step_ms": total / reps, "gemm_calls_per_step": len(gemm) / reps,
            "cell_launches_per_step": sum(1 for n, _, _ in kernels if n.startswith("lstm_cell")) / reps,
            "share_lstm_layer_gemms": gemm_ms / total, "share_lstm_cell_kernels": cell_ms / total, "share_other_project_kernels": other_ms / total,
            "share_rest": 1.0 - (gemm_ms + cell_ms + other_ms) / total}


def bench(method, rows, batch_size, dev):
    import ctgcn_amd
    from ctgcn_amd import DynamicEmbedding
    n, look_back = rows.n, SHAPE["look_back"]
    nodes = list(range(n))
    torch.manual_seed(0)
    if method == "DynRNN":
        model = ctgcn_amd.DynRNN(input_dim=n, output_dim=OUT, look_back=look_back, n_units=UNITS, bias=True)
    else:
        model = ctgcn_amd.DynAERNN(input_dim=n, output_dim=OUT, look_back=look_back, ae_units=UNITS, rnn_units=RNN_UNITS, bias=True)
    loss_fn = ctgcn_amd.DynGraph2VecLoss(PARAMS["beta"], PARAMS["nu1"], PARAMS["nu2"])
    gen = ctgcn_amd.BatchGenerator(nodes, batch_size, look_back, PARAMS["beta"], shuffle=True, has_cuda=True)
    pred = ctgcn_amd.BatchPredictor(nodes, batch_size, has_cuda=True)
    start = rows.T - look_back
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
        ms, rng = round_robin({k: make(k) for k in models}, REPS)
        res[label + "_ms"], res[label + "_ms_min_max"] = ms, rng
        res[label + "_speedup_fused_vs_torch"] = ratio(ms["torch"], ms["fused"])
        print(method, batch_size, label, json.dumps(ms), flush=True)
    res["step_peak_bytes_above_inputs"] = {k: peak_above_inputs(step_of(k)) for k in models}
    res["fused_step_breakdown"] = where_the_time_goes(step_of("fused"), REPS)
    print(method, batch_size, "breakdown", json.dumps(res["fused_step_breakdown"]), flush=True)
    del models, opts
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dynrnn_bench_uci-like.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dynrnn_bench measures on the GPU; no device found")
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    dev = torch.device("cuda:0")
    graphs = dynamic_graph(SHAPE["n"], SHAPE["avg_deg"], SHAPE["look_back"] + 1, seed=3, max_degree_hint=None)
    rows = ops.SnapshotRows(graphs, dev)
    res = {"workload": "uci-like", "device": torch.cuda.get_device_name(0), "reps": REPS, "warmup": 3,
           "shape": dict(SHAPE, snapshots=rows.T, n_units=UNITS, ae_units=UNITS, rnn_units=RNN_UNITS, embed_dim=OUT, stored_entries=rows.nnz,
                         longest_row=int(np.max(rows.host_len)), **PARAMS),
           "results": {}}
    for method in ("DynRNN", "DynAERNN"):
        for batch_size in BATCHES:
            res["results"]["%s_b%d" % (method, batch_size)] = bench(method, rows, batch_size, dev)
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "w") as fh:                          # kept after every leg: a later leg may run out of time
                json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
