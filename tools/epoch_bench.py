"""One epoch of the reference's unsupervised schedule (embedding.py:330-368) on a BASELINE window: the epoch-fused trainer
(ctgcn_amd.embedding, fused=True: one forward, the losses of all batches from ctgcn_epoch.hip, one backward, one Adam step) against the
reference's per-batch loop (a full forward + loss(batch) + backward per batch), timed over 3 batches and extrapolated x ceil(N / bs).

    python tools/epoch_bench.py [--workload synthetic-1m|enron-like] [--loss neg|own] [--batch-size 2048] [--out profiles/epoch_bench.json]

--loss neg: CTGCN-C with the negative-sampling loss (U-neg; pair CSR = the snapshot graph, negative table from the degrees);
--loss own: CTGCN-S with the reconstruction loss (U-own).  The sampling and loss kernels are timed with HIP events per snapshot in a
separate pass over the same embeddings; `loss_bytes_to_move` counts what the loss kernels must read / write at least.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {       # bench.py's shapes (BASELINE configs 5 and 2), one-hot features
    "synthetic-1m": dict(nodes=1_000_000, T=16, edges=8_000_000, max_core=8, hid=128),
    "enron-like": dict(nodes=87_036, T=12, edges=530_284, max_core=5, hid=500),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="synthetic-1m", choices=sorted(WORKLOADS))
    ap.add_argument("--loss", default="neg", choices=["neg", "own"])
    ap.add_argument("--batch-size", type=int, default=2048)
    ap.add_argument("--neg-num", type=int, default=20)
    ap.add_argument("--per-batch", type=int, default=3, help="per-batch-mode batches to time")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    from ctgcn_amd import CTGCN, CoreAdj, NegativeSamplingLoss, ReconstructionLoss
    from ctgcn_amd.embedding import UnsupervisedEmbedding, batch_count
    from ctgcn_amd.metrics import epoch_batch_seed
    from ctgcn_amd.synth import window_graph_device
    from ctgcn_amd.walks import WalkPairs, negative_table

    W = WORKLOADS[args.workload]
    dev = torch.device("cuda:0")
    n, T, bs = W["nodes"], W["T"], args.batch_size
    B = batch_count(n, bs)
    t0 = time.time()
    graphs = window_graph_device(n, W["edges"], T, dev)
    adj_list, pairs, tables = [], [], []
    for t in range(T):
        rp, col, val = graphs[t]
        adj_list.append(CoreAdj.from_graph(rp, col, val, max_core=W["max_core"])[0])
        pairs.append(WalkPairs(rp, col))
        tables.append(torch.from_numpy(negative_table((rp[1:] - rp[:-1]).long())))
    eye = torch.arange(n, device=dev).repeat(2, 1)
    x_list = [torch.sparse_coo_tensor(eye, torch.ones(n, device=dev), (n, n)) for _ in range(T)]
    print("window: %d nodes x %d snapshots, %.1f s" % (n, T, time.time() - t0), file=sys.stderr, flush=True)

    torch.manual_seed(0)
    mt = "C" if args.loss == "neg" else "S"
    with torch.device(dev):
        model = CTGCN(n, W["hid"], 128, 1, 2, T, model_type=mt, trans_activate_type="L" if mt == "C" else "N")
    loss = NegativeSamplingLoss(pairs, tables, neg_num=args.neg_num, Q=10, seed=1) if mt == "C" else ReconstructionLoss()
    base = tempfile.mkdtemp()
    os.makedirs(os.path.join(base, "origin"))
    for t in range(T):
        open(os.path.join(base, "origin", "%02d.csv" % t), "w").close()
    trainer = UnsupervisedEmbedding(base, "origin", "emb", [str(i) for i in range(n)], model, loss, has_cuda=True)

    def sync_time(fn):
        torch.cuda.synchronize()
        t1 = time.time()
        fn()
        torch.cuda.synchronize()
        return time.time() - t1

    # fused epochs: a warm-up, then the timed one
    run = lambda: trainer.learn_embedding(adj_list, x_list, epoch=1, batch_size=bs, model_file=None, export=False, fused=True)
    warm = sync_time(run)
    torch.cuda.reset_peak_memory_stats(dev)
    fused = sync_time(run)
    peak = torch.cuda.max_memory_allocated(dev)
    print("fused epoch: %.3f s (warm-up %.3f s), peak %.1f GB" % (fused, warm, peak / 1e9), file=sys.stderr, flush=True)

    # the sampling and loss kernels on one forward's embeddings, HIP events per snapshot
    model.train()
    res = model(x_list, adj_list)
    out = res if mt == "C" else res[0]
    node_indices = torch.randperm(n).to(dev)
    samp_ms, loss_ms, samples, moved = 0.0, 0.0, 0, 0
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    with torch.no_grad():
        grad = torch.zeros_like(out)
        if mt == "C":
            for t in range(T):
                seeds = [epoch_batch_seed(1, 0, b, t) for b in range(B)]
                ev[0].record()
                total = loss.batched_sample_indices(t, node_indices, bs, seeds)[0]
                ev[1].record()
                loss.epoch_loss(out[t:t + 1], node_indices, bs, [seeds], grad[t:t + 1])     # draws again inside: timed as sampling + loss
                ev[2].record()
                torch.cuda.synchronize()
                s_ms = ev[0].elapsed_time(ev[1])
                samp_ms += s_ms
                loss_ms += ev[1].elapsed_time(ev[2]) - s_ms
                samples += total
                # node kernel: e_u, S_b, e_v per sample; scatter: e_u per sample + dE[v] rmw; dE[u] rmw; gpos, indices
                moved += total * (128 * 4 * 2 + 8 * 4 + 4 * 2) + n * 128 * 4 * 5 + B * 128 * 4 * (args.neg_num + 2)
        else:
            struct = res[1]
            gs = [torch.zeros_like(s) for s in struct]
            ev[0].record()
            loss.epoch_loss(out, struct, node_indices, bs, grad, gs)
            ev[1].record()
            torch.cuda.synchronize()
            loss_ms = ev[0].elapsed_time(ev[1])
            moved = T * n * 128 * 4 * 6          # read s, e; read-modify-write ds, de
    del res, out, grad

    # per-batch mode: the reference's loop over the first --per-batch batches
    perm = torch.randperm(n).to(dev)
    per = []
    for j in range(args.per_batch):
        batch = perm[j * bs:(j + 1) * bs]

        def one():
            r = model(x_list, adj_list)
            if mt == "C":
                l = loss([r, batch], seeds=[epoch_batch_seed(1, 0, j, t) for t in range(T)])
            else:
                l = loss([r[0], r[1], batch])
            l.backward()
        per.append(sync_time(one))
    model.zero_grad()
    per_batch_s = sum(per) / len(per)
    line = {
        "tool": "epoch_bench", "workload": args.workload, "model": "CTGCN-" + mt, "loss": "U-neg" if mt == "C" else "U-own",
        "nodes": n, "snapshots": T, "batch_size": bs, "batches": B, "neg_num": args.neg_num if mt == "C" else None,
        "fused_epoch_s": round(fused, 4), "fused_warmup_epoch_s": round(warm, 4), "fused_peak_GB": round(peak / 1e9, 2),
        "per_batch_s": [round(x, 4) for x in per], "per_batch_epoch_extrapolated_s": round(per_batch_s * B, 2),
        "speedup": round(per_batch_s * B / fused, 1),
        "sampling_ms_per_epoch": round(samp_ms, 3) if mt == "C" else None, "loss_ms_per_epoch": round(loss_ms, 3),
        "samples_per_epoch": samples if mt == "C" else None, "loss_bytes_to_move": moved,
        "loss_GBps": round(moved / (loss_ms * 1e-3) / 1e9, 1) if loss_ms > 0 else None,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(line, fh, indent=1)


if __name__ == "__main__":
    main()
