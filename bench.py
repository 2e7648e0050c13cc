#!/usr/bin/env python3
"""bench.py — CTGCN hot-path benchmark on MI355X (driver contract: ONE JSON line on rank 0's stdout).

step     = one embedding (forward) pass of CTGCN over the whole T-snapshot window: per-snapshot MLP -> CoreDiffusion
           layers (HIP nested-k-core aggregation + core-axis GRU + LayerNorm) -> exchange -> temporal GRU + LayerNorm.
           Graphs, features and weights are resident in HBM before the timed region.
metric   = aggregated edges/s over the window = sum_t sum_layers sum_k nnz(A(t,k)) / step time        (BASELINE.json)
workload = default `synthetic-1m` = BASELINE config 5 (1M nodes x 16 cumulative snapshots, avg-deg 16, max_core capped at 8,
           hid = embed = 128): fits one GPU; with --gpus N the SAME window is sharded snapshot-parallel over
           N ranks (strong scaling).  --workload picks the other BASELINE configs' shapes (enron-like = config 2,
           facebook-like = config 3 (CTGCN-S), math-like / as-like = config 4); their lines are committed under profiles/.

`python bench.py --gpus N` with N > 1 and no launcher environment re-launches itself under torch.distributed.run
(one process per GPU, RCCL, 127.0.0.1 rendezvous); under a launcher (RANK/WORLD_SIZE set) it runs as that rank.

Output.  stdout carries ONE compact JSON line, < 4 KB (bench.MAX_LINE_BYTES; the driver keeps ~9 KB of stdout — round 5's
23 KB line reached it truncated and unparsed): the contract's keys, `config` {workload, name, nodes, snapshots, max_core,
aggregated_edges_per_step, parallelism}, `roofline`, `cpu_baseline`, `also` (one-number summaries of the legs) and `detail_file`.

A plain run does only what the headline needs: set-up, what has always come before the timed steps (one second of device copies, whose
rate goes into `also`, and the pre-warm, --prewarm-s), the W warm-up and N timed steps, --dump-outputs and the line; on windows of
<= 200 000 nodes also the same forward replayed from one hipGraph, since the headline is the faster of the two.  Its `roofline`,
`cpu_baseline` and `detail_file` are null, and it writes no detail file unless --detail-file names one.
--full adds every other leg below, fills those fields and writes the FULL record (--detail-file; by default bench_detail.json, per workload
bench_detail_<name>.json, in the output folder of the repository root).  The timed steps are the same with and without --full.
  roofline            dominant kernel (the aggregation): algorithmic bytes per launch / HIP-event duration on the launch stream; under the
                      row plan the algorithmic bytes are those of the rows actually written, frac_8d keeps SURVEY §8d's formula;
                      `traffic` = HBM bytes per launch measured BY THIS RUN: two `rocprofv3 --pmc` passes (FETCH_SIZE, WRITE_SIZE apart, the
                      gfx950 x2 correction of MI355X_MICROARCH.md) over a 2-step run of this script (pmc_traffic; --no-pmc: null)
  cpu_baseline        the reference's torch.sparse.mm loop on the host cores (uncoalesced COO as the reference builds it + a coalesced-CSR
                      variant), a bounded sample (--cpu-budget-s, default 100 s: the median of three passes of the full 8-matrix loop of
                      the largest snapshot where they fit, one pass each otherwise), rank 0, N=1 only
  (detail file only)  roofline_by_width, roofline_gru (matrix-core kernels), roofline_kcore, exact_fp32 (CTGCN_FP32_MFMA_ONLY=1),
                      training_step (+ backward rooflines, the reference-loss training batch), hbm_copy_GBps_measured, configs (BASELINE
                      configs 2-4: short --full runs of this script, with their own baselines), hipgraph (small windows: the same forward
                      replayed from one hipGraph, frozen and live weights), pmc, torch_rocm_baseline (the reference's own GPU path, stock
                      PyTorch-ROCm) and forced_dist (the forced single-rank RCCL leg)
A plain run of config 5 spends ~10 s outside its steps on an MI355X box (the graphs, the copy pass, the pre-warm); --full several minutes.

--dump-outputs DIR writes what the last timed step returned (dump_outputs): graphs, features and weights are seeded, so two builds run
with the same arguments can be compared output for output.
"""
import argparse
import copy
import json
import os
import socket
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md); ~6300 GB/s is the measured copy ceiling

WORKLOADS = {
    "synthetic-1m": dict(nodes=1_000_000, T=16, edges=8_000_000, cumulative=True, max_core=8, hid=128, emb=128, model="C", trans=1,
                         diff=2, act="L", features="one-hot",
                         desc="BASELINE config 5: synthetic 1M nodes x 16 cumulative snapshots, avg-deg 16"),
    "enron-like": dict(nodes=87_036, T=12, edges=530_284, cumulative=True, max_core=5, hid=500, emb=128, model="C", trans=1, diff=2,
                       act="L", features="one-hot",
                       desc="BASELINE config 2 shape: Enron statistics (87 036 nodes, 530 284 edges), 12-snapshot window, max_core 5 "
                            "(synthetic stand-in, the dataset is not available offline)"),
    "facebook-like": dict(nodes=60_730, T=27, edges=607_487, cumulative=True, max_core=-1, hid=500, emb=128, model="S", trans=3, diff=1,
                          act="N", features="gaussian-degree",
                          desc="BASELINE config 3 shape: Facebook statistics (60 730 nodes, 607 487 edges), full 27-snapshot window, "
                               "CTGCN-S (3 transform layers, 1 diffusion layer at d=128, gaussian degree features; synthetic stand-in)"),
    "math-like": dict(nodes=24_740, T=8, edges=323_357, cumulative=True, max_core=-1, hid=500, emb=128, model="C", trans=1, diff=2, act="L",
                      features="one-hot",
                      desc="BASELINE config 4 shape (math): 24 740 nodes, 323 357 edges, 8-snapshot window (synthetic stand-in)"),
    "as-like": dict(nodes=6_828, T=8, edges=19_500, cumulative=False, max_core=-1, hid=500, emb=128, model="C", trans=1, diff=2, act="L",
                    features="one-hot",
                    desc="BASELINE config 4 shape (AS): 6 828 nodes, ~19.5k edges per snapshot, NON-cumulative 8-snapshot window "
                         "(synthetic stand-in)"),
    "tiny": dict(nodes=20_000, T=4, edges=80_000, cumulative=True, max_core=4, hid=64, emb=64, model="C", trans=1, diff=2, act="L",
                 features="one-hot", desc="debug"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--workload", default="synthetic-1m", choices=sorted(WORKLOADS))
    ap.add_argument("--exchange", default="all_to_all", choices=["all_to_all", "all_gather"])
    ap.add_argument("--train", action="store_true",
                    help="time forward + backward + Adam step (surrogate loss out.square().mean(); the reference's "
                         "negative-sampling loss is outside the hot path) instead of the embedding forward")
    ap.add_argument("--graph", action="store_true",
                    help="replay the window from one captured hipGraph (ctgcn_amd.graph_capture; single GPU, inference): "
                         "removes launch/Python overhead on small graphs; per-launch HIP-event timing (roofline) is off")
    ap.add_argument("--dry", action="store_true",
                    help="launcher / rendezvous / per-rank bookkeeping only, on the CPU with the gloo backend and no kernels (the `not gpu` test of "
                         "the multi-rank path of this script: self-launch, assignment, stats gather, barriers, max-over-ranks timing, one JSON line)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the host-core baseline and the stock-PyTorch-on-this-GPU baseline")
    ap.add_argument("--train-leg", action="store_true", help="run the training-step leg even with --no-extras (the per-config runs of --full)")
    ap.add_argument("--no-extras", action="store_true", help="skip the exact-fp32 forward and the k-core roofline legs")
    ap.add_argument("--cpu-budget-s", type=float, default=100.0,
                    help="seconds of host time for the CPU baseline (SURVEY 8d: a bounded sample; three passes of each operand format where "
                         "they fit; config 5: one pass of the full 8-matrix loop as COO + one as CSR)")
    ap.add_argument("--full", action="store_true",
                    help="every leg besides the headline: rooflines and kernel times, exact-fp32 forward, k-core, "
                         "training step, CPU and stock-PyTorch baselines, PMC traffic, BASELINE configs 2-4, forced single-rank RCCL leg, and the "
                         "detail file (minutes; a plain run keeps to set-up, warm-up, the timed steps and the line).  --no-cpu-baseline, "
                         "--train-leg, --no-extras, --cpu-budget-s and --no-pmc shape these legs")
    ap.add_argument("--no-pmc", action="store_true",
                    help="do not measure roofline.traffic (two `rocprofv3 --pmc` passes of a 2-step run of this script, FETCH_SIZE and WRITE_SIZE apart)")
    ap.add_argument("--prewarm-s", type=float, default=1.0, help="seconds of untimed stepping before the warm-up steps (clocks)")
    ap.add_argument("--detail-file", default=None,
                    help="where the full record goes (--full: by default bench_detail.json, per workload bench_detail_<name>.json, in the output "
                         "folder of the repository root; a plain run writes it only when named here); stdout carries ONE compact JSON line (< 4 KB)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/<name>.npy (float32; at most 64 MB in all: "
                         "beyond that a fixed seeded sample of node rows, listed in DIR/<name>__index.npy)")
    a = ap.parse_args()
    if a.steps < 1 or a.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    return a


def algorithmic_bytes(n, nnz, K, d):
    """SURVEY.md §8d, fused nested kernel: one pass over the largest matrix (4d B gathered row + 4 B col + 4 B val
    + 1 B slot per entry), K output rows of 4d B per node, row_ptr."""
    return nnz * (4 * d + 9) + n * K * 4 * d + 4 * (n + 1)


def moved_bytes(n, nnz, K, d, rows_written):
    """Bytes the aggregation launch has to move under the graph's row plan (ctgcn_amd.core_adj.CoreAdj.row_plan): the §8d entry
    stream, but only `rows_written` of the n*K output rows (4d B of fp16 planes + 4 B scale each), plus row_ptr, the row order and
    the tile masks."""
    return nnz * (4 * d + 9) + rows_written * (4 * d + 4) + 4 * (n + 1) + 4 * n + 4 * ((n + 15) // 16)


def measure_copy_bandwidth(dev, seconds=1.0):
    """Device-to-device copy of a 1 GiB buffer for about `seconds`: (bytes read + bytes written) / time in GB/s — SURVEY §8d asks for
    the measured copy bandwidth of the bench box next to the 8 TB/s spec figure."""
    import torch
    a = torch.empty(1 << 28, dtype=torch.float32, device=dev).normal_()
    b = torch.empty_like(a)
    for _ in range(3):
        b.copy_(a)
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    reps, best = 0, 0.0
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        s.record()
        for _ in range(10):
            b.copy_(a)
        e.record()
        e.synchronize()
        best = max(best, 10 * 2.0 * a.numel() * 4 / (s.elapsed_time(e) * 1e-3) / 1e9)
        reps += 10
    del a, b
    return {"value": round(best, 1), "unit": "GB/s", "what": "torch copy_ of 1 GiB fp32 device->device, read + written bytes / HIP-event time, best "
            "10-copy batch of %d copies" % reps, "spec_peak": HBM_PEAK_GBS}


def kcore_bytes(n, nnz):
    """SURVEY.md §8d k-core minimum traffic: one read of the CSR for the degrees, one for the decrements, core array r/w."""
    return 2 * (4 * (n + 1) + 4 * nnz) + 8 * n


def agg_kernel_name(d, split=False):
    chunks = (d + 3) // 4
    if split:
        kern = "agg_fwd_split32_kernel" if chunks <= 32 else "agg_fwd_split_kernel<64,%d,4>" % (-(-chunks // 64))
        return ("%s (CoreDiffusion fused nested-core SpMM, d=%d, one pass; rows leave as fp16 operand planes + row scales for the %s, "
                "4d B per row like the fp32 rows they replace)" % (kern, d, "GRU layer kernel" if d == 128 else "split GEMM"))
    lpr = 8
    while lpr < 64 and lpr < chunks:
        lpr <<= 1
    return "agg_fwd_kernel<4,%d,4> (CoreDiffusion fused nested-core SpMM, d=%d%s)" % (lpr, d, ", %d passes" % (-(-chunks // lpr)) if chunks > lpr else "")


def self_launch(args):
    """--gpus N > 1 without a launcher: re-run this script under torch.distributed.run, one rank per GPU."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    args = parse()
    if os.environ.get("CTGCN_BENCH_WATCHDOG"):      # debugging aid: dump every thread's Python stack and exit after N seconds
        import faulthandler
        faulthandler.dump_traceback_later(float(os.environ["CTGCN_BENCH_WATCHDOG"]), exit=True)
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    if args.dry:
        return dry_run(args)
    import torch
    import torch.distributed as dist
    # stdout carries exactly ONE JSON line: anything libraries print on fd 1 meanwhile (RCCL's version banner ...)
    # is routed to stderr until the result is ready.
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    assert torch.cuda.is_available(), "bench.py needs an MI355X"
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # CTGCN_FORCE_DIST=1 runs the RCCL/sharded code path even with one rank (1-GPU boxes can exercise it)
    force_dist = os.environ.get("CTGCN_FORCE_DIST") == "1"
    use_dist = world > 1 or force_dist
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=dev)

    from ctgcn_amd import CTGCN, CoreAdj, ops, _lib
    from ctgcn_amd import snapshot_parallel as spp
    from ctgcn_amd.synth import window_graph_device, prefix_sizes, DEFAULT_SEED
    _lib.load()

    W = WORKLOADS[args.workload]
    n, T, hid, emb = W["nodes"], W["T"], W["hid"], W["emb"]
    log = (lambda *a: print(*a, file=sys.stderr, flush=True)) if rank == 0 else (lambda *a: None)

    # ---------------------------------------------------------------- plan + graphs (owned snapshots only)
    sizes = prefix_sizes(W["edges"], T) if W["cumulative"] else [W["edges"]] * T
    assignment = spp.plan_assignment(sizes, world)
    mine = assignment[rank]
    t0 = time.time()
    need = sorted(set(mine) | ({0} if W["max_core"] == -1 else set()))    # sticky max_core: snapshot 0's file count caps the window
    graphs = window_graph_device(n, W["edges"], T, dev, seed=DEFAULT_SEED, cumulative=W["cumulative"], which=need)
    log("generated %d/%d snapshots in %.1fs" % (len(mine), T, time.time() - t0))
    t0 = time.time()
    max_core = W["max_core"]
    if max_core == -1:      # helper.py:61-62: -1 becomes the FIRST snapshot's k-core file count and stays that
        _, max_core = ops.kcore(graphs[0][0], graphs[0][1])
    adj_list, local_stats, degrees = [None] * T, {}, {}
    for t in mine:
        rp, col, val = graphs[t]
        adj, core, files = CoreAdj.from_graph(rp, col, val, max_core=max_core)
        adj_list[t] = adj
        local_stats[t] = dict(K=adj.K, nnz=adj.nnz, agg=adj.aggregated_edges, max_core=files)
        if W["features"] == "gaussian-degree":
            degrees[t] = (rp[1:] - rp[:-1]).to(torch.float32)          # unit weights: weighted degree = neighbour count
    torch.cuda.synchronize()
    log("k-core + slot tagging of %d snapshots in %.2fs (max_core %d)" % (len(mine), time.time() - t0, max_core))
    kc_t = max(mine, key=lambda t: local_stats[t]["nnz"]) if mine else None
    kc_graph = graphs[kc_t][:2] if kc_t is not None else None
    del graphs

    # every rank needs the window totals (metric numerator)
    if use_dist:
        gathered = [None] * world
        dist.all_gather_object(gathered, local_stats)
        stats = {}
        for g in gathered:
            stats.update(g)
    else:
        stats = local_stats
    layers = W["diff"]
    agg_edges_step = layers * sum(stats[t]["agg"] for t in range(T))

    # ------------------------------------------------------------------------------- features + model
    x_list = [None] * T
    if W["features"] == "one-hot":           # sparse identity (reference helper.py:161-172)
        input_dim = n
        eye_idx = torch.arange(n, device=dev).repeat(2, 1)
        for t in mine:
            x_list[t] = torch.sparse_coo_tensor(eye_idx, torch.ones(n, device=dev), (n, n))
    else:                                    # Normal(degree, 1e-4) rows of width max-degree + 1 (reference helper.py:128-135)
        md = torch.tensor([max([int(d.max().item()) for d in degrees.values()] + [0])], device=dev)
        if use_dist:
            dist.all_reduce(md, op=dist.ReduceOp.MAX)
        input_dim = int(md.item()) + 1
        gen = torch.Generator(device=dev)
        for t in mine:
            gen.manual_seed(DEFAULT_SEED + t)
            # built once, fed to every forward (reference train.py:72-76): declared static, as ctgcn_amd.helper.DataLoader does for its outputs
            x_list[t] = ops.mark_static(torch.randn(n, input_dim, generator=gen, device=dev).mul_(1e-4).add_(degrees[t].unsqueeze(1)))
    torch.manual_seed(0)
    with torch.device(dev):
        model = CTGCN(input_dim, hid, emb, W["trans"], layers, T, rnn_type="GRU", model_type=W["model"], trans_activate_type=W["act"])
    model.eval()
    if use_dist:
        spp.shard_ctgcn(model, n, assignment=assignment, exchange=args.exchange, gather_output=False)
        model.shard_timing = []            # HIP events at the phase boundaries of every sharded forward (spp.shard_phase_ms)

    # HIP-event timing of every aggregation launch (same stream the kernel is launched on)
    launches = []
    if args.graph:
        if use_dist or args.train:
            raise SystemExit("--graph: single-GPU inference only")
        from ctgcn_amd.graph_capture import GraphedInference
        runner = GraphedInference(model, x_list, adj_list)
    else:
        ops.set_launch_timer(lambda name, start, end, meta: launches.append((name, start, end, meta)))

    if args.train:
        model.train()
        params = list(spp.owned_parameters(model)) if use_dist else list(model.parameters())
        opt = torch.optim.Adam(params, lr=1e-3)

    def first(res):
        return res[0] if isinstance(res, tuple) else res     # 'S' models also return the transform outputs

    def eager_step():
        """What a caller of the timed path receives: the embeddings, and for 'S' models (embeddings, transform outputs)."""
        if args.graph:
            return runner()
        if not args.train:
            with torch.no_grad():
                return model(x_list, adj_list)
        opt.zero_grad(set_to_none=True)
        res = model(x_list, adj_list)
        first(res).square().mean().backward()
        if use_dist:
            spp.allreduce_replicated_grads(model)
        opt.step()
        if torch.is_tensor(res):
            return res.detach()
        return res[0].detach(), [None if t is None else t.detach() for t in res[1]]

    def fence():
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()

    prewarm = {"steps": 0}

    def timed(steps, warmup, prewarm_s=0.0, step=None):
        step = step or eager_step
        # untimed, before the W warm-up steps: keep stepping until the device has been busy for prewarm_s seconds — a fresh box
        # starts at idle clocks and a 20 ms window measured 29 vs 21.5 ms depending on what ran before it (the number of steps
        # this took is on the JSON line as `prewarm_steps`); same count on every rank (decided by rank 0)
        if prewarm_s > 0:
            # training: the clock decides how many Adam steps the pre-warm takes, so the weights and optimizer state are put back
            # afterwards — the timed steps then start from the same state in every run (--dump-outputs compares runs)
            saved = copy.deepcopy((model.state_dict(), opt.state_dict())) if args.train else None
            t0 = time.perf_counter()
            while True:
                step()
                torch.cuda.synchronize()
                prewarm["steps"] += 1
                go = torch.tensor([1.0 if time.perf_counter() - t0 < prewarm_s else 0.0], device=dev)
                if use_dist:
                    dist.broadcast(go, src=0)
                if float(go.item()) == 0.0 or prewarm["steps"] >= 200:
                    break
            if saved is not None:
                model.load_state_dict(saved[0])
                opt.load_state_dict(saved[1])
                del saved
        for _ in range(warmup):
            step()
        fence()
        launches.clear()
        t_start = time.perf_counter()
        for _ in range(steps):
            res = step()
        fence()
        elapsed = time.perf_counter() - t_start
        if use_dist:
            tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            elapsed = float(tt.item())
        return 1000.0 * elapsed / steps, res

    # in every run, --full or not: the timed steps have always followed this second of copies, and without it config 5 measured ~1 % faster
    # on the same box (149.8 against 151.4 ms, two runs each), so it stays part of what comes before them
    copy_bw = measure_copy_bandwidth(dev) if rank == 0 else None
    ms_per_step, res = timed(args.steps, args.warmup, prewarm_s=args.prewarm_s)
    out = first(res)
    assert torch.isfinite(out).all()
    if args.dump_outputs:
        arrays = {"embeddings": out}
        if not torch.is_tensor(res):
            arrays.update(("transform_t%02d" % t, tr) for t, tr in enumerate(res[1]) if tr is not None)
        if world > 1:
            arrays = {"%s_rank%d" % (k, rank): v for k, v in arrays.items()}
        dump_outputs(args.dump_outputs, arrays, DUMP_BYTES // world, log)
    del res
    per_rank_ms = None
    if use_dist and args.full:
        # DESIGN §5's model, line by line: every rank's compute / exposed exchange / temporal head over the timed steps
        mine_ms = spp.shard_phase_ms(model, last=args.steps) or {}
        mine_ms.update(rank=rank, snapshots=mine, aggregated_edges=layers * sum(stats[t]["agg"] for t in mine))
        per_rank_ms = [None] * world
        dist.all_gather_object(per_rank_ms, mine_ms)
        model.shard_timing = None
    # the launch timer (and model.shard_timing) stay on in the timed steps of every run, so that they are the same steps with and without
    # --full; a plain run reads none of those events: the roofline objects below stay empty
    recorded = list(launches) if args.full else []
    roof_steps = args.steps
    roof_pass = "the timed steps"
    if args.full and not use_dist and not args.train and not args.graph and n <= 200_000 and os.environ.get("CTGCN_STREAMS", "") != "1":
        # small graphs run their snapshot branches on several streams: kernels overlap, and an event pair around one launch then
        # also times its neighbours.  Per-kernel durations for the roofline objects come from a separate single-stream pass.
        os.environ["CTGCN_STREAMS"] = "1"
        try:
            roof_steps = 2
            out1 = first(timed(roof_steps, 1)[1])
            assert torch.equal(out1, out)                 # same kernels, same inputs
            recorded = list(launches)
            roof_pass = "a separate single-stream pass (CTGCN_STREAMS=1, %d steps) after the timed multi-stream steps" % roof_steps
        finally:
            del os.environ["CTGCN_STREAMS"]

    # ------------------------------------------------------------------------- roofline of the dominant kernel
    ops.set_launch_timer(None)
    # small windows (launch-bound: a forward is a few dozen launches of 5 - 200 us): the SAME forward replayed from one hipGraph is the
    # headline, the eager time stays next to it (ctgcn_amd.graph_capture — the grouped launches are capturable since ABI 28)
    eager_ms, graph_info = None, None
    if n <= 200_000 and not use_dist and not args.train and not args.graph and os.environ.get("CTGCN_BENCH_GRAPH", "1") != "0":
        try:
            from ctgcn_amd.graph_capture import GraphedInference
            t0 = time.time()
            g_runner = GraphedInference(model, x_list, adj_list, frozen_weights=True)
            cap_s = time.time() - t0
            g_ms, g_out = timed(args.steps, args.warmup, step=lambda: first(g_runner()))
            assert torch.equal(g_out, out), "hipGraph replay differs from the eager forward"
            graph_info = {"replay_ms_per_step": round(g_ms, 4), "eager_ms_per_step": round(ms_per_step, 4), "capture_s": round(cap_s, 2),
                          "bit_identical_to_eager": True, "mode": "frozen_weights=True: cached operand forms of the weights recorded; re-capture after an update"}
            del g_runner, g_out
            if args.full:
                g_runner = GraphedInference(model, x_list, adj_list)
                g2_ms, g_out = timed(args.steps, args.warmup, step=lambda: first(g_runner()))
                assert torch.equal(g_out, out), "hipGraph replay differs from the eager forward"
                graph_info["replay_ms_per_step_live_weights"] = round(g2_ms, 4)
                del g_runner, g_out
            # headline = the faster of the two ways to run the SAME forward (same kernels, same bits); both are on the record
            if g_ms < ms_per_step:
                eager_ms, ms_per_step = ms_per_step, g_ms
        except Exception as exc:
            graph_info = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
            log("hipGraph replay leg failed: %s" % graph_info["error"])
    fwd = [(s.elapsed_time(e), meta) for name, s, e, meta in recorded if name == "agg_fwd"]
    pmc_file = os.path.join(ROOT, "profiles", "pmc_traffic.json")
    pmc = {}
    if os.path.exists(pmc_file):
        try:
            pmc = json.load(open(pmc_file))
        except Exception:
            pmc = {}

    def roofline_of(group, d):
        avg_ms = sum(ms for ms, _ in group) / len(group)
        # SURVEY §8d prices the fused kernel at nnz (4d + 9) + N K 4d + 4 (N + 1) bytes: every (node, core) output row.  Under the row
        # plan (CoreAdj.row_plan) the rows that repeat the row before them are not written, so the bytes a launch HAS to move are fewer;
        # `achieved` / `frac` use those (a fraction of the HBM peak must be physical), `survey_8d_*` keep the §8d formula (the work the
        # reference defines — it can exceed the peak precisely because part of it is no longer done).  Without a plan both coincide.
        # a grouped launch (ops.core_diffusion_split_group: all snapshots of a small window in one grid) carries the sums over its snapshots:
        # nnz and rows_written are window totals, K_sum = sum of the snapshots' K, group = their number
        def survey_of(m):
            g = m.get("group", 1)
            return m["nnz"] * (4 * m["d"] + 9) + m["n"] * m.get("K_sum", m["K"]) * 4 * m["d"] + g * 4 * (m["n"] + 1)

        def moved_of(m):
            g, ks = m.get("group", 1), m.get("K_sum", m["K"])
            if m.get("rows_written", m["n"] * ks) == m["n"] * ks:
                return survey_of(m)
            return m["nnz"] * (4 * m["d"] + 9) + m["rows_written"] * (4 * m["d"] + 4) + g * (4 * (m["n"] + 1) + 4 * m["n"] + 4 * ((m["n"] + 15) // 16))
        survey = sum(survey_of(m) for _, m in group) / len(group)
        moved = sum(moved_of(m) for _, m in group) / len(group)
        rows_frac = sum(m.get("rows_written", m["n"] * m.get("K_sum", m["K"])) for _, m in group) / float(sum(m["n"] * m.get("K_sum", m["K"]) for _, m in group))
        achieved = moved / (avg_ms * 1e-3) / 1e9
        survey_gbps = survey / (avg_ms * 1e-3) / 1e9
        rec = pmc.get(args.workload, {}).get(str(world)) if d == 128 else None
        copy_peak = copy_bw["value"] if copy_bw else 6300.0
        m0 = group[0][1]
        x_bytes = m0["n"] * m0["d"] * 4                  # the gathered operand (per snapshot): <= 256 MB lives in the Infinity Cache / L2
        cached = x_bytes <= (256 << 20)
        written = sum(m.get("rows_written", m["n"] * m.get("K_sum", m["K"])) * (4 * m["d"] + 4) for _, m in group) / len(group)
        out = {"kernel": agg_kernel_name(d, bool(m0.get("split"))),
               "bound": "cache" if cached else "hbm",
               "bound_note": ("the gathered X of a snapshot is %.0f MB: it is served by L2 / the 256 MB Infinity Cache, not by HBM - `achieved` is a "
                              "rate of bytes moved on-die and may exceed what HBM can deliver; the HBM side of this launch is what it WRITES "
                              "(`hbm_written_GBps`)" % (x_bytes / 1e6)) if cached else
                             ("X of a snapshot is %.0f MB; on the power-law snapshots L2 / Infinity Cache still serve the hub rows: the cache-hostile "
                              "bracket of this kernel (uniform graph, X = 2 GB) is `frac_dram_bracket`" % (x_bytes / 1e6)),
               "achieved": round(achieved, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
               "frac": round(achieved / HBM_PEAK_GBS, 4),
               # the three ways to price this launch
               "frac_8d": round(survey_gbps / HBM_PEAK_GBS, 4),
               "frac_moved": round(achieved / HBM_PEAK_GBS, 4),
               "frac_note": "frac_8d: SURVEY 8d's bytes (every (node, core) output row) / time - can exceed 1 because the row plan does not write the "
                            "rows that repeat the row before them; frac_moved (= frac): the bytes this launch has to move / time.  (The DRAM-bound "
                            "bracket of this kernel - hub-free uniform graph, X = 2 GB - was measured once in round 4: 5.88 TB/s = 0.735, "
                            "profiles/r04_agg_dram_bracket.txt; not re-measured by this run, so not a field)",
               "hbm_written_GBps": round(written / (avg_ms * 1e-3) / 1e9, 1),
               # measured by THIS run (pmc_traffic below fills it in) or null; an earlier round's figure is kept apart, with its provenance
               "traffic": None,
               "traffic_earlier_profile": {"hbm_bytes_per_launch": rec["hbm_bytes_per_launch"], "round": rec.get("round"),
                                           "source": rec.get("source", "profiles/pmc_traffic.json")} if rec else None,
               "launches_timed": len(group), "avg_launch_ms": round(avg_ms, 4), "algorithmic_bytes_per_launch": int(moved),
               "snapshots_per_launch": m0.get("group", 1),
               "ms_per_step_rank0": round(sum(ms for ms, _ in group) / roof_steps, 3),
               "output_rows_written_frac": round(rows_frac, 4),
               "survey_8d_bytes_per_launch": int(survey), "survey_8d_GBps": round(survey_gbps, 1), "survey_8d_frac": round(survey_gbps / HBM_PEAK_GBS, 4),
               "bytes_note": "algorithmic bytes = entries x (4d + 9) + output rows WRITTEN x (4d + 4) + row_ptr + the plan's order / tile masks; "
                             "survey_8d_* = SURVEY 8d's formula, which prices every (node, core) output row",
               "frac_of_measured_copy_bw": round(achieved / copy_peak, 4)}
        return out

    by_width = {}
    for ms, m in fwd:
        by_width.setdefault(m["d"], []).append((ms, m))
    roofs = {d: roofline_of(g, d) for d, g in by_width.items()}
    roof = None
    if roofs:
        roof = roofs[max(roofs, key=lambda d: roofs[d]["ms_per_step_rank0"])]      # dominant = most time per step
    kern_ms = [ms for ms, _ in fwd]
    spmm_ms_step = sum(kern_ms) / roof_steps if kern_ms else None
    # the matrix-core kernels: GRU recurrence (+ sum/LayerNorm) and the input projection
    gru = [(s.elapsed_time(e), meta) for name, s, e, meta in recorded if name == "gru_seq"]
    proj = [(s.elapsed_time(e), meta) for name, s, e, meta in recorded if name == "gru_proj"]
    fused = [(s.elapsed_time(e), meta) for name, s, e, meta in recorded if name == "gru_layer"]
    roof_mfma = None
    mode = ops.forward_split_mode()
    peak = {2: 2500.0 / 3.0, 1: 2500.0 / 6.0, 0: 157.3}[mode]
    if gru:
        # fp32-equivalent flops; step 0 (h = 0) issues no MFMA.  The matrix-core bound is the dense 16-bit peak divided by
        # the number of 16-bit products per fp32 product (fp16x2: 3, bf16x3: 6), or the fp32 MFMA peak for the exact path.
        name = {2: "gru_seq_h2_kernel (GRU recurrence + sum + LayerNorm; fp32 operands scaled per row and split into two fp16 "
                   "terms, 3 x v_mfma_f32_16x16x32_f16 per product, fp32 accumulate)",
                1: "gru_seq_x3_kernel (GRU recurrence + sum + LayerNorm; fp32 operands split 3-way into bf16, "
                   "6 x v_mfma_f32_16x16x32_bf16 per product, fp32 accumulate)",
                0: "gru_seq_kernel (GRU recurrence + sum + LayerNorm, v_mfma_f32_16x16x4_f32)"}[mode]
        pname = {2: "gru_proj_h2_kernel", 1: "gru_proj_x3_kernel", 0: "hipBLASLt fp32 GEMM"}[mode]
        # (a grouped launch — the first layer of a small window's snapshots in one grid — carries row_steps = sum of rows x steps, group = T)
        grs = lambda m: m.get("row_steps", m["rows"] * m["steps"])
        flops = sum((grs(m) - m["rows"] * m.get("group", 1)) * 2.0 * 128 * 384 for _, m in gru)
        gi_bytes = sum(grs(m) * 1536.0 for _, m in gru)    # the projection's output read back, 1536 B per row-step
        ms = sum(t for t, _ in gru)
        roof_mfma = {"kernel": name,
                     "bound": "mfma", "achieved": round(flops / (ms * 1e-3) / 1e12, 2), "peak": round(peak, 1),
                     "unit": "TFLOP/s (fp32-equivalent)", "frac": round(flops / (ms * 1e-3) / 1e12 / peak, 4),
                     "gi_read_GBps": round(gi_bytes / (ms * 1e-3) / 1e9, 1),
                     "launches_timed": len(gru), "ms_per_step_rank0": round(ms / roof_steps, 3)}
        if proj:
            pms = sum(t for t, _ in proj)
            pbytes = sum(m["rows"] * 2048.0 for _, m in proj)          # 512 B read + 1536 B written per row
            roof_mfma["input_projection"] = {"kernel": pname, "bound": "hbm", "ms_per_step_rank0": round(pms / roof_steps, 3),
                                             "achieved": round(pbytes / (pms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                             "frac": round(pbytes / (pms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    if fused:
        # projection + recurrence in one kernel: 2*128*384 flops per row-step for the projection, the same for every step but the first
        def layer_obj(group, name, per_step):
            # grouped launches (a window's snapshots in one grid) carry row_steps = sum over the snapshots of rows x steps and group = their number
            rsteps = lambda m: m.get("row_steps", m["rows"] * m["steps"])
            ref_flops = sum((2 * rsteps(m) - m["rows"] * m.get("group", 1)) * 2.0 * 128 * 384 for _, m in group)
            # executed: x·W_ih only for the row-steps that bring a new x (row plan), h·W_hh for every step but the first
            flops = sum((m.get("new_rows", rsteps(m)) + rsteps(m) - m["rows"] * m.get("group", 1)) * 2.0 * 128 * 384 for _, m in group)
            ms = sum(t for t, _ in group)
            # compulsory traffic: the x rows in (as fp32 or as two fp16 planes: 512 B per row-step either way), one output row out
            # (per step for the temporal form)
            hbm = sum(m.get("new_rows", rsteps(m)) * 512.0 + m["rows"] * m.get("group", 1) * (m["steps"] * 512.0 if per_step else 512.0) for _, m in group)
            return {"kernel": name, "bound": "mfma", "achieved": round(flops / (ms * 1e-3) / 1e12, 2), "peak": round(peak, 1),
                    "unit": "TFLOP/s (fp32-equivalent)", "frac": round(flops / (ms * 1e-3) / 1e12 / peak, 4),
                    # tools/probes/mfma_peak_probe.hip: v_mfma_f32_16x16x32_f16 sustains 2.15-2.3 PFLOP/s with real operands on this
                    # chip (clock 2.0-2.1 GHz under load), not the 2.5 of the data sheet
                    "frac_of_sustained_mfma_rate_2200": round(flops / (ms * 1e-3) / 1e12 / (2200.0 / 3.0), 4),
                    "reference_flops_TFLOPs": round(ref_flops / (ms * 1e-3) / 1e12, 2), "executed_over_reference_flops": round(flops / ref_flops, 4),
                    "flops_note": "`achieved` counts the products the kernel executes (matrix-core utilisation); `reference_flops_TFLOPs` the "
                                  "products of the reference's GRU on the same input (repeated x rows multiplied again)",
                    "compulsory_hbm_GBps": round(hbm / (ms * 1e-3) / 1e9, 1), "launches_timed": len(group),
                    "ms_per_step_rank0": round(ms / roof_steps, 3)}
        red = [(t, m) for t, m in fused if m.get("reduce_sum", True)]
        seqf = [(t, m) for t, m in fused if not m.get("reduce_sum", True)]
        fr = None
        if red:
            pres = any(m.get("presplit") for _, m in red)
            fr = layer_obj(red, "gru_layer8_h2_kernel (CoreDiffusion GRU: input projection + recurrence + sum over cores + LayerNorm in one "
                                "kernel, both weight matrices resident on the CU — registers + 120 KB of LDS, 8 waves — the projection "
                                "consumed from the MFMA accumulators; fp16x2 split%s)"
                                % ("; x arrives as fp16 planes + row scales written by the aggregation kernel" if pres else ""), False)
        if seqf:
            tl = layer_obj(seqf, "gru_layer8_h2_kernel<per step> (temporal GRU: the same kernel emitting LayerNorm(h_t) of every step through an "
                                 "fp32 staging buffer in LDS)", True)
            if fr is None:
                fr = tl
            else:
                fr["temporal_layer"] = tl
        if roof_mfma is None:
            roof_mfma = fr
        else:
            roof_mfma["fused_layers"] = fr

    # ------------------------------------------------------------------------- extras: exact fp32 forward, k-core peel
    exact = None
    roof_kcore = None
    if args.full and not args.no_extras and not args.train and not args.graph:
        prev = os.environ.get("CTGCN_FP32_MFMA_ONLY")
        os.environ["CTGCN_FP32_MFMA_ONLY"] = "1"
        try:
            ms_exact, out_exact = timed(max(2, min(3, args.steps)), 1)
            out_exact = first(out_exact)
        finally:
            if prev is None:
                del os.environ["CTGCN_FP32_MFMA_ONLY"]
            else:
                os.environ["CTGCN_FP32_MFMA_ONLY"] = prev
        diff = float((out_exact - out).abs().max().item())
        exact = {"ms_per_step": round(ms_exact, 3), "mode": "CTGCN_FP32_MFMA_ONLY=1: hipBLASLt fp32 GEMM projection + v_mfma_f32_16x16x4_f32 "
                 "recurrence (no 16-bit operand split)", "max_abs_diff_vs_default": diff,
                 "note": "the default line's GRU products use the fp16x2 split (22 mantissa bits per operand, fp32 accumulate)"}
        if kc_graph is not None and rank == 0:
            rp, col = kc_graph
            res = {}
            for label, cap in (("exact", -1), ("capped", max_core)):
                ops.kcore(rp, col, level_cap=cap)
                times = []
                for _ in range(5):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    _, mk = ops.kcore(rp, col, level_cap=cap)
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b))
                res[label] = (statistics.median(times), mk)
            nb = kcore_bytes(n, int(col.numel()))
            ms_k = res["exact"][0]
            roof_kcore = {"kernel": "exact core numbers: kcore_hindex_kernel + kcore_hindex_hub_kernel x ~40 sweeps (local h-index iteration, round 5; "
                                    "CTGCN_KCORE=peel: one kcore_level_kernel per level, 7.3 ms here); capped at the loader's max_core: the "
                                    "level-synchronous peel (<= 16 levels).  Integer, bit-exact either way", "bound": "hbm",
                          "achieved": round(nb / (ms_k * 1e-3) / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                          "frac": round(nb / (ms_k * 1e-3) / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                          "algorithmic_bytes": nb, "peel_ms_exact": round(ms_k, 3), "max_core": int(res["exact"][1]),
                          "peel_ms_capped_at_max_core_%d" % max_core: round(res["capped"][0], 3),
                          "snapshot": kc_t, "stored_entries": int(col.numel()),
                          "note": "includes the host read-backs of the convergence counters (every 8 sweeps / 16 levels); bound by the number of dependent "
                                  "sweeps x (launch + a pass over the active vertices), not by bandwidth: profiles/r05_kcore_hindex.txt"}
    # ------------------------------------------------------------------------- the reference's own GPU path on THIS GPU (baseline only)
    torch_rocm = None
    if world == 1 and not use_dist and args.full and not args.no_cpu_baseline and not args.train and not args.graph:
        try:
            torch_rocm = torch_rocm_baseline(model, x_list, adj_list, W, ms_per_step, first, log)
        except Exception as exc:
            torch_rocm = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
            log("torch-ROCm baseline failed: %s" % torch_rocm["error"])
        torch.cuda.empty_cache()
    # ------------------------------------------------------------------------- training step (fwd AND fwd+bwd)
    train = None
    if args.full and (not args.no_extras or args.train_leg) and not args.train and not args.graph and not use_dist and \
            os.environ.get("CTGCN_BENCH_TRAIN_LEG", "1") != "0":
        try:
            train = training_leg(model, x_list, adj_list, ops, first, agg_edges_step, log)
        except Exception as exc:          # e.g. out of memory on a box that is not empty: the forward line above must still be printed
            train = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:400])}
            log("training leg failed: %s" % train["error"])
            torch.cuda.empty_cache()
    if use_dist:
        dist.barrier()
    if rank != 0:
        dist.destroy_process_group()
        return

    # ------------------------------------------------------------------------------------- CPU baselines (N=1)
    cpu = cpu_k = None
    if world == 1 and args.full and not args.no_cpu_baseline:
        widths = [hid if W["model"] == "C" else emb] + [emb] * (layers - 1)
        cpu = cpu_baseline(adj_list, widths, args.cpu_budget_s, log)
        cpu_k = cpu_baseline_kcore(kc_graph, n, log) if kc_graph is not None else None

    agg_rate = None if not spmm_ms_step else layers * sum(stats[t]["agg"] for t in mine) / (spmm_ms_step * 1e-3)
    line = {
        "metric": "aggregated edges/s over T-snapshot window (CTGCN-%s %s)" % (W["model"], "training step: forward + backward + Adam" if args.train else "embedding forward"),
        "value": agg_edges_step / (ms_per_step * 1e-3),
        "unit": "edges/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "prewarm_steps": prewarm["steps"],
        "ms_per_step": round(ms_per_step, 3),
        "higher_is_better": True,
        "scaling": "strong",
        "vs_baseline": None,
        "dtype": "f32 (fp16x2-split MFMA operands)",
        "dtype_note": "fp32 storage and accumulation everywhere; the dense GRU / Linear products run as fp32-accurate two-term fp16 splits on the "
                      "matrix cores (22 mantissa bits per operand, 3 MFMAs per product, fp32 accumulate; error vs fp64 asserted <= a plain fp32 "
                      "GEMM's in tests/), and in inference the aggregation hands its rows over in that split form. `exact_fp32` times the same "
                      "forward without any 16-bit operand",
        "operand_plane_cache": "the fp16 operand planes of the dense layers' WEIGHTS and of the model's INPUT feature tensors (x_list: built once by the "
                               "caller and fed to every forward, reference train.py:72-76) are split once per tensor version and kept "
                               "(ctgcn_amd.ops._PlaneCache; CTGCN_PLANE_CACHE=0 splits them on every call: facebook-like 26.7 -> 30.4 ms, the other configs "
                               "within noise, profiles/r04_mlp_chain_ab.txt); intermediate activations are split on every call",
        "parity_rule": "SURVEY 8c's rtol 1e-4 / atol 1e-5 holds at UCI size; at the BASELINE config sizes the fp32 CPU path itself misses it on 2e-6 .. 6e-5 of the "
                       "entries, so tests/test_gpu_configs.py evaluates the oracle in float64 too (on a node sample of 4 112 - 8 320 rows; the fp32 oracle on every row) and holds the HIP path to <= 1.25 x the fp32 CPU path's fraction of "
                       "entries outside that tolerance, <= 1.5 x its worst error and <= 5e-4 absolute (T = 16 depth: 2.0 x the fraction); gradients at 1 M rows: 1e-4 "
                       "of each tensor's largest entry vs float64 autograd.  Observed: profiles/r05_parity_errors.json",
        "hbm_copy_GBps_measured": copy_bw,
        "data": "synthetic (seed %d power-law dynamic graph, random-init weights)" % DEFAULT_SEED,
        "config": {"workload": "%s; CTGCN-%s hid=%d embed=%d, %d transform + %d diffusion layers, max_core=%d, %s features" % (
                       W["desc"], W["model"], hid, emb, W["trans"], layers, max_core, W["features"]),
                   "name": args.workload, "nodes": n, "snapshots": T, "edges_last_snapshot": sizes[-1], "max_core": max_core,
                   "input_dim": input_dim,
                   "K_per_snapshot": [stats[t]["K"] for t in range(T)],
                   "stored_entries_per_snapshot": [stats[t]["nnz"] for t in range(T)],
                   "aggregated_edges_per_step": agg_edges_step,
                   "parallelism": "snapshot-parallel x%d (%s exchange before the temporal GRU)" % (world, args.exchange) if world > 1 else ("single GPU, hipGraph replay" if (args.graph or eager_ms is not None) else "single GPU"),
                   "assignment": assignment},
        "value_definition": "headline `value` = aggregated edges / WHOLE forward wall-clock (embed_wall_ms; conservative: includes the dense "
                            "GRU/Linear/LayerNorm time); `aggregation_edges_per_s_rank0` = the same edges / time inside the aggregation "
                            "kernels only (SURVEY §8d(i))",
        "embed_wall_ms": round(ms_per_step, 3),
        "eager_ms_per_step": None if eager_ms is None else round(eager_ms, 4),
        "hipgraph": graph_info,
        "aggregation_ms_per_step_rank0": None if spmm_ms_step is None else round(spmm_ms_step, 3),
        "aggregation_edges_per_s_rank0": agg_rate,
        "per_rank_ms": per_rank_ms,
        "kernel_timing_pass": roof_pass,
        "kernel_ms_per_step_rank0": {k: round(sum(st.elapsed_time(en) for nm, st, en, _ in recorded if nm == k) / roof_steps, 3)
                                     for k in sorted({nm for nm, _, _, _ in recorded})},
        "roofline_note": "`roofline` is the aggregation kernel — the HBM-bound kernel the metric is named after (BASELINE north_star); by time "
                         "the largest kernel of the config-5 forward is the matrix-core-bound GRU (`roofline_gru.fused_layers`), see "
                         "`kernel_ms_per_step_rank0`",
        "roofline": roof,
        "roofline_by_width": {str(d): r for d, r in sorted(roofs.items())} if len(roofs) > 1 else None,
        "roofline_gru": roof_mfma,
        "roofline_kcore": roof_kcore,
        "exact_fp32": exact,
        "training_step": train,
        "cpu_baseline": cpu,
        "torch_rocm_baseline": torch_rocm,
        "cpu_baseline_kcore": cpu_k,
    }
    line["forced_dist"] = None
    line["exact_fp32_ms_per_step"] = exact["ms_per_step"] if exact else None
    line["training_step_ms_per_step"] = train.get("ms_per_step") if train else None
    # roofline.traffic measured by THIS run: two rocprofv3 --pmc passes (FETCH_SIZE, WRITE_SIZE apart) over a 2-step run of this very script
    headline = args.workload == "synthetic-1m" and world == 1 and not use_dist and not args.train and not args.graph
    line["pmc"] = None
    del model, x_list, adj_list, out
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    if world == 1 and args.full and not use_dist and not args.no_pmc and not args.train and not args.graph and roof is not None:
        line["pmc"] = pmc_traffic(args, roof, log)
        if line["pmc"].get("hbm_bytes_per_launch") is not None:
            roof["traffic"] = line["pmc"]["hbm_bytes_per_launch"]
            roof["traffic_over_algorithmic_bytes"] = round(roof["traffic"] / float(roof["algorithmic_bytes_per_launch"]), 4)
    # the other BASELINE configs (2, 3, 4 math / AS) in the SAME driver run: short runs of this script, one after the other, on the same GPU
    line["configs"] = None
    if headline and args.full and not args.no_extras and os.environ.get("CTGCN_BENCH_OTHER_CONFIGS", "1") != "0":
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        line["configs"] = other_configs(line, log)
        line["forced_dist"] = forced_dist_leg(args, log)
    line["bench_wall_s"] = round(time.time() - T_START, 1)
    detail_path = args.detail_file or os.path.join(ROOT, "gpurun_out", "bench_detail%s.json" % ("" if args.workload == "synthetic-1m" else "_" + args.workload))
    if not args.full and args.detail_file is None:
        detail_path = None                     # a plain run keeps to its one line
    else:
        try:
            os.makedirs(os.path.dirname(detail_path) or ".", exist_ok=True)
            with open(detail_path, "w") as fh:
                json.dump(line, fh, indent=1)
            log("full record: %s (%d bytes)" % (detail_path, os.path.getsize(detail_path)))
        except OSError as exc:
            log("could not write %s: %s" % (detail_path, exc))
            detail_path = None
    record = compact_record(line, detail_path)
    text = json.dumps(record, separators=(",", ":"))
    assert len(text) < MAX_LINE_BYTES, "bench line is %d bytes (limit %d): move fields to the detail file" % (len(text), MAX_LINE_BYTES)
    sys.stdout.flush()
    os.dup2(saved_stdout, 1)
    print(text, flush=True)
    os.dup2(2, 1)               # whatever RCCL prints while shutting down must not follow the JSON line on stdout
    if use_dist:
        dist.destroy_process_group()


MAX_LINE_BYTES = 4096       # the driver keeps ~9 KB of stdout: round 5's 23 KB line did not parse there
T_START = time.time()
DUMP_BYTES = 64 * 10 ** 6   # --dump-outputs: size of all files written, .npy headers included
DUMP_SEED = 20261015


def dump_outputs(path, arrays, budget, log):
    """{name: tensor} -> path/<name>.npy, float64 kept, anything else as float32.  When the arrays would take more than `budget` bytes,
    each keeps the rows of one fixed seeded sample along its largest axis (the node axis of every CTGCN output), the same rows for
    arrays with as many nodes, and path/<name>__index.npy lists them (float64)."""
    import numpy as np
    import torch
    os.makedirs(path, exist_ok=True)
    header = 128                                                    # an .npy header of these shapes is 128 bytes
    itemsize = {k: 8 if t.dtype == torch.float64 else 4 for k, t in arrays.items()}
    axis = {k: max(range(t.dim()), key=lambda i: t.shape[i]) for k, t in arrays.items()}
    full = sum(t.numel() * itemsize[k] + header for k, t in arrays.items())
    # bytes per sampled row: the row itself + its index
    per_row = {k: t.numel() // max(1, t.shape[axis[k]]) * itemsize[k] + 8 for k, t in arrays.items()}
    frac = 1.0 if full <= budget else (budget - 2 * header * len(arrays)) / sum(t.shape[axis[k]] * per_row[k] for k, t in arrays.items())
    written = 0
    for k, t in arrays.items():
        dtype = torch.float64 if itemsize[k] == 8 else torch.float32
        if frac < 1.0:
            rows = t.shape[axis[k]]
            idx = np.sort(np.random.default_rng(DUMP_SEED).choice(rows, size=int(rows * frac), replace=False))
            t = t.index_select(axis[k], torch.from_numpy(idx).to(t.device))
            np.save(os.path.join(path, k + "__index.npy"), idx.astype(np.float64))
            written += os.path.getsize(os.path.join(path, k + "__index.npy"))
        np.save(os.path.join(path, k + ".npy"), t.detach().to(dtype).cpu().numpy())
        written += os.path.getsize(os.path.join(path, k + ".npy"))
    assert written <= budget, "dumped %d bytes, budget %d" % (written, budget)
    log("outputs of the last timed step: %s (%s, %d bytes)" % (path, "full" if frac == 1.0 else "%.4f of the rows" % frac, written))


def _pick(d, keys):
    return {k: d[k] for k in keys if d is not None and k in d}


def compact_record(line, detail_path):
    """The ONE stdout line: the driver contract's keys + `roofline` + `cpu_baseline` + one-number summaries of the short legs.
    Everything else (per-config records, kernel tables, GRU / k-core / backward rooflines, notes) is in the detail file."""
    cfg = line["config"]
    rec = _pick(line, ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"))
    rec["config"] = _pick(cfg, ("workload", "name", "nodes", "snapshots", "max_core", "aggregated_edges_per_step", "parallelism"))
    rec["config"]["workload"] = cfg["workload"][:240]
    r = line.get("roofline")
    if r:
        rr = _pick(r, ("bound", "achieved", "peak", "unit", "frac", "frac_8d", "traffic", "traffic_over_algorithmic_bytes", "avg_launch_ms",
                       "algorithmic_bytes_per_launch", "launches_timed", "frac_of_measured_copy_bw"))
        rr["kernel"] = r["kernel"].split(" (")[0]
        if r["bound"] == "cache":       # the contract's vocabulary is hbm | mfma: the gather of a small window is served on-die (detail: bound_note)
            rr["bound"], rr["served_by"] = "hbm", "L2 / Infinity Cache (X of a snapshot fits on-die)"
        rec["roofline"] = rr
    else:
        rec["roofline"] = None
    c = line.get("cpu_baseline")
    if c:
        rec["cpu_baseline"] = _pick(c, ("value", "unit", "cores", "kind", "value_coalesced_csr", "protocol"))
        rec["cpu_baseline"]["sample"] = c.get("sample_short", c.get("sample", ""))[:300]
    else:
        rec["cpu_baseline"] = None
    also = {}
    if line.get("hbm_copy_GBps_measured"):
        also["hbm_copy_GBps_measured"] = line["hbm_copy_GBps_measured"]["value"]
    k = line.get("kernel_ms_per_step_rank0")
    if k:
        also["kernel_ms_per_step"] = k
    g = line.get("roofline_gru") or {}
    g = g.get("fused_layers", g)
    if g.get("frac") is not None:
        also["gru_layer_mfma_frac"] = g["frac"]
    if line.get("eager_ms_per_step") is not None:
        also["eager_ms_per_step"] = line["eager_ms_per_step"]
    if line.get("exact_fp32"):
        also["exact_fp32_ms"] = line["exact_fp32"]["ms_per_step"]
    ts = line.get("training_step")
    if ts:
        also["training_step_ms"] = ts.get("ms_per_step", ts.get("error"))
    kc = line.get("roofline_kcore")
    if kc:
        also["kcore_exact_ms"], also["kcore_frac"] = kc["peel_ms_exact"], kc["frac"]
    if line.get("cpu_baseline_kcore"):
        also["kcore_cpu_ms"] = round(line["cpu_baseline_kcore"]["value"], 1)
    if line.get("configs"):
        also["configs_ms"] = {w: ([c.get("ms_per_step"), c.get("eager_ms_per_step"), (c.get("roofline_d128") or {}).get("frac"), (c.get("training_step") or {}).get("ms_per_step")]
                                  if "error" not in c else c["error"][:60]) for w, c in line["configs"].items() if w != "synthetic-1m"}
        also["configs_ms_fields"] = "forward ms (hipGraph replay), eager forward ms, d=128 aggregation frac, training step ms"
    if line.get("forced_dist"):
        also["forced_dist_ms"] = line["forced_dist"].get("ms_per_step", "error")
    if line.get("per_rank_ms"):
        also["per_rank_ms"] = [[round(p.get(q, 0.0), 2) for q in ("snapshot_branches_ms", "exchange_exposed_ms", "temporal_head_ms")] for p in line["per_rank_ms"]]
    also["bench_wall_s"] = line.get("bench_wall_s")
    rec["also"] = also
    rec["detail_file"] = os.path.relpath(detail_path, ROOT) if detail_path else None
    return rec


def pmc_traffic(args, roof, log):
    """HBM bytes per launch of the dominant aggregation kernel, measured now: `rocprofv3 --kernel-trace --pmc FETCH_SIZE` and `... --pmc WRITE_SIZE`
    as SEPARATE passes (MI355X_MICROARCH.md: the two do not share a pass) over `bench.py --steps 1 --warmup 1` of the same workload; every
    launch of the kernel in those runs is averaged, like `achieved` averages every launch of the timed steps.  FETCH_SIZE is in KiB and, on
    gfx950, counts the 128-byte requests of 16 B/lane streams at 64 B: doubled, as the guide prescribes; WRITE_SIZE in KiB."""
    import csv
    import glob
    import shutil
    import tempfile
    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return {"error": "rocprofv3 not found"}
    kern = roof["kernel"].split(" ")[0].split("<")[0]
    res = {"kernel": kern, "command": "rocprofv3 --kernel-trace --pmc <C> -- python bench.py --workload %s --steps 1 --warmup 1 --prewarm-s 0 --full "
                                      "--no-cpu-baseline --no-extras --no-pmc (C = FETCH_SIZE, then WRITE_SIZE)" % args.workload}
    t0 = time.time()
    for counter in ("FETCH_SIZE", "WRITE_SIZE"):
        tmp = tempfile.mkdtemp(prefix="ctgcn_pmc_", dir="/tmp")
        cmd = [exe, "--kernel-trace", "--pmc", counter, "--output-format", "csv", "-d", tmp, "-o", "bench", "--", sys.executable, os.path.abspath(__file__),
               "--workload", args.workload, "--steps", "1", "--warmup", "1", "--prewarm-s", "0", "--full", "--no-cpu-baseline", "--no-extras", "--no-pmc",
               "--detail-file", os.path.join(tmp, "detail.json")]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"))
            files = glob.glob(tmp + "/**/*counter_collection.csv", recursive=True)
            if p.returncode != 0 or not files:
                res["error"] = "%s pass: rc %d, %d csv: %s" % (counter, p.returncode, len(files), p.stderr.decode()[-300:])
                break
            vals = [float(r["Counter_Value"]) for f in files for r in csv.DictReader(open(f)) if kern in r["Kernel_Name"] and r["Counter_Name"] == counter]
            if not vals:
                res["error"] = "%s pass: no %s rows" % (counter, kern)
                break
            res[counter] = {"launches": len(vals), "mean_KiB": sum(vals) / len(vals)}
        except subprocess.TimeoutExpired:
            res["error"] = "%s pass timed out after 240 s" % counter
            break
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    if "error" not in res:
        res["fetch_bytes_corrected_x2"] = res["FETCH_SIZE"]["mean_KiB"] * 1024 * 2
        res["write_bytes"] = res["WRITE_SIZE"]["mean_KiB"] * 1024
        res["hbm_bytes_per_launch"] = int(res["fetch_bytes_corrected_x2"] + res["write_bytes"])
    res["seconds"] = round(time.time() - t0, 1)
    log("pmc traffic: %s (%.0f s)" % (res.get("hbm_bytes_per_launch", res.get("error")), res["seconds"]))
    return res


def dry_run(args):
    """bench.py --dry: everything of a multi-rank run except the GPU — process group (gloo, 127.0.0.1), LPT assignment from the window's
    snapshot sizes, per-rank stats gathered with all_gather_object, W warm-up + K timed "steps" (an all_to_all of a few floats, where the
    real step exchanges the snapshot states) between barriers, max over ranks, ONE JSON line from rank 0."""
    import torch
    import torch.distributed as dist
    sys.stdout.flush()
    saved_stdout = os.dup(1)
    os.dup2(2, 1)
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ctgcn_amd import snapshot_parallel as spp
    from ctgcn_amd.synth import prefix_sizes
    W = WORKLOADS[args.workload]
    T = W["T"]
    sizes = prefix_sizes(W["edges"], T) if W["cumulative"] else [W["edges"]] * T
    assignment = spp.plan_assignment(sizes, world)
    mine = assignment[rank]
    local_stats = {t: dict(K=1, nnz=2 * sizes[t], agg=2 * sizes[t], max_core=1) for t in mine}
    gathered = [None] * world
    dist.all_gather_object(gathered, local_stats)
    stats = {}
    for g in gathered:
        stats.update(g)
    assert sorted(stats) == list(range(T)), "every snapshot must be owned by exactly one rank"
    agg_edges_step = W["diff"] * sum(stats[t]["agg"] for t in range(T))
    send = torch.full((world, 4), float(rank))
    recv = torch.empty_like(send)

    def step():
        dist.all_to_all_single(recv, send)

    for _ in range(args.warmup):
        step()
    dist.barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    dist.barrier()
    tt = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(tt, op=dist.ReduceOp.MAX)
    assert recv[:, 0].tolist() == [float(r) for r in range(world)]
    per_rank = [None] * world
    dist.all_gather_object(per_rank, {"rank": rank, "snapshots": mine, "edges": sum(sizes[t] for t in mine)})
    if rank == 0:
        ms = 1000.0 * float(tt.item()) / max(1, args.steps)
        line = {"metric": "dry run (no kernels): launcher, rendezvous and bookkeeping of the multi-rank bench", "value": agg_edges_step / max(ms * 1e-3, 1e-12),
                "unit": "edges/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms, "higher_is_better": True,
                "scaling": "strong", "vs_baseline": None, "dtype": "f32", "data": "none (dry)", "dry": True,
                "config": {"workload": W["desc"], "name": args.workload, "snapshots": T, "aggregated_edges_per_step": agg_edges_step,
                           "assignment": assignment, "parallelism": "snapshot-parallel x%d" % world},
                "per_rank": per_rank}
        sys.stdout.flush()
        os.dup2(saved_stdout, 1)
        print(json.dumps(line), flush=True)
        os.dup2(2, 1)
    dist.destroy_process_group()


def config_summary(line):
    r = line.get("roofline") or {}
    by = line.get("roofline_by_width") or {}
    r128 = by.get("128", r)
    cpu = line.get("cpu_baseline") or {}
    ts = line.get("training_step") or {}
    return {"workload": line["config"]["workload"], "ms_per_step": line["ms_per_step"], "eager_ms_per_step": line.get("eager_ms_per_step"),
            "value": line["value"], "unit": line["unit"],
            "steps": line["steps"], "warmup": line["warmup"],
            "roofline_d128": {k: r128.get(k) for k in ("kernel", "bound", "achieved", "peak", "unit", "frac", "avg_launch_ms", "launches_timed",
                                                         "survey_8d_frac", "output_rows_written_frac")} if r128 else None,
            "roofline_dominant_frac": r.get("frac"),
            "training_step": {k: ts.get(k) for k in ("ms_per_step", "steps", "what", "memory", "gradients", "error") if k in ts} if ts else None,
            "torch_rocm_baseline": line.get("torch_rocm_baseline"),
            "cpu_baseline": {k: cpu.get(k) for k in ("value", "unit", "cores", "kind", "value_coalesced_csr", "protocol")} if cpu else None}


def other_configs(main_line, log):
    """{name: summary} for BASELINE configs 2-4 (+ this run's config 5): `python bench.py --workload W --steps 20 --full --no-extras --train-leg`
    each (with a 4 s CPU baseline and the stock-PyTorch baseline)."""
    out = {"synthetic-1m": config_summary(main_line)}
    for w in ("enron-like", "facebook-like", "math-like", "as-like"):
        detail = os.path.join(ROOT, "gpurun_out", "bench_detail_%s.json" % w)
        cmd = [sys.executable, os.path.abspath(__file__), "--workload", w, "--steps", "20", "--warmup", "3", "--no-extras", "--train-leg", "--no-pmc",
               "--detail-file", detail, "--full", "--cpu-budget-s", "4"]
        t0 = time.time()
        try:
            if os.path.exists(detail):
                os.remove(detail)
            p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=240)
            if p.returncode != 0 or not os.path.exists(detail):
                out[w] = {"error": "rc %d: %s" % (p.returncode, p.stderr.decode()[-400:])}
            else:
                out[w] = config_summary(json.load(open(detail)))
        except subprocess.TimeoutExpired:
            out[w] = {"error": "timed out after 240 s"}
        log("config %s: %s (%.1f s)" % (w, out[w].get("ms_per_step", out[w].get("error")), time.time() - t0))
    return out


def forced_dist_leg(args, log):
    """The SAME window through the sharded code path with ONE rank under RCCL (CTGCN_FORCE_DIST=1: process group, all_to_all exchange of the
    snapshot states, temporal GRU on the receive buffer) — the first point of a SCALE curve is this path at N = 1, so the driver's N = 1 number
    can be checked against the headline (what is left is RCCL's send -> recv copy of 8 GB that a single rank does for nothing)."""
    detail = os.path.join(ROOT, "gpurun_out", "bench_detail_forced_dist.json")
    cmd = [sys.executable, os.path.abspath(__file__), "--workload", args.workload, "--steps", str(args.steps), "--warmup", str(args.warmup),
           "--full", "--no-extras", "--no-cpu-baseline", "--no-pmc", "--detail-file", detail]
    env = dict(os.environ, CTGCN_FORCE_DIST="1", MASTER_ADDR="127.0.0.1", MASTER_PORT="29541", RANK="0", WORLD_SIZE="1", LOCAL_RANK="0",
               HSA_ENABLE_IPC_MODE_LEGACY="0")
    t0 = time.time()
    try:
        p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
        if p.returncode != 0 or not os.path.exists(detail):
            return {"error": "rc %d: %s" % (p.returncode, p.stderr.decode()[-300:])}
        r = json.load(open(detail))
        out = {"ms_per_step": r["ms_per_step"], "what": "CTGCN_FORCE_DIST=1: one rank, RCCL process group, sharded forward (all_to_all exchange)",
               "per_rank_ms": r.get("per_rank_ms")}
    except subprocess.TimeoutExpired:
        out = {"error": "timed out after 300 s"}
    log("forced single-rank RCCL path: %s (%.1f s)" % (out.get("ms_per_step", out.get("error")), time.time() - t0))
    return out


def training_leg(model, x_list, adj_list, ops, first, agg_edges_step, log):
    """fwd + bwd + Adam on the same window (the reference's training step, embedding.py:346-352, with the surrogate loss
    out.square().mean(): the negative-sampling loss is outside the hot path):
    2 warm-up + 3 timed steps after the forward measurement,
    plus the backward kernels' HIP-event times and their rooflines."""
    import torch
    recs = []
    ops.set_launch_timer(lambda name, s, e, meta: recs.append((name, s, e, meta)))
    model.train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    try:
        def one():
            opt.zero_grad(set_to_none=True)
            out = first(model(x_list, adj_list))
            out.square().mean().backward()
            opt.step()
        # steady state: the caching allocator still holds the blocks of the inference legs (other sizes); training's first steps would
        # pay hipFree / hipMalloc of tens of GB inside the timed region (measured: 1373 ms against 926 ms for the same step under --train)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        for _ in range(2):
            one()
        torch.cuda.synchronize()
        recs.clear()
        retries0 = torch.cuda.memory_stats().get("num_alloc_retries", 0)
        steps = 3
        t0 = time.perf_counter()
        for _ in range(steps):
            one()
        torch.cuda.synchronize()
        ms = 1000.0 * (time.perf_counter() - t0) / steps
        # the gradients of the last timed step (opt.zero_grad runs at the START of a step): every one finite, and a checksum a reader can
        # compare between runs / builds (sum of |g| over all parameters in float64, and the largest entry)
        gsum, gmax, gcount = 0.0, 0.0, 0
        for name, prm in model.named_parameters():
            if prm.grad is None:
                continue
            assert bool(torch.isfinite(prm.grad).all()), "training step: non-finite gradient in %s" % name
            gsum += float(prm.grad.double().abs().sum())
            gmax = max(gmax, float(prm.grad.abs().max()))
            gcount += 1
        assert gcount > 0 and gsum > 0.0, "training step: no gradients"
        mem = {"max_allocated_GB": round(torch.cuda.max_memory_allocated() / 1e9, 1), "reserved_GB": round(torch.cuda.memory_reserved() / 1e9, 1),
               "alloc_retries_in_timed_steps": int(torch.cuda.memory_stats().get("num_alloc_retries", 0) - retries0)}
        by = {}
        for name, s_, e_, meta in recs:
            by.setdefault(name, []).append((s_.elapsed_time(e_), meta))
        res = {"ms_per_step": round(ms, 2), "steps": steps, "what": "forward + backward + Adam, surrogate loss out.square().mean(), same window and weights",
               "aggregated_edges_per_s_fwd_plus_bwd": 2.0 * agg_edges_step / (ms * 1e-3),
               "kernel_ms_per_step": {k: round(sum(t for t, _ in v) / steps, 3) for k, v in sorted(by.items())}, "memory": mem,
               "gradients": {"all_finite": True, "tensors": gcount, "sum_abs": gsum, "max_abs": gmax,
                             "parity": "tests/test_gpu_configs.py::test_config5_training_* hold this path to float64 autograd of the reference "
                                       "at 1 M rows (1e-4 of each gradient tensor's largest entry)"}}
        if "agg_bwd" in by:
            g = by["agg_bwd"]
            t_ms = sum(t for t, _ in g) / len(g)
            b = sum(m["nnz"] * (4 * m["d"] + 9) + m["n"] * 8 * m["d"] + 4 * (m["n"] + 1) for _, m in g) / len(g)
            res["roofline_agg_bwd"] = {"kernel": "agg_bwd_kernel (gather of Z[col, slot] rows: dX = S0 + sum_e val_e Z[col_e, slot_e])", "bound": "hbm",
                                       "achieved": round(b / (t_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                       "frac": round(b / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "avg_launch_ms": round(t_ms, 4),
                                       "algorithmic_bytes_per_launch": int(b), "launches_timed": len(g)}
        if "agg_bwd_prep" in by:
            g = by["agg_bwd_prep"]
            t_ms = sum(t for t, _ in g) / len(g)
            b = sum(3.0 * m["n"] * m["K"] * 4 * m["d"] + (m["n"] * 4 * m["d"] if m.get("self_loop") else 0) for _, m in g) / len(g)
            res["roofline_agg_bwd_prep"] = {"kernel": "agg_bwd_prep_kernel (elementwise: dH, H in; Z, S0 out)", "bound": "hbm",
                                            "achieved": round(b / (t_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                            "frac": round(b / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "avg_launch_ms": round(t_ms, 4),
                                            "launches_timed": len(g)}
        # the two backward kernels of ctgcn_gru_bwd.hip: HBM-bound by design (their only HBM intermediates are the recompute pass's gates
        # + h in and the fresh steps' d_gi out / in); the matrix-core side is reported next to it (bf16 x 2: three MFMAs per product of the
        # gate products, four per weight-gradient product — K = 32 of the MFMA filled with the tile's 16 rows twice)
        def bwd_roof(name, what, bytes_of, mfma_of):
            g = by.get(name)
            if not g:
                return None
            t_ms = sum(t for t, _ in g)
            b = sum(bytes_of(m) for _, m in g)
            fl = sum(mfma_of(m) for _, m in g)
            return {"kernel": what, "bound": "hbm", "achieved": round(b / (t_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(b / (t_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4), "ms_per_step": round(t_ms / steps, 3), "launches_timed": len(g),
                    "algorithmic_bytes_per_step": int(b / steps),
                    "mfma_executed_TFLOPs": round(fl / (t_ms * 1e-3) / 1e12, 1), "mfma_frac_of_dense_16bit_peak_2500": round(fl / (t_ms * 1e-3) / 1e12 / 2500.0, 4)}
        rs = lambda m: float(m["rows"]) * m["steps"]
        res["roofline_gru_bwd_rec"] = bwd_roof(
            "gru_bwd_rec", "gru_bwd_rec_kernel (backward recurrence, W_hh^T resident, dW_hh in registers; in: gates 2 KB + h 0.5 KB per row-step, "
            "out: d_gi 1.5 KB per fresh row-step)",
            lambda m: rs(m) * 2560.0 + rs(m) * m["fresh"] * 1536.0 + m["rows"] * 512.0 * (m["steps"] if m.get("per_step") else 1),
            lambda m: float(m["rows"]) * (m["steps"] - 1) * 2.0 * 128 * 384 * (3 + 4))
        res["roofline_gru_bwd_in"] = bwd_roof(
            "gru_bwd_in", "gru_bwd_in_kernel (dx = d_gi W_ih, dW_ih in registers, ReLU mask + suffix sums of the aggregation backward in the "
            "epilogue; in: d_gi 1.5 KB + x 0.5 KB, out: Z 0.5 KB per fresh row-step)",
            lambda m: rs(m) * m["fresh"] * (1536.0 + 516.0 + 512.0),
            lambda m: rs(m) * m["fresh"] * 2.0 * 128 * 384 * (3 + 4))
        log("training step: %.1f ms" % ms)
        if os.environ.get("CTGCN_BENCH_REFERENCE_LOSS", "1") != "0":
            try:
                res["reference_loss_batch_step"] = reference_loss_leg(model, x_list, adj_list, first, opt, log)
            except Exception as exc:
                res["reference_loss_batch_step"] = {"error": "%s: %s" % (type(exc).__name__, str(exc)[:300])}
                log("reference-loss leg failed: %s" % res["reference_loss_batch_step"]["error"])
        return res
    finally:
        ops.set_launch_timer(None)
        model.eval()
        del opt
        for p in model.parameters():
            p.grad = None
        torch.cuda.empty_cache()


def torch_rocm_baseline(model, x_list, adj_list, W, our_ms, first, log):
    """The reference's OWN GPU path on this GPU (reference embedding.py:32 runs on cuda:0): torch.sparse.mm on the uncoalesced COO tensors of
    utils.py:89-95 (hipSPARSE) in the loop of layers.py:41-48, nn.GRU (MIOpen; rows in chunks below its 2^31 limit), nn.LayerNorm, driven by
    the model's state dict through oracle/torch_path.py — stock PyTorch-ROCm, none of this library's kernels.  Baseline only.
    Windows up to 200 000 nodes: the whole CTGCN forward, warm-up 2, 5 repeats, median, next to this library's forward of the same window.
    Config 5: the snapshot branch (MLP + CoreDiffusion layers, models.py:244-246) of the LARGEST snapshot, warm-up 1, 3 repeats, next to this
    library's time for the same branch (the whole window on stock PyTorch would hold 16 x 8 COO matrices + [N, K, d] stacks: not the point)."""
    import torch
    from oracle import torch_path as TP
    dev = next(model.parameters()).device
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    owned = [t for t, a in enumerate(adj_list) if a is not None]
    n = adj_list[owned[0]].n

    def coo_lists(ts):
        return {t: [TP.coo_like_reference(m).to(dev) for m in adj_list[t].cpu().to_scipy_list()] for t in ts}

    def median_ms(fn, warm, reps):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times.append(1000.0 * (time.perf_counter() - t0))
        return statistics.median(times), min(times), max(times)

    with torch.no_grad():
        if n <= 200_000:
            ref_adj = coo_lists(owned)
            lists = [ref_adj[t] for t in owned]
            fn = lambda: TP.ctgcn(sd, x_list, lists, "GRU", W["model"], W["act"])
            got, want = first(model(x_list, adj_list)), first(fn())
            err = float((got - want).abs().max())
            med, lo, hi = median_ms(fn, 2, 5)
            out = {"what": "whole CTGCN-%s forward of the window" % W["model"], "ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                   "this_library_ms": round(our_ms, 3), "ratio": round(med / our_ms, 2), "protocol": "warm-up 2, 5 repeats, median"}
        else:
            t = max(owned, key=lambda q: adj_list[q].aggregated_edges)
            lists = coo_lists([t])[t]
            pre = "duffision_list.%d." % t
            fn = lambda: TP.cdn(sd, pre, TP.mlp(sd, "mlp_list.%d." % t, x_list[t], W["act"]), lists)
            ours = lambda: model.snapshot_branch(t, x_list[t], adj_list[t])[0]
            got, want = ours(), fn()
            err = float((got - want).abs().max())
            med, lo, hi = median_ms(fn, 1, 3)
            omed, _, _ = median_ms(ours, 2, 5)
            out = {"what": "snapshot branch (MLP + %d CoreDiffusion layers) of snapshot %d, the largest (%d stored entries, K = %d)" % (
                       W["diff"], t, adj_list[t].nnz, adj_list[t].K), "ms": round(med, 3), "min_ms": round(lo, 3), "max_ms": round(hi, 3),
                   "this_library_ms": round(omed, 3), "ratio": round(med / omed, 2), "protocol": "warm-up 1, 3 repeats, median (this library: warm-up 2, 5 repeats)"}
    out.update(kind="reference path restated (oracle/torch_path.py) on stock PyTorch-ROCm %s: torch.sparse.mm (COO, hipSPARSE) + nn.GRU (MIOpen) + "
                    "nn.LayerNorm on the same GPU" % torch.__version__, max_abs_diff_vs_this_library=err, baseline_only=True)
    log("torch-ROCm baseline: %.2f ms vs %.2f ms (x%.1f), max |diff| %.1e" % (out["ms"], out["this_library_ms"], out["ratio"], err))
    return out


def reference_loss_leg(model, x_list, adj_list, first, opt, log):
    """The reference's REAL training batch (embedding.py:340-352 with metrics.py:38-93): full-graph forward of the window, NegativeSamplingLoss on
    ONE batch of 2 048 nodes (config/uci.json:21 batch_size; neg_num 20, Q 20) with positives from a random-walk corpus (walk_time 20, walk_length 5, config/uci.json:750-751:
    preprocessing/random_walk.py:8-69, here ctgcn_walks.hip) + negatives from the node-frequency table, loss.backward().  The reference steps the
    optimizer once per EPOCH (gradient accumulation over the batches, embedding.py:349-351), so a batch is forward + loss + backward; the
    optimizer step is timed on its own.  Corpus generation (once per dataset in the reference's preprocessing task) is outside the timed region."""
    import numpy as np
    import torch
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import negative_table, random_walk_corpus
    owned = [t for t, a in enumerate(adj_list) if a is not None]
    n = adj_list[owned[0]].n
    dev = next(model.parameters()).device
    t0 = time.perf_counter()
    pairs, tables = [], []
    for t in owned:
        a = adj_list[t]
        # the snapshot graph = the largest matrix of the k-core list without the + I (every stored entry of the slot-tagged CSR)
        pr, fr = random_walk_corpus(a.row_ptr, a.col, a.val, walk_length=5, walk_time=20, weighted=True, seed=1000 + t)
        pairs.append(pr)
        tables.append(torch.from_numpy(negative_table(fr).astype(np.int32)).to(dev))
    torch.cuda.synchronize()
    corpus_s = time.perf_counter() - t0
    loss_model = NegativeSamplingLoss(pairs, tables, neg_num=20, Q=20, seed=7)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    batch = torch.randperm(n, device=dev, generator=gen)[:2048]

    def one():
        out = first(model(x_list, adj_list))
        loss = loss_model([list(out), batch])
        loss.backward()
        return loss

    model.zero_grad(set_to_none=True)
    for _ in range(2):
        one()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    steps = 3
    for _ in range(steps):
        loss = one()
    torch.cuda.synchronize()
    ms = 1000.0 * (time.perf_counter() - t0) / steps
    assert bool(torch.isfinite(loss).all())
    for name, prm in model.named_parameters():
        if prm.grad is not None:
            assert bool(torch.isfinite(prm.grad).all()), "reference-loss batch: non-finite gradient in %s" % name
    t0 = time.perf_counter()
    opt.step()
    torch.cuda.synchronize()
    opt_ms = 1000.0 * (time.perf_counter() - t0)
    model.zero_grad(set_to_none=True)
    res = {"ms_per_batch": round(ms, 2), "batch_nodes": 2048, "neg_num": 20, "Q": 20, "walk_time": 20, "walk_length": 5, "steps": steps,
           "loss": float(loss.item()), "optimizer_step_ms": round(opt_ms, 2), "corpus_generation_s": round(corpus_s, 2),
           "walk_partner_entries": int(sum(p.col.numel() for p in pairs)),
           "what": "forward of the window + NegativeSamplingLoss on one batch + backward (reference embedding.py:346-348); the optimizer steps once per epoch there"}
    log("reference-loss batch: %.1f ms (+ optimizer step %.1f ms; corpus %.1f s)" % (ms, opt_ms, corpus_s))
    return res


def cpu_baseline(adj_list, widths, budget_s, log):
    """Reference CPU path (layers.py:41-47 + 48: the loop of torch.sparse.mm over the WHOLE k-core list of one snapshot + add + ReLU; operands
    built as utils.py:89-95 builds them: int64-index, uncoalesced COO) on all host cores, plus the same loop on coalesced CSR operands.
    Sample (bounded, ~10-30 s): the window's LARGEST snapshot, every one of its K matrices, at the model's layer widths (one
    width when all layers share it: edges are counted per width).  Protocol: warm-up 2, 5 timed repeats, median — as many of those as fit
    the budget: on an MI355X host one pass of the 8-matrix loop at 1M nodes is ~17 s as COO (ATen's N x d passes dominate, whatever the
    edge count), so config 5 gets the first pass as warm-up-free measurement of the loop; the small configs run the full protocol.  What ran
    is written into `protocol`."""
    import torch
    from oracle import torch_path as TP
    cores = os.cpu_count() or 1
    torch.set_num_threads(cores)
    owned = [t for t, a in enumerate(adj_list) if a is not None]
    pick = max(owned, key=lambda t: adj_list[t].aggregated_edges)
    adj = adj_list[pick]
    n = adj.n
    if len(set(widths)) == 1:
        widths = widths[:1]
    xs = {d: torch.randn(n, d) for d in set(widths)}
    mats = adj.cpu().to_scipy_list()                       # reference order: highest k (smallest matrix) first
    coo = [TP.coo_like_reference(m) for m in mats]
    csr = [torch.sparse_csr_tensor(torch.from_numpy(m.indptr.astype("int64")), torch.from_numpy(m.indices.astype("int64")),
                                   torch.from_numpy(m.data), size=m.shape) for m in mats]
    edges = sum(m.nnz for m in mats) * len(widths)

    def loop(ops_):
        t0 = time.perf_counter()
        for d in widths:
            hs = TP.aggregate_loop(ops_, xs[d])
        del hs
        return time.perf_counter() - t0

    TP.aggregate_loop(coo[:1], xs[widths[0]])              # spin up the thread pool on the smallest matrix (not a pass)
    res, proto = {}, {}
    for label, ops_ in (("coo", coo), ("csr", csr)):
        share = budget_s * (0.62 if label == "coo" else 0.38)      # the COO pass is ~1.8x the CSR pass
        first = loop(ops_)
        fit = int(share / max(first, 1e-9))                 # passes of this variant the budget holds, the first one included
        if fit < 3:
            res[label], proto[label] = (first, first, first), "1 pass, no warm-up (a pass is %.1f s, the budget holds %d)" % (first, fit)
            continue
        if fit < 5:                                         # >= 3 timed passes matter more than a warm-up: the first pass is a sample
            times = [first] + [loop(ops_) for _ in range(2)]
            warm = 0
        else:
            warm = 2 if fit >= 7 else 1                     # the first pass is the (first) warm-up
            if warm == 2:
                loop(ops_)
            times = [loop(ops_) for _ in range(max(3, min(5, fit - warm)))]
        res[label] = (statistics.median(times), min(times), max(times))
        proto[label] = "warm-up %d, %d timed passes, median (min %.3f / max %.3f s)" % (warm, len(times), min(times), max(times))
    log("cpu baseline: snapshot %d, all %d matrices, %d aggregated edges/pass, coo %.3fs csr %.3fs" % (pick, len(mats), edges, res["coo"][0], res["csr"][0]))
    return {"value": edges / res["coo"][0], "unit": "edges/s", "cores": cores, "kind": "port",
            "value_coalesced_csr": edges / res["csr"][0],
            "protocol": "COO: %s; CSR: %s" % (proto["coo"], proto["csr"]),
            "sample_short": "reference layers.py:41-48 loop (torch.sparse.mm on uncoalesced int64 COO + add + relu; value_coalesced_csr: same on torch CSR) over ALL "
                            "%d k-core matrices of snapshot %d (largest of the window), %d nodes, widths %s, %d aggregated edges/pass, %d threads" % (
                                len(mats), pick, n, widths, edges, cores),
            "sample": "oracle/torch_path.py (reference layers.py:41-48 restated: torch.sparse.mm on uncoalesced int64 COO operands as "
                      "utils.py:89-95 builds them + add + relu; `value_coalesced_csr` = the same loop on coalesced torch CSR operands), "
                      "snapshot %d of the window (the largest), the full loop over its %d k-core matrices (%d nodes), feature widths %s, "
                      "%d aggregated edges per pass, pass %.3f s (COO) / %.3f s (CSR), torch.set_num_threads(%d)" % (
                          pick, len(mats), n, widths, edges, res["coo"][0], res["csr"][0], cores)}


def cpu_baseline_kcore(kc_graph, n, log):
    """k-core baseline (reference structure_generation.py:35 nx.core_number): the oracle's C Batagelj-Zaversnik peel, one thread,
    on the same snapshot the GPU peel was timed on; warm-up 1, 5 repeats, median.  networkx itself is timed when the snapshot is
    small enough to finish in seconds."""
    import ctypes
    import numpy as np
    from oracle import oracle as O
    rp, col = kc_graph
    indptr = rp.cpu().numpy().astype(np.int64)
    indices = col.cpu().numpy().astype(np.int32)
    core = np.zeros(n, dtype=np.int32)
    lib = O.lib()
    call = lambda: lib.oracle_kcore_bz(ctypes.c_int64(n), indptr.ctypes.data_as(ctypes.c_void_p), indices.ctypes.data_as(ctypes.c_void_p),
                                       core.ctypes.data_as(ctypes.c_void_p))
    call()
    times = []
    for _ in range(5):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    out = {"value": statistics.median(times) * 1e3, "unit": "ms", "cores": 1, "kind": "port",
           "sample": "oracle/ctgcn_oracle.c Batagelj-Zaversnik bin-sort peel (the algorithm of networkx.core_number, reference "
                     "structure_generation.py:35), %d nodes, %d stored entries, warm-up 1, 5 repeats, median" % (n, len(indices)),
           "max_core": int(core.max(initial=0))}
    if len(indices) <= 1_500_000:
        try:
            import networkx as nx
            import scipy.sparse as sp
            g = nx.from_scipy_sparse_array(sp.csr_matrix((np.ones(len(indices), dtype=np.int8), indices, indptr), shape=(n, n)))
            t0 = time.perf_counter()
            cn = nx.core_number(g)
            out["networkx_core_number_ms"] = (time.perf_counter() - t0) * 1e3
            assert max(cn.values(), default=0) == out["max_core"]
        except ImportError:
            pass
    log("cpu k-core baseline: %.1f ms" % out["value"])
    return out


if __name__ == "__main__":
    main()
