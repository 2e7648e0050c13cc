"""GCRN (hid_dim 500, embed_dim 128, dropout 0.5, GRU, identity features: the GCRN block of every reference config) on three window
shapes, with the GCN steps computed three ways:

  fused      ctgcn_amd.baseline.GCRN as shipped: ops.gcn_conv (ctgcn_gcn.hip) with the bias, ReLU + dropout or the row normalisation in
             the aggregation's epilogue, the backward as one pre-pass and the aggregation over the transposed CSR; the fused GRU
  composed   the same module with GraphConvolution.aggregate composed from ops.spmm_csr over Â (forward) and Â^T (backward) and torch
             ops for the bias, ReLU, dropout, F.normalize and the stack; the same fused GRU
  torch      stock torch: torch.sparse.mm, F.relu, F.dropout, F.normalize, torch.stack, nn.GRU, nn.LayerNorm, autograd

    python tools/gcrn_bench.py --workload {uci-like,enron-like,synthetic-1m} [--out profiles/gcrn_bench_<workload>.json]     (GPU)

  uci-like       1 899 nodes, 7 snapshots, average degree 14
  enron-like     87 000 nodes, 10 snapshots, average degree 13 (largest degree about 500)
  synthetic-1m   1 M nodes, 8 M edges per snapshot, a window of 2 snapshots (layer 1's weight is N x 500 per snapshot: 2 GB, and as
                 much again for its gradient and for each Adam moment)

Per variant: the median over REPS timed calls (after 3 warm-up calls, the variants taking turns inside every repetition) of one epoch
in train() mode (forward with dropout, surrogate loss sum(out * C), backward, Adam step) and of one forward in eval() mode under
no_grad, both between device events followed by a synchronise, with the smallest and largest time of each; and the largest
difference of the eval-mode forward from the torch variant's, over the largest magnitude.  The GCN steps of the last snapshot are
also timed alone, fused against composed piece by piece (gcn_step_ms): layer 1's forward (500 wide, bias + ReLU + dropout), its
backward (pre-pass with the bias gradient + transposed aggregation), layer 2's forward (128 wide, bias + row normalisation) and its
backward.  By-bytes traffic of those pieces (from the shapes, see gcn_step_bytes) goes on the record beside the times.
"""
import argparse
import copy
import json
import os
import sys
import types

import numpy as np
import torch
from torch.nn import functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HID, D, DROPOUT = 500, 128, 0.5
REPS = {"uci-like": 30, "enron-like": 10, "synthetic-1m": 5}
SHAPES = {"uci-like": dict(n=1899, snapshots=7, avg_deg=14, max_degree_hint=None),
          "enron-like": dict(n=87000, snapshots=10, avg_deg=13, max_degree_hint=500),
          "synthetic-1m": dict(n=1000000, snapshots=2, avg_deg=16, max_degree_hint=None)}


def window(name, dev):
    """(features, GcnAdj list): the sparse identity for every snapshot, D^-1 (A + I) of every snapshot, scaled on the GPU"""
    import scipy.sparse as sp
    from ctgcn_amd import ops
    from ctgcn_amd.synth import dynamic_graph
    s = SHAPES[name]
    graphs = dynamic_graph(s["n"], s["avg_deg"], s["snapshots"], seed=3, max_degree_hint=s["max_degree_hint"])
    adjs = []
    for g in graphs:
        m = (g + sp.eye(s["n"])).tocsr()
        m.sort_indices()
        raw = ops.GcnAdj.from_scipy(m, dev)
        adjs.append(ops.GcnAdj(raw.row_ptr, raw.col, ops.gcn_normalize(raw.row_ptr, raw.col, raw.val, True)))
    idx = torch.arange(s["n"], device=dev)
    eye = torch.sparse_coo_tensor(torch.stack((idx, idx)), torch.ones(s["n"], device=dev), torch.Size((s["n"], s["n"])))
    return [eye for _ in graphs], adjs


class _Spmm(torch.autograd.Function):
    """Â S by ops.spmm_csr, with Â^T dY by the same kernel over the transposed CSR as its backward"""

    @staticmethod
    def forward(ctx, S, adj):
        from ctgcn_amd import ops
        ctx.adj = adj
        return ops.spmm_csr(adj.row_ptr, adj.col, adj.val, S.contiguous())

    @staticmethod
    def backward(ctx, dY):
        from ctgcn_amd import ops
        t = ctx.adj.transposed()
        return ops.spmm_csr(t.row_ptr, t.col, t.val, dY.contiguous()), None


def epilogue(P, bias, epi, p):
    from ctgcn_amd import ops
    if bias is not None:
        P = P + bias
    if epi == ops.GCN_EPI_RELU:
        return F.dropout(F.relu(P), p, training=p > 0)
    if epi == ops.GCN_EPI_L2NORM:
        return F.normalize(P, p=2)
    return P


def composed_aggregate(self, S, adj, epi, p, key, out):
    res = epilogue(_Spmm.apply(S, adj), self.bias, epi, p)
    if out is not None:
        out.copy_(res)
        return out
    return res


_sparse = {}


def torch_adj(adj):
    A = _sparse.get(id(adj))
    if A is None:
        A = _sparse[id(adj)] = adj.to_sparse_tensor().coalesce()
    return A


def torch_forward(self, x_list, edge_list):
    """the reference's GCRN.forward in stock torch ops on this module's parameters (X = I: X W = W)"""
    hx = []
    for t, adj in enumerate(edge_list):
        gcn, A = self.gcn_list[t], torch_adj(adj)
        h = F.dropout(F.relu(torch.sparse.mm(A, gcn.gc1.weight) + gcn.gc1.bias), self.dropout, training=self.training)
        hx.append(F.normalize(torch.sparse.mm(A, h @ gcn.gc2.weight) + gcn.gc2.bias, p=2))
    out, _ = self.rnn(torch.stack(hx, dim=0).transpose(0, 1))
    return self.norm(out).transpose(0, 1)


def variant(model, kind):
    m = copy.deepcopy(model)
    if kind == "composed":
        for gcn in m.gcn_list:
            for gc in (gcn.gc1, gcn.gc2):
                gc.aggregate = types.MethodType(composed_aggregate, gc)
    elif kind == "torch":
        m.forward = types.MethodType(torch_forward, m)
    return m


def timed(fn):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def round_robin(fns, reps):
    """(median, [min, max]) ms per key: 3 warm-up calls each, then `reps` rounds in which the variants take turns"""
    for fn in fns.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            times[k].append(timed(fn))
    return {k: float(np.median(v)) for k, v in times.items()}, {k: [float(min(v)), float(max(v))] for k, v in times.items()}


def gcn_step_bytes(n, nnz, d):
    """bytes one GCN step moves, by the shapes: the gather reads one d-wide row per stored entry plus the CSR, every N x d pass moves
    n d 4 bytes (row below); torch's dropout also stores a byte mask.
    fused forward, any epilogue: gather + write Y.
    composed forward: gather + write P; bias read + write; then ReLU (read + write) and dropout (read + write + mask), or F.normalize
      (read for the norm, read + write for the division).
    fused backward: pre-pass reads dY and Y and writes G; gather of G + write dS.
    composed backward: dropout (read dY + mask, write), ReLU (read 2, write 1), or F.normalize's (read 3, write 1 and the row dots);
      the bias gradient reads G; gather of G + write dS."""
    row, gather, csr = n * d * 4, nnz * d * 4, nnz * 8 + n * 4
    return {"fused_fwd": gather + csr + row,
            "composed_fwd_relu_dropout": gather + csr + 7 * row + n * d, "composed_fwd_l2norm": gather + csr + 6 * row,
            "fused_bwd": 3 * row + gather + csr + row,
            "composed_bwd_relu_dropout": 6 * row + n * d + gather + csr + row, "composed_bwd_l2norm": 5 * row + gather + csr + row}


def gcn_step_ms(adj, reps):
    """the two GCN steps alone on one snapshot, fused against composed, forward and backward"""
    from ctgcn_amd import ops
    dev = adj.device
    adj_t = adj.transposed()
    gen = torch.Generator(device=dev).manual_seed(2)
    fns = {}
    for name, d, epi, p in (("relu_dropout", HID, ops.GCN_EPI_RELU, DROPOUT), ("l2norm", D, ops.GCN_EPI_L2NORM, 0.0)):
        S, dY = (torch.randn(adj.n, d, generator=gen, device=dev) for _ in range(2))
        b = torch.randn(d, generator=gen, device=dev)
        Y, norm = ops._gcn_conv_fwd(adj, S, b, epi, p, 11)
        scale = 1.0 / (1.0 - p)

        def fused_fwd(S=S, b=b, epi=epi, p=p):
            return ops._gcn_conv_fwd(adj, S, b, epi, p, 11)

        def composed_fwd(S=S, b=b, epi=epi, p=p):
            return epilogue(ops.spmm_csr(adj.row_ptr, adj.col, adj.val, S), b, epi, p)

        def fused_bwd(dY=dY, Y=Y, norm=norm, epi=epi, p=p):
            G, db = ops._gcn_conv_prep(dY, Y, norm, epi, p, want_db=True)
            return ops._gcn_conv_fwd(adj_t, G, None, ops.GCN_EPI_NONE)[0], db

        def composed_bwd(dY=dY, Y=Y, norm=norm, epi=epi, scale=scale):
            if epi == ops.GCN_EPI_RELU:
                G = torch.where(Y > 0, dY * scale, torch.zeros((), device=dev))
            else:
                G = (dY - Y * (Y * dY).sum(dim=1, keepdim=True)) / norm.clamp_min(1e-12).view(-1, 1)
            return ops.spmm_csr(adj_t.row_ptr, adj_t.col, adj_t.val, G), G.sum(dim=0)

        fns.update({"fused_fwd_" + name: fused_fwd, "composed_fwd_" + name: composed_fwd,
                    "fused_bwd_" + name: fused_bwd, "composed_bwd_" + name: composed_bwd})
    return round_robin(fns, reps)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", required=True, choices=sorted(SHAPES))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    name = args.workload
    out_path = args.out or os.path.join(ROOT, "profiles", "gcrn_bench_%s.json" % name)
    if not torch.cuda.is_available():
        raise SystemExit("gcrn_bench measures on the GPU; no device found")
    from ctgcn_amd import GCRN
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    xs, adjs = window(name, dev)
    n, T = adjs[0].n, len(adjs)
    base_model = GCRN(n, 0, HID, D, dropout=DROPOUT, duration=T, rnn_type="GRU").to(dev)
    gen = torch.Generator(device=dev).manual_seed(1)
    C = torch.randn(T, n, D, generator=gen, device=dev)
    kinds = ("fused", "composed", "torch")
    models = {k: variant(base_model, k) for k in kinds}
    del base_model
    opts = {k: torch.optim.Adam(models[k].parameters(), lr=1e-3) for k in kinds}

    def epoch_of(k):
        def run():
            models[k].train()
            (models[k](xs, adjs) * C).sum().backward()
            opts[k].step()
            opts[k].zero_grad(set_to_none=True)
        return run

    def forward_of(k):
        def run():
            models[k].eval()
            with torch.no_grad():
                return models[k](xs, adjs)
        return run

    first = {k: forward_of(k)().clone() for k in kinds}
    top = float(first["torch"].abs().max())
    agreement = {k: float((first[k] - first["torch"]).abs().max()) / top for k in ("fused", "composed")}
    del first
    forward_ms, forward_range = round_robin({k: forward_of(k) for k in kinds}, REPS[name])
    epoch_ms, epoch_range = round_robin({k: epoch_of(k) for k in kinds}, REPS[name])
    del models, opts
    torch.cuda.empty_cache()
    nnz = [a.nnz for a in adjs]
    step_ms, step_range = gcn_step_ms(adjs[-1], REPS[name])
    res = {"workload": name, "device": torch.cuda.get_device_name(0),
           "shape": dict(SHAPES[name], hid_dim=HID, embed_dim=D, dropout=DROPOUT, features="identity", stored_entries=nnz),
           "reps": REPS[name], "warmup": 3, "rnn_type": "GRU",
           "epoch_ms": epoch_ms, "epoch_ms_min_max": epoch_range, "forward_ms": forward_ms, "forward_ms_min_max": forward_range,
           "eval_forward_max_diff_vs_torch": agreement,
           "epoch_speedup_fused_vs_composed": epoch_ms["composed"] / epoch_ms["fused"],
           "epoch_speedup_fused_vs_torch": epoch_ms["torch"] / epoch_ms["fused"],
           "forward_speedup_fused_vs_composed": forward_ms["composed"] / forward_ms["fused"],
           "forward_speedup_fused_vs_torch": forward_ms["torch"] / forward_ms["fused"],
           "gcn_step_ms_last_snapshot": step_ms, "gcn_step_ms_min_max": step_range,
           "gcn_step_bytes_last_snapshot": {"hid_%d" % HID: gcn_step_bytes(n, nnz[-1], HID), "embed_%d" % D: gcn_step_bytes(n, nnz[-1], D)}}
    os.makedirs(os.path.dirname(out_path), exist_ok=True)
    with open(out_path, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
