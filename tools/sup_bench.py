"""One supervised training epoch (ctgcn_amd.embedding.SupervisedEmbedding's train step: forward, classifier head, loss, backward, Adam)
with the fused head (ctgcn_supervised.hip) against fused=False, the same step with the head in stock torch ops (E[idx], Linear,
cross_entropy, index_put backward), on two shapes:

  air-like       an America-Air-like window (1 190 nodes, 10 snapshots, d = 128): CTGCN-C, S-node with every node labelled (4 classes)
                 and S-edge with every edge labelled (3 classes)
  synthetic-1m   config 5's last snapshot (synthetic 1 M nodes / 8 M edges via ctgcn_amd.synth.powerlaw_edges): CGCN-C on the one
                 snapshot, S-edge with every edge labelled (3 classes) and S-link-st-shaped scores over the same pairs

    python tools/sup_bench.py [--workload air-like|synthetic-1m|all] [--out profiles/supervised_bench.json]        (GPU)

Per case and path: ms per epoch (median of REPS calls after three warm-up calls), ms of the head alone (logits + loss + backward into dE on a detached
embedding) and peak device memory over what the inputs and the model hold.  The baseline is fused=False: stock torch ops on the same
model, what the library computed a supervised step with before the kernels existed.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

D = 128
REPS = {"air-like": 30, "synthetic-1m": 5}      # timed repetitions after 3 warm-up calls


def tertiles(key, k):
    order = np.lexsort((np.arange(len(key)), key))
    lab = np.empty(len(key), np.int64)
    lab[order] = (k * np.arange(len(key))) // len(key)
    return lab


def air_like(dev):
    import scipy.sparse as sp
    from ctgcn_amd import CTGCN
    from ctgcn_amd.helper import core_adj_from_scipy
    from ctgcn_amd.synth import dynamic_graph
    n, T = 1190, 10
    graphs = dynamic_graph(n, avg_deg=23, snapshots=T, seed=2)
    adjs = [core_adj_from_scipy(g, 10, dev)[0] for g in graphs]
    gen = torch.Generator().manual_seed(0)
    xs = [torch.randn(n, 48, generator=gen).to(dev) for _ in range(T)]
    node_idx, node_lab, edge_idx, edge_lab = [], [], [], []
    for g in graphs:
        a = sp.triu(sp.csr_matrix(g), 1).tocoo()
        deg = np.asarray(sp.csr_matrix(g).sum(1)).reshape(-1)
        node_idx.append(torch.arange(n, device=dev))
        node_lab.append(torch.from_numpy(tertiles(deg, 4)).to(dev))
        edge_idx.append(torch.from_numpy(np.stack([a.row, a.col]).astype(np.int64)).to(dev))
        edge_lab.append(torch.from_numpy(tertiles(deg[a.row] * deg[a.col], 3)).to(dev))
    model = CTGCN(48, 128, D, 1, 2, T, model_type="C", trans_activate_type="L").to(dev)
    return model, adjs, xs, {"S-node": (node_idx, node_lab, 4), "S-edge": (edge_idx, edge_lab, 3)}, dict(nodes=n, snapshots=T)


def synthetic_1m(dev):
    from ctgcn_amd import CGCN
    from ctgcn_amd.helper import core_adj_from_edge_rows
    from ctgcn_amd.synth import powerlaw_edges
    n, m = 1_000_000, 8_000_000
    u, v = powerlaw_edges(n, m, 1)
    adj = core_adj_from_edge_rows(u, v, np.ones(len(u), np.float32), n, 8, dev)[0]
    deg = np.bincount(np.concatenate([u, v]), minlength=n)
    gen = torch.Generator().manual_seed(0)
    xs = [torch.randn(n, 48, generator=gen).to(dev)]
    idx = [torch.from_numpy(np.stack([u, v]).astype(np.int64)).to(dev)]
    lab = [torch.from_numpy(tertiles(deg[u] * deg[v], 3)).to(dev)]
    link = [torch.from_numpy((np.arange(len(u)) % 2).astype(np.float32)).to(dev)]
    model = CGCN(48, 128, D, 1, 2, model_type="C", trans_activate_type="L").to(dev)
    return model, [adj], xs, {"S-edge": (idx, lab, 3), "S-link-st": (idx, link, 2)}, dict(nodes=n, snapshots=1)


def median_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        fn()
        ev[1].record()
        torch.cuda.synchronize()
        out.append(ev[0].elapsed_time(ev[1]))
    return float(np.median(out))


def run_case(model, adjs, xs, ltype, idx, lab, n_class, fused, reps):
    from ctgcn_amd import ClassificationLoss, EdgeClassifier, InnerProduct, MLPClassifier
    dev = xs[0].device
    T = len(xs)
    torch.manual_seed(1)
    if ltype == "S-node":
        classifier = MLPClassifier(D, D, n_class, 1, T).to(dev)
    elif ltype == "S-edge":
        classifier = EdgeClassifier(D, D, n_class, 1, T).to(dev)
    else:
        classifier = InnerProduct()
    for p in classifier.parameters():           # the reference's Adam does not hold the classifier: no gradient for it
        p.requires_grad_(False)
    loss_model = ClassificationLoss(n_class)
    loss_model.fused = classifier.fused = fused
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)

    def epoch():
        emb = model(xs, adjs)
        loss, _, _ = loss_model(classifier(emb, idx), lab)
        loss.backward()
        opt.step()
        model.zero_grad()
        return float(loss.detach())

    with torch.no_grad():
        emb0 = model(xs, adjs)
    emb0 = [e.detach().clone().requires_grad_(True) for e in emb0]

    def head():
        loss, _, _ = loss_model(classifier(emb0, idx), lab)
        loss.backward()
        for e in emb0:
            e.grad = None

    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    head_ms = median_ms(head, reps)
    head_peak = torch.cuda.max_memory_allocated() - base
    del emb0
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.time()
    first_loss = epoch()
    torch.cuda.synchronize()
    first_s = time.time() - t0
    epoch_ms = median_ms(epoch, reps)
    return dict(epoch_ms=epoch_ms, head_ms=head_ms, first_epoch_s=first_s, first_loss=first_loss,
                epoch_peak_mem_gib=(torch.cuda.max_memory_allocated() - base) / 2 ** 30, head_peak_mem_gib=head_peak / 2 ** 30)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["air-like", "synthetic-1m", "all"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "supervised_bench.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "d": D, "reps": REPS, "workloads": {}}
    for name, make in (("air-like", air_like), ("synthetic-1m", synthetic_1m)):
        if args.workload not in (name, "all"):
            continue
        torch.manual_seed(0)
        model, adjs, xs, cases, meta = make(dev)
        state = {k: v.detach().clone() for k, v in model.state_dict().items()}
        out = dict(meta, cases={})
        for ltype, (idx, lab, n_class) in cases.items():
            rec = {"items_per_snapshot": [int(i.shape[-1]) for i in idx], "classes": n_class}
            for tag, fused in (("fused", True), ("torch", False)):
                model.load_state_dict(state)
                rec[tag] = run_case(model, adjs, xs, ltype, idx, lab, n_class, fused, REPS[name])
                torch.cuda.empty_cache()
                print(name, ltype, tag, json.dumps(rec[tag]), flush=True)
            rec["epoch_speedup"] = rec["torch"]["epoch_ms"] / rec["fused"]["epoch_ms"]
            rec["head_speedup"] = rec["torch"]["head_ms"] / rec["fused"]["head_ms"]
            out["cases"][ltype] = rec
        res["workloads"][name] = out
        del model, adjs, xs, cases
        torch.cuda.empty_cache()
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
