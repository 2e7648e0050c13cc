"""Golden data of the P-GNN baseline: tests/golden/pgnn_uci.npz.  Runs only where the reference tree is; imports the reference's
baseline/pgnn.py in-process (behind an empty stand-in for torch_geometric, which it imports by name alone) and stores data only: the
anchor sets, the reference's dist_max / dist_argmax, expected outputs, gradients and losses in float64, the reference's own
float32-vs-float64 error as the yardstick, and the parameters whose gradient the reference leaves None.

Setup (gin_sage_uci.npz's): the first 3 UCI snapshots (n = 1899) as the pattern of the raw symmetric adjacency; anchor sets from the
reference's get_random_anchorset(n, c=1) under np.random.seed(ANCHOR_SEED); its precompute_dist_data (networkx all-pairs BFS, dense
[N, N]) and get_dist_max for cutoffs -1 and 2, stored as int8 levels (dist_max = float32(1) / float32(level + 1), checked bit for bit
here; -1 unreached) and int32 positions (those of cutoff 2 as their exclusive or with the exact run's, see below).  Model cases (_pgnn_ref.CASES) on the exact distances: dense formula features, dropout 0.0
in train() mode, parameters from conftest.seeded_parameters, surrogate loss sum_t sum(out_t * C_t), 3 Adam steps at lr 1e-3.  Both
precisions are fed the same float32 dist_max values."""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
sys.modules.setdefault("torch_geometric", types.ModuleType("torch_geometric"))
import baseline.pgnn as ref_pgnn  # noqa: E402
import _pgnn_ref as P  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 1
ANCHOR_SEED = 5


def run_case(case, dtype, dists_max, dists_argmax):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = P.build(case, ref_pgnn.PGNN)
        seeded_parameters(model, SEED)
        model = model.to(dtype).train()
        x = P.features(dtype)
        dm = [d.to(dtype) for d in dists_max]
        width = dm[0].shape[1]
        losses, (outs, grads) = P.adam_losses(model, lambda: model(x, dm, dists_argmax), P.surrogate_weights(width, dtype))
    finally:
        torch.set_default_dtype(before)
    return losses, outs, grads, {k: tuple(v.shape) for k, v in model.state_dict().items()}


def main():
    d = {"seed": np.int64(SEED), "anchor_seed": np.int64(ANCHOR_SEED)}
    np.random.seed(ANCHOR_SEED)
    sets = ref_pgnn.get_random_anchorset(P.N, c=1)
    d["anchor_offsets"] = np.concatenate(([0], np.cumsum([len(s) for s in sets]))).astype(np.int32)
    d["anchor_members"] = np.concatenate(sets).astype(np.int32)
    edges = []
    for t in range(P.T):
        coo = P.G.raw_csr(t).tocoo()
        edges.append(torch.from_numpy(np.vstack((coo.row, coo.col)).astype(np.int64)))
    exact = None
    for cutoff in P.CUTOFFS:
        dense = ref_pgnn.precompute_dist_data(edges, P.N, cutoff)
        dms, das = ref_pgnn.get_dist_max(sets, dense, "cpu")
        tag = "exact" if cutoff <= 0 else "cut%d" % cutoff
        for t in range(P.T):
            dm = dms[t].numpy()
            assert dm.dtype == np.float32
            level = np.where(dm > 0, np.rint(1.0 / np.where(dm > 0, dm, 1.0)) - 1, -1).astype(np.int32)
            assert level.max() < 127
            again = np.where(level >= 0, np.float32(1) / (level + 1).astype(np.float32), np.float32(0)).astype(np.float32)
            assert np.array_equal(again.view(np.uint32), dm.view(np.uint32)), "dist_max is not float32(1) / float32(level + 1)"
            d["level_%s_t%d" % (tag, t)] = level.astype(np.int8)
            pos = das[t].numpy().astype(np.int32)
            if cutoff <= 0:
                d["pos_exact_t%d" % t] = pos
            else:
                # a cutoff hides anchors, it does not change which one is closest: stored as the exclusive or with the exact run's
                # positions where this run reaches (all zeros, which compress to nothing; any deviation would be kept bit for bit)
                d["posxor_%s_t%d" % (tag, t)] = pos ^ np.where(level >= 0, d["pos_exact_t%d" % t], 0).astype(np.int32)
            print(tag, t, "levels up to", level.max(), "unreached", int((level < 0).sum()), "of", level.size)
        if cutoff <= 0:
            exact = (dms, das)
    for case in P.CASES:
        losses, outs, grads, shapes = run_case(case, torch.float64, *exact)
        losses32, outs32, grads32, _ = run_case(case, torch.float32, *exact)
        d[case + "_losses"] = np.asarray(losses, dtype=np.float64)
        d[case + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
        for t in range(P.T):
            put_tensor(d, "%s_out_t%d" % (case, t), outs[t])
        d[case + "_yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(P.T)])
        names = sorted(k for k in grads if grads[k] is not None)
        none = sorted(k for k in grads if grads[k] is None)
        assert none == sorted(k for k in grads32 if grads32[k] is None)
        d[case + "_keys"] = np.asarray(names)
        d[case + "_none_keys"] = np.asarray(none if none else [""])[:len(none)]
        for k in names:
            put_tensor(d, "%s_grad_%s" % (case, k), grads[k])
        d[case + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
        state = sorted(shapes)
        d[case + "_state_keys"] = np.asarray(state)
        d[case + "_state_shapes"] = np.asarray([",".join(str(s) for s in shapes[k]) for k in state])
        print(case, "losses", losses, "yard out", d[case + "_yard_out"], "yard losses", d[case + "_yard_losses"], "yard grad",
              d[case + "_yard_grad"].min(), d[case + "_yard_grad"].max(), "none", none)
    np.savez_compressed(os.path.join(OUT, "pgnn_uci.npz"), **d)
    print("wrote pgnn_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "pgnn_uci.npz")))


if __name__ == "__main__":
    main()
