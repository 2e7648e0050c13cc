"""Golden data of the GIN and GraphSAGE baselines: tests/golden/gin_sage_uci.npz.  Runs only where the reference tree is; imports the
reference's baseline/gin.py and baseline/sage.py in-process (behind an empty stand-in for torch_geometric, which they import for their
Tg* variants and which need not be installed) and stores data only: expected outputs, gradients, losses and BatchNorm running buffers
in float64, and the reference's own float32-vs-float64 error as the yardstick.

Setup (gat_uci.npz's): the first 3 UCI snapshots (n = 1899) with the raw adjacency the reference's loader hands these two models
(get_date_adj_list(normalize=False)); identity features (dense formula features for gin_dense); dropout 0.0 in train() mode; parameters
from conftest.seeded_parameters; surrogate loss sum_t sum(out_t * C_t); 3 Adam steps at lr 1e-3.  The reference makes default-dtype
torch.ones (GIN's unit diagonal and degrees, SAGE's mask), so each run is wrapped in torch.set_default_dtype(dtype)."""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
sys.modules.setdefault("torch_geometric", types.ModuleType("torch_geometric"))
import baseline.gin as ref_gin  # noqa: E402
import baseline.sage as ref_sage  # noqa: E402
import _gin_sage_ref as G  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 1


def run_case(case, dtype):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = G.build(case, ref_gin.GIN, ref_sage.SAGE)
        seeded_parameters(model, SEED)
        model = model.to(dtype).train()
        x, adj = G.features(case, dtype), G.adjacency(dtype)
        losses, (outs, grads) = G.adam_losses(model, lambda: model(x, adj), G.surrogate_weights(dtype))
        bufs = G.buffers(model)
    finally:
        torch.set_default_dtype(before)
    return losses, outs, grads, bufs, {k: tuple(v.shape) for k, v in model.state_dict().items()}


def main():
    d = {"seed": np.int64(SEED)}
    for case in G.CASES:
        losses, outs, grads, bufs, shapes = run_case(case, torch.float64)
        losses32, outs32, grads32, bufs32, _ = run_case(case, torch.float32)
        d[case + "_losses"] = np.asarray(losses, dtype=np.float64)
        d[case + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
        for t in range(G.T):
            put_tensor(d, "%s_out_t%d" % (case, t), outs[t])
        d[case + "_yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(G.T)])
        names = sorted(grads)
        d[case + "_keys"] = np.asarray(names)
        d[case + "_shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
        for k in names:
            put_tensor(d, "%s_grad_%s" % (case, k), grads[k])
        d[case + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
        state = sorted(shapes)
        d[case + "_state_keys"] = np.asarray(state)
        d[case + "_state_shapes"] = np.asarray([",".join(str(s) for s in shapes[k]) for k in state])
        bnames = sorted(bufs)
        d[case + "_buffer_keys"] = np.asarray(bnames if bnames else [""])[:len(bnames)]
        for k in bnames:
            d["%s_buffer_%s" % (case, k)] = bufs[k].double().numpy()
        d[case + "_yard_buffer"] = np.asarray([rel_err(bufs32[k], bufs[k]) for k in bnames], dtype=np.float64)
        print(case, "losses", losses, "yard out", d[case + "_yard_out"], "yard losses", d[case + "_yard_losses"], "yard grad",
              d[case + "_yard_grad"].min(), d[case + "_yard_grad"].max(), "yard buffer", d[case + "_yard_buffer"].max(initial=0.0))
    np.savez_compressed(os.path.join(OUT, "gin_sage_uci.npz"), **d)
    print("wrote gin_sage_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "gin_sage_uci.npz")))


if __name__ == "__main__":
    main()
