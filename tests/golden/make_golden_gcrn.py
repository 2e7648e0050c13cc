"""Golden data of the GCN / GCRN baselines: tests/golden/gcrn_uci.npz.  Runs only where the reference tree is; imports the reference's
baseline/gcn.py and baseline/gcrn.py in-process (behind an empty stand-in for torch_geometric, which gcn.py imports for its Tg*
variants and which need not be installed) and stores data only: expected outputs, gradients and losses in float64, and the
reference's own float32-vs-float64 error as the yardstick.

Setup: the first 3 UCI snapshots (n = 1899), row-normalised D^-1 (A + I) with the float32 values the reference's loader produces
(egcn_uci.npz: norm1_t*); identity features (dense formula features for gcn_dense); dropout 0.0 in train() mode; parameters from
conftest.seeded_parameters; surrogate loss sum_t sum(out_t * C_t); 3 Adam steps at lr 1e-3.  The smallest row norm F.normalize meets
is stored: no comparison sits on its 1e-12 clamp."""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
sys.modules.setdefault("torch_geometric", types.ModuleType("torch_geometric"))
import baseline.gcn as ref_gcn  # noqa: E402
import baseline.gcrn as ref_gcrn  # noqa: E402
import _gcrn_ref as R  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 1


def run_case(case, dtype, norms):
    model = R.build(case, ref_gcn.GCN, ref_gcrn.GCRN)
    seeded_parameters(model, SEED)
    model = model.to(dtype).train()
    if R.CASES[case][0] == "GCRN":
        for gcn in model.gcn_list:
            gcn.register_forward_hook(lambda m, a, out: norms.append(float(out.detach().norm(dim=1).min())))
    x, adj = R.features(case, dtype), R.adjacency(dtype)
    losses, (outs, grads) = R.adam_losses(model, lambda: model(x, adj), R.surrogate_weights(case, dtype))
    return losses, outs, grads


def main():
    d = {"seed": np.int64(SEED)}
    norms = []
    for case in R.CASES:
        losses, outs, grads = run_case(case, torch.float64, norms)
        losses32, outs32, grads32 = run_case(case, torch.float32, [])
        d[case + "_losses"] = np.asarray(losses, dtype=np.float64)
        d[case + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
        for t in range(R.T):
            put_tensor(d, "%s_out_t%d" % (case, t), outs[t])
        d[case + "_yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(R.T)])
        names = sorted(grads)
        d[case + "_keys"] = np.asarray(names)
        d[case + "_shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
        for k in names:
            put_tensor(d, "%s_grad_%s" % (case, k), grads[k])
        d[case + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
        print(case, "losses", losses, "yard out", d[case + "_yard_out"], "yard grad max", d[case + "_yard_grad"].max())
    d["min_row_norm"] = np.float64(min(norms))
    print("smallest row norm before F.normalize: %.4f" % min(norms))
    np.savez_compressed(os.path.join(OUT, "gcrn_uci.npz"), **d)
    print("wrote gcrn_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "gcrn_uci.npz")))


if __name__ == "__main__":
    main()
