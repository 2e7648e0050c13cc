"""Golden data of the GAT baseline: tests/golden/gat_uci.npz.  Runs only where the reference tree is; imports the reference's
baseline/gat.py in-process (behind an empty stand-in for torch_geometric, which it imports for its Tg* variant and which need not be
installed) and stores data only: expected outputs, gradients and losses in float64, and the reference's own float32-vs-float64 error
as the yardstick.

Setup (gcrn_uci.npz's): the first 3 UCI snapshots (n = 1899; 5 441 / 19 929 / 6 677 stored entries, rows of 1 to 199 entries, none
empty), the pattern of the row-normalised D^-1 (A + I) the reference's loader hands over; identity features (dense formula features
for gat_dense); dropout 0.0 in train() mode; parameters from conftest.seeded_parameters; surrogate loss sum_t sum(out_t * C_t); 3 Adam
steps at lr 1e-3.  The reference's layer makes a default-dtype torch.ones for its row sums, so each run is wrapped in
torch.set_default_dtype(dtype): as written it cannot run in float64."""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
sys.modules.setdefault("torch_geometric", types.ModuleType("torch_geometric"))
import baseline.gat as ref_gat  # noqa: E402
import _gat_ref as A  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 1


def run_case(case, dtype):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        model = A.build(case, ref_gat.GAT)
        seeded_parameters(model, SEED)
        model = model.to(dtype).train()
        x, adj = A.features(case, dtype), A.adjacency(dtype)
        losses, (outs, grads) = A.adam_losses(model, lambda: model(x, adj), A.surrogate_weights(case, dtype))
    finally:
        torch.set_default_dtype(before)
    return losses, outs, grads


def main():
    d = {"seed": np.int64(SEED)}
    for case in A.CASES:
        losses, outs, grads = run_case(case, torch.float64)
        losses32, outs32, grads32 = run_case(case, torch.float32)
        d[case + "_losses"] = np.asarray(losses, dtype=np.float64)
        d[case + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
        for t in range(A.T):
            put_tensor(d, "%s_out_t%d" % (case, t), outs[t])
        d[case + "_yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(A.T)])
        names = sorted(grads)
        d[case + "_keys"] = np.asarray(names)
        d[case + "_shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
        for k in names:
            put_tensor(d, "%s_grad_%s" % (case, k), grads[k])
        d[case + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
        print(case, "losses", losses, "yard out", d[case + "_yard_out"], "yard losses", d[case + "_yard_losses"], "yard grad",
              d[case + "_yard_grad"].min(), d[case + "_yard_grad"].max())
    np.savez_compressed(os.path.join(OUT, "gat_uci.npz"), **d)
    print("wrote gat_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "gat_uci.npz")))


if __name__ == "__main__":
    main()
