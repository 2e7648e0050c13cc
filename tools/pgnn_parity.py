"""Where the P-GNN gradients' error comes from, on the fixture case pgnn_l2 (tests/golden/pgnn_uci.npz: 3 UCI snapshots, the recorded
anchor tensors, 24 -> 32 / 32 / 128, dropout 0): per parameter gradient and per output the largest deviation from the float64 mirror
over the tensor's largest magnitude, for

  fused            ctgcn_amd.baseline.PGNN as shipped (ops.pgnn_conv; long sums and the products in front of the pass in fp64)
  torch_gpu        the mirror (tests/_pgnn_ref.PgnnMirror: the reference's materialising form) in float32 stock torch ops on the GPU
  torch_gpu_fp64_products   the same with every Linear's product formed in fp64 and rounded to fp32 once
  torch_cpu        the mirror in float32 on the CPU
  reference_cpu    the reference's own float32-vs-float64 error, as recorded in the fixture (the tests' yardstick)

    python tools/pgnn_parity.py [--out profiles/pgnn_parity_errors.json]     (GPU)
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _egcn_ref as E  # noqa: E402
import _pgnn_ref as P  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

CASE = "pgnn_l2"


def run(cls, dtype, dev, dm, da, seed):
    model = P.build(CASE, cls)
    seeded_parameters(model, seed)
    model = model.to(dtype).to(dev).train()
    outs = list(model(P.features(dtype, dev), [d.to(dev) for d in dm], [a.to(dev) for a in da]))
    E.surrogate(outs, P.surrogate_weights(dm[0].shape[1], dtype, dev)).backward()
    grads = {k: p.grad.detach().double().cpu() for k, p in model.named_parameters() if p.grad is not None}
    return [o.detach().double().cpu() for o in outs], grads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pgnn_parity_errors.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pgnn_parity measures on the GPU; no device found")
    import ctgcn_amd
    dev = "cuda:0"
    g = P.fixture()
    seed = int(g["seed"])
    dm, da = P.anchor_tensors(g, dev)
    runs = {"fused": run(ctgcn_amd.PGNN, torch.float32, dev, dm, da, seed),
            "torch_gpu": run(P.PgnnMirror, torch.float32, dev, dm, da, seed),
            "torch_cpu": run(P.PgnnMirror, torch.float32, "cpu", dm, da, seed)}
    plain = F.linear

    def exact_linear(x, w, b=None):
        return plain(x.double(), w.double(), None if b is None else b.double()).to(x.dtype)

    F.linear = exact_linear                            # nn.Linear looks the function up at call time
    try:
        runs["torch_gpu_fp64_products"] = run(P.PgnnMirror, torch.float32, dev, dm, da, seed)
    finally:
        F.linear = plain
    outs64, grads64 = run(P.PgnnMirror, torch.float64, "cpu", dm, da, seed)
    res = {"case": CASE, "device": torch.cuda.get_device_name(0), "gradients": {}, "outputs": {},
           "what": "largest |x - float64 mirror| over the tensor's largest magnitude"}
    yard = dict(zip((str(k) for k in g[CASE + "_keys"]), (float(v) for v in g[CASE + "_yard_grad"])))
    for k in sorted(grads64):
        top = float(grads64[k].abs().max())
        res["gradients"][k] = {name: float((r[1][k] - grads64[k]).abs().max()) / top for name, r in runs.items()}
        res["gradients"][k]["reference_cpu"] = yard[k]
    for t in range(P.T):
        top = float(outs64[t].abs().max())
        res["outputs"]["t%d" % t] = {name: float((r[0][t] - outs64[t]).abs().max()) / top for name, r in runs.items()}
        res["outputs"]["t%d" % t]["reference_cpu"] = float(g[CASE + "_yard_out"][t])
    res["largest_gradient_error"] = {name: max(v[name] for v in res["gradients"].values()) for name in list(runs) + ["reference_cpu"]}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res["largest_gradient_error"]))


if __name__ == "__main__":
    main()
