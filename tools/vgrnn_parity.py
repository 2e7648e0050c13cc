"""How far ops.vae_nll (the VGRNN decoder loss without an [N, N] matrix, ctgcn_vgrnn.hip) is from the float64 mirror, next to the same
dense expression in stock fp32 torch ops on the same GPU: loss and gradient, as the largest deviation over the largest magnitude, on
the cases of tests/test_gpu_vgrnn.py (N around the 32-row tile, d around the accumulator widths, extreme logits, long rows).  The
tests allow the kernel 4 x the stock error with floors of 2e-6 (loss) and 1e-5 (gradient).

    python tools/vgrnn_parity.py [--out profiles/vgrnn_parity_errors.json]     (GPU)
"""
import argparse
import json
import os
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vgrnn_parity_errors.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vgrnn_parity measures on the GPU; no device found")
    import test_gpu_vgrnn as G
    res = {"device": torch.cuda.get_device_name(0), "cases": {},
           "what": "largest |x - float64 mirror| over the largest magnitude: kernel and stock fp32 torch on the same GPU"}
    with tempfile.TemporaryDirectory() as tmp:
        os.environ["CTGCN_PARITY_OUT"] = tmp
        for n in (1, G.TILE - 1, G.TILE, G.TILE + 1, 2 * G.TILE + 3, 1899):
            for d in (1, 3, 16, 128, 130):
                z, target = G.make_case(n, d)
                loss, grad, _ = G.kernel(z, target)
                G.held("n%d d%d" % (n, d), loss, grad, z, target)
        z, target = G.make_case(G.TILE + 9, 16)
        for case, zz in (("large", z * 40.0), ("zero", torch.zeros_like(z))):
            loss, grad, _ = G.kernel(zz, target)
            G.held("extreme " + case, loss, grad, zz, target)
        for f in sorted(os.listdir(tmp)):
            with open(os.path.join(tmp, f)) as fh:
                res["cases"][f[len("vgrnn_nll_"):-len(".json")]] = json.load(fh)
    res["largest"] = {k: max(c[k] for c in res["cases"].values()) for k in ("loss", "loss_stock_fp32", "grad", "grad_stock_fp32")}
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(res["largest"]))


if __name__ == "__main__":
    main()
