"""The observed errors of TgGCN, TgGAT, TgSAGE and TgGIN on the UCI fixture (tests/test_gpu_tg.py's setup: the first 3 snapshots' edge
lists, identity features, 32 / 16 / 8, dropout 0, 3 Adam steps): per output, per parameter gradient and for the losses the largest
deviation from the float64 stock-torch mirror (tests/_tg_ref.py) over the tensor's largest magnitude, for

  fused        ctgcn_amd.baseline.tg as shipped
  mirror_f32   the mirror in float32 on the CPU: the tests' yardstick (tolerance = max(4 x this, floor))

with the share of the tolerance the fused run uses (floors: 2e-6 outputs and losses, 1e-5 gradients).

    python tools/tg_parity.py [--out profiles/tg_parity_errors.json]     (GPU)
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import _tg_ref as G  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 20260
CONFIGS = [(2, True, None), (3, True, None), (3, True, 16), (2, False, None)]            # layer_num, feature_pre, long_threshold


def run(kind, layer_num, feature_pre, thr, which, dev):
    import ctgcn_amd
    from ctgcn_amd import ops
    model = G.build(kind, getattr(ctgcn_amd, kind), feature_pre=feature_pre, layer_num=layer_num)
    seeded_parameters(model, SEED)
    if which == "fused":
        model = model.to(dev).train()
        x, edges = G.identity_features(device=dev), [ops.TgGraph(G.uci_edges(t, dev), G.N, long_threshold=thr) for t in range(G.T)]
        weights = G.surrogate_weights(device=dev)
    else:
        dtype = torch.float64 if which == "f64" else torch.float32
        mirror = G.build(kind, None, feature_pre=feature_pre, layer_num=layer_num)
        mirror.load_state_dict(model.state_dict())
        model = mirror.to(dtype).train()
        x, edges, weights = G.identity_features(dtype), G.edge_lists(), G.surrogate_weights(dtype)
    losses, (outs, grads) = G.adam_losses(model, lambda: model(x, edges), weights)
    tensors = {"out_t%d" % t: o for t, o in enumerate(outs)}
    tensors.update({"grad " + k: v for k, v in grads.items()})
    tensors["losses"] = torch.tensor(losses, dtype=torch.float64)
    return {k: v.detach().double().cpu() for k, v in tensors.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tg_parity_errors.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tg_parity measures on the GPU; no device found")
    dev = "cuda:0"
    res = {"device": torch.cuda.get_device_name(0), "what": "largest |x - float64 mirror| over the tensor's largest magnitude", "cases": {}}
    worst = {}
    for kind in G.KINDS:
        for layer_num, feature_pre, thr in CONFIGS:
            ref = run(kind, layer_num, feature_pre, thr, "f64", dev)
            yard = run(kind, layer_num, feature_pre, thr, "f32", dev)
            got = run(kind, layer_num, feature_pre, thr, "fused", dev)
            case = {}
            for k in sorted(ref):
                top = float(ref[k].abs().max())
                floor = 1e-5 if k.startswith("grad") else 2e-6
                own, err = float((yard[k] - ref[k]).abs().max()) / top, float((got[k] - ref[k]).abs().max()) / top
                case[k] = {"fused": err, "mirror_f32": own, "share_of_tolerance": err / max(4 * own, floor)}
            label = "%s layers=%d feature_pre=%s long_threshold=%s" % (kind, layer_num, feature_pre, thr)
            res["cases"][label] = case
            worst[label] = max(v["share_of_tolerance"] for v in case.values())
    res["largest_share_of_tolerance"] = worst
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
    print(json.dumps(worst))


if __name__ == "__main__":
    main()
