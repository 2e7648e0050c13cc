"""Child of tests/test_gpu_kcore_shapes.py::test_forced_algorithms_give_the_same_integers: argv = mode, output .npz.

The library reads CTGCN_KCORE once per process, so the parent starts one fresh process per mode with the variable set and compares
what this one writes with the closed forms.  Nothing is checked here."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(mode, out):
    import _kcore_ref as R
    from ctgcn_amd import ops
    assert os.environ.get("CTGCN_KCORE") == mode
    d = torch.device("cuda:0")

    def run(csr, cap=-1):
        core, mx = ops.kcore(torch.from_numpy(csr.indptr.astype(np.int32)).to(d), torch.from_numpy(csr.indices.astype(np.int32)).to(d),
                             level_cap=cap)
        return core.cpu().numpy(), mx

    res = {}
    caps = R.caps_graph()[0]
    if mode == "peel":
        res["caps_core"], res["caps_max"] = run(caps)
        res["path_core"], res["path_max"] = run(R.path(50001)[0])
    else:
        for cap in (1, 2, 16):
            res["caps_core_%d" % cap], res["caps_max_%d" % cap] = run(caps, cap)
    np.savez(out, **res)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
