"""Golden data of the VGRNN baseline: tests/golden/vgrnn_uci.npz.  Runs only where the reference tree is; imports the reference's
baseline/vgrnn.py and metrics.VAELoss in-process behind the stand-ins below for torch_scatter and torch_geometric.utils (neither need
be installed: scatter_add / mean / max become an index_add, add_self_loops returns (index, None)), and stores data only: expected
outputs, gradients and losses in float64, and the reference's own float32-vs-float64 error as the yardstick.

Setup (gcrn_uci.npz's): the first 3 UCI snapshots (n = 1899) as [2, E] index lists for the model and as weighted sparse tensors for the
loss; dense identity features; VGRNN(1899, 20, 16, 1); parameters from conftest.seeded_parameters; the reparameterisation noise pinned
by patching _reparameterized_sample to read _vgrnn_ref.noise (closed-form tensors, the same at every step); loss = VAELoss; 3 Adam
steps at lr 1e-3.  The reference makes default-dtype zeros for h, so each run is wrapped in torch.set_default_dtype(dtype)."""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)


def _scatter_add(src, index, dim=0, out=None, dim_size=None):
    assert dim == 0 and out is None
    return torch.zeros((dim_size,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device).index_add(0, index, src)


def _remove_self_loops(edge_index, edge_attr=None):
    keep = edge_index[0] != edge_index[1]
    return edge_index[:, keep], (None if edge_attr is None else edge_attr[keep])


def _add_self_loops(edge_index, num_nodes=None):
    loops = torch.arange(num_nodes, dtype=edge_index.dtype, device=edge_index.device)
    return torch.cat([edge_index, torch.stack((loops, loops))], dim=1), None


scatter = types.ModuleType("torch_scatter")
scatter.scatter_add = scatter.scatter_mean = scatter.scatter_max = _scatter_add        # only scatter_add is reached with conv_type 'GCN'
geometric, geometric_utils = types.ModuleType("torch_geometric"), types.ModuleType("torch_geometric.utils")
geometric_utils.remove_self_loops, geometric_utils.add_self_loops = _remove_self_loops, _add_self_loops
geometric.utils = geometric_utils
sys.modules["torch_scatter"], sys.modules["torch_geometric"], sys.modules["torch_geometric.utils"] = scatter, geometric, geometric_utils
import baseline.vgrnn as ref_vgrnn  # noqa: E402
import metrics as ref_metrics  # noqa: E402
import _vgrnn_ref as V  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

SEED = 1


def run(dtype):
    before = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    sample = ref_vgrnn.VGRNN._reparameterized_sample
    try:
        model = V.build(ref_vgrnn.VGRNN)
        seeded_parameters(model, SEED)
        model = model.to(dtype).train()
        x = [torch.eye(V.N, dtype=dtype) for _ in range(V.T)]
        edges, adj, noise = V.edge_lists(), V.target_adjacency(dtype), V.noise(dtype)
        loss_fn = ref_metrics.VAELoss()
        step = {"t": 0}

        def pinned(mean, std):
            eps = noise[step["t"] % V.T]
            step["t"] += 1
            return eps.mul(std).add_(mean)

        ref_vgrnn.VGRNN._reparameterized_sample = staticmethod(pinned)

        def forward_loss():
            emb, h, data = model(x, edges)
            return emb, h, loss_fn(data + [adj])

        losses, first = V.adam_run(model, forward_loss)
    finally:
        ref_vgrnn.VGRNN._reparameterized_sample = sample
        torch.set_default_dtype(before)
    return losses, first


def main():
    d = {"seed": np.int64(SEED)}
    losses, (outs, h, grads) = run(torch.float64)
    losses32, (outs32, h32, grads32) = run(torch.float32)
    d["losses"] = np.asarray(losses, dtype=np.float64)
    d["yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
    for t in range(V.T):
        put_tensor(d, "out_t%d" % t, outs[t])
    d["yard_out"] = np.asarray([rel_err(outs32[t], outs[t]) for t in range(V.T)])
    put_tensor(d, "h", h)
    d["yard_h"] = np.float64(rel_err(h32, h))
    names = sorted(grads)
    d["keys"] = np.asarray(names)
    d["shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
    for k in names:
        put_tensor(d, "grad_%s" % k, grads[k])
    d["yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
    print("losses", losses, "yard losses", d["yard_losses"], "yard out", d["yard_out"], "yard h", d["yard_h"], "yard grad",
          d["yard_grad"].min(), d["yard_grad"].max())
    np.savez_compressed(os.path.join(OUT, "vgrnn_uci.npz"), **d)
    print("wrote vgrnn_uci.npz, %d bytes" % os.path.getsize(os.path.join(OUT, "vgrnn_uci.npz")))


if __name__ == "__main__":
    main()
