"""Golden data of the DynGEM and DynAE baselines: tests/golden/dyngem_uci.npz.  Runs only where the reference tree is; imports the
reference's baseline/dynGEM.py and baseline/dynAE.py in-process and stores data only: the drawn batches as node ids and values,
expected losses, outputs and gradients in float64, and the reference's own float32-vs-float64 error as the yardstick of each.

Setup (tests/_dyngem_ref.py holds the constants): UCI snapshots with entry (i, j) given the weight 1 + (i + j) mod 3, because UCI's
stored weights are all 1 and would hide a confusion of weight, count and degree.
  DynGEM  snapshot 1 (n = 1899), n_units [24, 16], output_dim 8, alpha 0.5, beta 10, nu1 = nu2 = 1e-4, a batch of 64 drawn entries.
  DynAE   snapshots 0-2, look_back 2, the same widths, beta 5, nu1 = nu2 = 1e-4, 64 records.
Both: the reference's own generator draws the batch (np.random.seed(seed) before its shuffle) and builds the dense tensors; the batch
is stored as node ids and values, not as positions in sp.find's order; parameters from conftest.seeded_parameters; the same batch for
3 Adam steps at lr 1e-3.

Seed condition: the first seed for which, in the float64 run of both models, every Linear has between 20 % and 80 % of its outputs
positive at step 0 (a dead ReLU stack would pass any comparison), and at least a quarter of DynAE's 64 records have a stored target
entry.  The fractions are stored."""
import os
import sys

import numpy as np
import scipy.sparse as sp
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
import baseline.dynAE as ref_dynae  # noqa: E402
import baseline.dynGEM as ref_dyngem  # noqa: E402
import _dyngem_ref as D  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

NODES = list(range(D.N))


class Active(object):
    """fraction of positive outputs of every Linear at the first forward"""

    def __init__(self, model):
        self.frac = {}
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.Linear):
                m.register_forward_hook(self.hook(name))

    def hook(self, name):
        def fn(module, args, output):
            self.frac.setdefault(name, float((output > 0).double().mean()))
        return fn


def draw_dyngem(seed):
    """the reference generator's first batch and the node ids and values it drew"""
    graph = D.dyngem_window()[0].tolil()
    gen = ref_dyngem.DynGEMBatchGenerator(NODES, D.BATCH, D.DYNGEM["beta"], shuffle=True, has_cuda=False)
    np.random.seed(seed)
    [xi, xj], [yi, yj, value] = next(gen.generate(graph))
    rows, cols, values = sp.find(graph)
    np.random.seed(seed)
    order = np.arange(rows.shape[0])
    np.random.shuffle(order)
    pick = order[:D.BATCH]
    i, j, w = rows[pick].astype(np.int64), cols[pick].astype(np.int64), values[pick].astype(np.float64)
    dense = graph.toarray()
    assert np.array_equal(xi.numpy(), dense[i].astype(np.float32)) and np.array_equal(xj.numpy(), dense[j].astype(np.float32))
    assert np.array_equal(value.numpy().reshape(-1), w.astype(np.float32))
    return (xi, xj, yi, yj, value), (i, j, w)


def draw_dynae(seed):
    graphs = [m.tolil() for m in D.dynae_window()]
    gen = ref_dynae.BatchGenerator(NODES, D.BATCH, D.LOOK_BACK, D.DYNAE["beta"], shuffle=True, has_cuda=False)
    np.random.seed(seed)
    x_pre, x_cur, y = next(gen.generate(graphs))
    np.random.seed(seed)
    order = np.arange(D.N * (len(graphs) - D.LOOK_BACK))
    np.random.shuffle(order)
    rec = order[:D.BATCH]
    graph, node = (rec // D.N).astype(np.int64), (rec % D.N).astype(np.int64)
    for s in range(D.LOOK_BACK):
        assert np.array_equal(x_pre[:, s].numpy(), np.stack([graphs[g + s][v].toarray().reshape(-1) for g, v in zip(graph, node)]).astype(np.float32))
    return (x_pre.reshape(D.BATCH, -1), x_cur, y), (graph, node)


def run_dyngem(seed, dtype, tensors):
    model = ref_dyngem.DynGEM(input_dim=D.N, output_dim=D.OUT, n_units=D.UNITS, bias=True)
    seeded_parameters(model, seed)
    model = model.to(dtype)
    watch = Active(model)
    loss_fn = ref_dyngem.DynGEMLoss(D.DYNGEM["alpha"], D.DYNGEM["beta"], D.DYNGEM["nu1"], D.DYNGEM["nu2"])
    xi, xj, yi, yj, value = (t.to(dtype) for t in tensors)

    def forward_loss():
        hx_i, xi_pred = model(xi)
        hx_j, xj_pred = model(xj)
        return loss_fn(model, [xi_pred, xi, yi, xj_pred, xj, yj, hx_i, hx_j, value]), hx_i, xi_pred

    return D.adam_run(model, forward_loss), watch.frac


def run_dynae(seed, dtype, tensors):
    model = ref_dynae.DynAE(input_dim=D.N, output_dim=D.OUT, look_back=D.LOOK_BACK, n_units=D.UNITS, bias=True)
    seeded_parameters(model, seed)
    model = model.to(dtype)
    watch = Active(model)
    loss_fn = ref_dynae.DynGraph2VecLoss(D.DYNAE["beta"], D.DYNAE["nu1"], D.DYNAE["nu2"])
    x_pre, x_cur, y = (t.to(dtype) for t in tensors)

    def forward_loss():
        hx, pred = model(x_pre)
        return loss_fn(model, [pred, x_cur, y]), hx, pred

    return D.adam_run(model, forward_loss), watch.frac


def store(d, prefix, run64, run32, frac):
    (losses, (hx, pred, grads)), (losses32, (hx32, pred32, grads32)) = run64, run32
    d[prefix + "_losses"] = np.asarray(losses, dtype=np.float64)
    d[prefix + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
    put_tensor(d, prefix + "_hx", hx)
    put_tensor(d, prefix + "_pred", pred)
    d[prefix + "_yard_hx"], d[prefix + "_yard_pred"] = np.float64(rel_err(hx32, hx)), np.float64(rel_err(pred32, pred))
    names = sorted(grads)
    d[prefix + "_keys"] = np.asarray(names)
    d[prefix + "_shapes"] = np.asarray([",".join(str(s) for s in grads[k].shape) for k in names])
    for k in names:
        put_tensor(d, "%s_grad_%s" % (prefix, k), grads[k])
    d[prefix + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
    d[prefix + "_active_layers"] = np.asarray(sorted(frac))
    d[prefix + "_active"] = np.asarray([frac[k] for k in sorted(frac)])
    print(prefix, "losses", losses, "yard losses", d[prefix + "_yard_losses"], "yard hx", d[prefix + "_yard_hx"], "yard pred",
          d[prefix + "_yard_pred"], "yard grad", d[prefix + "_yard_grad"].min(), d[prefix + "_yard_grad"].max(), "active", d[prefix + "_active"])


def main():
    for seed in range(1, 200):
        gem_tensors, (i, j, w) = draw_dyngem(seed)
        ae_tensors, (graph, node) = draw_dynae(seed)
        stored_targets = int((ae_tensors[1] != 0).any(dim=1).sum())
        gem64, gem_frac = run_dyngem(seed, torch.float64, gem_tensors)
        ae64, ae_frac = run_dynae(seed, torch.float64, ae_tensors)
        fracs = list(gem_frac.values()) + list(ae_frac.values())
        if min(fracs) >= 0.2 and max(fracs) <= 0.8 and stored_targets >= D.BATCH // 4:
            break
        print("seed %d: active fractions %.2f .. %.2f, %d records with a stored target" % (seed, min(fracs), max(fracs), stored_targets))
    else:
        raise SystemExit("no seed met the condition")
    assert len(gem_frac) == 6 and len(ae_frac) == 6
    d = {"seed": np.int64(seed), "dyngem_i": i, "dyngem_j": j, "dyngem_w": w, "dynae_graph": graph, "dynae_node": node,
         "dynae_stored_targets": np.int64(stored_targets)}
    store(d, "dyngem", gem64, run_dyngem(seed, torch.float32, gem_tensors)[0], gem_frac)
    store(d, "dynae", ae64, run_dynae(seed, torch.float32, ae_tensors)[0], ae_frac)
    np.savez_compressed(os.path.join(OUT, "dyngem_uci.npz"), **d)
    print("seed %d; wrote dyngem_uci.npz, %d bytes" % (seed, os.path.getsize(os.path.join(OUT, "dyngem_uci.npz"))))


if __name__ == "__main__":
    main()
