"""Golden data of the DynRNN and DynAERNN baselines: tests/golden/dynrnn_uci.npz.  Runs only where the reference tree is; imports the
reference's baseline/dynRNN.py and baseline/dynAERNN.py (and the loss and generator of baseline/dynAE.py) in-process and stores data
only: the drawn batch as record ids, expected losses, outputs and gradients in float64, and the reference's own float32-vs-float64
error as the yardstick of each.

Setup (tests/_dynrnn_ref.py and tests/_dyngem_ref.py hold the constants): UCI snapshots 0-4 with entry (i, j) given the weight
1 + (i + j) mod 3, look_back 3, so every node has two training positions and a window has a step 0, a first recurrent step and a
general one.  DynRNN n_units [24, 16], DynAERNN ae_units [24, 16] and rnn_units [24], output_dim 8, beta 5, nu1 = nu2 = 1e-4, 64
records.  The reference's own generator draws the batch (np.random.seed(seed) before its shuffle) and builds the dense tensors;
parameters from conftest.seeded_parameters; the same batch for 3 Adam steps at lr 1e-3.  DynRNN's last decoder layer has hidden size
1899: its [7596, 1899] and [7596, 24] gradients, like every tensor of more than 6000 entries, are stored as 256 picked entries.

Seed condition: the first seed for which, in the float64 run of both models, at least a quarter of the 64 records have a stored
target entry, no LSTM layer has more than 1 % of its step-0 sigmoid outputs outside (0.01, 0.99) (a saturated gate passes no
gradient and would pass any comparison), and every Linear of DynAERNN has between 20 % and 80 % of its outputs positive at step 0.
The found values are stored."""
import os
import sys

import numpy as np
import torch

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
from make_golden_egcn import put_tensor, rel_err  # noqa: E402  (puts the reference tree and tests/ on sys.path)
from make_golden_dyngem import Active  # noqa: E402
import baseline.dynAE as ref_dynae  # noqa: E402
import baseline.dynAERNN as ref_dynaernn  # noqa: E402
import baseline.dynRNN as ref_dynrnn  # noqa: E402
import _dyngem_ref as D  # noqa: E402
import _dynrnn_ref as R  # noqa: E402
from conftest import seeded_parameters  # noqa: E402

NODES = list(range(R.N))


class Saturated(object):
    """per nn.LSTM, the fraction of its step-0 sigmoid outputs (gates i, f, o) outside (0.01, 0.99) at the first forward"""

    def __init__(self, model):
        self.frac = {}
        for name, m in model.named_modules():
            if isinstance(m, torch.nn.LSTM):
                m.register_forward_hook(self.hook(name))

    def hook(self, name):
        def fn(module, args, output):
            if name in self.frac:
                return
            with torch.no_grad():
                z = args[0][:, 0] @ module.weight_ih_l0.t() + module.bias_ih_l0 + module.bias_hh_l0     # h_{-1} = 0
                zi, zf, _, zo = z.chunk(4, dim=1)
                s = torch.sigmoid(torch.cat((zi, zf, zo), dim=1))
                self.frac[name] = float(((s <= 0.01) | (s >= 0.99)).double().mean())
        return fn


def draw(seed):
    """the reference generator's first batch and the records it drew"""
    graphs = [m.tolil() for m in R.window()]
    gen = ref_dynae.BatchGenerator(NODES, R.BATCH, R.LOOK_BACK, R.BETA, shuffle=True, has_cuda=False)
    np.random.seed(seed)
    x_pre, x_cur, y = next(gen.generate(graphs))
    np.random.seed(seed)
    order = np.arange(R.N * (len(graphs) - R.LOOK_BACK))
    np.random.shuffle(order)
    rec = order[:R.BATCH]
    graph, node = (rec // R.N).astype(np.int64), (rec % R.N).astype(np.int64)
    for s in range(R.LOOK_BACK):
        assert np.array_equal(x_pre[:, s].numpy(), np.stack([graphs[g + s][v].toarray().reshape(-1) for g, v in zip(graph, node)]).astype(np.float32))
    assert np.array_equal(x_cur.numpy(), np.stack([graphs[g + R.LOOK_BACK][v].toarray().reshape(-1) for g, v in zip(graph, node)]).astype(np.float32))
    return (x_pre, x_cur, y), (graph, node)


def run(method, seed, dtype, tensors):
    if method == "dynrnn":
        model = ref_dynrnn.DynRNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, n_units=R.UNITS, bias=True)
    else:
        model = ref_dynaernn.DynAERNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, ae_units=R.UNITS, rnn_units=R.RNN_UNITS, bias=True)
    seeded_parameters(model, seed)
    model = model.to(dtype)
    active, saturated = Active(model), Saturated(model)
    loss_fn = ref_dynae.DynGraph2VecLoss(R.BETA, R.NU1, R.NU2)
    x_pre, x_cur, y = (t.to(dtype) for t in tensors)

    def forward_loss():
        hx, pred = model(x_pre)
        return loss_fn(model, [pred, x_cur, y]), hx, pred

    result = D.adam_run(model, forward_loss)
    shapes = {k: tuple(v.shape) for k, v in model.state_dict().items()}
    return result, active.frac, saturated.frac, shapes


def store(d, prefix, run64, run32, shapes):
    (losses, (hx, pred, grads)), (losses32, (hx32, pred32, grads32)) = run64, run32
    d[prefix + "_losses"] = np.asarray(losses, dtype=np.float64)
    d[prefix + "_yard_losses"] = np.float64(max(abs(a - b) for a, b in zip(losses32, losses)) / max(abs(b) for b in losses))
    put_tensor(d, prefix + "_hx", hx)
    put_tensor(d, prefix + "_pred", pred)
    d[prefix + "_yard_hx"], d[prefix + "_yard_pred"] = np.float64(rel_err(hx32, hx)), np.float64(rel_err(pred32, pred))
    names = sorted(grads)
    assert names == sorted(shapes)
    d[prefix + "_keys"] = np.asarray(names)
    d[prefix + "_shapes"] = np.asarray([",".join(str(s) for s in shapes[k]) for k in names])
    for k in names:
        assert float(grads[k].abs().max()) > 0, k
        put_tensor(d, "%s_grad_%s" % (prefix, k), grads[k])
    d[prefix + "_yard_grad"] = np.asarray([rel_err(grads32[k], grads[k]) for k in names])
    print(prefix, "losses", losses, "yard losses", d[prefix + "_yard_losses"], "yard hx", d[prefix + "_yard_hx"], "yard pred",
          d[prefix + "_yard_pred"], "yard grad", d[prefix + "_yard_grad"].min(), d[prefix + "_yard_grad"].max())


def main():
    for seed in range(1, 200):
        tensors, (graph, node) = draw(seed)
        stored_targets = int((tensors[1] != 0).any(dim=1).sum())
        if stored_targets < R.BATCH // 4:
            print("seed %d: %d records with a stored target" % (seed, stored_targets))
            continue
        runs = {m: run(m, seed, torch.float64, tensors) for m in R.METHODS}
        sat = {m + "." + k: v for m in R.METHODS for k, v in runs[m][2].items()}
        act = runs["dynaernn"][1]
        if max(sat.values()) <= 0.01 and min(act.values()) >= 0.2 and max(act.values()) <= 0.8:
            break
        print("seed %d: saturated at most %.4f, active %.2f .. %.2f, %d records with a stored target"
              % (seed, max(sat.values()), min(act.values()), max(act.values()), stored_targets))
    else:
        raise SystemExit("no seed met the condition")
    assert len(sat) == 6 + 2 and len(act) == 3 * 3 + 3 and not runs["dynrnn"][1]
    d = {"seed": np.int64(seed), "graph": graph, "node": node, "stored_targets": np.int64(stored_targets),
         "saturated_layers": np.asarray(sorted(sat)), "saturated": np.asarray([sat[k] for k in sorted(sat)]),
         "active_layers": np.asarray(sorted(act)), "active": np.asarray([act[k] for k in sorted(act)])}
    for m in R.METHODS:
        store(d, m, runs[m][0], run(m, seed, torch.float32, tensors)[0], runs[m][3])
    np.savez_compressed(os.path.join(OUT, "dynrnn_uci.npz"), **d)
    print("seed %d; saturated %s; active %s; %d stored targets; wrote dynrnn_uci.npz, %d bytes"
          % (seed, d["saturated"], d["active"], stored_targets, os.path.getsize(os.path.join(OUT, "dynrnn_uci.npz"))))


if __name__ == "__main__":
    main()
