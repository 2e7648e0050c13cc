"""TIMERS end to end on the six golden snapshots (tests/golden/timers_synth.npz: what the reference's functions gave), for Update=True
and Update=False, and timers_embedding() on a three-file folder.

Allowance: Loss_store and Loss_bound within relative 1000·tol/g_min of the reference's, the picked entries of U_cur V_curᵀ within the
same factor times σ₁ (g_min: the golden's smallest relative gap among the K + 1 leading |λ|; tol = 1e-12 gives 6.5e-7 here).  The factor
1000 allows TRIP to amplify an eigenvector error of tol/gap over five steps.
Largest deviations seen on an MI355X: see MEASURED below."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest

import _timers_ref as T
from conftest import load_golden

pytestmark = pytest.mark.gpu
TM = importlib.import_module("ctgcn_amd.baseline.timers")

# Largest deviations from the reference observed on an MI355X (Update=True / Update=False), far inside the allowance of 6.5e-7:
MEASURED = ("loss 4.7e-13 / 2.3e-15 relative, bound 2.1e-16 / 4.3e-16 relative, reconstruction entries 1.0e-13 / 7.4e-14 of sigma_1; "
            "solver iterations: 157 and 152 for the two decompositions, 2 to 50 for the bounds")


@pytest.mark.parametrize("update", [True, False])
def test_timers_reproduces_the_reference_run(update):
    g = load_golden("timers_synth.npz")
    m = "u_" if update else "f_"
    K = int(g["K"])
    snaps = [T.get_csr(g, "snap%d" % i) for i in range(T.STEPS + 1)]
    model = TM.TIMERS(K, Theta=float(g["theta"]), Update=update, tol=T.TOL).fit_first(snaps[0])
    allow = 1000 * T.TOL / float(g["g_min"])
    rc = g[m + "pick_rc"]
    worst = dict(loss=0.0, bound=0.0, pick=0.0)

    def check(i):
        emb = model.embedding().cpu().numpy()
        assert emb.shape == (snaps[0].shape[0], 2 * K) and emb.dtype == np.float64
        Uc, Vc = emb[:, :K], emb[:, K:]
        got = (Uc[rc[i, :, 0]] * Vc[rc[i, :, 1]]).sum(axis=1)
        sigma1 = float(g[m + "sigma"][i].max())
        worst["pick"] = max(worst["pick"], float(np.abs(got - g[m + "pick"][i]).max()) / sigma1)
        assert (np.abs(got - g[m + "pick"][i]) <= allow * sigma1).all(), i
        assert (np.abs(model.S.cpu().numpy() - g[m + "sigma"][i]) <= allow * sigma1).all(), i

    check(0)
    decisions = [False]
    for i in range(1, T.STEPS + 1):
        decisions.append(model.step(T.delta(snaps[i - 1], snaps[i])))
        tested_loss, tested_bound = model.tested[-1]
        for key, got, want in (("loss", tested_loss, g[m + "tested_loss"][i]), ("bound", tested_bound, g[m + "tested_bound"][i]),
                               ("loss", model.Loss_store[i], g[m + "loss"][i]), ("bound", model.Loss_bound[i], g[m + "bound"][i])):
            worst[key] = max(worst[key], abs(got - want) / abs(want))
        check(i)
    print("  TIMERS Update=%s: largest deviations: loss %.2e, bound %.2e (relative), reconstruction %.2e of sigma_1; allowance %.2e; "
          "iterations %s" % (update, worst["loss"], worst["bound"], worst["pick"], allow, model.iterations))
    assert decisions == [bool(r) for r in g[m + "restart"]]
    assert model.Run_t == [i for i, r in enumerate(g[m + "restart"]) if r]
    assert worst["loss"] <= allow and worst["bound"] <= allow
    assert abs(model.Loss_store[0] - g[m + "loss"][0]) <= allow * g[m + "loss"][0] and model.Loss_bound[0] == model.Loss_store[0]


def test_timers_embedding_writes_the_reference_layout(tmp_path):
    g = load_golden("timers_synth.npz")
    n, K = int(g["tiny_n"]), int(g["tiny_K"])
    names = ["node%03d" % i for i in range(n)]
    os.makedirs(tmp_path / "1.format")
    with open(tmp_path / "nodes_set.csv", "w") as fh:
        fh.write("\n".join(names) + "\n")
    files = ["2020-01.csv", "2020-02.csv", "2020-03.csv"]
    snaps = [T.get_csr(g, "tiny_snap%d" % i) for i in range(3)]
    for f, S in zip(files, snaps):
        coo = S.tocoo()
        keep = coo.row < coo.col
        with open(tmp_path / "1.format" / f, "w") as fh:
            fh.write("from_id\tto_id\tweight\n")
            for r, c, w in zip(coo.row[keep], coo.col[keep], coo.data[keep]):
                fh.write("%s\t%s\t%g\n" % (names[r], names[c], w))
    args = dict(base_path=str(tmp_path), origin_folder="1.format", embed_folder="2.embedding/timers", node_file="nodes_set.csv", file_sep="\t",
                embed_dim=2 * K, theta=float(g["tiny_theta"]))
    import ctgcn_amd
    model = ctgcn_amd.timers_embedding(args)
    out = tmp_path / "2.embedding" / "timers"
    assert sorted(os.listdir(out)) == files
    allow = 1000 * T.TOL / float(g["tiny_g_min"])
    for i, f in enumerate(files):
        df = pd.read_csv(out / f, sep="\t", index_col=0)
        assert list(df.index) == names and list(df.columns) == [str(j) for j in range(2 * K)] and df.shape == (n, 2 * K)
        vals = df.values
        Uc, Vc = vals[:, :K], vals[:, K:]
        rc = g["tiny_u_pick_rc"][i]
        got = (Uc[rc[:, 0]] * Vc[rc[:, 1]]).sum(axis=1)
        sigma1 = float(g["tiny_u_sigma"][i].max())
        # float32 factors: each product moves by 2·2⁻²⁴ relative, and Σ_j |U_cur[r, j] V_cur[c, j]| <= sigma_1 (Cauchy–Schwarz on unit columns)
        assert (np.abs(got - g["tiny_u_pick"][i]) <= (allow + 4 * 2.0 ** -24) * sigma1).all(), f
    last = pd.read_csv(out / files[-1], sep="\t", index_col=0).values
    # float32 values, as every method's files here: the text reads back to exactly the float32 embedding
    assert np.array_equal(last.astype(np.float32), model.embedding().cpu().numpy().astype(np.float32))
    assert [bool(r) for r in g["tiny_u_restart"][:3]] == [False] + [i in model.Run_t for i in (1, 2)]
