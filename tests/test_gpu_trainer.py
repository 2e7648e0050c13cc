"""UnsupervisedEmbedding (ctgcn_amd/embedding.py): one fused epoch against one epoch of the reference's per-batch loop with the same
torch seed and the same sample seeds — accumulated gradients, per-batch losses, exported CSVs, checkpoints."""
import filecmp
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _window(n, T, seed):
    from ctgcn_amd.helper import core_adj_from_scipy
    from ctgcn_amd.synth import dynamic_graph
    graphs = dynamic_graph(n, avg_deg=5, snapshots=T, seed=seed)
    adjs = [core_adj_from_scipy(g, 4, torch.device(DEV))[0] for g in graphs]
    return graphs, adjs


def _neg_loss(graphs, seed):
    """negative-sampling loss whose pair CSR is the snapshot graph itself and whose table is a random node list"""
    from ctgcn_amd.metrics import NegativeSamplingLoss
    from ctgcn_amd.walks import WalkPairs
    import scipy.sparse as sp
    rng = np.random.default_rng(seed)
    pairs, tables = [], []
    for g in graphs:
        g = sp.csr_matrix(g)
        pairs.append(WalkPairs(torch.from_numpy(g.indptr.astype(np.int32)).to(DEV), torch.from_numpy(g.indices.astype(np.int32)).to(DEV)))
        tables.append(rng.integers(0, g.shape[0], size=300).astype(np.int32))
    return NegativeSamplingLoss(pairs, tables, neg_num=6, Q=2.0, seed=seed)


def _folders(tmp_path, T):
    origin = tmp_path / "origin"
    origin.mkdir(exist_ok=True)
    for t in range(T):
        (origin / ("2020-0%d.csv" % (t + 1))).write_text("")
    return str(tmp_path)


def _build(kind, n, T, seed):
    from ctgcn_amd import CGCN, CTGCN, ReconstructionLoss
    graphs, adjs = _window(n, T, seed)
    if kind == "CTGCN-C":
        model = CTGCN(48, 500, 128, 1, 2, T, model_type="C", trans_activate_type="L")
    elif kind == "CTGCN-S":
        model = CTGCN(48, 96, 128, 2, 1, T, model_type="S", trans_activate_type="N")
    else:
        model = CGCN(48, 96, 128, 1, 2, model_type="C", trans_activate_type="L")
    loss = ReconstructionLoss() if kind.endswith("-S") else _neg_loss(graphs, seed)
    g = torch.Generator().manual_seed(seed)
    xs = [torch.randn(n, 48, generator=g).to(DEV) for _ in range(T)]
    return model, loss, adjs, xs


def _train(tmp_path, kind, fused, monkeypatch, n=1100, T=3, bs=256, seed=7, epoch=1, model_file="m.pt", load_model=False, model=None):
    from ctgcn_amd.embedding import UnsupervisedEmbedding
    torch.manual_seed(seed)                         # the same initial weights in every run
    m, loss, adjs, xs = _build(kind, n, T, seed)
    model = m if model is None else model
    grads = {}
    orig = torch.optim.Adam.step

    def step(opt, *a, **k):                        # the epoch's accumulated gradients, just before the one Adam step
        for i, grp in enumerate(opt.param_groups):
            for j, p in enumerate(grp["params"]):
                if p.grad is not None:
                    grads[(i, j)] = p.grad.detach().clone()
        return orig(opt, *a, **k)

    monkeypatch.setattr(torch.optim.Adam, "step", step)
    folder = "emb_%s_%s" % (kind, "fused" if fused else "batch")
    emb = UnsupervisedEmbedding(_folders(tmp_path, T), "origin", folder, ["node%d" % i for i in range(n)], model, loss, has_cuda=True)
    torch.manual_seed(123)                          # the epoch order: all_nodes[torch.randperm(N)]
    emb.learn_embedding(adjs, xs, epoch=epoch, batch_size=bs, lr=1e-3, model_file=model_file, load_model=load_model, fused=fused)
    monkeypatch.setattr(torch.optim.Adam, "step", orig)
    return emb, grads, os.path.join(str(tmp_path), folder)


@pytest.mark.parametrize("kind", ["CTGCN-C", "CTGCN-S", "CGCN-C"])
def test_fused_epoch_matches_per_batch_epoch(tmp_path, monkeypatch, kind):
    ef, gf, dir_f = _train(tmp_path, kind, True, monkeypatch, model_file="f.pt")
    eb, gb, dir_b = _train(tmp_path, kind, False, monkeypatch, model_file="b.pt")
    assert ef.sample_seed_base == eb.sample_seed_base or kind.endswith("-S")
    assert len(ef.last_epoch_losses) == len(eb.last_epoch_losses) == 5          # 1100 / 256: four full batches and a partial one
    lf, lb = np.array(ef.last_epoch_losses), np.array(eb.last_epoch_losses)
    assert np.all(np.abs(lf - lb) <= 1e-5 * np.abs(lb).max()), (lf, lb)
    assert set(gf) == set(gb) and len(gf) > 5
    for k in gb:
        scale = gb[k].abs().max().item()
        err = (gf[k] - gb[k]).abs().max().item()
        assert err <= 1e-4 * scale + 1e-9, "parameter %s: max|err| %.3e, max|grad| %.3e" % (k, err, scale)
    names = sorted(os.listdir(dir_f))
    assert names == sorted(os.listdir(dir_b)) and len(names) == 3 and names[0] == "2020-01.csv"
    for f in names:
        assert filecmp.cmp(os.path.join(dir_f, f), os.path.join(dir_b, f), shallow=False), f
    if kind == "CTGCN-S":                          # -S exports the structure list, the MLP outputs (width 128 here)
        row = open(os.path.join(dir_f, names[0])).readline().rstrip("\n").split("\t")
        assert len(row) == 129


def test_checkpoint_loads_strict_and_resumes(tmp_path, monkeypatch):
    from ctgcn_amd import CTGCN
    emb, _, _ = _train(tmp_path, "CTGCN-C", True, monkeypatch, model_file="ck.pt")
    path = os.path.join(str(tmp_path), "model", "ck.pt")
    sd = torch.load(path, map_location="cpu")
    fresh = CTGCN(48, 500, 128, 1, 2, 3, model_type="C", trans_activate_type="L")
    fresh.load_state_dict(sd, strict=True)
    trained = {k: v.detach().cpu() for k, v in emb.model.state_dict().items()}
    assert all(torch.equal(trained[k], v) for k, v in sd.items())
    # load_model=True: the run starts from the checkpoint (epoch=0 leaves it untouched and saves it again)
    other = CTGCN(48, 500, 128, 1, 2, 3, model_type="C", trans_activate_type="L")
    e2, _, _ = _train(tmp_path, "CTGCN-C", True, monkeypatch, epoch=0, model_file="ck.pt", load_model=True, model=other)
    assert all(torch.equal(v.detach().cpu(), sd[k]) for k, v in e2.model.state_dict().items())
    e3, g3, _ = _train(tmp_path, "CTGCN-C", True, monkeypatch, epoch=1, model_file="ck.pt", load_model=True,
                       model=CTGCN(48, 500, 128, 1, 2, 3, model_type="C", trans_activate_type="L"))
    assert g3 and not all(torch.equal(v.detach().cpu(), sd[k]) for k, v in e3.model.state_dict().items())


def test_has_cuda_false_raises(tmp_path):
    from ctgcn_amd import CTGCN, ReconstructionLoss
    from ctgcn_amd._lib import CtgcnHipError
    from ctgcn_amd.embedding import UnsupervisedEmbedding
    with pytest.raises(CtgcnHipError):
        UnsupervisedEmbedding(_folders(tmp_path, 2), "origin", "emb", ["a", "b"], CTGCN(4, 8, 8, 1, 1, 2, model_type="S"),
                              ReconstructionLoss(), has_cuda=False)
