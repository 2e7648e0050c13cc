"""evaluation/graph_reconstruction.py on the GPU against the float64 model of tests/_topk_ref.py.

The embedding rows hold 4 or 16 entries of ±s (s = 1, 2, 3) and zeros: their norms are 2 s and 4 s, so the operands of all three
metrics ('cosine' rows of ±1/2 or ±1/4, 'l2' biases of −2 s² or −8 s²) and every score are exact in fp32, the device and the model
rank the same numbers, and MAP, the counted rows and every precision@k must be EQUAL.  Nodes 0-39 share one row: the 39 pairs of
node 0 with them head the global order, which fills the first list widths of global_precision and forces it to double."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _topk_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, D = 300, 16
K_LIST = [10, 200]

GR = importlib.import_module("ctgcn_amd.evaluation.graph_reconstruction")


def _embedding(seed):
    rng = np.random.default_rng(seed)
    E = np.zeros((N, D), dtype=np.float32)
    for i in range(N):
        nz = rng.permutation(D)[:(4 if rng.integers(2) else 16)]
        E[i, nz] = rng.choice([-1.0, 1.0], size=len(nz)) * rng.integers(1, 4)
    E[:40] = 3 * np.where(np.arange(D) % 2, 1.0, -1.0)          # the largest norm there is: 144 is the highest score of every metric's order
    E[40] = 0                                                   # a zero row: 'cosine' leaves it zero
    return E


def _graph(seed, extra=()):
    """a symmetric edge set on N nodes (pairs both ways), with node 299 isolated"""
    rng = np.random.default_rng(seed)
    pairs = {(int(a), int(b)) for a, b in rng.integers(0, N - 1, size=(900, 2)) if a != b}
    pairs |= {(0, j) for j in range(1, 40, 2)} | set(extra)
    return sorted(pairs | {(b, a) for a, b in pairs})


def _adj(pairs):
    from ctgcn_amd import ops
    row_ptr, col = R.csr_from_pairs(N, pairs)
    return ops.GcnAdj(torch.from_numpy(row_ptr).to(DEV), torch.from_numpy(col).to(DEV),
                      torch.ones(len(col), dtype=torch.float32, device=DEV)), (row_ptr, col)


@pytest.fixture(scope="module")
def data():
    E = _embedding(1)
    first = _graph(2)
    second = _graph(3, extra=first[::3])                         # a later snapshot: keeps a third of the edges, adds new ones
    return E, _adj(first), _adj(second)


@pytest.mark.parametrize("metric", ["dot", "cosine", "l2"])
@pytest.mark.parametrize("mode", ["recon", "pred"])
def test_evaluate_equals_the_model(data, metric, mode):
    E, (adj1, csr1), (adj2, csr2) = data
    known_adj, known_csr = (adj1, csr1) if mode == "pred" else (None, None)
    out = GR.evaluate(torch.from_numpy(E).to(DEV), adj2, K_LIST, max_k=100, metric=metric, known=known_adj)
    X, rb, cb = GR.score_inputs(torch.from_numpy(E), metric)
    Xr, rbr, cbr = R.score_inputs(E, metric)
    assert np.array_equal(X.numpy().astype(np.float64), Xr) and (rb is None or np.array_equal(rb.numpy().astype(np.float64), rbr))
    ref = R.evaluate(E, csr2, K_LIST, 100, metric, known_csr)
    print("  %s/%s MAP %.6f rows %d P@k %s width %d doublings %d" % (mode, metric, out['MAP'], out['rows'], out['precision'], out['width'],
                                                                  out['doublings']))
    assert out['rows'] == ref['rows'] and 0 < ref['rows'] < N
    assert out['MAP'] == ref['MAP'] and 0.0 < ref['MAP'] < 1.0
    assert out['precision'] == ref['precision'] and out['pairs'] == ref['pairs'] == {10: 10, 200: 200}
    assert out['doublings'] >= 1 and out['width'] > GR.START_WIDTH                   # the planted copies of node 0


def _write_snapshots(base, E, graphs):
    os.makedirs(os.path.join(base, "1.format"))
    os.makedirs(os.path.join(base, "2.embedding", "GCN"))
    nodes = ["n%03d" % i for i in range(N)]
    with open(os.path.join(base, "nodes.csv"), "w") as f:
        f.write("\n".join(nodes) + "\n")
    for t, pairs in enumerate(graphs):
        name = "2020-0%d.csv" % (t + 1)
        with open(os.path.join(base, "1.format", name), "w") as f:
            f.write("from_id\tto_id\tweight\n")
            f.writelines("%s\t%s\t1.0\n" % (nodes[a], nodes[b]) for a, b in pairs if a < b)
        pd.DataFrame(E * (t + 1), index=nodes).to_csv(os.path.join(base, "2.embedding", "GCN", name), sep="\t")


@pytest.mark.parametrize("mode", ["recon", "pred"])
def test_graph_reconstructor_writes_the_table(tmp_path, mode):
    E = _embedding(4)
    graphs = [_graph(5), _graph(6), _graph(7)]
    base = str(tmp_path)
    _write_snapshots(base, E, graphs)
    rec = GR.GraphReconstructor(base, "1.format", "2.embedding", "3.recon", "nodes.csv", k_list=K_LIST, max_k=50, metric="l2", mode=mode)
    rec.graph_reconstruction_all_method(["GCN"])
    df = pd.read_csv(os.path.join(base, "3.recon", "GCN_%s.csv" % mode), float_precision="round_trip")
    assert list(df.columns) == ["date", "MAP", "P@10", "P@200"]
    dates = ["2020-01", "2020-02", "2020-03"][1 if mode == "pred" else 0:]           # pred has no embedding before the first snapshot
    assert list(df["date"]) == dates + ["avg"]
    for row, date in enumerate(dates):
        t = int(date[-1]) - 1
        emb = torch.from_numpy(E * (t if mode == "pred" else t + 1)).to(DEV)        # pred: the embedding of the snapshot before
        known = _adj(graphs[t - 1])[0] if mode == "pred" else None
        want = GR.evaluate(emb, _adj(graphs[t])[0], K_LIST, max_k=50, metric="l2", known=known)
        assert df["MAP"][row] == want["MAP"]                                     # the csv text round-trips a float64
        assert [df["P@10"][row], df["P@200"][row]] == [want["precision"][10], want["precision"][200]]
    assert df["MAP"][len(dates)] == pytest.approx(np.mean(df["MAP"][:len(dates)]), rel=1e-12)
