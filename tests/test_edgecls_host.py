"""CPU-only checks of the edge-classification host logic (ctgcn_amd/evaluation/edge_classification.py) against the reference fixture
edge_classification_uci.npz."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _ec_fixture
import _lp_fixture
from ctgcn_amd import _lib
from ctgcn_amd.evaluation import _ovr

EC = importlib.import_module("ctgcn_amd.evaluation.edge_classification")   # the package also exports the function edge_classification
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "edge_classification_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
REPS = GOLD["table_acc"].shape[0]
SEED = 20261017           # the embeddings
SPLIT_SEED = 20261022     # the reference drew its splits under np.random.seed(SPLIT_SEED) (make_golden_edgecls.py)
SIZES = [1771, 9015, 2389, 1016, 695, 498, 291]


def _month(t):
    return tuple(GOLD["labels_%d_%s" % (t, c)].astype(np.int64) for c in ("from", "to", "label"))


def _tree(tmp_path, labels=None):
    base = tmp_path
    (base / "1.format").mkdir()
    (base / "nodes_set").mkdir()
    (base / "edges_label").mkdir()
    for f in FILES:
        (base / "1.format" / f).write_text("from_id\tto_id\tweight\n")
    pd.DataFrame(NAMES).to_csv(str(base / "nodes_set" / "nodes.csv"), header=False, index=False)
    for t, f in enumerate(FILES):
        u, v, lab = _month(t) if labels is None else labels[t]
        pd.DataFrame({"from_id": [NAMES[i] for i in u], "to_id": [NAMES[i] for i in v], "label": lab}).to_csv(
            str(base / "edges_label" / f), sep="\t", index=False)
    return str(base)


def test_fixture_labels_and_embeddings_are_rebuilt_exactly():
    for t in range(len(FILES)):
        u, v, lab = _ec_fixture.month_edge_labels(SNAPSHOTS, t)
        assert len(u) == SIZES[t] and (u < v).all() and (np.diff(u * len(NAMES) + v) > 0).all()
        assert all(np.array_equal(a, b) for a, b in zip((u, v, lab), _month(t)))
        assert _lp_fixture.digest(_lp_fixture.month_embedding(SNAPSHOTS, t, len(NAMES), 128, SEED)) == GOLD["emb_sha256"][t]
        assert len(np.bincount(lab)) == 3 and np.ptp(np.bincount(lab)) <= 1


def test_split_files_identical_to_the_reference(tmp_path):
    base = _tree(tmp_path)
    np.random.seed(SPLIT_SEED)
    for r in range(REPS):
        EC.DataGenerator(base, "1.format", "edgecls_data_%d" % r, "nodes_set/nodes.csv", "edges_label", file_sep="\t").generate_edge_samples_all_time()
    for r in range(REPS):
        for t, f in enumerate(FILES):
            date = f.split(".")[0]
            for part in ("train", "val", "test"):
                path = os.path.join(base, "edgecls_data_%d" % r, "%s_%s.csv" % (date, part))
                rows = _ec_fixture.split_rows(GOLD, r, t, part)
                expected = pd.DataFrame({"from_id": rows[:, 0], "to_id": rows[:, 1], "label": rows[:, 2]}).to_csv(sep="\t", index=False)
                assert open(path).read() == expected, (r, date, part)


def test_split_counts():
    for t in range(len(FILES)):
        n = SIZES[t]
        counts = EC.split_counts(n, 0.7, 0.2, 0.1)
        assert counts == tuple(len(_ec_fixture.split_rows(GOLD, 0, t, p)) for p in ("train", "val", "test"))
        assert counts == (int(np.floor(n * 0.7)), int(np.floor(n * 0.2)), int(np.floor(n * 0.1)))
    tr, va, te = EC.shuffle_split(10, 0.7, 0.2, 0.1, np.random.RandomState(0))
    assert (len(tr), len(va), len(te)) == (7, 2, 1) and len(set(tr) | set(va) | set(te)) == 10


def test_bad_labels_raise(tmp_path):
    with pytest.raises(ValueError, match="0..K-1"):
        EC.check_classes([1, 2, 3])
    shifted = [(u, v, lab + 1) for u, v, lab in map(_month, range(len(FILES)))]
    base = _tree(tmp_path, shifted)
    with pytest.raises(ValueError, match="0..K-1"):
        EC.EdgeClassifier(base, "1.format", "2.embedding", "d", "r", "nodes_set/nodes.csv", "edges_label", C_list=[1.0])


def test_unknown_node_raises(tmp_path):
    base = _tree(tmp_path)
    with open(os.path.join(base, "edges_label", FILES[0]), "a") as fh:
        fh.write("%s\tno-such-node\t1\n" % NAMES[0])
    gen = EC.DataGenerator(base, "1.format", "out", "nodes_set/nodes.csv", "edges_label")
    with pytest.raises(ValueError, match="missing from the node file"):
        gen.generate_edge_samples(FILES[0])


def _classifier_on_one_month(tmp_path, column, value):
    """A tree with splits drawn and a zero embedding for month 0, whose val file has `column` of row 0 set to `value`."""
    base = _tree(tmp_path)
    np.random.seed(1)
    EC.DataGenerator(base, "1.format", "d_0", "nodes_set/nodes.csv", "edges_label").generate_edge_samples_all_time()
    path = os.path.join(base, "d_0", FILES[0].split(".")[0] + "_val.csv")
    df = pd.read_csv(path, sep="\t")
    df.loc[0, column] = value
    df.to_csv(path, sep="\t", index=False)
    os.makedirs(os.path.join(base, "emb", "M"))
    pd.DataFrame(np.zeros((len(NAMES), 2), np.float32), index=NAMES).to_csv(os.path.join(base, "emb", "M", FILES[0]), sep="\t")
    return EC.EdgeClassifier(base, "1.format", "emb", "d_0", "r", "nodes_set/nodes.csv", "edges_label", C_list=[1.0])


def test_split_label_outside_the_classes_raises(tmp_path, monkeypatch):
    ec = _classifier_on_one_month(tmp_path, "label", 7)
    monkeypatch.setattr(EC, "_device", lambda device: torch.device("cpu"))
    with pytest.raises(ValueError, match="outside the classes"):
        ec.edge_classification_all_time("M")


def test_split_endpoint_outside_the_nodes_raises(tmp_path, monkeypatch):
    ec = _classifier_on_one_month(tmp_path, "to_id", len(NAMES))
    monkeypatch.setattr(EC, "_device", lambda device: torch.device("cpu"))
    with pytest.raises(ValueError, match="endpoint index outside"):
        ec.edge_classification_all_time("M")


def test_last_of_ties_wins():
    for r in range(REPS):
        for t in range(len(FILES)):
            assert EC.select_C(list(GOLD["tight_val_acc"][r, t])) == GOLD["tight_best"][r, t]
    ties = list(GOLD["edge_ties_tight_val_acc"])
    assert ties.count(max(ties)) > 1 and ties[-1] == max(ties)
    assert float(GOLD["edge_ties_ref_C"]) == float(GOLD["C_list"][-1]) == float(GOLD["C_list"][EC.select_C(ties)])


def test_aggregate_results_matches_reference(tmp_path):
    for r in range(REPS):
        d = tmp_path / ("edgecls_res_%d" % r)
        d.mkdir()
        pd.DataFrame({"date": GOLD["table_dates"], "acc": GOLD["table_acc"][r]}).to_csv(str(d / "M_acc_record.csv"), sep=",", index=False)
    EC.aggregate_results(str(tmp_path), "edgecls_res", 0, REPS, ["M"])
    df = pd.read_csv(str(tmp_path / "edgecls_res" / "M_acc_record.csv"))
    assert list(df.columns) == [str(c) for c in GOLD["agg_columns"]]
    np.testing.assert_allclose(df.iloc[:, 1:].values, GOLD["agg_values"], rtol=0, atol=1e-15)


def test_acc_record_format(tmp_path, monkeypatch):
    """edge_classification_all_time writes date, acc with sep ',' for the dates that have an embedding."""
    base = _tree(tmp_path)
    np.random.seed(2)
    EC.DataGenerator(base, "1.format", "d_0", "nodes_set/nodes.csv", "edges_label").generate_edge_samples_all_time()
    os.makedirs(os.path.join(base, "emb", "M"))
    for f in FILES[1:]:
        pd.DataFrame(np.zeros((len(NAMES), 2), np.float32), index=NAMES).to_csv(os.path.join(base, "emb", "M", f), sep="\t")
    ec = EC.EdgeClassifier(base, "1.format", "emb", "d_0", "res_0", "nodes_set/nodes.csv", "edges_label", C_list=[1.0])
    accs = iter(GOLD["table_acc"][0][1:])
    monkeypatch.setattr(EC, "_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(EC, "evaluate_batch", lambda E, splits, *a, **k: ([{"acc": next(accs)} for _ in splits], []))
    ec.edge_classification_all_time("M")
    out = open(os.path.join(base, "res_0", "M_acc_record.csv")).read()
    expected = pd.DataFrame({"date": [str(d) for d in GOLD["table_dates"][1:]], "acc": GOLD["table_acc"][0][1:]}).to_csv(sep=",", index=False)
    assert out == expected


def test_edgecls_symbols_and_invalid_arguments():
    assert _lib.ABI_VERSION == 31
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "ctgcn_hip.h")).read()
    so = open(os.path.join(os.path.dirname(_lib.__file__), "csrc", "libctgcn_hip.so"), "rb").read()
    for name in ("ctgcn_ec_grad_f32", "ctgcn_ec_hess_f32", "ctgcn_ec_predict_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name) and name.encode() in so and "%s(" % name in header
        node = _lib.SIGNATURES[name.replace("_ec_", "_nc_")]
        at = 7 if "hess" in name or "predict" in name else 6          # rows' position: rows2 follows it
        assert _lib.SIGNATURES[name] == (node[0], node[1][:at + 1] + [node[1][at]] + node[1][at + 1:])
    p = 1     # never dereferenced: every call below fails its argument check first
    # the same codes as ctgcn_nc_* (test_nodecls_host.py), rows2 in place
    assert lib.ctgcn_ec_grad_f32(0, 128, 18, p, p, 1, p, p, p, p, p, p, p, 10, p, 128, p, 18, p, p, p, 1 << 30, None) == -1   # no problems
    assert lib.ctgcn_ec_grad_f32(1, 257, 18, p, p, 1, p, p, p, p, p, p, p, 10, p, 257, p, 18, p, p, p, 1 << 30, None) == -4   # d > 256
    assert lib.ctgcn_ec_grad_f32(1, 128, 18, None, p, 1, p, p, p, p, p, p, p, 10, p, 128, p, 18, p, p, p, 1 << 30, None) == -1
    assert lib.ctgcn_ec_grad_f32(1, 128, 18, p, p, 1, p, None, p, p, p, p, p, 10, p, 128, p, 18, p, p, p, 1 << 30, None) == -1  # null rows2
    assert lib.ctgcn_ec_grad_f32(1, 128, 18, p, p, 1, p, p, p, p, p, p, p, 10, p, 128, p, 18, p, p, p, 0, None) == -3         # workspace
    assert lib.ctgcn_ec_hess_f32(1, 128, 18, p, p, 1, 0, p, p, p, p, p, p, p, 10, p, 128, p, 18, p, p, 1 << 30, None) == -1    # hess_max 0
    assert lib.ctgcn_ec_hess_f32(1, 128, 18, p, p, 1, 256, p, None, p, p, p, p, p, 10, p, 128, p, 18, p, p, 1 << 30, None) == -1  # null rows2
    assert lib.ctgcn_ec_predict_f32(1, 128, 1, 6, p, p, 1, p, p, p, p, p, p, 10, p, 128, p, 6, p, p, None) == -1            # K < 2
    assert lib.ctgcn_ec_predict_f32(1, 128, 3, 6, p, p, 1, p, None, p, p, p, p, 10, p, 128, p, 18, p, p, None) == -1         # null rows2
    assert lib.ctgcn_ec_predict_f32(1, 200, 40, 6, p, p, 1, p, p, p, p, p, p, 10, p, 200, p, 240, p, p, None) == -4         # K > 32


def test_mixed_pair_and_node_problems_raise():
    z = torch.zeros(3, dtype=torch.int64)
    pair, node = _ovr.Problem(z, z.to(torch.int32), 2, rows2=z), _ovr.Problem(z, z.to(torch.int32), 2)
    assert pair.rows2 is not None and node.rows2 is None
    with pytest.raises(ValueError, match="all have rows2"):
        _ovr.Table(torch.zeros(4, 2), [pair, node], [1.0])
    with pytest.raises(ValueError, match="all have rows2"):
        _ovr._pair([node, pair])
    assert _ovr._pair([pair, pair]) is True and _ovr._pair([node]) is False


def test_cpu_tensors_fail_loudly():
    E = torch.zeros(6, 4)
    split = torch.tensor([[0, 1, 0], [1, 2, 1], [2, 2, 0]])
    with pytest.raises(RuntimeError, match="edge-classification evaluation runs on the GPU, no CPU fallback"):
        EC.evaluate(E, split, split, split, [1.0], [0, 1])
    trip = (np.arange(3), np.array([1, 2, 2]), np.array([0, 1, 0]))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        EC.evaluate_window([E, E], [trip] * 2, [1.0], rep_num=1)
    z = torch.zeros(3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="edge-classification evaluation runs on the GPU, no CPU fallback"):
        _ovr._cat_rows([_ovr.Problem(z, z.to(torch.int32), 2, rows2=z)], True, "edge-classification", E.device)
