"""CPU-only checks of the node-classification host logic (ctgcn_amd/evaluation/node_classification.py) against the reference fixture
node_classification_uci.npz."""
import importlib
import os

import numpy as np
import pandas as pd
import pytest
import torch

import _lp_fixture
import _nc_fixture
from ctgcn_amd import _lib

NC = importlib.import_module("ctgcn_amd.evaluation.node_classification")   # the package also exports the function node_classification
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "node_classification_uci.npz"))
SNAPSHOTS = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
FILES = [str(f) for f in GOLD["files"]]
NAMES = [str(x) for x in GOLD["node_names"]]
REPS = GOLD["table_acc"].shape[0]
SEED = 20261016


def _tree(tmp_path, labels=None):
    base = tmp_path
    (base / "1.format").mkdir()
    (base / "nodes_set").mkdir()
    (base / "nodes_label").mkdir()
    for f in FILES:
        (base / "1.format" / f).write_text("from_id\tto_id\tweight\n")
    pd.DataFrame(NAMES).to_csv(str(base / "nodes_set" / "nodes.csv"), header=False, index=False)
    for t, f in enumerate(FILES):
        nodes, lab = (GOLD["labels_%d_node" % t], GOLD["labels_%d_label" % t]) if labels is None else labels[t]
        pd.DataFrame({"node": [NAMES[i] for i in nodes], "label": lab}).to_csv(str(base / "nodes_label" / f), sep="\t", index=False)
    return str(base)


def test_fixture_labels_and_embeddings_are_rebuilt_exactly():
    for t in range(len(FILES)):
        nodes, lab = _nc_fixture.month_labels(SNAPSHOTS, t)
        assert np.array_equal(nodes, GOLD["labels_%d_node" % t]) and np.array_equal(lab, GOLD["labels_%d_label" % t])
        assert _lp_fixture.digest(_lp_fixture.month_embedding(SNAPSHOTS, t, len(NAMES), 128, SEED)) == GOLD["emb_sha256"][t]
        assert np.bincount(lab).min() >= len(lab) // 4 - 1


def test_split_files_identical_to_the_reference(tmp_path):
    base = _tree(tmp_path)
    np.random.seed(SEED)
    for r in range(REPS):
        NC.DataGenerator(base, "1.format", "nodecls_data_%d" % r, "nodes_set/nodes.csv", "nodes_label", file_sep="\t").generate_node_samples_all_time()
    for r in range(REPS):
        for t, f in enumerate(FILES):
            date = f.split(".")[0]
            for part in ("train", "val", "test"):
                path = os.path.join(base, "nodecls_data_%d" % r, "%s_%s.csv" % (date, part))
                rows = _nc_fixture.split_rows(GOLD, r, t, part)
                expected = pd.DataFrame({"node": rows[:, 0], "label": rows[:, 1]}).to_csv(sep="\t", index=False)
                assert open(path).read() == expected, (r, date, part)


def test_split_counts():
    for t in range(len(FILES)):
        n = len(GOLD["labels_%d_node" % t])
        counts = NC.split_counts(n, 0.7, 0.2, 0.1)
        assert counts == tuple(len(_nc_fixture.split_rows(GOLD, 0, t, p)) for p in ("train", "val", "test"))
        assert counts == (int(np.floor(n * 0.7)), int(np.floor(n * 0.2)), int(np.floor(n * 0.1)))
    tr, va, te = NC.shuffle_split(10, 0.7, 0.2, 0.1, np.random.RandomState(0))
    assert (len(tr), len(va), len(te)) == (7, 2, 1) and len(set(tr) | set(va) | set(te)) == 10


def test_bad_labels_raise(tmp_path):
    with pytest.raises(ValueError, match="0..K-1"):
        NC.check_classes([1, 2, 3])
    with pytest.raises(ValueError, match="0..K-1"):
        NC.check_classes([0, 0, 0])
    assert NC.check_classes([3, 0, 2, 1, 1]) == [0, 1, 2, 3]
    shifted = [(GOLD["labels_%d_node" % t], GOLD["labels_%d_label" % t] + 1) for t in range(len(FILES))]
    base = _tree(tmp_path, shifted)
    with pytest.raises(ValueError, match="0..K-1"):
        NC.NodeClassifier(base, "1.format", "2.embedding", "d", "r", "nodes_set/nodes.csv", "nodes_label", C_list=[1.0])


def test_unknown_node_raises(tmp_path):
    base = _tree(tmp_path)
    with open(os.path.join(base, "nodes_label", FILES[0]), "a") as fh:
        fh.write("no-such-node\t1\n")
    gen = NC.DataGenerator(base, "1.format", "out", "nodes_set/nodes.csv", "nodes_label")
    with pytest.raises(ValueError, match="missing from the node file"):
        gen.generate_node_samples(FILES[0])


def test_split_label_outside_the_classes_raises(tmp_path, monkeypatch):
    base = _tree(tmp_path)
    np.random.seed(1)
    NC.DataGenerator(base, "1.format", "d_0", "nodes_set/nodes.csv", "nodes_label").generate_node_samples_all_time()
    path = os.path.join(base, "d_0", FILES[0].split(".")[0] + "_val.csv")
    df = pd.read_csv(path, sep="\t")
    df.loc[0, "label"] = 7
    df.to_csv(path, sep="\t", index=False)
    os.makedirs(os.path.join(base, "emb", "M"))
    pd.DataFrame(np.zeros((len(NAMES), 2), np.float32), index=NAMES).to_csv(os.path.join(base, "emb", "M", FILES[0]), sep="\t")
    nc = NC.NodeClassifier(base, "1.format", "emb", "d_0", "r", "nodes_set/nodes.csv", "nodes_label", C_list=[1.0])
    monkeypatch.setattr(NC, "_device", lambda device: torch.device("cpu"))
    with pytest.raises(ValueError, match="outside the classes"):
        nc.node_classification_all_time("M")


def test_last_of_ties_wins():
    assert NC.select_C([0.7, 0.8, 0.8, 0.6]) == 2
    assert NC.select_C([0.5] * 6) == 5
    for r in range(REPS):
        for t in range(len(FILES)):
            assert NC.select_C(list(GOLD["tight_val_acc"][r, t])) == GOLD["tight_best"][r, t]
    assert float(GOLD["edge_ties_ref_C"]) == float(GOLD["C_list"][-1])


def test_aggregate_results_matches_reference(tmp_path):
    for r in range(REPS):
        d = tmp_path / ("nodecls_res_%d" % r)
        d.mkdir()
        pd.DataFrame({"date": GOLD["table_dates"], "acc": GOLD["table_acc"][r]}).to_csv(str(d / "M_acc_record.csv"), sep=",", index=False)
    NC.aggregate_results(str(tmp_path), "nodecls_res", 0, REPS, ["M"])
    df = pd.read_csv(str(tmp_path / "nodecls_res" / "M_acc_record.csv"))
    assert list(df.columns) == [str(c) for c in GOLD["agg_columns"]]
    np.testing.assert_allclose(df.iloc[:, 1:].values, GOLD["agg_values"], rtol=0, atol=1e-15)


def test_acc_record_format(tmp_path, monkeypatch):
    """node_classification_all_time writes date, acc with sep ',' for the dates that have an embedding."""
    base = _tree(tmp_path)
    np.random.seed(2)
    NC.DataGenerator(base, "1.format", "d_0", "nodes_set/nodes.csv", "nodes_label").generate_node_samples_all_time()
    os.makedirs(os.path.join(base, "emb", "M"))
    for f in FILES[1:]:
        pd.DataFrame(np.zeros((len(NAMES), 2), np.float32), index=NAMES).to_csv(os.path.join(base, "emb", "M", f), sep="\t")
    nc = NC.NodeClassifier(base, "1.format", "emb", "d_0", "res_0", "nodes_set/nodes.csv", "nodes_label", C_list=[1.0])
    accs = iter(GOLD["table_acc"][0][1:])
    monkeypatch.setattr(NC, "_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(NC, "evaluate_batch", lambda E, splits, *a, **k: ([{"acc": next(accs)} for _ in splits], []))
    nc.node_classification_all_time("M")
    out = open(os.path.join(base, "res_0", "M_acc_record.csv")).read()
    expected = pd.DataFrame({"date": [str(d) for d in GOLD["table_dates"][1:]], "acc": GOLD["table_acc"][0][1:]}).to_csv(sep=",", index=False)
    assert out == expected


def test_nodecls_symbols_and_invalid_arguments():
    assert _lib.ABI_VERSION == 31
    lib = _lib.load()
    for name in ("ctgcn_nc_chunks", "ctgcn_nc_hess_parts", "ctgcn_nc_grad_workspace_bytes", "ctgcn_nc_grad_f32", "ctgcn_nc_hess_workspace_bytes",
                 "ctgcn_nc_hess_f32", "ctgcn_nc_predict_f32"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert "%s(" % name in open(os.path.join(os.path.dirname(__file__), "..", "include", "ctgcn_hip.h")).read()
    assert lib.ctgcn_nc_chunks(0) == 1 and lib.ctgcn_nc_chunks(833) == 7 and lib.ctgcn_nc_chunks(10 ** 7) == 1024
    assert lib.ctgcn_nc_hess_parts(833, 1 << 17) == 1 and lib.ctgcn_nc_hess_parts(700_000, 1 << 17) == 64
    assert lib.ctgcn_nc_grad_workspace_bytes(10, 128, 24) >= 10 * 24 * 130 * 8
    assert lib.ctgcn_nc_hess_workspace_bytes(10, 128, 24) >= 10 * 24 * 129 * 129 * 4
    p = 1     # never dereferenced: every call below fails its argument check first
    assert lib.ctgcn_nc_grad_f32(0, 128, 24, p, p, 1, p, p, p, p, p, p, 10, p, 128, p, 24, p, p, p, 1 << 30, None) == -1   # no problems
    assert lib.ctgcn_nc_grad_f32(1, 257, 24, p, p, 1, p, p, p, p, p, p, 10, p, 257, p, 24, p, p, p, 1 << 30, None) == -4   # d > 256
    assert lib.ctgcn_nc_grad_f32(1, 128, 24, None, p, 1, p, p, p, p, p, p, 10, p, 128, p, 24, p, p, p, 1 << 30, None) == -1
    assert lib.ctgcn_nc_grad_f32(1, 128, 24, p, p, 1, p, p, p, p, p, p, 10, p, 128, p, 24, p, p, p, 0, None) == -3         # workspace
    assert lib.ctgcn_nc_hess_f32(1, 128, 24, p, p, 1, 0, p, p, p, p, p, p, 10, p, 128, p, 24, p, p, 1 << 30, None) == -1    # hess_max 0
    assert lib.ctgcn_nc_predict_f32(1, 128, 1, 6, p, p, 1, p, p, p, p, p, 10, p, 128, p, 6, p, p, None) == -1            # K < 2
    assert lib.ctgcn_nc_predict_f32(1, 200, 40, 6, p, p, 1, p, p, p, p, p, 10, p, 200, p, 240, p, p, None) == -4         # K > 32


def test_class_limit_of_predict_is_named_and_matches_the_wrapper():
    """predict refuses K above the models of a block (64 up to d = 131, 32 above): the C message carries the count, the limit and d,
    and _ovr.max_classes, which Table.predict checks before any launch, is the same step function."""
    from ctgcn_amd.evaluation import _ovr
    lib = _lib.load()
    p = 1     # never dereferenced: the class check comes first
    for d in (1, 127, 128, 131, 132, 200, 256):
        limit = _ovr.max_classes(d)
        assert limit == (64 if d <= 131 else 32)
        K = limit + 1
        for fn, extra in ((lib.ctgcn_nc_predict_f32, ()), (lib.ctgcn_ec_predict_f32, (p,))):
            assert fn(1, d, K, 2, p, p, 1, p, *extra, p, p, p, p, 10, p, d, p, 2 * K, p, p, None) == -4
            msg = lib.ctgcn_last_error().decode()
            assert "%d classes, at most %d at d = %d" % (K, limit, d) in msg, msg


def test_cpu_tensors_fail_loudly():
    E = torch.zeros(6, 4)
    split = torch.tensor([[0, 0], [1, 1], [2, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NC.evaluate(E, split, split, split, [1.0], [0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        NC.evaluate_window([E, E], [(np.arange(3), np.array([0, 1, 0]))] * 2, [1.0], rep_num=1)
