"""CPU-only checks of the link-prediction host logic (ctgcn_amd/evaluation) against the reference fixture link_prediction_uci.npz."""
import os

import numpy as np
import pandas as pd
import pytest
import torch

import importlib

import _lp_fixture
from ctgcn_amd.evaluation import _logreg

LP = importlib.import_module("ctgcn_amd.evaluation.link_prediction")   # the package also exports the function link_prediction
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "link_prediction_uci.npz"))
MONTHS = range(1, len(GOLD["files"]))
N = len(GOLD["node_names"])


def test_split_counts_match_reference():
    for lines, train, val, test in GOLD["counts"]:
        assert LP.split_counts(2 * int(lines), 0.5, 0.3, 0.2) == (train, val, test)


def test_fixture_splits_have_the_reference_layout():
    for t in MONTHS:
        _, train, val, test = GOLD["counts"][t]
        for part, num in (("train", train), ("val", val), ("test", test)):
            arr = _lp_fixture.decode_split(GOLD, t, part, N)
            assert arr.shape == (2 * num, 3)
            assert (arr[:num, 2] == 1).all() and (arr[num:, 2] == 0).all()


def test_assemble_splits_slices_val_test_train_then_negatives():
    edge_num = 1000
    shuffled = torch.stack([torch.arange(edge_num), torch.arange(edge_num) + 5000], 1)
    train_num, val_num, test_num = LP.split_counts(edge_num, 0.5, 0.3, 0.2)
    neg = torch.stack([-torch.arange(train_num + test_num + val_num) - 1] * 2, 1)
    train, val, test = LP.assemble_splits(shuffled, neg, 0.5, 0.3, 0.2)
    assert (val[:val_num, 0] == torch.arange(val_num)).all()
    assert (test[:test_num, 0] == torch.arange(val_num, val_num + test_num)).all()
    assert (train[:train_num, 0] == torch.arange(val_num + test_num, val_num + test_num + train_num)).all()
    for split, num in ((train, train_num), (val, val_num), (test, test_num)):
        assert split.shape == (2 * num, 3)
        assert (split[:num, 2] == 1).all() and (split[num:, 2] == 0).all() and (split[num:, 0] < 0).all()
    # negatives are consumed train, test, val
    assert int(train[train_num, 0]) == -1 and int(test[test_num, 0]) == -1 - train_num
    assert int(val[val_num, 0]) == -1 - train_num - test_num


def test_lp_data_round_trip_is_byte_identical_to_pandas(tmp_path):
    arr = _lp_fixture.decode_split(GOLD, 1, "val", N)
    ours, ref = tmp_path / "ours.csv", tmp_path / "ref.csv"
    LP.write_split(str(ours), torch.from_numpy(arr), "\t")
    pd.DataFrame(arr, columns=['from_id', 'to_id', 'label']).to_csv(str(ref), sep="\t", index=False)
    assert ours.read_bytes() == ref.read_bytes()
    assert (pd.read_csv(str(ours), sep="\t").values == arr).all()


def test_auc_record_format(tmp_path, monkeypatch):
    """LinkPredictor.link_prediction_all_time writes the reference's table: date + measures, sep ','."""
    dates, auc = GOLD["table_dates"], GOLD["table_auc"]
    measures = ["Avg", "Had", "L1", "L2", "sigmoid"]
    base = tmp_path
    (base / "orig").mkdir()
    for f in GOLD["files"]:
        (base / "orig" / str(f)).write_text("from_id\tto_id\tweight\n")
    (base / "nodes.csv").write_text("a\nb\n")
    pred = LP.LinkPredictor(str(base), "orig", "emb", "lp", "res", "nodes.csv", C_list=[1.0], measure_list=measures)
    rows = iter([{"auc": dict(zip(measures, r))} for r in auc])
    monkeypatch.setattr(LP, "_device", lambda device: torch.device("cpu"))
    monkeypatch.setattr(LP, "evaluate", lambda *a, **k: next(rows))
    monkeypatch.setattr(pred, "_read_split", lambda *a: None)
    for f in GOLD["files"][:-1]:
        os.makedirs(base / "emb" / "M", exist_ok=True)
        pd.DataFrame(np.zeros((2, 3), np.float32), index=["a", "b"]).to_csv(str(base / "emb" / "M" / str(f)), sep="\t")
    pred.link_prediction_all_time("M")
    out = base / "res" / "M_auc_record.csv"
    expected = pd.DataFrame([[str(d)] + list(r) for d, r in zip(dates, auc)], columns=["date"] + measures)
    assert out.read_bytes() == expected.to_csv(sep=",", index=False).encode()


def test_fixture_embedding_is_rebuilt_exactly():
    snapshots = np.load(os.path.join(os.path.dirname(__file__), "golden", "uci_snapshots.npz"))
    for t in range(len(GOLD["files"]) - 1):
        assert _lp_fixture.digest(_lp_fixture.month_embedding(snapshots, t, N)) == GOLD["emb_sha256"][t]


def test_balanced_weights():
    w_neg, w_pos = _logreg.balanced_weights(30, 10)
    assert (w_neg, w_pos) == (40 / 60, 40 / 20)
    assert 30 * w_neg + 10 * w_pos == pytest.approx(40)
    for t in MONTHS:
        y = _lp_fixture.decode_split(GOLD, t, "train", N)[:, 2]
        w_neg, w_pos = _logreg.balanced_weights(int((y == 0).sum()), int((y == 1).sum()))
        assert w_neg == w_pos == 1.0        # the reference's splits are balanced by construction


def test_last_of_ties_wins():
    assert LP.select_C([0.7, 0.8, 0.8, 0.6]) == 2
    assert LP.select_C([0.5, 0.5, 0.5, 0.5]) == 3
    assert LP.select_C([0.9, 0.1]) == 0
    for t in MONTHS:
        for mi in range(4):
            assert LP.select_C(list(GOLD["ref_val_auc"][t - 1, mi])) == GOLD["ref_best"][t - 1, mi]


def test_auc_with_ties_matches_sklearn():
    y = torch.from_numpy(GOLD["auc_ties_y"])
    s = torch.from_numpy(GOLD["auc_ties_s"])
    assert _logreg.roc_auc(y, s) == pytest.approx(float(GOLD["auc_ties_auc"]), abs=1e-15)
    with pytest.raises(ValueError):
        _logreg.roc_auc(torch.ones(4), torch.rand(4))


def test_aggregate_results_columns(tmp_path):
    measures = ["Avg", "Had"]
    for i, vals in ((0, [0.6, 0.7]), (1, [0.8, 0.5])):
        d = tmp_path / ("lp_res_%d" % i)
        d.mkdir()
        pd.DataFrame([["2004-05"] + vals], columns=["date"] + measures).to_csv(str(d / "M_auc_record.csv"), sep=",", index=False)
    LP.aggregate_results(str(tmp_path), "lp_res", 0, 2, ["M"], measures)
    df = pd.read_csv(str(tmp_path / "lp_res" / "M_Avg_record.csv"))
    assert list(df.columns) == ["date", "Avg_0", "Avg_1", "avg", "max", "min"]
    assert df.loc[0, "avg"] == pytest.approx(0.7) and df.loc[0, "max"] == 0.8 and df.loc[0, "min"] == 0.6
    assert list(pd.read_csv(str(tmp_path / "lp_res" / "M_Had_record.csv")).columns) == ["date", "Had_0", "Had_1", "avg", "max", "min"]


def test_cpu_tensors_fail_loudly():
    E = torch.zeros(4, 8)
    edges = torch.tensor([[0, 1, 1], [2, 3, 0]])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LP.evaluate(E, edges, edges, edges, [1.0], ["Had"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        LP.make_splits(edges[:, :2], 4, 0.5, 0.3, 0.2, seed=0)
