"""Host-side pieces of the supervised trainer (no GPU): split arithmetic, label loaders, state-dict keys, the incidence builder, the
limits that raise, and the new symbols of the C ABI."""
import os

import numpy as np
import pytest
import torch

import _sup_fixture as SF
from conftest import load_golden


@pytest.fixture(scope="module")
def gold():
    return load_golden("supervised_uci.npz")


@pytest.fixture(scope="module")
def snapshots():
    return load_golden("uci_snapshots.npz")


def test_label_splits_floor_and_file_order(gold, snapshots):
    from ctgcn_amd.embedding import label_splits, supervised_split_counts
    seed = int(gold["label_seed"])
    assert supervised_split_counts(481, 0.5, 0.3, 0.2) == (240, 144, 96) and supervised_split_counts(7, 0.5, 0.3, 0.2) == (3, 2, 1)
    for case, rows_of, width in (("node_c", SF.node_label_rows, 2), ("edge_ctgcn", SF.edge_label_rows, 3)):
        labels = [torch.from_numpy(rows_of(snapshots, t, seed)) for t in SF.MONTHS]
        parts = label_splits(labels, *SF.RATIOS)
        items = gold[case + "_items"].astype(int)                  # per loss call (train, train, val, train, val, test) and snapshot
        for s, lab in enumerate(labels):
            n = lab.shape[0]
            tr, va, te = (int(np.floor(n * r)) for r in SF.RATIOS)
            assert [items[0, s], items[2, s], items[5, s]] == [tr, va, te]
            for k, (lo, hi) in enumerate(((0, tr), (tr, tr + va), (tr + va, tr + va + te))):
                idx, y = parts[2 * k][s], parts[2 * k + 1][s]
                assert torch.equal(y, lab[lo:hi, -1])              # file order, no shuffle
                if width == 2:
                    assert idx.shape == (hi - lo,) and torch.equal(idx, lab[lo:hi, 0])
                else:
                    assert idx.shape == (2, hi - lo) and torch.equal(idx, lab[lo:hi, :2].t())


def test_link_dy_starts_at_snapshot_one(gold, snapshots):
    assert int(gold["link_st_snapshots"]) == 3 and int(gold["link_dy_snapshots"]) == 2
    edges = [SF.edge_list(snapshots, t) for t in SF.MONTHS]
    for case, first in (("link_st", 0), ("link_dy", 1)):
        splits = SF.stored_splits(gold, case)
        for s in range(int(gold[case + "_snapshots"])):
            E = edges[first + s].shape[1]
            keys = set((edges[first + s][0] * SF.N_NODES + edges[first + s][1]).tolist())
            for k, r in enumerate(SF.RATIOS):
                idx, lab = splits[2 * k][s], splits[2 * k + 1][s]
                cnt = int(np.floor(E * r))
                assert idx.shape == (2, 2 * cnt) and lab.sum() == cnt
                pos = idx[0, :cnt] * SF.N_NODES + idx[1, :cnt]
                assert all(int(p) in keys for p in pos)            # positives of THIS snapshot: S-link-dy starts at snapshot 1


def test_label_loaders(tmp_path):
    from ctgcn_amd import DataLoader
    names = ["n%d" % i for i in range(6)]
    nl, el = tmp_path / "nlabel", tmp_path / "elabel"
    nl.mkdir()
    el.mkdir()
    # written out of order on disk: the loader visits sorted(listdir)
    (nl / "2020-03.csv").write_text("node\tlabel\nn5\t7\nn0\t1\n")
    (nl / "2020-01.csv").write_text("node\tlabel\nn3\t1\nn1\t0\nn2\t1\n")
    (nl / "2020-02.csv").write_text("node\tlabel\nn4\t2\nn0\t0\n")
    (el / "2020-02.csv").write_text("from_id\tto_id\tlabel\nn4\tn0\t1\n")
    (el / "2020-01.csv").write_text("from_id\tto_id\tlabel\nn3\tn1\t0\nn1\tn2\t2\n")
    dl = DataLoader(names, 3, has_cuda=False)
    lists, n_label = dl.get_node_label_list(str(nl), 0, 2)
    assert n_label == 3 and len(lists) == 2 and lists[0].dtype == torch.int64
    assert lists[0].tolist() == [[3, 1], [1, 0], [2, 1]] and lists[1].tolist() == [[4, 2], [0, 0]]
    lists, n_label = dl.get_node_label_list(str(nl), 1, 5)                  # the window stops at max_time_num; labels over the window only
    assert n_label == 4 and [x.tolist() for x in lists] == [[[4, 2], [0, 0]], [[5, 7], [0, 1]]]
    lists, n_label = dl.get_edge_label_list(str(el), 0, 2)
    assert n_label == 3 and lists[0].tolist() == [[3, 1, 0], [1, 2, 2]] and lists[1].tolist() == [[4, 0, 1]]


def test_state_dict_keys_match_the_reference(gold):
    from ctgcn_amd import EdgeClassifier, InnerProduct, MLPClassifier
    mods = {"MLPClassifier": MLPClassifier(128, 128, 4, 1, 3), "InnerProduct": InnerProduct(), "EdgeClassifier": EdgeClassifier(128, 128, 3, 1, 3)}
    for name, mod in mods.items():
        want = [str(k) for k in gold["state_keys_" + name]]
        assert list(mod.state_dict().keys()) == want
        shaped = {k: torch.full_like(v, 0.25) for k, v in mod.state_dict().items()}     # a reference-shaped state dict
        mod.load_state_dict(shaped, strict=True)
        assert all(bool((v == 0.25).all()) for v in mod.state_dict().values())
    assert len(mods["MLPClassifier"].mlp_list) == 3                                      # all duration MLPs are kept


def test_incidence_builder_hand_case():
    from ctgcn_amd import ops
    a, b = torch.tensor([0, 2, 2, 4, 2]), torch.tensor([1, 2, 0, 4, 3])                 # item 1 and item 3 have from == to; node 5: no item
    inc = ops.cls_incidence(a, b, 6, piece=2)
    assert inc.row_ptr.tolist() == [0, 2, 3, 7, 8, 10, 10]
    assert inc.inc_item.tolist() == [0, 2, 0, 1, 2, 4, 1, 4, 3, 3]                      # first-endpoint incidences in item order, then second
    assert inc.inc_other.tolist() == [1, 2, 0, 2, 0, 3, 2, 2, 4, 4]                     # item 1 twice in node 2's list, item 3 twice in node 4's
    assert inc.piece_node.tolist() == [0, 1, 2, 2, 3, 4, 5] and inc.piece_ptr.tolist() == [0, 2, 3, 5, 7, 8, 10, 10]
    assert inc.piece_slot.tolist() == [-1, -1, 0, 1, -1, -1, -1]
    assert inc.hub_node.tolist() == [2] and inc.hub_slot_ptr.tolist() == [0, 2] and inc.hub_pieces == 2 and inc.n_pieces == 7
    node = ops.cls_incidence(torch.tensor([3, 1, 3, 3]), None, 5, piece=2)
    assert node.row_ptr.tolist() == [0, 0, 1, 1, 4, 4] and node.inc_item.tolist() == [1, 0, 2, 3]
    assert node.piece_node.tolist() == [0, 1, 2, 3, 3, 4] and node.piece_slot.tolist() == [-1, -1, -1, 0, 1, -1]
    big = ops.cls_incidence(torch.zeros(2 * ops.CLS_PULL_PIECE + 5, dtype=torch.int64), None, 2)
    assert big.piece_ptr.tolist() == [0, ops.CLS_PULL_PIECE, 2 * ops.CLS_PULL_PIECE, 2 * ops.CLS_PULL_PIECE + 5, 2 * ops.CLS_PULL_PIECE + 5]


def test_two_layer_head_raises():
    from ctgcn_amd import EdgeClassifier, MLPClassifier
    for cls in (MLPClassifier, EdgeClassifier):
        with pytest.raises(NotImplementedError, match="layer_num"):
            cls(128, 64, 4, 2, 3)


def test_cpu_tensors_raise():
    from ctgcn_amd import EdgeClassifier, InnerProduct, MLPClassifier
    from ctgcn_amd._lib import CtgcnHipError
    x = torch.zeros(5, 8)
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        MLPClassifier(8, 8, 3, 1, 1)(x, torch.tensor([0, 1]))
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        InnerProduct()(x, torch.tensor([[0, 1], [2, 3]]))
    with pytest.raises(CtgcnHipError, match="no CPU fallback"):
        EdgeClassifier(8, 8, 3, 1, 1)([x], [torch.tensor([[0, 1], [2, 3]])])
    assert InnerProduct(reduce=False).reduce is False


def test_has_cuda_false_raises(tmp_path):
    from ctgcn_amd import CTGCN, ClassificationLoss, MLPClassifier, SupervisedEmbedding
    from ctgcn_amd._lib import CtgcnHipError
    (tmp_path / "origin").mkdir()
    with pytest.raises(CtgcnHipError):
        SupervisedEmbedding(str(tmp_path), "origin", "emb", ["a", "b"], CTGCN(4, 8, 8, 1, 1, 2), ClassificationLoss(3),
                            MLPClassifier(8, 8, 3, 1, 2), has_cuda=False)


def test_new_symbols_and_workspace_sizes():
    import ctgcn_amd
    from ctgcn_amd import _lib, ops
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ctgcn_hip.h")).read()
    names = ["ctgcn_cls_pull_piece", "ctgcn_cls_check_items", "ctgcn_cls_head_fwd_f32", "ctgcn_cls_loss_workspace_bytes", "ctgcn_cls_loss_f32",
             "ctgcn_cls_head_bwd_workspace_bytes", "ctgcn_cls_head_bwd_f32"]
    for name in names:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31          # additive change
    assert lib.ctgcn_cls_pull_piece() == ops.CLS_PULL_PIECE
    assert lib.ctgcn_cls_loss_workspace_bytes(0) == 0 and lib.ctgcn_cls_loss_workspace_bytes(1) == 16
    assert lib.ctgcn_cls_loss_workspace_bytes(257) == 32 and lib.ctgcn_cls_loss_workspace_bytes(10 ** 9) == 1024 * 16
    small, hub = lib.ctgcn_cls_head_bwd_workspace_bytes(100, 128, 4, 0), lib.ctgcn_cls_head_bwd_workspace_bytes(100, 128, 4, 3)
    assert small > 0 and hub - small == 3 * 128 * 8
    assert lib.ctgcn_cls_head_bwd_workspace_bytes(100, 257, 4, 0) == 0 and lib.ctgcn_cls_head_bwd_workspace_bytes(100, 128, 33, 0) == 0
    for name in ("SupervisedEmbedding", "MLPClassifier", "InnerProduct", "EdgeClassifier", "ClassificationLoss", "StructureClassificationLoss"):
        assert name in ctgcn_amd.__all__ and hasattr(ctgcn_amd, name)
