"""CPU-only checks of the top-k link ranking: the C entries in the header and the binding, the driver's graph_recon task, and the
plain-torch metric functions of evaluation/graph_reconstruction.py on CPU tensors against hand-computed cases and the float64 model."""
import importlib
import json
import math
import os

import numpy as np
import pytest
import torch

import _topk_ref as R
from conftest import ROOT

from ctgcn_amd import _cdecl, _lib, main

GR = importlib.import_module("ctgcn_amd.evaluation.graph_reconstruction")      # the package exports the function of that name

HEADER = open(os.path.join(ROOT, "include", "ctgcn_topk.h")).read()         # the top-k entries have a header of their own
MAIN_HEADER = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
ENTRIES = ("ctgcn_topk_max_k", "ctgcn_topk_max_d", "ctgcn_topk_workspace_bytes", "ctgcn_topk_scores_f32")


# ------------------------------------------------------------------------------------ binding
def test_header_declares_the_entries_and_the_binding_exposes_them():
    funcs = _cdecl.functions(HEADER)
    for name in ENTRIES:
        assert name in funcs and name in _lib.TOPK_SIGNATURES
    assert len(funcs["ctgcn_topk_scores_f32"][1]) == 18 and funcs["ctgcn_topk_max_k"][1] == []
    consts = _cdecl.constants(HEADER)
    assert (_lib.TOPK_NO_SELF, _lib.TOPK_UPPER) == (consts["CTGCN_TOPK_NO_SELF"], consts["CTGCN_TOPK_UPPER"]) == (1, 2)
    assert sorted(funcs) == sorted(ENTRIES) and _lib.TOPK_SIGNATURES == funcs
    assert _cdecl.constants(MAIN_HEADER)["CTGCN_ABI_VERSION"] == 31 and not set(ENTRIES) & set(_lib.SIGNATURES)      # additive
    lib = _lib.load()
    assert lib.ctgcn_topk_max_k() >= 128 and lib.ctgcn_topk_max_d() >= 512
    assert lib.ctgcn_topk_workspace_bytes(10, 1000, 100, 1) == 0
    assert lib.ctgcn_topk_workspace_bytes(10, 1000, 100, 7) == 10 * 7 * 100 * 8
    assert lib.ctgcn_topk_workspace_bytes(1 << 24, 1 << 24, 128, 4) == (1 << 24) * 4 * 128 * 8        # 64-bit
    # refused before any launch, on a machine without a GPU too
    assert lib.ctgcn_topk_scores_f32(4, 4, 8, 0, None, 8, None, None, None, None, None, 0, 1, None, None, None, 0, None) == -1
    assert lib.ctgcn_topk_scores_f32(4, 4, 8, 129, None, 8, None, None, None, None, None, 0, 1, None, None, None, 0, None) == -4
    assert lib.ctgcn_topk_scores_f32(4, 4, 513, 4, None, 513, None, None, None, None, None, 0, 1, None, None, None, 0, None) == -4
    assert b"ctgcn_topk_max_d" in lib.ctgcn_last_error()


def test_source_is_built():
    from ctgcn_amd import build
    assert any(os.path.basename(s) == "ctgcn_topk.hip" for s in build.SRCS)


def test_cpu_tensors_are_refused():
    from ctgcn_amd import ops
    with pytest.raises(_lib.CtgcnHipError):
        ops.topk_scores(torch.zeros(4, 4), 2)


# ------------------------------------------------------------------------------------ dispatch
def test_main_sends_graph_recon_to_its_entry_with_its_section(tmp_path, monkeypatch):
    seen = []
    monkeypatch.setattr(GR, "graph_reconstruction", lambda args: seen.append(args))
    cfg = tmp_path / "c.json"
    cfg.write_text(json.dumps({"graph_recon": {"base_path": "x", "mode": "pred"}, "sim_pred": {"base_path": "y"}}))
    assert "graph_recon" in main.TASKS
    main.main(["prog", "--config", str(cfg), "--task", "graph_recon"])
    assert seen == [{"base_path": "x", "mode": "pred"}]
    with pytest.raises(AttributeError):
        main.main(["prog", "--config", str(cfg), "--task", "train"])


def test_driver_entry_reads_its_config_keys(tmp_path, monkeypatch):
    made = {}

    class Fake(object):
        def __init__(self, **kw):
            made.update(kw)

        def graph_reconstruction_all_method(self, method_list=None, worker=-1):
            made["method_list"] = method_list

    monkeypatch.setattr(GR, "GraphReconstructor", Fake)
    GR.graph_reconstruction({"base_path": "b", "origin_folder": "1.format", "embed_folder": "2.embedding", "graph_recon_res_folder": "3.out",
                             "node_file": "nodes.csv", "file_sep": "\t", "method_list": ["GCN"], "k_list": [5], "mode": "pred"})
    assert made == {"base_path": "b", "origin_folder": "1.format", "embedding_folder": "2.embedding", "output_folder": "3.out",
                    "node_file": "nodes.csv", "file_sep": "\t", "k_list": [5], "max_k": 100, "metric": "dot", "mode": "pred",
                    "method_list": ["GCN"]}


def test_constructor_refuses_unknown_mode_and_metric(tmp_path):
    (tmp_path / "nodes.csv").write_text("a\nb\n")
    for kw in ({"mode": "both"}, {"metric": "manhattan"}):
        with pytest.raises(ValueError):
            GR.GraphReconstructor(str(tmp_path), "o", "e", "r", "nodes.csv", **kw)


# ------------------------------------------------------------------------------------ metrics on CPU tensors
def _pattern(n, pairs):
    row_ptr, col = R.csr_from_pairs(n, pairs)
    return GR.Pattern(torch.from_numpy(row_ptr), torch.from_numpy(col))


def test_ranked_hits_by_hand():
    target = _pattern(5, [(0, 1), (0, 3), (2, 4), (4, 2), (3, 3)])
    index = torch.tensor([[1, 2, 3], [0, 2, -1], [4, -1, -1], [2, 4, 0]], dtype=torch.int32)
    hits = GR.ranked_hits(index, torch.tensor([0, 1, 2, 4]), target)
    assert hits.tolist() == [[True, False, True], [False, False, False], [True, False, False], [True, False, False]]
    assert GR.ranked_hits(index[:3], None, target).tolist() == [[True, False, True], [False, False, False], [True, False, False]]
    # index -1 is a miss even where (q, 0) is stored, and an empty target has no hits
    assert GR.ranked_hits(torch.tensor([[-1, 0]]), torch.tensor([4]), _pattern(5, [(4, 0), (3, 4)])).tolist() == [[False, True]]
    assert not GR.ranked_hits(index, torch.tensor([0, 1, 2, 4]), _pattern(5, [])).any()


def test_average_precision_by_hand():
    hits = torch.tensor([[1, 0, 1], [0, 0, 0], [1, 1, 1], [0, 1, 0]], dtype=torch.bool)
    n_rel = torch.tensor([2, 0, 5, 1])
    mean_ap, rows, ap = GR.average_precision(hits, n_rel, 3)
    assert ap[0].item() == (1 + 2 / 3) / 2                          # hits [1, 0, 1], n_rel = 2
    assert ap[2].item() == 3 / 3                                    # K = 3 < n_rel = 5: the denominator is K
    assert ap[3].item() == 0.5
    assert rows == 3 and abs(mean_ap - ((1 + 2 / 3) / 2 + 1.0 + 0.5) / 3) < 1e-15         # the n_rel = 0 row is left out, and counted out
    assert GR.average_precision(hits, n_rel, 2)[2].tolist() == [0.5, 0.0, 1.0, 0.5]
    ref_map, ref_rows = R.average_precision(hits.numpy(), n_rel.numpy(), 3)
    assert abs(mean_ap - ref_map) < 1e-15 and rows == ref_rows
    empty, rows0, _ = GR.average_precision(hits, torch.zeros(4, dtype=torch.int64), 3)
    assert math.isnan(empty) and rows0 == 0
    with pytest.raises(ValueError):
        GR.average_precision(hits, n_rel, 4)


def test_target_pattern_drops_the_diagonal_and_the_known():
    t = GR.target_pattern(_pattern(4, [(0, 0), (0, 1), (1, 0), (1, 2), (2, 1), (2, 3), (3, 2)]), _pattern(4, [(1, 2), (2, 1)]))
    assert t.row_ptr.tolist() == [0, 1, 2, 3, 4] and t.col.tolist() == [1, 0, 3, 2]


def _host_topk(X, k, rows=None, row_bias=None, col_bias=None, exclude_self=False, upper_only=False, exclude=None):
    """ops.topk_scores's signature on the float64 model"""
    ex = None if exclude is None else (exclude.row_ptr.numpy(), exclude.col.numpy())
    np_ = lambda t: None if t is None else t.numpy()
    s, i = R.topk(X.numpy(), k, np_(rows), np_(row_bias), np_(col_bias), exclude_self, upper_only, ex)
    _host_topk.widths.append(k)
    return torch.from_numpy(s.astype(np.float32)), torch.from_numpy(i)


def _hub_inputs(n):
    """(X, row_bias, col_bias): s(0, j) = 100 for every j > 0, s(i, j) = e_i e_j in [-16, 16] otherwise"""
    e = np.random.default_rng(2).integers(-4, 5, size=n).astype(np.float32)
    X = np.zeros((n, 2), dtype=np.float32)
    X[:, 0] = e
    X[0] = (0, 10)
    X[1:, 1] = 10
    X[0, 0] = 0
    # s(0, j) = 10 * 10 = 100; s(i, j) = e_i e_j + 100 for i, j >= 1: take the 100 back out with a row bias on the rows >= 1
    row_bias = np.full(n, -100, dtype=np.float32)
    row_bias[0] = 0
    return torch.from_numpy(X), torch.from_numpy(row_bias), None


def test_global_select_orders_pairs_and_certifies():
    # three rows of width 2; row 0 is full, rows 1 and 2 are not
    score = torch.tensor([[5.0, 3.0], [4.0, -math.inf], [-math.inf, -math.inf]])
    index = torch.tensor([[2, 1], [2, -1], [-1, -1]], dtype=torch.int32)
    i, j, ok = GR.global_select(score, index, 2)
    assert (i.tolist(), j.tolist(), ok) == ([0, 1], [2, 2], True)            # row 0's last entry (3.0) ranks third: after the 2nd pair
    i, j, ok = GR.global_select(score, index, 3)
    assert (i.tolist(), j.tolist(), ok) == ([0, 1, 0], [2, 2, 1], False)     # it IS the 3rd pair: more of row 0 may follow at 3.0
    assert GR.global_select(score, index, 4)[2] is False                     # fewer listed than asked for, and a full row
    # equal scores: i ascending, then j ascending
    score = torch.tensor([[1.0, 1.0, -math.inf], [1.0, -math.inf, -math.inf], [-math.inf] * 3])
    index = torch.tensor([[1, 2, -1], [2, -1, -1], [-1, -1, -1]], dtype=torch.int32)
    i, j, ok = GR.global_select(score, index, 10)
    assert (i.tolist(), j.tolist(), ok) == ([0, 0, 1], [1, 2, 2], True)      # no full row: everything admissible is listed


def test_global_precision_doubles_at_a_hub_and_matches_the_model():
    n = 40
    X, rb, cb = _hub_inputs(n)
    pairs = [(0, j) for j in range(1, n, 2)] + [(3, 7), (5, 9), (2, 30)]
    target = _pattern(n, pairs + [(c, r) for r, c in pairs])
    _host_topk.widths = []
    out = GR.global_precision(X, rb, cb, target, None, [5, 20, 30], width=8, topk=_host_topk)
    # 30 pairs asked for, all of them in row 0 (39 pairs at score 100): widths 8 and 16 are full at the threshold, 32 is not
    assert _host_topk.widths == [8, 16, 32] and out['width'] == 32 and out['doublings'] == 2
    S = R.scores(X.numpy(), None, rb.numpy(), None)
    up = R.admissible(n, None, False, True, None)
    assert [R.certified(S, up, w, 30) for w in (8, 16, 32)] == [False, False, True]
    gi, gj = R.global_pairs(S, up)
    T = R.targets(n, (target.row_ptr.numpy(), target.col.numpy()))
    for k in (5, 20, 30):
        assert out['pairs'][k] == k and out['precision'][k] == T[gi[:k], gj[:k]].sum() / k
    assert out['precision'][20] == 0.5                               # row 0's pairs in j order: every second one is an edge


def test_global_precision_refuses_at_the_limit():
    n = 40
    X, rb, cb = _hub_inputs(n)
    target = _pattern(n, [(0, 1), (1, 0)])
    _host_topk.widths = []
    with pytest.raises(ValueError, match="ctgcn_topk_max_k"):
        GR.global_precision(X, rb, cb, target, None, [30], width=8, max_width=16, topk=_host_topk)
    assert _host_topk.widths == [8, 16]


def test_global_precision_with_fewer_pairs_than_k_reports_the_denominator():
    n = 6
    X = torch.from_numpy(np.arange(12, dtype=np.float32).reshape(6, 2) % 5)
    known = _pattern(n, [(r, c) for r in range(n) for c in range(n) if (r + c) % 2 == 0])      # 6 of the 15 pairs are known
    target = _pattern(n, [(0, 1), (1, 0), (2, 5), (5, 2)])
    _host_topk.widths = []
    out = GR.global_precision(X, None, None, target, known, [4, 50], width=16, topk=_host_topk)
    assert out['pairs'] == {4: 4, 50: 9} and out['precision'][50] == 2 / 9


# ------------------------------------------------------------------------------------ score_inputs
def test_score_inputs_l2_biases_reproduce_the_distance():
    g = torch.Generator().manual_seed(1)
    E = torch.randn(30, 12, generator=g)
    X, rb, cb = GR.score_inputs(E, 'l2')
    assert X is not None and torch.equal(X, E) and rb.dtype == cb.dtype == torch.float32 and rb.shape == (30,)
    s = X.double() @ X.double().T + cb.double()[None, :] + rb.double()[:, None]
    want = -0.5 * ((E.double()[:, None, :] - E.double()[None, :, :]) ** 2).sum(-1)
    # each bias is one fp32 rounding of −‖e‖²/2: two of them a pair
    tol = 2.0 ** -24 * (0.5 * (E.double() ** 2).sum(1)[:, None] + 0.5 * (E.double() ** 2).sum(1)[None, :]) + 1e-12
    assert bool(((s - want).abs() <= tol).all())
    Xr, rbr, cbr = R.score_inputs(E.numpy(), 'l2')
    assert np.allclose(rb.numpy(), rbr, rtol=2.0 ** -23, atol=0)


def test_score_inputs_cosine_keeps_a_zero_row_zero_and_dot_is_the_input():
    E = torch.tensor([[3.0, 4.0], [0.0, 0.0], [0.0, -2.0]])
    X, rb, cb = GR.score_inputs(E, 'cosine')
    assert rb is None and cb is None and X.dtype == torch.float32
    assert X.tolist() == [[np.float32(0.6), np.float32(0.8)], [0.0, 0.0], [0.0, -1.0]]
    X, rb, cb = GR.score_inputs(E, 'dot')
    assert torch.equal(X, E) and rb is None and cb is None
    with pytest.raises(ValueError):
        GR.score_inputs(E, 'manhattan')
