"""The P-GNN baseline on the host, against the reference's recorded results (tests/golden/pgnn_uci.npz): the host model of the distance
pass equals the reference's dist_max / dist_argmax exactly; the float64 mirror reproduces its outputs, gradients and losses; the
modules have its state_dict keys and shapes and leave None the gradients it leaves None; the reference's dense [N, N] arrays through
get_dist_max give the same tensors; anchor-set counts and sizes; the C entry points' argument checks; the trainers' gates.  No kernel
runs here.

Tolerance per tensor (tests/test_gpu_gat.py's rule): the largest error over the tensor's largest magnitude may reach the larger of
4 x the reference's own float32-vs-float64 error and a floor of 2e-6 for outputs and losses, 1e-5 for gradients."""
import ctypes

import numpy as np
import pytest
import torch

import _pgnn_ref as P
from conftest import seeded_parameters

_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def share(what, got, ref, top, yard, floor):
    got, ref = np.asarray(got, dtype=np.float64).reshape(-1), np.asarray(ref, dtype=np.float64).reshape(-1)
    if top == 0.0:
        print("  [tol] %-46s the reference is exactly zero; largest |got| %.3e" % (what, float(np.abs(got).max(initial=0.0))))
        return 0.0 if not got.any() else float("inf")
    err = float(np.abs(got - ref).max(initial=0.0) / top)
    used = err / max(4 * float(yard), floor)
    print("  [tol] %-46s |err| / max|ref| %.3e  = %.3f of max(4 x %.3e, %g)" % (what, err, used, float(yard), floor))
    return used


def measure(g, key, got, yard, floor):
    ref, pick, top = stored(g, key)
    got = got.double().numpy().reshape(-1)
    return share(key, got if pick is None else got[pick], ref, top, yard, floor)


@pytest.mark.parametrize("cutoff", P.CUTOFFS)
@pytest.mark.parametrize("t", range(P.T))
def test_the_host_bfs_model_equals_the_reference_s_dist_max_and_dist_argmax(t, cutoff):
    g = P.fixture()
    sets = P.anchor_sets(g)
    assert len(sets) == 100 and [len(s) for s in sets[::10]] == [int(P.N / 2 ** (i + 1)) for i in range(10)]
    level, dist, pos, node = P.host_dist(*P.pattern(t), sets, cutoff)
    want_level, want_dist, want_pos = P.recorded_dist(g, t, cutoff)
    assert np.array_equal(level, want_level)
    assert np.array_equal(dist.view(np.uint32), want_dist.view(np.uint32))
    assert np.array_equal(pos.astype(np.int64), want_pos)
    members = [np.asarray(s) for s in sets]
    assert all(np.array_equal(node[:, a], members[a][pos[:, a]]) for a in range(len(sets)))
    assert (level < 0).any() and (cutoff > 0 or level.max() > 2)


def mirror_run(case):
    if case not in _runs:
        g = P.fixture()
        model = P.build(case, P.PgnnMirror)
        seeded_parameters(model, int(g["seed"]))
        model = model.double().train()
        dm, da = P.anchor_tensors(g)
        x = P.features(torch.float64)
        _runs[case] = P.adam_losses(model, lambda: model(x, dm, da), P.surrogate_weights(dm[0].shape[1], torch.float64))
    return _runs[case]


@pytest.mark.parametrize("case", P.CASES)
def test_the_float64_mirror_reproduces_the_reference(case):
    g = P.fixture()
    losses, (outs, grads) = mirror_run(case)
    used = {}
    for t in range(P.T):
        used["out_t%d" % t] = measure(g, "%s_out_t%d" % (case, t), outs[t], g[case + "_yard_out"][t], 2e-6)
    assert sorted(k for k in grads if grads[k] is None) == [str(k) for k in g[case + "_none_keys"]]
    assert sorted(k for k in grads if grads[k] is not None) == [str(k) for k in g[case + "_keys"]]
    for k, yard in zip(g[case + "_keys"], g[case + "_yard_grad"]):
        used["grad_" + str(k)] = measure(g, "%s_grad_%s" % (case, k), grads[str(k)], yard, 1e-5)
    used["losses"] = share(case + "_losses", losses, g[case + "_losses"], float(np.abs(g[case + "_losses"]).max()), g[case + "_yard_losses"], 2e-6)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "%s: share of the tolerance used %s" % (case, over)


@pytest.mark.parametrize("case", P.CASES)
def test_state_dict_keys_shapes_and_none_gradients_are_the_reference_s(case):
    import ctgcn_amd
    g = P.fixture()
    want = {str(k): tuple(int(s) for s in str(shape).split(",") if s) for k, shape in zip(g[case + "_state_keys"], g[case + "_state_shapes"])}
    for cls in (ctgcn_amd.PGNN, P.PgnnMirror):
        assert {k: tuple(v.shape) for k, v in P.build(case, cls).state_dict().items()} == want
    model = P.build(case, ctgcn_amd.PGNN)
    assert model.method_name == "PGNN" and model.anchor_node_ids is False
    assert sorted(k for k, _ in model.named_parameters()) == sorted([str(k) for k in g[case + "_keys"]] + [str(k) for k in g[case + "_none_keys"]])
    none = [str(k) for k in g[case + "_none_keys"]]
    if P.CASES[case][1]["layer_num"] > 1:                       # every layer but the last: its position output is never used
        assert none and all(".linear_out_position." in k and not k.startswith("conv_out.") for k in none)
    else:
        assert not none
    state = {k: torch.full(shape, 0.25) for k, shape in want.items()}
    model.load_state_dict(state, strict=True)


def test_initialisers_and_constructor_defaults_are_the_reference_s():
    import ctgcn_amd
    from ctgcn_amd.baseline.pgnn import Nonlinear, PGNN_layer
    torch.manual_seed(3)
    layer = PGNN_layer(8, 6)
    gain = torch.nn.init.calculate_gain("relu")
    for lin in (layer.linear_hidden, layer.linear_out_position, layer.dist_compute.linear1, layer.dist_compute.linear2):
        bound = gain * np.sqrt(6.0 / (lin.weight.shape[0] + lin.weight.shape[1]))
        top = float(lin.weight.detach().abs().max())
        assert 0.3 * bound < top <= bound and not lin.bias.any()
    assert tuple(layer.linear_hidden.weight.shape) == (6, 16) and tuple(layer.dist_compute.linear1.weight.shape) == (6, 1)
    assert not hasattr(PGNN_layer(8, 6, dist_trainable=False), "dist_compute")
    assert sorted(Nonlinear(1, 4, 1, bias=False).state_dict()) == ["linear1.weight", "linear2.weight"]
    model = ctgcn_amd.PGNN(10, 8, 6, 4)
    assert (model.feature_pre, model.layer_num, model.dropout, model.bias) == (True, 2, 0.5, True)
    assert len(model.conv_hidden) == 0 and tuple(model.conv_out.linear_hidden.weight.shape) == (4, 12)
    one = ctgcn_amd.PGNN(10, 8, 6, 4, layer_num=1)
    assert not hasattr(one, "conv_out") and tuple(one.conv_first.linear_hidden.weight.shape) == (4, 16)
    assert ctgcn_amd.baseline.PGNN is ctgcn_amd.PGNN


def test_the_reference_s_dense_arrays_through_get_dist_max_give_the_recorded_tensors():
    """the dense [N, N] matrix of 1 / (d + 1) that the reference's precompute_dist_data builds, here from scipy's BFS distances"""
    from scipy.sparse.csgraph import shortest_path
    from ctgcn_amd.baseline import get_dist_max
    g = P.fixture()
    sets = P.anchor_sets(g)
    dist = shortest_path(P.G.raw_csr(0), method="D", unweighted=True)
    for cutoff in P.CUTOFFS:
        dense = np.where(np.isfinite(dist) & ((cutoff <= 0) | (dist <= cutoff)), 1.0 / (dist + 1.0), 0.0)
        _, want_dist, want_pos = P.recorded_dist(g, 0, cutoff)
        dm, da = get_dist_max(sets, dense, "cpu")
        assert dm.dtype == torch.float32 and da.dtype == torch.int64
        assert np.array_equal(dm.numpy().view(np.uint32), want_dist.view(np.uint32)) and np.array_equal(da.numpy(), want_pos)
        dms, das = get_dist_max(sets, [dense], "cpu", node_ids=True)
        members = [np.asarray(s) for s in sets]
        assert isinstance(dms, list) and all(np.array_equal(das[0][:, a].numpy(), members[a][want_pos[:, a]]) for a in range(len(sets)))


@pytest.mark.parametrize("n", [2, 65, 1899, 87000])
def test_anchor_sets_have_the_reference_s_count_and_sizes(n):
    from ctgcn_amd.baseline import anchor_set_count, get_random_anchorset
    m = int(np.log2(n))
    for c in (0.5, 1):
        sets = get_random_anchorset(n, c=c, device="cpu")
        assert [len(s) for s in sets] == [int(n / np.exp2(i + 1)) for i in range(m) for _ in range(int(c * m))]
        assert len(sets) == anchor_set_count(n, c)
        assert all(len(torch.unique(s)) == len(s) and (len(s) == 0 or (int(s.min()) >= 0 and int(s.max()) < n)) for s in sets)
    assert anchor_set_count(1899) == 100 and anchor_set_count(87000) == 256 and anchor_set_count(1000000) == 361
    torch.manual_seed(11)
    first = get_random_anchorset(65, c=1, device="cpu")
    torch.manual_seed(11)
    assert all(torch.equal(a, b) for a, b in zip(first, get_random_anchorset(65, c=1, device="cpu")))


def test_the_torch_model_of_the_dropout_draw_equals_the_host_model():
    from ctgcn_amd import ops
    for key in (0, 1, 2 ** 62 - 5, 2 ** 64 - 1):
        assert np.array_equal(ops.dropout_keep_mask(key, 37, 19, 0.5, "cpu").numpy(), P.R.keep_mask(key, 37, 19, 0.5))


def test_the_entry_points_reject_bad_sizes_and_null_pointers():
    from ctgcn_amd import _lib
    lib = _lib.load()
    assert lib.ctgcn_abi_version() == _lib.ABI_VERSION == 31
    header = open(__file__.replace("tests/test_pgnn_host.py", "include/ctgcn_hip.h")).read()
    names = ["ctgcn_pgnn_dist_workspace_bytes", "ctgcn_pgnn_anchor_dist", "ctgcn_pgnn_conv_fwd_f32", "ctgcn_pgnn_bwd_row_workspace_bytes",
             "ctgcn_pgnn_conv_bwd_row_f32", "ctgcn_pgnn_bwd_pull_workspace_bytes", "ctgcn_pgnn_conv_bwd_pull_f32",
             "ctgcn_pgnn_table_grad_workspace_bytes", "ctgcn_pgnn_table_grad_f32"]
    for name in names:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    E_INVALID, E_WORKSPACE, E_UNSUPPORTED = -1, -3, -4
    p = ctypes.c_void_p(4096)            # never dereferenced: every call below is refused before a launch
    assert lib.ctgcn_pgnn_dist_workspace_bytes() >= 8
    dist = lambda n=5, nnz=4, rp=p, col=p, A=3, off=p, mem=p, nm=3, lvl=p, dm=p, pos=p, ws=p, wb=64: lib.ctgcn_pgnn_anchor_dist(  # noqa: E731
        n, nnz, rp, col, A, off, mem, nm, -1, lvl, dm, pos, None, None, ws, wb, None)
    assert dist(n=-1) == E_INVALID and dist(A=0) == E_INVALID and dist(nm=-1) == E_INVALID and dist(nnz=-1) == E_INVALID
    assert dist(n=2 ** 31) == E_INVALID and dist(n=2 ** 30, A=2) == E_UNSUPPORTED
    assert dist(rp=None) == E_INVALID and dist(col=None) == E_INVALID and dist(off=None) == E_INVALID and dist(mem=None) == E_INVALID
    assert dist(lvl=None) == E_INVALID and dist(dm=None) == E_INVALID and dist(pos=None) == E_INVALID
    assert dist(ws=None) == E_WORKSPACE and dist(wb=4) == E_WORKSPACE
    assert dist(n=0, rp=None, col=None, off=None, mem=None, lvl=None, dm=None, pos=None, ws=None) == 0
    assert b"ctgcn_pgnn_anchor_dist" in lib.ctgcn_last_error()
    fwd = lambda n=5, A=3, d=4, PS=p, ld=8, lvl=p, tab=p, U=2, idx=p, w=p, pos=p, st=p, lds=4, nrm=0, norm=p, pr=0.0: lib.ctgcn_pgnn_conv_fwd_f32(  # noqa: E731
        n, A, d, PS, ld, lvl, tab, U, idx, w, None, pos, st, lds, nrm, norm, pr, 0, None)
    assert fwd(n=-1) == E_INVALID and fwd(A=0) == E_INVALID and fwd(d=0) == E_INVALID and fwd(U=0) == E_INVALID and fwd(ld=7) == E_INVALID
    assert fwd(d=513, ld=1026) == E_UNSUPPORTED and fwd(n=2 ** 30, A=2) == E_UNSUPPORTED
    assert fwd(pr=1.0) == E_INVALID and fwd(pr=-0.1) == E_INVALID
    for name in ("PS", "lvl", "tab", "idx", "w"):
        assert fwd(**{name: None}) == E_INVALID
    assert fwd(pos=None, st=None) == E_INVALID and fwd(lds=3) == E_INVALID and fwd(nrm=1, norm=None) == E_INVALID
    assert fwd(n=0) == 0
    assert lib.ctgcn_pgnn_bwd_row_workspace_bytes(33, 7) == 3 * 8 * 4 and lib.ctgcn_pgnn_bwd_row_workspace_bytes(0, 7) == 0
    row = lambda n=5, A=3, d=4, gps=p, ldg=8, gd=p, gs=p, gse=p, gpos=p, ypos=p, nrm=1, gx=p, gw=p, ws=p, wb=1 << 20: lib.ctgcn_pgnn_conv_bwd_row_f32(  # noqa: E731
        n, A, d, p, 8, p, p, 2, p, p, gpos, ypos, nrm, gs, 4, 0.0, 0, gps, ldg, gd, gx, gse, 4, gw, p, ws, wb, None)
    assert row(n=-1) == E_INVALID and row(gps=None) == E_INVALID and row(gd=None) == E_INVALID and row(ldg=7) == E_INVALID
    assert row(gse=None) == E_INVALID and row(ypos=None) == E_INVALID and row(gx=None) == E_INVALID and row(gw=None) == E_INVALID
    assert row(ws=None) == E_WORKSPACE and row(wb=8) == E_WORKSPACE
    assert lib.ctgcn_pgnn_bwd_pull_workspace_bytes(3, 5) == 60
    pull = lambda n=5, np_=2, pieces=p, nm=1, mn=p, mp=p, rows=2, gps=p, ldg=8, ws=p, wb=1 << 20, perm=p: lib.ctgcn_pgnn_conv_bwd_pull_f32(  # noqa: E731
        n, 3, 4, p, 8, p, p, 2, p, p, p, 4, perm, pieces, np_, mn, mp, nm, rows, gps, ldg, ws, wb, None)
    assert pull(n=-1) == E_INVALID and pull(np_=-1) == E_INVALID and pull(pieces=None) == E_INVALID and pull(mn=None) == E_INVALID
    assert pull(mp=None) == E_INVALID and pull(gps=None) == E_INVALID and pull(ldg=7) == E_INVALID and pull(perm=None) == E_INVALID
    assert pull(ws=None) == E_WORKSPACE and pull(wb=8) == E_WORKSPACE and pull(n=0) == 0
    assert lib.ctgcn_pgnn_table_grad_workspace_bytes(6) == 24
    tab = lambda items=15, U=2, gd=p, perm=p, pieces=p, np_=2, pp=p, gt=p, ws=p, wb=64: lib.ctgcn_pgnn_table_grad_f32(  # noqa: E731
        items, U, gd, perm, pieces, np_, pp, gt, ws, wb, None)
    assert tab(items=-1) == E_INVALID and tab(U=0) == E_INVALID and tab(np_=-1) == E_INVALID
    for name in ("gd", "perm", "pieces", "pp", "gt"):
        assert tab(**{name: None}) == E_INVALID
    assert tab(ws=None) == E_WORKSPACE and tab(wb=4) == E_WORKSPACE


class _Foreign(torch.nn.Module):
    method_name = "PGNN"

    def forward(self, x, a, b):
        return x


def test_the_trainers_name_pgnn_refuse_a_foreign_module_and_need_node_dist_list(tmp_path):
    import ctgcn_amd
    from ctgcn_amd import embedding
    assert "PGNN" in embedding._SUPPORTED
    (tmp_path / "origin").mkdir()
    loss = ctgcn_amd.NegativeSamplingLoss.__new__(ctgcn_amd.NegativeSamplingLoss)
    torch.nn.Module.__init__(loss)
    for model, error in ((_Foreign(), NotImplementedError), (ctgcn_amd.PGNN(6, 4, 4, 4), None)):
        for trainer in ("UnsupervisedEmbedding", "SupervisedEmbedding"):
            if error is not None:
                with pytest.raises(error, match="ctgcn_amd.baseline.PGNN"):
                    embedding._check_own_baseline(trainer, model, "PGNN")
            else:
                embedding._check_own_baseline(trainer, model, "PGNN")
    with pytest.raises(ValueError, match="node_dist_list"):
        embedding._check_node_dist("PGNN", None)
    embedding._check_node_dist("GCN", None)
    embedding._check_node_dist("PGNN", [object()])
    doc = embedding.UnsupervisedEmbedding.learn_embedding.__doc__
    assert "PGNN" in doc and "unused here." not in doc
