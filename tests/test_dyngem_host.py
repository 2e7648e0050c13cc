"""Host checks of the DynGEM / DynAE baselines: the torch mirror (tests/_dyngem_ref.py) against the reference's recorded results
(tests/golden/dyngem_uci.npz), the generators' semantics on a 5-node window, the losses' host-side parts, the new C entry points'
declarations and argument checks, and the modules' interface and refusals.  No GPU needed."""
import ctypes
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import _dyngem_ref as D
from conftest import check_sampled_tensor, seeded_parameters

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ctgcn_rowsel_max_slots", "ctgcn_rowsel_conv_fwd_f32", "ctgcn_rowsel_bucket_f32", "ctgcn_wrecon_loss_workspace_bytes",
               "ctgcn_wrecon_loss_f32")
KEYS = sorted("%s.layer_list.%d.%s" % (m, i, p) for m in ("encoder", "decoder") for i in range(3) for p in ("weight", "bias"))
_runs = {}


def stored(g, key):
    if key in g.files:
        return g[key].astype(np.float64).reshape(-1), None, float(g[key + "__maxabs"])
    return g[key + "__vals"].astype(np.float64), g[key + "__pick"], float(g[key + "__maxabs"])


def mirror_run(method, dtype):
    if (method, dtype) not in _runs:
        g = D.fixture()
        if method == "dyngem":
            csr = D.stacked(D.dyngem_window())
            model = D.AeMirror(D.N, D.OUT, D.UNITS)
            xi, xj = D.dense_rows(csr, g["dyngem_i"], dtype)[:, 0], D.dense_rows(csr, g["dyngem_j"], dtype)[:, 0]
            values = torch.from_numpy(g["dyngem_w"]).to(dtype)
            c = D.DYNGEM
            step = lambda: D.dyngem_loss(model, xi, xj, values, c["alpha"], c["beta"], c["nu1"], c["nu2"])  # noqa: E731
        else:
            csr = D.stacked(D.dynae_window())
            model = D.AeMirror(D.N, D.OUT, D.UNITS, D.LOOK_BACK)
            idx, tgt = D.dynae_rows(g)
            x_pre, x_cur = D.dense_rows(csr, idx, dtype).reshape(D.BATCH, -1), D.dense_rows(csr, tgt, dtype)[:, 0]
            c = D.DYNAE
            step = lambda: D.dynae_loss(model, x_pre, x_cur, c["beta"], c["nu1"], c["nu2"])  # noqa: E731
        seeded_parameters(model, int(g["seed"]))
        model.to(dtype)
        _runs[(method, dtype)] = D.adam_run(model, step)
    losses, (hx, pred, grads) = _runs[(method, dtype)]
    return losses, hx, pred, grads


@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_mirror_float64_matches_the_reference(method):
    g = D.fixture()
    losses, hx, pred, grads = mirror_run(method, torch.float64)
    assert sorted(grads) == KEYS == [str(k) for k in g[method + "_keys"]] and len(KEYS) == 12
    for k, shape in zip(g[method + "_keys"], g[method + "_shapes"]):
        assert ",".join(str(s) for s in grads[str(k)].shape) == str(shape)
    check_sampled_tensor(g, method + "_hx", hx.numpy(), 1e-9, 1e-9)
    check_sampled_tensor(g, method + "_pred", pred.numpy(), 1e-9, 1e-9)
    for k in g[method + "_keys"]:
        check_sampled_tensor(g, "%s_grad_%s" % (method, k), grads[str(k)].numpy(), 1e-9, 1e-9)
    assert np.abs(np.asarray(losses) - g[method + "_losses"]).max() <= 1e-9 * np.abs(g[method + "_losses"]).max()
    # the recipe's condition on the seed: no dead ReLU stack, and records whose target row stores something
    assert len(g[method + "_active"]) == 6 and g[method + "_active"].min() >= 0.2 and g[method + "_active"].max() <= 0.8
    assert int(g["dynae_stored_targets"]) >= D.BATCH // 4


@pytest.mark.parametrize("method", ["dyngem", "dynae"])
def test_mirror_float32_is_within_twice_the_reference_s_own_float32_error(method):
    g = D.fixture()
    losses, hx, pred, grads = mirror_run(method, torch.float32)

    def worst(got, key):
        ref, pick, top = stored(g, key)
        got = got.double().numpy().reshape(-1)
        return np.abs((got if pick is None else got[pick]) - ref).max() / top

    assert worst(hx, method + "_hx") <= max(2 * float(g[method + "_yard_hx"]), 2e-7)
    assert worst(pred, method + "_pred") <= max(2 * float(g[method + "_yard_pred"]), 2e-7)
    for k, yard in zip(g[method + "_keys"], g[method + "_yard_grad"]):
        assert worst(grads[str(k)], "%s_grad_%s" % (method, k)) <= max(2 * yard, 1e-6), str(k)
    ref = g[method + "_losses"]
    assert np.abs(np.asarray(losses) - ref).max() <= max(2 * float(g[method + "_yard_losses"]), 2e-7) * np.abs(ref).max()


def test_the_fixture_weights_tell_weight_count_and_degree_apart():
    m = D.dyngem_window()[0]
    assert m.shape == (D.N, D.N) and np.diff(m.indptr).max() == 198 and set(np.unique(m.data)) == {1.0, 2.0, 3.0}
    assert (abs(m - m.T)).nnz == 0
    g = D.fixture()
    assert np.array_equal(np.asarray(m[g["dyngem_i"], g["dyngem_j"]]).reshape(-1), g["dyngem_w"])
    assert len(set(g["dyngem_i"].tolist() + g["dyngem_j"].tolist())) < 2 * D.BATCH          # a node occurs more than once in the batch


# ------------------------------------------------------------------------------------------------ generators
def tiny_window():
    """5 nodes, 3 snapshots; node 4 is isolated in snapshot 0, snapshot 2 stores a zero"""
    a = sp.csr_matrix(np.array([[0, 1, 0, 2, 0], [1, 0, 3, 0, 0], [0, 3, 0, 0, 0], [2, 0, 0, 0, 0], [0, 0, 0, 0, 0]], dtype=np.float64))
    b = sp.csr_matrix(np.array([[0, 0, 0, 0, 1], [0, 0, 2, 0, 0], [0, 2, 0, 1, 0], [0, 0, 1, 0, 0], [1, 0, 0, 0, 0]], dtype=np.float64))
    c = sp.csr_matrix((np.array([1.0, 0.0, 1.0]), (np.array([0, 1, 2]), np.array([2, 3, 0]))), shape=(5, 5))
    return [a, b, c]


def test_dynae_generator_pads_and_draws_afresh():
    from ctgcn_amd.baseline import BatchGenerator
    window = tiny_window()
    gen = BatchGenerator(list("abcde"), batch_size=4, look_back=2, beta=5.0, shuffle=False)
    assert gen.batch_num(window) == 2                                # 5 records (one trainable snapshot), 4 a batch
    it = gen.generate(window)
    first, second, third = next(it), next(it), next(it)
    assert first.host_idx.tolist() == [[0, 5], [1, 6], [2, 7], [3, 8]] and first.host_tgt.tolist() == [10, 11, 12, 13]
    assert second.host_idx.tolist() == [[4, 9], [-1, -1], [-1, -1], [-1, -1]] and second.host_tgt.tolist() == [14, -1, -1, -1]   # padding rows
    assert third.host_idx.tolist() == first.host_idx.tolist() and first.beta == 5.0
    # a fresh generator per batch, as learn_embedding makes one: shuffle=False repeats the first batch
    assert next(gen.generate(window)).host_idx.tolist() == first.host_idx.tolist()
    shuffled = BatchGenerator(list("abcde"), 4, 2, 5.0, shuffle=True)
    torch.manual_seed(3)
    a = next(shuffled.generate(window)).host_tgt.tolist()
    b = next(shuffled.generate(window)).host_tgt.tolist()
    torch.manual_seed(3)
    order = torch.randperm(5)                                        # drawn from torch's CPU generator, as epoch_order does
    assert a == (10 + order[:4]).tolist() and b == (10 + torch.randperm(5)[:4]).tolist() and a != b
    with pytest.raises(AssertionError):
        next(BatchGenerator(list("abcde"), 4, 3, 5.0).generate(window))          # no snapshot left to predict


def test_dyngem_generator_draws_stored_nonzero_entries():
    from ctgcn_amd.baseline import DynGEMBatchGenerator
    graph = tiny_window()[0]
    gen = DynGEMBatchGenerator(list("abcde"), batch_size=4, beta=10.0, shuffle=False)
    assert gen.batch_num(graph) == 2                                 # 6 stored entries
    it = gen.generate([graph])
    first, second = next(it), next(it)
    assert first.pairs == 4 and first.host_idx.tolist() == [0, 0, 1, 1, 1, 3, 0, 2] and first.host_values.tolist() == [1, 2, 1, 3]
    assert second.pairs == 2 and second.host_idx.tolist() == [2, 3, 1, 0]         # the last batch is not padded
    assert first.host_tgt is first.host_idx
    assert next(gen.generate(graph)).host_idx.tolist() == first.host_idx.tolist()
    zero = tiny_window()[2]
    assert DynGEMBatchGenerator(list("abcde"), 4, 10.0).batch_num(zero) == 1      # the stored zero is no entry: 2 elements
    assert sorted(next(DynGEMBatchGenerator(list("abcde"), 4, 10.0, shuffle=False).generate(zero)).host_idx.tolist()) == [0, 0, 2, 2]
    with pytest.raises(AssertionError):
        next(gen.generate(tiny_window()))                            # DynGEM trains on one snapshot


def test_the_embedding_term_is_the_product_of_two_means():
    """the reference multiplies [B] by [B, 1]: the mean of the [B, B] outer product.  baseline.dyngem.embedding_term, which both
    branches of DynGEMLoss call, gives that number and not the mean of the paired products"""
    from ctgcn_amd.baseline.dyngem import embedding_term
    gen = torch.Generator().manual_seed(2)
    hi, hj = torch.randn(7, 3, generator=gen, dtype=torch.float64), torch.randn(7, 3, generator=gen, dtype=torch.float64)
    w = torch.rand(7, 1, generator=gen, dtype=torch.float64) + 0.5
    outer = torch.sum(torch.square(hi - hj), dim=1) * w               # the reference's expression
    assert tuple(outer.shape) == (7, 7)
    paired = (torch.sum(torch.square(hi - hj), dim=1) * w.view(-1)).mean()
    for weights in (w, w.view(-1)):                                   # the composed path hands [B, 1], the kernel path [B]
        got = embedding_term(hi, hj, weights)
        assert got.dim() == 0 and abs(float(got) - float(outer.mean())) <= 1e-14 * float(outer.mean())
        assert abs(float(got) - float(paired)) > 1e-3 * float(paired)
    hi.requires_grad_(True)
    g, = torch.autograd.grad(embedding_term(hi, hj, w), hi)
    g_ref, = torch.autograd.grad((torch.sum(torch.square(hi - hj), dim=1) * w).mean(), hi)
    assert float((g - g_ref).abs().max()) <= 1e-14 * float(g_ref.abs().max())


def write_snapshot_files(folder, mats, names):
    """the snapshots as the reference's edge files (from_id, to_id, weight; every undirected edge once)"""
    os.makedirs(folder, exist_ok=True)
    for t, m in enumerate(mats):
        coo = sp.triu(m, k=1).tocoo()
        with open(os.path.join(folder, "2020-0%d.csv" % (t + 1)), "w") as fp:
            fp.write("from_id\tto_id\tweight\n")
            for i, j, w in zip(coo.row, coo.col, coo.data):
                fp.write("%s\t%s\t%s\n" % (names[i], names[j], repr(float(w))))


def test_a_window_from_the_data_loader_feeds_the_generators(tmp_path):
    """DataLoader.get_date_adj_list(..., data_type='matrix') is what the reference's driver hands the trainer"""
    from ctgcn_amd import DataLoader
    from ctgcn_amd.baseline import BatchGenerator, DynGEMBatchGenerator
    mats = [m for m in tiny_window()]
    mats[2] = sp.csr_matrix(np.array([[0, 0, 1, 0, 0], [0, 0, 0, 2, 0], [1, 0, 0, 0, 0], [0, 2, 0, 0, 3], [0, 0, 0, 3, 0]], dtype=np.float64))
    names = list("abcde")
    write_snapshot_files(str(tmp_path / "origin"), mats, names)
    window = DataLoader(names, 3).get_date_adj_list(str(tmp_path / "origin"), start_idx=0, duration=3, data_type='matrix')
    assert len(window) == 3 and all(sp.issparse(w) and (abs(sp.csr_matrix(w) - m)).nnz == 0 for w, m in zip(window, mats))
    same = lambda a, b: a.host_idx.tolist() == b.host_idx.tolist() and np.array_equal(a.host_tgt, b.host_tgt)  # noqa: E731
    gen = BatchGenerator(names, 4, 2, 5.0, shuffle=False)
    assert gen.batch_num(window) == 2 and same(next(gen.generate(window)), next(gen.generate(mats)))
    gem = DynGEMBatchGenerator(names, 4, 10.0, shuffle=False)
    a, b = next(gem.generate(window[:1])), next(gem.generate(mats[:1]))
    assert same(a, b) and a.host_values.tolist() == b.host_values.tolist() == [1, 2, 1, 3]


def test_regularization_loss_edge_cases():
    from ctgcn_amd.baseline import RegularizationLoss
    from ctgcn_amd.baseline.dynae import MLP
    model = MLP(5, 2, [4, 3]).double()
    seeded_parameters(model, 5)
    weights = [p for n, p in model.named_parameters() if "weight" in n]
    assert [n for n, _ in RegularizationLoss.get_weight(model)] == ["layer_list.%d.weight" % i for i in range(3)]
    zero = RegularizationLoss(0., 0.)(model)
    assert tuple(zero.shape) == (1,) and float(zero) == 0.0
    l1 = float(RegularizationLoss(0.5, 0.)(model))
    l2 = float(RegularizationLoss(0., 0.25)(model))
    both = RegularizationLoss(0.5, 0.25)(model)
    assert abs(l1 - 0.5 * sum(float(p.abs().sum()) for p in weights) / 3) <= 1e-12
    assert abs(l2 - 0.25 * sum(float(p.pow(2).sum().sqrt()) for p in weights) / 3) <= 1e-12      # the unsquared 2-norm
    assert abs(float(both) - l1 - l2) <= 1e-12 and both.dim() == 0
    assert abs(float(D.regularization(model, 0.5, 0.25)) - float(both)) <= 1e-12
    both.backward()
    assert all(p.grad is None for n, p in model.named_parameters() if "bias" in n)


# ------------------------------------------------------------------------------------------------ the library and the interface
def test_new_symbols_are_declared_bound_and_additive():
    from ctgcn_amd import _lib, build
    lib = _lib.load()
    header = open(os.path.join(ROOT, "include", "ctgcn_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in _lib.SIGNATURES and hasattr(lib, name)
    assert "#define CTGCN_ABI_VERSION 31" in header and lib.ctgcn_abi_version() == 31 and _lib.ABI_VERSION == 31
    assert any(os.path.basename(s) == "ctgcn_dyngem.hip" for s in build.SRCS)
    assert lib.ctgcn_rowsel_max_slots() == 64


def test_entry_points_reject_invalid_arguments():
    from ctgcn_amd import _lib
    lib = _lib.load()
    INVALID, WORKSPACE, UNSUPPORTED = -1, -3, -4
    p = ctypes.c_void_p(64)          # never dereferenced: every call below fails its argument checks before any launch

    def conv(n=4, slots=1, d=8, idx=p, rp=p, col=p, val=p, S=p, lds=8, cs=0, epi=1, Y=p, ldy=8, lp=None, nl=0, thr=8, ws=None, wsb=0):
        return lib.ctgcn_rowsel_conv_fwd_f32(n, slots, d, idx, rp, col, val, S, lds, cs, None, epi, Y, ldy, lp, nl, thr, ws, wsb, None)

    assert conv(n=-1) == INVALID and conv(n=2 ** 31) == INVALID and conv(d=0) == INVALID
    assert conv(slots=0) == INVALID and conv(slots=65) == INVALID and conv(epi=2) == INVALID and conv(cs=-1) == INVALID
    assert conv(lds=7) == INVALID and conv(ldy=7) == INVALID
    for name in ("idx", "rp", "col", "val", "S", "Y"):
        assert conv(**{name: None}) == INVALID, name
    assert conv(nl=1, lp=None) == INVALID and conv(nl=5, lp=p) == INVALID
    assert conv(nl=1, lp=p, thr=0, ws=p, wsb=1 << 20) == INVALID
    assert conv(nl=1, lp=p, ws=None, wsb=0) == WORKSPACE and conv(nl=1, lp=p, ws=p, wsb=16) == WORKSPACE
    assert conv(n=70000, nl=65536, lp=p, ws=p, wsb=1 << 30) == UNSUPPORTED
    assert conv(n=0) == 0
    assert b"rowsel_conv_fwd" in lib.ctgcn_last_error()

    def bucket(rows=4, d=8, ip=p, pos=p, G=p, ldg=8, out=p, ldo=8):
        return lib.ctgcn_rowsel_bucket_f32(rows, d, ip, pos, G, ldg, out, ldo, None)

    assert bucket(rows=-1) == INVALID and bucket(rows=2 ** 31) == INVALID and bucket(d=0) == INVALID
    assert bucket(ldg=7) == INVALID and bucket(ldo=7) == INVALID
    for name in ("ip", "pos", "G", "out"):
        assert bucket(**{name: None}) == INVALID, name
    assert bucket(rows=0) == 0
    assert b"rowsel_bucket" in lib.ctgcn_last_error()

    def loss(n=4, w=8, Z=p, ldz=8, tgt=p, ep=p, ent=10, rp=p, col=p, val=p, relu=1, dZ=p, lddz=8, out=p, ws=p, wsb=1 << 10):
        return lib.ctgcn_wrecon_loss_f32(n, w, Z, ldz, tgt, ep, ent, rp, col, val, 2.0, None, 1.0, relu, dZ, lddz, out, ws, wsb, None)

    assert loss(n=-1) == INVALID and loss(n=2 ** 31) == INVALID and loss(w=0) == INVALID and loss(ent=-1) == INVALID
    assert loss(relu=2) == INVALID and loss(ldz=7) == INVALID and loss(lddz=7) == INVALID and loss(out=None) == INVALID
    for name in ("Z", "tgt", "ep", "rp", "col", "val"):
        assert loss(**{name: None}) == INVALID, name
    assert loss(ws=None, wsb=0) == WORKSPACE and loss(ws=ctypes.c_void_p(68)) == WORKSPACE
    assert loss(wsb=32 + 40 - 1) == WORKSPACE                         # 4 row sums (rounded up to 32 bytes) and 10 staged values
    assert b"wrecon_loss" in lib.ctgcn_last_error()
    assert lib.ctgcn_wrecon_loss_workspace_bytes(4, 10) == 72 and lib.ctgcn_wrecon_loss_workspace_bytes(3, 0) == 32
    assert lib.ctgcn_wrecon_loss_workspace_bytes(-1, 0) == 0


def test_interface_state_dict_keys_and_refusals(tmp_path):
    import ctgcn_amd
    from ctgcn_amd import _lib, baseline, layers, ops
    from ctgcn_amd.baseline import dynae, dyngem
    for name in ("DynAE", "RegularizationLoss", "DynGraph2VecLoss", "BatchGenerator", "BatchPredictor", "DynamicEmbedding", "DynGEM", "DynGEMLoss",
                 "DynGEMBatchGenerator", "DynGEMBatchPredictor"):
        assert name in ctgcn_amd.__all__ and getattr(ctgcn_amd, name) is getattr(baseline, name)
    assert ctgcn_amd.MLP is layers.MLP and dynae.MLP is not layers.MLP and dyngem.MLP is dynae.MLP
    g = D.fixture()
    gem = ctgcn_amd.DynGEM(input_dim=D.N, output_dim=D.OUT, n_units=D.UNITS, bias=True, look_back=0, ae_units=[], rnn_units=[])
    ae = ctgcn_amd.DynAE(input_dim=D.N, output_dim=D.OUT, look_back=D.LOOK_BACK, n_units=D.UNITS, bias=True, ae_units=[], rnn_units=[])
    assert gem.method_name == "DynGEM" and ae.method_name == "DynAE" and ae.look_back == D.LOOK_BACK
    for model, method in ((gem, "dyngem"), (ae, "dynae")):
        state = model.state_dict()
        assert sorted(state) == KEYS == [str(k) for k in g[method + "_keys"]]
        for k, shape in zip(g[method + "_keys"], g[method + "_shapes"]):
            assert ",".join(str(s) for s in state[str(k)].shape) == str(shape)
        mirror = D.AeMirror(D.N, D.OUT, D.UNITS, D.LOOK_BACK if method == "dynae" else 1)
        mirror.load_state_dict(state)                                 # checkpoints move both ways
        model.load_state_dict(mirror.state_dict())
    assert tuple(ae.encoder.layer_list[0].weight.shape) == (24, 2 * D.N) and tuple(ae.decoder.layer_list[2].weight.shape) == (D.N, 24)
    assert not ctgcn_amd.DynGEM(6, 2, n_units=[3], bias=False).state_dict().keys() - {"encoder.layer_list.0.weight", "encoder.layer_list.1.weight",
                                                                                    "decoder.layer_list.0.weight", "decoder.layer_list.1.weight"}
    # CPU tensors
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        gem(torch.zeros(2, D.N))
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ctgcn_amd.DynGraph2VecLoss(5.0, 0., 0.)(ae, [torch.zeros(2, 3), torch.zeros(2, 3), torch.ones(2, 3)])
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ctgcn_amd.DynGEMLoss(0.5, 10.0, 0., 0.)(gem, [torch.zeros(2, 4)] * 9)
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.SnapshotRows(tiny_window(), "cpu")
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ctgcn_amd.DynGEMBatchPredictor(list("abcde"), 4).predict(ctgcn_amd.DynGEM(5, 2, n_units=[3]), tiny_window()[0])
    fake = type("Rows", (), {"val": torch.zeros(1)})()
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.rowsel_conv(torch.zeros(5, 4), fake, [0, 1])
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ops.wrecon_loss(torch.zeros(2, 5), fake, [0, 1], 2.0)
    # the trainer: has_cuda=False, a foreign module
    (tmp_path / "origin").mkdir()
    nodes = list("abcde")
    args = (str(tmp_path), "origin", "emb", nodes)
    gen, pred = ctgcn_amd.DynGEMBatchGenerator(nodes, 4, 10.0), ctgcn_amd.DynGEMBatchPredictor(nodes, 4)
    with pytest.raises(_lib.CtgcnHipError, match="no CPU fallback"):
        ctgcn_amd.DynamicEmbedding(*args, ctgcn_amd.DynGEM(5, 2, n_units=[3]), ctgcn_amd.DynGEMLoss(0.5, 10.0, 0., 0.), gen, pred, has_cuda=False)

    class Foreign(torch.nn.Module):
        method_name = "DynGEM"

    with pytest.raises(NotImplementedError, match="ctgcn_amd.baseline.DynGEM"):
        ctgcn_amd.DynamicEmbedding(*args, Foreign(), ctgcn_amd.DynGEMLoss(0.5, 10.0, 0., 0.), gen, pred, has_cuda=True)
