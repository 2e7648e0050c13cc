"""ctgcn_amd.baseline.DynRNN / DynAERNN on the GPU against the reference's recorded float64 results (tests/golden/dynrnn_uci.npz), through
DynamicEmbedding.get_model_res and DynGraph2VecLoss, by tests/test_gpu_vgrnn.py's rule: error <= max(4 x the stored yardstick, 2e-6)
max|ref| for outputs and losses, 1e-5 for gradients.  The kernel path (row gathers, ops.lstm_layer, ops.wrecon_loss) and the composed
path (dense [B, L, N] rows through nn.LSTM / nn.Linear and the dense loss) are held to it separately.  CTGCN_PARITY_OUT=<dir> keeps the
shares of the tolerance used."""
import numpy as np
import pytest
import torch

import _dyngem_ref as D
import _dynrnn_ref as R
from conftest import seeded_parameters

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_runs = {}


def rows_of():
    from ctgcn_amd import ops
    if "rows" not in _runs:
        _runs["rows"] = ops.SnapshotRows(R.window(), DEV)
    return _runs["rows"]


def build(method, seed=None, bias=True):
    import ctgcn_amd
    if method == "dynrnn":
        model = ctgcn_amd.DynRNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, n_units=R.UNITS, bias=bias)
    else:
        model = ctgcn_amd.DynAERNN(input_dim=R.N, output_dim=R.OUT, look_back=R.LOOK_BACK, ae_units=R.UNITS, rnn_units=R.RNN_UNITS, bias=bias)
    seeded_parameters(model, int(R.fixture()["seed"]) if seed is None else seed)
    return model.to(DEV).train()


def fixture_batch():
    from ctgcn_amd.baseline.dynae import RowBatch
    idx, tgt = R.batch_rows(R.fixture())
    return RowBatch(rows_of(), idx, tgt, R.BETA)


def step_fn(method, model, fused):
    """forward_loss() -> (loss, embedding, prediction) through the trainer's own get_model_res"""
    import ctgcn_amd
    loss_fn = ctgcn_amd.DynGraph2VecLoss(R.BETA, R.NU1, R.NU2)
    batch = fixture_batch()

    def forward_loss():
        res = ctgcn_amd.DynamicEmbedding.get_model_res(model, iter([batch]), fused)
        assert len(res) == (2 if fused else 3)
        if fused:                                                    # a copy, made before the loss consumes z
            pred = res[0].detach().clone() if method == "dynrnn" else torch.relu(res[0].detach())
        else:
            pred = res[0]
        with torch.no_grad():                                        # the step does not keep the embedding
            if fused:
                hx = model.encode(batch)[1] if method == "dynrnn" else model.encode(batch)
            else:
                x = batch.dense()[0].view(R.BATCH, R.LOOK_BACK, R.N)
                hx = model.encoder(x)[1] if method == "dynrnn" else model.rnn_encoder(model.ae_encoder(x))[1]
        return loss_fn(model, res), hx, pred

    return forward_loss


def gpu_run(method, fused):
    if (method, fused) not in _runs:
        model = build(method)
        losses, (hx, pred, grads) = D.adam_run(model, step_fn(method, model, fused))
        _runs[(method, fused)] = (losses, hx.cpu(), pred.cpu(), {k: v.cpu() for k, v in grads.items()})
    return _runs[(method, fused)]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "composed"])
@pytest.mark.parametrize("method", R.METHODS)
def test_outputs_gradients_and_losses_match_the_reference(method, fused):
    g = R.fixture()
    losses, hx, pred, grads = gpu_run(method, fused)
    assert sorted(grads) == [str(k) for k in g[method + "_keys"]]
    used = {"hx": R.share_used(g, method + "_hx", hx, g[method + "_yard_hx"], 2e-6),
            "pred": R.share_used(g, method + "_pred", pred, g[method + "_yard_pred"], 2e-6)}
    for k, yard in zip(g[method + "_keys"], g[method + "_yard_grad"]):
        used["grad_" + str(k)] = R.share_used(g, "%s_grad_%s" % (method, k), grads[str(k)], yard, 1e-5)
    ref = g[method + "_losses"]
    err = float(np.abs(np.asarray(losses) - ref).max() / np.abs(ref).max())
    used["losses"] = err / max(4 * float(g[method + "_yard_losses"]), 2e-6)
    print("  [tol] %-58s |err| / max|ref| %.3e  = %.3f of the tolerance" % (method + " losses", err, used["losses"]))
    R.record_parity("%s_%s" % (method, "fused" if fused else "composed"), used)
    over = {k: round(v, 3) for k, v in used.items() if not v <= 1.0}
    assert not over, "share of the tolerance used %s" % over


@pytest.mark.parametrize("method", R.METHODS)
def test_a_fused_training_step_is_bit_identical_when_run_twice(method):
    def run():
        torch.manual_seed(77)
        model = build(method)
        losses, (hx, pred, grads) = D.adam_run(model, step_fn(method, model, True), steps=2)
        return losses, hx, pred, grads

    a, b = run(), run()
    assert a[0] == b[0] and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    assert all(torch.equal(a[3][k], b[3][k]) for k in a[3]) and all(float(v.abs().max()) > 0 for v in a[3].values())


@pytest.mark.parametrize("method", R.METHODS)
def test_bias_free_models_agree_between_the_paths(method):
    """bias=False: the kernel path against the composed one on the fixture's batch, by the fixture's rule for the prediction"""
    g = R.fixture()
    model = build(method, bias=False)
    batch = fixture_batch()
    with torch.no_grad():
        hx, x = model(batch)
        hx_c, x_c = model(batch.dense()[0].view(R.BATCH, R.LOOK_BACK, R.N))
    tol_h, tol_x = max(4 * float(g[method + "_yard_hx"]), 2e-6), max(4 * float(g[method + "_yard_pred"]), 2e-6)
    assert float((hx - hx_c).abs().max()) <= tol_h * float(hx_c.abs().max()) and float(hx_c.abs().max()) > 0
    assert float((x - x_c).abs().max()) <= tol_x * float(x_c.abs().max()) and float(x_c.abs().max()) > 0


@pytest.mark.parametrize("method", R.METHODS)
def test_predictor_and_the_forms_of_a_batch(method):
    import ctgcn_amd
    g = R.fixture()
    model = build(method)
    rows = rows_of()
    start = rows.T - R.LOOK_BACK
    pred = ctgcn_amd.BatchPredictor(list(range(R.N)), 700)            # 1899 nodes: two full batches and a remainder
    emb, x_pred = pred.predict(model, rows, start=start)
    emb_c, x_pred_c = pred.predict(model, rows, fused=False, start=start)
    only, none = pred.predict(model, rows, need_pred=False, start=start)
    only_c, none_c = pred.predict(model, rows, need_pred=False, fused=False, start=start)
    assert tuple(emb.shape) == (R.N, R.OUT) and tuple(x_pred.shape) == (R.N, R.N) and none is None and none_c is None
    assert torch.equal(only, emb) and torch.equal(only_c, emb_c)
    tol_h, tol_x = max(4 * float(g[method + "_yard_hx"]), 2e-6), max(4 * float(g[method + "_yard_pred"]), 2e-6)
    assert float((emb - emb_c).abs().max()) <= tol_h * float(emb_c.abs().max())
    assert float((x_pred - x_pred_c).abs().max()) <= tol_x * float(x_pred_c.abs().max())
    batch = fixture_batch()
    with torch.no_grad():
        hx, x = model(batch)                                         # a RowBatch and (SnapshotRows, idx) agree to the bit
        hx2, x2 = model((rows, batch.host_idx))
    assert torch.equal(hx, hx2) and torch.equal(x, x2)
    if method == "dynaernn":
        with pytest.raises(ValueError, match="look_back 3"):
            pred.predict(model, rows, start=start - 1)                # a window of 4 snapshots
    else:                                                            # DynRNN's reconstruction comes from the sequence, not from hx
        with torch.no_grad():
            seq, hx3 = model.encode(batch)
            assert torch.equal(model.decode(seq), x) and tuple(seq.shape) == (R.BATCH, R.LOOK_BACK, R.OUT) and torch.equal(hx3, seq[:, -1])
