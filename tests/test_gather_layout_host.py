"""Host side of the gather layout (no GPU needed): ops.to_gather_layout re-lays a Linear weight [out, N] in place as the .t() view of a
contiguous [N, out] buffer.  Shape, values and the state_dict entry stay what they were; checkpoints written before the switch load after
it and the other way round; deepcopy keeps the layout; an optimizer step on the re-laid parameter equals the step on a row-major copy."""
import copy
import io

import torch

from ctgcn_amd import CTGCN, MLP, ops

N, HID = 23, 12


def _mlp(seed=0):
    torch.manual_seed(seed)
    return MLP(N, 7, HID, 1, activate_type='L')


def test_the_switch_keeps_the_parameter_its_shape_and_its_values():
    mlp = _mlp()
    p = mlp.linear.weight
    want = p.detach().clone()
    assert not ops.in_gather_layout(p)
    assert ops.to_gather_layout(p) is p and mlp.linear.weight is p and isinstance(p, torch.nn.Parameter) and p.requires_grad
    assert tuple(p.shape) == (HID, N) and tuple(p.stride()) == (1, HID) and p.t().is_contiguous() and ops.in_gather_layout(p)
    sd = mlp.state_dict()
    assert sorted(sd) == ["linear.bias", "linear.weight"] and tuple(sd["linear.weight"].shape) == (HID, N)
    assert torch.equal(sd["linear.weight"], want) and torch.equal(sd["linear.weight"].contiguous(), want)
    ptr = p.data_ptr()
    ops.to_gather_layout(p)                                  # idempotent: no second copy
    assert p.data_ptr() == ptr


def test_seeded_initial_weights_do_not_depend_on_the_switch():
    a, b = _mlp(5), _mlp(5)
    ops.to_gather_layout(b.linear.weight)
    assert torch.equal(a.linear.weight, b.linear.weight) and torch.equal(a.linear.bias, b.linear.bias)


def test_checkpoints_cross_the_switch_in_both_directions():
    old = _mlp(1)
    blob = io.BytesIO()
    torch.save(old.state_dict(), blob)                       # saved before the switch
    new = _mlp(2)
    ops.to_gather_layout(new.linear.weight)
    blob.seek(0)
    new.load_state_dict(torch.load(blob))
    assert torch.equal(new.linear.weight, old.linear.weight) and ops.in_gather_layout(new.linear.weight)      # layout kept, values loaded
    blob = io.BytesIO()
    torch.save(new.state_dict(), blob)                       # saved after the switch
    blob.seek(0)
    fresh = _mlp(3)
    fresh.load_state_dict(torch.load(blob))
    assert torch.equal(fresh.linear.weight, old.linear.weight) and fresh.linear.weight.is_contiguous()


def test_deepcopy_and_to_keep_the_layout():
    mlp = _mlp()
    ops.to_gather_layout(mlp.linear.weight)
    twin = copy.deepcopy(mlp)
    assert ops.in_gather_layout(twin.linear.weight) and torch.equal(twin.linear.weight, mlp.linear.weight)
    assert twin.linear.weight.data_ptr() != mlp.linear.weight.data_ptr()
    moved = copy.deepcopy(mlp).to(torch.float64).to(torch.float32)
    assert ops.in_gather_layout(moved.linear.weight) and torch.equal(moved.linear.weight, mlp.linear.weight)


def test_an_adam_step_on_the_relaid_parameter_equals_the_step_on_a_row_major_copy():
    a, b = _mlp(4), _mlp(4)
    ops.to_gather_layout(b.linear.weight)
    opts = [torch.optim.Adam(m.parameters(), lr=1e-2, weight_decay=1e-3) for m in (a, b)]
    g = torch.Generator().manual_seed(9)
    for _ in range(3):
        rows = torch.randn(N, HID, generator=g)             # the gradient as the aggregation's backward delivers it: [N, out] rows
        for m, opt in zip((a, b), opts):
            opt.zero_grad(set_to_none=True)
            m.linear.weight.grad = rows.t() if m is b else rows.t().contiguous()
            m.linear.bias.grad = rows.sum(0)
            opt.step()
        assert torch.equal(a.linear.weight, b.linear.weight) and torch.equal(a.linear.bias, b.linear.bias)
    assert ops.in_gather_layout(b.linear.weight) and a.linear.weight.is_contiguous()


def test_autograd_hands_the_relaid_parameter_its_gradient_by_value():
    a, b = _mlp(6), _mlp(6)
    ops.to_gather_layout(b.linear.weight)
    coef = torch.arange(N * HID, dtype=torch.float32).reshape(N, HID) / 7
    for m in (a, b):
        (m.linear.weight.t() * coef).sum().backward()
    assert torch.equal(a.linear.weight.grad, b.linear.weight.grad) and torch.equal(b.linear.weight.grad, coef.t())


def test_dense_features_through_a_relaid_linear_give_the_same_bits():
    mlp = _mlp(7)
    x = torch.randn(9, N)
    with torch.no_grad():
        want = mlp(x)
        ops.to_gather_layout(mlp.linear.weight)
        assert torch.equal(mlp(x), want)
    eye = torch.sparse_coo_tensor(torch.arange(N).repeat(2, 1), torch.ones(N), (N, N))
    with torch.no_grad():
        assert torch.equal(mlp(eye), mlp.linear.weight.t() + mlp.linear.bias)


def test_the_gather_operand_is_offered_only_where_nobody_else_reads_the_mlp_output(monkeypatch):
    eye = torch.sparse_coo_tensor(torch.arange(N).repeat(2, 1), torch.ones(N), (N, N))
    model = CTGCN(N, HID, 8, 1, 2, 2)
    assert model.gather_operand(0, eye) is None               # host tensors: the kernels that gather run on the device only
    assert model.gather_operand(0, torch.randn(N, N)) is None
    assert not ops.in_gather_layout(model.mlp_list[0].linear.weight)
    for kw in (dict(model_type='S'), dict(trans_activate_type='N')):
        other = CTGCN(N, HID, 8, 1, 2, 2, **kw)
        assert other.gather_operand(0, eye) is None
    assert CTGCN(N, HID, 8, 2, 2, 2).gather_operand(0, eye) is None          # two transform layers
    monkeypatch.setenv("CTGCN_LINEAR_GATHER", "0")
    assert not ops.linear_gather_enabled()
    monkeypatch.delenv("CTGCN_LINEAR_GATHER")
    assert ops.linear_gather_enabled()
