"""ParamBucket alone (ick_amd/bucket.py), on the CPU and without the built library: the layout at the sizes where the
64-float padding rule can go wrong, adoption, slots, torch.optim.Adam's state layout both ways, the tensor list, the
exchange with the average and the residency check."""
import pytest
import torch

from ick_amd.bucket import ParamBucket

SHAPES = [(1,), (63,), (64,), (65,), (3, 5)]
OFFSETS = [0, 64, 128, 192, 320, 384]           # 1 -> 64, 63 -> 64, 64 -> 64, 65 -> 128, 15 -> 64 floats


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def make(average=False, seed=0):
    g = torch.Generator().manual_seed(seed)
    params = [torch.nn.Parameter(torch.randn(s, generator=g)) for s in SHAPES]
    values = [p.detach().clone() for p in params]
    b = ParamBucket(params)
    if average:
        b.start_average()
    return b, params, values, g


def pad_mask(b):
    mask = torch.ones(b.n, dtype=torch.bool)
    for p in b.params:
        b.slot(mask, p).fill_(False)
    return mask


def test_layout_adoption_and_slots():
    b, params, values, g = make(average=True)
    assert b.offsets == OFFSETS and all(o % 64 == 0 for o in b.offsets)
    assert b.n == OFFSETS[-1] == sum((p.numel() + 63) // 64 * 64 for p in params)
    assert [t.numel() for t in (b.p, b.m, b.v, b.e)] == [b.n] * 4 and b.p.dtype == torch.float32
    for p, off, val in zip(params, b.offsets, values):
        assert p.data_ptr() == b.p.data_ptr() + 4 * off and p.shape == val.shape and p.is_contiguous()
        assert same_bits(p.detach(), val)
        assert same_bits(b.p[off:off + p.numel()], val.reshape(-1))
        for flat in (b.m, b.v, b.e):
            s = b.slot(flat, p)
            assert s.data_ptr() == flat.data_ptr() + 4 * off and s.shape == p.shape
    mask = pad_mask(b)
    assert int(mask.sum()) == b.n - sum(p.numel() for p in params)
    assert not b.p[mask].any() and not b.e[mask].any()
    assert same_bits(b.e, b.p) and b.e.data_ptr() != b.p.data_ptr()
    # the gradient views map an extent of the owner's allocation the same way
    flat_g = torch.zeros(7 + b.n + 2)
    grads = b.grad_views(flat_g[7:7 + b.n])
    assert list(grads) == [id(p) for p in params]
    for p, off in zip(params, b.offsets):
        assert grads[id(p)].data_ptr() == flat_g.data_ptr() + 4 * (7 + off) and grads[id(p)].shape == p.shape


def test_adam_state_interchanges_with_torch_adam():
    b, params, values, g = make()
    b.m.copy_(torch.randn(b.n, generator=g))
    b.v.copy_(torch.rand(b.n, generator=g))
    order = [params[i] for i in (3, 0, 4, 1, 2)]                  # the optimizer's order need not be the bucket's
    sd = b.adam_state(order, 7, 3e-4, (0.8, 0.95), 1e-6)
    opt = torch.optim.Adam(order, lr=1.0)
    opt.load_state_dict(sd)
    grp = opt.param_groups[0]
    assert (grp["lr"], tuple(grp["betas"]), grp["eps"]) == (3e-4, (0.8, 0.95), 1e-6)
    for p in order:
        st = opt.state[p]
        assert float(st["step"]) == 7.0
        assert same_bits(st["exp_avg"], b.slot(b.m, p)) and same_bits(st["exp_avg_sq"], b.slot(b.v, p))
        assert st["exp_avg"].data_ptr() != b.slot(b.m, p).data_ptr()          # copies
    # ... and back: the optimizer's own state_dict() loads with equal bits, into moments that held something else
    m0, v0 = b.m.clone(), b.v.clone()
    b.m.fill_(3.0)
    b.v.fill_(4.0)
    steps, group = b.load_adam_state(opt.state_dict(), order, "optimizer state", "unused")
    assert steps == {7} and group["lr"] == 3e-4 and tuple(group["betas"]) == (0.8, 0.95)
    mask = pad_mask(b)
    assert same_bits(b.m[~mask], m0[~mask]) and same_bits(b.v[~mask], v0[~mask])
    assert not b.m[mask].any() and not b.v[mask].any()            # loading zeroes the pads
    # step 0: nothing has been accumulated, torch reports an empty state
    sd0 = b.adam_state(order, 0, 3e-4, (0.9, 0.999), 1e-8)
    assert sd0["state"] == {} and sd0["param_groups"][0]["params"] == [0, 1, 2, 3, 4]
    torch.optim.Adam(order, lr=1.0).load_state_dict(sd0)
    assert b.load_adam_state(sd0, order, "optimizer state", "unused")[0] == set()
    assert not b.m.any() and not b.v.any()


def test_load_refuses_what_does_not_fit_and_zeroes_absent_parameters():
    b, params, values, g = make()
    b.m.fill_(1.0)
    b.v.fill_(2.0)
    sd = b.adam_state(params, 3, 1e-3, (0.9, 0.999), 1e-8)
    short = {"state": sd["state"], "param_groups": [dict(sd["param_groups"][0], params=[0, 1, 2, 3])]}
    with pytest.raises(RuntimeError, match="optimizer state holds 4 parameters, the decoder has 5 trainable ones"):
        b.load_adam_state(short, params, "optimizer state", "the decoder has 5 trainable ones")
    with pytest.raises(RuntimeError, match="encoder optimizer state holds 4 parameters, the step trains conv1.weight"):
        b.load_adam_state(short, params, "encoder optimizer state", "the step trains conv1.weight and conv1.bias")
    bad = {"state": dict(sd["state"]), "param_groups": sd["param_groups"]}
    bad["state"][4] = dict(sd["state"][4], exp_avg=torch.zeros(5, 3))
    with pytest.raises(RuntimeError, match=r"encoder optimizer state 4 has shape \(5, 3\), parameter has \(3, 5\)"):
        b.load_adam_state(bad, params, "encoder optimizer state", "unused")
    assert bool((b.m == 1.0).all()) and bool((b.v == 2.0).all())   # a refused state wrote nothing
    part = {"state": {k: v for k, v in sd["state"].items() if k != 1}, "param_groups": sd["param_groups"]}
    steps, _ = b.load_adam_state(part, params, "optimizer state", "unused")
    assert steps == {3}
    assert not b.slot(b.m, params[1]).any() and not b.slot(b.v, params[1]).any()
    assert bool((b.slot(b.m, params[0]) == 1.0).all()) and bool((b.slot(b.v, params[4]) == 2.0).all())


def test_tensor_list_and_exchange():
    b, params, values, g = make()
    assert b.e is None and [t.data_ptr() for t in b.tensors()] == [t.data_ptr() for t in (b.p, b.m, b.v)]
    b.start_average()
    assert [t.data_ptr() for t in b.tensors()] == [t.data_ptr() for t in (b.p, b.m, b.v, b.e)]
    b.e.copy_(torch.randn(b.n, generator=g))
    p0, e0 = b.p.clone(), b.e.clone()
    ptrs = (b.p.data_ptr(), b.e.data_ptr())
    b.exchange_average()
    assert same_bits(b.p, e0) and same_bits(b.e, p0)
    assert same_bits(params[3].detach(), b.slot(e0, params[3]))    # the parameters see the average through their views
    b.exchange_average()
    assert same_bits(b.p, p0) and same_bits(b.e, e0) and (b.p.data_ptr(), b.e.data_ptr()) == ptrs


@pytest.mark.parametrize("which", [0, -1])
def test_residency_check(which):
    b, params, values, g = make()
    assert b.resident()
    params[which].data = params[which].data.clone()
    assert not b.resident()
