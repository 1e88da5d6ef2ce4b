"""Weight decay inside the fused Adam pass, the parts that need no GPU:
  * tests/weight_decay_ref.py's float64 step against torch.optim.AdamW and torch.optim.Adam(weight_decay=) in float64;
  * ParamBucket.decay_mask: the granules of the selected parameters, byte for byte;
  * check_weight_decay and train.Config;
  * ParamBucket.adam_state with per-parameter groups, the unchanged dict without decay, load_adam_state on both layouts;
  * the header declares the two entries, the binding holds them, they refuse bad arguments without a launch, and the
    wrapper's argument errors come before the library is reached."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ick_amd.lib as L
import ick_amd.ops as ops
from ick_amd.bucket import ALIGN, ParamBucket
from ick_amd.lib import IckError
from ick_amd.training import check_weight_decay, default_decay_filter
from weight_decay_ref import adam_l2_step64, adamw_step64, clamped_grad32, coupled_grad32, decoupled_factor32, shrink32

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1,), (63,), (64,), (65,), (300, 7)]


def make_params(dtype=torch.float32, seed=3):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g, dtype=torch.float64).to(dtype)) for s in SHAPES]


@pytest.mark.parametrize("decoupled", [True, False], ids=["adamw", "adam_l2"])
def test_float64_restatement_is_torchs_optimizer(decoupled):
    """Five steps on five small tensors, decay on three of them (a mixed selection), double on both sides: the same
    arithmetic, so 1e-12 of each tensor's largest magnitude."""
    lr, wd = 3e-3, 0.3
    params = make_params(torch.float64)
    selected = [False, True, False, True, True]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[p], weight_decay=wd if s else 0.0) for p, s in zip(params, selected)], lr=lr, weight_decay=0.0)
    mine = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in params]
    step = adamw_step64 if decoupled else adam_l2_step64
    g = torch.Generator().manual_seed(11)
    for t in range(1, 6):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
        for p, gr in zip(params, grads):
            p.grad = gr.clone()
        opt.step()
        mine = [step(p, gr.numpy(), m, v, t, lr, wd, decay=s) for (p, m, v), gr, s in zip(mine, grads, selected)]
        for (p, m, v), tp in zip(mine, params):
            st = opt.state[tp]
            for a, b in ((p, tp.detach()), (m, st["exp_avg"]), (v, st["exp_avg_sq"])):
                b = b.numpy()
                assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (t, decoupled)
    # the decay did something: an undecayed run of the same gradients ends elsewhere on the selected tensors only
    plain = [(p.detach().numpy().copy(), np.zeros(p.shape), np.zeros(p.shape)) for p in make_params(torch.float64)]
    g = torch.Generator().manual_seed(11)
    for t in range(1, 6):
        grads = [torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]
        plain = [step(p, gr.numpy(), m, v, t, lr, 0.0, decay=True) for (p, m, v), gr in zip(plain, grads)]
    for (p, _, _), (q, _, _), s in zip(mine, plain, selected):
        assert (np.abs(p - q).max() > 1e-6) == s


def test_float32_pieces_round_after_every_operation():
    f = decoupled_factor32(4e-4, 2.5)
    assert f.dtype == np.float32 and f == np.float32(1.0) - np.float32(np.float32(4e-4) * np.float32(2.5))
    assert decoupled_factor32(4e-4, 0.0) == np.float32(1.0)
    p = np.array([0.3, -1.7, 0.0], dtype=np.float32)
    assert np.array_equal(shrink32(p, 1.0), p) and shrink32(p, f).dtype == np.float32
    x = clamped_grad32(np.array([70.0, -70.0, 0.7], dtype=np.float32), 7.0, 5.0, coef=0.25)
    assert np.array_equal(x, np.array([2.5, -2.5, np.float32(np.float32(0.7) * np.float32(1 / np.float32(7.0))) *
                                       np.float32(0.25)], dtype=np.float32))
    assert np.array_equal(clamped_grad32(np.array([70.0], dtype=np.float32), 7.0, 5.0), np.array([5.0], dtype=np.float32))
    assert np.array_equal(coupled_grad32(x, p, 0.0), x)
    want = (x + (np.float32(0.1) * p).astype(np.float32)).astype(np.float32)
    assert np.array_equal(coupled_grad32(x, p, 0.1), want)


def test_decay_mask_marks_the_selected_parameters_granules():
    params = make_params()
    names = ["one", "b63", "b64", "b65", "matrix"]
    b = ParamBucket(params, IckError)
    assert b.offsets == [0, 64, 128, 192, 320, 320 + 2112] and b.n % ALIGN == 0
    granules = [1, 1, 1, 2, 33]
    # the default filter: ndim >= 2 only
    chosen = [p for n, p in zip(names, params) if default_decay_filter(n, p)]
    assert [p is params[4] for p in chosen] == [True]
    mask = b.decay_mask(chosen)
    assert mask.dtype == torch.uint8 and mask.device == b.p.device and mask.numel() == b.n // ALIGN == sum(granules)
    assert mask.tolist() == [0, 0, 0, 0, 0] + [1] * 33
    # a custom filter: by name
    chosen = [p for n, p in zip(names, params) if n in ("one", "b65")]
    assert b.decay_mask(chosen).tolist() == [1, 0, 0, 1, 1] + [0] * 33
    assert b.decay_mask(id(p) for p in chosen).tolist() == [1, 0, 0, 1, 1] + [0] * 33          # ids serve as well
    assert b.decay_mask([]).tolist() == [0] * 38 and b.decay_mask(params).tolist() == [1] * 38
    # every granule belongs to exactly one parameter: the masks of the single parameters partition the table
    singles = torch.stack([b.decay_mask([p]) for p in params])
    assert singles.sum(dim=0).tolist() == [1] * 38 and singles.sum(dim=1).tolist() == granules
    with pytest.raises(IckError):
        b.decay_mask([torch.nn.Parameter(torch.zeros(3))])


def test_check_weight_decay_and_config():
    from ick_amd import train as tr
    for bad in (-0.1, -1e-9, float("nan"), float("inf"), float("-inf")):
        with pytest.raises(IckError):
            check_weight_decay(bad)
        with pytest.raises(ValueError, match="weight_decay"):
            tr.Config(weight_decay=bad)
        with pytest.raises(ValueError, match="weight_decay"):
            tr.Config(train_conv1=True, encoder_weight_decay=bad)
    assert check_weight_decay(None) is None and check_weight_decay(0) == 0.0 and check_weight_decay(0.01) == 0.01
    assert check_weight_decay(12.5) == 12.5
    cfg = tr.Config()
    assert cfg.weight_decay is None and cfg.decoupled_weight_decay is True and cfg.encoder_weight_decay is None
    assert tr.Config(weight_decay=0.1, decoupled_weight_decay=False).weight_decay == 0.1
    with pytest.raises(ValueError, match="train_conv1"):
        tr.Config(encoder_weight_decay=0.1)


TODAY = {"lr": 4e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
         "foreach": None, "capturable": False, "differentiable": False, "fused": None, "decoupled_weight_decay": False}


def filled_bucket():
    params = make_params()
    b = ParamBucket(params, IckError)
    g = torch.Generator().manual_seed(5)
    b.m.copy_(torch.randn(b.n, generator=g))
    b.v.copy_(torch.rand(b.n, generator=g))
    return b, params


def test_adam_state_without_decay_is_the_unchanged_dict():
    b, params = filled_bucket()
    sd = b.adam_state(params, 3, 4e-4, [0.9, 0.999], 1e-8)
    assert list(sd) == ["state", "param_groups"] and len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert list(group) == list(TODAY) + ["params"]
    for k, v in TODAY.items():
        assert group[k] == v and type(group[k]) is type(v), k
    assert group["params"] == [0, 1, 2, 3, 4]
    assert sorted(sd["state"]) == [0, 1, 2, 3, 4]
    for i, p in enumerate(params):
        assert list(sd["state"][i]) == ["step", "exp_avg", "exp_avg_sq"] and float(sd["state"][i]["step"]) == 3.0
        assert torch.equal(sd["state"][i]["exp_avg"], b.slot(b.m, p))
        assert torch.equal(sd["state"][i]["exp_avg_sq"], b.slot(b.v, p))
    assert b.adam_state(params, 0, 4e-4, [0.9, 0.999], 1e-8)["state"] == {}
    # ... and torch's own Adam loads it
    torch.optim.Adam(params, lr=1.0).load_state_dict(sd)


@pytest.mark.parametrize("decoupled", [True, False])
def test_adam_state_reports_one_group_per_parameter_with_decay(decoupled):
    b, params = filled_bucket()
    decay = [0.0, 0.0, 0.3, 0.0, 0.3]
    sd = b.adam_state(params, 2, 4e-4, [0.9, 0.999], 1e-8, decay=decay, decoupled=decoupled)
    assert [g["params"] for g in sd["param_groups"]] == [[0], [1], [2], [3], [4]]
    assert [g["weight_decay"] for g in sd["param_groups"]] == decay
    assert all(g["decoupled_weight_decay"] is decoupled for g in sd["param_groups"])
    for g in sd["param_groups"]:
        assert {k: g[k] for k in TODAY if k not in ("weight_decay", "decoupled_weight_decay")} == \
            {k: TODAY[k] for k in TODAY if k not in ("weight_decay", "decoupled_weight_decay")}
    # torch's own optimizer of that kind, built over the same groups, reports the same groups and loads the state
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[p], weight_decay=w) for p, w in zip(params, decay)], lr=4e-4, weight_decay=0.0)
    assert opt.state_dict()["param_groups"] == sd["param_groups"]
    opt.load_state_dict(sd)
    assert torch.equal(opt.state[params[4]]["exp_avg"], b.slot(b.m, params[4]))
    with pytest.raises(IckError):
        b.adam_state(params, 2, 4e-4, [0.9, 0.999], 1e-8, decay=decay[:-1])


def test_load_adam_state_round_trips_both_layouts():
    b, params = filled_bucket()
    one = b.adam_state(params, 4, 4e-4, [0.9, 0.999], 1e-8)
    many = b.adam_state(params, 4, 4e-4, [0.9, 0.999], 1e-8, decay=[0.1] * 5, decoupled=True)
    m0, v0 = b.m.clone(), b.v.clone()
    for sd in (one, many):
        fresh = ParamBucket(make_params(), IckError)
        steps, group = fresh.load_adam_state(sd, fresh.params, "optimizer state", "five expected")
        assert steps == {4} and group["lr"] == 4e-4
        for p, q in zip(fresh.params, params):
            assert torch.equal(fresh.slot(fresh.m, p), b.slot(m0, q)) and torch.equal(fresh.slot(fresh.v, p), b.slot(v0, q))
        back = fresh.adam_state(fresh.params, 4, 4e-4, [0.9, 0.999], 1e-8)
        assert all(torch.equal(back["state"][i]["exp_avg"], one["state"][i]["exp_avg"]) for i in range(5))
    with pytest.raises(IckError):
        b.load_adam_state(dict(many, param_groups=many["param_groups"][:-1]), params, "optimizer state", "five expected")


def test_header_and_binding_hold_both_entries():
    import ick_amd.build as build
    src = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    declared = set(re.findall(r"^int\s+(ick_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name, nargs in (("ick_adam_step", 26), ("ick_adam_step_derive", 28)):
        assert name in declared and name in L.SIGNATURES
        assert len(L.SIGNATURES[name]) == nargs and L.SIGNATURES[name][-1] is L.vp
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == nargs
    assert re.search(r"#define ICK_DECAY_DECOUPLED 0\b", src) and re.search(r"#define ICK_DECAY_COUPLED 1\b", src)
    assert (ops.DECAY_DECOUPLED, ops.DECAY_COUPLED) == (0, 1)
    # the entries these two replaced are gone: from the binding, from the header, from the built library
    exported = ctypes.CDLL(build.build())
    for name in ["ick_adam_" + kind + form for kind in ("clamp", "opt", "ema", "decay") for form in ("", "_derive")]:
        assert name not in L.SIGNATURES and not re.search(r"\b%s\b" % name, src) and not hasattr(exported, name), name


def test_entries_refuse_bad_arguments_without_a_launch():
    """No GPU here: ICK_EINVAL (-1) means the entry returned before it touched the runtime."""
    import ick_amd.build as build
    build.build()
    lib = L.load()
    buf = (ctypes.c_float * 256)()
    p = ctypes.addressof(buf)
    p = p + (-p) % 16
    sch = L.LrSchedule()
    #       p  g  m  v  e     n    gscale clip lr   words sched b1  b2     eps   step sp    den   ema_d w  wd mask gr form
    flat = [p, p, p, p, None, 130, 1.0, 5.0, 4e-4, None, sch, 0.9, 0.999, 1e-8, 1, None, None, None, 0, p, p, 3, 0,
            0, None, None]                                          # (... bump_inc, ticket, stream)
    for i, bad in ((19, None), (20, None), (21, 2), (21, 0), (22, 2), (22, -1), (0, None), (5, 0)):
        a = list(flat)          # mask without word, word without mask, granules below ceil(130 / 64), an unknown form,
        a[i] = bad              # no p, no floats
        assert lib.ick_adam_step(*a) == -1, (i, bad)
    a = list(flat)
    a[4] = p                                                        # with an average: its decay word must be there
    assert lib.ick_adam_step(*a) == -1
    a = list(flat)
    a[9], a[10] = p, L.LrSchedule(7, 0, 0, 0.0)                     # with the words: an unknown schedule kind
    assert lib.ick_adam_step(*a) == -1
    a = list(flat)
    a[23], a[24] = 1, p                                             # a ticket without the counter it advances
    assert lib.ick_adam_step(*a) == -1
    cover = [p, p, p, p, None, p, p, 1, 1.0, 5.0, 4e-4, None, sch, 0.9, 0.999, 1e-8, 1, None, None, None, 0, p, p, 3, 0,
             0, None, None]
    for i, bad in ((21, None), (22, None), (23, 0), (24, 2), (6, None)):
        a = list(cover)
        a[i] = bad
        assert lib.ick_adam_step_derive(*a) == -1, (i, bad)


def test_wrapper_errors_come_before_the_library(monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    four = lambda: [torch.zeros(130) for _ in range(4)]            # noqa: E731
    word, mask = torch.zeros(1), torch.zeros(3, dtype=torch.uint8)
    bad = [
        dict(decay_word=word, decay_mask=mask),                                              # host tensors
        dict(decay_word=word),                                                               # one without the other
        dict(decay_mask=mask),
        dict(decay_word=0.01, decay_mask=mask),                                              # a host scalar decay
        dict(decay_word=word.double(), decay_mask=mask),
        dict(decay_word=word, decay_mask=mask.float()),
        dict(decay_word=word, decay_mask=mask[:2]),                                          # fewer granules than the bucket
    ]
    for kw in bad:
        with pytest.raises(IckError):
            ops.adam_update(*four(), 1, lr=4e-4, **kw)
