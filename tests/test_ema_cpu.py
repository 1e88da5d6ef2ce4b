"""The moving average of the parameters, the parts that need no GPU:
  * tests/ema_ref.py against a torch loop of e.lerp_(p, 1 - d) on the CPU;
  * d_t against hand values;
  * the header declares the two entries, the binding holds them, and they refuse bad arguments without a launch;
  * the wrapper's argument errors come before the library is reached;
  * ema_decay outside [0, 1) is refused by TrainStep's check and by train.Config."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import ick_amd.lib as L
import ick_amd.ops as ops
from ema_ref import decay_at32, decay_at64, ema_update32, ema_update64
from ick_amd.lib import IckError
from ick_amd.training import check_ema_decay, ema_decay_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("decay", [0.9, 0.99, 0.999])
def test_restatement_is_torchs_lerp(decay, warmup):
    """Twenty steps over 4099 elements.  torch's lerp_ computes start + weight * (end - start) for a weight below 0.5 --
    the restatement's expression -- and end - (end - start) * (1 - weight) from 0.5 on; the float32 comparison therefore
    takes the steps whose weight 1 - d_t is below 0.5, from the same state (with warmup that is every step from t = 9 on;
    the earlier ones are compared in float64 only).
    Float32: equal, or within 1 ulp where torch fuses.  torch's vectorised lerp contracts weight * diff + start into one
    fused multiply-add, the restatement (like the kernel) rounds the product first; the two can differ by the product's
    rounding, half an ulp of the product, plus the sum's own.  Where the sum cancels (e and w * diff of opposite sign)
    the result is smaller than its operands, so the ulp that bounds the difference is the ulp at the larger operand's
    magnitude, not at the result's.  Observed on the CPU: most elements equal, the rest within that 1 ulp (up to a few
    hundred ulps OF THE RESULT at cancelling elements).  Float64 within 1e-12."""
    g = torch.Generator().manual_seed(7)
    e32 = torch.randn(4099, generator=g)
    e64 = e32.double()
    mine32, mine64 = e32.numpy().copy(), e64.numpy().copy()
    worst, differing = 0.0, 0
    for t in range(1, 21):
        p = torch.randn(4099, generator=g) * 0.1 + e32 * 0.9
        d32, d64 = decay_at32(t, decay, warmup), decay_at64(t, decay, warmup)
        w32 = np.float32(1.0) - d32
        if w32 < 0.5:
            state = torch.from_numpy(mine32.copy())
            state.lerp_(p, float(w32))
            new = ema_update32(mine32, p.numpy(), t, decay, warmup)
            prod = (w32 * (p.numpy() - mine32)).astype(np.float32)
            ulp = np.spacing(np.maximum(np.maximum(np.abs(mine32), np.abs(prod)), np.abs(new)))
            off = np.abs(new.astype(np.float64) - state.numpy().astype(np.float64)) / ulp
            worst, differing = max(worst, float(off.max())), differing + int((off > 0).sum())
            assert off.max() <= 1.0, (t, off.max())
        mine32 = ema_update32(mine32, p.numpy(), t, decay, warmup)
        e64.lerp_(p.double(), 1.0 - d64)
        mine64 = ema_update64(mine64, p.double().numpy(), t, decay, warmup)
        assert np.abs(mine64 - e64.numpy()).max() <= 1e-12, t
        assert np.abs(mine32.astype(np.float64) - mine64).max() <= 1e-5          # the two forms follow each other
    print("float32 restatement against torch.lerp_: at most %.2f ulp, %d elements differ" % (worst, differing))


def test_decay_hand_values():
    hand = {1: 2.0 / 11.0, 2: 0.25, 100: 101.0 / 110.0, 10 ** 5: 0.999}         # (100001 / 100010 = 0.99991 > 0.999)
    for t, want in hand.items():
        assert abs(decay_at64(t, 0.999, True) - want) <= 1e-15, t
        assert abs(ema_decay_at(t, 0.999, True) - want) <= 1e-15, t
        assert abs(float(decay_at32(t, 0.999, True)) - want) <= 2.0 ** -23, t    # a float32 in (0.125, 1): ulp <= 2^-24
        assert decay_at64(t, 0.999) == ema_decay_at(t, 0.999) == 0.999           # without warmup: the decay itself
        assert decay_at32(t, 0.999) == np.float32(0.999)
    assert decay_at64(10 ** 5, 0.99995, True) == 100001.0 / 100010.0             # ... and the ramp where it is the smaller
    assert decay_at64(1, 0.1, True) == 0.1


# the eight entries, one pair per optimizer feature, that ick_adam_step[_derive] replaced
REMOVED = ["ick_adam_" + kind + form for kind in ("clamp", "opt", "ema", "decay") for form in ("", "_derive")]


def test_header_and_binding_hold_both_entries():
    import ick_amd.build as build
    src = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    declared = set(re.findall(r"^int\s+(ick_[a-z0-9_]+)\s*\(", src, flags=re.M))
    for name, nargs in (("ick_adam_step", 26), ("ick_adam_step_derive", 28)):
        assert name in declared and name in L.SIGNATURES
        assert len(L.SIGNATURES[name]) == nargs and L.SIGNATURES[name][-1] is L.vp
        decl = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, src, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == nargs
    # the two are the optimizer's only entries: the others are gone from the binding, the header and the library
    exported = ctypes.CDLL(build.build())
    for name in REMOVED:
        assert name not in L.SIGNATURES and not re.search(r"\b%s\b" % name, src) and not hasattr(exported, name), name
    assert hasattr(exported, "ick_adam_step") and hasattr(exported, "ick_adam_step_derive")


def test_entries_refuse_bad_arguments_without_a_launch():
    """No GPU here: ICK_EINVAL (-1) / ICK_EALIGN (-2) mean the entry returned before it touched the runtime."""
    import ick_amd.build as build
    build.build()
    lib = L.load()
    buf = (ctypes.c_float * 64)()
    p = ctypes.addressof(buf)
    p = p + (-p) % 16
    sch = L.LrSchedule()
    #       p  g  m  v  e  n  gscale clip lr   words sched b1  b2     eps   step sp    den   ema_d w
    flat = [p, p, p, p, p, 8, 1.0, 5.0, 4e-4, None, sch, 0.9, 0.999, 1e-8, 1, None, None, p, 0,
            None, None, 0, 0, 0, None, None]                       # decay, mask, granules, form, bump_inc, ticket, stream
    for i, want in ((4, -1), (17, -1), (0, -1), (5, -1)):          # no average, no decay word, no parameters, no floats
        a = list(flat)
        a[i] = 0 if i == 5 else None
        assert lib.ick_adam_step(*a) == want, i
    a = list(flat)
    a[4], a[17], a[18] = None, None, 1                              # a warmup without an average
    assert lib.ick_adam_step(*a) == -1
    a = list(flat)
    a[4] = p + 2                                                    # not on a float
    assert lib.ick_adam_step(*a) == -2
    a = list(flat)
    a[9], a[10] = p, L.LrSchedule(7, 0, 0, 0.0)                     # with the words: an unknown schedule kind
    assert lib.ick_adam_step(*a) == -1
    a = list(flat)
    a[23], a[24] = 1, p                                             # a ticket without the counter it advances
    assert lib.ick_adam_step(*a) == -1
    cover = [p, p, p, p, p, p, p, 1, 1.0, 5.0, 4e-4, None, sch, 0.9, 0.999, 1e-8, 1, None, None, p, 0,
             None, None, 0, 0, 0, None, None]
    for i in (4, 19, 6):                                            # no average, no decay word, no blocks
        a = list(cover)
        a[i] = None
        assert lib.ick_adam_step_derive(*a) == -1, i
    a = list(cover)
    a[4], a[19], a[20] = None, None, 1
    assert lib.ick_adam_step_derive(*a) == -1
    a = list(cover)
    a[4] = p + 4                                                    # the cover's float4 accesses need 16 bytes
    assert lib.ick_adam_step_derive(*a) == -2
    a = list(cover)
    a[25], a[26] = 1, p
    assert lib.ick_adam_step_derive(*a) == -1


def test_wrapper_errors_come_before_the_library(monkeypatch):
    def no_launch():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(L, "load", no_launch)
    four = lambda: [torch.zeros(8) for _ in range(4)]              # noqa: E731
    bad = [
        dict(lr=4e-4, ema=torch.zeros(8), ema_decay_word=torch.zeros(1)),                    # host tensors
        dict(lr=4e-4, ema=None, ema_decay_word=torch.zeros(1)),                              # a decay without an average
        dict(lr=4e-4, ema=None, ema_warmup=True),
        dict(lr=4e-4, ema=0.5, ema_decay_word=torch.zeros(1)),
        dict(lr=4e-4, ema=torch.zeros(8), ema_decay_word=0.999),                             # a host scalar decay
        dict(lr=4e-4, ema=torch.zeros(8), ema_decay_word=None),
        dict(lr=4e-4, ema=torch.zeros(8, dtype=torch.float64), ema_decay_word=torch.zeros(1)),
        dict(lr=4e-4, ema=torch.zeros(4), ema_decay_word=torch.zeros(1)),                    # shorter than the bucket
        dict(ema=torch.zeros(8), ema_decay_word=torch.zeros(1)),                             # neither lr nor words
    ]
    for kw in bad:
        with pytest.raises(IckError):
            ops.adam_update(*four(), 1, **kw)


def test_bad_decays_are_refused():
    from ick_amd import train as tr
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(IckError):
            check_ema_decay(bad)
        with pytest.raises(ValueError, match="ema_decay"):
            tr.Config(ema_decay=bad)
    assert check_ema_decay(None) is None and check_ema_decay(0) == 0.0 and check_ema_decay(0.999) == 0.999
    cfg = tr.Config()
    assert cfg.ema_decay is None and cfg.ema_warmup is False and cfg.ema_validate is True
    assert tr.Config(ema_decay=0.99, ema_warmup=True).ema_decay == 0.99
