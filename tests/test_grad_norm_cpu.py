"""Global-norm gradient clipping and the learning-rate schedule, the parts that need no GPU:
  * tests/grad_norm_ref.py (norm, coef, clamp, Adam in float64) against torch.nn.utils.clip_grad_norm_ + clamp_ +
    torch.optim.Adam over three steps, with the clip active and not;
  * training.lr_at against hand-computed values and against torch.optim.lr_scheduler.LambdaLR driving an optimizer;
  * bad arguments raise IckError;
  * the ctypes struct, the word count and the schedule kinds follow the header."""
import ctypes
import math
import os
import subprocess
import types

import numpy as np
import pytest
import torch

import ick_amd.lib as L
import ick_amd.ops as ops
from grad_norm_ref import clip_adam_step, clip_coef, global_norm
from ick_amd.lib import IckError
from ick_amd.training import check_lr_schedule, check_max_grad_norm, lr_at

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(7, 5), (33,), (1,), (4, 3, 2), (64,)]


@pytest.mark.parametrize("max_norm,clip", [(0.5, 5.0), (1e6, 5.0), (0.5, None), (None, 0.05), (3.0, 0.05)])
def test_restatement_is_torchs_clip_grad_norm_clamp_adam(max_norm, clip):
    g = torch.Generator().manual_seed(3)
    params = [torch.randn(s, generator=g, dtype=torch.float64).requires_grad_(True) for s in SHAPES]
    opt = torch.optim.Adam(params, lr=4e-4)
    p = [t.detach().numpy().copy() for t in params]
    m, v = [np.zeros_like(a) for a in p], [np.zeros_like(a) for a in p]
    active = []
    for t in range(1, 4):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * (0.3 * t) for s in SHAPES]
        for prm, gr in zip(params, grads):
            prm.grad = gr.clone()
        norm_t = float("nan")
        if max_norm is not None:
            norm_t = torch.nn.utils.clip_grad_norm_(params, max_norm, norm_type=2).item()
        if clip is not None:
            for prm in params:
                prm.grad.clamp_(-clip, clip)
        opt.step()
        p, gc, m, v, norm, coef = clip_adam_step(p, [x.numpy() for x in grads], m, v, t, 4e-4, max_norm, clip)
        active.append(coef < 1.0)
        if max_norm is not None:
            assert abs(norm - norm_t) <= 1e-12 * norm_t
        for mine, prm, gcl in zip(p, params, gc):
            assert np.abs(mine - prm.detach().numpy()).max() <= 1e-12
            assert np.abs(gcl - prm.grad.numpy()).max() <= 1e-12
        for i, prm in enumerate(params):
            assert np.abs(m[i] - opt.state[prm]["exp_avg"].numpy()).max() <= 1e-12
            assert np.abs(v[i] - opt.state[prm]["exp_avg_sq"].numpy()).max() <= 1e-12
    assert all(active) == (max_norm is not None and max_norm < 10) and any(active) == all(active)


def test_coef_definition():
    assert clip_coef(2.0, None) == 1.0 and clip_coef(2.0, 4.0) == 1.0
    assert clip_coef(2.0, 1.0) == 1.0 / (2.0 + 1e-6)
    assert math.isnan(clip_coef(float("nan"), 1.0)) and clip_coef(float("inf"), 1.0) == 0.0
    assert global_norm([np.array([3.0]), np.array([[4.0]])]) == 5.0


W, N, R_ = 4, 10, 0.1
HAND = {   # kind -> the factor at t = 1, W, W + 1, N, N + 5
    "constant": [0.25, 1.0, 1.0, 1.0, 1.0],
    "inverse_sqrt": [0.25, 1.0, math.sqrt(4 / 5), math.sqrt(4 / 10), math.sqrt(4 / 15)],
    "cosine": [0.25, 1.0, 0.1 + 0.9 * 0.5 * (1 + math.sqrt(3) / 2), 0.1, 0.1],          # cos(pi / 6) = sqrt(3) / 2
    "linear": [0.25, 1.0, 0.1 + 0.9 * 5 / 6, 0.1, 0.1],
}


@pytest.mark.parametrize("kind", sorted(HAND))
def test_lr_at_hand_values_and_lambda_lr(kind):
    sch = dict(kind=kind, warmup_steps=W, total_steps=N, min_lr_ratio=R_)
    base = 4e-4
    for t, f in zip((1, W, W + 1, N, N + 5), HAND[kind]):
        assert abs(lr_at(t, base, sch) - base * f) <= 1e-15 * base + 1e-12 * base * f, (kind, t)
    prm = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([prm], lr=base)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda k: lr_at(k + 1, 1.0, sch))
    for t in range(1, N + 7):
        assert abs(opt.param_groups[0]["lr"] - lr_at(t, base, sch)) <= 1e-15 * base, (kind, t)
        opt.step()
        sched.step()


def test_lr_at_without_warmup_and_without_schedule():
    assert lr_at(1, 3e-4, None) == 3e-4 and lr_at(1, 3e-4, dict(kind="constant")) == 3e-4
    assert lr_at(7, 3e-4, dict(kind="constant", warmup_steps=0)) == 3e-4
    sch = dict(kind="linear", warmup_steps=0, total_steps=4, min_lr_ratio=0.0)
    assert [lr_at(t, 1.0, sch) for t in (1, 2, 4, 9)] == [0.75, 0.5, 0.0, 0.0]


def test_bad_arguments_raise():
    for bad in (0, 0.0, -1.0, float("nan")):
        with pytest.raises(IckError):
            check_max_grad_norm(bad)
    assert check_max_grad_norm(None) is None and check_max_grad_norm(2) == 2.0
    for bad in (dict(kind="exponential"), dict(kind="cosine", warmup_steps=5, total_steps=5),
                dict(kind="linear", warmup_steps=6, total_steps=5), dict(kind="inverse_sqrt", warmup_steps=0),
                dict(kind="inverse_sqrt"), dict(kind="constant", warmup_steps=-1), dict(kind="cosine", total_steps=4,
                                                                                         min_lr_ratio=1.5),
                dict(kind="constant", warmup=3), "cosine"):
        with pytest.raises(IckError):
            check_lr_schedule(bad)
        with pytest.raises(IckError):
            lr_at(1, 1.0, bad)
    with pytest.raises(IckError):
        ops.lr_schedule_struct(dict(kind="exponential"))
    # the wrappers refuse host scalars where a device word is required (no GPU needed to be refused)
    cover = types.SimpleNamespace(items_dev=None, blocks_dev=None, n_blocks=1, nbytes=0)
    for bad in (4e-4, torch.zeros(L.OPT_WORDS), torch.zeros(L.OPT_WORDS, dtype=torch.float64)):
        with pytest.raises(IckError):
            ops.grad_sqnorm(torch.zeros(8), bad)
        with pytest.raises(IckError):
            ops.adam_update(*(torch.zeros(8) for _ in range(4)), 1, words=bad)
        with pytest.raises(IckError):
            ops.adam_update(*(torch.zeros(8) for _ in range(4)), 1, words=bad, cover=cover)
    # exactly one of lr and words; a schedule shapes the rate in the words only
    for kw, why in ((dict(lr=4e-4, words=torch.zeros(L.OPT_WORDS)), "exactly one"), (dict(), "exactly one"),
                    (dict(lr=4e-4, schedule=dict(kind="constant")), "schedule")):
        with pytest.raises(IckError, match=why):
            ops.adam_update(*(torch.zeros(8) for _ in range(4)), 1, **kw)


def test_struct_words_and_kinds_follow_the_header(tmp_path):
    src = ('#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu %d %d %d %d %d", sizeof(ick_lr_schedule), '
           'ICK_OPT_WORDS, ICK_LR_CONSTANT, ICK_LR_INVERSE_SQRT, ICK_LR_COSINE, ICK_LR_LINEAR);}\n')
    c, exe = str(tmp_path / "sz.c"), str(tmp_path / "sz")
    open(c, "w").write(src)
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
    size, words, k0, k1, k2, k3 = (int(x) for x in subprocess.check_output([exe]).split())
    assert ctypes.sizeof(L.LrSchedule) == size == 16 and L.OPT_WORDS == words
    assert L.LR_KINDS == {"constant": k0, "inverse_sqrt": k1, "cosine": k2, "linear": k3}
    s = ops.lr_schedule_struct(dict(kind="cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1))
    assert (s.kind, s.warmup, s.total) == (k2, 2, 6) and s.min_ratio == np.float32(0.1)
