"""Scheduled sampling without a GPU: the numpy restatement of ick_sched_sample_mix (tests/sched_sample_ref.py) on
hand-worked rows, the coin's rate, the probability staircase and the refusals, the ABI entry, and the two preconditions
the GPU tests lean on -- the float64 oracle's top-two margin at every eligible position of the step-level cases, and the
agreement of the float32 and float64 restatements on the kernel-alone cases' sampled draws."""
import math
import os
import re

import numpy as np
import pytest

import sched_sample_cases as SC
import sched_sample_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K, F = 8, 2, 2             # columns 0..7 words, 8..9 entities, 10..11 facts
START, PAD = 6, 0


def hand_case():
    """Two captions at L = 6: lengths 6 (n = 5, eligible q = 1..4, packed rows 0..4) and 3 (n = 2, eligible q = 1, rows
    5..6)."""
    lengths = [6, 3]
    caps = np.array([[START, 1, 2, 3, 4, 7], [START, 5, 7, PAD, PAD, PAD]], dtype=np.int64)
    masks = np.zeros_like(caps)
    rows = np.zeros((7, V + K + F), dtype=np.float32)
    rows[0, [3, 5]] = 2.0                   # a tie: the lower column, 3, wins           -> (0, 1) = (3, 0)
    rows[1, PAD] = 9.0; rows[1, 9] = 1.0    # <pad> holds the maximum and loses to 9     -> (0, 2) = (9, 1)
    rows[2, START] = 9.0; rows[2, 11] = 1.0  # <start> holds the maximum, loses to 11    -> (0, 3) = (11, 2)
    rows[3, 7] = 0.5                        # <end> may win                              -> (0, 4) = (7, 0)
    rows[4, 1] = 3.0                        # predicts position 5 = n: never fed back
    rows[5, 10] = 1.0                       #                                            -> (1, 1) = (10, 2)
    rows[6, 2] = 3.0                        # predicts position 2 = n of caption 1: not eligible
    return rows, lengths, caps, masks


def run(prob, argmax=True, seed=7, step=0, T=1.0):
    rows, lengths, caps, masks = hand_case()
    return SR.mix(rows, lengths, caps, masks, V, K, F, START, PAD, prob, T, seed, step, argmax) + (caps, masks)


def test_prob_zero_gives_gold():
    ci, mi, rep, margins, caps, masks = run(0.0)
    assert np.array_equal(ci, caps) and np.array_equal(mi, masks) and not rep.any() and not margins


def test_prob_one_argmax_on_hand_rows():
    ci, mi, rep, _, caps, masks = run(1.0)
    assert ci.tolist() == [[START, 3, 9, 11, 7, 7], [START, 10, 7, PAD, PAD, PAD]]
    assert mi.tolist() == [[0, 0, 1, 2, 0, 0], [0, 2, 0, 0, 0, 0]]
    assert rep.tolist() == [[0, 1, 1, 1, 1, 0], [0, 1, 0, 0, 0, 0]]
    # positions 0 and >= n_b stay gold whatever the rows say
    assert ci[0, 0] == caps[0, 0] and ci[0, 5] == caps[0, 5] and (ci[1, 2:] == caps[1, 2:]).all()


def test_mask_ranges_and_valid_rows():
    assert [SR.token_mask(c, V, K) for c in (0, 7, 8, 9, 10, 11)] == [0, 0, 1, 1, 2, 2]
    n, rowstart = SR.valid_rows([6, 3, 1, 0, 40], 6)
    assert n.tolist() == [5, 2, 0, 0, 5] and rowstart.tolist() == [0, 5, 7, 7, 7, 12]


def test_sampled_draw_is_the_perturbed_argmax_and_never_a_banned_column():
    rows, lengths, caps, masks = hand_case()
    for step in range(50):
        ci, mi, rep, _ = SR.mix(rows, lengths, caps, masks, V, K, F, START, PAD, 1.0, 0.8, 11, step, False)
        for (b, q) in [(0, 1), (0, 2), (0, 3), (0, 4), (1, 1)]:
            row = rows[SR.valid_rows(lengths, 6)[1][b] + q - 1]
            v = row / np.float32(0.8) + SR.noise(11, step, b, q, V + K + F)
            v[[START, PAD]] = -np.inf
            assert ci[b, q] == int(np.argmax(v)) and ci[b, q] not in (START, PAD)
            assert mi[b, q] == SR.token_mask(int(ci[b, q]), V, K) and rep[b, q] == 1


@pytest.mark.parametrize("prob", [0.05, 0.25, 0.5, 0.9])
def test_coin_fraction(prob):
    n = 100000
    bs, qs = np.arange(n) // 50, np.arange(n) % 50 + 1
    frac = SR.coins(0xC0FFEE, 5, bs, qs, prob).mean()
    sigma = math.sqrt(prob * (1 - prob) / n)
    assert abs(frac - prob) <= 4 * sigma, (frac, prob, sigma)
    # exact at the ends, and new words give new coins
    assert not SR.coins(1, 0, bs, qs, 0.0).any() and SR.coins(1, 0, bs, qs, 1.0).all()
    a = SR.coins(1, 0, bs, qs, 0.5)
    assert (a != SR.coins(1, 1, bs, qs, 0.5)).any() and (a != SR.coins(2, 0, bs, qs, 0.5)).any()


def test_staircase():
    from ick_amd.training import sampling_prob_at
    args = (2, 5, 0.05, 0.25)          # start, increase_every, increase_prob, max_prob
    got = [sampling_prob_at(e, *args) for e in (0, 1, 2, 6, 7, 12, 21, 22, 27, 500)]
    assert got == pytest.approx([0.0, 0.0, 0.05, 0.05, 0.10, 0.15, 0.20, 0.25, 0.25, 0.25], abs=1e-12)
    assert sampling_prob_at(3, -1, 5, 0.05, 0.25) == 0.0
    assert sampling_prob_at(0, 0, 1, 0.3, 0.25) == 0.25


def test_refusals():
    from ick_amd.lib import IckError
    from ick_amd.train import Config
    from ick_amd.training import (check_sampling_prob, check_sampling_temperature, check_scheduled_sampling,
                                  sampling_prob_at)
    assert check_scheduled_sampling(None) is None
    assert check_scheduled_sampling({}) == dict(prob=0.25, mode="sample", temperature=1.0, seed=None)
    for bad in (dict(prob=-0.1), dict(prob=1.5), dict(prob=float("nan")), dict(temperature=0.0), dict(temperature=-1.0),
                dict(temperature=float("inf")), dict(mode="greedy"), dict(probability=0.5), dict(seed=1.5), 0.25):
        with pytest.raises(IckError, match="scheduled_sampling"):
            check_scheduled_sampling(bad)
    with pytest.raises(IckError, match=r"prob must lie in \[0, 1\]"):
        check_sampling_prob(2)
    with pytest.raises(IckError, match="temperature must be"):
        check_sampling_temperature(0)
    with pytest.raises(IckError, match="increase_every"):
        sampling_prob_at(1, 0, 0, 0.05, 0.25)
    cfg = Config(scheduled_sampling_start=3)
    assert (cfg.scheduled_sampling_increase_every, cfg.scheduled_sampling_increase_prob, cfg.scheduled_sampling_max_prob,
            cfg.scheduled_sampling_mode) == (5, 0.05, 0.25, "sample") and Config().scheduled_sampling_start == -1
    for kw in (dict(scheduled_sampling_start=0, fused=False), dict(scheduled_sampling_start=0, scst=True),
               dict(scheduled_sampling_start=0, fine_tune_encoder=True), dict(scheduled_sampling_mode="greedy"),
               dict(scheduled_sampling_max_prob=1.5), dict(scheduled_sampling_increase_every=0)):
        with pytest.raises(ValueError):
            Config(**kw)


def test_symbol_declared_exported_bound():
    import ctypes
    import ick_amd.build as build
    import ick_amd.lib as L
    import ick_amd.ops as ops
    hdr = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    assert re.search(r"^int\s+ick_sched_sample_mix\s*\(", hdr, flags=re.M)
    assert hasattr(ctypes.CDLL(build.build()), "ick_sched_sample_mix")
    assert len(L.SIGNATURES["ick_sched_sample_mix"]) == 22
    assert callable(ops.sched_sample_mix)


def test_gumbel_lives_beside_philox():
    csrc = os.path.join(ROOT, "image-captioning-with-external-knowledge_amd", "csrc")
    owners = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h"))
              and re.search(r"float gumbel\(", open(os.path.join(csrc, f)).read())]
    assert owners == ["philox.h"]


@pytest.mark.parametrize("c", SC.CASES, ids=[c.name for c in SC.CASES])
def test_oracle_margin_precondition(c):
    """What lets tests/test_sched_sample_gpu.py hold the step's mixed inputs to the float64 oracle's WITHOUT excuses: at
    every eligible position the oracle's winner leads by at least 1e-3, fifty times the 2e-5 the device's scores differ
    from the oracle's by (tests/test_model_geometry_gpu.py's table)."""
    o = SC.oracle(c)
    n_el = sum(max(0, n - 2) for n in o["batch"]["caption_lengths"].view(-1).tolist())
    assert len(o["margins"]) == n_el == int(o["replaced"].sum()) and n_el > 0
    worst = min(o["margins"].values())
    print("%s: %d eligible positions, smallest top-two margin %.3e" % (c.name, n_el, worst))
    assert worst >= SC.MIN_MARGIN
    if c.variant != "geo":
        # the knowledge case must feed a pointer token back, or the GPU test could not see the indicators follow the mix
        assert int((o["masks_in"][o["replaced"] == 1] > 0).sum()) >= 1


@pytest.mark.parametrize("T", [0.7, 1.0])
@pytest.mark.parametrize("name", [s[0] for s in SC.KERNEL_SHAPES])
def test_float32_and_float64_restatements_agree_on_the_kernel_cases(name, T):
    """... so the GPU test of the sampled draws allows no excuse on these seeds."""
    k = SC.kernel_case(name)
    args = (k["rows"].numpy(), k["lengths"], k["captions"].numpy(), k["masks"].numpy(), k["V"], k["K"], k["F"], k["start"],
            k["pad"], 0.5, T, SC.KERNEL_SEED, SC.KERNEL_STEP, False)
    a, b = SR.mix(*args, dtype=np.float32), SR.mix(*args, dtype=np.float64)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b[:3]))
    if a[3]:
        print("%s T %.1f: %d draws, smallest perturbed margin %.3e" % (name, T, len(a[3]), min(a[3].values())))
