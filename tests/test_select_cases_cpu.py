"""Without a GPU: the selection case tables (tests/select_cases.py) are checked before the device sees them.  For every
case the float64 reference (tests/select_ref.py) runs clean -- every decision is an intended tie or 1e-2 apart, or it
raises -- and the case's `expect` tags, the reasons it exists, are true of the reference's own result.  Together the
tags cover the situations the selection kernels can get wrong, and the table reaches every kernel instantiation.  The
beam reference is also held against the step references that take log-probability rows (diverse_step of
tests/diverse_beam_ref.py, constrained_step of tests/constrained_beam_ref.py)."""
import numpy as np
import pytest
import torch

import select_cases as SC
import select_ref as ref
from beam_rules_ref import lp_table
from constrained_beam_ref import constrained_step
from diverse_beam_ref import diverse_step


@pytest.mark.parametrize("case", SC.BEAM, ids=lambda c: c.name)
def test_beam_case_is_decidable_and_does_what_it_is_for(case):
    trace = SC.beam_trace(case.name)                        # raises Undecidable on a gap between 0 and 1e-2
    assert case.expect, case.name
    for tag in case.expect:
        assert SC.BEAM_TAGS[tag](case, trace), (case.name, tag)
    for t in trace:
        for x in t["rows"].values():
            assert np.isfinite(x).all() and np.abs(x).max() <= 16


@pytest.mark.parametrize("case", SC.SAMPLE, ids=lambda c: c.name)
def test_sample_case_is_decidable_and_does_what_it_is_for(case):
    trace = SC.sample_trace(case.name)
    assert case.expect, case.name
    for tag in case.expect:
        assert SC.SAMPLE_TAGS[tag](case, trace), (case.name, tag)


def test_tables_cover_every_situation_and_every_kernel_instantiation():
    assert len({c.name for c in SC.BEAM}) == len(SC.BEAM) and len({c.name for c in SC.SAMPLE}) == len(SC.SAMPLE)
    assert SC.BEAM_TAGS_REQUIRED - {t for c in SC.BEAM for t in c.expect} == set()
    assert SC.SAMPLE_TAGS_REQUIRED - {t for c in SC.SAMPLE for t in c.expect} == set()
    assert set().union(*(c.kernels() for c in SC.BEAM)) == SC.BEAM_KERNELS
    assert set().union(*(c.kernels() for c in SC.SAMPLE)) == SC.SAMPLE_KERNELS
    # the shapes of the envelope
    assert {c.beam for c in SC.BEAM} >= {1, 2, 5, 8} and {c.B for c in SC.BEAM} >= {1, 3}
    assert {c.Vx for c in SC.BEAM} >= {3, 1023, 1024, 1025, 65536, 66560}
    assert {(c.Vx, c.beam) for c in SC.BEAM} >= {(65536, 8), (66560, 2)}
    assert {c.F > 0 for c in SC.BEAM} == {False, True}
    assert {c.Vx for c in SC.SAMPLE} >= {5, 4097, 16384, 16385, 65536} and {c.rps for c in SC.SAMPLE} >= {1, 3}
    for form in ("plain", "diverse", "forced"):
        assert any(c.form == form and "scripted" in c.expect for c in SC.BEAM), form
    assert any(c.form == "plain" and c.rules and "scripted" in c.expect for c in SC.BEAM)
    for c in SC.BEAM + SC.SAMPLE:
        assert c.R <= 16 or c.Vx < 65536, c.name


def test_an_undecidable_step_raises():
    """The margins are the reference's: a gap between 0 and 1e-2 is refused, for a beam candidate, a top-k threshold and a
    top-p boundary."""
    case = SC.BEAM_BY_NAME["beam1"]
    st, t = SC.beam_state(case), SC.tables(case)
    rows = {r: SC.row(54, {7: 3.0, 8: 2.0}) for r in range(3)}
    ref.beam_step(case, st, rows, 0, t)
    case2 = SC.BeamCase(**{**case.__dict__, "beam": 2, "B": 1})
    st2 = SC.beam_state(case2)
    with pytest.raises(ref.Undecidable):
        ref.beam_step(case2, st2, {0: SC.row(54, {7: 3.0, 8: 2.0, 9: 1.995})}, 0, SC.tables(case2))
    sc = SC.SAMPLE_BY_NAME["topk_vx_minus_1"]
    ss, stb = SC.sample_state(sc), SC.tables(sc)
    with pytest.raises(ref.Undecidable):
        ref.sample_step(sc, ss, {0: np.float32([0, 1, 2, 3, -4]), 1: np.float32([-4, 1, 2, 3, -3.995])}, 0, stb)
    sp = SC.SampleCase(**{**sc.__dict__, "top_k": 0, "top_p": 0.64})        # e^3 / sum = 0.6403
    with pytest.raises(ref.Undecidable):
        ref.sample_step(sp, ss, {0: np.float32([0, 1, 2, 3, -4]), 1: np.float32([-4, 1, 2, 3, 0])}, 0, stb)


def _slots_equal(case, new, out, b, pos):
    for j, h in enumerate(new):
        r = b * case.beam + j
        if h is None:
            assert out["cum"][r] == ref.NEG and out["fin"][r] == 1, (case.name, pos, r)
            continue
        assert out["cum"][r] != ref.NEG, (case.name, pos, r)
        assert [int(t) for t in out["seq"][r, :len(h["seq"])]] == h["seq"], (case.name, pos, r)
        assert bool(out["fin"][r]) == h["fin"] and abs(out["cum"][r] - h["score"]) < 1e-4, (case.name, pos, r)
        if case.form == "forced":
            assert int(out["met"][r]) == h["met"], (case.name, pos, r)


@pytest.mark.parametrize("case", [c for c in SC.BEAM if c.Vx <= 4096], ids=lambda c: c.name)
def test_beam_reference_agrees_with_the_log_probability_step_references(case):
    """diverse_step (one group and no penalty: plain beam search) and constrained_step take fp32 log-probability rows
    and keep fp32 keys; the decisions are 1e-2 apart, so both references must choose alike."""
    ngram, min_len, alpha = case.rules if case.rules else (0, 0, 0.0)
    lp = lp_table(alpha, case.max_len)
    for t in SC.beam_trace(case.name):
        pos, st = t["pos"], t["st"]
        for b in range(case.B):
            if b in t["info"]["carried"]:
                continue
            hyps = ref.to_hyps(case, st, b, pos)
            rows, bans = {}, {}
            for j in range(case.beam):
                r = b * case.beam + j
                if r in t["rows"]:
                    x = torch.from_numpy(t["rows"][r]).double()
                    rows[j] = x.log_softmax(0).float()
                    bans[j] = ref.banned_set(hyps[j]["seq"], pos, ngram, min_len, case.end)
            if case.form == "forced":
                new = constrained_step(hyps, rows, pos, list(case.force[b]), lp, case.end, bans)
            else:
                groups, lam = (case.groups, case.lam) if case.form == "diverse" else (1, 0.0)
                new = diverse_step(hyps, rows, pos, groups, lam, lp, case.end, bans)
            _slots_equal(case, new, t["out"], b, pos)
