"""CPU checks of the column bias (predict_beam / predict_sample(column_bias=)): the argument forms
and errors, the padded device inputs, the references of tests/column_bias_ref.py pinned to steps worked by hand and to
the references without a bias, the case table of tests/column_bias_cases.py (every case decidable, every tag exhibited),
and the ABI of the two new entry points."""
import ctypes
import dataclasses
import inspect
import math
import os
import subprocess
import tempfile

import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.decoder as D
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
import column_bias_cases as CB
import column_bias_ref as ref
import sample_ref
import select_cases as SC
import select_ref
from beam_rules_ref import predict_beam_rules

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, K = 50, 5
WM = synth.make_word_map(V)
NINF = float("-inf")


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def cpu_decoder(variant="geo"):
    m = ick_amd.load_models(variant)
    return m.DecoderTransformer(word_map=WM, emb_dim=300, decoder_dim=512, encoder_dim=512, num_heads=10, num_layers=3)


# ------------------------------------------------------------------------------------------------ argument forms
def check(bias, B=2, Vx=V + K, **kw):
    return D.check_column_bias("x", B, Vx, WM, bias, **kw)


def test_none_is_the_default_and_returns_none():
    assert check(None) is None
    for fn in (D.DecoderTransformer.predict_beam, D.DecoderTransformer.predict_sample):
        assert inspect.signature(fn).parameters["column_bias"].default is None


def test_every_form_gives_the_same_padded_tensors():
    unk = WM["<unk>"]
    want_i = [[unk, V + 2] + [-1] * 62] * 2
    forms = [{"<unk>": NINF, V + 2: 1.5}, {unk: NINF, V + 2: 1.5}, ([unk, V + 2], [NINF, 1.5]),
             ([[unk, V + 2]] * 2, [[NINF, 1.5]] * 2), (torch.tensor([unk, V + 2], dtype=torch.int32), torch.tensor([NINF, 1.5])),
             (torch.tensor([[unk, V + 2]] * 2), torch.tensor([[NINF, 1.5]] * 2, dtype=torch.float64))]
    for f in forms:
        ids, vals = check(f)
        assert ids.dtype == torch.int32 and vals.dtype == torch.float32 and ids.shape == vals.shape == (2, 64)
        assert ids.tolist() == want_i
        assert vals[:, 0].tolist() == [NINF] * 2 and vals[:, 1].tolist() == [1.5] * 2 and (vals[:, 2:] == 0).all()


def test_empty_slots_ignore_their_value_and_c_64_is_accepted():
    ids, vals = check(([[3, -1, 5], [-1, -1, -1]], [[1.0, float("nan"), -2.0], [float("inf"), 3.0, NINF]]))
    assert ids[:, :3].tolist() == [[3, -1, 5], [-1, -1, -1]]
    assert vals[:, :3].tolist() == [[1.0, 0.0, -2.0], [0.0, 0.0, 0.0]]
    ids, vals = check((list(range(64)), [0.125] * 64), Vx=100)
    assert ids[1].tolist() == list(range(64)) and (vals == 0.125).all()
    same = D.bias_tensors(2, torch.arange(64), torch.full((64,), 0.125))
    assert torch.equal(same[0], ids) and torch.equal(same[1], vals)


BAD = [([3], [float("inf")]), ([3], [float("nan")]), ([-2], [0.0]), ([V + K], [0.0]), ([3, 3], [1.0, 2.0]),
       ([[3, 4], [5, 5]], [[1.0, 1.0], [1.0, 1.0]]), (list(range(65)), [0.0] * 65), ([], []), {}, {"<nope>": 1.0},
       ([3, 4], [1.0]), ([[3]], [[1.0]]), ([[3], [4], [5]], [[1.0]] * 3), ([3.5], [1.0]), ([True], [1.0]), "3", (3, 1.0),
       ([3], ["a"]), {3: "a"}, ([[3], [4, 5]], [[1.0], [1.0, 2.0]]), ([3],)]


@pytest.mark.parametrize("bias", BAD, ids=lambda b: repr(b)[:40])
def test_refused_values(bias):
    with pytest.raises(IckError):
        check(bias)


def test_refused_bans_and_combinations():
    wm3 = {"<pad>": 0, "<end>": 1, "<start>": 2}
    with pytest.raises(IckError):                       # nothing but <start> / <pad> is left
        D.check_column_bias("x", 1, 5, wm3, ([1, 3, 4], [NINF] * 3))
    D.check_column_bias("x", 1, 5, wm3, ([3, 4], [NINF] * 2))           # <end> stays
    with pytest.raises(IckError):
        check({3: 1.0}, num_beam_groups=2)
    with pytest.raises(IckError):
        check({3: 1.0}, force_tokens=[[4]])


@pytest.mark.parametrize("kw", [dict(column_bias={3: float("inf")}), dict(column_bias={"<nope>": 0.0}),
                                dict(column_bias={3: 1.0}, num_beam_groups=2, diversity_penalty=0.5),
                                dict(column_bias={3: 1.0}, force_tokens=[[4]]),
                                dict(column_bias=([V + K], [1.0]), beam_size=1)], ids=lambda k: repr(k)[:50])
def test_predict_beam_raises_before_any_device_work(kw):
    dec = cpu_decoder()
    kw = dict(dict(beam_size=4), **kw)
    with pytest.raises(IckError):
        dec.predict_beam(torch.zeros(1, 512, 14, 14), 12, synth.make_entities("geo", 1, K, V, 1), **kw)


def test_predict_sample_raises_before_any_device_work():
    dec = cpu_decoder()
    for bias in ({3: float("nan")}, ([3, 3], [1.0, 1.0]), ([[3], [4]], [[1.0], [1.0]])):
        with pytest.raises(IckError):
            dec.predict_sample(torch.zeros(1, 512, 14, 14), 12, synth.make_entities("geo", 1, K, V, 1), column_bias=bias)


# ------------------------------------------------------------------------------------------------ by hand
def hand_case(steps, cols, vals, beam=2, rules=None, state0=None):
    return CB.BiasBeamCase("hand", "plain", 1, beam, 2, 1, 0, 4, steps, rules=rules, state0=state0, bias_cols=cols,
                           bias_vals=vals)


def test_beam_steps_by_hand():
    """Columns {<pad>, <end>, entity}, probabilities (0.5, 0.3, 0.2), a boost of 1 on the entity.  Step 0: the keys are
    log 0.5 = -0.693, log 0.3 = -1.204, log 0.2 + 1 = -0.609, so the entity wins and <pad> follows; cum stays raw and the
    winner carries bsum = 1.  Step 1, probabilities (0.6, 0.3, 0.1) for both: the boosted hypothesis leads by its sum:
    log 0.2 + log 0.6 + 1 = -1.120 against log 0.5 + log 0.6 = -1.204."""
    x0 = np.log(np.float64([0.5, 0.3, 0.2])).astype(np.float32)
    x1 = np.log(np.float64([0.6, 0.3, 0.1])).astype(np.float32)
    case = hand_case([(0, SC.fixed({0: x0})), (1, SC.fixed({0: x1, 1: x1}))], [[2]], [[1.0]])
    tr = CB.run_beam(case)
    o = tr[0]["out"]
    assert tr[0]["info"]["tok"].tolist() == [2, 0] and o["bsum"].tolist() == [1.0, 0.0]
    assert np.allclose(o["cum"], [math.log(0.2), math.log(0.5)], atol=1e-6)
    assert [round(p[2], 3) for p in tr[0]["info"]["picks"][0]] == [-0.609, -0.693]
    o = tr[1]["out"]
    assert tr[1]["info"]["parent"].tolist() == [0, 1] and tr[1]["info"]["tok"].tolist() == [0, 0]
    assert np.allclose(o["cum"], [math.log(0.2 * 0.6), math.log(0.5 * 0.6)], atol=1e-6) and o["bsum"].tolist() == [1.0, 0.0]
    assert [round(p[2], 3) for p in tr[1]["info"]["picks"][0]] == [-1.120, -1.204]
    # a step-local bias forgets the sum and loses the boosted hypothesis: log 0.5 + log 0.3 = -1.897 beats -2.120
    assert CB.run_beam(case, step_local=True)[1]["info"]["parent"].tolist() == [1, 1]


def test_beam_ban_and_ended_by_hand():
    """-inf takes the entity out of the pool, not out of the sums: the survivors keep log 0.5 and log 0.3.  Then an ended
    hypothesis (cum -3, sum 2: key -1) against a live one (cum -1) expanded by 0.6 / 0.3 / 0.1: -1.511, -1, -2.204."""
    x0 = np.log(np.float64([0.5, 0.3, 0.2])).astype(np.float32)
    tr = CB.run_beam(hand_case([(0, SC.fixed({0: x0}))], [[2, 2]], [[NINF, 3.0]]))
    assert tr[0]["info"]["tok"].tolist() == [0, 1]
    assert np.allclose(tr[0]["out"]["cum"], [math.log(0.5), math.log(0.3)], atol=1e-6)
    x1 = np.log(np.float64([0.6, 0.3, 0.1])).astype(np.float32)
    st0 = [CB.bhyp([0, 1], -3.0, fin=True, bsum=2.0), CB.bhyp([0, 0], -1.0)]
    case = dataclasses.replace(hand_case([(2, SC.fixed({1: x1}))], [[2]], [[0.5]], state0=st0), max_len=6)
    tr = CB.run_beam(case)
    o = tr[0]["out"]
    assert tr[0]["info"]["parent"].tolist() == [0, 1] and o["fin"].tolist() == [1, 0]
    assert o["cum"][0] == -3.0 and o["bsum"].tolist() == [2.0, 0.0]
    assert [round(p[2], 3) for p in tr[0]["info"]["picks"][0]] == [-1.0, -1.511]


def sample_hand(top_k, cols, vals, top_p=1.0):
    case = CB.BiasSampleCase("hand", 1, 1, 3, 1, 1, 4, [(0, SC.fixed({0: np.float32([0, 1, 2, 3, 4])}))], top_k=top_k,
                             top_p=top_p, bias_cols=cols, bias_vals=vals)
    return CB.run_sample(case)[0]


def test_sample_steps_by_hand():
    """Scores 0..4.  top-k 2 keeps {3, 4}; with +1.5 on column 2 (3.5) it keeps {2, 4}.  -inf on column 4 with top-k 1
    leaves column 3 as the only kept one; log_prob is the raw 3 - lse(0..4) either way."""
    t = sample_hand(2, [[2]], [[1.5]])
    assert np.nonzero(t["info"]["kept"][0])[0].tolist() == [2, 4]
    assert np.nonzero(t["info"]["kept_unbiased"][0])[0].tolist() == [3, 4]
    t = sample_hand(1, [[4]], [[NINF]])
    lse = math.log(sum(math.exp(v) for v in range(5)))
    assert t["info"]["tok"][0] == 3 and abs(t["out"]["log_prob"][0, 0] - (3 - lse)) < 1e-12
    # top-p 0.6 alone keeps {4} (mass 0.636); -2 on column 4 makes column 3 the first (0.521 of the mass) and the run
    # of columns 2 and 4 (both 2 now) follows it whole
    t = sample_hand(0, [[4]], [[-2.0]], top_p=0.6)
    assert np.nonzero(t["info"]["kept_unbiased"][0])[0].tolist() == [4]
    assert np.nonzero(t["info"]["kept"][0])[0].tolist() == [2, 3, 4]


def test_draw_is_sample_ref_on_s_plus_b():
    g = np.random.default_rng(0)
    s = (g.integers(-40, 40, 200) / 8).astype(np.float32)
    b = np.zeros(200)
    b[[3, 50, 199]] = [1.5, -2.0, NINF]
    noise = sample_ref.gumbel(5, 0, 0, 0, 200)
    tok, keep, vals, ratio, cols = ref.draw(s, b, 0.75, 10, 0.9, noise, ban={7})
    allowed = np.array([c for c in range(200) if c not in (7, 199)])
    w, keep2, vals2, _ = sample_ref.draw((s + b.astype(np.float32))[allowed], 0.75, 10, 0.9, noise[allowed])
    assert tok == allowed[w] and np.array_equal(keep[allowed], keep2) and not keep[[7, 199]].any()
    assert np.array_equal(vals, vals2) and np.array_equal(cols, allowed)


# ------------------------------------------------------------------------------------------------ no bias: the old refs
PLAIN = [c for c in SC.BEAM if c.form == "plain" and c.Vx < 60000]


@pytest.mark.parametrize("case", PLAIN, ids=lambda c: c.name)
@pytest.mark.parametrize("zero", ["empty", "zeros"])
def test_beam_step_without_a_bias_is_select_ref(case, zero):
    cols = [[-1, -1]] * case.B if zero == "empty" else [[0, case.Vx - 1]] * case.B
    vals = [[5.0, NINF]] * case.B if zero == "empty" else [[0.0, -0.0]] * case.B
    mine = CB.run_beam(CB.BiasBeamCase(**case.__dict__, bias_cols=cols, bias_vals=vals))
    for a, b in zip(mine, SC.beam_trace(case.name)):
        for n in ("cum", "fin", "len", "seq", "anc", "n_done"):
            assert np.array_equal(a["out"][n], b["out"][n]), (case.name, n)
        assert (a["out"]["bsum"] == 0).all()
        for n in ("next_token", "next_mask", "x0", "dead", "parent", "tok"):
            assert np.array_equal(a["info"][n], b["info"][n]), (case.name, n)


@pytest.mark.parametrize("case", [c for c in SC.SAMPLE if c.Vx < 60000], ids=lambda c: c.name)
def test_sample_step_without_a_bias_is_select_ref(case):
    mine = CB.run_sample(CB.BiasSampleCase(**case.__dict__, bias_cols=[[3, -1]] * case.B, bias_vals=[[0.0, NINF]] * case.B))
    for a, b in zip(mine, SC.sample_trace(case.name)):
        for n in ("output", "finished", "log_prob", "n_done"):
            assert np.array_equal(a["out"][n], b["out"][n]), (case.name, n)
        assert a["info"]["tok"] == b["info"]["tok"]
        for r in a["info"]["kept"]:
            assert np.array_equal(a["info"]["kept"][r], b["info"]["kept"][r])


def oracle_case(variant, V=50, K=5, Fn=4, seed=3):
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    P = synth.make_params(variant, V, seed)
    ents = synth.make_entities(variant, 1, K, V, seed)
    facts = synth.make_facts(variant, 1, Fn, K, seed) if variant != "geo" else None
    return cfg, P, ents, facts, synth.make_enc_out(1, seed)


@pytest.mark.parametrize("variant,beam,rules", [("geo", 3, True), ("knowledge", 2, False)])
def test_search_without_a_bias_is_the_rules_beam(variant, beam, rules):
    cfg, P, ents, facts, enc = oracle_case(variant)
    Vx = 55 + (4 if facts is not None else 0)
    kw = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3) if rules else {}
    want = predict_beam_rules(cfg, P, enc, 7, ents, facts, beam, **kw)
    for bias in (None, np.zeros(Vx)):
        mine = ref.predict_beam_bias(cfg, P, enc, 7, ents, facts, beam, bias=bias, **kw)
        assert torch.equal(mine[0], want[0]) and abs(mine[1] - want[1]) < 1e-5 and abs(mine[2] - want[2]) < 1e-5
        assert [h[0] for h in mine[3]] == [h[0] for h in want[3]] and all(h[3] == 0 for h in mine[3])


def test_search_with_a_ban_never_emits_the_column():
    cfg, P, ents, facts, enc = oracle_case("geo")
    plain = predict_beam_rules(cfg, P, enc, 7, ents, None, 3)
    w = plain[0].tolist()[0]
    bias = np.zeros(55)
    bias[w] = NINF
    mine = ref.predict_beam_bias(cfg, P, enc, 7, ents, None, 3, bias=bias)
    assert all(w not in h[0] for h in mine[3]) and mine[1] <= plain[1] + 1e-6


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", CB.BEAM, ids=lambda c: c.name)
def test_beam_case_is_decidable_and_shows_its_tags(case):
    trace = CB.beam_trace(case.name)                    # raises Undecidable otherwise
    assert all(len(l) <= 64 and len(l) == len(v) for l, v in zip(case.bias_cols, case.bias_vals))
    assert len(case.bias_cols) == case.B
    for l in case.bias_vals:
        assert all(v == NINF or float(v * 8).is_integer() for v in l)      # multiples of 1/8: bias sums are exact
    for tag in case.expect:
        assert CB.BEAM_TAGS[tag](case, trace), (case.name, tag)


@pytest.mark.parametrize("case", CB.SAMPLE, ids=lambda c: c.name)
def test_sample_case_is_decidable_and_shows_its_tags(case):
    trace = CB.sample_trace(case.name)
    for tag in case.expect:
        assert CB.SAMPLE_TAGS[tag](case, trace), (case.name, tag)


def test_every_required_tag_is_exhibited():
    assert {t for c in CB.BEAM for t in c.expect} == CB.BEAM_TAGS_REQUIRED
    assert {t for c in CB.SAMPLE for t in c.expect} == CB.SAMPLE_TAGS_REQUIRED


# ------------------------------------------------------------------------------------------------ ABI
def test_bias_layout_matches_header(built_lib):
    import ick_amd.lib as L
    src = '#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu %d", sizeof(ick_decode_bias), ICK_BIAS_MAX);}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size, nmax = (int(x) for x in subprocess.check_output([exe]).split())
    assert ctypes.sizeof(L.DecodeBias) == size == 24 and nmax == D.BIAS_MAX == ref.BIAS_MAX == 64


def test_library_exports_and_binds_the_biased_symbols(built_lib):
    import ick_amd.lib as L
    lib = ctypes.CDLL(built_lib)
    for s in ("ick_decode_select_beam_biased", "ick_decode_select_sample_biased"):
        assert hasattr(lib, s) and s in L.SIGNATURES and len(L.SIGNATURES[s]) == 6
    # argument errors come back without a launch (no device is touched): null pointers, sum missing for the beam entry
    c, bs, st, b = L.DecodeCtx(), L.BeamState(), L.SampleState(), L.DecodeBias()
    loaded = L.load()
    assert loaded.ick_decode_select_beam_biased(ctypes.byref(c), ctypes.byref(bs), None, None, 0, None) != 0
    assert loaded.ick_decode_select_beam_biased(ctypes.byref(c), ctypes.byref(bs), None, ctypes.byref(b), 0, None) != 0
    assert loaded.ick_decode_select_sample_biased(ctypes.byref(c), ctypes.byref(st), None, None, 0, None) != 0
    assert loaded.ick_decode_select_sample_biased(ctypes.byref(c), ctypes.byref(st), None, ctypes.byref(b), 0, None) != 0
