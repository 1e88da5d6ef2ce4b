"""CPU checks of caption prefixes (predict_beam / predict_sample(prefix=)): check_prefix's refusals and the
table it builds, the references of tests/prefix_ref.py pinned to the references they are built on, the state a prefix
leaves behind, the case table of tests/prefix_cases.py (every case decidable, every tag true of the reference's own
trace), the float64 oracle's own decision margins on the end-to-end cases of tests/test_prefix_gpu.py, and the ABI."""
import dataclasses
import inspect

import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.decoder as D
import ick_amd.lib as L
import ick_amd.ops as ops
import ick_amd.synth as synth
from ick_amd.lib import IckError
import column_bias_cases as CB
import column_bias_ref
import prefix_cases as PC
import prefix_ref as ref
import select_cases as SC
import select_ref
from test_sample_gpu import BOUNDARY, MARGIN

V, K, MAXLEN = 50, 5, 6
WM = synth.make_word_map(V)
NINF = float("-inf")


def check(prefix, B=2, Vx=V + K, max_len=MAXLEN, **kw):
    return D.check_prefix("x", B, Vx, max_len, WM, prefix, **kw)


# ------------------------------------------------------------------------------------------------ check_prefix
def test_none_is_the_default_and_predict_does_not_take_it():
    assert check(None) is None
    for fn in (D.DecoderTransformer.predict_beam, D.DecoderTransformer.predict_sample):
        assert inspect.signature(fn).parameters["prefix"].default is None
    assert "prefix" not in inspect.signature(D.DecoderTransformer.predict).parameters


def test_the_table_it_builds():
    t = check([[3, V + 1, -1], [7, -1, -1]])
    assert t.dtype == torch.int32 and t.shape == (2, MAXLEN)
    assert t.tolist() == [[3, V + 1, -1, -1, -1, -1], [7, -1, -1, -1, -1, -1]]
    for same in (torch.tensor([[3, V + 1, -1], [7, -1, -1]], dtype=torch.int32), [[3, V + 1], [7]], ((3, V + 1), (7,))):
        assert torch.equal(check(same), t)
    full = check([list(range(3, 3 + MAXLEN))] * 2)                  # Pn = max_pred_len
    assert full.tolist() == [list(range(3, 3 + MAXLEN))] * 2
    assert check([[-1, -1]] * 2).tolist() == [[-1] * MAXLEN] * 2    # all free
    assert check([[3]] * 2, max_len=9).shape == (2, 9)              # the shape follows max_pred_len, not Pn


def test_broadcast_and_words():
    assert check([3, 4]).tolist() == [[3, 4, -1, -1, -1, -1]] * 2
    assert check(torch.tensor([3, 4])).tolist() == [[3, 4, -1, -1, -1, -1]] * 2
    assert check(["w3", V + 2, "<unk>"]).tolist() == [[3, V + 2, WM["<unk>"], -1, -1, -1]] * 2
    assert check([["w3", "w4"], ["w9"]]).tolist() == [[3, 4, -1, -1, -1, -1], [9, -1, -1, -1, -1, -1]]


BAD = [
    ([WM["<start>"]], "<start>"), (["<end>"], "<end>"), ([[3, WM["<pad>"]], [3, 4]], "<pad>"),
    ([V + K], "column ids"), ([-2], "column ids"), ([[3, -1, 4], [3, 4, 5]], "behind a -1"),
    ([[3, 4]], "integer tensor"), ([[3], [4], [5]], "integer tensor"), (list(range(3, 3 + MAXLEN + 1)), "integer tensor"),
    ([], "integer tensor"), ([3.5], "integer tensor"), (torch.zeros(2, 2, 2, dtype=torch.long), "integer tensor"),
    ("w3", "integer tensor"), (["<nope>"], "unknown word"),
]


@pytest.mark.parametrize("prefix,says", BAD, ids=lambda v: repr(v)[:30])
def test_refusals_by_name(prefix, says):
    with pytest.raises(IckError, match=says):
        check(prefix)


def test_refused_compositions():
    with pytest.raises(IckError, match="force_tokens"):
        check([3], force_tokens=[[4]])
    bias = D.check_column_bias("x", 2, V + K, WM, ([[3, 9], [4, 9]], [[NINF, 1.0], [0.5, NINF]]))
    with pytest.raises(IckError, match="caption 1's prefix holds at step 1"):
        check([[4, 8], [4, 9]], bias=bias)
    assert check([[4, 9], [3, 8]], bias=bias) is not None          # the same columns in the other caption: no clash
    m = ick_amd.load_models("geo")
    dec = m.DecoderTransformer(word_map=WM, emb_dim=300, decoder_dim=512, encoder_dim=512, num_heads=10, num_layers=3)
    ents = synth.make_entities("geo", 1, K, V, 1)
    for kw in (dict(prefix=[3], force_tokens=[[4]]), dict(prefix=["<end>"]), dict(prefix=[3], column_bias={3: NINF}),
               dict(prefix=[V + K])):
        with pytest.raises(IckError):
            dec.predict_beam(torch.zeros(1, 512, 14, 14), MAXLEN, ents, beam_size=3, **kw)
    for kw in (dict(prefix=["<pad>"]), dict(prefix=[3], column_bias={3: NINF}), dict(prefix=[[3, -1, 3]])):
        with pytest.raises(IckError):
            dec.predict_sample(torch.zeros(1, 512, 14, 14), MAXLEN, ents, **kw)


def test_bindings_and_ops_take_the_prefix():
    assert [f[0] for f in L.DecodePrefix._fields_] == ["cols"]
    for name, n in (("ick_decode_select_beam_prefix", 8), ("ick_decode_select_sample_prefix", 7)):
        assert len(L.SIGNATURES[name]) == n
    assert "prefix" in inspect.signature(ops.decode_select_beam).parameters
    assert "prefix" in inspect.signature(ops.decode_select_sample).parameters
    with pytest.raises(IckError):                       # refused before the library is touched
        ops.decode_select_beam(L.DecodeCtx(), L.BeamState(), 0, None, None, L.DecodeConstraints(), None, L.DecodePrefix())
    with pytest.raises(IckError):
        ops.decode_select_beam(L.DecodeCtx(), L.BeamState(), 0, None, L.DecodeDiversity(), None, L.DecodeBias(), L.DecodePrefix())


# ------------------------------------------------------------------ the new references are the old ones when nothing is forced
def same_state(a, b):
    assert a.keys() == b.keys()
    for n in a:
        if a[n] is None or b[n] is None:
            assert a[n] is None and b[n] is None, n
        else:
            assert np.array_equal(np.asarray(a[n]), np.asarray(b[n])), n


EMPTY = [None, "minus_ones"]


@pytest.mark.parametrize("empty", EMPTY)
@pytest.mark.parametrize("case", [c for c in SC.BEAM if c.form != "forced" and c.Vx < 60000] + [c for c in CB.BEAM if c.Vx < 60000],
                         ids=lambda c: c.name)
def test_beam_step_with_an_empty_table_is_the_existing_reference(case, empty):
    biased = isinstance(case, CB.BiasBeamCase)
    trace = CB.beam_trace(case.name) if biased else SC.beam_trace(case.name)
    cls = PC.PrefixBiasBeamCase if biased else PC.PrefixBeamCase
    mine = cls(**case.__dict__, prefix=None if empty is None else [[-1] * case.max_len] * case.B)
    t = SC.tables(case)
    for step in trace:
        out, info = ref.beam_step(mine, step["st"], step["rows"], step["pos"], t)
        same_state(out, step["out"])
        for n in ("next_token", "next_mask", "x0", "dead", "parent", "tok"):
            assert np.array_equal(info[n], step["info"][n]), n


@pytest.mark.parametrize("case", [c for c in SC.SAMPLE if c.Vx < 60000] + [c for c in CB.SAMPLE if c.Vx < 60000],
                         ids=lambda c: c.name)
def test_sample_step_with_an_empty_table_is_the_existing_reference(case):
    biased = isinstance(case, CB.BiasSampleCase)
    trace = CB.sample_trace(case.name) if biased else SC.sample_trace(case.name)
    cls = PC.PrefixBiasSampleCase if biased else PC.PrefixSampleCase
    mine = cls(**case.__dict__, prefix=[[-1] * case.max_len] * case.B)
    t = SC.tables(case)
    for step in trace:
        out, info = ref.sample_step(mine, step["st"], step["rows"], step["pos"], t)
        same_state(out, step["out"])
        assert info["tok"] == step["info"]["tok"] and np.array_equal(info["x0"], step["info"]["x0"])


def test_the_patched_name_is_put_back():
    case = PC.BEAM_BY_NAME["beam1_ngram_facts"]
    PC.run_beam(case)
    import beam_rules_ref
    for mod in (select_ref, column_bias_ref):
        assert mod.banned_set is beam_rules_ref.banned_set


# ------------------------------------------------------------------------------------- the state a prefix leaves
def test_after_a_prefix_one_hypothesis_holds_it_and_the_rest_is_unused():
    fn = PC.rows_fn(21, -8.0)
    pre = [7, 52]
    a = PC.PrefixBeamCase("a", "plain", 1, 3, 50, 4, 0, 6, PC.steps(3, fn), prefix=[pre])
    tr = PC.run_beam(a)
    logp = 0.0
    for t, f in zip(tr[:2], pre):
        x = t["rows"][0].astype(np.float64)
        logp += x[f] - select_ref.lse64(x)
        assert sorted(t["rows"]) == [0]                              # one live row through the prefix
    st = tr[2]["st"]
    assert abs(st["cum"][0] - logp) < 1e-12 and (st["cum"][1:] == SC.NEG).all() and st["n_done"] == 2
    assert st["seq"][0, :2].tolist() == pre and st["fin"][0] == 0
    # the same search entered through state0 with that hypothesis
    b = PC.PrefixBeamCase("b", "plain", 1, 3, 50, 4, 0, 6, [(2, fn)], state0=[SC.hyp(pre, logp), None, None], prefix=[pre])
    tb = PC.run_beam(b)
    for n in ("cum", "fin", "seq", "n_done"):
        assert np.array_equal(tr[2]["out"][n], tb[0]["out"][n]), n
    assert np.array_equal(tr[2]["info"]["x0"], tb[0]["info"]["x0"])
    assert not tr[2]["info"]["dead"].any() and (tr[2]["info"]["parent"] == 0).all()         # the fan-out: one parent


# ------------------------------------------------------------------------------------------------ the case table
@pytest.mark.parametrize("case", PC.BEAM, ids=lambda c: c.name)
def test_beam_cases_are_decidable_and_their_tags_true(case):
    tr = PC.beam_trace(case.name)
    assert PC.not_argmax_everywhere(case, tr), "a forced column is its row's best: the case shows nothing"
    for tag in case.expect:
        assert PC.BEAM_TAGS[tag](case, tr), (case.name, tag)
    assert case.max_len == 6


@pytest.mark.parametrize("case", PC.SAMPLE, ids=lambda c: c.name)
def test_sample_cases_are_decidable_and_their_tags_true(case):
    tr = PC.sample_trace(case.name)
    assert PC.not_argmax_everywhere(case, tr), "a forced column is its row's best: the case shows nothing"
    for tag in case.expect:
        assert PC.SAMPLE_TAGS[tag](case, tr), (case.name, tag)
    for t in tr:                                                     # a forced step: the column, with its raw log-probability
        for r, f in t["info"]["forced"].items():
            if f >= 0:
                assert t["out"]["output"][r, t["pos"]] == f


def test_every_tag_is_exhibited():
    assert PC.BEAM_TAGS_REQUIRED == {t for c in PC.BEAM for t in c.expect}
    assert PC.SAMPLE_TAGS_REQUIRED == {t for c in PC.SAMPLE for t in c.expect}
    assert {c.beam for c in PC.BEAM} >= {1, 3, 8} and any(c.form == "diverse" and c.lam > 0 for c in PC.BEAM)
    assert any(isinstance(c, CB.BiasBeamCase) for c in PC.BEAM) and any(isinstance(c, CB.BiasSampleCase) for c in PC.SAMPLE)
    assert any(c.Vx > 16384 for c in PC.SAMPLE) and any(c.F > 0 for c in PC.BEAM)


# ------------------------------------------------------------------ the oracle's own margins on the end-to-end cases
def _bias_vec(cfg, ents, facts):
    Vx = cfg.vocab_size + ents.shape[1] + (facts.shape[1] if facts is not None else 0)
    ids, vals = PC.e2e_bias(cfg.vocab_size)
    return column_bias_ref.bias_row(Vx, ids, vals)


@pytest.mark.parametrize("name", list(PC.E2E_BEAM))
def test_the_oracle_decides_every_free_beam_step_by_ten_margins(name):
    variant, V_, seed, kw = PC.E2E_BEAM[name]
    cfg, P, ents, facts, enc = PC.e2e_inputs(variant, V_, seed)
    prefix = PC.e2e_prefix(V_, facts is not None)
    kw = dict(kw)
    bias = _bias_vec(cfg, ents, facts) if kw.pop("column_bias", None) else None
    for b in range(PC.E2E_B):
        fb = None if facts is None else facts[b:b + 1]
        got = ref.predict_beam_prefix(cfg, P, enc[b:b + 1], PC.E2E_LEN, ents[b:b + 1], fb, prefix=prefix[b], bias=bias, **kw)
        print(name, b, "margin %.3g" % got["margin"], got["best"].tolist())
        assert got["margin"] >= 10 * MARGIN, (name, b, got["margin"])
        p = sum(1 for c in prefix[b] if c >= 0)
        assert got["best"].tolist()[:p] == prefix[b][:p]


@pytest.mark.parametrize("name", list(PC.E2E_SAMPLE))
def test_the_oracle_decides_every_free_draw_by_ten_margins(name):
    variant, V_, seed, kw = PC.E2E_SAMPLE[name]
    cfg, P, ents, facts, enc = PC.e2e_inputs(variant, V_, seed)
    prefix = PC.e2e_prefix(V_, facts is not None)
    kw = dict(kw)
    bias = _bias_vec(cfg, ents, facts) if kw.pop("column_bias", None) else None
    n, s = kw.pop("num_samples"), kw.pop("seed")
    for b in range(PC.E2E_B):
        fb = None if facts is None else facts[b:b + 1]
        toks, _, margin, boundary = ref.sample_cpu(cfg, P, enc[b:b + 1], ents[b:b + 1], fb, prefix[b], b, n, s, PC.E2E_LEN,
                                                   bias=bias, **kw)
        print(name, b, "margin %.3g boundary %.3g" % (margin, boundary), toks)
        assert margin >= 10 * MARGIN and boundary >= 10 * BOUNDARY, (name, b, margin, boundary)
