"""Caption prefixes on the device.  Kernel level: every case of tests/prefix_cases.py through
ick_decode_select_beam_prefix / ick_decode_select_sample_prefix on the hand-filled context of
tests/test_select_envelope_gpu.py, against the step references of tests/prefix_ref.py -- integers exactly, cum and
log_prob at that test's 1e-4, bias sums exactly -- with guards and poisoned buffers; an all-empty table bit for bit
against the rules, diverse and biased entries; argument errors without a launch.  End to end: predict_beam /
predict_sample(prefix=) on the small geo and knowledge models against the CPU searches and draws over the oracle's
scores, in all three product modes of the large GEMM tiles (tests/test_prefix_cpu.py holds the oracle's own margins to
ten times MARGIN, so no device decision is excused)."""
import ctypes

import numpy as np
import pytest
import torch

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
import test_column_bias_gpu as TB
import test_select_envelope_gpu as E
from attn_ref import cross_weights, prefix_feeds
from decode_ref import Fp64Decode
from test_decode_attention_gpu import check_weights
from test_sample_gpu import make_case, upto_end

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # cum and log_prob against float64: test_select_envelope_gpu.py's
SCORE_TOL = 1e-3                # a device beam score against the oracle's (test_decode_rules_gpu.py, test_column_bias_gpu.py)
NINF = float("-inf")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ kernel level
def _with_prefix(h, case, table=None):
    t = ref.table(getattr(case, "prefix", None), case.B, case.max_len) if table is None else table
    h.add("pcols", case.B, (case.max_len,), torch.int32, t)
    h.px = L.DecodePrefix()
    h.px.cols = h.bufs["pcols"].ptr()
    return h


class PrefixBeamHarness(TB.BiasBeamHarness):
    """The beam harness with a prefix table; a case without bias slots runs without an ick_decode_bias."""

    def __init__(self, case, st, table=None):
        self.biased = isinstance(case, CB.BiasBeamCase)
        if self.biased:
            super().__init__(case, st)
        else:
            E.BeamHarness.__init__(self, case, st)
            self.bias = None
        _with_prefix(self, case, table)

    def select(self, pos):
        ops.decode_select_beam(self.ctx, self.bs, pos, self.rules, self.div, None, self.bias, self.px)
        torch.cuda.synchronize()


class PrefixSampleHarness(TB.BiasSampleHarness):
    def __init__(self, case, st, table=None):
        self.biased = isinstance(case, CB.BiasSampleCase)
        if self.biased:
            super().__init__(case, st)
        else:
            E.SampleHarness.__init__(self, case, st)
            self.bias = None
        _with_prefix(self, case, table)

    def select(self, pos):
        ops.decode_select_sample(self.ctx, self.state, pos, self.rules, self.bias, self.px)
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", PC.BEAM, ids=lambda c: c.name)
def test_prefix_beam_selection_matches_the_reference_step_by_step(case):
    trace = PC.beam_trace(case.name)
    h = PrefixBeamHarness(case, trace[0]["st"])
    cur = 0
    for t in trace:
        pos, out, info = t["pos"], t["out"], t["info"]
        what = (case.name, pos)
        nxt = h.point(cur)
        h.write_rows(t["rows"])
        h.bufs["rec"].t.fill_(NAN)              # a forced step must write every record slot stage 2 reads
        h.poison_outputs()
        h.select(pos)
        b = h.bufs
        cum, fin = b["cum"].np().astype(np.float64), b["fin"].np()
        print(what, "cum", cum, "want", out["cum"])
        dead = out["cum"] == SC.NEG
        assert np.array_equal(cum == SC.NEG, dead), what
        assert np.abs(cum[~dead] - out["cum"][~dead]).max(initial=0.0) < TOL, what
        if h.biased:
            assert np.array_equal(b["bsum"].np().astype(np.float64), out["bsum"]), (what, b["bsum"].np(), out["bsum"])
        assert np.array_equal(fin, out["fin"]), what
        if case.rules is not None:
            assert np.array_equal(b["len"].np(), out["len"]), what
        assert int(b["n_done"].np()[0]) == out["n_done"], (what, int(b["n_done"].np()[0]), out["n_done"])
        keep = ~info["dead"]
        assert np.array_equal(h.seq[nxt].np()[keep], out["seq"][keep]), (what, h.seq[nxt].np(), out["seq"])
        assert np.array_equal(h.anc[nxt].np()[keep], out["anc"][keep]), (what, h.anc[nxt].np(), out["anc"])
        if h.cap:
            assert np.array_equal(h.cap[nxt].np()[keep], out["cap"][keep]), (what, h.cap[nxt].np(), out["cap"])
        h.check_next(info, np.ones(case.R, bool), what)
        h.check_x0(info, info["x0_written"], what)
        h.check_guards(what)
        cur = nxt


@pytest.mark.parametrize("case", PC.SAMPLE, ids=lambda c: c.name)
def test_prefix_sampled_selection_matches_the_reference_step_by_step(case):
    trace = PC.sample_trace(case.name)
    h = PrefixSampleHarness(case, trace[0]["st"])
    R_ = case.R
    for t in trace:
        pos, out, info = t["pos"], t["out"], t["info"]
        what = (case.name, pos)
        h.write_rows(t["rows"])
        h.poison_outputs()
        b = h.bufs
        live = np.array([r in t["rows"] for r in range(R_)])
        if live.any():
            rows = torch.from_numpy(np.nonzero(live)[0]).cuda()
            b["output"].t[rows, pos] = E.POISON_I
            b["log_prob"].t[rows, pos] = NAN
        h.select(pos)
        written = np.full(R_, bool(info["written"]))
        print(what, "tokens", b["output"].np()[:, pos], "want", out["output"][:, pos], "log_prob", b["log_prob"].np()[:, pos])
        assert np.array_equal(b["output"].np(), out["output"]), (what, b["output"].np(), out["output"])
        assert np.array_equal(b["finished"].np(), out["finished"]), what
        assert int(b["n_done"].np()[0]) == out["n_done"], what
        assert np.abs(b["log_prob"].np().astype(np.float64) - out["log_prob"]).max() < TOL, what
        if "cap_buf" in b:
            assert np.array_equal(b["cap_buf"].np(), out["cap_buf"]), (what, b["cap_buf"].np(), out["cap_buf"])
        h.check_next(info, written, what)
        h.check_x0(info, written & (pos + 1 < case.max_len), what)
        h.check_guards(what)


EMPTY_BEAM = [("sc", n) for n in ("ties_1023", "tie_chunk_1025", "lp_order", "ngram_ban", "ban_chunk1_seam", "script_plain",
                                  "script_rules", "beam1", "div_penalty", "div_ended_rules", "script_diverse")] + \
             [("cb", n) for n in ("edge_1025", "persistence", "lp_and_bias", "ban_beats_bias", "script_batch")]


@pytest.mark.parametrize("table,name", EMPTY_BEAM, ids=lambda v: v)
def test_an_empty_table_is_the_rules_diverse_and_biased_beam_bit_for_bit(table, name):
    biased = table == "cb"
    base = (CB.BEAM_BY_NAME if biased else SC.BEAM_BY_NAME)[name]
    trace = CB.beam_trace(name) if biased else SC.beam_trace(name)
    cls = PC.PrefixBiasBeamCase if biased else PC.PrefixBeamCase
    mine = TB._beam_bits(PrefixBeamHarness(cls(**base.__dict__, prefix=None), trace[0]["st"]), trace)
    theirs = TB._beam_bits((TB.BiasBeamHarness if biased else E.BeamHarness)(base, trace[0]["st"]), trace)
    assert mine == theirs


EMPTY_SAMPLE = [("sc", n) for n in ("topk_run_zero", "topp_run_kept", "temperature_philox", "ban_on_max", "rules_16385",
                                    "end_and_finished", "script_sample", "topk_1")] + \
               [("cb", n) for n in ("s_vx5_topk", "s_16385", "s_ban_and_bias", "s_script")]


@pytest.mark.parametrize("table,name", EMPTY_SAMPLE, ids=lambda v: v)
def test_an_empty_table_is_the_rules_and_biased_sampler_bit_for_bit(table, name):
    biased = table == "cb"
    base = (CB.SAMPLE_BY_NAME if biased else SC.SAMPLE_BY_NAME)[name]
    trace = CB.sample_trace(name) if biased else SC.sample_trace(name)
    cls = PC.PrefixBiasSampleCase if biased else PC.PrefixSampleCase

    def run(h):
        got = []
        for t in trace:
            h.write_rows(t["rows"])
            h.poison_outputs()
            h.select(t["pos"])
            got.append([h.bufs[n].np().tobytes() for n in ("output", "finished", "log_prob", "n_done", "x0", "next_token",
                                                           "next_mask")])
        return got

    mine = run(PrefixSampleHarness(cls(**base.__dict__, prefix=None), trace[0]["st"]))
    assert mine == run((TB.BiasSampleHarness if biased else E.SampleHarness)(base, trace[0]["st"]))


def test_entry_points_refuse_bad_arguments_without_a_launch():
    case = PC.BEAM_BY_NAME["bias_on_prefix"]
    trace = PC.beam_trace(case.name)
    h = PrefixBeamHarness(case, trace[0]["st"])
    h.point(0)
    h.write_rows(trace[0]["rows"])
    h.poison_outputs()
    before = h.bufs["cum"].np().copy()
    lib = L.load()
    keep = h.px.cols
    h.px.cols = None                                    # a NULL table
    E.refused(lambda: h.select(0))
    h.px.cols = keep
    for field in ("cols", "vals", "sum"):               # an incomplete ick_decode_bias
        was = getattr(h.bias, field)
        setattr(h.bias, field, None)
        E.refused(lambda: h.select(0))
        setattr(h.bias, field, was)
    ref_ = ctypes.byref
    assert lib.ick_decode_select_beam_prefix(ref_(h.ctx), ref_(h.bs), None, None, ref_(h.bias), None, 0, None) != 0
    pen = torch.zeros(1, device="cuda")
    dv = L.DecodeDiversity()
    dv.groups, dv.penalty = 1, pen.data_ptr()           # diversity and bias together
    assert lib.ick_decode_select_beam_prefix(ref_(h.ctx), ref_(h.bs), None, ref_(dv), ref_(h.bias), ref_(h.px), 0, None) != 0
    dv.groups = 2                                       # groups that do not divide the beam of 3
    assert lib.ick_decode_select_beam_prefix(ref_(h.ctx), ref_(h.bs), None, ref_(dv), None, ref_(h.px), 0, None) != 0
    h.ctx.rows_per_sample = 9                           # an unsupported size
    E.refused(lambda: h.select(0))
    h.ctx.rows_per_sample = case.beam
    torch.cuda.synchronize()
    assert np.array_equal(h.bufs["cum"].np(), before) and np.isnan(h.bufs["x0"].np()).all()       # nothing ran
    h.check_guards("beam")
    sc = PC.SAMPLE_BY_NAME["s_biased"]
    st = PC.sample_trace(sc.name)
    s = PrefixSampleHarness(sc, st[0]["st"])
    s.write_rows(st[0]["rows"])
    s.poison_outputs()
    keep = s.px.cols
    s.px.cols = None
    E.refused(lambda: s.select(0))
    s.px.cols = keep
    s.bias.vals = None
    E.refused(lambda: s.select(0))
    assert lib.ick_decode_select_sample_prefix(ref_(s.ctx), ref_(s.state), None, None, None, 0, None) != 0
    torch.cuda.synchronize()
    assert np.isnan(s.bufs["x0"].np()).all() and (s.bufs["output"].np() == 0).all()
    s.check_guards("sample")
    with pytest.raises(IckError):                       # ops refuses the composition that is out of scope
        ops.decode_select_beam(h.ctx, h.bs, 0, None, None, L.DecodeConstraints(), None, h.px)


# ------------------------------------------------------------------------------------------------ end to end
def args_of(enc, max_len, ents, facts):
    return [enc.cuda(), max_len, ents] + ([facts.cuda()] if facts is not None else [])


def one(x, b):
    return None if x is None else x[b:b + 1]


def graphs(dec):
    return len(dec.__dict__.get("_graphs", {}))


def kinds(dec):
    return {k[0] for k in dec.__dict__.get("_graphs", {})}


def e2e(variant, V, seed):
    dec, cfg, P, ents, facts, enc = make_case(variant, PC.E2E_B, PC.E2E_K, V, PC.E2E_F, seed)
    return dec, cfg, P, ents, facts, enc, PC.e2e_prefix(V, facts is not None)


def plen(row):
    return sum(1 for c in row if c >= 0)


@pytest.mark.parametrize("name", list(PC.E2E_BEAM))
def test_beam_search_is_the_cpu_search_over_the_oracles_scores(name, gemm_split):
    variant, V, seed, kw = PC.E2E_BEAM[name]
    dec, cfg, P, ents, facts, enc, prefix = e2e(variant, V, seed)
    kw = dict(kw)
    bias = None
    if kw.pop("column_bias", None):
        kw["column_bias"] = PC.e2e_bias(V)
        Vx = V + ents.shape[1] + (facts.shape[1] if facts is not None else 0)
        bias = column_bias_ref.bias_row(Vx, *PC.e2e_bias(V))
    beam = kw["beam_size"]
    seq, score, allseq, allscore = [x.cpu() for x in dec.predict_beam(*args_of(enc, PC.E2E_LEN, ents, facts), prefix=prefix,
                                                                      return_all=True, **kw)]
    assert seq.shape == (PC.E2E_LEN, PC.E2E_B) and allseq.shape == (PC.E2E_B, beam, PC.E2E_LEN)
    cpu_kw = {k: v for k, v in kw.items() if k != "column_bias"}
    for b in range(PC.E2E_B):
        want = ref.predict_beam_prefix(cfg, P, enc[b:b + 1], PC.E2E_LEN, ents[b:b + 1], one(facts, b), prefix=prefix[b],
                                       bias=bias, **cpu_kw)
        what = (name, b)
        print(what, "oracle margin %.3g" % want["margin"], "best", want["best"].tolist(), "device", seq[:, b].tolist())
        p = plen(prefix[b])
        assert seq[:p, b].tolist() == prefix[b][:p], what
        assert seq[:, b].tolist() == want["best"].tolist(), what
        assert abs(score[b].item() - want["score"]) < SCORE_TOL, (what, score[b].item(), want["score"])
        for h, hyp in enumerate(want["hyps"]):
            if hyp is None:                             # a slot no hypothesis ever filled
                assert allscore[b, h].item() == NINF and (allseq[b, h] == cfg.pad).all(), (what, h)
                continue
            mine = upto_end(allseq[b, h].tolist(), cfg.end)
            assert mine[:len(hyp[0])] == hyp[0] and abs(allscore[b, h].item() - hyp[1]) < SCORE_TOL, (what, h, mine, hyp)
            assert mine[:p] == prefix[b][:p], (what, h)
        if p == PC.E2E_LEN:
            assert sum(h is not None for h in want["hyps"]) == kw.get("num_beam_groups", 1)


@pytest.mark.parametrize("name", list(PC.E2E_SAMPLE))
def test_sampled_tokens_are_the_cpu_draws_over_the_oracles_scores(name, gemm_split):
    variant, V, seed, kw = PC.E2E_SAMPLE[name]
    dec, cfg, P, ents, facts, enc, prefix = e2e(variant, V, seed)
    kw = dict(kw)
    bias = None
    if kw.pop("column_bias", None):
        kw["column_bias"] = PC.e2e_bias(V)
        Vx = V + ents.shape[1] + (facts.shape[1] if facts is not None else 0)
        bias = column_bias_ref.bias_row(Vx, *PC.e2e_bias(V))
    n, s = kw["num_samples"], kw["seed"]
    seqs, lps = [x.cpu() for x in dec.predict_sample(*args_of(enc, PC.E2E_LEN, ents, facts), prefix=prefix,
                                                      return_log_probs=True, **kw)]
    cpu_kw = {k: v for k, v in kw.items() if k not in ("column_bias", "num_samples", "seed")}
    for b in range(PC.E2E_B):
        toks, lp, margin, boundary = ref.sample_cpu(cfg, P, enc[b:b + 1], ents[b:b + 1], one(facts, b), prefix[b], b, n, s,
                                                    PC.E2E_LEN, bias=bias, **cpu_kw)
        for j in range(n):
            r = b * n + j
            got = upto_end(seqs[:, r].tolist(), cfg.end)
            print((name, b, j), "device", got, "oracle", toks[j], "margin %.3g" % margin)
            assert got == toks[j], (name, b, j)                     # every token restated, none excused
            assert np.abs(lps[:len(got), r].double().numpy() - np.array(lp[j])).max() < TOL, (name, b, j)
            assert (seqs[len(got):, r] == cfg.pad).all() and (lps[len(got):, r] == 0).all()


def test_refeeding_its_own_beginning_reproduces_a_caption():
    dec, cfg, P, ents, facts, enc, _ = e2e("knowledge", 50, 3)
    args = args_of(enc, PC.E2E_LEN, ents, facts)
    rule = dict(no_repeat_ngram_size=2)
    seq, score, _, _ = [x.clone() for x in dec.predict_beam(*args, beam_size=1, return_all=True, **rule)]
    skw = dict(num_samples=2, seed=21, top_p=0.9, return_log_probs=True)
    sam, slp = [x.clone() for x in dec.predict_sample(*args, **skw)]
    for p in (1, 3):
        live = [b for b in range(PC.E2E_B) if cfg.end not in seq[:p, b].tolist()]
        pre = [seq[:p, b].tolist() if b in live else [-1] * p for b in range(PC.E2E_B)]
        again, ascore, _, _ = dec.predict_beam(*args, beam_size=1, return_all=True, prefix=pre, **rule)
        assert live and torch.equal(again, seq)
        gap = (ascore - score).abs().max().item()
        print("beam 1 re-fed %d tokens: max score gap %.2e" % (p, gap))
        assert gap < TOL
        # every sample of a caption shares its prefix: sample 0's beginning goes back in, and sample 0 comes out again
        rows = [b * 2 for b in range(PC.E2E_B) if cfg.end not in sam[:p, b * 2].tolist()]
        pre = [sam[:p, b * 2].tolist() if b * 2 in rows else [-1] * p for b in range(PC.E2E_B)]
        tok2, lp2 = dec.predict_sample(*args, prefix=pre, **skw)
        assert rows and torch.equal(tok2[:, rows], sam[:, rows])
        gap = (lp2[:, rows] - slp[:, rows]).abs().max().item()
        print("sample re-fed %d tokens: max log-probability gap %.2e" % (p, gap))
        assert gap < 1e-5                               # fp32 log-probabilities of magnitude < 16: a few ulp


def test_scores_are_score_tokens_of_the_returned_captions():
    dec, cfg, P, ents, facts, enc, prefix = e2e("geo", 1000, 3)
    beam = 3
    _, score, allseq, allscore = dec.predict_beam(*args_of(enc, PC.E2E_LEN, ents, facts), beam_size=beam, return_all=True,
                                                  prefix=prefix, length_penalty=0.6)
    used = (allscore > NINF).reshape(-1)
    assert used.view(PC.E2E_B, beam).sum(dim=1).tolist() == [beam, beam, 1]
    sb = dec.score_tokens(allseq.reshape(-1, PC.E2E_LEN).t().contiguous(), enc.cuda(), ents, None, samples_per_image=beam)
    gap = (sb.log_prob - allscore.reshape(-1))[used].abs().max().item()
    print("score_tokens vs prefixed beam scores: max gap %.2e" % gap)
    assert gap < 2e-3                                   # test_score_captions_gpu.py's bound for predict_beam scores
    assert torch.isin(score, allscore).all()


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_whole_caption_prefix_gives_the_attention_maps_of_that_caption(variant):
    dec, cfg, P, ents, facts, enc, prefix = e2e(variant, 50, 3)
    toks = torch.tensor([prefix[2][b:] + prefix[2][:b] for b in range(PC.E2E_B)])       # a given caption per image
    args = args_of(enc, PC.E2E_LEN, ents, facts)
    seq, attn = dec.predict_beam(*args, beam_size=1, prefix=toks, return_attention=True)
    assert torch.equal(seq.t().cpu(), toks)
    fed, live = prefix_feeds(toks, cfg.start, cfg.end)
    fp64 = Fp64Decode(cfg, P, enc, ents, facts)
    want = cross_weights(fp64, fed, torch.arange(PC.E2E_B))
    worst = check_weights("beam prefix " + variant, attn.cpu(), want, live)
    s2, a2 = dec.predict_sample(*args, num_samples=1, seed=1, prefix=toks, return_attention=True)
    assert torch.equal(s2.t().cpu(), toks)
    print("whole-caption attention: max |weight - fp64| %.2e (beam), %.2e (sample)"
          % (worst, check_weights("sample prefix " + variant, a2.cpu(), want, live)))


@pytest.mark.parametrize("variant,rules", [("geo", False), ("knowledge", True)])
def test_none_captures_nothing_new_and_an_empty_table_is_the_same_bits(variant, rules):
    dec, cfg, P, ents, facts, enc, prefix = e2e(variant, 200, 2)
    kw = PC.RULES if rules else {}
    skw = {k: v for k, v in kw.items() if k != "length_penalty"}
    args = args_of(enc, PC.E2E_LEN, ents, facts)
    calls = [lambda **x: dec.predict_beam(*args, beam_size=4, return_all=True, return_attention=True, **kw, **x),
             lambda **x: dec.predict_beam(*args, beam_size=4, return_all=True, num_beam_groups=2, diversity_penalty=0.5, **kw, **x),
             lambda **x: dec.predict_beam(*args, beam_size=3, return_all=True, column_bias={7: 0.5, 9: NINF}, **kw, **x),
             lambda **x: dec.predict_sample(*args, num_samples=3, top_p=0.9, top_k=20, seed=5, return_log_probs=True, **skw, **x)]
    want = [[t.clone() for t in c()] for c in calls]
    n, before = graphs(dec), kinds(dec)
    for c, w in zip(calls, want):
        for x, y in zip(c(prefix=None), w):
            assert torch.equal(x, y)
    assert graphs(dec) == n and kinds(dec) == before and not any("prefix" in k for k in before)
    empty = [[[-1] * 3] * PC.E2E_B, [-1], torch.full((PC.E2E_B, PC.E2E_LEN), -1)]
    for c, w in zip(calls, want):
        for e in empty:
            for x, y in zip(c(prefix=e), w):
                assert torch.equal(x, y)
    assert graphs(dec) == n + 4 and len([k for k in kinds(dec) if "prefix" in k]) == 4
    # a caption whose row is all -1 beside prefixed ones gets its own search, bit for bit
    got = calls[0](prefix=prefix)
    assert torch.equal(got[0][:, 0], want[0][0][:, 0]) and torch.equal(got[3][0], want[0][3][0])


def test_new_ids_and_lengths_replay_without_a_capture():
    dec, cfg, P, ents, facts, enc, prefix = e2e("geo", 60, 2)
    args = args_of(enc, PC.E2E_LEN, ents, facts)
    p1, p2 = prefix, [[9, 10, 11], [-1, -1, -1], [5, -1, -1]]

    def beam_(p, **kw):
        return [x.clone() for x in dec.predict_beam(*args, beam_size=3, return_all=True, prefix=p, **kw)]

    def samp(p):
        return [x.clone() for x in dec.predict_sample(*args, num_samples=2, seed=3, return_log_probs=True, prefix=p)]

    a1, s1 = beam_(p1), samp(p1)
    n = graphs(dec)
    b1, t1 = beam_(p2), samp(p2)
    a2, s2 = beam_(p1), samp(p1)
    assert graphs(dec) == n
    for x, y in zip(a1 + s1, a2 + s2):
        assert torch.equal(x, y)
    assert b1[0][:3, 0].tolist() == [9, 10, 11] and t1[0][0, 4:].tolist() == [5, 5]
    dec.use_hip_graphs = False                           # the replays computed the new tables
    for want, got in ((a1, beam_(p1)), (b1, beam_(p2)), (s1, samp(p1)), (t1, samp(p2))):
        for x, y in zip(want, got):
            assert torch.equal(x, y)


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_a_captions_result_does_not_depend_on_its_neighbours_prefixes(variant):
    dec, cfg, P, ents, facts, enc, prefix = e2e(variant, 80, 4)
    kw = dict(no_repeat_ngram_size=2, length_penalty=0.6)
    full = [x.clone() for x in dec.predict_beam(*args_of(enc, PC.E2E_LEN, ents, facts), beam_size=4, return_all=True,
                                                prefix=prefix, **kw)]
    sfull = dec.predict_sample(*args_of(enc, PC.E2E_LEN, ents, facts), num_samples=2, seed=8, top_k=10, prefix=prefix).clone()
    other = [prefix[1], prefix[2], prefix[0]]
    for b in range(PC.E2E_B):
        mixed = [prefix[q] if q == b else other[q] for q in range(PC.E2E_B)]
        got = dec.predict_beam(*args_of(enc, PC.E2E_LEN, ents, facts), beam_size=4, return_all=True, prefix=mixed, **kw)
        assert torch.equal(full[0][:, b], got[0][:, b])
        for x, y in zip(full[1:], got[1:]):
            assert torch.equal(x[b], y[b])
        single = dec.predict_beam(*args_of(enc[b:b + 1], PC.E2E_LEN, ents[b:b + 1], one(facts, b)), beam_size=4,
                                  return_all=True, prefix=[prefix[b]], **kw)
        assert torch.equal(full[0][:, b:b + 1], single[0]) and torch.equal(full[3][b:b + 1], single[3])
        sgot = dec.predict_sample(*args_of(enc, PC.E2E_LEN, ents, facts), num_samples=2, seed=8, top_k=10, prefix=mixed)
        assert torch.equal(sfull[:, 2 * b:2 * b + 2], sgot[:, 2 * b:2 * b + 2])


def test_refused_combinations_and_beam_1():
    dec, cfg, P, ents, facts, enc, prefix = e2e("geo", 50, 2)
    args = args_of(enc, PC.E2E_LEN, ents, facts)
    for kw in (dict(prefix=prefix, force_tokens=[[5]] * PC.E2E_B), dict(prefix=[5], column_bias={5: NINF}),
               dict(prefix=["<end>"]), dict(prefix=[[5, -1, 6]] * PC.E2E_B), dict(prefix=[50 + PC.E2E_K])):
        with pytest.raises(IckError):
            dec.predict_beam(*args, beam_size=3, **kw)
    with pytest.raises(TypeError):
        dec.predict(*args, prefix=prefix)
    out = dec.predict_beam(*args, beam_size=1, prefix=prefix, return_all=True)           # beam 1: the beam kernels
    assert out[2].shape == (PC.E2E_B, 1, PC.E2E_LEN) and "beam_prefix" in kinds(dec)
    assert out[0][:, 2].tolist() == prefix[2]
    groups = dec.predict_beam(*args, beam_size=4, num_beam_groups=2, diversity_penalty=0.5, return_groups=True, prefix=prefix)
    assert groups.shape == (PC.E2E_LEN, PC.E2E_B * 2) and groups[:2, 2].tolist() == groups[:2, 3].tolist() == prefix[1][:2]


def test_evaluate_writes_captions_that_begin_with_the_prefix(tmp_path):
    from ick_amd import eval as ev
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    from test_forward_gpu import build_decoder
    data_dir = str(tmp_path / "data")
    V, max_len = 60, 10
    wm = synth.write_dataset(data_dir, "toy", "geo", n_train=4, n_val=2, n_test=5, L=12, K=6, V=V, F=5)
    dec = build_decoder("geo", V, synth.make_params("geo", V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=2, shuffle=False)
    seen = []

    def per_batch(bi, batch):
        seen.append(bi)
        return [7 + bi, V + 1]

    for value, first in (([9, V + 2], lambda i: [9, V + 2]), (per_batch, lambda i: [7 + i // 2, V + 1])):
        _, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=str(tmp_path / "b.csv"),
                              beam=dict(beam_size=3, prefix=value))
        assert len(seqs) == 5 and all(list(s[:2]) == first(i) for i, s in enumerate(seqs))
        _, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=str(tmp_path / "s.csv"),
                              sample=dict(num_samples=2, seed=1, prefix=value))
        assert len(seqs) == 10 and all(list(s[:2]) == first(i // 2) for i, s in enumerate(seqs))
    assert seen == [0, 1, 2, 0, 1, 2]
