"""The column bias on the device.  Kernel level: every case of tests/column_bias_cases.py through
ick_decode_select_beam_biased / ick_decode_select_sample_biased on the hand-filled context of
tests/test_select_envelope_gpu.py, against the step references of tests/column_bias_ref.py -- integers exactly, cum and
log_prob at that test's 1e-4, bsum exactly (the table's biases are multiples of 1/8) -- and empty or zero lists bit for bit
against the rules entries.  End to end: predict_beam / predict_sample(column_bias=) on the small geo and knowledge models
against the CPU beam search and the numpy restatement of every sampled token."""
import ctypes

import numpy as np
import pytest
import torch

import ick_amd.decoder as D
import ick_amd.lib as L
import ick_amd.ops as ops
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
import column_bias_cases as CB
import column_bias_ref as ref
import select_cases as SC
import test_select_envelope_gpu as E
from sample_ref import gumbel
from test_sample_gpu import MARGIN, BOUNDARY, make_case, teacher_forced_scores, upto_end

pytestmark = pytest.mark.gpu

TOL = 1e-4                      # cum and log_prob against float64: test_select_envelope_gpu.py's, on the same quantities
NINF = float("-inf")
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ kernel level
def padded(case, cols, vals):
    """(B, 64) slots as the entry points read them; the value of an empty slot is NaN: it must not be looked at."""
    c = np.full((case.B, 64), -1, np.int32)
    v = np.full((case.B, 64), NAN, np.float32)
    for b in range(case.B):
        c[b, :len(cols[b])] = cols[b]
        v[b, :len(vals[b])] = vals[b]
    v[c < 0] = NAN
    return c, v


class BiasBeamHarness(E.BeamHarness):
    def __init__(self, case, st, cols=None, vals=None):
        super().__init__(case, st)
        c, v = padded(case, case.bias_cols if cols is None else cols, case.bias_vals if vals is None else vals)
        self.add("bcols", case.B, (64,), torch.int32, c)
        self.add("bvals", case.B, (64,), torch.float32, v)
        self.add("bsum", case.R, (), torch.float32, st["bsum"].astype(np.float32))
        self.bias = L.DecodeBias()
        self.bias.cols, self.bias.vals = self.bufs["bcols"].ptr(), self.bufs["bvals"].ptr()
        self.bias.sum = self.bufs["bsum"].ptr()

    def select(self, pos):
        ops.decode_select_beam(self.ctx, self.bs, pos, self.rules, bias=self.bias)
        torch.cuda.synchronize()


class BiasSampleHarness(E.SampleHarness):
    def __init__(self, case, st, cols=None, vals=None):
        super().__init__(case, st)
        c, v = padded(case, case.bias_cols if cols is None else cols, case.bias_vals if vals is None else vals)
        self.add("bcols", case.B, (64,), torch.int32, c)
        self.add("bvals", case.B, (64,), torch.float32, v)
        self.bias = L.DecodeBias()
        self.bias.cols, self.bias.vals = self.bufs["bcols"].ptr(), self.bufs["bvals"].ptr()

    def select(self, pos):
        ops.decode_select_sample(self.ctx, self.state, pos, self.rules, bias=self.bias)
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", CB.BEAM, ids=lambda c: c.name)
def test_biased_beam_selection_matches_the_reference_step_by_step(case):
    trace = CB.beam_trace(case.name)
    h = BiasBeamHarness(case, trace[0]["st"])
    R_ = case.R
    cur = 0
    for t in trace:
        pos, out, info = t["pos"], t["out"], t["info"]
        what = (case.name, pos)
        nxt = h.point(cur)
        h.write_rows(t["rows"])
        h.bufs["rec"].t.fill_(NAN)
        h.poison_outputs()
        h.select(pos)
        b = h.bufs
        cum, fin, bsum = b["cum"].np().astype(np.float64), b["fin"].np(), b["bsum"].np().astype(np.float64)
        print(what, "cum", cum, "want", out["cum"], "bsum", bsum, "want", out["bsum"])
        dead = out["cum"] == SC.NEG
        assert np.array_equal(cum == SC.NEG, dead), what
        assert np.abs(cum[~dead] - out["cum"][~dead]).max(initial=0.0) < TOL, what
        assert np.array_equal(bsum, out["bsum"]), (what, bsum, out["bsum"])      # the exact sum of the emitted biases
        assert np.array_equal(fin, out["fin"]), what
        if case.rules is not None:
            assert np.array_equal(b["len"].np(), out["len"]), what
        assert int(b["n_done"].np()[0]) == out["n_done"], (what, int(b["n_done"].np()[0]), out["n_done"])
        keep = ~info["dead"]
        assert np.array_equal(h.seq[nxt].np()[keep], out["seq"][keep]), (what, h.seq[nxt].np(), out["seq"])
        assert np.array_equal(h.anc[nxt].np()[keep], out["anc"][keep]), (what, h.anc[nxt].np(), out["anc"])
        if h.cap:
            assert np.array_equal(h.cap[nxt].np()[keep], out["cap"][keep]), (what, h.cap[nxt].np(), out["cap"])
        h.check_next(info, np.ones(R_, bool), what)
        h.check_x0(info, info["x0_written"], what)
        h.check_guards(what)
        cur = nxt


@pytest.mark.parametrize("case", CB.SAMPLE, ids=lambda c: c.name)
def test_biased_sampled_selection_matches_the_reference_step_by_step(case):
    trace = CB.sample_trace(case.name)
    h = BiasSampleHarness(case, trace[0]["st"])
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
        assert np.abs(b["log_prob"].np().astype(np.float64) - out["log_prob"]).max() < TOL, what     # the raw scores'
        if "cap_buf" in b:
            assert np.array_equal(b["cap_buf"].np(), out["cap_buf"]), (what, b["cap_buf"].np(), out["cap_buf"])
        h.check_next(info, written, what)
        h.check_x0(info, written & (pos + 1 < case.max_len), what)
        h.check_guards(what)


def _beam_bits(h, trace):
    """Every step's outgoing state of a harness run over the rows of `trace`, as bytes."""
    got, cur = [], 0
    for t in trace:
        nxt = h.point(cur)
        h.write_rows(t["rows"])
        h.bufs["rec"].t.fill_(NAN)
        h.poison_outputs()
        h.select(t["pos"])
        names = ["cum", "fin", "x0", "next_token", "next_mask", "n_done"] + (["len"] if "len" in h.bufs else [])
        got.append([h.bufs[n].np().tobytes() for n in names] + [h.seq[nxt].np().tobytes(), h.anc[nxt].np().tobytes()] +
                   ([h.cap[nxt].np().tobytes()] if h.cap else []))
        cur = nxt
    return got


# the rules entry needs rules: the rule-free cases of the table get rules with every word zero, which the header promises
# to be the bits of the entry without rules
ZERO_BEAM = ["ties_1023", "tie_chunk_1025", "lp_order", "carry_next_to_live", "ngram_ban", "ban_chunk1_seam",
             "v65536_beam8", "script_plain", "script_rules", "beam1"]


@pytest.mark.parametrize("zero", ["empty", "zeros"])
@pytest.mark.parametrize("name", ZERO_BEAM)
def test_empty_and_zero_lists_are_the_rules_beam_bit_for_bit(name, zero):
    base = SC.BEAM_BY_NAME[name]
    trace = SC.beam_trace(name)
    st = dict(trace[0]["st"], bsum=np.zeros(base.R))
    if zero == "empty":
        cols, vals = [[-1] * 64] * base.B, [[0.0] * 64] * base.B
    else:       # 64 slots over the best columns of the first rows, the last column and <end>, +0.0 and -0.0 in turn
        first = np.argsort(-next(iter(trace[0]["rows"].values())))[:61].tolist()
        cs = list(dict.fromkeys(first + [base.Vx - 1, SC.END, 0]))[:64]
        cols, vals = [cs] * base.B, [[0.0 if q % 2 else -0.0 for q in range(len(cs))]] * base.B
    case = CB.BiasBeamCase(**base.__dict__, bias_cols=cols, bias_vals=vals)
    mine = _beam_bits(BiasBeamHarness(case, st), trace)
    plain = E.BeamHarness(base, trace[0]["st"])
    if base.rules is None:                              # every rule word zero
        plain.rules_t = D.rules_tensor(base.max_len, 0.0, 0, 0, "cuda")
        plain.add("len", base.R, (), torch.int32, 0)
        plain.rules = D._rules_struct(plain.rules_t, plain.bufs["len"].full)
    theirs = _beam_bits(plain, trace)
    if base.rules is None:
        theirs = [t[:6] + t[7:] for t in theirs]        # (the length buffer the zero rules needed)
    assert mine == theirs


ZERO_SAMPLE = ["topk_run_zero", "topp_run_kept", "topp_run_dropped", "both_65536", "temperature_philox", "ban_on_max",
               "rules_16385", "end_and_finished", "script_sample", "topk_1"]


@pytest.mark.parametrize("zero", ["empty", "zeros"])
@pytest.mark.parametrize("name", ZERO_SAMPLE)
def test_empty_and_zero_lists_are_the_rules_sampler_bit_for_bit(name, zero):
    base = SC.SAMPLE_BY_NAME[name]
    trace = SC.sample_trace(name)
    if zero == "empty":
        cols, vals = [[-1] * 64] * base.B, [[0.0] * 64] * base.B
    else:
        rows0 = next((t["rows"] for t in trace if t["rows"]), None)
        first = np.argsort(-next(iter(rows0.values())))[:61].tolist() if rows0 else [3]
        cs = list(dict.fromkeys(first + [base.Vx - 1, SC.END, 0]))[:64]
        cols, vals = [cs] * base.B, [[0.0 if q % 2 else -0.0 for q in range(len(cs))]] * base.B
    case = CB.BiasSampleCase(**base.__dict__, bias_cols=cols, bias_vals=vals)

    def run(h):
        got = []
        for t in trace:
            h.write_rows(t["rows"])
            h.poison_outputs()
            h.select(t["pos"])
            got.append([h.bufs[n].np().tobytes() for n in ("output", "finished", "log_prob", "n_done", "x0", "next_token",
                                                           "next_mask")])
        return got

    plain = E.SampleHarness(base, trace[0]["st"])
    if base.rules is None:
        plain.rules_t = D.rules_tensor(base.max_len, 0.0, 0, 0, "cuda")
        plain.rules = D._rules_struct(plain.rules_t)
    assert run(BiasSampleHarness(case, trace[0]["st"])) == run(plain)


def test_entry_points_refuse_bad_arguments_without_a_launch():
    case = CB.BEAM_BY_NAME["persistence"]
    st = CB.beam_state(case)
    h = BiasBeamHarness(case, st)
    h.point(0)
    h.write_rows(CB.beam_trace("persistence")[0]["rows"])
    h.poison_outputs()
    before = h.bufs["cum"].np().copy()
    for field in ("cols", "vals", "sum"):
        keep = getattr(h.bias, field)
        setattr(h.bias, field, None)
        E.refused(lambda: h.select(0))
        setattr(h.bias, field, keep)
    assert L.load().ick_decode_select_beam_biased(ctypes.byref(h.ctx), ctypes.byref(h.bs), None, None, 0, None) != 0
    assert np.array_equal(h.bufs["cum"].np(), before) and np.isnan(h.bufs["x0"].np()).all()       # nothing ran
    h.check_guards("beam")
    sc = CB.SAMPLE_BY_NAME["s_vx5_topk"]
    s = BiasSampleHarness(sc, SC.sample_state(sc))
    s.write_rows(CB.sample_trace("s_vx5_topk")[0]["rows"])
    s.poison_outputs()
    for field in ("cols", "vals"):
        keep = getattr(s.bias, field)
        setattr(s.bias, field, None)
        E.refused(lambda: s.select(0))
        setattr(s.bias, field, keep)
    assert np.isnan(s.bufs["x0"].np()).all() and (s.bufs["output"].np() == 0).all()
    s.bias.sum = None                                   # sampling has no sum
    s.select(0)
    assert not np.isnan(s.bufs["x0"].np()).any()
    with pytest.raises(IckError):                       # ops refuses the compositions that are out of scope
        ops.decode_select_beam(h.ctx, h.bs, 0, None, None, L.DecodeConstraints(), h.bias)


# ------------------------------------------------------------------------------------------------ end to end
def args_of(enc, max_len, ents, facts):
    return [enc.cuda(), max_len, ents] + ([facts.cuda()] if facts is not None else [])


def beam_all(dec, enc, max_len, ents, facts, beam, **kw):
    return [x.clone() for x in dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam, return_all=True, **kw)]


def one(x, b):
    return None if x is None else x[b:b + 1]


def graphs(dec):
    return len(dec.__dict__.get("_graphs", {}))


def vx_of(cfg, ents, facts):
    return cfg.vocab_size + ents.shape[1] + (facts.shape[1] if facts is not None else 0)


def lists_for(cfg, ents, facts, plain_best, B):
    """One list per caption: the first token of the caption's unbiased best banned, an entity pointer and (with facts)
    a fact pointer boosted, <end> held back; caption 1 also carries empty slots."""
    V, K = cfg.vocab_size, ents.shape[1]
    ids, vals = [], []
    for b in range(B):
        first = int(plain_best[0, b])
        row = [(first, NINF), (V + (b + 1) % K, 1.0), (cfg.end, -0.5)]
        if facts is not None:
            row.append((V + K + b % facts.shape[1], 0.75))
        if first == cfg.end:
            row = row[1:]
        row = [(c, v) for i, (c, v) in enumerate(row) if c not in [q[0] for q in row[:i]]]
        if b == 1:
            row = [(-1, 3.0)] + row
        ids.append([c for c, _ in row])
        vals.append([v for _, v in row])
    n = max(len(r) for r in ids)
    return ([r + [-1] * (n - len(r)) for r in ids], [r + [0.0] * (n - len(r)) for r in vals])


RULES = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)
# (variant, V, beam, rules)
REF_CASES = [("geo", 50, 1, False), ("geo", 50, 3, True), ("geo", 1000, 5, False), ("knowledge", 50, 5, True),
             ("knowledge", 1000, 3, False), ("knowledge", 1000, 1, True)]
# A decision of the float64 reference is the device's wherever its two candidates are further apart than the device's
# keys can be off: the suite holds a device score to 1e-3 of the oracle's (test_decode_rules_gpu.py), so two keys move
# against each other by at most 2e-3.
DECIDED = 2e-3


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "%s_V%d_b%d_%s" % (c[0], c[1], c[2], "rules" if c[3] else "plain"))
def test_beam_search_matches_the_cpu_reference_hypothesis_by_hypothesis(case):
    variant, V, beam, rules = case
    B, max_len = 2, 8
    kw = RULES if rules else {}
    compared = 0
    for seed in (3, 4, 5, 6):
        dec, cfg, P, ents, facts, enc = make_case(variant, B, 6, V, 5, seed)
        plain = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=max(beam, 2), **kw).cpu()
        ids, vals = lists_for(cfg, ents, facts, plain, B)
        seq, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, column_bias=(ids, vals), **kw)
        assert seq.shape == (max_len, B) and allseq.shape == (B, beam, max_len) and allscore.shape == (B, beam)
        Vx = vx_of(cfg, ents, facts)
        for b in range(B):
            what = (case, seed, b)
            bias = ref.bias_row(Vx, ids[b], vals[b])
            want = ref.predict_beam_bias(cfg, P, enc[b:b + 1], max_len, ents[b:b + 1], one(facts, b), beam, bias=bias, **kw)
            print(what, "reference margin %.3g" % want[4], "best", want[0].tolist(), "device", seq[:, b].tolist())
            banned = [c for c in range(Vx) if bias[c] == NINF]
            for h in range(beam):                           # a banned column occurs in no final hypothesis
                if allscore[b, h].item() > NINF:
                    assert not set(banned) & set(upto_end(allseq[b, h].tolist(), cfg.end)), (what, h)
            own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], one(facts, b), seq[:, b].cpu().tolist(), max_len)
            assert abs(score[b].item() - own) < 1e-3, (what, score[b].item(), own)         # the model's log-probability
            if want[4] < DECIDED:
                continue
            compared += 1
            assert seq[:, b].cpu().tolist() == want[0].tolist(), what
            assert abs(score[b].item() - want[1]) < 1e-3, what
            for h, (hs, hscore, _, _) in enumerate(want[3]):
                mine = upto_end(allseq[b, h].cpu().tolist(), cfg.end)
                assert mine[:len(hs)] == hs and abs(allscore[b, h].item() - hscore) < 1e-3, (what, h, mine, hs)
    assert compared >= 1, "no caption of this case is decided at %g: the comparison would be empty" % DECIDED


def test_scores_are_score_tokens_of_the_returned_captions():
    B, max_len, beam = 3, 8, 3
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 6, 300, 0, 9)
    bias = {cfg.vocab_size + 2: 1.5, "<unk>": NINF, "<end>": -0.75}
    _, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, column_bias=bias, length_penalty=0.6)
    assert torch.isfinite(allscore).all()
    sb = dec.score_tokens(allseq.reshape(-1, max_len).t().contiguous(), enc.cuda(), ents, None, samples_per_image=beam)
    gap = (sb.log_prob - allscore.reshape(-1)).abs().max().item()
    print("score_tokens vs biased beam scores: max gap %.2e" % gap)
    assert gap < 2e-3                                   # test_score_captions_gpu.py's bound for the same comparison
    assert torch.isin(score, allscore).all()


@pytest.mark.parametrize("variant,rules", [("geo", False), ("knowledge", True)])
def test_none_captures_nothing_new_and_zeros_are_the_same_bits(variant, rules):
    B, max_len = 3, 10
    dec, cfg, P, ents, facts, enc = make_case(variant, B, 6, 200, 5, 2)
    kw = RULES if rules else {}
    args = args_of(enc, max_len, ents, facts)
    want = [x.clone() for x in dec.predict_beam(*args, beam_size=4, return_all=True, return_attention=True, **kw)]
    swant = [x.clone() for x in dec.predict_sample(*args, num_samples=3, top_p=0.9, top_k=20, seed=5, return_log_probs=True,
                                                   **{k: v for k, v in kw.items() if k != "length_penalty"})]
    n = graphs(dec)
    again = dec.predict_beam(*args, beam_size=4, return_all=True, return_attention=True, column_bias=None, **kw)
    sagain = dec.predict_sample(*args, num_samples=3, top_p=0.9, top_k=20, seed=5, return_log_probs=True, column_bias=None,
                                **{k: v for k, v in kw.items() if k != "length_penalty"})
    assert graphs(dec) == n
    for x, y in zip(list(again) + list(sagain), want + swant):
        assert torch.equal(x, y)
    Vx = vx_of(cfg, ents, facts)
    zeros = [(list(range(64)), [0.0] * 64), ([[-1, -1]] * B, [[1.0, NINF]] * B), {Vx - 1: -0.0, "<end>": 0.0}]
    for z in zeros:
        got = dec.predict_beam(*args, beam_size=4, return_all=True, return_attention=True, column_bias=z, **kw)
        for x, y in zip(got, want):
            assert torch.equal(x, y)
        got = dec.predict_sample(*args, num_samples=3, top_p=0.9, top_k=20, seed=5, return_log_probs=True, column_bias=z,
                                 **{k: v for k, v in kw.items() if k != "length_penalty"})
        for x, y in zip(got, swant):
            assert torch.equal(x, y)
    kinds = {k[0] for k in dec.__dict__["_graphs"]}
    suffix = "_rules" if rules else ""
    assert "beam_bias%s_attn" % suffix in kinds and "sample_bias%s" % suffix in kinds
    assert graphs(dec) == n + 2                         # one capture each, replayed for every later list


def test_new_values_ids_and_c_replay_without_a_capture():
    B, max_len, beam = 3, 10, 3
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 6, 60, 0, 2)
    args = args_of(enc, max_len, ents, facts)
    V = cfg.vocab_size
    f1 = {V + 1: 2.0, 7: NINF}
    f2 = ([[9, 11, V + 3, -1]] * B, [[NINF, -1.0, 1.5, 0.0]] * B)                         # new ids, new values, another C

    def beam_(f, **kw):
        return beam_all(dec, enc, max_len, ents, facts, beam, column_bias=f, **kw)

    def samp(f):
        return [x.clone() for x in dec.predict_sample(*args, num_samples=2, seed=3, return_log_probs=True, column_bias=f)]

    a1, s1 = beam_(f1), samp(f1)
    n = graphs(dec)
    b1, t1 = beam_(f2), samp(f2)
    a2, s2 = beam_(f1), samp(f1)
    assert graphs(dec) == n
    r1 = beam_(f2, **RULES)
    assert graphs(dec) == n + 1                          # one capture more: the rules graph
    for x, y in zip(a1 + s1, a2 + s2):
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(a1, b1))
    dec.use_hip_graphs = False                           # the replays computed the new lists
    for want, got in ((a1, beam_(f1)), (b1, beam_(f2)), (r1, beam_(f2, **RULES)), (s1, samp(f1)), (t1, samp(f2))):
        for x, y in zip(want, got):
            assert torch.equal(x, y)


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_batch_is_independent(variant):
    B, max_len, beam = 3, 10, 4
    dec, cfg, P, ents, facts, enc = make_case(variant, B, 6, 80, 5, 4)
    plain = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam).cpu()
    ids, vals = lists_for(cfg, ents, facts, plain, B)
    kw = dict(no_repeat_ngram_size=2, length_penalty=0.6)
    full = beam_all(dec, enc, max_len, ents, facts, beam, column_bias=(ids, vals), **kw)
    sfull = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=2, seed=8, top_k=10, column_bias=(ids, vals)).clone()
    for b in range(B):
        single = beam_all(dec, enc[b:b + 1], max_len, ents[b:b + 1], one(facts, b), beam, column_bias=([ids[b]], [vals[b]]), **kw)
        assert torch.equal(full[0][:, b:b + 1], single[0])
        for x, y in zip(full[1:], single[1:]):
            assert torch.equal(x[b:b + 1], y)
    # a sampled row's noise is keyed by its caption index: caption 0 alone is caption 0 of the batch
    s0 = dec.predict_sample(*args_of(enc[:1], max_len, ents[:1], one(facts, 0)), num_samples=2, seed=8, top_k=10,
                            column_bias=([ids[0]], [vals[0]]))
    assert torch.equal(sfull[:, :2], s0)


KNOBS = [(1.0, 0, 1.0), (0.8, 4, 1.0), (1.2, 0, 0.85), (1.0, 6, 0.9)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "T%g_k%d_p%g" % k)
@pytest.mark.parametrize("variant,rules", [("geo", False), ("knowledge", True)])
def test_sampled_tokens_restated_on_s_plus_b(variant, rules, knobs):
    B, K, V, Fn, ns, max_len, seed = 2, 6, 50, 5, 3, 10, 7
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 3, end_bias=-1.0)
    T, k, p = knobs
    n, m = (2, 3) if rules else (0, 0)
    plain = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=1, top_k=1).cpu()
    ids, vals = lists_for(cfg, ents, facts, plain, B)
    seqs, lps = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=ns, temperature=T, top_k=k, top_p=p,
                                   seed=seed, return_log_probs=True, no_repeat_ngram_size=n, min_len=m,
                                   column_bias=(ids, vals))
    seqs, lps = seqs.cpu(), lps.cpu()
    Vx = vx_of(cfg, ents, facts)
    excused, moved = [], 0
    for r in range(B * ns):
        b, j = r // ns, r % ns
        bias = ref.bias_row(Vx, ids[b], vals[b])
        toks = upto_end(seqs[:, r].tolist(), cfg.end)
        sc = teacher_forced_scores(cfg, P, enc[b:b + 1], ents[b:b + 1], one(facts, b), toks, max_len)
        for i, t in enumerate(toks):
            s = sc[i].astype(np.float32)
            ban = ref.banned_set(toks, i, n, m, cfg.end) if rules else set()
            g = gumbel(seed, b, j, i, s.size)
            want, keep, top, ratio, cols = ref.draw(s, bias, T, k, p, g, ban)
            moved += want != ref.draw(s, np.zeros(Vx), T, k, p, g, ban)[0]
            assert t not in ban and bias[t] != NINF, (r, i, t)                  # a banned column is in no sampled row
            if t != want:
                margin = top[0] - top[1] if top.size > 1 else np.inf
                sp = (s + bias.astype(np.float32))[cols]
                kth = np.sort(sp)[::-1][k - 1] if 0 < k < sp.size else None
                ti, wi = int(np.searchsorted(cols, t)), int(np.searchsorted(cols, want))
                near_k = kth is not None and (abs(sp[ti] - kth) < MARGIN or abs(sp[wi] - kth) < MARGIN)
                near_p = p < 1 and (abs(ratio[ti]) < BOUNDARY or abs(ratio[wi]) < BOUNDARY)
                assert margin < MARGIN or near_k or near_p, (r, i, t, want, margin)
                excused.append((r, i))
            lsm = sc[i] - (sc[i].max() + np.log(np.exp(sc[i] - sc[i].max()).sum()))
            assert abs(lps[i, r].item() - lsm[t]) < 1e-4, (r, i, lps[i, r].item(), lsm[t])      # raw, untruncated
        Ln = len(toks)
        assert all(q == cfg.pad for q in seqs[Ln:, r].tolist()) and (lps[Ln:, r] == 0).all()
    assert moved > 0 and len(excused) <= 1, (moved, excused)


def test_return_attention_composes():
    B, max_len = 2, 8
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 6, 60, 5, 5)
    args = args_of(enc, max_len, ents, facts)
    bias = {cfg.vocab_size + 1: 1.0, 9: NINF}
    a = dec.predict_beam(*args, beam_size=3, return_all=True, column_bias=bias)
    a = [x.clone() for x in a]
    b = dec.predict_beam(*args, beam_size=3, return_all=True, return_attention=True, column_bias=bias)
    assert len(b) == 6 and b[4].shape[:2] == (max_len, B) and b[5].shape[:3] == (max_len, B, 3)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    s = dec.predict_sample(*args, num_samples=2, seed=4, column_bias=bias).clone()
    t, attn = dec.predict_sample(*args, num_samples=2, seed=4, column_bias=bias, return_attention=True)
    assert torch.equal(s, t) and attn.shape[:2] == (max_len, B * 2)


def test_refused_combinations_raise():
    dec, cfg, P, ents, facts, enc = make_case("geo", 1, 6, 50, 0, 2)
    args = args_of(enc, 8, ents, facts)
    with pytest.raises(IckError):
        dec.predict_beam(*args, beam_size=4, column_bias={3: 1.0}, num_beam_groups=2, diversity_penalty=0.5)
    with pytest.raises(IckError):
        dec.predict_beam(*args, beam_size=4, column_bias={3: 1.0}, force_tokens=[[5]])
    with pytest.raises(IckError):
        dec.predict_sample(*args, column_bias={3: float("inf")})
    out = dec.predict_beam(*args, beam_size=1, column_bias={3: 1.0}, return_all=True)       # beam 1: the beam kernels
    assert isinstance(out, tuple) and out[2].shape == (1, 1, 8)
    assert "beam_bias" in {k[0] for k in dec.__dict__["_graphs"]}


def test_evaluate_writes_captions_without_the_banned_word(tmp_path):
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
    _, plain = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=str(tmp_path / "p.csv"),
                           beam=dict(beam_size=3))
    counts = np.bincount([t for s in plain for t in s if t not in (wm["<end>"], wm["<pad>"])], minlength=V + 6)
    word = int(np.argmax(counts))
    assert counts[word] > 0
    seen = []

    def per_batch(bi, batch):
        seen.append(bi)
        return {word: NINF}

    for bias in ({word: NINF}, per_batch):
        _, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=str(tmp_path / "b.csv"),
                              beam=dict(beam_size=3, column_bias=bias))
        assert len(seqs) == 5 and not any(word in s for s in seqs)
        _, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=str(tmp_path / "s.csv"),
                              sample=dict(num_samples=2, seed=1, column_bias=bias))
        assert len(seqs) == 10 and not any(word in s for s in seqs)
    assert seen == [0, 1, 2, 0, 1, 2]


def test_cfg5_sizes_with_unk_banned_and_pointers_boosted():
    """cfg5: 32 captions x beam 5, V 10 000, 21 slots: <unk> banned and the 20 entity pointers at +1."""
    B, V, K, max_len, beam = 32, 10000, 20, 20, 5
    dec, cfg, P, ents, facts, enc = make_case("geo", B, K, V, 0, 6)
    bias = {"<unk>": NINF}
    bias.update({V + k: 1.0 for k in range(K)})
    plain = beam_all(dec, enc, max_len, ents, facts, beam)
    seq, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, column_bias=bias)
    unk = dec.word_map["<unk>"]
    assert seq.shape == (max_len, B) and not (allseq[allscore > NINF] == unk).any()
    ptr = lambda x: int(((x >= V) & (x < V + K)).sum())
    print("cfg5: pointer tokens in the best captions: %d plain, %d boosted" % (ptr(plain[0]), ptr(seq)))
    for b in (0, 17, 31):
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], None, seq[:, b].cpu().tolist(), max_len)
        assert abs(score[b].item() - own) < 1e-3
    rows = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=5, seed=2, top_p=0.9, column_bias=bias)
    assert rows.shape == (max_len, B * 5) and not (rows == unk).any()


def test_vocab_50k_beam_8():
    B, V, max_len = 2, 50000, 8
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 30, V, 40, 9)
    plain = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=8).cpu()
    ban = sorted({int(t) for t in plain[0].tolist()} - {cfg.end, cfg.pad})
    bias = {c: NINF for c in ban}
    bias.update({V + 29: 1.0, V + 30 + 39: 1.0, 49999: -0.5})
    seq, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, 8, column_bias=bias, length_penalty=0.6)
    for b in range(B):
        for h in range(8):
            if allscore[b, h].item() > NINF:
                assert not set(ban) & set(allseq[b, h].tolist())
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], facts[b:b + 1], seq[:, b].cpu().tolist(), max_len)
        assert abs(score[b].item() - own) < 1e-3
    rows = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=4, seed=1, top_p=0.95, column_bias=bias)
    assert not torch.isin(rows.cpu(), torch.tensor(ban)).any()
