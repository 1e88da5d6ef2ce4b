"""The fused decode kernels (csrc/decode.hip) across their supported envelope, against the float64 oracle
(tests/decode_ref.py): every case of tests/decode_cases.py, every row, every step up to <end>.

Greedy cases drive the production sequence of predict() (selection fused into the next step's first launch) and keep
each step's raw scores; beam and sample cases check every hypothesis / every log-probability.  Bars: raw scores within
2e-4 of fp64, summed beam scores within 1e-3, sampled log-probabilities within 1e-4; a token may differ from the
oracle's only where the fp64 margin is < 1e-4, at most once per case."""
import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.ops as ops
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
from decode_cases import BY_NAME, CASES, Case, shape_params
from decode_ref import Fp64Decode, float64_default, greedy_choices, log_softmax, params64, upto_end
from sample_ref import kept_set

pytestmark = pytest.mark.gpu

TOL, SEQ_TOL, LP_TOL, MARGIN, BOUNDARY = 2e-4, 1e-3, 1e-4, 1e-4, 1e-5


def build(case):
    P = shape_params(case, synth.make_params(case.variant, case.V, case.seed, d=case.d, decoder_dim=case.FF,
                                             num_layers=case.layers))
    wm = synth.make_word_map(case.V)
    m = ick_amd.load_models(case.variant)
    dec = m.DecoderTransformer(word_map=wm, emb_dim=case.d, decoder_dim=case.FF, encoder_dim=512, num_heads=case.H,
                               num_layers=case.layers)
    missing, unexpected = dec.load_state_dict(P, strict=False)
    assert missing == ["pos_encoder.pe"] and not unexpected
    dec = dec.cuda().eval()
    cfg = R.config_from_word_map(case.variant, wm, emb_dim=case.d, num_heads=case.H, num_layers=case.layers)
    ents = synth.make_entities(case.variant, case.B, case.K, case.V, case.seed)
    facts = synth.make_facts(case.variant, case.B, case.F, case.K, case.seed) if case.variant != "geo" else None
    enc = synth.make_enc_out(case.B, case.seed, emb_dim=case.d)
    return dec, cfg, P, ents, facts, enc


def check_plan(case):
    got = ops.decode_plan(case.R, case.rps, case.d, case.H, case.FF)
    assert {k: got[k] for k in case.plan} == case.plan, (case.name, got)
    assert ops.decode_supported(case.d, case.H, case.FF, case.S, case.max_len)


def args_of(enc, ents, facts):
    return [enc.cuda(), ents] + ([facts.cuda()] if facts is not None else [])


# ------------------------------------------------------------------------------------------------ greedy
def greedy_production(dec, enc, ents, facts, max_len, fuse=True):
    """predict()'s launch sequence, recording what each row was fed and each step's raw scores.  fuse: the selection of
    step i - 1 inside the first launch of step i (production); otherwise ick_decode_select_greedy after every step."""
    enc_out, ents, facts = dec._prepare_inputs(enc.cuda(), ents, None if facts is None else facts.cuda())
    enc_tok = dec._image_input(enc_out)[0].contiguous()
    K, V = ents.shape[1], dec.vocab_size
    ee, fe, kv, _, side = dec._encode_context(enc_tok, ents.contiguous(), facts, None)
    side.join()
    c, t = dec._decode_ctx(kv, ee, fe, 1, max_len, kv.shape[3], want_scores=True, fuse_select=fuse)

    def indicators():
        ops.context_indicators(t["cap_buf"], facts, K, V, dec._pred_wt(), dec.fc_predicate.bias.detach(), mode=1,
                               eib=t["eib"], gate=t["gate"])

    fed = [torch.full((c.R,), dec.word_map["<start>"], dtype=torch.long, device="cuda")]
    rows = []
    for i in range(max_len):
        if fuse and i > 0:
            ops.decode_layers_part(c, i, 1)       # selection of step i - 1 + first self-attention block
            fed.append(t["next_token"].clone())
            if dec.has_facts:
                indicators()
            ops.decode_layers_part(c, i, 2)
        else:
            if dec.has_facts:
                indicators()
            ops.decode_layers(c, i)
        rows.append(torch.cat([t["scores"], t["ptr"]], dim=1).clone())
        if not fuse:
            ops.decode_select_greedy(c, i)
            if i + 1 < max_len:
                fed.append(t["next_token"].clone())
    if fuse:
        ops.decode_select_greedy(c, max_len - 1)
    torch.cuda.synchronize()
    assert int(t["n_done"].item()) == int(t["finished"].sum().item())
    return (t["output"].cpu(), torch.stack(fed, dim=1).cpu(), torch.stack(rows, dim=1).cpu().double().numpy())


def check_greedy_rows(case, cfg, out, fed, ref, got=None):
    """Every row and step up to <end>: raw scores (if `got`) within TOL of fp64, each decision == the oracle's (excused
    only at an fp64 margin < MARGIN, once per case), and the final output (after the n-gram clean-up) == the oracle's."""
    end = cfg.end
    worst, excused = 0.0, []
    for r in range(out.shape[0]):
        choice, ref_out, margins = greedy_choices(cfg, ref[r], case.max_len)
        kern = out[r].tolist()
        for i, want in enumerate(choice):
            if got is not None:
                worst = max(worst, float(np.abs(got[r, i] - ref[r, i]).max()))
            have = kern[i] if want == end or i + 1 == case.max_len else int(fed[r, i + 1])
            if have != want:
                assert margins[i] < MARGIN, (case.name, r, i, have, want, margins[i])
                excused.append((r, i, have, want, float(margins[i])))
                break                       # the histories part here: the rest of the row is not comparable
        else:
            assert kern == ref_out, (case.name, r, kern, ref_out)
    assert worst < TOL, (case.name, "max |score - fp64|", worst)
    assert len(excused) <= 1, (case.name, excused)
    return worst, excused


def run_greedy(case):
    check_plan(case)
    dec, cfg, P, ents, facts, enc = build(case)
    out, fed, got = greedy_production(dec, enc, ents, facts, case.max_len)
    pred = dec.predict(*args_of(enc, ents, facts)[:1], case.max_len, *args_of(enc, ents, facts)[1:])
    again = dec.predict(*args_of(enc, ents, facts)[:1], case.max_len, *args_of(enc, ents, facts)[1:])   # graph replay
    assert torch.equal(pred, again), case.name
    assert torch.equal(pred.t().cpu(), out), case.name               # predict() == the sequence driven here
    out2, fed2, got2 = greedy_production(dec, enc, ents, facts, case.max_len)
    assert torch.equal(out2, out) and torch.equal(fed2, fed) and np.array_equal(got2, got), case.name
    if case.end_bias > 0:           # the raised last word (<end>) is chosen somewhere: the vocabulary's edge is selected
        assert (out == case.V - 1).any(), case.name
    fp64 = Fp64Decode(cfg, P, enc, ents, facts)
    ref = fp64.scores(fed, torch.arange(case.B), case.max_len)
    worst, excused = check_greedy_rows(case, cfg, out, fed, ref, got)
    print("%s: plan %s, max |score - fp64| %.2e, excused %s" % (case.name, case.plan, worst, excused))
    # the same decode with the stand-alone selection kernel after every step (dec_select_kernel at every position,
    # dec_self_kernel<G, false> at steps >= 1)
    out_u, fed_u, got_u = greedy_production(dec, enc, ents, facts, case.max_len, fuse=False)
    ref_u = ref if torch.equal(fed_u, fed) else fp64.scores(fed_u, torch.arange(case.B), case.max_len)
    worst_u, excused_u = check_greedy_rows(case, cfg, out_u, fed_u, ref_u, got_u)
    if case.end_bias > 0:
        assert (out_u == case.V - 1).any(), case.name
    print("%s unfused: max |score - fp64| %.2e, excused %s" % (case.name, worst_u, excused_u))


GREEDY = [c.name for c in CASES if c.kind == "greedy"]


@pytest.mark.parametrize("name", GREEDY)
def test_greedy_envelope(name):
    run_greedy(BY_NAME[name])


@pytest.mark.parametrize("name", ["greedy_b3", "greedy_b131"])
def test_greedy_envelope_gemm_split(name, gemm_split):
    run_greedy(BY_NAME[name])


# ------------------------------------------------------------------------------------------------ beam search
@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind == "beam"])
def test_beam_envelope(name):
    case = BY_NAME[name]
    check_plan(case)
    assert ops.decode_beam_supported(case.Vx, case.rps)
    dec, cfg, P, ents, facts, enc = build(case)
    a = args_of(enc, ents, facts)
    seq, score, allseq, allscore = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=case.rps, return_all=True)
    again = dec.predict_beam(a[0], case.max_len, *a[1:], beam_size=case.rps, return_all=True)          # graph replay
    for x, y in zip((seq, score, allseq, allscore), again):
        assert torch.equal(x, y), name
    allseq, allscore = allseq.cpu(), allscore.cpu()
    ref = Fp64Decode(cfg, P, enc, ents, facts)
    assert case.Vx >= case.rps and torch.isfinite(allscore).all(), (name, allscore)     # every slot holds a hypothesis
    hyps = [(b, j) for b in range(case.B) for j in range(case.rps)]
    lp = ref.sequence_logprobs([allseq[b, j].tolist() for b, j in hyps], [b for b, _ in hyps], case.max_len)
    err = max(abs(allscore[b, j].item() - v) for (b, j), v in zip(hyps, lp))
    assert err < SEQ_TOL, (name, "max |cumulative score - fp64|", err)
    # the best hypothesis against the fp64 beam search (ties: a different sequence must score as well under fp64)
    P64, flips = params64(P), []
    for b in range(case.B):
        with float64_default(), torch.no_grad():
            fb = None if facts is None else facts[b:b + 1]
            ref_seq, ref_score, _ = R.predict_beam(cfg, P64, enc[b:b + 1].double(), case.max_len, ents[b:b + 1], fb,
                                                   case.rps)
        mine = seq[:, b].cpu().tolist()
        if mine != ref_seq.tolist():
            own = ref.sequence_logprobs([mine], [b], case.max_len)[0]
            assert own > ref_score - SEQ_TOL, (name, b, mine, ref_seq.tolist(), own, ref_score)
            flips.append(b)
    assert len(flips) <= 1, (name, flips)
    print("%s: plan %s, max |cumulative - fp64| %.2e, flips %s" % (name, case.plan, err, flips))


# ------------------------------------------------------------------------------------------------ sampling
SAMPLE_KNOBS = (1.0, 8, 0.9)


@pytest.mark.parametrize("name", [c.name for c in CASES if c.kind == "sample"])
def test_sample_envelope(name):
    case = BY_NAME[name]
    check_plan(case)
    assert ops.decode_sample_supported(case.Vx, case.rps)
    dec, cfg, P, ents, facts, enc = build(case)
    T, k, p = SAMPLE_KNOBS
    a = args_of(enc, ents, facts)
    kw = dict(num_samples=case.rps, temperature=T, top_k=k, top_p=p, seed=11, return_log_probs=True)
    seqs, lps = dec.predict_sample(a[0], case.max_len, *a[1:], **kw)
    s2, l2 = dec.predict_sample(a[0], case.max_len, *a[1:], **kw)                                      # graph replay
    assert torch.equal(seqs, s2) and torch.equal(lps, l2), name
    seqs, lps = seqs.cpu(), lps.cpu()
    toks = [upto_end(seqs[:, r].tolist(), cfg.end) for r in range(case.R)]
    n = max(len(t) for t in toks)
    fed = torch.full((case.R, n), cfg.start, dtype=torch.long)
    for r, t in enumerate(toks):
        if len(t) > 1:
            fed[r, 1:len(t)] = torch.tensor(t[:-1])
    sc = Fp64Decode(cfg, P, enc, ents, facts).scores(fed, torch.arange(case.R) // case.rps)
    lsm = log_softmax(sc)
    worst, excused = 0.0, []
    for r, t in enumerate(toks):
        for i, q in enumerate(t):
            worst = max(worst, abs(lps[i, r].item() - lsm[r, i, q]))
            s = sc[r, i].astype(np.float32)
            keep, ratio = kept_set(s, T, k, p)
            if not keep[q]:
                kth = np.sort(s)[::-1][k - 1]
                assert abs(s[q] - kth) < MARGIN or abs(ratio[q]) < BOUNDARY, (name, r, i, q)
                excused.append((r, i, q))
        assert all(x == cfg.pad for x in seqs[len(t):, r].tolist()) and (lps[len(t):, r] == 0).all(), (name, r)
    assert worst < LP_TOL, (name, "max |log-prob - fp64|", worst)
    assert len(excused) <= 1, (name, excused)
    print("%s: plan %s, max |log-prob - fp64| %.2e, excused %s" % (name, case.plan, worst, excused))


# ------------------------------------------------------------------------------------------------ just outside
@pytest.mark.parametrize("K,max_len", [(829, 8), (20, 129)], ids=["S1025", "max_len129"])
def test_just_outside_the_envelope(K, max_len):
    """S = 1025 / max_len = 129: greedy still matches the fp64 oracle (through the per-op launches); beam search and
    sampling refuse before any capture."""
    case = Case("outside", "greedy", 2, K=K, max_len=max_len, V=300, end_bias=-30.0 if max_len > 100 else 0.0)
    assert not ops.decode_supported(case.d, case.H, case.FF, case.S, case.max_len)
    dec, cfg, P, ents, facts, enc = build(case)
    out = dec.predict(enc.cuda(), max_len, ents).t().cpu()
    assert torch.equal(dec.predict(enc.cuda(), max_len, ents).t().cpu(), out)
    # this path does not record what each row was fed, so the fp64 oracle decodes on its own and must reproduce the
    # output (a difference is excused only where one of its decisions had a margin < MARGIN)
    ref = Fp64Decode(cfg, P, enc, ents, facts)
    outs, excused = ref.greedy(torch.arange(case.B), max_len), []
    for r in range(case.B):
        if out[r].tolist() != outs[r][0]:
            assert outs[r][1] < MARGIN, (r, out[r].tolist(), outs[r][0], outs[r][1])
            excused.append(r)
    assert len(excused) <= 1, excused
    with pytest.raises(IckError):
        dec.predict_beam(enc.cuda(), max_len, ents, beam_size=3)
    with pytest.raises(IckError):
        dec.predict_sample(enc.cuda(), max_len, ents, num_samples=2, seed=1)


def test_vocabulary_limit_of_beam_and_sample():
    """Vx = 65536 is taken (beam8_vx65536, sample1_vx65536); Vx = 65537 refuses before any capture."""
    case = Case("vx65537", "beam", 1, rps=8, V=65517, K=20, max_len=4)
    assert not ops.decode_beam_supported(case.Vx, 8) and not ops.decode_sample_supported(case.Vx, 1)
    dec, cfg, P, ents, facts, enc = build(case)
    with pytest.raises(IckError):
        dec.predict_beam(enc.cuda(), case.max_len, ents, beam_size=8)
    with pytest.raises(IckError):
        dec.predict_sample(enc.cuda(), case.max_len, ents, num_samples=1, seed=1)
