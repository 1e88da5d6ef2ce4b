"""Decoding rules on the device: GNMT length penalty, no-repeat n-gram blocking and minimum length in
the beam selection kernels (csrc/decode_select.hip) and the sampled selection (csrc/sample.hip).  Beam search is held to the
rules beam search of tests/beam_rules_ref.py; sampling is restated token for token with the oracle's teacher-forced
scores, the bans, the kept set and the Philox-Gumbel draw (tests/sample_ref.py)."""
import numpy as np
import pytest
import torch

import ick_amd.synth as synth
from oracle import restatement as R
from beam_rules_ref import banned_set, has_banned_ngram, lp_table, predict_beam_rules
from sample_ref import draw, gumbel
from test_sample_gpu import MARGIN, make_case, teacher_forced_scores, upto_end

pytestmark = pytest.mark.gpu

DEFAULTS = dict(length_penalty=0.0, no_repeat_ngram_size=0, min_len=0)


def args_of(enc, max_len, ents, facts):
    return [enc.cuda(), max_len, ents] + ([facts.cuda()] if facts is not None else [])


def beam_all(dec, enc, max_len, ents, facts, beam, **kw):
    return dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam, return_all=True, **kw)


def one(x, b):
    return None if x is None else x[b:b + 1]


# ------------------------------------------------------------------------------------------------ 1. defaults
@pytest.mark.parametrize("beam", [3, 5])
def test_explicit_defaults_are_the_same_bits(beam):
    dec, cfg, P, ents, facts, enc = make_case("knowledge", 3, 6, 200, 5, 2)
    args = args_of(enc, 10, ents, facts)
    a = dec.predict_beam(*args, beam_size=beam, return_all=True, return_attention=True)
    b = dec.predict_beam(*args, beam_size=beam, return_all=True, return_attention=True, **DEFAULTS)
    assert len(a) == len(b) == 6
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    a = dec.predict_sample(*args, num_samples=3, top_p=0.9, seed=5, return_log_probs=True)
    b = dec.predict_sample(*args, num_samples=3, top_p=0.9, seed=5, return_log_probs=True, no_repeat_ngram_size=0,
                           min_len=0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(dec.predict_beam(*args, beam_size=1, **DEFAULTS), dec.predict(*args))


# ------------------------------------------------------------------------------------------------ 2. vs CPU reference
# (variant, V, beam, n, alpha, m)
REF_CASES = [
    ("geo", 50, 5, 1, 0.0, 0), ("geo", 50, 3, 2, 0.6, 3), ("geo", 1000, 5, 3, 1.0, 3), ("geo", 1000, 1, 2, 0.6, 0),
    ("geo", 1000, 3, 0, 0.6, 0), ("knowledge", 50, 3, 1, 1.0, 3), ("knowledge", 1000, 5, 2, 0.0, 3),
    ("knowledge", 1000, 3, 3, 0.6, 0), ("knowledge", 50, 1, 3, 0.0, 3), ("knowledge", 50, 5, 0, 1.0, 0),
]


def check_against_reference(dec, cfg, P, enc, ents, facts, max_len, beam, n, alpha, m, b, what):
    """Caption b of the batch against the rules beam reference; True when the sequences are identical."""
    kw = dict(length_penalty=alpha, no_repeat_ngram_size=n, min_len=m)
    return check_one(dec, cfg, P, enc, ents, facts, max_len, beam, kw, b, what, None)


def check_one(dec, cfg, P, enc, ents, facts, max_len, beam, kw, b, what, res):
    if res is None:
        res = beam_all(dec, enc, max_len, ents, facts, beam, **kw)
    seq, score, allseq, allscore = res
    eb, nb, fb = enc[b:b + 1], ents[b:b + 1], one(facts, b)
    ref_seq, ref_score, ref_key, _ = predict_beam_rules(cfg, P, eb, max_len, nb, fb, beam, **kw)
    lp = lp_table(kw["length_penalty"], max_len)
    mine = seq[:, b].cpu().tolist()
    toks = upto_end(mine, cfg.end)
    own = R.sequence_logprob(cfg, P, eb, nb, fb, mine, max_len)
    assert abs(score[b].item() - own) < 1e-3, (what, score[b].item(), own)             # its own score is right
    for h in range(beam):                                                                 # every hypothesis obeys
        hyp = allseq[b, h].cpu().tolist()
        if allscore[b, h].item() > float("-inf"):
            assert has_banned_ngram(upto_end(hyp, cfg.end), kw["no_repeat_ngram_size"], kw["min_len"],
                                    cfg.end) is None, (what, h, hyp)
    if mine == ref_seq.tolist():
        assert abs(score[b].item() - ref_score) < 1e-3, (what, score[b].item(), ref_score)
        return True
    my_key = own / lp[len(toks)].item()
    assert my_key > ref_key - 1e-3, (what, mine, ref_seq.tolist(), my_key, ref_key)
    return False


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "%s_V%d_b%d_n%d_a%g_m%d" % c)
def test_beam_rules_vs_cpu_reference(case):
    variant, V, beam, n, alpha, m = case
    seeds = (3, 4)
    exact = 0
    for seed in seeds:
        dec, cfg, P, ents, facts, enc = make_case(variant, 1, 6, V, 5, seed)
        exact += check_against_reference(dec, cfg, P, enc, ents, facts, 8, beam, n, alpha, m, 0, (case, seed))
    assert exact >= len(seeds) - 1


# ------------------------------------------------------------------------------------------------ 3. rules hold
def find_repeating_case(variant, V, n, decode):
    """The first seed whose decode WITHOUT rules breaks the n-gram rule somewhere (the test's teeth)."""
    for seed in range(1, 9):
        dec, cfg, P, ents, facts, enc = make_case(variant, 2, 6, V, 5, seed, end_bias=-2.0)
        rows = decode(dec, enc, ents, facts, {})
        if any(has_banned_ngram(r, n, 0, cfg.end) is not None for r in rows):
            return dec, cfg, ents, facts, enc
    raise AssertionError("no seed repeats an %d-gram without rules" % n)


@pytest.mark.parametrize("variant,n,m", [("geo", 2, 4), ("knowledge", 3, 5), ("geo", 1, 2)])
def test_beam_rules_hold_on_every_hypothesis(variant, n, m):
    max_len, beam = 14, 4

    def decode(dec, enc, ents, facts, kw):
        _, _, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, **kw)
        return [upto_end(allseq[b, h].cpu().tolist(), dec.word_map["<end>"])
                for b in range(allseq.shape[0]) for h in range(beam) if allscore[b, h].item() > float("-inf")]

    dec, cfg, ents, facts, enc = find_repeating_case(variant, 60, n, decode)
    rows = decode(dec, enc, ents, facts, dict(no_repeat_ngram_size=n, min_len=m, length_penalty=0.6))
    assert rows
    for r in rows:
        assert has_banned_ngram(r, n, m, cfg.end) is None, r


@pytest.mark.parametrize("variant,n,m", [("geo", 2, 4), ("knowledge", 1, 3)])
def test_sample_rules_hold_on_every_row(variant, n, m):
    max_len, ns = 14, 4

    def decode(dec, enc, ents, facts, kw):
        seqs = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=ns, top_k=5, seed=11, **kw)
        return [upto_end(seqs[:, r].cpu().tolist(), dec.word_map["<end>"]) for r in range(seqs.shape[1])]

    dec, cfg, ents, facts, enc = find_repeating_case(variant, 60, n, decode)
    rows = decode(dec, enc, ents, facts, dict(no_repeat_ngram_size=n, min_len=m))
    for r in rows:
        assert has_banned_ngram(r, n, m, cfg.end) is None, r


# ------------------------------------------------------------------------------------------------ 4. sampling restated
KNOBS = [(1.0, 0, 1.0), (0.8, 4, 1.0), (1.2, 0, 0.85), (1.0, 6, 0.9)]


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "T%g_k%d_p%g" % k)
@pytest.mark.parametrize("variant,n,m", [("geo", 1, 3), ("knowledge", 2, 4)])
def test_sample_rules_restated_exactly(variant, n, m, knobs):
    B, K, V, Fn, ns, max_len, seed = 2, 6, 50, 5, 3, 10, 7
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 3, end_bias=-1.0)
    T, k, p = knobs
    seqs, lps = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=ns, temperature=T, top_k=k,
                                   top_p=p, seed=seed, return_log_probs=True, no_repeat_ngram_size=n, min_len=m)
    seqs, lps = seqs.cpu(), lps.cpu()
    excused, fired = [], 0
    for r in range(B * ns):
        b, j = r // ns, r % ns
        toks = upto_end(seqs[:, r].tolist(), cfg.end)
        sc = teacher_forced_scores(cfg, P, enc[b:b + 1], ents[b:b + 1], one(facts, b), toks, max_len)
        for i, t in enumerate(toks):
            s = sc[i].astype(np.float32)
            ban = banned_set(toks, i, n, m, cfg.end)
            fired += bool(ban)
            allowed = np.array([c for c in range(s.size) if c not in ban])
            g = gumbel(seed, b, j, i, s.size)
            w, keep, vals, ratio = draw(s[allowed], T, k, p, g[allowed])
            want = int(allowed[w])
            assert t not in ban, (r, i, t, ban)
            if t != want:
                margin = vals[0] - vals[1] if vals.size > 1 else np.inf
                sa = np.sort(s[allowed])[::-1]
                kth = sa[k - 1] if 0 < k < sa.size else None
                ti, wi = int(np.searchsorted(allowed, t)), w
                near_k = kth is not None and (abs(s[t] - kth) < MARGIN or abs(s[want] - kth) < MARGIN)
                near_p = p < 1 and (abs(ratio[ti]) < 1e-5 or abs(ratio[wi]) < 1e-5)
                assert margin < MARGIN or near_k or near_p, (r, i, t, want, margin)
                excused.append((r, i))
            lsm = sc[i] - (sc[i].max() + np.log(np.exp(sc[i] - sc[i].max()).sum()))
            assert abs(lps[i, r].item() - lsm[t]) < 1e-4, (r, i, lps[i, r].item(), lsm[t])     # untruncated
        L = len(toks)
        assert all(q == cfg.pad for q in seqs[L:, r].tolist()) and (lps[L:, r] == 0).all()
    assert fired > 0 and len(excused) <= 1, (fired, excused)


def test_sample_without_a_firing_ban_is_the_same_draw():
    """min_len = 1 bans only <end> at step 0: where <end> would not have been drawn there, the samples are the bits
    of a call without rules (the noise of a column does not depend on the rules; no top-k / top-p, so the kept set is
    the allowed set)."""
    dec, cfg, P, ents, facts, enc = make_case("geo", 3, 6, 50, 0, 5, end_bias=-3.0)
    args = args_of(enc, 10, ents, facts)
    a = dec.predict_sample(*args, num_samples=4, seed=9, return_log_probs=True)
    b = dec.predict_sample(*args, num_samples=4, seed=9, return_log_probs=True, min_len=1)
    ok = a[0][0] != cfg.end
    assert ok.any()
    assert torch.equal(a[0][:, ok], b[0][:, ok]) and torch.equal(a[1][:, ok], b[1][:, ok])


# ------------------------------------------------------------------------------------------------ 5. replay, batching
def test_rules_change_replays_the_same_graph():
    dec, cfg, P, ents, facts, enc = make_case("geo", 3, 6, 60, 0, 2)
    args = args_of(enc, 12, ents, facts)
    A = dict(no_repeat_ngram_size=1, min_len=3, length_penalty=1.0)
    Bk = dict(no_repeat_ngram_size=2, min_len=0, length_penalty=0.3)

    def beam(**kw):         # the scores of return_all are the graph's own buffers: copies, before the next replay
        return [x.clone() for x in dec.predict_beam(*args, beam_size=3, return_all=True, **kw)]

    a1 = beam(**A)
    graphs = len(dec.__dict__["_graphs"])
    b1 = beam(**Bk)
    a2 = beam(**A)
    As = dict(no_repeat_ngram_size=1, min_len=3)
    s1 = dec.predict_sample(*args, num_samples=2, seed=3, **As)
    s2 = dec.predict_sample(*args, num_samples=2, seed=3, no_repeat_ngram_size=3)
    graphs2 = len(dec.__dict__["_graphs"])
    s3 = dec.predict_sample(*args, num_samples=2, seed=3, **As)
    assert len(dec.__dict__["_graphs"]) == graphs2 == graphs + 1          # one capture for the sampled rules graph
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    assert torch.equal(s1, s3)
    dec.use_hip_graphs = False                                            # the replays computed the new rules
    b0 = beam(**Bk)
    s0 = dec.predict_sample(*args, num_samples=2, seed=3, no_repeat_ngram_size=3)
    for x, y in zip(b0, b1):
        assert torch.equal(x, y)
    assert torch.equal(s0, s2)


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_beam_rules_batch_is_independent(variant):
    dec, cfg, P, ents, facts, enc = make_case(variant, 3, 6, 80, 5, 4)
    kw = dict(no_repeat_ngram_size=2, min_len=3, length_penalty=0.6)
    full = [x.clone() for x in beam_all(dec, enc, 10, ents, facts, 4, **kw)]
    for b in range(3):
        single = beam_all(dec, enc[b:b + 1], 10, ents[b:b + 1], one(facts, b), 4, **kw)
        assert torch.equal(full[0][:, b:b + 1], single[0])                   # best sequence (max_len, B)
        for x, y in zip(full[1:], single[1:]):                                # score, every hypothesis and its score
            assert torch.equal(x[b:b + 1], y)


# ------------------------------------------------------------------------------------------------ 6. envelope
def test_cfg5_sizes_with_rules():
    """cfg5: 32 captions x beam 5, V 10 000, max_len 20, every rule on; a few captions against the CPU reference."""
    B, V, max_len, beam = 32, 10000, 20, 5
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 20, V, 0, 6)
    kw = dict(no_repeat_ngram_size=3, length_penalty=0.6, min_len=5)
    res = beam_all(dec, enc, max_len, ents, facts, beam, **kw)
    assert res[0].shape == (max_len, B)
    exact = sum(check_one(dec, cfg, P, enc, ents, facts, max_len, beam, kw, b, ("cfg5", b), res) for b in (0, 17, 31))
    assert exact >= 2


def test_max_len_128_with_8_grams():
    B, V, max_len, beam = 2, 1000, 128, 3
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 6, V, 0, 8, end_bias=-4.0)
    kw = dict(no_repeat_ngram_size=8, min_len=100, length_penalty=1.0)
    seq, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, **kw)
    for b in range(B):
        for h in range(beam):
            hyp = upto_end(allseq[b, h].cpu().tolist(), cfg.end)
            assert len(hyp) >= 100 and has_banned_ngram(hyp, 8, 100, cfg.end) is None
    own = R.sequence_logprob(cfg, P, enc[:1], ents[:1], None, seq[:, 0].cpu().tolist(), max_len)
    assert abs(score[0].item() - own) < 2e-3
    rows = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=3, seed=2, top_k=3,
                              no_repeat_ngram_size=8, min_len=100)
    for r in range(rows.shape[1]):
        hyp = upto_end(rows[:, r].cpu().tolist(), cfg.end)
        assert has_banned_ngram(hyp, 8, 100, cfg.end) is None


def test_vocab_50k_beam_8():
    """V+K+F ~ 50 k (the wide chunk grid of the beam selection, the 16-group sampled selection) with beam 8."""
    B, V, max_len = 2, 50000, 8
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 30, V, 40, 9)
    kw = dict(no_repeat_ngram_size=1, length_penalty=0.6, min_len=4)
    seq, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, 8, **kw)
    for b in range(B):
        for h in range(8):
            if allscore[b, h].item() > float("-inf"):
                assert has_banned_ngram(upto_end(allseq[b, h].cpu().tolist(), cfg.end), 1, 4, cfg.end) is None
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], facts[b:b + 1], seq[:, b].cpu().tolist(), max_len)
        assert abs(score[b].item() - own) < 1e-3
    rows = dec.predict_sample(*args_of(enc, max_len, ents, facts), num_samples=4, seed=1, top_p=0.95,
                              no_repeat_ngram_size=1, min_len=4)
    for r in range(rows.shape[1]):
        assert has_banned_ngram(upto_end(rows[:, r].cpu().tolist(), cfg.end), 1, 4, cfg.end) is None


# ------------------------------------------------------------------------------------------------ 7. evaluation
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_evaluate_with_beam(tmp_path, variant):
    import pandas as pd
    from ick_amd import eval as ev
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    from test_forward_gpu import build_decoder
    data_dir = str(tmp_path / "data")
    V, max_len = 60, 10
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=2, n_test=5, L=12, K=6, V=V, F=5)
    dec = build_decoder(variant, V, synth.make_params(variant, V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=2, shuffle=False)
    beam = dict(beam_size=3, length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)
    out, npz = str(tmp_path / "beam.csv"), str(tmp_path / "beam_attn.npz")
    caps, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=out, beam=beam, attention_out=npz)
    df = pd.read_csv(out, keep_default_na=False)
    assert list(df.columns) == ["generated_caption"] and df["generated_caption"].tolist() == caps and len(caps) == 5
    dec.attach_encoder(enc)
    want, want_attn = [], []
    for batch in loader:
        extra = (batch[6].cuda(),) if len(batch) > 6 else ()
        x = batch[0].cuda()
        x = x if x.dim() == 4 and x.shape[1] == enc.encoder_dim else enc(x)
        s, a = dec.predict_beam(x, max_len, batch[4], *extra, return_attention=True, **beam)
        want += s.t().cpu().tolist()
        want_attn.append(a[:, :, -1].mean(dim=2).transpose(0, 1).to(torch.float16).cpu())
    assert seqs == want
    z = np.load(npz)
    assert z["tokens"].tolist() == want
    assert np.array_equal(z["attention"], torch.cat(want_attn).numpy())
    with pytest.raises(ValueError):
        ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=None, beam=beam, sample=dict(num_samples=2))
