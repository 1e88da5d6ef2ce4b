"""DecoderTransformer.predict_sample (csrc/sample.hip) on the GPU: every sampled token restated exactly -- the row's
sequence teacher-forced through the oracle, the kept set and the Philox-Gumbel draw rebuilt in numpy (sample_ref.py)
-- plus the first-token distribution, determinism / batch independence, top_k = 1 == argmax, early ends, the bench
sizes, argument errors and eval's sampled CSV."""
import math

import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.synth as synth
from ick_amd.lib import IckError
from oracle import restatement as R
from sample_ref import draw, gumbel
from test_forward_gpu import build_decoder

pytestmark = pytest.mark.gpu

KNOBS = [(1.0, 0, 1.0), (0.7, 5, 1.0), (1.3, 0, 0.8), (1.0, 8, 0.9)]
MARGIN, BOUNDARY = 1e-4, 1e-5


def upto_end(seq, end):
    seq = list(seq)
    return seq[:seq.index(end) + 1] if end in seq else seq


def teacher_forced_scores(cfg, P, enc_b, ents_b, facts_b, toks, max_len):
    """Oracle raw scores (V+K+F, float64) of every step of the token list `toks` (one caption, <start> first)."""
    V, K = cfg.vocab_size, ents_b.shape[1]
    with torch.no_grad():
        ee = R.entity_encode(cfg, P, ents_b, facts_b)
        fe = R.fact_encode(P, facts_b, ee) if cfg.has_facts else None
        mem = R.build_memory(cfg, P, enc_b, ee, fe)
        cap = [cfg.start] + toks[:max_len - 1]
        cap = cap + [cfg.start] * (max_len - len(cap))
        masks = [0] + [2 if (cfg.has_facts and q >= V + K) else (1 if q >= V else 0) for q in cap[1:]]
        emb = R.caption_embed(cfg, P, torch.tensor([cap]), torch.tensor([masks]), ee, fe)
        pe = R.pe_table(max_len, cfg.emb_dim).unsqueeze(0)
        h = R.decoder_stack(cfg, P, emb * math.sqrt(cfg.emb_dim) + pe, mem)
        out = []
        for i in range(len(toks)):
            hh = h[:, i:i + 1]
            if cfg.has_facts:
                buf = torch.tensor([cap[:i + 1] + [cfg.start] * (max_len - i - 1)])
                eib, pi = R.context_indicators(cfg, buf, facts_b, K, 1)
                sc = R.get_scores(cfg, P, hh, ee, fe, eib, pi)
            else:
                sc = R.get_scores(cfg, P, hh, ee)
            out.append(sc[0, 0].double().numpy())
    return out


def restate_rows(cfg, P, enc, ents, facts, seqs, lps, rows, n, seed, knobs, max_len, what):
    """Asserts the rule-by-rule restatement on the given rows; returns the number of excused steps."""
    T, k, p = knobs
    excused = []
    for r in rows:
        b, j = r // n, r % n
        toks = upto_end(seqs[:, r].tolist(), cfg.end)
        fb = None if facts is None else facts[b:b + 1]
        sc = teacher_forced_scores(cfg, P, enc[b:b + 1], ents[b:b + 1], fb, toks, max_len)
        for i, t in enumerate(toks):
            s = sc[i].astype(np.float32)
            g = gumbel(seed, b, j, i, s.size)
            want, keep, vals, ratio = draw(s, T, k, p, g)
            if t != want:
                margin = vals[0] - vals[1] if vals.size > 1 else np.inf
                kth = np.sort(s)[::-1][k - 1] if 0 < k < s.size else None
                near_k = kth is not None and (abs(s[t] - kth) < MARGIN or abs(s[want] - kth) < MARGIN)
                near_p = p < 1 and (abs(ratio[t]) < BOUNDARY or abs(ratio[want]) < BOUNDARY)
                assert margin < MARGIN or near_k or near_p, (what, r, i, t, want, margin)
                excused.append((r, i, t, want, float(margin)))
            else:
                assert keep[t]
            lsm = sc[i] - (sc[i].max() + np.log(np.exp(sc[i] - sc[i].max()).sum()))
            assert abs(lps[i, r].item() - lsm[t]) < 1e-4, (what, r, i, lps[i, r].item(), lsm[t])
        L = len(toks)
        assert all(q == cfg.pad for q in seqs[L:, r].tolist()) and (lps[L:, r] == 0).all()
    assert len(excused) <= 1, (what, excused)
    if excused:
        print("%s: excused near-tie step %s" % (what, excused))
    return len(excused)


def make_case(variant, B, K, V, Fn, seed, end_bias=0.0):
    P = synth.make_params(variant, V, seed)
    if end_bias:
        P["fc_vocab.bias"] = P["fc_vocab.bias"].clone()
        P["fc_vocab.bias"][V - 1] += end_bias
    dec = build_decoder(variant, V, P)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    ents = synth.make_entities(variant, B, K, V, seed)
    facts = synth.make_facts(variant, B, Fn, K, seed) if variant != "geo" else None
    enc = synth.make_enc_out(B, seed)
    return dec, cfg, P, ents, facts, enc


def call(dec, enc, max_len, ents, facts, **kw):
    args = [enc.cuda(), max_len, ents] + ([facts.cuda()] if facts is not None else [])
    return dec.predict_sample(*args, return_log_probs=True, **kw)


# ------------------------------------------------------------------------------------------------ exact restatement
@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "T%g_k%d_p%g" % k)
@pytest.mark.parametrize("variant", ["geo", "knowledge", "news"])
def test_sample_restated_exactly(variant, knobs, gemm_split):
    B, K, V, Fn, n, max_len, seed = 2, 6, 50, 5, 3, 8, 7
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 3)
    T, k, p = knobs
    seqs, lps = call(dec, enc, max_len, ents, facts, num_samples=n, temperature=T, top_k=k, top_p=p, seed=seed)
    assert seqs.shape == (max_len, B * n) and lps.shape == (max_len, B * n)
    seqs, lps = seqs.cpu(), lps.cpu()
    restate_rows(cfg, P, enc, ents, facts, seqs, lps, range(B * n), n, seed, knobs, max_len, variant)
    # the log-probabilities sum to the oracle's sequence log-probability
    toks = upto_end(seqs[:, 0].tolist(), cfg.end)
    own = R.sequence_logprob(cfg, P, enc[:1], ents[:1], None if facts is None else facts[:1], toks, max_len)
    assert abs(lps[:, 0].sum().item() - own) < 1e-3


# ------------------------------------------------------------------------------------------------ distribution
def tv_and_chi2(first, prob, n):
    from scipy.stats import chi2
    counts = np.bincount(first, minlength=prob.size).astype(np.float64)
    tv = 0.5 * np.abs(counts / n - prob).sum()
    exp = prob * n
    big = exp >= 5
    obs_b = np.append(counts[big], counts[~big].sum())
    exp_b = np.append(exp[big], exp[~big].sum())
    keep = exp_b > 0
    stat = (((obs_b - exp_b) ** 2)[keep] / exp_b[keep]).sum()
    return tv, chi2.sf(stat, keep.sum() - 1)


def test_first_token_distribution():
    """4096 samples of one caption's first token against softmax(s / T) over the kept set.  (An untruncated leg at
    T = 3 over all 23 scores is not asserted on: its distribution is nearly flat, and the expected total variation of
    4096 draws over 23 near-equal bins is itself ~0.03.)"""
    variant, K, V, seed, n = "geo", 3, 20, 9, 4096
    dec, cfg, P, ents, _, enc = make_case(variant, 1, K, V, 0, seed)
    s = teacher_forced_scores(cfg, P, enc, ents, None, [0], 2)[0]
    top3 = np.argsort(-s)[:3]
    for T, k in ((1.5, 0), (3.0, 3)):
        seqs = dec.predict_sample(enc.cuda(), 2, ents, num_samples=n, temperature=T, top_k=k, seed=1234).cpu()
        z = s / T
        prob = np.exp(z - z.max())
        if k:
            mask = np.zeros(s.size, dtype=bool)
            mask[top3] = True
            prob = np.where(mask, prob, 0.0)
            assert set(seqs[0].tolist()) == set(top3.tolist())       # exactly the three top tokens appear
        prob /= prob.sum()
        tv, pval = tv_and_chi2(seqs[0].numpy(), prob, n)
        assert tv <= 0.03 and pval > 1e-4, (T, k, tv, pval)


# ------------------------------------------------------------------------------------------------ determinism
def test_determinism_and_independence():
    variant, B, K, V, max_len, n = "geo", 32, 6, 50, 8, 2
    dec, cfg, P, ents, _, enc = make_case(variant, B, K, V, 0, 21)
    kw = dict(num_samples=n, temperature=1.2, top_k=10, top_p=0.95)
    s1, l1 = call(dec, enc, max_len, ents, None, seed=5, **kw)
    s2, l2 = call(dec, enc, max_len, ents, None, seed=5, **kw)           # graph replay
    dec.use_hip_graphs = False
    s3, l3 = call(dec, enc, max_len, ents, None, seed=5, **kw)           # eager
    dec.use_hip_graphs = True
    assert torch.equal(s1, s2) and torch.equal(l1, l2) and torch.equal(s1, s3) and torch.equal(l1, l3)
    s4, _ = call(dec, enc, max_len, ents, None, seed=6, **kw)
    assert not torch.equal(s1, s4)
    torch.manual_seed(17)
    a, _ = call(dec, enc, max_len, ents, None, **kw)
    b_, _ = call(dec, enc, max_len, ents, None, **kw)
    torch.manual_seed(17)
    c, _ = call(dec, enc, max_len, ents, None, **kw)
    assert torch.equal(a, c) and not torch.equal(a, b_)
    # the samples of captions 0..3 do not depend on the rest of the batch.  The tokens are bit-identical; the
    # log-probabilities agree to rounding only: the decoder-stack kernels group rows by batch size (plan_groups), which
    # changes the summation order of the scores in their last bits
    s5, l5 = call(dec, enc[:4], max_len, ents[:4], None, seed=5, **kw)
    assert torch.equal(s5, s1[:, :4 * n]) and (l5 - l1[:, :4 * n]).abs().max().item() < 1e-5
    # feature-map input (attached encoder) == the encoder output it makes
    from test_bench_sizes_gpu import make_encoder
    encm, _, _ = make_encoder(21)
    feats = synth.make_feats(4, 21).cuda()
    with torch.no_grad():
        e = encm(feats)
    ref = call(dec, e, max_len, ents[:4], None, seed=5, **kw)
    dec.attach_encoder(encm)
    got = call(dec, feats, max_len, ents[:4], None, seed=5, **kw)
    assert torch.equal(ref[0], got[0]) and torch.equal(ref[1], got[1])


# ------------------------------------------------------------------------------------------------ top_k = 1
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_top_k_1_is_argmax_without_cleanup(variant):
    B, K, V, Fn, max_len = 4, 6, 50, 5, 10
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 13)
    seqs, lps = call(dec, enc, max_len, ents, facts, top_k=1, seed=3, temperature=0.9)
    seqs = seqs.cpu()
    ties = 0
    for b in range(B):
        toks = upto_end(seqs[:, b].tolist(), cfg.end)
        sc = teacher_forced_scores(cfg, P, enc[b:b + 1], ents[b:b + 1], None if facts is None else facts[b:b + 1],
                                   toks, max_len)
        for i, t in enumerate(toks):
            top2 = np.sort(sc[i])[::-1][:2]
            if t != int(np.argmax(sc[i])):
                assert top2[0] - top2[1] < MARGIN
                ties += 1
    assert ties <= 1


# ------------------------------------------------------------------------------------------------ early ends
@pytest.mark.parametrize("max_len", [9, 10])
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_every_row_ends_early(variant, max_len):
    B, K, V, Fn, n = 4, 6, 50, 5, 3
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 5, end_bias=50.0)
    for graphs in (True, False):
        dec.use_hip_graphs = graphs
        seqs, lps = call(dec, enc, max_len, ents, facts, num_samples=n, seed=11)
        seqs, lps = seqs.cpu(), lps.cpu()
        for r in range(B * n):
            toks = upto_end(seqs[:, r].tolist(), cfg.end)
            assert toks[-1] == cfg.end and len(toks) < max_len
            assert all(q == cfg.pad for q in seqs[len(toks):, r].tolist()) and (lps[len(toks):, r] == 0).all()
            assert (lps[:len(toks), r] <= 0).all()
        restate_rows(cfg, P, enc, ents, facts, seqs, lps, range(B * n), n, 11, (1.0, 0, 1.0), max_len, "end")
    dec.use_hip_graphs = True


# ------------------------------------------------------------------------------------------------ bench sizes
@pytest.mark.parametrize("n", [1, 5])
def test_cfg5_sizes(n):
    variant, B, K, V, max_len, seed = "geo", 32, 20, 10000, 20, 52
    dec, cfg, P, ents, _, enc = make_case(variant, B, K, V, 0, seed)
    knobs = (1.0, 0, 1.0) if n == 1 else (0.8, 0, 0.9)
    kw = dict(num_samples=n, temperature=knobs[0], top_k=knobs[1], top_p=knobs[2], seed=77)
    s1, l1 = call(dec, enc, max_len, ents, None, **kw)
    s2, l2 = call(dec, enc, max_len, ents, None, **kw)
    assert torch.equal(s1, s2) and torch.equal(l1, l2) and s1.shape == (max_len, B * n)
    restate_rows(cfg, P, enc, ents, None, s1.cpu(), l1.cpu(), [0, B * n - 1], n, 77, knobs, max_len, "cfg5")


def test_cfg4_knowledge_sizes():
    variant, B, K, V, Fn, max_len, seed = "knowledge", 4, 20, 50000, 51, 20, 41
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, seed)
    knobs = (1.0, 0, 0.9)
    kw = dict(num_samples=2, temperature=1.0, top_p=0.9, seed=8)
    s1, l1 = call(dec, enc, max_len, ents, facts, **kw)
    s2, l2 = call(dec, enc, max_len, ents, facts, **kw)
    assert torch.equal(s1, s2) and torch.equal(l1, l2)
    restate_rows(cfg, P, enc, ents, facts, s1.cpu(), l1.cpu(), [0, 7], 2, 8, knobs, max_len, "cfg4")


# ------------------------------------------------------------------------------------------------ argument errors
def test_argument_errors_raise_before_capture():
    dec, cfg, P, ents, _, enc = make_case("geo", 2, 6, 50, 0, 1)
    e = enc.cuda()
    bad = [dict(temperature=0.0), dict(temperature=-1.0), dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.5),
           dict(num_samples=0), dict(num_samples=40000)]
    for kw in bad:
        with pytest.raises(IckError):
            dec.predict_sample(e, 8, ents, **kw)
    with pytest.raises(IckError):
        dec.predict_sample(e, 200, ents)                # longer than the fused decode kernels handle
    assert not dec.__dict__.get("_graphs")              # nothing was captured


# ------------------------------------------------------------------------------------------------ eval
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_evaluate_writes_one_row_per_sample(tmp_path, variant):
    import pandas as pd
    from ick_amd import eval as ev
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    data_dir = str(tmp_path / "data")
    V = 60
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=2, n_test=5, L=12, K=6, V=V, F=5)
    dec = build_decoder(variant, V, synth.make_params(variant, V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=2, shuffle=False)
    out = str(tmp_path / "sampled.csv")
    caps, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=10, out_csv=out,
                             sample=dict(num_samples=3, temperature=1.0, top_p=0.9, seed=4))
    df = pd.read_csv(out, keep_default_na=False)
    assert list(df.columns) == ["image", "sample", "generated_caption"] and len(df) == 5 * 3 == len(caps)
    assert df["image"].tolist() == [i // 3 for i in range(15)] and df["sample"].tolist() == [i % 3 for i in range(15)]
    greedy = str(tmp_path / "greedy.csv")
    ev.evaluate(enc, dec, loader, wm, max_caption_len=10, out_csv=greedy)
    assert list(pd.read_csv(greedy).columns) == ["generated_caption"] and len(pd.read_csv(greedy)) == 5
