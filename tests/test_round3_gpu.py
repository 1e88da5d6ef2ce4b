"""Round-3 parity additions (VERDICT r2 "untested configs" + ADVICE r2):
  * cfg4 at the batch the bench quotes (B = 64, V = 50 000, K = 20, F = 51): forward against a digest of the REAL
    reference's forward, and one captured TrainStep against the reference sequence on the oracle, with the GEMM
    plans of that instantiation asserted;
  * the news variant at V = 50 000, K = 51, F = 51 (name-word mean over the full embedding) against the reference digest;
  * cfg5 beam 5 at its real size (32 captions x 5 hypotheses = 160 rows, V = 10 000, K = 20): batch == per-caption,
    oracle beam search on three captions, beam 1 == greedy;
  * beam search where EVERY hypothesis ends before max_pred_len, at both parities of max_pred_len (the ping-pong
    hypothesis tables);
  * the public get_scores / get_context_indicators methods against the reference's own outputs.
"""
import numpy as np
import pytest
import torch

import ick_amd
import ick_amd.synth as synth
from helpers import case_from_golden, load_golden, t
from oracle import restatement as R
from test_bench_sizes_gpu import plan_log, plans_of, run_train_step_vs_oracle  # noqa: F401  (plan_log is a fixture)
from test_forward_gpu import build_decoder, run_forward
from test_oracle_golden import check_digest, unpack_pi

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------ cfg4 at B = 64
def test_cfg4_b64_forward_vs_reference_digest(plan_log, gemm_split):
    g = load_golden("digest_cfg4_b64")
    cfg, P, wm, batch, enc_out = case_from_golden(g)
    assert (int(g["B"]), int(g["V"]), int(g["F"])) == (64, 50000, 51)
    dec = build_decoder(cfg.variant, cfg.vocab_size, P)
    scores, caps, dl = run_forward(dec, batch, enc_out)
    assert dl == g["decode_lengths"].tolist() and torch.equal(caps.cpu(), t(g["captions_sorted"]))
    check_digest(g, scores.float().cpu(), tol=2e-4)
    # the instantiation behind DESIGN's cfg4 numbers: M = 1280 rows of the vocabulary GEMM, 12 544 rows of the K/V projection
    M = 64 * 20
    vocab = plans_of(plan_log, M, 50000, 300)
    assert vocab and vocab[0]["tile_m"] >= 64 and vocab[0]["vec"] == 1
    assert vocab[0]["split_bf16"] == (1 if gemm_split else 0)      # the mode under test really ran on this GEMM
    kv = plans_of(plan_log, 64 * 196, 1800, 300)
    assert kv and kv[0]["tile_m"] >= 64


def test_cfg4_b64_train_step_vs_oracle(plan_log, gemm_split):
    """One captured TrainStep of the knowledge variant at the bench batch against CE -> backward -> clamp -> Adam on the
    oracle (which the digest above pins to the real reference at this very size)."""
    c = synth.CONFIGS["cfg4"]
    ts, log = run_train_step_vs_oracle(c["variant"], c["B"], c["L"], c["K"], c["V"], c["F"], 41, plan_log)
    M = c["B"] * c["L"]
    dgrad = plans_of(log, M, 300, c["V"])
    assert dgrad and dgrad[0]["split_k"] >= 2          # the 50 000-long reduction is split over workgroups


# ------------------------------------------------------------------------------------------------ news at V = 50 000
def test_news_v50k_forward_vs_reference_digest(gemm_split):
    g = load_golden("digest_news_v50k")
    cfg, P, wm, batch, enc_out = case_from_golden(g)
    assert cfg.variant == "news" and int(g["V"]) == 50000 and int(g["K"]) == 51 and int(g["F"]) == 51
    dec = build_decoder(cfg.variant, cfg.vocab_size, P)
    stages = {}
    scores, caps, dl = run_forward(dec, batch, enc_out, stages)
    assert dl == g["decode_lengths"].tolist() and torch.equal(caps.cpu(), t(g["captions_sorted"]))
    check_digest(g, scores.float().cpu(), tol=2e-4)
    # the name-word mean gathers rows of the 50 000 x 300 embedding: exact against the oracle's gather
    with torch.no_grad():
        ee_ref = R.entity_encode(cfg, P, batch["entities"], batch["facts"])
    sort = batch["caption_lengths"].squeeze(1).sort(dim=0, descending=True).indices
    assert (stages["entities_encoded"].cpu() - ee_ref[sort]).abs().max().item() < 1e-6
    # and the graph-replayed inference path gives the same scores
    again, _, _ = run_forward(dec, batch, enc_out)
    assert (again - scores).abs().max().item() < 2e-5


# ------------------------------------------------------------------------------------------------ cfg5 beam 5 x 32
def test_cfg5_beam5_at_bench_size():
    """R = 32 x 5 = 160 rows (five 32-row blocks in dec_vocab), 10 020 scores per row (ten 1 024-score chunks)."""
    variant, B, K, V, max_len, beam, seed = "geo", 32, 20, 10000, 20, 5, 51
    P = synth.make_params(variant, V, seed)
    dec = build_decoder(variant, V, P)
    ents = synth.make_entities(variant, B, K, V, seed)
    enc = synth.make_enc_out(B, seed)
    full, score, allseq, allscore = dec.predict_beam(enc.cuda(), max_len, ents, beam_size=beam, return_all=True)
    assert full.shape == (max_len, B)
    again = dec.predict_beam(enc.cuda(), max_len, ents, beam_size=beam)          # graph replay
    assert torch.equal(again, full)
    flips = 0
    for b in range(B):
        one, s1, _, _ = dec.predict_beam(enc[b:b + 1].cuda(), max_len, ents[b:b + 1], beam_size=beam, return_all=True)
        if not torch.equal(one[:, 0], full[:, b]):      # a different row block / tile order may flip an exact tie only
            flips += 1
            assert abs(s1.item() - score[b].item()) < 1e-4, (b, s1.item(), score[b].item())
    assert flips <= 1
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    for b in (0, 13, 31):
        with torch.no_grad():
            ref_seq, ref_score, _ = R.predict_beam(cfg, P, enc[b:b + 1], max_len, ents[b:b + 1], None, beam)
        mine = full[:, b].cpu().tolist()
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], None, mine, max_len)
        assert abs(score[b].item() - own) < 1e-3                        # the device's cumulative score is right
        assert mine == ref_seq.tolist() or own > ref_score - 1e-3, (b, mine, ref_seq.tolist())
    assert torch.equal(dec.predict_beam(enc.cuda(), max_len, ents, beam_size=1), dec.predict(enc.cuda(), max_len, ents))


def test_cfg5_greedy_at_bench_size_vs_oracle(gemm_split):
    """Greedy at cfg5's size: 32 captions decoded together == each caption decoded by the oracle's full recompute."""
    variant, B, K, V, max_len, seed = "geo", 32, 20, 10000, 20, 52
    P = synth.make_params(variant, V, seed)
    dec = build_decoder(variant, V, P)
    ents = synth.make_entities(variant, B, K, V, seed)
    enc = synth.make_enc_out(B, seed)
    seqs = dec.predict(enc.cuda(), max_len, ents).cpu()
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    for b in (0, 7, 19, 31):
        with torch.no_grad():
            ref = R.predict(cfg, P, enc[b:b + 1], max_len, ents[b:b + 1])
        assert seqs[:, b].tolist() == ref.view(-1).tolist(), b


# ------------------------------------------------------------------------------------------------ beams that all end
@pytest.mark.parametrize("max_len", [9, 10])
@pytest.mark.parametrize("variant,bias,seed", [("geo", 50.0, 5), ("geo", 2.0, 5), ("geo", 2.5, 6), ("knowledge", 6.0, 5)])
def test_beam_every_hypothesis_ends_early(variant, bias, seed, max_len):
    """An <end>-biased vocabulary head: every hypothesis of every caption ends well before max_pred_len, after which the
    remaining steps only carry the tables between their two buffers.  Odd and even max_pred_len read the result from
    different buffers, and the cases end at step 1 (bias 50, 6) or step 2 (bias 2, 2.5: captions of one batch end at
    different steps)."""
    B, K, V, Fn, beam = 4, 6, 50, 5, 3
    P = synth.make_params(variant, V, seed)
    P["fc_vocab.bias"] = P["fc_vocab.bias"].clone()
    P["fc_vocab.bias"][V - 1] += bias
    dec = build_decoder(variant, V, P)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    ents = synth.make_entities(variant, B, K, V, seed)
    facts = synth.make_facts(variant, B, Fn, K, seed) if variant != "geo" else None
    enc = synth.make_enc_out(B, seed)
    args = [enc.cuda(), max_len, ents] + ([facts.cuda()] if facts is not None else [])
    for graphs in (True, False):
        dec.use_hip_graphs = graphs
        seq, score, allseq, allscore = dec.predict_beam(*args, beam_size=beam, return_all=True)
        ended = 0
        for b in range(B):
            with torch.no_grad():
                ref_seq, ref_score, hyps = R.predict_beam(cfg, P, enc[b:b + 1], max_len, ents[b:b + 1],
                                                          None if facts is None else facts[b:b + 1], beam)
            mine = seq[:, b].cpu().tolist()
            if all(len(h) < max_len - 1 for h, _ in hyps):
                ended += 1
            own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], None if facts is None else facts[b:b + 1],
                                     mine, max_len)
            assert abs(score[b].item() - own) < 1e-3, (b, mine, score[b].item(), own)
            assert mine == ref_seq.tolist() or own > ref_score - 1e-3, (graphs, b, mine, ref_seq.tolist())
            assert abs(score[b].item() - ref_score) < 1e-3
            # every surviving hypothesis of the caption: same set of (sequence, score) as the oracle's beam
            def upto_end(s):      # <pad> = 0 is a legal token inside a hypothesis; the padding starts after <end>
                return tuple(s[:s.index(cfg.end) + 1]) if cfg.end in s else tuple(s)
            got = sorted((upto_end(s), v) for s, v in
                         zip(allseq[b].cpu().tolist(), allscore[b].cpu().tolist()) if v != float("-inf"))
            want = sorted((tuple(h), v) for h, v in hyps)
            assert [q[0] for q in got] == [q[0] for q in want], (graphs, b, got, want)
            assert all(abs(q[1] - w[1]) < 1e-3 for q, w in zip(got, want)), (graphs, b, got, want)
        assert ended == B, "the case must end every beam early (%d of %d did)" % (ended, B)
    dec.use_hip_graphs = True


def test_beam_capacity_is_checked_before_capture():
    """beam^2 x ceil(Vx / 1024) candidates must fit the selection kernel; the check raises before anything is captured
    (ADVICE r2 low); beam 8 at the knowledge vocabulary of 50 071 scores is inside the capacity now."""
    import ick_amd.ops as ops
    assert ops.decode_beam_supported(50071, 8) and ops.decode_beam_supported(10020, 5)
    assert not ops.decode_beam_supported(70000, 8) and not ops.decode_beam_supported(100, 9)
    variant, B, K, V, seed = "geo", 2, 6, 50, 1
    dec = build_decoder(variant, V, synth.make_params(variant, V, seed))
    with pytest.raises(ick_amd.lib.IckError):
        dec.predict_beam(synth.make_enc_out(B, seed).cuda(), 8, synth.make_entities(variant, B, K, V, seed), beam_size=9)


# ------------------------------------------------------------------------------------------------ public score head
@pytest.mark.parametrize("name", ["score_head_geo", "score_head_knowledge", "score_head_news"])
def test_public_get_scores_and_context_indicators(name):
    """decoder.get_scores / get_context_indicators (geo-aware/models.py:291-313, knowledge-aware/models.py:380-455)
    with the reference's argument layout, against outputs of the reference's own methods."""
    g = load_golden(name)
    variant = str(g["variant"])
    B, L, K, V, Fn, seed = (int(g[k]) for k in ("B", "L", "K", "V", "F", "seed"))
    dec = build_decoder(variant, V, synth.make_params(variant, V, seed))
    h, ee = t(g["h"]).cuda(), t(g["ee"]).cuda()
    ref = t(g["scores"])
    if variant == "geo":
        out = dec.get_scores(h, ee)
        assert out.shape == ref.shape and (out.cpu() - ref).abs().max().item() < 2e-4
        with pytest.raises(AttributeError):          # the geo reference has no such method
            dec.get_context_indicators(None, None, K, L)
        return
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    facts = batch["facts"].clone()
    facts[:, :, 2] %= 3
    for tag, ol in (("full", L), ("short", L - 3), ("one", 1)):
        eib, pi = dec.get_context_indicators(batch["captions"].cuda(), facts.cuda(), K, ol)
        assert eib.shape == (B, ol, Fn, 1) and pi.shape == (B, ol, dec.num_predicates, 1)
        assert torch.equal(eib.cpu(), t(g["eib_" + tag]).float()), tag
        assert torch.equal(pi.cpu(), unpack_pi(g, tag, dec.num_predicates)), tag
    eib, pi = dec.get_context_indicators(batch["captions"].cuda(), facts.cuda(), K, L)
    out = dec.get_scores(h, ee, t(g["fe"]).cuda(), eib, pi)
    assert out.shape == ref.shape and (out.cpu() - ref).abs().max().item() < 2e-4
    # out_length beyond the caption buffer: the extra positions see every mention (reference loop semantics)
    eib2, pi2 = dec.get_context_indicators(batch["captions"].cuda(), facts.cuda(), K, L + 2)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    caps_pad = torch.cat([batch["captions"], torch.zeros(B, 2, dtype=torch.long)], dim=1)
    e_ref, p_ref = R.context_indicators(cfg, caps_pad, facts, K, L + 2)
    assert torch.equal(eib2.squeeze(3).cpu(), e_ref) and torch.equal(pi2.squeeze(3).cpu(), p_ref)
