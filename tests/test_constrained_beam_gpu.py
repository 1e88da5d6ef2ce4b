"""Constrained beam search on the device: the FORCED instantiations of dec_beam_partial_kernel and
dec_select_beam_kernel (csrc/decode_select.hip) behind predict_beam(force_tokens), held slot by slot to the CPU search of
tests/constrained_beam_ref.py on the oracle's scores, with the decoding rules of §3.2e composed."""
import pytest
import torch

import ick_amd.synth as synth
from ick_amd.decoder import length_penalty_table
from oracle import restatement as R
from beam_rules_ref import has_banned_ngram
from constrained_beam_ref import predict_constrained_beam
from test_decode_rules_gpu import args_of, one
from test_sample_gpu import make_case, upto_end

pytestmark = pytest.mark.gpu

RULES = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)


def beam_all(dec, enc, max_len, ents, facts, beam, **kw):
    """predict_beam with return_all, its values copied out of the graph's buffers."""
    res = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam, return_all=True, **kw)
    return [x.clone() for x in res]


def listed(res):
    return [x.clone() for x in res] if isinstance(res, tuple) else [res.clone()]


def graphs(dec):
    return len(dec.__dict__.get("_graphs", {}))


def forced_of(row):
    return [int(w) for w in row if int(w) >= 0]


def check_promise(cfg, force, best, allseq, allscore, rules=None):
    """Test 4's promise for every caption: the best contains every forced column, every ended hypothesis has them
    all, and with rules no hypothesis breaks one."""
    for b, row in enumerate(force):
        want = forced_of(row)
        got = upto_end(best[:, b].cpu().tolist(), cfg.end)
        assert all(w in got for w in want), (b, want, got)
        for h in range(allseq.shape[1]):
            if allscore[b, h].item() == float("-inf"):
                continue
            hyp = upto_end(allseq[b, h].cpu().tolist(), cfg.end)
            if hyp[-1] == cfg.end:
                assert all(w in hyp for w in want), (b, h, want, hyp)
            if rules:
                assert has_banned_ngram(hyp, rules["no_repeat_ngram_size"], rules["min_len"], cfg.end) is None, (b, h)


# ------------------------------------------------------------------------------------------------ 1. None
@pytest.mark.parametrize("rules", [False, True])
def test_none_is_the_call_without_the_argument(rules):
    dec, cfg, P, ents, facts, enc = make_case("knowledge", 3, 6, 200, 5, 2)
    args = args_of(enc, 10, ents, facts)
    kw = dict(RULES) if rules else {}
    for ra in (False, True):
        for at in (False, True):
            a = listed(dec.predict_beam(*args, beam_size=4, return_all=ra, return_attention=at, **kw))
            n = graphs(dec)
            b = listed(dec.predict_beam(*args, beam_size=4, return_all=ra, return_attention=at, force_tokens=None, **kw))
            assert len(a) == len(b)
            for x, y in zip(a, b):
                assert torch.equal(x, y), (ra, at)
            assert graphs(dec) == n                                           # the same graph kinds
    assert torch.equal(dec.predict_beam(*args, beam_size=1, force_tokens=None), dec.predict(*args))


# ------------------------------------------------------------------------------------------------ 2. all slots empty
@pytest.mark.parametrize("variant,beam,C", [("geo", 4, 1), ("knowledge", 5, 8), ("geo", 8, 3)])
@pytest.mark.parametrize("rules", [False, True])
def test_all_slots_empty_is_the_plain_search(variant, beam, C, rules):
    dec, cfg, P, ents, facts, enc = make_case(variant, 3, 6, 1500, 5, 5)
    kw = dict(RULES) if rules else {}
    want = beam_all(dec, enc, 10, ents, facts, beam, **kw)
    n = graphs(dec)
    got = beam_all(dec, enc, 10, ents, facts, beam, force_tokens=torch.full((3, C), -1), **kw)
    assert graphs(dec) == n + 1                                               # a graph kind of its own
    assert ("beam_force_rules" if rules else "beam_force") in {k[0] for k in dec.__dict__["_graphs"]}
    for x, y in zip(got, want):
        assert torch.equal(x, y)


def test_beam_one_runs_the_beam_kernels():
    """beam_size = 1 with force_tokens is one hypothesis on the beam kernels, as with a rule on (min_len = 1 bans
    nothing a caption could use at step 0 but <end>): not predict() and its clean-up."""
    dec, cfg, P, ents, facts, enc = make_case("geo", 3, 6, 300, 0, 5)
    empty = torch.full((3, 2), -1)
    got = dec.predict_beam(*args_of(enc, 10, ents, facts), beam_size=1, force_tokens=empty, return_all=True)
    assert isinstance(got, tuple) and got[2].shape == (3, 1, 10)
    assert "beam_force" in {k[0] for k in dec.__dict__["_graphs"]}
    want = beam_all(dec, enc, 10, ents, facts, 1, min_len=1)
    got = beam_all(dec, enc, 10, ents, facts, 1, force_tokens=empty, min_len=1)
    for x, y in zip(got, want):
        assert torch.equal(x, y)
    force = torch.tensor([[300 + 1, 20], [300 + 2, -1], [30, 300 + 5]])
    best, score, allseq, allscore = beam_all(dec, enc, 10, ents, facts, 1, force_tokens=force)
    check_promise(cfg, force.tolist(), best, allseq, allscore)


# ------------------------------------------------------------------------------------------------ 3. vs CPU reference
# (variant, V, beam, C, rules)
REF_CASES = [
    ("geo", 50, 3, 1, False), ("geo", 1000, 5, 2, True), ("geo", 1000, 1, 2, False), ("geo", 1000, 8, 4, True),
    ("knowledge", 50, 4, 3, True), ("knowledge", 1000, 5, 2, False), ("knowledge", 1000, 8, 8, False),
    ("geo", 10000, 5, 3, False), ("knowledge", 10000, 6, 2, True),
]
INEXACT = []                    # (case, seed) of every inexact input so far: at most two over the whole table


def draw_force(seed, V, Vx, C, special):
    """Slots in order: an even one holds V + randint(0, 6) (an entity pointer), an odd one randint(0, V+K+F); drawn
    again when the id is <start>, <end>, <pad> or already taken."""
    g = torch.Generator().manual_seed(100 + seed)
    out = []
    for s in range(C):
        while True:
            w = V + int(torch.randint(0, 6, (1,), generator=g)) if s % 2 == 0 else \
                int(torch.randint(0, Vx, (1,), generator=g))
            if w not in special and w not in out:
                break
        out.append(w)
    return out


def check_case(cfg, P, enc, ents, facts, max_len, beam, force, kw, what, res):
    """One caption against the reference, slot by slot; True when every hypothesis is identical.  Whatever the outcome,
    every returned score is the model's log-probability of its sequence; on a mismatch the device's best has at least
    the reference's bank, and at the same bank a key above the reference's minus 1e-3."""
    best, best_score, allseq, allscore = res
    ref_seq, ref_score, ref_key, ref_bank, slots = predict_constrained_beam(cfg, P, enc, max_len, ents, facts, beam,
                                                                            force, **kw)
    same = True
    for h in range(beam):
        ref = slots[h]
        s = allscore[0, h].item()
        if s == float("-inf"):
            same = same and ref is None
            continue
        hyp = upto_end(allseq[0, h].cpu().tolist(), cfg.end)
        own = R.sequence_logprob(cfg, P, enc, ents, facts, hyp, max_len)
        print(what, "slot", h, "device", hyp, s, "own", own, "ref", ref)
        assert abs(s - own) < 1e-3, (what, h, s, own)
        if ref is None or hyp != ref[0]:
            same = False
        else:
            assert abs(s - ref[1]) < 1e-3, (what, h, s, ref[1])
    got = upto_end(best[:, 0].cpu().tolist(), cfg.end)
    same = same and got == upto_end(ref_seq.tolist(), cfg.end)
    if not same:
        lp = length_penalty_table(kw.get("length_penalty", 0.0), max_len)
        bank = sum(1 for w in force if w in got)
        k = (best_score[0].cpu() / lp[len(got)]).item()
        print(what, "inexact: device best", got, "bank", bank, "key", k, "reference bank", ref_bank, "key", ref_key)
        assert bank >= ref_bank, (what, bank, ref_bank)
        assert bank > ref_bank or k > ref_key - 1e-3, (what, k, ref_key)
    return same


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "%s_V%d_b%d_C%d_r%d" % c)
def test_constrained_beam_vs_cpu_reference(case):
    variant, V, beam, C, rules = case
    kw = dict(RULES) if rules else {}
    max_len = 12 if C == 8 else 8
    exact = 0
    for seed in (3, 4):
        dec, cfg, P, ents, facts, enc = make_case(variant, 1, 6, V, 5, seed)
        Vx = V + 6 + (facts.shape[1] if facts is not None else 0)
        force = draw_force(seed, V, Vx, C, (cfg.start, cfg.end, cfg.pad))
        res = beam_all(dec, enc, max_len, ents, facts, beam, force_tokens=[force], **kw)
        ok = check_case(cfg, P, enc, ents, facts, max_len, beam, force, kw, (case, seed), res)
        exact += ok
        if not ok:
            INEXACT.append((case, seed))
    assert exact >= 1, case
    assert len(INEXACT) <= 2, INEXACT


# ------------------------------------------------------------------------------------------------ 4. the promise
def promise_force(variant, V, K, Fn):
    """0, 1, 3 and 8 slots for the four captions; fact pointers (V + K + j) in the knowledge case."""
    f = V + K if variant != "geo" else 7
    rows = [[], [V + 2], [V + 4, 11 if variant == "geo" else f + 1, V + 1],
            [V + 0, 5, V + 3, 9, V + 5, f, 13 if variant == "geo" else f + Fn - 1, 17]]
    return torch.tensor([r + [-1] * (8 - len(r)) for r in rows])


@pytest.mark.parametrize("variant", ["geo", "knowledge"])
@pytest.mark.parametrize("rules", [False, True])
def test_every_forced_column_is_in_the_caption(variant, rules):
    B, K, V, Fn, max_len, beam = 4, 6, 300, 5, 14, 4
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, V, Fn, 11)
    kw = dict(RULES) if rules else {}
    force = promise_force(variant, V, K, Fn)
    assert not any(w in (cfg.start, cfg.end, cfg.pad) for w in force.flatten().tolist())
    best, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, force_tokens=force, **kw)
    check_promise(cfg, force.tolist(), best, allseq, allscore, kw)
    for b in range(B):
        hyp = upto_end(best[:, b].cpu().tolist(), cfg.end)
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], one(facts, b), hyp, max_len)
        assert abs(score[b].item() - own) < 1e-3, (b, score[b].item(), own)
    # the teeth: the plain search does not name them all
    plain = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam, **kw)
    missed = sum(1 for b in range(B) for w in forced_of(force[b].tolist())
                 if w not in upto_end(plain[:, b].cpu().tolist(), cfg.end))
    assert missed >= 1
    # the caption without slots is the plain search's
    assert torch.equal(best[:, 0], plain[:, 0])


# ------------------------------------------------------------------------------------------------ 5. replay
def test_new_ids_replay_the_same_graph():
    dec, cfg, P, ents, facts, enc = make_case("geo", 3, 6, 60, 0, 2)
    V = 60

    def run(force, **kw):
        return beam_all(dec, enc, 12, ents, facts, 4, force_tokens=force, **kw)

    f1 = [[V + 1, 7, -1], [V + 2, -1, -1], [9, 10, V + 5]]
    f2 = torch.tensor([[V + 3], [V + 4], [12]])                              # another C: the same graph
    a1 = run(f1)
    n = graphs(dec)
    b1 = run(f2)
    a2 = run(f1)
    assert graphs(dec) == n
    r1 = run(f2, **RULES)
    assert graphs(dec) == n + 1                                                # one capture more: the rules graph
    r2 = run(f1, **RULES)
    assert graphs(dec) == n + 1
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(a1, b1))                  # the ids changed the decode
    dec.use_hip_graphs = False                                                  # the replays computed the new ids
    for want, f, kw in ((a1, f1, {}), (b1, f2, {}), (r1, f2, RULES), (r2, f1, RULES)):
        for x, y in zip(want, run(f, **kw)):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 6. batching
@pytest.mark.parametrize("variant,rules", [("geo", True), ("knowledge", False)])
def test_batch_is_independent(variant, rules):
    dec, cfg, P, ents, facts, enc = make_case(variant, 3, 6, 80, 5, 4)
    kw = dict(RULES) if rules else {}
    force = torch.tensor([[80 + 1, 20, -1], [-1, -1, -1], [30, 80 + 4, 80 + 2]])
    full = beam_all(dec, enc, 10, ents, facts, 4, force_tokens=force, **kw)
    for b in range(3):
        single = beam_all(dec, enc[b:b + 1], 10, ents[b:b + 1], one(facts, b), 4, force_tokens=force[b:b + 1], **kw)
        assert torch.equal(full[0][:, b:b + 1], single[0])
        for x, y in zip(full[1:], single[1:]):
            assert torch.equal(x[b:b + 1], y)


# ------------------------------------------------------------------------------------------------ 7. attention
@pytest.mark.parametrize("rules", [False, True])
def test_attention_does_not_change_the_decode(rules):
    B, beam, max_len, V = 3, 4, 10, 120
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 6, V, 5, 6)
    args = args_of(enc, max_len, ents, facts)
    kw = dict(beam_size=beam, force_tokens=[[V + 1, V + 6 + 2], [15, -1], [V + 3, 16]], **(RULES if rules else {}))
    best, score, allseq, allscore = listed(dec.predict_beam(*args, return_all=True, **kw))
    best2, score2, allseq2, allscore2, best_at, all_at = listed(dec.predict_beam(*args, return_all=True,
                                                                                 return_attention=True, **kw))
    assert torch.equal(best, best2) and torch.equal(score, score2)
    assert torch.equal(allseq, allseq2) and torch.equal(allscore, allscore2)
    layers, H, S = all_at.shape[3:]
    assert best_at.shape == (max_len, B, layers, H, S) and all_at.shape == (max_len, B, beam, layers, H, S)
    for b in range(B):
        rows = [h for h in range(beam) if torch.equal(allseq[b, h], best[:, b]) and allscore[b, h] == score[b]]
        assert rows and any(torch.equal(best_at[:, b], all_at[:, b, h]) for h in rows), b
    s, a = dec.predict_beam(*args, return_attention=True, **kw)
    assert torch.equal(s, best) and torch.equal(a, best_at)
    assert torch.equal(dec.predict_beam(*args, **kw), best)


# ------------------------------------------------------------------------------------------------ 8. envelope
def test_cfg5_sizes():
    """cfg5: 32 captions x 20 tokens, V 10 000, beam 5, three slots per caption."""
    B, V, K, max_len, beam = 32, 10000, 20, 20, 5
    dec, cfg, P, ents, facts, enc = make_case("geo", B, K, V, 0, 6)
    g = torch.Generator().manual_seed(5)
    force = torch.stack([V + torch.randint(0, K, (B,), generator=g), torch.randint(10, V - 10, (B,), generator=g),
                         torch.randint(10, V - 10, (B,), generator=g)], dim=1)
    best, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, force_tokens=force,
                                             no_repeat_ngram_size=3, length_penalty=0.6, min_len=5)
    assert best.shape == (max_len, B) and allseq.shape == (B, beam, max_len)
    check_promise(cfg, force.tolist(), best, allseq, allscore, dict(no_repeat_ngram_size=3, min_len=5))
    for b in (0, 17, 31):
        hyp = upto_end(best[:, b].cpu().tolist(), cfg.end)
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], None, hyp, max_len)
        print("cfg5", b, score[b].item(), own)
        assert abs(score[b].item() - own) < 1e-3, (b, score[b].item(), own)


def test_vocab_50k_beam_8_eight_slots():
    """V+K+F ~ 50 k (49 chunks of 1024 columns) with beam 8 and every slot in use."""
    B, V, K, Fn, max_len = 2, 50000, 30, 40, 10
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, K, V, Fn, 9)
    force = torch.tensor([[V + 3, 1024, V + K + 7, 2047, V + 29, 40000, V + K + 39, 49990],
                          [V + K, 2048, V, 10, 30000, V + 1, 1023, -1]])
    best, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, 8, force_tokens=force)
    check_promise(cfg, force.tolist(), best, allseq, allscore)
    for b in range(B):
        hyp = upto_end(best[:, b].cpu().tolist(), cfg.end)
        own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], facts[b:b + 1], hyp, max_len)
        print("50k", b, score[b].item(), own)
        assert abs(score[b].item() - own) < 1e-3, (b, score[b].item(), own)


def test_max_len_128_with_8_grams():
    B, V, max_len, beam = 2, 1000, 128, 3
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 6, V, 0, 8, end_bias=-4.0)
    kw = dict(no_repeat_ngram_size=8, min_len=100, length_penalty=1.0)
    force = torch.tensor([[V + 2, 50, V + 4, 60], [70, -1, -1, -1]])
    best, score, allseq, allscore = beam_all(dec, enc, max_len, ents, facts, beam, force_tokens=force, **kw)
    check_promise(cfg, force.tolist(), best, allseq, allscore, kw)
    for b in range(B):
        for h in range(beam):
            assert len(upto_end(allseq[b, h].cpu().tolist(), cfg.end)) >= 100
    own = R.sequence_logprob(cfg, P, enc[:1], ents[:1], None, upto_end(best[:, 0].cpu().tolist(), cfg.end), max_len)
    print("len128", score[0].item(), own)
    assert abs(score[0].item() - own) < 1e-3, (score[0].item(), own)


# ------------------------------------------------------------------------------------------------ 9. evaluation
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_evaluate_with_forced_entities(tmp_path, variant):
    import pandas as pd
    from ick_amd import eval as ev
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    from test_forward_gpu import build_decoder
    data_dir = str(tmp_path / "data")
    V, K, max_len = 60, 6, 10
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=2, n_test=5, L=12, K=K, V=V, F=5)
    dec = build_decoder(variant, V, synth.make_params(variant, V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=2, shuffle=False)
    seen = []

    def force(bi, batch):
        n = batch[0].shape[0]
        seen.append((bi, n))
        return torch.tensor([[V + (bi + b) % K, V + (bi + b + 2) % K] for b in range(n)])

    out = str(tmp_path / "forced.csv")
    caps, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=out,
                             beam=dict(beam_size=4, force_tokens=force, no_repeat_ngram_size=2))
    assert seen == [(0, 2), (1, 2), (2, 1)] and len(caps) == 5
    assert pd.read_csv(out, keep_default_na=False)["generated_caption"].tolist() == caps
    i = 0
    for bi, n in seen:
        for b in range(n):
            assert V + (bi + b) % K in seqs[i] and V + (bi + b + 2) % K in seqs[i], (i, seqs[i])
            i += 1
    plain, pseqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=out,
                               beam=dict(beam_size=4, no_repeat_ngram_size=2))
    assert pseqs != seqs
