"""Diverse beam search on the device: the DIVERSE instantiations of dec_select_beam_kernel
(csrc/decode_select.hip) behind predict_beam(num_beam_groups, diversity_penalty, return_groups), held group by group to the
CPU search of tests/diverse_beam_ref.py on the oracle's scores, with the decoding rules of §3.2e composed."""
import numpy as np
import pytest
import torch

import ick_amd.synth as synth
from oracle import restatement as R
from beam_rules_ref import has_banned_ngram, step_logp
from diverse_beam_ref import group_best, predict_diverse_beam
from test_decode_rules_gpu import args_of, one
from test_sample_gpu import make_case, upto_end

pytestmark = pytest.mark.gpu

RULES = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)


def beam_all(dec, enc, max_len, ents, facts, beam, **kw):
    """predict_beam with return_all, its values copied out of the graph's buffers."""
    res = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam, return_all=True, **kw)
    return [x.clone() for x in res]


# ------------------------------------------------------------------------------------------------ 1. G = 1
@pytest.mark.parametrize("lam", [0.0, 0.7, 5.0])
@pytest.mark.parametrize("rules", [False, True])
def test_one_group_is_the_call_without_groups(lam, rules):
    dec, cfg, P, ents, facts, enc = make_case("knowledge", 3, 6, 200, 5, 2)
    args = args_of(enc, 10, ents, facts)
    kw = dict(RULES) if rules else {}
    for ra in (False, True):
        for at in (False, True):
            a = dec.predict_beam(*args, beam_size=4, return_all=ra, return_attention=at, **kw)
            a = [x.clone() for x in a] if isinstance(a, tuple) else [a.clone()]
            graphs = len(dec.__dict__["_graphs"])
            for extra in (dict(num_beam_groups=1, diversity_penalty=lam),
                          dict(num_beam_groups=1, diversity_penalty=lam, return_groups=True)):
                b = dec.predict_beam(*args, beam_size=4, return_all=ra, return_attention=at, **kw, **extra)
                b = list(b) if isinstance(b, tuple) else [b]
                assert len(a) == len(b)
                for x, y in zip(a, b):
                    assert torch.equal(x, y), (ra, at, extra)
            assert len(dec.__dict__["_graphs"]) == graphs                      # the same graph kinds
    assert torch.equal(dec.predict_beam(*args, beam_size=1, num_beam_groups=1, diversity_penalty=lam),
                       dec.predict(*args))


# ------------------------------------------------------------------------------------------------ 2. lambda = 0
@pytest.mark.parametrize("variant,beam,G", [("geo", 4, 2), ("knowledge", 6, 3), ("geo", 6, 3)])
def test_zero_penalty_groups_are_the_narrow_beam(variant, beam, G):
    dec, cfg, P, ents, facts, enc = make_case(variant, 3, 6, 300, 5, 5)
    kg = beam // G
    _, _, nseq, nscore = beam_all(dec, enc, 10, ents, facts, kg)
    _, _, seq, score = beam_all(dec, enc, 10, ents, facts, beam, num_beam_groups=G, diversity_penalty=0.0)
    for g in range(G):
        assert torch.equal(seq[:, g * kg:(g + 1) * kg], nseq), g
        assert torch.allclose(score[:, g * kg:(g + 1) * kg], nscore, atol=1e-4, rtol=0), g


# ------------------------------------------------------------------------------------------------ 3. vs CPU reference
# (variant, V, beam, G, lambda, rules)
REF_CASES = [
    ("geo", 50, 4, 2, 0.5, False), ("geo", 1000, 6, 3, 2.0, True), ("geo", 10000, 8, 4, 10.0, False),
    ("geo", 1000, 8, 8, 2.0, True), ("geo", 50, 6, 2, 10.0, True), ("knowledge", 50, 6, 2, 2.0, True),
    ("knowledge", 1000, 8, 8, 0.5, False), ("knowledge", 10000, 6, 3, 0.5, True), ("knowledge", 1000, 4, 2, 10.0, True),
    ("knowledge", 50, 8, 4, 2.0, False),
]


def check_case(dec, cfg, P, enc, ents, facts, max_len, beam, G, kw, b, what, res):
    """Caption b against the reference, group by group; True when every group's hypotheses are identical.  Whatever
    the outcome, every returned score is the model's log-probability of its sequence and every hypothesis obeys the
    rules."""
    _, _, allseq, allscore = res
    eb, nb, fb = enc[b:b + 1], ents[b:b + 1], one(facts, b)
    _, _, _, groups = predict_diverse_beam(cfg, P, eb, max_len, nb, fb, beam, G, **kw)
    kg = beam // G
    same = True
    for h in range(beam):
        ref = groups[h // kg][h % kg]
        s = allscore[b, h].item()
        if s == float("-inf"):
            same = same and ref is None
            continue
        hyp = upto_end(allseq[b, h].cpu().tolist(), cfg.end)
        own = R.sequence_logprob(cfg, P, eb, nb, fb, hyp, max_len)
        assert abs(s - own) < 1e-3, (what, h, s, own)
        assert has_banned_ngram(hyp, kw.get("no_repeat_ngram_size", 0), kw.get("min_len", 0), cfg.end) is None, \
            (what, h, hyp)
        if ref is None or hyp != ref[0]:
            same = False
        else:
            assert abs(s - ref[1]) < 1e-3, (what, h, s, ref[1])
    return same


@pytest.mark.parametrize("case", REF_CASES, ids=lambda c: "%s_V%d_b%d_G%d_l%g_r%d" % c)
def test_diverse_beam_vs_cpu_reference(case):
    variant, V, beam, G, lam, rules = case
    kw = dict(diversity_penalty=lam, **(RULES if rules else {}))
    seeds = (3, 4)
    exact = 0
    for seed in seeds:
        dec, cfg, P, ents, facts, enc = make_case(variant, 1, 6, V, 5, seed)
        res = beam_all(dec, enc, 8, ents, facts, beam, num_beam_groups=G, **kw)
        exact += check_case(dec, cfg, P, enc, ents, facts, 8, beam, G, kw, 0, (case, seed), res)
    assert exact >= len(seeds) - 1


# ------------------------------------------------------------------------------------------------ 4. step 0
@pytest.mark.parametrize("variant,beam", [("geo", 4), ("knowledge", 8)])
def test_large_penalty_spreads_the_first_tokens(variant, beam):
    """G = beam, lambda = 1e4, no rules: at step 0 the groups emit the caption's beam best first tokens, in order."""
    B, K = 3, 6
    dec, cfg, P, ents, facts, enc = make_case(variant, B, K, 500, 5, 7)
    _, _, seq, _ = beam_all(dec, enc, 4, ents, facts, beam, num_beam_groups=beam, diversity_penalty=1e4)
    checked = 0
    for b in range(B):
        eb, nb, fb = enc[b:b + 1], ents[b:b + 1], one(facts, b)
        with torch.no_grad():
            ee = R.entity_encode(cfg, P, nb, fb)
            fe = R.fact_encode(P, fb, ee) if cfg.has_facts else None
            mem = R.build_memory(cfg, P, eb, ee, fe)
            logp = step_logp(cfg, P, ee, fe, mem, R.pe_table(4, cfg.emb_dim).unsqueeze(0), fb, K, [], 0, 4)
        top = logp.topk(beam + 1)
        if (top.values[:-1] - top.values[1:]).min().item() < 1e-4:          # too close to call in fp32
            continue
        assert seq[b, :, 0].cpu().tolist() == top.indices[:beam].tolist(), b
        checked += 1
    assert checked >= 2


# ------------------------------------------------------------------------------------------------ 5. replay
def test_penalty_change_replays_the_same_graph():
    dec, cfg, P, ents, facts, enc = make_case("geo", 3, 6, 60, 0, 2)
    args = args_of(enc, 12, ents, facts)

    def run(lam, **kw):
        return [x.clone() for x in dec.predict_beam(*args, beam_size=6, return_all=True, num_beam_groups=3,
                                                    diversity_penalty=lam, **kw)]

    a1 = run(0.5)
    graphs = len(dec.__dict__["_graphs"])
    b1 = run(3.0)
    a2 = run(0.5)
    r1 = run(3.0, **RULES)
    assert len(dec.__dict__["_graphs"]) == graphs + 1                        # one capture more: the rules graph
    r2 = run(1.0, **RULES)
    assert len(dec.__dict__["_graphs"]) == graphs + 1
    for x, y in zip(a1, a2):
        assert torch.equal(x, y)
    assert not all(torch.equal(x, y) for x, y in zip(a1, b1))                # lambda changed the decode
    dec.use_hip_graphs = False                                                # the replays computed the new lambda
    for want, lam, kw in ((b1, 3.0, {}), (r1, 3.0, RULES), (r2, 1.0, RULES)):
        for x, y in zip(want, run(lam, **kw)):
            assert torch.equal(x, y)


# ------------------------------------------------------------------------------------------------ 6. batching
@pytest.mark.parametrize("variant,rules", [("geo", True), ("knowledge", False)])
def test_batch_is_independent(variant, rules):
    dec, cfg, P, ents, facts, enc = make_case(variant, 3, 6, 80, 5, 4)
    kw = dict(num_beam_groups=2, diversity_penalty=1.5, **(RULES if rules else {}))
    full = beam_all(dec, enc, 10, ents, facts, 4, **kw)
    for b in range(3):
        single = beam_all(dec, enc[b:b + 1], 10, ents[b:b + 1], one(facts, b), 4, **kw)
        assert torch.equal(full[0][:, b:b + 1], single[0])
        for x, y in zip(full[1:], single[1:]):
            assert torch.equal(x[b:b + 1], y)


# ------------------------------------------------------------------------------------------------ 7. return_groups
@pytest.mark.parametrize("rules", [False, True])
def test_return_groups_shapes_and_consistency(rules):
    B, beam, G, max_len = 3, 6, 3, 10
    kg = beam // G
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 6, 120, 5, 6)
    args = args_of(enc, max_len, ents, facts)
    kw = dict(beam_size=beam, num_beam_groups=G, diversity_penalty=1.0, **(RULES if rules else {}))
    best, best_lp, allseq, allscore, best_at, all_at = [x.clone() for x in dec.predict_beam(
        *args, return_all=True, return_attention=True, **kw)]
    gseq, glp, allseq2, allscore2, gat, all_at2 = [x.clone() for x in dec.predict_beam(
        *args, return_all=True, return_attention=True, return_groups=True, **kw)]
    layers, H, S = all_at.shape[3:]
    assert gseq.shape == (max_len, B * G) and glp.shape == (B * G,) and gat.shape == (max_len, B * G, layers, H, S)
    assert best.shape == (max_len, B) and best_at.shape == (max_len, B, layers, H, S)
    assert torch.equal(allseq, allseq2) and torch.equal(allscore, allscore2) and torch.equal(all_at, all_at2)
    lp = torch.tensor([((5.0 + L) / 6.0) ** RULES["length_penalty"] if rules else 1.0 for L in range(max_len + 1)],
                      dtype=torch.float64).float()
    lp[0] = 1.0
    for b in range(B):
        keys = []
        for h in range(beam):
            L = len(upto_end(allseq[b, h].cpu().tolist(), cfg.end))
            keys.append((allscore[b, h].cpu() / lp[L]).item() if rules else allscore[b, h].item())
        for g in range(G):
            h = g * kg + group_best([(None, 0, 0, k) for k in keys[g * kg:(g + 1) * kg]])
            col = b * G + g
            assert torch.equal(gseq[:, col], allseq[b, h]) and glp[col].item() == allscore[b, h].item(), (b, g)
            assert torch.equal(gat[:, col], all_at[:, b, h]), (b, g)
        h = max(range(beam), key=lambda q: (keys[q], -q))
        assert torch.equal(best[:, b], allseq[b, h]) and torch.equal(best_at[:, b], all_at[:, b, h])
    # without return_all / return_attention: the same group columns
    assert torch.equal(dec.predict_beam(*args, return_groups=True, **kw), gseq)
    s, a = dec.predict_beam(*args, return_groups=True, return_attention=True, **kw)
    assert torch.equal(s, gseq) and torch.equal(a, gat)


def test_groups_differ_more_than_the_plain_beam():
    """With a penalty, the group bests of a width-6 beam share fewer first tokens than the plain beam's top three."""
    B = 8
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 6, 300, 0, 8)
    args = args_of(enc, 10, ents, facts)
    g = dec.predict_beam(*args, beam_size=6, num_beam_groups=3, diversity_penalty=2.0, return_groups=True)
    _, _, allseq, _ = dec.predict_beam(*args, beam_size=6, return_all=True)
    div = sum(len({tuple(upto_end(g[:, b * 3 + j].cpu().tolist(), cfg.end)) for j in range(3)}) for b in range(B))
    plain = sum(len({tuple(upto_end(allseq[b, j].cpu().tolist(), cfg.end)) for j in range(3)}) for b in range(B))
    assert div == 3 * B and div >= plain
    first_div = sum(len({g[0, b * 3 + j].item() for j in range(3)}) for b in range(B))
    first_plain = sum(len({allseq[b, j, 0].item() for j in range(3)}) for b in range(B))
    assert first_div > first_plain


# ------------------------------------------------------------------------------------------------ 8. envelope
def test_cfg5_sizes():
    """cfg5: 32 captions x 20 tokens, V 10 000, beam 6 in 3 groups, rules on; a few captions' scores checked."""
    B, V, max_len, beam, G = 32, 10000, 20, 6, 3
    dec, cfg, P, ents, facts, enc = make_case("geo", B, 20, V, 0, 6)
    kw = dict(num_beam_groups=G, diversity_penalty=0.5, no_repeat_ngram_size=3, length_penalty=0.6, min_len=5)
    gseq, glp, allseq, allscore = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=beam,
                                                   return_all=True, return_groups=True, **kw)
    assert gseq.shape == (max_len, B * G) and allseq.shape == (B, beam, max_len)
    assert torch.isfinite(allscore).all()
    for b in (0, 17, 31):
        for g in range(G):
            hyp = upto_end(gseq[:, b * G + g].cpu().tolist(), cfg.end)
            assert has_banned_ngram(hyp, 3, 5, cfg.end) is None
            own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], None, hyp, max_len)
            assert abs(glp[b * G + g].item() - own) < 2e-3, (b, g)


def test_vocab_50k_beam_8_four_groups():
    """V+K+F ~ 50 k (49 chunks of 1024 columns) with beam 8 in 4 groups."""
    B, V, max_len = 2, 50000, 8
    dec, cfg, P, ents, facts, enc = make_case("knowledge", B, 30, V, 40, 9)
    gseq, glp, allseq, allscore = dec.predict_beam(*args_of(enc, max_len, ents, facts), beam_size=8, return_all=True,
                                                   return_groups=True, num_beam_groups=4, diversity_penalty=1.0)
    assert gseq.shape == (max_len, B * 4) and torch.isfinite(allscore).all()
    for b in range(B):
        for g in range(4):
            hyp = upto_end(gseq[:, b * 4 + g].cpu().tolist(), cfg.end)
            own = R.sequence_logprob(cfg, P, enc[b:b + 1], ents[b:b + 1], facts[b:b + 1], hyp, max_len)
            assert abs(glp[b * 4 + g].item() - own) < 1e-3, (b, g)


# ------------------------------------------------------------------------------------------------ 9. evaluation
@pytest.mark.parametrize("variant", ["geo", "knowledge"])
def test_evaluate_with_groups(tmp_path, variant):
    import pandas as pd
    from ick_amd import eval as ev
    from ick_amd.datasets import CaptionDataset
    from test_bench_sizes_gpu import make_encoder
    from test_forward_gpu import build_decoder
    data_dir = str(tmp_path / "data")
    V, max_len, G = 60, 10, 3
    wm = synth.write_dataset(data_dir, "toy", variant, n_train=4, n_val=2, n_test=5, L=12, K=6, V=V, F=5)
    dec = build_decoder(variant, V, synth.make_params(variant, V, 2))
    enc, _, _ = make_encoder(2)
    loader = torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"), batch_size=2, shuffle=False)
    beam = dict(beam_size=6, num_beam_groups=G, diversity_penalty=0.5, return_groups=True, no_repeat_ngram_size=2)
    out, npz = str(tmp_path / "div.csv"), str(tmp_path / "div_attn.npz")
    caps, seqs = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=out, beam=beam, attention_out=npz)
    df = pd.read_csv(out, keep_default_na=False)
    assert list(df.columns) == ["image", "group", "generated_caption"] and len(caps) == 5 * G
    assert df["image"].tolist() == [i for i in range(5) for _ in range(G)] and df["group"].tolist() == [0, 1, 2] * 5
    assert df["generated_caption"].tolist() == caps
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
    plain = dict(beam)
    plain.pop("return_groups")
    caps1, _ = ev.evaluate(enc, dec, loader, wm, max_caption_len=max_len, out_csv=out, beam=plain)
    assert len(caps1) == 5 and list(pd.read_csv(out, keep_default_na=False).columns) == ["generated_caption"]
