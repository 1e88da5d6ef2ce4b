"""tests/context_ref.py (the float64 references of the context, embedding and pointer kernels) against the oracle
restatement on in-range inputs, against the real reference's own indicators and pointer scores (the score_head_*
fixtures), and -- where the restatement has no answer, the clamping contract -- against rows written out by hand.  Also:
the case table (tests/context_cases.py) reaches every hand-placed index it promises and stays inside the kernels'
limits."""
import math

import numpy as np
import pytest
import torch

import context_ref as CR
import ick_amd.synth as synth
from context_cases import (BIG, BIG_INDEX, CAPTION_LABELS, ENTITY_LABELS, FACT_LABELS, GATE, GATE_BWD_REJECTED, GATHER,
                           INDICATORS_REJECTED, NTYPES, POINTER, POINTER_BWD_REJECTED, V, gate_inputs, gather_inputs)
from helpers import load_golden, t
from oracle import restatement as R


def _case(variant, B=3, L=9, K=6, Vv=40, Fn=7, seed=5):
    P = synth.make_params(variant, Vv, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(Vv))
    batch = synth.make_batch(variant, B, L, K, Vv, 0 if variant == "geo" else Fn, seed)
    return P, cfg, batch


@pytest.mark.parametrize("variant", synth.VARIANTS)
def test_in_range_inputs_equal_the_restatement(variant):
    P, cfg, batch = _case(variant)
    Vv, d = cfg.vocab_size, 300
    facts = batch.get("facts")
    with torch.no_grad():
        ee_r = R.entity_encode(cfg, P, batch["entities"], facts)
    ee = CR.entity_encode(variant, batch["entities"], P["entity_encoder.type_embedding.weight"], d, facts,
                          P["word_embedding.weight"] if variant == "news" else None)
    if variant == "news":       # the restatement multiplies in float32
        assert (ee - ee_r.double()).abs().max().item() < 1e-7
    else:
        assert torch.equal(ee.float(), ee_r)
    fe = fe_r = None
    if variant != "geo":
        fe_r = R.fact_encode(P, facts, ee_r)
        fe = CR.fact_encode(facts, ee_r, P["predicate_embedding.weight"])
        assert torch.equal(fe.float(), fe_r)
    emb_r = R.caption_embed(cfg, P, batch["captions"], batch["caption_masks"], ee_r, fe_r)
    pe = R.pe_table(32, d)
    x, emb = CR.caption_embed(batch["captions"], batch["caption_masks"], P["word_embedding.weight"], ee_r, fe_r, pe, Vv,
                              cfg.pad, math.sqrt(d), pos0=2, round32=True)
    assert torch.equal(emb.float(), emb_r)
    assert torch.equal(x.float(), emb_r * math.sqrt(d) + pe[2:2 + emb_r.shape[1]].unsqueeze(0))
    if variant == "geo":
        return
    K = batch["entities"].shape[1]
    for mode, ol in ((0, batch["captions"].shape[1]), (1, 1)):
        eib_r, pi_r = R.context_indicators(cfg, batch["captions"], facts, K, ol)
        eib, gate, pi = CR.context_indicators(batch["captions"], facts, K, Vv, P["fc_predicate.weight"],
                                              P["fc_predicate.bias"], mode)
        assert torch.equal(eib.float(), eib_r) and torch.equal(pi.float(), pi_r)
        gate_r = torch.nn.functional.linear(pi_r.double(), P["fc_predicate.weight"].double(),
                                            P["fc_predicate.bias"].double())
        assert (gate - gate_r).abs().max().item() < 1e-12
    assert eib_r.sum() > 0


@pytest.mark.parametrize("name", ["score_head_geo", "score_head_knowledge", "score_head_news"])
def test_reproduces_the_reference_score_head(name):
    """The real reference's get_context_indicators / pointer columns of get_scores."""
    g = load_golden(name)
    variant = str(g["variant"])
    B, L, K, Vv, Fn, seed = (int(g[k]) for k in ("B", "L", "K", "V", "F", "seed"))
    P = synth.make_params(variant, Vv, seed)
    h, ee = t(g["h"]).permute(1, 0, 2), t(g["ee"])
    ref = t(g["scores"]).permute(1, 0, 2).double()
    ent = CR.pointer_scores(h, ee, P["fc_entity.weight"], P["fc_entity.bias"])
    assert (ent - ref[:, :, Vv:Vv + K]).abs().max().item() < 1e-5
    if variant == "geo":
        return
    batch = synth.make_batch(variant, B, L, K, Vv, Fn, seed)
    batch["facts"][:, :, 2] %= 3
    num_pred = synth.NUM_PREDICATES[variant]
    full = CR.indicator_tables(batch["captions"], batch["facts"], K, Vv, num_pred, 0)
    one = CR.indicator_tables(batch["captions"], batch["facts"], K, Vv, num_pred, 1)
    for tag, (eib, pi) in (("full", full), ("short", (full[0][:, :L - 3], full[1][:, :L - 3])), ("one", one)):
        assert torch.equal(eib.float(), t(g["eib_" + tag]).float().squeeze(3)), tag
        pi_ref = t(np.unpackbits(g["pi_" + tag], axis=2)[:, :, :num_pred]).float().squeeze(3)
        assert torch.equal(pi.float(), pi_ref), tag
    fact = CR.pointer_scores(h, t(g["fe"]), P["fc_fact.weight"], P["fc_fact.bias"], full[0])
    assert (fact - ref[:, :, Vv + K:]).abs().max().item() < 1e-5


def test_clamping_contract_by_hand():
    d = 8
    # ---- entity type and name words
    type_emb = torch.arange(3 * 3, dtype=torch.float64).view(3, 3) + 1.0           # news: d - 5 = 3 columns
    word_emb = (torch.arange(4 * d, dtype=torch.float64).view(4, d) + 1.0) / 8.0
    ent = torch.zeros(1, 4, 10)
    ent[0, :, 1], ent[0, :, 2], ent[0, :, 3] = 2.0, 1.0, 1.0
    ent[0, :, 4] = torch.tensor([-3.0, 3.0, 2.7, 1.0])
    ent[0, 0, 5:] = torch.tensor([-1.0, 4.0, 1.0, 1.0, 1.0])       # -> rows 0, 3, 1, 1, 1
    ent[0, 1, 5:] = 2.0
    ent[0, 2, 5:] = 2.0
    ent[0, 3, 5:] = 2.0
    facts = torch.tensor([[[0, 0, 0], [1, BIG + 1, 0], [2, 3, 0], [3, 0, 1]]])    # counts: entity 0 -> 2, entity 3 (last) -> 0
    ee = CR.entity_encode("news", ent, type_emb, d, facts, word_emb)
    avg0 = (word_emb[0] + word_emb[3] + 3 * word_emb[1]) / 5.0
    row0 = torch.cat([torch.tensor([2.0, 1.0, 1.0, 2.0, 1.0], dtype=torch.float64), type_emb[0]]) * avg0
    assert torch.allclose(ee[0, 0], row0, rtol=0, atol=1e-15)
    for k, ty in ((1, 2), (2, 2), (3, 1)):
        row = torch.cat([torch.tensor([2.0, 1.0, 1.0, 0.0, 0.0], dtype=torch.float64), type_emb[ty]]) * word_emb[2]
        assert torch.allclose(ee[0, k], row, rtol=0, atol=1e-15), k
    # ---- fact subject / predicate: clamped in int64
    e = torch.arange(3 * d, dtype=torch.float64).view(1, 3, d)
    pred = 100.0 + torch.arange(2 * d, dtype=torch.float64).view(2, d)
    facts = torch.tensor([[[0, -1, -1], [1, 3, 2], [2, 2, 1], [3, BIG + 1, BIG + 2], [4, 1, 0]]])
    fe = CR.fact_encode(facts, e, pred)
    for j, (s, q) in enumerate([(0, 0), (2, 1), (2, 1), (2, 1), (1, 0)]):
        assert torch.equal(fe[0, j], e[0, s] + pred[q]), j
    # ---- caption tokens
    Vv, K, F = 4, 3, 5
    words = 1000.0 + torch.arange(Vv * d, dtype=torch.float64).view(Vv, d)
    fer = 500.0 + torch.arange(F * d, dtype=torch.float64).view(1, F, d)
    toks = [(2, 0, words[2]), (Vv, 1, e[0, 0]), (Vv + K - 1, 1, e[0, 2]), (Vv + K, 2, fer[0, 0]),
            (Vv + K + F - 1, 2, fer[0, 4]), (Vv + K + F + 5, 1, e[0, 2]), (Vv + K + F + 5, 2, fer[0, 4]),
            (Vv + K + F + 5, 0, words[0]), (-1, 0, words[0]), (-1, 1, e[0, 2]), (1, 1, e[0, 2]), (1, 2, fer[0, 4]),
            (Vv + 1, 3, words[0]), (3, 3, words[3])]
    caps = torch.tensor([[q[0] for q in toks]])
    masks = torch.tensor([[q[1] for q in toks]])
    pe = torch.zeros(32, d, dtype=torch.float64)
    _, emb = CR.caption_embed(caps, masks, words, e, fer, pe, Vv, 0, 1.0)
    for l, q in enumerate(toks):
        assert torch.equal(emb[0, l], q[2]), l
    _, emb = CR.caption_embed(caps, masks, words, e, None, pe, Vv, 0, 1.0)          # geo: mask 2 reads a word row
    assert torch.equal(emb[0, 3], words[0]) and torch.equal(emb[0, 11], words[1])
    # ---- indicators: out of range = not active, never clamped
    caps = torch.tensor([[9, Vv + 1, 9, Vv + 2]])
    facts = torch.tensor([[[0, 1, 0], [1, BIG + 1, 1], [2, 3, 1], [3, -1, 1], [4, 1, 2], [5, 1, BIG + 2], [6, 2, 0],
                           [7, 0, 1]]])
    eib, pi = CR.indicator_tables(caps, facts, K, Vv, 2, 0)
    assert eib[0].tolist() == [[0.0] * 8, [0.0] * 8, [1, 0, 0, 0, 1, 1, 0, 0], [1, 0, 0, 0, 1, 1, 0, 0]]
    assert pi[0].tolist() == [[0, 0], [0, 0], [1, 0], [1, 0]]      # entity 2, first named at L - 1, activates nothing
    eib, pi = CR.indicator_tables(caps, facts, K, Vv, 2, 1)
    assert eib[0].tolist() == [[1, 0, 0, 0, 1, 1, 1, 0]] and pi[0].tolist() == [[1, 0]]


def test_abs_evaluations_bound_the_values():
    g = torch.Generator().manual_seed(1)
    h, ctx = torch.randn(2, 3, 9, generator=g), torch.randn(2, 4, 9, generator=g)
    w, b = torch.randn(1, 9, generator=g), torch.randn(1, generator=g)
    ind = (torch.rand(2, 3, 4, generator=g) > 0.5).float()
    s, a = CR.pointer_scores(h, ctx, w, b, ind), CR.pointer_scores_abs(h, ctx, w, b, ind)
    assert (a - s.abs()).min().item() >= -1e-12
    expect = (h.double().abs().unsqueeze(2) * ctx.double().abs().unsqueeze(1) * w.double().abs().view(1, 1, 1, -1)).sum(-1) \
        * ind.double() + b.double().abs()
    assert torch.allclose(a, expect, rtol=1e-14, atol=0)
    up = torch.randn(2, 3, 4, generator=g)
    fn = lambda absval=False, **kw: CR.pointer_scores(kw["h"], kw["ctx"], CR.A(w, absval), CR.A(b, absval), ind, absval=absval)     # noqa: E731
    gr = CR.grads(fn, dict(h=h, ctx=ctx), up)
    ga = CR.grads(fn, dict(h=h, ctx=ctx), up, absval=True)
    assert all((ga[k] - gr[k].abs()).min().item() >= -1e-12 for k in gr)
    dh = ((up.double() * ind.double()).abs().unsqueeze(3) * ctx.double().abs().unsqueeze(1)).sum(2) * w.double().abs()
    assert torch.allclose(ga["h"], dh, rtol=1e-14, atol=0)


def test_case_table_reaches_what_it_promises():
    placed = set()
    for c in GATHER:
        batch, done = gather_inputs(c)
        placed |= done
        assert batch["captions"].shape == (c.B, c.L) and batch["entities"].shape[1] == c.K
        assert torch.isfinite(batch["entities"]).all()
    batch, done = gather_inputs(BIG_INDEX, big=True)
    assert {"subj_2^32+1", "pred_2^32+2"} <= done and (batch["facts"] > BIG).sum().item() == 2
    assert not any((gather_inputs(c)[0].get("facts", torch.zeros(1)) > BIG).any() for c in GATHER)
    for c in GATE:
        caps, facts, done = gate_inputs(c)
        placed |= done
        T = c.L if c.mode == 0 else 1
        assert (c.K + 5 * c.F + 1) * 4 <= 65536
        if c.bwd:
            assert (c.K + 3 * c.F) * 4 + T * 1024 <= 65536
    missing = (CAPTION_LABELS | ENTITY_LABELS | FACT_LABELS) - placed
    assert not missing, missing
    B, L, K, F, d = GATE_BWD_REJECTED
    assert (K + 3 * F) * 4 + L * 1024 > 65536 >= (K + 3 * F) * 4 + (L - 1) * 1024 and K + 3 * F <= 256
    B, L, K, F = INDICATORS_REJECTED
    assert (K + 5 * F + 1) * 4 > 65536 >= (K + 5 * (F - 1) + 1) * 4
    B, T, Kc, d = POINTER_BWD_REJECTED
    assert (T * Kc + 260) * 4 > 65536 >= (T * (Kc - 1) + 260) * 4
    for c in POINTER:
        assert (c.T * c.Kc + 260) * 4 <= 65536 and len(c.lengths) == c.B
    assert any(2 in c.lengths for c in POINTER)
    assert {c.Kc for c in POINTER} >= {1, 7, 8, 9, 16, 17, 71}
    assert {c.d for c in POINTER} >= {64, 300, 320, 321, 512, 513, 1024}
    for rows in (lambda c: c.B * c.L, lambda c: c.B * c.K, lambda c: c.B * c.F):
        assert {rows(c) for c in GATHER} >= {1, 3, 4, 5, 35}
    assert {c.K for c in GATHER} >= {1, 5, 20, 257} and {c.F for c in GATHER} >= {1, 3, 51, 65, 130, 257}
    assert {c.L for c in GATE if c.bwd} >= {1, 2, 20, 63}
    assert NTYPES["news"] < NTYPES["geo"] and V > 8
