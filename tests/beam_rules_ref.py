"""CPU restatement of the decoding rules of predict_beam / predict_sample, built on the public
functions of oracle/restatement.py: the banned set of a step, the GNMT length-penalty table and a beam search that
applies all three rules (full recompute per step, as R.predict_beam).  With every rule off the beam search is
R.predict_beam."""
import math

import torch

from oracle import restatement as R

import ick_amd.decoder as D


def banned_set(seq, t, n, m, end):
    """The tokens banned at step t for a row whose generated tokens are seq[0..t-1]: the no-repeat n-gram rule
    (n > 0: every seq[p], n-1 <= p <= t-1, with seq[p-n+1..p-1] == seq[t-n+1..t-1]) and the min-length rule (<end>
    while t < m)."""
    ban = set()
    if n > 0:
        tail = list(seq[t - n + 1:t]) if n > 1 else []
        for p in range(n - 1, t):
            if list(seq[p - n + 1:p]) == tail:
                ban.add(int(seq[p]))
    if t < m:
        ban.add(end)
    return ban


def banned_brute(seq, t, n, m, end):
    """The same set by enumerating every n-gram of seq[0..t-1] and every candidate continuation."""
    ban = set()
    if n > 0 and t >= n - 1:
        grams = {tuple(seq[q:q + n]) for q in range(0, t - n + 1)}
        prefix = tuple(seq[t - n + 1:t]) if n > 1 else ()
        for g in grams:
            if g[:-1] == prefix:
                ban.add(int(g[-1]))
    if t < m:
        ban.add(end)
    return ban


def lp_table(alpha, max_len):
    """float32 lp[0..max_len], the device's table (lp[L] = ((5 + L) / 6) ** alpha in float64, rounded)."""
    return D.length_penalty_table(alpha, max_len)


def key(score, L, lp):
    """The fp32 ranking key cum / lp[L]."""
    return float(torch.tensor(score, dtype=torch.float32) / lp[L])


def step_logp(cfg, P, ee, fe, mem, pe, facts, K, seq, i, max_len):
    V = cfg.vocab_size
    captions = [cfg.start] + seq + [cfg.start] * (max_len - 1 - len(seq))
    masks = [0] + [2 if (cfg.has_facts and t >= V + K) else (1 if t >= V else 0) for t in seq]
    masks = masks + [0] * (max_len - len(masks))
    cap_t = torch.tensor([captions[:max_len]])
    emb = R.caption_embed(cfg, P, cap_t, torch.tensor([masks[:max_len]]), ee, fe)
    hh = R.decoder_stack(cfg, P, emb * math.sqrt(cfg.emb_dim) + pe, mem)[:, i:i + 1]
    if cfg.has_facts:
        eib, pi = R.context_indicators(cfg, cap_t, facts, K, 1)
        sc = R.get_scores(cfg, P, hh, ee, fe, eib, pi)
    else:
        sc = R.get_scores(cfg, P, hh, ee)
    return sc[0, 0].log_softmax(dim=-1)


@torch.no_grad()
def predict_beam_rules(cfg, P, enc_out, max_pred_len, entities, facts=None, beam_size=5, length_penalty=0.0,
                       no_repeat_ngram_size=0, min_len=0):
    """enc_out (1, d, 196) -> (best sequence LongTensor (max_pred_len,), its summed log-probability, its key,
    all [(seq, score, length)]).  Candidates are ranked by (key desc, hypothesis asc, token asc), key = score /
    lp[L] with L = i + 1 for a live expansion at step i and the ended length for an ended hypothesis."""
    assert enc_out.shape[0] == 1
    K = entities.shape[1]
    ee = R.entity_encode(cfg, P, entities, facts)
    fe = R.fact_encode(P, facts, ee) if cfg.has_facts else None
    mem = R.build_memory(cfg, P, enc_out, ee, fe)
    pe = R.pe_table(max_pred_len, cfg.emb_dim).unsqueeze(0)
    lp = lp_table(length_penalty, max_pred_len)
    hyps = [dict(seq=[], score=0.0, fin=False, L=0)] + [None] * (beam_size - 1)
    for i in range(max_pred_len):
        cands = []
        for j, h in enumerate(hyps):
            if h is None:
                continue
            if h["fin"]:
                cands.append((key(h["score"], h["L"], lp), j, 0, h["score"]))
                continue
            logp = step_logp(cfg, P, ee, fe, mem, pe, facts, K, h["seq"], i, max_pred_len)
            ban = banned_set(h["seq"], i, no_repeat_ngram_size, min_len, cfg.end)
            masked = logp.clone()
            if ban:
                masked[list(ban)] = float("-inf")
            top = masked.topk(min(beam_size, masked.numel()))
            for v, idx in zip(top.values.tolist(), top.indices.tolist()):
                if idx in ban:
                    continue
                s = h["score"] + v
                cands.append((key(s, i + 1, lp), j, idx, s))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        new = []
        for _, j, tok, s in cands[:beam_size]:
            h = hyps[j]
            if h["fin"]:
                new.append(dict(h, seq=list(h["seq"])))
            else:
                new.append(dict(seq=h["seq"] + [tok], score=s, fin=tok == cfg.end, L=i + 1))
        hyps = new + [None] * (beam_size - len(new))
        if all(h is None or h["fin"] for h in hyps):
            break
    live = [h for h in hyps if h is not None]
    keys = [key(h["score"], h["L"], lp) for h in live]
    best = max(range(len(live)), key=lambda q: (keys[q], -q))
    seq = live[best]["seq"] + [cfg.pad] * (max_pred_len - len(live[best]["seq"]))
    return (torch.tensor(seq[:max_pred_len], dtype=torch.long), live[best]["score"], keys[best],
            [(h["seq"], h["score"], h["L"]) for h in live])


def has_banned_ngram(seq, n, m, end):
    """First step at which seq (generated tokens, <end> included) breaks a rule, or None."""
    for t, tok in enumerate(seq):
        if tok in banned_set(seq, t, n, m, end):
            return t
        if tok == end:
            break
    return None
