"""CPU restatement of constrained beam search (predict_beam(force_tokens)) on the oracle's scores,
recomputing every step as predict_beam_rules in tests/beam_rules_ref.py does, with the decoding rules included.  It is
dynamic beam allocation (Post & Vilar, NAACL 2018) for single-column constraints.  Every column of every live row is
ranked: nothing here leans on the device's argument that the k best columns of a 1024-column chunk suffice.  The
selection of one step, constrained_step(), works on given log-probability rows, so that small examples can be checked
by hand."""
import torch

from oracle import restatement as R
from beam_rules_ref import banned_set, key, lp_table, step_logp

import ick_amd.decoder as D

FORCE_MAX = D.FORCE_MAX         # slots per caption, the device's limit


def slots_of(force, w):
    """Bit mask of the slots of `force` (a list of column ids, -1 = empty) that hold column w."""
    m = 0
    for s, f in enumerate(force):
        if f >= 0 and f == w:
            m |= 1 << s
    return m


def bank_of(met):
    return bin(met).count("1")


def allocate(cands, n_req, beam):
    """Step 3 of §3.2g.  cands: (key, slot, column, bank, ...) tuples.  The banks n_req, n_req - 1, .., 0 are visited
    in turn and round again; each visit takes that bank's best remaining candidate (key descending, then the lower
    slot, then the lower column); empty banks are skipped.  Returns the candidates in the order they were taken."""
    banks = {}
    for c in cands:
        banks.setdefault(c[3], []).append(c)
    for b in banks:
        banks[b].sort(key=lambda c: (-c[0], c[1], c[2]))
    taken = []
    while len(taken) < beam and any(banks.values()):
        for b in range(n_req, -1, -1):
            if banks.get(b) and len(taken) < beam:
                taken.append(banks[b].pop(0))
    return taken


def constrained_step(hyps, rows, i, force, lp, end, bans=None):
    """One step.  hyps: beam slots (dict(seq, score, fin, L, met) or None); rows: {slot: fp32 log-probability row} of
    every live slot; force: the caption's forced columns (-1 = empty); bans: {slot: set of banned columns}.  A live
    hypothesis offers every column that is not banned, <end> only once all its slots are met; an ended hypothesis
    competes as it is.  Keys are fp32 (score + logp) / lp[i + 1] as on the device."""
    assert len(force) <= FORCE_MAX
    beam = len(hyps)
    n_req = sum(1 for f in force if f >= 0)
    cands = []
    for j, h in enumerate(hyps):
        if h is None:
            continue
        if h["fin"]:
            cands.append((key(h["score"], h["L"], lp), j, 0, bank_of(h["met"]), None, h["met"]))
            continue
        logp = rows[j]
        s = (torch.tensor(h["score"], dtype=torch.float64) + logp.double()).float()         # fp32 summed log-prob
        kv = s / lp[i + 1]
        closed = set((bans or {}).get(j, set()))
        if bank_of(h["met"]) < n_req:
            closed.add(end)
        if closed:
            kv[list(closed)] = float("-inf")
        newmet = torch.full((logp.numel(),), h["met"], dtype=torch.int64)
        for f in set(f for f in force if f >= 0):
            newmet[f] = h["met"] | slots_of(force, f)
        bank = torch.tensor([bank_of(m) for m in range(1 << FORCE_MAX)])[newmet]
        for b in bank.unique().tolist():                     # every column of the row, bank by bank
            cols = (bank == b).nonzero().flatten()
            order = torch.sort(kv[cols], descending=True, stable=True).indices[:beam]       # ties: the lower column
            for w in cols[order].tolist():
                if kv[w].item() == float("-inf"):
                    continue
                cands.append((kv[w].item(), j, w, b, h["score"] + float(logp[w]), int(newmet[w])))
    new = []
    for _, j, w, _, s, met in allocate(cands, n_req, beam):
        h = hyps[j]
        if h["fin"]:
            new.append(dict(h, seq=list(h["seq"])))
        else:
            new.append(dict(seq=h["seq"] + [w], score=s, fin=w == end, L=i + 1, met=met))
    return new + [None] * (beam - len(new))


def best_slot(hyps, lp):
    """Step 4: the best hypothesis by (bank, key), ties to the lower slot."""
    live = [q for q, h in enumerate(hyps) if h is not None]
    return max(live, key=lambda q: (bank_of(hyps[q]["met"]), key(hyps[q]["score"], hyps[q]["L"], lp), -q))


@torch.no_grad()
def predict_constrained_beam(cfg, P, enc_out, max_pred_len, entities, facts=None, beam_size=5, force=(),
                             length_penalty=0.0, no_repeat_ngram_size=0, min_len=0):
    """enc_out (1, d, 196), force: the caption's forced columns -> (best sequence LongTensor (max_pred_len,), its
    summed log-probability, its key, its bank, slots): slots[h] = (seq, score, length, key, bank) or None."""
    assert enc_out.shape[0] == 1
    force = [int(f) for f in force]
    K = entities.shape[1]
    ee = R.entity_encode(cfg, P, entities, facts)
    fe = R.fact_encode(P, facts, ee) if cfg.has_facts else None
    mem = R.build_memory(cfg, P, enc_out, ee, fe)
    pe = R.pe_table(max_pred_len, cfg.emb_dim).unsqueeze(0)
    lp = lp_table(length_penalty, max_pred_len)
    hyps = [dict(seq=[], score=0.0, fin=False, L=0, met=0)] + [None] * (beam_size - 1)
    for i in range(max_pred_len):
        rows, bans = {}, {}
        for j, h in enumerate(hyps):
            if h is not None and not h["fin"]:
                rows[j] = step_logp(cfg, P, ee, fe, mem, pe, facts, K, h["seq"], i, max_pred_len)
                bans[j] = banned_set(h["seq"], i, no_repeat_ngram_size, min_len, cfg.end)
        hyps = constrained_step(hyps, rows, i, force, lp, cfg.end, bans)
        if all(h is None or h["fin"] for h in hyps):
            break
    best = best_slot(hyps, lp)
    seq = hyps[best]["seq"] + [cfg.pad] * (max_pred_len - len(hyps[best]["seq"]))
    slots = [None if h is None else (h["seq"], h["score"], h["L"], key(h["score"], h["L"], lp), bank_of(h["met"]))
             for h in hyps]
    return (torch.tensor(seq[:max_pred_len], dtype=torch.long), hyps[best]["score"], slots[best][3], slots[best][4],
            slots)
