"""CPU restatement of diverse beam search (predict_beam(num_beam_groups, diversity_penalty)) on the
oracle's scores, recomputing every step as predict_beam_rules in tests/beam_rules_ref.py does, with the decoding rules
included.  Every group's hypotheses and their unpenalised keys are returned, so that the device can be compared group
by group.  The selection of one step, diverse_step(), works on given log-probability rows, so that small examples can
be checked by hand."""
import torch

from oracle import restatement as R
from beam_rules_ref import banned_set, key, lp_table, step_logp


def diverse_step(hyps, rows, i, groups, lam, lp, end, bans=None):
    """One step of diverse beam search.  hyps: beam_size slots (dict(seq, score, fin, L) or None), group g owning slots
    g*k_g .. (g+1)*k_g - 1; rows: {slot: fp32 log-probability row} of every live slot; end: the <end> column; bans:
    {slot: set of banned columns}.  The groups choose in order; a live candidate (slot j, column w) of group g is ranked
    by its fp32 key minus lam * (the number of slots of groups 0 .. g-1 expanded with w at this step), an fp32 product
    and difference as on the device; an ended hypothesis by its key as it is.  Ties: lower slot, lower column.  Returns
    the new slots, group-major, each group's in the order they were chosen."""
    beam = len(hyps)
    kg = beam // groups
    new, expanded = [], []
    for g in range(groups):
        cands = []
        for j in range(g * kg, (g + 1) * kg):
            h = hyps[j]
            if h is None:
                continue
            if h["fin"]:
                cands.append((key(h["score"], h["L"], lp), j, 0, None))
                continue
            logp = rows[j]
            s = (torch.tensor(h["score"], dtype=torch.float64) + logp.double()).float()     # fp32 summed log-prob
            kv = s / lp[i + 1]
            cnt = torch.zeros(logp.numel(), dtype=torch.float32)
            for w in expanded:
                cnt[w] += 1
            pk = kv - torch.tensor(lam, dtype=torch.float32) * cnt
            ban = (bans or {}).get(j, set())
            if ban:
                pk[list(ban)] = float("-inf")
            order = torch.sort(pk, descending=True, stable=True).indices[:kg]        # ties: the lower column
            for w in order.tolist():
                if pk[w].item() == float("-inf"):
                    continue
                cands.append((pk[w].item(), j, w, h["score"] + float(logp[w])))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        for _, j, w, s in cands[:kg]:
            h = hyps[j]
            if h["fin"]:
                new.append(dict(h, seq=list(h["seq"])))
            else:
                new.append(dict(seq=h["seq"] + [w], score=s, fin=w == end, L=i + 1))
                expanded.append(w)
        new += [None] * (kg - len(cands[:kg]))
    return new


@torch.no_grad()
def predict_diverse_beam(cfg, P, enc_out, max_pred_len, entities, facts=None, beam_size=6, num_beam_groups=3,
                         diversity_penalty=0.5, length_penalty=0.0, no_repeat_ngram_size=0, min_len=0):
    """enc_out (1, d, 196) -> (best sequence LongTensor (max_pred_len,), its summed log-probability, its key,
    groups): groups[g] = [(seq, score, length, key)] of group g's final hypotheses in slot order, key the unpenalised
    ranking key score / lp[length].  The best is the best key over all slots (ties: the lower slot)."""
    assert enc_out.shape[0] == 1 and beam_size % num_beam_groups == 0
    K = entities.shape[1]
    ee = R.entity_encode(cfg, P, entities, facts)
    fe = R.fact_encode(P, facts, ee) if cfg.has_facts else None
    mem = R.build_memory(cfg, P, enc_out, ee, fe)
    pe = R.pe_table(max_pred_len, cfg.emb_dim).unsqueeze(0)
    lp = lp_table(length_penalty, max_pred_len)
    kg = beam_size // num_beam_groups
    hyps = [dict(seq=[], score=0.0, fin=False, L=0) if j % kg == 0 else None for j in range(beam_size)]
    for i in range(max_pred_len):
        rows, bans = {}, {}
        for j, h in enumerate(hyps):
            if h is not None and not h["fin"]:
                rows[j] = step_logp(cfg, P, ee, fe, mem, pe, facts, K, h["seq"], i, max_pred_len)
                bans[j] = banned_set(h["seq"], i, no_repeat_ngram_size, min_len, cfg.end)
        hyps = diverse_step(hyps, rows, i, num_beam_groups, diversity_penalty, lp, cfg.end, bans)
        if all(h is None or h["fin"] for h in hyps):
            break
    keys = [float("-inf") if h is None else key(h["score"], h["L"], lp) for h in hyps]
    best = max(range(beam_size), key=lambda q: (keys[q], -q))
    seq = hyps[best]["seq"] + [cfg.pad] * (max_pred_len - len(hyps[best]["seq"]))
    groups = [[None if hyps[j] is None else (hyps[j]["seq"], hyps[j]["score"], hyps[j]["L"], keys[j])
               for j in range(g * kg, (g + 1) * kg)] for g in range(num_beam_groups)]
    return torch.tensor(seq[:max_pred_len], dtype=torch.long), hyps[best]["score"], keys[best], groups


def group_best(group):
    """Index in its group of the best hypothesis by the unpenalised key (ties: the lower slot)."""
    keys = [float("-inf") if h is None else h[3] for h in group]
    return max(range(len(group)), key=lambda q: (keys[q], -q))
