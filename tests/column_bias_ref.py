"""float64 references of the column bias of beam search and sampling (csrc/decode_select.hip and
csrc/sample.hip, the BIASED instantiations).  They extend the references the suite already has without editing them:

  beam_step / sample_step    one selection step on hand-built rows, as select_ref.beam_step / sample_step, with the same
                             MARGIN and Undecidable discipline
  predict_beam_bias          a whole CPU beam search with rules and bias on the oracle's scores, as
                             beam_rules_ref.predict_beam_rules
  draw                       sample_ref.kept_set / draw on s + b

The semantics, from the issue: hypothesis j expanded with column w ranks by (cum_j - lse_j + s_w + bsum_j + b_w), an
ended one by cum_j + bsum_j, each over its own lp[L]; lse runs over the raw scores and cum stays raw; a column with
b = -inf leaves the pool like a banned one, and a rule ban wins over any bias.  Sampling selects on s' = s + b (top-k,
z, the top-p weights and their maximum, the Gumbel arg-max); log_prob stays log_softmax(s)[token]."""
import numpy as np
import torch

import sample_ref
from beam_rules_ref import banned_set, key as lp_key, lp_table, step_logp
from select_ref import MARGIN, NEG, Undecidable, _check_window, _ranked, _window, embed, lse64, token_kind

BIAS_MAX = 64


def bias_row(Vx, cols, vals):
    """The (Vx,) float64 bias of one caption from its slots: -1 = an empty slot, and of two slots holding one id the
    lowest counts (the raw ABI's rule; the Python front end refuses such a list)."""
    b = np.zeros(Vx)
    seen = set()
    for c, v in zip(cols, vals):
        c = int(c)
        if c < 0 or c in seen:
            continue
        seen.add(c)
        b[c] = float(v)
    return b


# ------------------------------------------------------------------------------------------------------------ beam
def beam_step(case, st, rows, pos, tables):
    """select_ref.beam_step for the plain form with a column bias.  case: column_bias_cases.BiasBeamCase (bias_cols,
    bias_vals: (B, <= 64) slots); st also holds bsum (float64, (R)).  Returns (state out, info) with the same fields, the
    state also holding bsum."""
    k, V, K, F, Vx = case.beam, case.V, case.K, case.F, case.Vx
    R, L, end = case.R, case.max_len, case.end
    ngram, min_len, alpha = case.rules if case.rules else (0, 0, 0.0)
    lp_on = case.rules is not None and alpha != 0
    lp = lp_table(alpha, L).double().numpy() if case.rules else None
    live_all = [r for r in range(R) if not st["fin"][r] and st["cum"][r] != NEG]
    if sorted(rows) != live_all:
        raise AssertionError("score rows %s given for live rows %s" % (sorted(rows), live_all))
    out = {n: st[n].copy() for n in ("cum", "fin", "len", "met", "seq", "anc", "bsum")}
    out["cap"] = None if st["cap"] is None else st["cap"].copy()
    out["n_done"] = st["n_done"]
    info = dict(next_token=np.zeros(R, np.int64), next_mask=np.zeros(R, np.int64), x0=np.zeros((R, case.d), np.float32),
                x0_written=np.zeros(R, bool), dead=np.zeros(R, bool), parent=np.zeros(R, np.int64),
                tok=np.full(R, -1, np.int64), carried=[], banned={}, picks=[], unbiased_picks=[])
    for b in range(case.B):
        r0 = b * k
        if not any((r0 + j) in rows for j in range(k)):
            info["carried"].append(b)
            continue
        bias = bias_row(Vx, case.bias_cols[b], case.bias_vals[b])
        key, raw_key, slot, col, ncum, nbsum, sig_of_slot = [], [], [], [], [], [], {}
        for j in range(k):
            r = r0 + j
            cum, bs = st["cum"][r], st["bsum"][r]
            if cum == NEG:
                continue
            if st["fin"][r]:
                kv = cum + bs
                key.append(np.array([kv / lp[st["len"][r]] if lp_on else kv]))
                raw_key.append(np.array([cum / lp[st["len"][r]] if lp_on else cum]))
                slot.append(np.array([j])); col.append(np.array([0])); ncum.append(np.array([cum])); nbsum.append(np.array([bs]))
                sig_of_slot[j] = [("ended", cum, bs, int(st["len"][r]) if lp_on else 0)]
                continue
            x = np.asarray(rows[r])
            assert x.dtype == np.float32 and x.shape == (Vx,) and np.isfinite(x).all() and np.abs(x).max() <= 16
            s = cum + (x.astype(np.float64) - lse64(x))
            with np.errstate(invalid="ignore"):
                kv = s + bs + bias
            rk = s.copy()
            if lp_on:
                kv, rk = kv / lp[pos + 1], rk / lp[pos + 1]
            ban = banned_set([int(t) for t in st["seq"][r, :pos]], pos, ngram, min_len, end) if case.rules else set()
            info["banned"][r] = ban
            if ban:
                kv[sorted(ban)] = NEG               # the ban wins over any bias
                rk[sorted(ban)] = NEG
            key.append(kv); raw_key.append(rk); slot.append(np.full(Vx, j)); col.append(np.arange(Vx)); ncum.append(s)
            nbsum.append(bs + np.where(np.isfinite(bias), bias, 0.0))
            sig_of_slot[j] = (cum, bs, x.tobytes(), x)
        key, raw_key, slot, col, ncum, nbsum = (np.concatenate(a) for a in (key, raw_key, slot, col, ncum, nbsum))

        def signature(i):
            s_ = sig_of_slot[int(slot[i])]
            if isinstance(s_, list):
                return s_[0]
            return ("live", s_[0], s_[1], s_[2], float(s_[3][col[i]]), float(bias[col[i]]))

        o = _ranked(key, slot, col)
        lim = _window(key[o], k)
        tl = [(float(key[i]), int(slot[i]), int(col[i]), signature(i), int(i)) for i in o[:lim]]
        _check_window(tl, k, "%s step %d caption %d" % (case.name, pos, b))
        got = [t[4] for t in tl[:k]]
        picks = got + [None] * (k - len(got))
        ro = _ranked(raw_key, slot, col)[:k]
        info["unbiased_picks"].append([(int(slot[i]), int(col[i])) for i in ro])
        before = sum(1 for j in range(k) if st["fin"][r0 + j] or st["cum"][r0 + j] == NEG)
        after = 0
        for h, i in enumerate(picks):
            r = r0 + h
            info["x0_written"][r] = pos + 1 < L
            if i is None:                                # fewer candidates than beams: a dead slot
                info["dead"][r] = True
                out["cum"][r], out["fin"][r], out["bsum"][r] = NEG, 1, 0.0
                if lp_on:
                    out["len"][r] = 0
                after += 1
                tok_in = 0
            else:
                j, c = int(slot[i]), int(col[i])
                src = r0 + j
                info["parent"][r] = j
                out["cum"][r], out["bsum"][r] = ncum[i], nbsum[i]
                out["seq"][r] = st["seq"][src]
                out["anc"][r] = st["anc"][src]
                if out["cap"] is not None:
                    out["cap"][r] = st["cap"][src]
                if st["fin"][src]:                       # an ended hypothesis is carried as it is, with its sum
                    out["fin"][r] = 1
                    if lp_on:
                        out["len"][r] = st["len"][src]
                    after += 1
                    tok_in = 0
                    if out["cap"] is not None:
                        out["cap"][r, pos + 1:] = case.start
                else:
                    info["tok"][r] = c
                    out["fin"][r] = int(c == end)
                    if lp_on:
                        out["len"][r] = pos + 1
                    out["seq"][r, pos] = c
                    out["seq"][r, pos + 1:] = case.pad
                    after += int(c == end)
                    tok_in = 0 if c == end else c
                    if out["cap"] is not None:
                        out["cap"][r, pos + 1:] = case.start
                        if pos + 1 < L and c != end:
                            out["cap"][r, pos + 1] = c
                out["anc"][r, pos] = src
                out["anc"][r, pos + 1:] = 0
            kind = token_kind(tok_in, V, K, F)
            info["next_token"][r], info["next_mask"][r] = tok_in, kind
            if pos + 1 < L:
                info["x0"][r] = embed(tables, tok_in, kind, b, pos + 1, V, K)
        out["n_done"] += after - before
        info["picks"].append([None if i is None else (int(slot[i]), int(col[i]), float(key[i])) for i in picks])
    return out, info


# -------------------------------------------------------------------------------------------------------- sampling
def draw(s, b, T, top_k, top_p, g, ban=()):
    """sample_ref.draw on s' = s + b (fp32, as the kernel adds them) over the allowed columns: those neither in `ban` nor
    biased with -inf.  g: the row's Gumbel noise by column.  Returns (token, kept mask over all columns, the sorted
    perturbed values of the kept set, the top-p ratio of every allowed column, the allowed columns)."""
    s = np.asarray(s, dtype=np.float32)
    b = np.asarray(b, dtype=np.float64)
    sp = np.where(np.isfinite(b), s + b.astype(np.float32), np.float32(NEG)).astype(np.float32)
    allowed = np.isfinite(b)
    allowed[sorted(ban)] = False
    cols = np.nonzero(allowed)[0]
    w, keep_a, vals, ratio = sample_ref.draw(sp[cols], T, top_k, top_p, np.asarray(g)[cols])
    keep = np.zeros(s.size, bool)
    keep[cols[keep_a]] = True
    return int(cols[w]), keep, vals, ratio, cols


def sample_step(case, st, rows, pos, tables):
    """select_ref.sample_step with a column bias.  case: column_bias_cases.BiasSampleCase (bias_cols, bias_vals)."""
    V, K, F, Vx, R, L, end = case.V, case.K, case.F, case.Vx, case.R, case.max_len, case.end
    out = {n: st[n].copy() for n in ("output", "finished", "log_prob")}
    out["cap_buf"] = None if st["cap_buf"] is None else st["cap_buf"].copy()
    out["n_done"] = st["n_done"]
    info = dict(next_token=np.zeros(R, np.int64), next_mask=np.zeros(R, np.int64), x0=np.zeros((R, case.d), np.float32),
                written=st["n_done"] < R, tok={}, kept={}, kept_unbiased={}, banned={}, smax={}, allowed={})
    if not info["written"]:
        return out, info
    live = [r for r in range(R) if not st["finished"][r]]
    if sorted(rows) != live:
        raise AssertionError("score rows %s given for live rows %s" % (sorted(rows), live))
    ngram, min_len = case.rules if case.rules else (0, 0)
    T, top_k, top_p = np.float32(case.T), case.top_k, np.float32(case.top_p)
    for r in range(R):
        b, j = divmod(r, case.rps)
        tok_in = 0
        if not st["finished"][r]:
            s = np.asarray(rows[r])
            assert s.dtype == np.float32 and s.shape == (Vx,) and np.isfinite(s).all() and np.abs(s).max() <= 16
            bias = bias_row(Vx, case.bias_cols[b], case.bias_vals[b])
            ban = banned_set([int(t) for t in st["output"][r, :pos]], pos, ngram, min_len, end) if case.rules else set()
            g = sample_ref.gumbel(case.seed, b, j, pos, Vx)
            tok, keep, top, ratio, cols = draw(s, bias, T, top_k, float(top_p), g, ban)
            sa = (s[cols] + bias[cols].astype(np.float32)).astype(np.float32)
            if 0 < top_k < sa.size:
                thr = np.sort(sa)[::-1][top_k - 1]
                gap = np.abs(sa.astype(np.float64) - float(thr))
                if ((gap > 0) & (gap < MARGIN)).any():
                    raise Undecidable("%s row %d: a score %.3g from the top-k threshold" % (case.name, r, gap[gap > 0].min()))
            if top_p < 1 and (np.abs(ratio) < MARGIN).any():
                raise Undecidable("%s row %d: strictly-greater mass %.3g of W from p" % (case.name, r, np.abs(ratio).min()))
            if len(top) > 1 and top[0] - top[1] < MARGIN:
                raise Undecidable("%s row %d: best two perturbed values %.3g apart" % (case.name, r, top[0] - top[1]))
            _, keep0, _, _, _ = draw(s, np.zeros(Vx), T, top_k, float(top_p), g, ban)
            info["tok"][r], info["kept"][r], info["kept_unbiased"][r] = tok, keep, keep0
            info["banned"][r], info["smax"][r], info["allowed"][r] = ban, int(np.argmax(s)), cols
            out["output"][r, pos] = tok
            out["log_prob"][r, pos] = float(s[tok]) - lse64(s)          # the model's: raw scores
            if tok == end:
                out["finished"][r] = 1
                out["n_done"] += 1
            else:
                tok_in = tok
        kind = token_kind(tok_in, V, K, F)
        info["next_token"][r], info["next_mask"][r] = tok_in, kind
        if pos + 1 < L:
            if out["cap_buf"] is not None:
                out["cap_buf"][r, pos + 1] = tok_in
            info["x0"][r] = embed(tables, tok_in, kind, b, pos + 1, V, K)
    return out, info


# ------------------------------------------------------------------------------------------- whole CPU beam search
@torch.no_grad()
def predict_beam_bias(cfg, P, enc_out, max_pred_len, entities, facts=None, beam_size=5, length_penalty=0.0,
                      no_repeat_ngram_size=0, min_len=0, bias=None):
    """beam_rules_ref.predict_beam_rules with a column bias.  bias: a (Vx,) float64 vector (bias_row) or None.  Returns
    (best sequence LongTensor (max_pred_len,), its summed log-probability, its key, all [(seq, score, length, bsum)],
    margin): margin is the smallest gap, over all steps and the final choice, between the last candidate taken and the
    first one left (inf when nothing was left) -- the decisions are the device's wherever it clears the tolerance."""
    from oracle import restatement as R
    assert enc_out.shape[0] == 1
    K = entities.shape[1]
    ee = R.entity_encode(cfg, P, entities, facts)
    fe = R.fact_encode(P, facts, ee) if cfg.has_facts else None
    mem = R.build_memory(cfg, P, enc_out, ee, fe)
    pe = R.pe_table(max_pred_len, cfg.emb_dim).unsqueeze(0)
    lp = lp_table(length_penalty, max_pred_len)
    hyps = [dict(seq=[], score=0.0, fin=False, L=0, bsum=0.0)] + [None] * (beam_size - 1)
    margin = float("inf")
    for i in range(max_pred_len):
        cands = []
        for j, h in enumerate(hyps):
            if h is None:
                continue
            if h["fin"]:
                cands.append((lp_key(h["score"] + h["bsum"], h["L"], lp), j, 0, h["score"], h["bsum"]))
                continue
            logp = step_logp(cfg, P, ee, fe, mem, pe, facts, K, h["seq"], i, max_pred_len).double()
            bvec = torch.zeros_like(logp) if bias is None else torch.from_numpy(np.asarray(bias, dtype=np.float64))
            ban = banned_set(h["seq"], i, no_repeat_ngram_size, min_len, cfg.end)
            masked = logp + bvec
            if ban:
                masked[list(ban)] = float("-inf")
            top = masked.topk(min(beam_size + 1, masked.numel()))
            for v, idx in zip(top.values.tolist(), top.indices.tolist()):
                if v == float("-inf"):
                    continue
                s = h["score"] + float(logp[idx])
                bs = h["bsum"] + float(bvec[idx])
                cands.append((lp_key(s + bs, i + 1, lp), j, idx, s, bs))
        cands.sort(key=lambda c: (-c[0], c[1], c[2]))
        if len(cands) > beam_size:
            margin = min(margin, cands[beam_size - 1][0] - cands[beam_size][0])
        for a, b in zip(cands[:beam_size], cands[1:beam_size]):
            margin = min(margin, a[0] - b[0])           # the order of the winners decides their slots
        new = []
        for _, j, tok, s, bs in cands[:beam_size]:
            h = hyps[j]
            if h["fin"]:
                new.append(dict(h, seq=list(h["seq"])))
            else:
                new.append(dict(seq=h["seq"] + [tok], score=s, fin=tok == cfg.end, L=i + 1, bsum=bs))
        hyps = new + [None] * (beam_size - len(new))
        if all(h is None or h["fin"] for h in hyps):
            break
    live = [h for h in hyps if h is not None]
    keys = [lp_key(h["score"] + h["bsum"], h["L"], lp) for h in live]
    best = max(range(len(live)), key=lambda q: (keys[q], -q))
    ks = sorted(keys, reverse=True)
    if len(ks) > 1:
        margin = min(margin, ks[0] - ks[1])
    seq = live[best]["seq"] + [cfg.pad] * (max_pred_len - len(live[best]["seq"]))
    return (torch.tensor(seq[:max_pred_len], dtype=torch.long), live[best]["score"], keys[best],
            [(h["seq"], h["score"], h["L"], h["bsum"]) for h in live], margin)
