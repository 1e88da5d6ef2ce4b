"""float64 step references of the beam and sampled token selection (csrc/decode_select.hip: dec_beam_partial_kernel +
dec_select_beam_kernel, plain / rules / diverse / forced; csrc/sample.hip: dec_sample_kernel), from the RAW score rows
of one step and the state going in.  Every column of every live row is ranked: nothing is taken from the device's
argument that the k best columns of a 1024-column chunk suffice.

Decidability is the references' business.  Two candidates that compete for a slot are either an intended tie (the same
cum, score rows that are copies of one another and the same raw score: the device's keys are then the same bits whatever
its rounding) or at least MARGIN apart in float64; the same bar holds for the two best perturbed values of a draw, for
every score against the top-k threshold and for every column's strictly-greater mass against p * W (relative to W).
Anything in between raises Undecidable: no step is ever excused."""
import numpy as np

from beam_rules_ref import banned_set, lp_table
from constrained_beam_ref import allocate, bank_of, slots_of
import sample_ref

MARGIN = 1e-2
NEG = float("-inf")


class Undecidable(AssertionError):
    pass


def token_kind(tok, V, K, F):
    return 2 if (F > 0 and tok >= V + K) else (1 if tok >= V else 0)


def embed(tables, tok, kind, b, pos, V, K):
    """x0 of token `tok` (kind: token_kind) of caption b as the input of position pos: fmaf(row, emb_scale, pe[pos]) --
    one rounding of the exact value, which float64 holds for the tables of select_cases.tables()."""
    row = tables["fe"][b, tok - V - K] if kind == 2 else tables["ee"][b, tok - V] if kind == 1 else tables["word_emb"][tok]
    return (row.astype(np.float64) * tables["emb_scale"] + tables["pe"][pos].astype(np.float64)).astype(np.float32)


def lse64(x):
    x = np.asarray(x, dtype=np.float64)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


# ------------------------------------------------------------------------------------------------------------ beam
def _window(keys, take):
    """How many of the candidates (keys descending) are winners or within MARGIN of the last winner."""
    if take == 0 or len(keys) == 0:
        return 0
    floor = keys[min(take, len(keys)) - 1] - MARGIN
    return int(np.searchsorted(-keys, -floor, side="left"))


def _check_window(cands, take, what):
    """cands: (key, slot, col, signature, ..) sorted by (-key, slot, col); the first `take` win.  Every candidate within MARGIN
    of the last winner's key (and every winner) must be, pair by adjacent pair, an intended tie or MARGIN apart."""
    if take == 0 or not cands:
        return
    take = min(take, len(cands))
    floor = cands[take - 1][0] - MARGIN
    n = take
    while n < len(cands) and cands[n][0] > floor:
        n += 1
    for a, b in zip(cands[:n - 1], cands[1:n]):
        if a[0] - b[0] >= MARGIN or a[3] == b[3]:
            continue
        raise Undecidable("%s: candidates (slot %d, col %d) and (slot %d, col %d) are %.3g apart"
                          % (what, a[1], a[2], b[1], b[2], a[0] - b[0]))


def _ranked(key, slot, col):
    order = np.lexsort((col, slot, -key))
    return order[np.isfinite(key[order])]


def beam_step(case, st, rows, pos, tables):
    """One selection step of beam search.  case: select_cases.BeamCase; st: the state going in (select_cases.beam_start
    / beam_given; cum float64); rows: {global row: fp32 (Vx,) raw scores} of exactly the live rows; tables: the embedding
    tables.  Returns (the state coming out, info): the outgoing state holds cum (float64), fin, len, met, seq, anc, cap,
    n_done; info holds next_token, next_mask, x0, x0_written (rows the kernel writes), dead (slots without a candidate:
    their histories are not specified), parent and tok of every slot, carried (captions moved over as they are), and
    what the case tags ask about."""
    k, V, K, F, Vx = case.beam, case.V, case.K, case.F, case.Vx
    R, L, end = case.R, case.max_len, case.end
    ngram, min_len, alpha = case.rules if case.rules else (0, 0, 0.0)
    lp_on = case.rules is not None and alpha != 0
    lp = lp_table(alpha, L).double().numpy() if case.rules else None
    groups = case.groups if case.form == "diverse" else 1
    kg = k // groups
    live_all = [r for r in range(R) if not st["fin"][r] and st["cum"][r] != NEG]
    if sorted(rows) != live_all:
        raise AssertionError("score rows %s given for live rows %s" % (sorted(rows), live_all))
    out = {n: st[n].copy() for n in ("cum", "fin", "len", "met", "seq", "anc")}
    out["cap"] = None if st["cap"] is None else st["cap"].copy()
    out["n_done"] = st["n_done"]
    info = dict(next_token=np.zeros(R, np.int64), next_mask=np.zeros(R, np.int64), x0=np.zeros((R, case.d), np.float32),
                x0_written=np.zeros(R, bool), dead=np.zeros(R, bool), parent=np.zeros(R, np.int64),
                tok=np.full(R, -1, np.int64), carried=[], banned={}, picks=[], counts=[], rank_of_pick={})
    for b in range(case.B):
        r0 = b * k
        live = [j for j in range(k) if (r0 + j) in rows]
        if not live:
            info["carried"].append(b)
            continue                                   # the tables move over as they are; x0 is not written
        # every candidate of the caption: key, slot, column, bank, new cum, and what makes two of them an intended tie
        key, slot, col, bank, ncum, sig_of_slot = [], [], [], [], [], {}
        force = list(case.force[b]) if case.form == "forced" else []
        for j in range(k):
            r = r0 + j
            cum = st["cum"][r]
            if cum == NEG:
                continue
            if st["fin"][r]:
                key.append(np.array([cum / lp[st["len"][r]] if lp_on else cum]))
                slot.append(np.array([j])); col.append(np.array([0])); ncum.append(np.array([cum]))
                bank.append(np.array([bank_of(int(st["met"][r]))]))
                sig_of_slot[j] = [("ended", cum, int(st["len"][r]) if lp_on else 0)]
                continue
            x = np.asarray(rows[r])
            assert x.dtype == np.float32 and x.shape == (Vx,) and np.isfinite(x).all() and np.abs(x).max() <= 16
            s = cum + (x.astype(np.float64) - lse64(x))
            kv = s / lp[pos + 1] if lp_on else s.copy()
            ban = banned_set([int(t) for t in st["seq"][r, :pos]], pos, ngram, min_len, end) if case.rules else set()
            info["banned"][r] = ban
            bk = np.full(Vx, bank_of(int(st["met"][r])))
            if force:
                met = int(st["met"][r])
                if any(f >= 0 and not (met >> q) & 1 for q, f in enumerate(force)):
                    ban = ban | {end}                  # <end> stays closed while a slot is unmet
                for f in set(f for f in force if f >= 0):
                    bk[f] = bank_of(met | slots_of(force, f))
            if ban:
                kv[sorted(ban)] = NEG
            key.append(kv); slot.append(np.full(Vx, j)); col.append(np.arange(Vx)); ncum.append(s); bank.append(bk)
            sig_of_slot[j] = (cum, x.tobytes(), x)      # a live candidate's signature: these and its raw score
        key, slot, col, bank, ncum = (np.concatenate(a) for a in (key, slot, col, bank, ncum))

        def signature(i, n=0):
            s_ = sig_of_slot[int(slot[i])]
            if isinstance(s_, list):
                return s_[0]
            return ("live", s_[0], s_[1], float(s_[2][col[i]]), n)

        def tuples(idx, keys, ns=None):
            return [(float(keys[q]), int(slot[i]), int(col[i]), signature(i, 0 if ns is None else int(ns[q])), int(i))
                    for q, i in enumerate(idx)]

        picks = []                                       # candidate index of every slot, or None
        if case.form == "forced":
            n_req = sum(1 for f in force if f >= 0)
            per_bank, cands = {}, []
            for bnk in np.unique(bank):
                sel = np.nonzero(bank == bnk)[0]
                o = sel[_ranked(key[sel], slot[sel], col[sel])]
                per_bank[int(bnk)] = o
                cands += [(float(key[i]), int(slot[i]), int(col[i]), int(bnk), int(i)) for i in o[:k]]
            taken = allocate(cands, n_req, k)
            for bnk, o in per_bank.items():
                t = sum(1 for c in taken if c[3] == bnk)
                lim = _window(key[o], t)
                _check_window(tuples(o[:lim], key[o[:lim]]), t, "%s step %d caption %d bank %d" % (case.name, pos, b, bnk))
            picks = [c[4] for c in taken] + [None] * (k - len(taken))
            info["banks_visited"] = info.get("banks_visited", []) + [([c[3] for c in taken], n_req)]
        else:
            lam = float(case.lam) if case.form == "diverse" else 0.0
            expanded = []
            for g in range(groups):
                sel = np.nonzero((slot >= g * kg) & (slot < (g + 1) * kg))[0]
                n = np.zeros(len(sel))
                ended = np.array([bool(st["fin"][r0 + j]) for j in slot[sel]], dtype=bool) if len(sel) else np.zeros(0, bool)
                for w in expanded:
                    n[(col[sel] == w) & ~ended] += 1
                pk = key[sel] - lam * n
                o = _ranked(pk, slot[sel], col[sel])
                lim = _window(pk[o], kg)
                tl = tuples(sel[o[:lim]], pk[o[:lim]], n[o[:lim]])
                _check_window(tl, kg, "%s step %d caption %d group %d" % (case.name, pos, b, g))
                got = [t[4] for t in tl[:kg]]
                info["counts"].append({int(col[i]): int(c) for i, c in zip(sel, n) if c > 0})
                for i in got:
                    if not st["fin"][r0 + int(slot[i])]:
                        expanded.append(int(col[i]))
                picks += got + [None] * (kg - len(got))
        # the winners become the caption's new slots
        before = sum(1 for j in range(k) if st["fin"][r0 + j] or st["cum"][r0 + j] == NEG)
        after = 0
        for h, i in enumerate(picks):
            r = r0 + h
            info["x0_written"][r] = pos + 1 < L
            if i is None:                                # fewer candidates than beams: a dead slot
                info["dead"][r] = True
                out["cum"][r], out["fin"][r], out["met"][r] = NEG, 1, 0
                if lp_on:
                    out["len"][r] = 0
                after += 1
                tok_in = 0
            else:
                j, c = int(slot[i]), int(col[i])
                src = r0 + j
                info["parent"][r] = j
                out["cum"][r] = ncum[i]
                out["seq"][r] = st["seq"][src]
                out["anc"][r] = st["anc"][src]
                if out["cap"] is not None:
                    out["cap"][r] = st["cap"][src]
                if st["fin"][src]:                       # an ended hypothesis is carried as it is
                    out["fin"][r], out["met"][r] = 1, st["met"][src]
                    if lp_on:
                        out["len"][r] = st["len"][src]
                    after += 1
                    tok_in = 0
                    if out["cap"] is not None:
                        out["cap"][r, pos + 1:] = case.start
                else:
                    info["tok"][r] = c
                    info["rank_of_pick"][(r, c)] = int((np.asarray(rows[src]) > rows[src][c]).sum())
                    out["fin"][r] = int(c == end)
                    out["met"][r] = int(st["met"][src]) | (slots_of(force, c) if force else 0)
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


def to_hyps(case, st, b, pos):
    """Caption b's slots going into step pos as diverse_step / constrained_step take them."""
    hyps = []
    for j in range(case.beam):
        r = b * case.beam + j
        if st["cum"][r] == NEG:
            hyps.append(None)
            continue
        seq = [int(t) for t in st["seq"][r]]
        n = seq.index(case.end) + 1 if st["fin"][r] else pos
        hyps.append(dict(seq=seq[:n], score=float(st["cum"][r]), fin=bool(st["fin"][r]), L=n, met=int(st["met"][r])))
    return hyps


# -------------------------------------------------------------------------------------------------------- sampling
def sample_step(case, st, rows, pos, tables):
    """One sampled selection step.  st: output, finished, n_done, log_prob (float64), cap_buf; rows: {row: fp32 (Vx,)}
    of the rows that have not finished.  Returns (state out, info): info holds next_token, next_mask, x0, written (the
    launch ran at all), tok, kept, banned and the gaps of every row."""
    V, K, F, Vx, R, L, end = case.V, case.K, case.F, case.Vx, case.R, case.max_len, case.end
    out = {n: st[n].copy() for n in ("output", "finished", "log_prob")}
    out["cap_buf"] = None if st["cap_buf"] is None else st["cap_buf"].copy()
    out["n_done"] = st["n_done"]
    info = dict(next_token=np.zeros(R, np.int64), next_mask=np.zeros(R, np.int64), x0=np.zeros((R, case.d), np.float32),
                written=st["n_done"] < R, tok={}, kept={}, banned={}, smax={})
    if not info["written"]:
        return out, info                                 # every row has finished: the launch leaves everything alone
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
            ban = banned_set([int(t) for t in st["output"][r, :pos]], pos, ngram, min_len, end) if case.rules else set()
            allowed = np.ones(Vx, bool)
            allowed[sorted(ban)] = False
            sa = s[allowed]
            keep_a, ratio = sample_ref.kept_set(sa, T, top_k, float(top_p))
            if 0 < top_k < sa.size:
                thr = np.sort(sa)[::-1][top_k - 1]
                gap = np.abs(sa.astype(np.float64) - float(thr))
                if ((gap > 0) & (gap < MARGIN)).any():
                    raise Undecidable("%s row %d: a score %.3g from the top-k threshold" % (case.name, r, gap[gap > 0].min()))
            if top_p < 1 and (np.abs(ratio) < MARGIN).any():
                raise Undecidable("%s row %d: strictly-greater mass %.3g of W from p" % (case.name, r, np.abs(ratio).min()))
            keep = np.zeros(Vx, bool)
            keep[np.nonzero(allowed)[0][keep_a]] = True
            g = sample_ref.gumbel(case.seed, b, j, pos, Vx)
            v = np.where(keep, s / T + g, -np.inf).astype(np.float32)
            tok = int(np.argmax(v))
            top = np.sort(v[keep])[::-1]
            if len(top) > 1 and top[0] - top[1] < MARGIN:
                raise Undecidable("%s row %d: best two perturbed values %.3g apart" % (case.name, r, top[0] - top[1]))
            info["tok"][r], info["kept"][r], info["banned"][r], info["smax"][r] = tok, keep, ban, int(np.argmax(s))
            out["output"][r, pos] = tok
            out["log_prob"][r, pos] = float(s[tok]) - lse64(s)
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
