"""float64 references of caption prefixes in beam search and sampling (csrc/decode_select.hip and
csrc/sample.hip, the PREFIX instantiations).  They are the references the suite already has, called as they are:

  a forced step   the existing step with every column but the forced one banned, and the row's rule bans dropped for
                  that step
  a free step     the existing step

The existing references take a row's bans from beam_rules_ref.banned_set, each through its own module's name.  While
one of them runs here, that name is bound to forced_bans(), which knows the forced column of the row it is asked
about; nothing else of the reference changes, so the ranking, the MARGIN / Undecidable discipline, the bias sums, the
log-softmax over every raw column and the bookkeeping are the existing code.

  beam_step / sample_step    one step on hand-built rows: select_ref (plain, diverse) or column_bias_ref (a case with
                             bias slots), with case.prefix (B lists of columns, -1 = free) applied
  predict_beam_prefix        a whole CPU search on the oracle's scores: column_bias_ref.predict_beam_bias (plain, rules,
                             bias; it reports its decision margin) or diverse_beam_ref.predict_diverse_beam
  forced_of                  the forced column of (caption, step) or -1"""
import contextlib
import dataclasses

import numpy as np
import torch

import beam_rules_ref
import column_bias_ref
import diverse_beam_ref
import select_ref
from select_ref import NEG

_real_banned_set = beam_rules_ref.banned_set


def forced_of(prefix, b, pos):
    """The forced column of caption b at step pos, or -1.  prefix: None, or B sequences of columns (-1 = free)."""
    if prefix is None:
        return -1
    p = prefix[b]
    return int(p[pos]) if pos < len(p) and p[pos] >= 0 else -1


def table(prefix, B, max_len):
    """The device form: int32 (B, max_len), -1 = a free step."""
    t = np.full((B, max_len), -1, np.int32)
    for b in range(B):
        for pos in range(max_len):
            t[b, pos] = forced_of(prefix, b, pos)
    return t


@contextlib.contextmanager
def forced_bans(modules, Vx, column_of_call):
    """Bind banned_set in `modules` to: every column but the forced one where column_of_call(seq, t) names one (the
    rule bans dropped), the real rule bans elsewhere."""
    def banned(seq, t, n, m, end):
        f = column_of_call(seq, t)
        if f < 0:
            return _real_banned_set(seq, t, n, m, end)
        return set(range(Vx)) - {f}
    saved = [m.banned_set for m in modules]
    for m in modules:
        m.banned_set = banned
    try:
        yield
    finally:
        for m, s in zip(modules, saved):
            m.banned_set = s


def _with_rules(case):
    """The references ask for bans only under rules: a rule-free case runs under rules whose every word is zero (the
    header's promise: the bits of the entry without rules)."""
    if case.rules is not None:
        return case
    zero = (0, 0, 0.0) if hasattr(case, "beam") else (0, 0)
    return dataclasses.replace(case, rules=zero)


def _by_row(case, rows_in_call_order, per, pos):
    """The step references ask for the bans of the live rows in ascending order, once each."""
    it = iter(rows_in_call_order)

    def column_of_call(seq, t):
        r = next(it)
        assert t == pos
        return forced_of(getattr(case, "prefix", None), r // per, pos)
    return column_of_call


def beam_step(case, st, rows, pos, tables):
    """select_ref.beam_step (plain, diverse) or column_bias_ref.beam_step (a case with bias_cols) under case.prefix."""
    biased = getattr(case, "bias_cols", None) is not None
    mod = column_bias_ref if biased else select_ref
    with forced_bans([mod], case.Vx, _by_row(case, sorted(rows), case.beam, pos)):
        out, info = mod.beam_step(_with_rules(case), st, rows, pos, tables)
    info["forced"] = {r: forced_of(getattr(case, "prefix", None), r // case.beam, pos) for r in rows}
    return out, info


def sample_step(case, st, rows, pos, tables):
    """select_ref.sample_step or column_bias_ref.sample_step (a case with bias_cols) under case.prefix.  A forced step
    has one allowed column: the knobs select nothing and no noise decides."""
    biased = getattr(case, "bias_cols", None) is not None
    mod = column_bias_ref if biased else select_ref
    with forced_bans([mod], case.Vx, _by_row(case, sorted(rows), case.rps, pos)):
        out, info = mod.sample_step(_with_rules(case), st, rows, pos, tables)
    info["forced"] = {r: forced_of(getattr(case, "prefix", None), r // case.rps, pos) for r in rows}
    return out, info


# ------------------------------------------------------------------------------------------- whole CPU searches
def _diverse_margin(hyps, new, rows, i, groups, lam, lp, end, bans):
    """The smallest gap of one diverse step between two candidates whose order decides something: winners among each
    other and the last winner against the first candidate left, group by group (penalised fp32 keys as diverse_step)."""
    beam = len(hyps)
    kg = beam // groups
    margin = float("inf")
    for g in range(groups):
        expanded = [h["seq"][-1] for h in new[:g * kg] if h is not None and not (h["fin"] and h["L"] <= i) and
                    len(h["seq"]) == i + 1]
        keys = []
        for j in range(g * kg, (g + 1) * kg):
            h = hyps[j]
            if h is None:
                continue
            if h["fin"]:
                keys.append(diverse_beam_ref.key(h["score"], h["L"], lp))
                continue
            s = (torch.tensor(h["score"], dtype=torch.float64) + rows[j].double()).float()
            cnt = torch.zeros(rows[j].numel(), dtype=torch.float32)
            for w in expanded:
                cnt[w] += 1
            pk = s / lp[i + 1] - torch.tensor(lam, dtype=torch.float32) * cnt
            ban = (bans or {}).get(j, set())
            if ban:
                pk[list(ban)] = float("-inf")
            keys += [v for v in pk.topk(min(kg + 1, pk.numel())).values.tolist() if v != float("-inf")]
        keys.sort(reverse=True)
        for a, b in zip(keys[:kg], keys[1:kg + 1]):
            margin = min(margin, a - b)
    return margin


@torch.no_grad()
def predict_beam_prefix(cfg, P, enc_out, max_pred_len, entities, facts=None, beam_size=5, prefix=None, bias=None,
                        num_beam_groups=1, diversity_penalty=0.0, length_penalty=0.0, no_repeat_ngram_size=0, min_len=0):
    """One caption's CPU search under a prefix (a list of columns; None or [] = none).  Returns dict(best, score, key,
    hyps, margin): hyps the final hypotheses [(seq, score, length)] in slot order (None: an unused slot), margin the
    smallest decision gap over the free steps and the final choice (a forced step decides nothing)."""
    Vx = cfg.vocab_size + entities.shape[1] + (facts.shape[1] if facts is not None else 0)
    pre = [list(prefix or [])]

    def column_of_call(seq, t):
        return forced_of(pre, 0, t)

    rules = dict(length_penalty=length_penalty, no_repeat_ngram_size=no_repeat_ngram_size, min_len=min_len)
    if num_beam_groups > 1:
        assert bias is None
        margins = []
        real_step = diverse_beam_ref.diverse_step

        def step(hyps, rows, i, groups, lam, lp, end, bans=None):
            new = real_step(hyps, rows, i, groups, lam, lp, end, bans)
            if forced_of(pre, 0, i) < 0:
                margins.append(_diverse_margin(hyps, new, rows, i, groups, lam, lp, end, bans))
            return new
        diverse_beam_ref.diverse_step = step
        try:
            with forced_bans([diverse_beam_ref], Vx, column_of_call):
                best, score, key, groups = diverse_beam_ref.predict_diverse_beam(
                    cfg, P, enc_out, max_pred_len, entities, facts, beam_size, num_beam_groups, diversity_penalty, **rules)
        finally:
            diverse_beam_ref.diverse_step = real_step
        hyps = [None if h is None else h[:3] for g in groups for h in g]
        # the final choice: two groups may hold one and the same hypothesis (both leaders follow the prefix), which is no
        # decision -- either is the same caption with the same score
        keys = sorted({tuple(h[0]): h[3] for g in groups for h in g if h is not None}.values(), reverse=True)
        if len(keys) > 1:
            margins.append(keys[0] - keys[1])
        return dict(best=best, score=score, key=key, hyps=hyps, groups=groups, margin=min(margins, default=float("inf")))
    with forced_bans([column_bias_ref], Vx, column_of_call):
        best, score, key, hyps, margin = column_bias_ref.predict_beam_bias(cfg, P, enc_out, max_pred_len, entities, facts,
                                                                           beam_size, bias=bias, **rules)
    hyps = [h[:3] for h in hyps] + [None] * (beam_size - len(hyps))
    return dict(best=best, score=score, key=key, hyps=hyps, margin=margin)


def sample_cpu(cfg, P, enc_b, ents_b, facts_b, prefix_row, b, n, seed, max_len, temperature=1.0, top_k=0, top_p=1.0,
               no_repeat_ngram_size=0, min_len=0, bias=None):
    """Caption b's n samples drawn on the CPU from the oracle's float64 scores, step by step: a forced step takes the
    prefix column, a free step is column_bias_ref.draw (sample_ref.draw on s + b) under the rule bans.  Returns
    (tokens [n lists, <end> included], log-probabilities [n lists], margin, boundary): margin the smallest gap at a free
    step between the two best perturbed values or between a score and the top-k threshold, boundary the smallest
    |strictly-greater mass / W - p| of top-p."""
    from test_sample_gpu import teacher_forced_scores
    toks_all, lps_all, margin, boundary = [], [], float("inf"), float("inf")
    for j in range(n):
        toks, lps = [], []
        for i in range(max_len):
            sc = teacher_forced_scores(cfg, P, enc_b, ents_b, facts_b, toks + [cfg.pad], max_len)[i]
            s = sc.astype(np.float32)
            f = forced_of([prefix_row], 0, i)
            if f >= 0:
                t = f
            else:
                bvec = np.zeros(s.size) if bias is None else bias
                ban = _real_banned_set(toks, i, no_repeat_ngram_size, min_len, cfg.end)
                g = select_ref.sample_ref.gumbel(seed, b, j, i, s.size)
                t, keep, top, ratio, cols = column_bias_ref.draw(s, bvec, temperature, top_k, top_p, g, ban)
                if top.size > 1:
                    margin = min(margin, float(top[0] - top[1]))
                sp = (s + bvec.astype(np.float32))[cols]
                if 0 < top_k < sp.size:
                    kth = np.sort(sp)[::-1][top_k - 1]
                    gap = np.abs(sp.astype(np.float64) - float(kth))
                    margin = min(margin, float(gap[gap > 0].min()))
                if top_p < 1:
                    boundary = min(boundary, float(np.abs(ratio).min()))
            toks.append(int(t))
            lps.append(float(sc[t] - (sc.max() + np.log(np.exp(sc - sc.max()).sum()))))
            if t == cfg.end:
                break
        toks_all.append(toks)
        lps_all.append(lps)
    return toks_all, lps_all, margin, boundary
