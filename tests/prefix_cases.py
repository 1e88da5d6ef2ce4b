"""Hand-built cases of caption prefixes in beam search and sampling, in the style of
column_bias_cases.py: scripted runs on raw score rows, the state going in, the knobs and every caption's prefix.
tests/prefix_ref.py says what must come out, tests/test_prefix_cpu.py checks the table (every case decidable, every tag
true of the reference's own trace) and tests/test_prefix_gpu.py runs it through ick_decode_select_beam_prefix /
ick_decode_select_sample_prefix.

In every forced step of every case the forced column is NOT the row's best: it scores 1.0 under peaks of 3 to 5, so a
selection that ignored the prefix would be seen.  max_len is 6.

The end-to-end cases of tests/test_prefix_gpu.py (E2E, e2e_inputs, e2e_prefix) are defined here as well, so that
tests/test_prefix_cpu.py can hold the float64 oracle's own decision margins to ten times the project's MARGIN."""
import functools
from dataclasses import dataclass

import numpy as np

import column_bias_cases as CB
import prefix_ref as ref
import select_cases as SC
from select_cases import END, NEG, PAD, START, hyp, row, srow

NINF = float("-inf")
L6 = 6


def rows_fn(seed, base, npeaks=10, per=None, end_high=()):
    """Rows for whichever rows are live: `npeaks` peaks from 5.0 down (start and spacing shifted by row and step, so that candidates of two parents do not tie) at columns
    that depend on (seed, row, step) and avoid the step's forced column, which scores 1.0; <end> scores 4.875 at the
    (row, step) pairs of end_high and -2 elsewhere."""
    def fn(case, st, live, pos):
        rps = case.beam if hasattr(case, "beam") else case.rps
        out = {}
        for r in live:
            f = ref.forced_of(case.prefix, r // rps, pos)
            peaks, span = {}, case.Vx - 3
            for q in range(min(npeaks, span - 1)):
                c = 3 + (seed * 13 + 7 * r + 5 * pos + 11 * q) % span
                while c == f or c in peaks:
                    c = 3 + (c - 2) % span
                peaks[c] = 5.0 - (0.375 + 0.0390625 * ((r + pos) % 8)) * q - 0.0546875 * (r % 8)
            peaks[END] = 4.875 if (r, pos) in end_high else -2.0
            if f >= 0:
                peaks[f] = 1.0
            out[r] = row(case.Vx, peaks, base)
        return out
    return fn


def scripted_fn(seed):
    """select_cases.scripted rows (random peaks on a 1/8 grid, <end> among the best from step 1 on for some rows), with
    the step's forced column at 1.0 and, should it have been the row's best, the best put elsewhere."""
    inner = SC.scripted(seed)

    def fn(case, st, live, pos):
        out = inner(case, st, live, pos)
        for r, x in out.items():
            f = ref.forced_of(case.prefix, r // case.beam, pos)
            if f >= 0:
                x[f] = 1.0
                assert int(np.argmax(x)) != f
        return out
    return fn


# ------------------------------------------------------------------------------------------------------------- beam
@dataclass
class PrefixBeamCase(SC.BeamCase):
    prefix: list = None                 # B lists of columns, -1 = free; shorter than max_len: free from its end on


@dataclass
class PrefixBiasBeamCase(CB.BiasBeamCase):
    prefix: list = None


def beam_state(case):
    return CB.beam_state(case) if isinstance(case, CB.BiasBeamCase) else SC.beam_state(case)


def run_beam(case):
    t, st, trace = SC.tables(case), beam_state(case), []
    for pos, fn in case.steps:
        live = [r for r in range(case.R) if not st["fin"][r] and st["cum"][r] != NEG]
        rows = fn(case, st, live, pos)
        out, info = ref.beam_step(case, st, rows, pos, t)
        trace.append(dict(pos=pos, st=st, rows=rows, out=out, info=info))
        st = out
    return trace


@functools.lru_cache(maxsize=None)
def beam_trace(name):
    return run_beam(BEAM_BY_NAME[name])


def steps(n, fn, first=0):
    return [(p, fn) for p in range(first, n)]


BEAM = [
    # three captions: no prefix, a prefix of 2 (a word, then entity pointer 2), a prefix over all 6 steps
    PrefixBeamCase("batch_p0_p2_p6", "plain", 3, 3, 50, 4, 0, L6, steps(6, scripted_fn(100)),
                   prefix=[[], [7, 52], [9, 10, 11, 12, 13, 14]],
                   expect=("width_3", "batch_p_zero_mid_full", "entity_pointer", "forced_run_then_fan_out",
                           "unused_slots_stay_unused", "full_prefix_never_fans_out")),
    # three chunks (Vx = 2104): the chunk edge 1023 | 1024 and the last column of the last chunk, then beam 8 fans out
    PrefixBeamCase("chunks_beam8", "plain", 1, 8, 2100, 4, 0, L6, steps(5, rows_fn(2, -8.0)),
                   prefix=[[1023, 1024, 2103]],
                   expect=("width_8", "chunk_edge", "last_chunk_of_three", "forced_run_then_fan_out", "entity_pointer")),
    # beam 1, knowledge-shaped (F > 0: caption buffers); 5 6 5 then 6 again is what the bigram rule bans; a fact pointer
    PrefixBeamCase("beam1_ngram_facts", "plain", 1, 1, 50, 4, 4, L6, steps(6, rows_fn(3, -8.0)), rules=(2, 0, 0.0),
                   prefix=[[5, 6, 5, 6, 55]],
                   expect=("width_1", "forced_column_rule_banned", "fact_pointer", "caption_buffers")),
    # <end>'s neighbour columns; min_len bans <end> and the length penalty ranks by a length that counts the prefix
    PrefixBeamCase("end_neighbours_lp", "plain", 1, 3, 50, 4, 0, L6,
                   steps(5, rows_fn(4, -8.0, end_high={(0, 3), (1, 3), (0, 4), (2, 4)})), rules=(0, 3, 0.75),
                   prefix=[[END - 1, END + 1]],
                   expect=("end_neighbours", "length_counts_prefix", "forced_run_then_fan_out")),
    # 4 hypotheses in 2 groups: both leaders follow the prefix although group 1 is penalised for it
    PrefixBeamCase("groups_4_2", "diverse", 1, 4, 50, 4, 0, L6, steps(4, rows_fn(5, -8.0)), groups=2, lam=0.75,
                   prefix=[[7, 8]], expect=("both_leaders_follow", "forced_run_then_fan_out")),
    # biased form: a finite bias on a prefix column is carried in the sum, a -inf bias sits elsewhere
    PrefixBiasBeamCase("bias_on_prefix", "plain", 2, 3, 50, 4, 0, L6, steps(4, rows_fn(6, -8.0)),
                       **dict(zip(("bias_cols", "bias_vals"), CB.per_caption([(7, 0.5), (30, NINF), (10, 1.0)], [(9, -0.25)]))),
                       prefix=[[7, 9], [-1]],
                       expect=("bias_sum_carries_prefix", "ninf_elsewhere", "caption_all_free_beside_forced")),
]
BEAM_BY_NAME = {c.name: c for c in BEAM}


def _forced_steps(case, tr):
    """(step dict, caption, forced column) of every (step, caption) with a forced column and a live row."""
    k = case.beam if hasattr(case, "beam") else case.rps
    for t in tr:
        for b in range(case.B):
            f = ref.forced_of(case.prefix, b, t["pos"])
            if f >= 0 and any(r // k == b for r in t["rows"]):
                yield t, b, f


def _p(case, b):
    return sum(1 for c in case.prefix[b] if c >= 0)


def not_argmax_everywhere(case, tr):
    """The property every case must have: at every forced step the forced column is not the row's best."""
    k = case.beam if hasattr(case, "beam") else case.rps
    n = 0
    for t, b, f in _forced_steps(case, tr):
        for r, x in t["rows"].items():
            if r // k == b:
                n += 1
                if int(np.argmax(x)) == f:
                    return False
    return n > 0


def _one_live_through_prefix(case, tr):
    k = case.beam
    groups = case.groups if case.form == "diverse" else 1
    for t, b, f in _forced_steps(case, tr):
        cum = t["out"]["cum"][b * k:(b + 1) * k]
        if (cum != NEG).sum() != groups:
            return False
        if not all(t["info"]["tok"][b * k + j] == f for j in range(k) if cum[j] != NEG):
            return False
    return True


def _fan_out(case, tr):
    """At the first free step after a forced run of two or more, every slot (of every group) is filled from one parent."""
    k = case.beam
    kg = k // (case.groups if case.form == "diverse" else 1)
    for b in range(case.B):
        p = _p(case, b)
        if p < 2 or p >= case.max_len:
            continue
        t = next((t for t in tr if t["pos"] == p), None)
        if t is None:
            continue
        sl = slice(b * k, (b + 1) * k)
        if t["info"]["dead"][sl].any() or (t["out"]["cum"][sl] == NEG).any():
            return False
        return all(t["info"]["parent"][b * k + j] == (j // kg) * kg for j in range(k))
    return False


def _rule_banned(case, tr):
    from beam_rules_ref import banned_set
    for t, b, f in _forced_steps(case, tr):
        for r in t["rows"]:
            seq = [int(q) for q in (t["st"]["seq"] if "seq" in t["st"] else t["st"]["output"])[r, :t["pos"]]]
            if f in banned_set(seq, t["pos"], case.rules[0], case.rules[1], case.end) and t["info"]["tok"][r] == f:
                return True
    return False


def _bias_sum(case, tr):
    for t, b, f in _forced_steps(case, tr):
        bias = CB.ref.bias_row(case.Vx, case.bias_cols[b], case.bias_vals[b])
        r = b * case.beam
        if bias[f] != 0 and np.isfinite(bias[f]) and t["out"]["bsum"][r] == t["st"]["bsum"][r] + bias[f]:
            return tr[-1]["out"]["bsum"][b * case.beam:(b + 1) * case.beam].min() >= bias[f]     # carried to the end
    return False


BEAM_TAGS = {
    "width_1": lambda c, tr: c.beam == 1,
    "width_3": lambda c, tr: c.beam == 3,
    "width_8": lambda c, tr: c.beam == 8,
    "batch_p_zero_mid_full": lambda c, tr: c.B == 3 and sorted(_p(c, b) for b in range(3))[0] == 0 and
    0 < sorted(_p(c, b) for b in range(3))[1] < c.max_len and sorted(_p(c, b) for b in range(3))[2] == c.max_len,
    "entity_pointer": lambda c, tr: any(c.V <= f < c.V + c.K for _, _, f in _forced_steps(c, tr)),
    "fact_pointer": lambda c, tr: c.F > 0 and any(f >= c.V + c.K for _, _, f in _forced_steps(c, tr)),
    "forced_run_then_fan_out": lambda c, tr: _one_live_through_prefix(c, tr) and _fan_out(c, tr),
    "unused_slots_stay_unused": _one_live_through_prefix,
    "full_prefix_never_fans_out": lambda c, tr: any(
        _p(c, b) == c.max_len and tr[-1]["pos"] == c.max_len - 1 and
        (tr[-1]["out"]["cum"][b * c.beam:(b + 1) * c.beam] != NEG).sum() == 1 for b in range(c.B)),
    "chunk_edge": lambda c, tr: {1023, 1024} <= {f for _, _, f in _forced_steps(c, tr)},
    "last_chunk_of_three": lambda c, tr: (c.Vx + 1023) // 1024 == 3 and any(f // 1024 == 2 for _, _, f in _forced_steps(c, tr)),
    "forced_column_rule_banned": _rule_banned,
    "caption_buffers": lambda c, tr: c.F > 0 and all(
        t["out"]["cap"][b * c.beam, t["pos"] + 1] == f for t, b, f in _forced_steps(c, tr) if t["pos"] + 1 < c.max_len),
    "end_neighbours": lambda c, tr: {c.end - 1, c.end + 1} <= {f for _, _, f in _forced_steps(c, tr)},
    "length_counts_prefix": lambda c, tr: c.rules is not None and c.rules[2] != 0 and all(
        t["out"]["len"][b * c.beam] == t["pos"] + 1 for t, b, f in _forced_steps(c, tr)) and
    any(t["out"]["fin"].any() for t in tr),
    "both_leaders_follow": lambda c, tr: c.form == "diverse" and c.lam > 0 and all(
        [t["info"]["tok"][b * c.beam + g * (c.beam // c.groups)] for g in range(c.groups)] == [f] * c.groups and
        any(f in n for n in t["info"]["counts"]) for t, b, f in _forced_steps(c, tr)),
    "bias_sum_carries_prefix": _bias_sum,
    "ninf_elsewhere": lambda c, tr: any(v == NINF for l in c.bias_vals for v in l),
    "caption_all_free_beside_forced": lambda c, tr: c.B > 1 and any(_p(c, b) == 0 for b in range(c.B)) and
    any(_p(c, b) > 0 for b in range(c.B)),
}
BEAM_TAGS_REQUIRED = set(BEAM_TAGS)


# --------------------------------------------------------------------------------------------------------- sampling
@dataclass
class PrefixSampleCase(SC.SampleCase):
    prefix: list = None


@dataclass
class PrefixBiasSampleCase(CB.BiasSampleCase):
    prefix: list = None


def run_sample(case):
    t, st, trace = SC.tables(case), SC.sample_state(case), []
    for pos, fn in case.steps:
        live = [r for r in range(case.R) if not st["finished"][r]] if st["n_done"] < case.R else []
        rows = fn(case, st, live, pos) if live else {}
        out, info = ref.sample_step(case, st, rows, pos, t)
        trace.append(dict(pos=pos, st=st, rows=rows, out=out, info=info))
        st = out
    return trace


@functools.lru_cache(maxsize=None)
def sample_trace(name):
    return run_sample(SAMPLE_BY_NAME[name])


SAMPLE = [
    # top_k = 1 would take the row's best; caption 1 has no prefix and does; a fact pointer (F > 0: caption buffer)
    PrefixSampleCase("s_topk1", 2, 2, 50, 4, 3, L6, steps(3, rows_fn(11, -14.0, npeaks=6)), top_k=1, seed=5,
                     prefix=[[7, 55], [-1, -1]],
                     expect=("topk_1_overruled", "fact_pointer", "caption_all_free_beside_forced", "caption_buffers")),
    # a tiny top_p keeps the row's best alone
    PrefixSampleCase("s_topp_tiny", 1, 3, 50, 4, 0, L6, steps(3, rows_fn(12, -14.0, npeaks=6)), top_p=0.02, seed=6,
                     prefix=[[9, 52]], expect=("topp_overruled", "entity_pointer", "rows_per_sample_3")),
    # the unigram rule bans the second 5
    PrefixSampleCase("s_rule_banned", 1, 2, 50, 4, 0, L6, steps(3, rows_fn(13, -14.0, npeaks=6)), rules=(1, 0), seed=7,
                     prefix=[[5, 5]], expect=("forced_column_rule_banned",)),
    # biased form: a finite bias on the prefix column, a -inf bias on the row's best of the free step
    PrefixBiasSampleCase("s_biased", 1, 2, 50, 4, 0, L6, steps(2, rows_fn(14, -14.0, npeaks=6)), top_k=3, seed=8,
                         **dict(zip(("bias_cols", "bias_vals"), CB.slots((7, -0.5), (20, NINF)))),
                         prefix=[[7]], expect=("biased_form", "log_prob_stays_raw")),
    # row 0 has ended; row 1 of the same caption is forced
    PrefixSampleCase("s_ended_beside", 1, 2, 50, 4, 0, L6, steps(4, rows_fn(15, -14.0, npeaks=6), first=2), seed=9,
                     state0=[srow([5, END], fin=True), srow([5, 6])], prefix=[[5, 6, 8]],
                     expect=("ended_row_beside_forced",)),
    # Vx = 16386: the NG = 16 instantiation; the forced columns are its last and one of the middle
    PrefixSampleCase("s_ng16", 1, 2, 16380, 4, 2, L6, steps(3, rows_fn(16, -14.0, npeaks=6)), top_k=5, seed=10,
                     prefix=[[16385, 4096]], expect=("ng_16", "fact_pointer")),
]
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE}


def _forced_rows(case, tr):
    for t, b, f in _forced_steps(case, tr):
        for r in t["rows"]:
            if r // case.rps == b:
                yield t, r, f


SAMPLE_TAGS = {
    "topk_1_overruled": lambda c, tr: c.top_k == 1 and all(t["info"]["tok"][r] == f != t["info"]["smax"][r]
                                                           for t, r, f in _forced_rows(c, tr)),
    "topp_overruled": lambda c, tr: c.top_p < 0.05 and all(t["info"]["tok"][r] == f != t["info"]["smax"][r]
                                                           for t, r, f in _forced_rows(c, tr)),
    "fact_pointer": lambda c, tr: c.F > 0 and any(f >= c.V + c.K for _, _, f in _forced_steps(c, tr)),
    "entity_pointer": lambda c, tr: any(c.V <= f < c.V + c.K for _, _, f in _forced_steps(c, tr)),
    "rows_per_sample_3": lambda c, tr: c.rps == 3,
    "caption_all_free_beside_forced": lambda c, tr: c.B > 1 and any(_p(c, b) == 0 for b in range(c.B)) and
    any(_p(c, b) > 0 for b in range(c.B)),
    "caption_buffers": lambda c, tr: c.F > 0 and all(t["out"]["cap_buf"][r, t["pos"] + 1] == f
                                                     for t, r, f in _forced_rows(c, tr) if t["pos"] + 1 < c.max_len),
    "forced_column_rule_banned": _rule_banned,
    "biased_form": lambda c, tr: isinstance(c, CB.BiasSampleCase) and any(
        CB.ref.bias_row(c.Vx, c.bias_cols[r // c.rps], c.bias_vals[r // c.rps])[f] != 0 for _, r, f in _forced_rows(c, tr)),
    "log_prob_stays_raw": lambda c, tr: all(
        abs(t["out"]["log_prob"][r, t["pos"]] - (float(t["rows"][r][f]) - SC.ref.lse64(t["rows"][r]))) < 1e-12
        for t, r, f in _forced_rows(c, tr)),
    "ended_row_beside_forced": lambda c, tr: any(
        t["st"]["finished"].any() and not t["st"]["finished"].all() and any(True for _ in _forced_rows(c, [t])) for t in tr),
    "ng_16": lambda c, tr: c.Vx > 16384 and any(f == c.Vx - 1 for _, _, f in _forced_steps(c, tr)),
}
SAMPLE_TAGS_REQUIRED = set(SAMPLE_TAGS)


# ------------------------------------------------------------------------------------------------ end to end
E2E_B, E2E_LEN, E2E_K, E2E_F = 3, 8, 6, 5
RULES = dict(length_penalty=0.6, no_repeat_ngram_size=2, min_len=3)
# name -> (variant, V, seed of the model and inputs, predict_beam keywords).  The seeds are the first at which the float64
# oracle alone decides every free step of every caption by at least twenty times the project's MARGIN.
E2E_BEAM = {
    "geo_beam3": ("geo", 50, 3, dict(beam_size=3)),
    "knowledge_groups": ("knowledge", 1000, 1, dict(beam_size=4, num_beam_groups=2, diversity_penalty=0.5)),
    "geo_rules": ("geo", 1000, 4, dict(beam_size=3, **RULES)),
    "knowledge_bias": ("knowledge", 50, 1, dict(beam_size=3, column_bias="bias")),
}
# name -> (variant, V, seed of the model and inputs, predict_sample keywords)
E2E_SAMPLE = {
    "geo_T1": ("geo", 50, 1, dict(num_samples=2, seed=11)),
    "knowledge_topk_topp": ("knowledge", 1000, 1, dict(num_samples=2, seed=12, temperature=0.8, top_k=6, top_p=0.9,
                                                       no_repeat_ngram_size=2)),
    "knowledge_bias": ("knowledge", 50, 1, dict(num_samples=2, seed=13, top_k=8, column_bias="bias")),
}


def e2e_inputs(variant, V, seed):
    """(cfg, P, entities, facts, encoder output) of test_sample_gpu.make_case, without the device decoder."""
    import ick_amd.synth as synth
    from oracle import restatement as R
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    ents = synth.make_entities(variant, E2E_B, E2E_K, V, seed)
    facts = synth.make_facts(variant, E2E_B, E2E_F, E2E_K, seed) if variant != "geo" else None
    return cfg, P, ents, facts, synth.make_enc_out(E2E_B, seed)


def e2e_prefix(V, has_facts):
    """Prefixes of length 0, 2 and 8 in one batch: words, entity pointers and (with facts) a fact pointer."""
    last = V + E2E_K + 1 if has_facts else 11
    return [[-1] * E2E_LEN, [5, V + 1] + [-1] * (E2E_LEN - 2), [4, 6, V + 2, 7, 9, last, 12, 13]]


def e2e_bias(V):
    """(ids, values) for every caption: a boost on a prefix column (5), a pointer boost, a ban off the prefixes."""
    return ([5, V + 3, 8], [0.5, 1.0, NINF])
