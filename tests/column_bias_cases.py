"""Hand-built cases of the column bias of beam search and sampling, in the style of select_cases.py:
raw score rows, the state going in, the knobs and the caption's bias slots.  tests/column_bias_ref.py says what must come
out, tests/test_column_bias_cpu.py checks the table (every case decidable, every tag exhibited) and
tests/test_column_bias_gpu.py runs it through ick_decode_select_beam_biased / ick_decode_select_sample_biased.

Scores are on a 1/8 or 1/2 grid and biases are multiples of 1/8, so s + b and every bias sum are exact in fp32."""
import functools
from dataclasses import dataclass

import numpy as np

import column_bias_ref as ref
import select_cases as SC
from select_cases import END, NEG, PAD, START, fixed, hyp, row, scripted, srow

NINF = float("-inf")


def slots(*pairs, B=1):
    """B copies of one list of (column, value) slots."""
    return [[p[0] for p in pairs]] * B, [[p[1] for p in pairs]] * B


def per_caption(*lists):
    """One list of (column, value) slots per caption, padded with empty slots to the longest."""
    n = max(1, max(len(l) for l in lists))
    return ([[p[0] for p in l] + [-1] * (n - len(l)) for l in lists],
            [[p[1] for p in l] + [7.0] * (n - len(l)) for l in lists])       # an empty slot's value is ignored


# ------------------------------------------------------------------------------------------------------------- beam
@dataclass
class BiasBeamCase(SC.BeamCase):
    bias_cols: list = None              # (B, C) column ids, -1 = empty slot, C <= 64
    bias_vals: list = None              # (B, C) finite or -inf


def beam_state(case):
    st = SC.beam_state(case)
    st["bsum"] = np.zeros(case.R)
    for r, h in enumerate(case.state0 or []):
        if h is not None:
            st["bsum"][r] = h.get("bsum", 0.0)
    return st


def run_beam(case, step_local=False):
    """The reference's run of a case.  step_local: the bias ranks only at the step it is applied (every sum forgotten
    before the next step): what the persistence case must differ from."""
    t, st, trace = SC.tables(case), beam_state(case), []
    for pos, fn in case.steps:
        if step_local:
            st = dict(st, bsum=np.zeros(case.R))
        live = [r for r in range(case.R) if not st["fin"][r] and st["cum"][r] != NEG]
        rows = fn(case, st, live, pos)
        out, info = ref.beam_step(case, st, rows, pos, t)
        trace.append(dict(pos=pos, st=st, rows=rows, out=out, info=info))
        st = out
    return trace


@functools.lru_cache(maxsize=None)
def beam_trace(name):
    return run_beam(BEAM_BY_NAME[name])


def bhyp(seq, cum, fin=False, bsum=0.0):
    return dict(hyp(seq, cum, fin), bsum=bsum)


def _c64():
    """64 slots over columns 3 .. 66: small values of both signs, two bans and one decisive boost."""
    cols = list(range(3, 67))
    vals = [((i * 3) % 9 - 4) / 8 for i in range(64)]
    vals[cols.index(20)] = NINF
    vals[cols.index(21)] = NINF
    vals[cols.index(40)] = 2.5
    return [cols], [vals]


def _big8_rows(case, st, live, pos):
    return SC._big8_rows(case, st, live, pos)


def _persist_rows(case, st, live, pos):
    if pos == 0:
        return {0: row(54, {10: 4.0, 11: 3.5, 12: 3.0})}
    return {0: row(54, {20: 3.0, 21: 1.0}), 1: row(54, {22: 3.0, 23: 2.5})}


def _batch_rows(case, st, live, pos):
    """Every live row: three peaks by row and step, <end> strong from step 2 on for the even rows."""
    out = {}
    for r in live:
        peaks = {10 + (r * 3 + pos) % 30: 4.0 - 0.375 * (r % 5), 41 + (r + pos) % 9: 3.0 + 0.125 * (r % 3),
                 5 + (r + 2 * pos) % 4: 2.5 - 0.25 * (r % 2)}
        peaks[END] = 4.25 if pos >= 2 and r % 2 == 0 else -2.0
        out[r] = row(case.Vx, peaks)
    return out


BEAM = [
    BiasBeamCase("vx3_ban_max", "plain", 1, 2, 2, 1, 0, 4, [(0, fixed({0: np.float32([0.5, -1.0, 1.5])}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((2, NINF)))), expect=("vx3", "ban_row_max", "c_1")),
    BiasBeamCase("dead_slots", "plain", 1, 5, 3, 2, 2, 4, [(0, fixed({0: np.float32([0.5, 1.0, 1.5, 2.0, -0.5, 3.0, 0.0])}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((0, NINF), (2, NINF), (5, NINF)))),
                 expect=("dead_slot_from_bias", "ban_row_max", "width_5")),
    BiasBeamCase("edge_1023", "plain", 1, 2, 1015, 8, 0, 4, [(0, fixed({0: row(1023, {100: 4.0, 1022: 3.0})}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((1022, 2.0)))),
                 expect=("boost_overturns_argmax", "bias_last_column", "pointer_without_facts", "c_1", "width_2")),
    BiasBeamCase("edge_1024", "plain", 1, 2, 1000, 24, 0, 4, [(0, fixed({0: row(1024, {1023: 5.0, 1022: 3.5, 10: 4.0})}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((1022, 1.0), (1023, NINF)))),
                 expect=("ban_row_max", "bias_last_column", "boost_overturns_argmax")),
    BiasBeamCase("edge_1025", "plain", 1, 2, 1016, 5, 4, 4,
                 [(0, fixed({0: row(1025, {1024: 3.0, 1023: 4.0, 1022: 2.0, 7: 3.75})}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((1022, 1.0), (1023, -0.5), (1024, 1.5)))),
                 expect=("bias_in_single_column_chunk", "bias_last_column", "pointer_with_facts", "boost_overturns_argmax")),
    BiasBeamCase("v65536_beam8", "plain", 2, 8, 65520, 8, 8, 4, [(1, _big8_rows)],
                 state0=[bhyp([10 + j], -0.125 * j, bsum=0.25 * (j % 3)) for j in range(8)] + [bhyp([3], 0.0)] + [None] * 7,
                 **dict(zip(("bias_cols", "bias_vals"),
                            per_caption([(65535, 3.0), (1023, NINF), (1024, 0.625), (64512, -1.0)], [(64512, 4.125)]))),
                 expect=("chunks_64", "width_8", "list_per_caption", "bias_last_column")),
    BiasBeamCase("v66560_beam2", "plain", 1, 2, 66550, 10, 0, 4, [(1, SC._big2_rows)],
                 state0=[bhyp([10], -0.5), bhyp([11], -0.25, bsum=0.5)],
                 **dict(zip(("bias_cols", "bias_vals"), slots((66559, NINF), (65536, 1.0), (66000, 2.5)))),
                 expect=("chunks_65", "ban_row_max")),
    BiasBeamCase("beam1_lists", "plain", 3, 1, 50, 4, 0, 4,
                 [(0, fixed({0: row(54, {7: 3.0, 8: 2.0}), 1: row(54, {52: 3.0, 9: 2.5}), 2: row(54, {1: 3.0, 9: 2.5})}))],
                 **dict(zip(("bias_cols", "bias_vals"), per_caption([(8, 1.5)], [(52, NINF)], [(1, -1.0)]))),
                 expect=("width_1", "batch_3", "list_per_caption", "boost_overturns_argmax", "end_penalised")),
    BiasBeamCase("c64", "plain", 1, 2, 200, 8, 0, 4, [(0, fixed({0: row(208, {20: 5.0, 21: 4.5, 30: 4.0, 40: 2.0, 50: 3.0})}))],
                 **dict(zip(("bias_cols", "bias_vals"), _c64())), expect=("c_64", "ban_row_max", "boost_overturns_argmax")),
    BiasBeamCase("persistence", "plain", 1, 2, 50, 4, 0, 4, [(0, _persist_rows), (1, _persist_rows)],
                 **dict(zip(("bias_cols", "bias_vals"), slots((12, 2.0)))), expect=("persistence", "boost_overturns_argmax")),
    BiasBeamCase("ended_keeps_sum", "plain", 1, 2, 50, 4, 0, 6, [(2, fixed({1: row(54, {10: 4.0, 11: 2.0})}))],
                 state0=[bhyp([12, 1], -4.0, fin=True, bsum=2.0), bhyp([5, 6], -1.0)],
                 **dict(zip(("bias_cols", "bias_vals"), slots((12, 2.0)))), expect=("ended_competes_with_sum",)),
    BiasBeamCase("lp_and_bias", "plain", 1, 3, 50, 4, 0, 8,
                 [(5, fixed({0: row(54, {10: 4.0, 11: 3.0}), 2: row(54, {12: 4.0})}))],
                 state0=[bhyp([5, 6, 7, 8, 9], -1.5, bsum=0.5), bhyp([5, 1], -2.0, fin=True, bsum=-0.25),
                         bhyp([9, 8, 7, 6, 5], -3.0)],
                 rules=(0, 0, 1.0), **dict(zip(("bias_cols", "bias_vals"), slots((11, 0.75), (5, 0.5), (1, -0.25)))),
                 expect=("lp_reorders_with_bias",)),
    BiasBeamCase("ban_beats_bias", "plain", 1, 2, 50, 4, 0, 6,
                 [(3, fixed({0: row(54, {6: 4.0, 10: 3.0, 11: 2.0}), 1: row(54, {12: 3.5, 13: 2.0})}))],
                 state0=[bhyp([5, 6, 5], -1.0), bhyp([7, 8, 9], -1.25)], rules=(2, 0, 0.0),
                 **dict(zip(("bias_cols", "bias_vals"), slots((6, 3.0)))), expect=("rule_ban_wins_over_bias",)),
    BiasBeamCase("end_bias_minlen", "plain", 1, 2, 50, 4, 0, 6, [(1, fixed({0: row(54, {1: 4.0, 10: 3.0, 11: 2.0})}))],
                 state0=[bhyp([5], -1.0), None], rules=(0, 4, 0.0),
                 **dict(zip(("bias_cols", "bias_vals"), slots((1, 2.0)))), expect=("end_bias_below_min_len",)),
    BiasBeamCase("duplicate_id", "plain", 1, 2, 50, 4, 0, 4, [(0, fixed({0: row(54, {10: 3.0, 11: 4.0, 12: 3.5})}))],
                 **dict(zip(("bias_cols", "bias_vals"), slots((10, 2.0), (13, 0.5), (10, NINF)))),
                 expect=("duplicate_lowest_slot",)),
    BiasBeamCase("script_batch", "plain", 3, 5, 50, 4, 4, 4, [(p, _batch_rows) for p in range(4)], rules=(2, 2, 0.75),
                 **dict(zip(("bias_cols", "bias_vals"),
                            per_caption([(10, 1.0), (41, NINF), (51, 0.5)], [], [(END, -1.5), (12, 0.75), (55, 1.25)]))),
                 expect=("scripted", "batch_3", "caption_all_empty", "list_per_caption", "width_5", "pointer_with_facts")),
]
BEAM_BY_NAME = {c.name: c for c in BEAM}


def _bias_of(case, b):
    return ref.bias_row(case.Vx, case.bias_cols[b], case.bias_vals[b])


def _picked(case, trace):
    """(step dict, row, parent row, column) of every live expansion."""
    for t in trace:
        for r, c in enumerate(t["info"]["tok"]):
            if c >= 0:
                yield t, r, (r // case.beam) * case.beam + int(t["info"]["parent"][r]), int(c)


def _row_max_banned(case, trace):
    return any(_bias_of(case, r // case.beam)[int(np.argmax(x))] == NINF for t in trace for r, x in t["rows"].items())


def _overturns(case, trace):
    """Some caption's first winner is not the candidate the unbiased key would have put first."""
    return any(p[0] is not None and (p[0][0], p[0][1]) != u[0]
               for t in trace for p, u in zip(t["info"]["picks"], t["info"]["unbiased_picks"]))


def _persistence(case, trace):
    local = run_beam(case, step_local=True)
    last, llast = trace[-1], local[-1]
    carried_wins = any(last["st"]["bsum"][p] != 0 for _, _, p, _ in _picked(case, [last]))
    return len(trace) == 2 and carried_wins and not np.array_equal(last["out"]["seq"], llast["out"]["seq"])


def _ended_with_sum(case, trace):
    t = trace[0]
    for b, picks in enumerate(t["info"]["picks"]):
        for h, p in enumerate(picks):
            if p is None:
                continue
            src = b * case.beam + p[0]
            if t["st"]["fin"][src] and t["st"]["bsum"][src] > 0:
                losers_best = max(q[2] for q in picks if q is not None and q != p)
                return t["st"]["cum"][src] < losers_best - ref.MARGIN and t["out"]["bsum"][b * case.beam + h] == t["st"]["bsum"][src]
    return False


def _lp_reorders(case, trace):
    flat = BiasBeamCase(**{**case.__dict__, "rules": (case.rules[0], case.rules[1], 0.0)})
    other = run_beam(flat)
    return case.rules[2] != 0 and not np.array_equal(trace[0]["out"]["seq"], other[0]["out"]["seq"])


def _ban_wins(case, trace):
    for t in trace:
        for r, x in t["rows"].items():
            b = _bias_of(case, r // case.beam)
            top = int(np.argmax(x.astype(np.float64) + np.where(np.isfinite(b), b, -100)))
            if top in t["info"]["banned"].get(r, ()) and b[top] > 0 and \
                    not any(p == r and c == top for _, _, p, c in _picked(case, [t])):
                return True
    return False


BEAM_TAGS = {
    "vx3": lambda c, tr: c.Vx == 3,
    "c_1": lambda c, tr: len(c.bias_cols[0]) == 1,
    "c_64": lambda c, tr: len(c.bias_cols[0]) == 64 and min(c.bias_cols[0]) >= 0,
    "width_1": lambda c, tr: c.beam == 1,
    "width_2": lambda c, tr: c.beam == 2,
    "width_5": lambda c, tr: c.beam == 5,
    "width_8": lambda c, tr: c.beam == 8,
    "batch_3": lambda c, tr: c.B == 3,
    "list_per_caption": lambda c, tr: c.B > 1 and c.bias_cols[0] != c.bias_cols[1],
    "caption_all_empty": lambda c, tr: any(max(l) < 0 for l in c.bias_cols) and any(max(l) >= 0 for l in c.bias_cols),
    "ban_row_max": _row_max_banned,
    "dead_slot_from_bias": lambda c, tr: tr[0]["info"]["dead"].any() and c.Vx > c.beam,
    "boost_overturns_argmax": _overturns,
    "bias_last_column": lambda c, tr: any(c.Vx - 1 in l for l in c.bias_cols),
    "bias_in_single_column_chunk": lambda c, tr: c.Vx % 1024 == 1 and any(col == c.Vx - 1 for _, _, _, col in _picked(c, tr)),
    "pointer_with_facts": lambda c, tr: c.F > 0 and any(col >= c.V and _bias_of(c, r // c.beam)[col] != 0
                                                        for _, r, _, col in _picked(c, tr)),
    "pointer_without_facts": lambda c, tr: c.F == 0 and any(col >= c.V and _bias_of(c, r // c.beam)[col] != 0
                                                            for _, r, _, col in _picked(c, tr)),
    "chunks_64": lambda c, tr: c.beam == 8 and c.Vx == 65536,
    "chunks_65": lambda c, tr: c.beam == 2 and c.Vx == 66560 and any(col >= 65536 for _, _, _, col in _picked(c, tr)),
    "persistence": _persistence,
    "ended_competes_with_sum": _ended_with_sum,
    "lp_reorders_with_bias": _lp_reorders,
    "rule_ban_wins_over_bias": _ban_wins,
    "end_bias_below_min_len": lambda c, tr: c.rules[1] > tr[0]["pos"] and _bias_of(c, 0)[c.end] > 0 and
    int(np.argmax(tr[0]["rows"][0])) == c.end and not any(col == c.end for _, _, _, col in _picked(c, tr)),
    "end_penalised": lambda c, tr: any(_bias_of(c, b)[c.end] < 0 for b in range(c.B)),
    "duplicate_lowest_slot": lambda c, tr: any(
        l.count(col) == 2 and v[l.index(col)] > 0 and v[len(l) - 1 - l[::-1].index(col)] == NINF and
        any(pc == col for _, _, _, pc in _picked(c, tr)) for l, v in zip(c.bias_cols, c.bias_vals) for col in set(l)),
    "scripted": lambda c, tr: 3 <= len(tr) <= 5 and tr[-1]["pos"] == c.max_len - 1 and tr[0]["pos"] == 0,
}
BEAM_TAGS_REQUIRED = set(BEAM_TAGS)


# --------------------------------------------------------------------------------------------------------- sampling
@dataclass
class BiasSampleCase(SC.SampleCase):
    bias_cols: list = None
    bias_vals: list = None


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


def _edge_rows(col):
    """The column `col` is third from the top: a boost of 2.5 makes it the row's best by a full point."""
    def fn(case, st, live, pos):
        return {r: row(case.Vx, {50 + r: 4.0, 900 + r: 3.5, col: 2.5}, -14.0) for r in live}
    return fn


def _topp_rows(case, st, live, pos):
    return {r: row(case.Vx, {50 + r: 4.0, 60 + r: 3.0, 70 + r: 2.0, 100: 0.0, 101: -0.0}, -14.0) for r in live}


SAMPLE = [
    BiasSampleCase("s_vx5_topk", 1, 3, 3, 1, 1, 4,
                   [(0, fixed({0: np.float32([0, 1, 2, 3, 4]), 1: np.float32([0, 1, 2, 4, 3]), 2: np.float32([4, 1, 2, 3, 0])}))],
                   top_k=2, **dict(zip(("bias_cols", "bias_vals"), slots((2, 1.5)))),
                   expect=("vx5", "rows_per_sample_3", "boost_crosses_topk")),
    BiasSampleCase("s_4097_topp", 2, 1, 4090, 4, 3, 4, [(0, _topp_rows)], top_p=0.7, seed=5,
                   **dict(zip(("bias_cols", "bias_vals"), per_caption([(70, 1.5), (100, 0.0), (101, -0.0)],
                                                                      [(71, 1.5), (100, -0.0), (4096, 0.0)]))),
                   expect=("vx4097", "rows_per_sample_1", "boost_crosses_topp", "zero_values")),
    BiasSampleCase("s_16384", 1, 3, 16370, 8, 6, 4, [(0, _edge_rows(16383))], top_k=1, seed=3,
                   **dict(zip(("bias_cols", "bias_vals"), slots((16383, 2.5)))), expect=("bias_last_of_ng4",)),
    BiasSampleCase("s_16385", 1, 3, 16371, 8, 6, 4, [(0, _edge_rows(16384))], top_k=1, seed=3,
                   **dict(zip(("bias_cols", "bias_vals"), slots((16384, 2.5)))), expect=("bias_first_of_ng16",)),
    BiasSampleCase("s_65536", 2, 1, 65520, 8, 8, 4, [(1, SC._big_rows)], T=0.75, top_k=50, top_p=0.85, seed=11,
                   state0=[srow([5]), srow([6])],
                   **dict(zip(("bias_cols", "bias_vals"), slots((65535, NINF), (40000, 1.5), (4099, -1.0), B=2))),
                   expect=("vx65536", "ban_on_max")),
    BiasSampleCase("s_forced", 1, 3, 3, 1, 1, 4, [(0, fixed({r: np.float32([3, 1.5, 1, 2, 2.5]) for r in range(3)}))],
                   **dict(zip(("bias_cols", "bias_vals"), slots((0, NINF), (1, NINF), (2, NINF), (4, NINF)))),
                   expect=("forced_draw", "ban_on_max")),
    BiasSampleCase("s_ban_and_bias", 1, 3, 3, 1, 1, 5, [(3, fixed({r: np.float32([3, 1.5, 1, 2, 2.5]) for r in range(3)}))],
                   top_k=1, rules=(1, 0), state0=[srow([0, 3, 4])] * 3,
                   **dict(zip(("bias_cols", "bias_vals"), slots((3, 4.0), (2, 1.0)))),
                   expect=("rule_ban_and_bias",)),
    BiasSampleCase("s_script", 2, 3, 4090, 4, 3, 4, [(p, SC._peaked_rows(110, npeaks=4)) for p in range(4)], T=0.875,
                   top_k=6, top_p=0.8, seed=77, rules=(2, 2),
                   **dict(zip(("bias_cols", "bias_vals"), per_caption([(END, -2.0), (4096, 1.0)], [(4096, NINF), (7, 0.5)]))),
                   expect=("scripted", "rows_per_sample_3", "end_penalised")),
]
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE}


def _kept(tr):
    return [(t, r, k) for t in tr for r, k in t["info"]["kept"].items()]


def _crosses(case, tr, knob):
    """A boosted column is kept that the unbiased selection drops, with the named truncation on alone."""
    for t, r, k in _kept(tr):
        b = ref.bias_row(case.Vx, case.bias_cols[r // case.rps], case.bias_vals[r // case.rps])
        moved = k & ~t["info"]["kept_unbiased"][r] & (b > 0)
        if moved.any() and knob:
            return True
    return False


def _ban_on_max(case, tr):
    return any(ref.bias_row(case.Vx, case.bias_cols[r // case.rps], case.bias_vals[r // case.rps])[t["info"]["smax"][r]] == NINF
               and t["info"]["tok"][r] != t["info"]["smax"][r] for t, r, _ in _kept(tr))


def _rule_ban_and_bias(case, tr):
    for t, r, k in _kept(tr):
        b = ref.bias_row(case.Vx, case.bias_cols[r // case.rps], case.bias_vals[r // case.rps])
        ban = t["info"]["banned"][r]
        if any(b[c] > 0 for c in ban) and any(b[c] > 0 and c not in ban for c in range(case.Vx)) and \
                t["info"]["tok"][r] not in ban and b[t["info"]["tok"][r]] > 0:
            return True
    return False


SAMPLE_TAGS = {
    "vx5": lambda c, tr: c.Vx == 5,
    "vx4097": lambda c, tr: c.Vx == 4097,
    "vx65536": lambda c, tr: c.Vx == 65536,
    "rows_per_sample_1": lambda c, tr: c.rps == 1 and c.B > 1,
    "rows_per_sample_3": lambda c, tr: c.rps == 3,
    "boost_crosses_topk": lambda c, tr: _crosses(c, tr, 0 < c.top_k < c.Vx and c.top_p == 1),
    "boost_crosses_topp": lambda c, tr: _crosses(c, tr, c.top_k == 0 and c.top_p < 1),
    "zero_values": lambda c, tr: any(v == 0 and np.signbit(v) for l in c.bias_vals for v in l) and
    any(v == 0 and not np.signbit(v) for l in c.bias_vals for v in l),
    "bias_last_of_ng4": lambda c, tr: c.Vx == 16384 and all(t["info"]["tok"][r] == 16383 != t["info"]["smax"][r] for t, r, _ in _kept(tr)),
    "bias_first_of_ng16": lambda c, tr: c.Vx == 16385 and all(t["info"]["tok"][r] == 16384 != t["info"]["smax"][r] for t, r, _ in _kept(tr)),
    "ban_on_max": _ban_on_max,
    "forced_draw": lambda c, tr: all(len(t["info"]["allowed"][r]) == 1 for t, r, _ in _kept(tr)),
    "rule_ban_and_bias": _rule_ban_and_bias,
    "end_penalised": lambda c, tr: any(v < 0 for l, vs in zip(c.bias_cols, c.bias_vals) for col, v in zip(l, vs) if col == c.end),
    "scripted": lambda c, tr: 3 <= len(tr) <= 5 and tr[-1]["pos"] == c.max_len - 1 and tr[0]["pos"] == 0,
}
SAMPLE_TAGS_REQUIRED = set(SAMPLE_TAGS)
