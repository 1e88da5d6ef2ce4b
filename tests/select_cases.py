"""Hand-built cases of the beam and sampled token selection (csrc/decode_select.hip, csrc/sample.hip): raw score rows,
the hypothesis / row state going in and the entry point's knobs.  A case is one selection step or a scripted run of
steps; tests/select_ref.py says what must come out, tests/test_select_cases_cpu.py checks the table (every case is
decidable, every `expect` tag is true of the reference's own result, every kernel instantiation is reached) and
tests/test_select_envelope_gpu.py runs it on the device.

Token ids are the same everywhere: <pad> = 0, <end> = 1, <start> = 2.  Columns are words [0, V), entity pointers
[V, V + K), fact pointers [V + K, V + K + F).  Scores are finite with |s| <= 16."""
import functools
from dataclasses import dataclass

import numpy as np

import select_ref as ref

PAD, END, START = 0, 1, 2
D = 8                                   # model width of the harness: free for the selection kernels
NEG = float("-inf")


# ------------------------------------------------------------------------------------------------ embedding tables
def tables(case):
    """Exact and telling tables: emb_scale = 2 and small dyadic values that differ by table, caption, row and position,
    so that 2 * row + pe is exactly representable and a row from the wrong table, caption or position is a mismatch."""
    c = np.arange(D, dtype=np.float64)
    t = dict(emb_scale=2.0)
    t["word_emb"] = (np.arange(case.V, dtype=np.float64)[:, None] * 8 + c).astype(np.float32)
    bk = (np.arange(case.B)[:, None] * 32 + np.arange(case.K)[None, :]).astype(np.float64)
    t["ee"] = (-(bk[..., None] * 8 + c + 0.5)).astype(np.float32)
    bf = (1024 + np.arange(case.B)[:, None] * 32 + np.arange(case.F)[None, :]).astype(np.float64)
    t["fe"] = (-(bf[..., None] * 8 + c + 0.25)).astype(np.float32) if case.F else None
    t["pe"] = ((np.arange(case.max_len, dtype=np.float64)[:, None] + 1) / 16 + 0 * c).astype(np.float32)
    return t


# -------------------------------------------------------------------------------------------------------- score rows
def row(Vx, peaks, base=-8.0):
    """A score row: a low background on a 0.5 grid (base .. base - 2) and the given {column: score} peaks."""
    c = np.arange(Vx)
    x = (base - 0.5 * ((c * 7) % 5)).astype(np.float32)
    for col, v in peaks.items():
        x[col] = v
    return x


def fixed(rows):
    return lambda case, st, live, pos: rows


def scripted(seed, npeaks=6, end_from=1, end_score=4.5):
    """Rows of a scripted run, made for whichever rows are live: `npeaks` peaks on a 1/8 grid at columns spread over
    words, entities and facts, from a generator seeded by (seed, step, row); <end> is among the best from step
    `end_from` on for the rows r with (r + step) even."""
    def fn(case, st, live, pos):
        out = {}
        for r in live:
            g = np.random.default_rng([seed, pos, r])
            cols = g.choice(np.arange(3, case.Vx), size=npeaks, replace=False)
            cols[0] = case.V + g.integers(case.K)
            if case.F:
                cols[1] = case.V + case.K + g.integers(case.F)
            peaks = {int(c): float(g.integers(0, 40)) / 8 for c in cols}
            peaks[END] = end_score - (r % 3) * 0.25 if pos >= end_from and (r + pos) % 2 == 0 else -2.0
            out[r] = row(case.Vx, peaks)
        return out
    return fn


# ------------------------------------------------------------------------------------------------------------- beam
@dataclass
class BeamCase:
    name: str
    form: str                           # "plain" | "diverse" | "forced"
    B: int
    beam: int
    V: int
    K: int
    F: int
    max_len: int
    steps: list                         # [(pos, rows_fn(case, state, live rows, pos) -> {row: fp32 (Vx,)})]
    state0: object = None               # state going into the first step: None = the start of a search, or hyps
    rules: tuple = None                 # (no_repeat_ngram_size, min_len, length penalty alpha) or None
    groups: int = 1
    lam: float = 0.0
    force: list = None                  # (B, 8) forced columns, -1 = empty
    expect: tuple = ()
    ld_pad: int = 5                     # scores_ld = V + ld_pad: poisoned columns after every row's words
    d: int = D
    end: int = END
    pad: int = PAD
    start: int = START

    @property
    def R(self):
        return self.B * self.beam

    @property
    def Vx(self):
        return self.V + self.K + self.F

    def kernels(self):
        rules = self.rules is not None
        return {("dec_select_beam_kernel", rules, self.form == "diverse", self.form == "forced"),
                ("dec_beam_partial_kernel", rules, self.form == "forced")}


def beam_state(case):
    """The state going into the case's first step.  state0 None: the start of a search (one live hypothesis per group,
    the unused slots count as done); else a list of R entries, None (an unused slot) or dict(seq, cum, fin, met)."""
    R, L, k = case.R, case.max_len, case.beam
    st = dict(cum=np.full(R, NEG), fin=np.zeros(R, np.int32), len=np.zeros(R, np.int32), met=np.zeros(R, np.int32),
              seq=np.full((R, L), case.pad, np.int64), anc=np.zeros((R, L), np.int32),
              cap=np.full((R, L), case.start, np.int64) if case.F else None)
    if case.state0 is None:
        kg = k // (case.groups if case.form == "diverse" else 1)
        st["cum"].reshape(case.B, k)[:, ::kg] = 0.0
    else:
        pos = case.steps[0][0]
        for r, h in enumerate(case.state0):
            if h is None:
                continue
            seq = h["seq"]
            assert len(seq) <= pos and (h.get("fin", False) == (seq[-1] == case.end if seq else False))
            st["cum"][r], st["fin"][r], st["met"][r] = h["cum"], int(h.get("fin", False)), h.get("met", 0)
            st["len"][r] = len(seq)
            st["seq"][r, :len(seq)] = seq
            st["anc"][r, :pos] = (r // k) * k + (r + np.arange(pos)) % k
            if st["cap"] is not None:
                n = min(len(seq), L - 1) - int(h.get("fin", False))
                st["cap"][r, 1:1 + n] = seq[:n]
    st["n_done"] = int(sum(1 for r in range(R) if st["fin"][r] or st["cum"][r] == NEG))
    return st


@functools.lru_cache(maxsize=None)
def beam_trace(name, lam=None):
    """The reference's run of a case: [dict(pos, st, rows, out, info)] step by step (lam: another diversity penalty)."""
    case = BEAM_BY_NAME[name]
    if lam is not None:
        case = BeamCase(**{**case.__dict__, "lam": lam})
    t, st, trace = tables(case), beam_state(case), []
    for pos, fn in case.steps:
        live = [r for r in range(case.R) if not st["fin"][r] and st["cum"][r] != NEG]
        rows = fn(case, st, live, pos)
        out, info = ref.beam_step(case, st, rows, pos, t)
        trace.append(dict(pos=pos, st=st, rows=rows, out=out, info=info))
        st = out
    return trace


def hyp(seq, cum, fin=False, met=0):
    return dict(seq=list(seq), cum=cum, fin=fin, met=met)


NOF = [-1] * 8


def _forced_script_rows(case, st, live, pos):
    """<end> is every row's best column from the start; the forced columns 51 and 55 are far down."""
    return {r: row(case.Vx, {END: 5.0, 10 + pos: 3.0 - 0.25 * (r % 3), 20 + r % 3: 2.0 + 0.125 * pos, 51: 1.5, 55: 1.0})
            for r in live}


def _force(*cols):
    return list(cols) + [-1] * (8 - len(cols))


def _big8_rows(case, st, live, pos):
    out = {}
    for r in live:
        j = r % 8
        out[r] = row(case.Vx, {j * 8000 + 1023: 5.0 - 0.25 * j, 65535 - j: 3.0 + 0.4375 * j, 1024 * j + 1024: 3.0,
                               63 * 1024 + j: 2.0 + 0.25 * j})
    return out


def _big2_rows(case, st, live, pos):
    out = {}
    for r in live:
        x = row(case.Vx, {66559: 6.0, 65536: 5.5, 0: 5.0} if r % 2 == 0 else {5: 5.0, 66000: 4.0})
        x[65600:65700] = 3.0                # mass in the 65th chunk: the second trip of the per-lane lse loop
        out[r] = x
    return out


BEAM = [
    BeamCase("dead_step0", "plain", 1, 5, 2, 1, 0, 4, [(0, fixed({0: np.float32([0.5, -1.0, 1.5])}))],
             expect=("dead_slot_step0", "end_chosen", "n_done_moves", "pointer_entity")),
    BeamCase("dead_later", "plain", 1, 5, 2, 1, 0, 4, [(2, fixed({0: np.float32([1.0, 0.0, -1.0])}))],
             state0=[hyp([0, 0], -1.0), hyp([0, 1], -0.5, fin=True), None, None, None],
             expect=("dead_slot_later", "ended_outranks_all")),
    BeamCase("beam1", "plain", 3, 1, 50, 4, 0, 4,
             [(0, fixed({0: row(54, {7: 3.0, 8: 2.0}), 1: row(54, {52: 3.0}), 2: row(54, {1: 3.0, 9: 2.5})}))],
             expect=("end_chosen",)),
    BeamCase("ties_1023", "plain", 3, 2, 1015, 8, 0, 4,
             [(0, fixed({0: row(1023, {100: 4.0, 700: 4.0}), 2: row(1023, {5: 4.0, 300: 3.0, 900: 3.0, 1022: 3.0}),
                         4: row(1023, {1022: 4.0, 0: 3.5})}))],
             expect=("tie_columns_one_row", "pointer_entity")),
    BeamCase("tie_chunk_1025", "plain", 1, 2, 1016, 5, 4, 4, [(0, fixed({0: row(1025, {1023: 4.0, 1024: 4.0})}))],
             expect=("tie_straddles_chunk", "single_column_chunk", "pointer_fact")),
    BeamCase("tie_parents_1024", "plain", 1, 2, 1000, 24, 0, 4,
             [(1, fixed({0: row(1024, {10: 4.0, 20: 3.0}), 1: row(1024, {10: 4.0, 20: 3.0})}))],
             state0=[hyp([5], -1.0), hyp([6], -1.0)], expect=("tie_between_parents",)),
    BeamCase("ended_pushed_out", "plain", 1, 2, 50, 4, 0, 4, [(2, fixed({0: row(54, {10: 4.0, 11: 3.5})}))],
             state0=[hyp([5, 6], -0.1), hyp([7, 1], -9.0, fin=True)], expect=("ended_pushed_out", "n_done_moves")),
    BeamCase("lp_order", "plain", 1, 3, 50, 4, 0, 8,
             [(5, fixed({0: row(54, {10: 4.0, 11: 3.0}), 2: row(54, {12: 4.0})}))],
             state0=[hyp([5, 6, 7, 8, 9], -1.5), hyp([5, 1], -2.0, fin=True), hyp([9, 8, 7, 6, 5], -3.0)],
             rules=(0, 0, 1.0), expect=("lp_reorders",)),
    BeamCase("carry_next_to_live", "plain", 3, 2, 50, 4, 4, 6,
             [(3, fixed({0: row(58, {10: 4.0, 11: 3.0}), 1: row(58, {12: 4.0, 55: 3.75}), 4: row(58, {1: 4.0, 51: 3.0})}))],
             state0=[hyp([5, 6, 7], -1.0), hyp([5, 6, 8], -1.25), hyp([5, 1], -0.5, fin=True), hyp([6, 7, 1], -0.75, fin=True),
                     hyp([9, 9, 9], -2.0), hyp([3, 1], -2.5, fin=True)],
             expect=("carry_copy_next_to_live", "end_chosen", "n_done_moves")),
    BeamCase("ngram_ban", "plain", 1, 2, 50, 4, 0, 6,
             [(3, fixed({0: row(54, {6: 4.0, 10: 3.0, 11: 2.0}), 1: row(54, {12: 3.5, 13: 2.0})}))],
             state0=[hyp([5, 6, 5], -1.0), hyp([7, 8, 9], -1.25)], rules=(2, 0, 0.0),
             expect=("ngram_ban_removes_winner",)),
    BeamCase("minlen_ban", "plain", 1, 2, 50, 4, 0, 6, [(1, fixed({0: row(54, {1: 4.0, 10: 3.0, 11: 2.0})}))],
             state0=[hyp([5], -1.0), None], rules=(0, 4, 0.0), expect=("minlen_ban_removes_winner",)),
    BeamCase("ban_chunk1_seam", "plain", 1, 2, 2040, 8, 8, 6,
             [(2, fixed({0: row(2056, {1500: 5.0, 300: 4.5, 2040: 4.0, 2039: 3.0, 2049: 2.5}),
                         1: row(2056, {2055: 4.0, 2048: 3.0})}))],
             state0=[hyp([1500, 300], -1.0), hyp([3, 4], -3.0)], rules=(1, 0, 0.0),
             expect=("ban_in_chunk_gt0", "pointer_entity", "pointer_fact", "seam_inside_chunk")),
    BeamCase("v65536_beam8", "plain", 2, 8, 65520, 8, 8, 4, [(1, _big8_rows)],
             state0=[hyp([10 + j], -0.125 * j) for j in range(8)] + [hyp([3], 0.0)] + [None] * 7,
             expect=("chunks_64",)),
    BeamCase("v66560_beam2", "plain", 1, 2, 66550, 10, 0, 4, [(1, _big2_rows)],
             state0=[hyp([10], -0.5), hyp([11], -0.25)], expect=("chunks_65", "pointer_entity")),
    BeamCase("script_plain", "plain", 3, 2, 50, 4, 4, 4, [(p, scripted(100)) for p in range(4)],
             expect=("scripted", "end_chosen")),
    BeamCase("script_rules", "plain", 2, 5, 50, 4, 0, 5, [(p, scripted(106)) for p in range(5)], rules=(2, 2, 0.75),
             expect=("scripted", "end_chosen")),
    # ---- diverse
    BeamCase("div_penalty", "diverse", 1, 4, 50, 4, 0, 4,
             [(0, fixed({0: row(54, {10: 3.0, 11: 2.5, 12: 2.0}), 2: row(54, {10: 3.0, 11: 2.5, 12: 2.0})}))],
             groups=2, lam=0.75, expect=("div_penalty_changes_choice",)),
    BeamCase("div_twice", "diverse", 1, 6, 50, 4, 0, 4,
             [(0, fixed({r: row(54, {10: 3.0, 11: 2.5, 12: 2.0, 13: 1.0}) for r in (0, 2, 4)}))],
             groups=3, lam=0.75, expect=("div_penalised_twice", "div_penalty_changes_choice")),
    BeamCase("div_dead", "diverse", 1, 8, 2, 1, 0, 4,
             [(0, fixed({0: np.float32([0.5, -1.0, 1.5]), 4: np.float32([0.5, -1.0, 1.5])}))],
             groups=2, lam=0.5, expect=("div_dead_slot",)),
    BeamCase("div_ended_rules", "diverse", 1, 4, 50, 4, 4, 6,
             [(2, fixed({0: row(58, {10: 4.0, 11: 3.0}), 2: row(58, {10: 4.0, 56: 3.5})}))],
             state0=[hyp([5, 6], -1.0), hyp([7, 1], -1.25, fin=True), hyp([8, 9], -1.5), hyp([3, 1], -2.0, fin=True)],
             groups=2, lam=1.5, rules=(0, 0, 1.0), expect=("div_ended_in_group", "div_penalty_changes_choice")),
    BeamCase("script_diverse", "diverse", 2, 4, 50, 4, 4, 4, [(p, scripted(100, npeaks=4)) for p in range(4)],
             groups=2, lam=0.5, expect=("scripted",)),
    # ---- forced
    BeamCase("forced_far", "forced", 1, 3, 1100, 8, 0, 4,
             [(0, fixed({0: row(1108, {10: 4.0, 11: 3.0, 12: 2.0, 1090: -12.0})}))], force=[_force(1090)],
             expect=("forced_far_from_topk", "empty_bank_skipped", "rotation_wraps")),
    BeamCase("forced_turn", "forced", 1, 3, 50, 4, 0, 4,
             [(1, fixed({0: row(54, {10: 4.0, 11: 3.0}), 1: row(54, {12: 4.0, 20: 1.0}), 2: row(54, {13: 4.0, 20: 0.0})}))],
             state0=[hyp([20], -1.0, met=1), hyp([5], -0.5), hyp([6], -0.75)], force=[_force(20)],
             expect=("rotation_wraps",)),
    BeamCase("forced_two_slots", "forced", 1, 2, 50, 4, 0, 4, [(0, fixed({0: row(54, {10: 4.0, 7: 0.0})}))],
             force=[_force(7, 7)], expect=("two_slots_one_id", "empty_bank_skipped")),
    BeamCase("forced_turn_rules", "forced", 1, 3, 50, 4, 4, 6,
             [(1, fixed({0: row(58, {10: 4.0, 11: 3.0}), 1: row(58, {12: 4.0, 56: 3.5}), 2: row(58, {13: 4.0, 56: 0.0})}))],
             state0=[hyp([56], -1.0, met=1), hyp([5], -0.5), hyp([6], -0.75)], force=[_force(56)], rules=(1, 3, 1.0),
             expect=("rotation_wraps", "forced_pointer")),
    BeamCase("script_forced", "forced", 2, 3, 50, 4, 4, 4, [(p, _forced_script_rows) for p in range(4)],
             force=[_force(51, 55), NOF],
             expect=("scripted", "end_closed_unmet", "end_open_met", "forced_pointer", "rotation_wraps")),
]
BEAM_BY_NAME = {c.name: c for c in BEAM}


def _picked(trace):
    """(step dict, row, parent row, column) of every live expansion."""
    for t in trace:
        k = len(t["st"]["cum"]) // max(1, len(t["info"]["picks"]) + len(t["info"]["carried"]))
        for r, c in enumerate(t["info"]["tok"]):
            if c >= 0:
                yield t, r, (r // k) * k + int(t["info"]["parent"][r]), int(c)


def _tag_div_changes(case, trace):
    other = beam_trace(case.name, lam=0.0)
    return any((a["info"]["tok"] != b["info"]["tok"]).any() for a, b in zip(trace, other))


def _tag_lp_reorders(case, trace):
    t = trace[0]
    k = case.beam
    lp = ref.lp_table(case.rules[2], case.max_len).double().numpy()
    cands = []
    for j in range(k):
        cum = t["st"]["cum"][j]
        if cum == NEG:
            continue
        if t["st"]["fin"][j]:
            cands.append((cum / lp[t["st"]["len"][j]], cum, j, 0))
        else:
            s = cum + t["rows"][j].astype(np.float64) - ref.lse64(t["rows"][j])
            cands += [(s[c] / lp[t["pos"] + 1], s[c], j, c) for c in range(case.Vx)]
    by_key = {c[2:] for c in sorted(cands, key=lambda c: -c[0])[:k]}
    by_cum = {c[2:] for c in sorted(cands, key=lambda c: -c[1])[:k]}
    ended_short = any(t["st"]["fin"][j] and t["st"]["len"][j] < t["pos"] for j in range(k))
    return by_key != by_cum and ended_short


def _visits(trace):
    return [v for t in trace for v in t["info"].get("banks_visited", [])]


def _tie(trace, pred):
    """Some step where two winners (or a winner and the first loser) share a key exactly and pred(a, b) holds for the
    (slot, column) pairs a before b."""
    for t in trace:
        for picks in t["info"]["picks"]:
            got = [p for p in picks if p is not None]
            for a, b in zip(got, got[1:]):
                if a[2] == b[2] and pred(a, b):
                    return True
    return False


BEAM_TAGS = {
    "dead_slot_step0": lambda c, tr: tr[0]["pos"] == 0 and c.Vx == 3 and tr[0]["info"]["dead"].any(),
    "dead_slot_later": lambda c, tr: tr[0]["pos"] > 0 and tr[0]["info"]["dead"].any(),
    "end_chosen": lambda c, tr: any(col == c.end for _, _, _, col in _picked(tr)),
    "n_done_moves": lambda c, tr: any(t["out"]["n_done"] != t["st"]["n_done"] for t in tr),
    "pointer_entity": lambda c, tr: any(t["info"]["next_mask"][r] == 1 for t, r, _, _ in _picked(tr)),
    "pointer_fact": lambda c, tr: any(t["info"]["next_mask"][r] == 2 for t, r, _, _ in _picked(tr)),
    "ended_outranks_all": lambda c, tr: tr[0]["info"]["picks"][0][0][1] == 0 and bool(
        tr[0]["st"]["fin"][tr[0]["info"]["picks"][0][0][0]]),
    "ended_pushed_out": lambda c, tr: tr[0]["st"]["fin"].sum() > 0 and tr[0]["out"]["fin"].sum() == 0,
    "lp_reorders": _tag_lp_reorders,
    "carry_copy_next_to_live": lambda c, tr: len(tr[0]["info"]["carried"]) > 0 and len(tr[0]["info"]["picks"]) > 0,
    "tie_columns_one_row": lambda c, tr: _tie(tr, lambda a, b: a[0] == b[0] and a[1] < b[1]),
    "tie_straddles_chunk": lambda c, tr: _tie(tr, lambda a, b: a[0] == b[0] and a[1] // 1024 != b[1] // 1024),
    "tie_between_parents": lambda c, tr: _tie(tr, lambda a, b: a[0] < b[0] and a[1] == b[1]),
    "single_column_chunk": lambda c, tr: c.Vx % 1024 == 1 and any(col == c.Vx - 1 for _, _, _, col in _picked(tr)),
    "ngram_ban_removes_winner": lambda c, tr: c.rules[0] > 0 and any(
        int(np.argmax(x)) in t["info"]["banned"][r] and int(np.argmax(x)) != c.end for t in tr for r, x in t["rows"].items()),
    "minlen_ban_removes_winner": lambda c, tr: c.rules[1] > 0 and any(
        int(np.argmax(x)) == c.end and c.end in t["info"]["banned"][r] for t in tr for r, x in t["rows"].items()),
    "ban_in_chunk_gt0": lambda c, tr: any(
        int(np.argmax(x)) >= 1024 and int(np.argmax(x)) in t["info"]["banned"][r] for t in tr for r, x in t["rows"].items()),
    "seam_inside_chunk": lambda c, tr: c.V % 1024 != 0 and c.V < 2048 and c.Vx == 2048 + c.K,
    "chunks_64": lambda c, tr: c.beam == 8 and c.Vx == 65536 and c.R <= 16,
    "chunks_65": lambda c, tr: c.beam == 2 and c.Vx == 66560 and any(col >= 65536 for _, _, _, col in _picked(tr)),
    "scripted": lambda c, tr: 3 <= len(tr) <= 5 and tr[-1]["pos"] == c.max_len - 1 and tr[0]["pos"] == 0,
    "div_penalty_changes_choice": _tag_div_changes,
    "div_penalised_twice": lambda c, tr: any(max(n.values(), default=0) >= 2 for t in tr for n in t["info"]["counts"]),
    "div_ended_in_group": lambda c, tr: any(t["st"]["fin"][r] and t["st"]["cum"][r] != NEG for t in tr for r in range(c.R)),
    "div_dead_slot": lambda c, tr: tr[0]["info"]["dead"].reshape(c.groups, -1).any(axis=1).all(),
    "forced_far_from_topk": lambda c, tr: any(
        col in c.force[r // c.beam] and t["info"]["rank_of_pick"][(r, col)] >= c.Vx // 2 for t, r, _, col in _picked(tr)),
    "two_slots_one_id": lambda c, tr: any(ref.bank_of(int(m)) == 2 for m in tr[0]["out"]["met"]) and c.force[0][0] == c.force[0][1],
    "empty_bank_skipped": lambda c, tr: any(
        (a - b) % (n + 1) != 1 for v, n in _visits(tr) for a, b in zip(v, v[1:])) or any(
        n > 0 and v and v[0] != n for v, n in _visits(tr)),
    "rotation_wraps": lambda c, tr: any(b >= a for v, n in _visits(tr) if n > 0 for a, b in zip(v, v[1:])),
    "forced_pointer": lambda c, tr: any(col >= c.V and col in c.force[r // c.beam] for _, r, _, col in _picked(tr)),
    "end_closed_unmet": lambda c, tr: any(
        int(np.argmax(x)) == c.end and ref.bank_of(int(t["st"]["met"][r])) < sum(f >= 0 for f in c.force[r // c.beam])
        and not any(p == r and col == c.end for tt, _, p, col in _picked([t])) for t in tr for r, x in t["rows"].items()),
    "end_open_met": lambda c, tr: any(
        col == c.end and sum(f >= 0 for f in c.force[r // c.beam]) > 0 and
        ref.bank_of(int(t["st"]["met"][p])) == sum(f >= 0 for f in c.force[r // c.beam]) for t, r, p, col in _picked(tr)),
}
BEAM_TAGS_REQUIRED = set(BEAM_TAGS)
BEAM_KERNELS = {("dec_select_beam_kernel", r, d, f) for r in (False, True) for d, f in ((False, False), (True, False), (False, True))} | \
               {("dec_beam_partial_kernel", r, f) for r in (False, True) for f in (False, True)}


# --------------------------------------------------------------------------------------------------------- sampling
@dataclass
class SampleCase:
    name: str
    B: int
    rps: int                            # rows_per_sample: samples per caption
    V: int
    K: int
    F: int
    max_len: int
    steps: list
    T: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    seed: int = 1234
    state0: object = None               # None: the start, or a list of R dict(out, fin)
    rules: tuple = None                 # (no_repeat_ngram_size, min_len) or None
    n_done0: int = None                 # None: the number of finished rows
    expect: tuple = ()
    ld_pad: int = 5
    d: int = D
    end: int = END
    pad: int = PAD
    start: int = START

    @property
    def R(self):
        return self.B * self.rps

    @property
    def Vx(self):
        return self.V + self.K + self.F

    def kernels(self):
        return {("dec_sample_kernel", 4 if self.Vx <= 16384 else 16, self.rules is not None)}


def sample_state(case):
    R, L = case.R, case.max_len
    st = dict(output=np.zeros((R, L), np.int64), finished=np.zeros(R, np.int32), log_prob=np.zeros((R, L)),
              cap_buf=np.full((R, L), case.start, np.int64) if case.F else None)
    for r, h in enumerate(case.state0 or []):
        st["output"][r, :len(h["out"])] = h["out"]
        st["finished"][r] = int(h.get("fin", False))
    st["n_done"] = int(st["finished"].sum()) if case.n_done0 is None else case.n_done0
    return st


@functools.lru_cache(maxsize=None)
def sample_trace(name):
    case = SAMPLE_BY_NAME[name]
    t, st, trace = tables(case), sample_state(case), []
    for pos, fn in case.steps:
        live = [r for r in range(case.R) if not st["finished"][r]] if st["n_done"] < case.R else []
        rows = fn(case, st, live, pos) if live else {}
        out, info = ref.sample_step(case, st, rows, pos, t)
        trace.append(dict(pos=pos, st=st, rows=rows, out=out, info=info))
        st = out
    return trace


def srow(out, fin=False):
    return dict(out=list(out), fin=fin)


def _flat_rows(seed, lo=-16, hi=16):
    """Flat rows on a 1/8 grid: the draw is the noise's."""
    def fn(case, st, live, pos):
        return {r: (np.random.default_rng([seed, pos, r]).integers(lo, hi + 1, case.Vx) / 8).astype(np.float32) for r in live}
    return fn


def _peaked_rows(seed, npeaks=8, base=-14.0, last=True):
    """Peaks on a 0.5 grid in [0, 6] over a background whose whole mass is negligible; the last column is one of them."""
    def fn(case, st, live, pos):
        out = {}
        for r in live:
            g = np.random.default_rng([seed, pos, r])
            cols = g.choice(np.arange(3, case.Vx - 1), size=npeaks, replace=False)
            vals = g.permutation(13)[:npeaks] / 2.0
            peaks = {int(c): float(v) for c, v in zip(cols, vals)}
            if last:
                peaks[case.Vx - 1] = 5.25
            peaks[END] = 5.75 if pos >= 2 and r % 2 == 0 else -2.0
            out[r] = row(case.Vx, peaks, base)
        return out
    return fn


def _big_rows(case, st, live, pos):
    out = {}
    for r in live:
        g = np.random.default_rng([5, pos, r])
        x = (g.integers(-128, -95, case.Vx) / 8).astype(np.float32)         # 33 levels, -16 .. -12
        for q, c in enumerate((0, 4099, 16384, 40000, 65519, 65535)):
            x[c] = 2.0 + 0.5 * ((q + r) % 6) + (1.5 if q == 5 else 0.0)
        out[r] = x
    return out


def _ban_max_rows(case, st, live, pos):
    """The row's maximum (16) is banned; of the allowed columns one holds -6.25, one -6.75, forty -7.25."""
    out = {}
    for r in live:
        top = int(st["output"][r, 0])
        peaks = {top: 16.0, 40 + r: -6.25, 80 + r: -6.75}
        peaks.update({1000 + 3 * q + r: -7.25 for q in range(40)})
        out[r] = row(case.Vx, peaks, base=-14.0)
    return out


_RUN = {7: 2.0, 100: 0.0, 101: -0.0, 4095: 0.0, 4096: -0.0}
SAMPLE = [
    SampleCase("topk_1", 1, 3, 3, 1, 1, 4, [(0, fixed({0: np.float32([0, 1, 2, 3, 4]), 1: np.float32([0, 1, 2, 4, 3]),
                                                         2: np.float32([4, 1, 2, 3, 0])}))], top_k=1,
               expect=("topk_1", "pointer_entity", "pointer_fact")),
    SampleCase("topk_vx_minus_1", 2, 1, 3, 1, 1, 4, [(0, fixed({0: np.float32([0, 1, 2, 3, -4]), 1: np.float32([-4, 1, 2, 3, 0])}))],
               top_k=4, expect=("topk_vx_minus_1",)),
    SampleCase("topk_off", 2, 1, 3, 1, 1, 4, [(0, fixed({0: np.float32([0, 1, 2, 3, -4]), 1: np.float32([-4, 1, 2, 3, 0])}))],
               top_k=5, expect=("topk_off",)),
    SampleCase("topk_run_zero", 2, 1, 4090, 4, 3, 4, [(0, fixed({0: row(4097, _RUN), 1: row(4097, {**_RUN, 7: -0.0, 9: 2.0})}))],
               top_k=3, seed=7, expect=("topk_run_all_kept_pm_zero", "seam_inside_quad", "vx_not_multiple_of_4")),
    SampleCase("topp_run_kept", 1, 3, 16370, 8, 6, 4,
               [(0, fixed({r: row(16384, {50 + r: 4.0, 16383: 3.0, 16369 + r: 3.0}, -14.0) for r in range(3)}))],
               top_p=0.7, seed=3, expect=("topp_run_all_kept", "seam_inside_quad", "last_of_ng4")),
    SampleCase("topp_run_dropped", 1, 3, 16371, 8, 6, 4,
               [(0, fixed({r: row(16385, {50 + r: 4.0, 16384: 3.0, 16370 + r: 3.0}, -14.0) for r in range(3)}))],
               top_p=0.56, seed=3, expect=("topp_run_all_dropped", "first_of_ng16", "vx_not_multiple_of_4")),
    SampleCase("topp_one", 2, 1, 3, 1, 1, 4, [(0, fixed({0: np.float32([0, 1, 2, 3, -4]), 1: np.float32([-4, 1, 2, 3, 0])}))],
               top_p=0.05, expect=("topp_one_kept",)),
    SampleCase("both_65536", 2, 1, 65520, 8, 8, 4, [(1, _big_rows)], T=0.75, top_k=50, top_p=0.85, seed=11,
               state0=[srow([5]), srow([6])], expect=("topk_and_topp", "temperature_not_1")),
    SampleCase("temperature_philox", 2, 3, 4090, 4, 3, 4, [(2, _flat_rows(9))], T=2.0, seed=(1 << 40) + 99,
               state0=[srow([5, 6])] * 6, expect=("temperature_not_1", "rows_per_sample_3", "noise_decides")),
    SampleCase("rows_per_sample_1", 3, 1, 4090, 4, 3, 4, [(1, _flat_rows(10))], T=0.5, seed=-5,
               state0=[srow([5])] * 3, expect=("temperature_not_1", "noise_decides")),
    SampleCase("bans_fewer_than_topk", 1, 3, 3, 1, 1, 5,
               [(3, fixed({r: np.float32([3, 1.5, 1, 2, 2.5]) for r in range(3)}))], top_k=3, rules=(1, 0),
               state0=[srow([0, 3, 4])] * 3, expect=("bans_leave_fewer_than_topk",)),
    SampleCase("ban_on_max", 1, 3, 4090, 4, 3, 4, [(1, _ban_max_rows)], top_p=0.5, rules=(1, 0), seed=21,
               state0=[srow([500]), srow([4096]), srow([4091])], expect=("ban_on_max_topp",)),
    SampleCase("rules_16385", 2, 1, 16371, 8, 6, 4, [(1, _peaked_rows(4))], top_k=5, rules=(1, 3), seed=2,
               state0=[srow([16384]), srow([7])], expect=("first_of_ng16", "minlen_bans_end")),
    SampleCase("end_and_finished", 4, 1, 3, 1, 1, 4,
               [(1, fixed({0: np.float32([0, 4, 2, 3, 1]), 2: np.float32([4, 1, 2, 3, 0]), 3: np.float32([0, 1, 2, 3, 4])}))],
               top_k=1, state0=[srow([3]), srow([1], fin=True), srow([0]), srow([4])], expect=("end_drawn", "finished_row")),
    SampleCase("all_done", 1, 3, 3, 1, 1, 4, [(2, fixed({}))], state0=[srow([1], fin=True)] * 3, expect=("n_done_is_R",)),
    SampleCase("script_sample", 2, 3, 4090, 4, 3, 4, [(p, _peaked_rows(108, npeaks=4)) for p in range(4)], T=0.875, top_k=6, top_p=0.8,
               seed=77, rules=(2, 2), expect=("scripted", "end_drawn", "finished_row", "topk_and_topp")),
]
SAMPLE_BY_NAME = {c.name: c for c in SAMPLE}


def _kept(tr):
    return [(t, r, k) for t in tr for r, k in t["info"]["kept"].items()]


def _run_at_topp(tr, kept_all):
    """A run of two or more equal scores just past the last strictly-greater kept level: all kept or all dropped."""
    for t, r, k in _kept(tr):
        s = t["rows"][r]
        lv = np.unique(s)[::-1]
        for hi, lo in zip(lv, lv[1:]):
            run = s == lo
            if run.sum() >= 2 and k[s == hi].all() and (k[run].all() if kept_all else not k[run].any()):
                below = s < lo
                if kept_all and not k[below].any():
                    return True
                if not kept_all:
                    return True
    return False


SAMPLE_TAGS = {
    "topk_1": lambda c, tr: c.top_k == 1 and all(k.sum() == 1 for _, _, k in _kept(tr)),
    "topk_vx_minus_1": lambda c, tr: c.top_k == c.Vx - 1 and all(k.sum() == c.Vx - 1 for _, _, k in _kept(tr)),
    "topk_off": lambda c, tr: c.top_k >= c.Vx and all(k.all() for _, _, k in _kept(tr)),
    "topk_run_all_kept_pm_zero": lambda c, tr: any(
        k.sum() > c.top_k and (k & (t["rows"][r] == 0) & np.signbit(t["rows"][r])).any() and
        (k & (t["rows"][r] == 0) & ~np.signbit(t["rows"][r])).any() for t, r, k in _kept(tr)),
    "topp_run_all_kept": lambda c, tr: c.top_p < 1 and _run_at_topp(tr, True),
    "topp_run_all_dropped": lambda c, tr: c.top_p < 1 and _run_at_topp(tr, False),
    "topp_one_kept": lambda c, tr: c.top_p < 1 and all(k.sum() == 1 for _, _, k in _kept(tr)),
    "topk_and_topp": lambda c, tr: 0 < c.top_k < c.Vx and c.top_p < 1,
    "temperature_not_1": lambda c, tr: c.T != 1,
    "rows_per_sample_3": lambda c, tr: c.rps == 3 and c.B > 1,
    "noise_decides": lambda c, tr: any(t["info"]["tok"][r] != t["info"]["smax"][r] for t in tr for r in t["info"]["tok"]),
    "bans_leave_fewer_than_topk": lambda c, tr: any(
        c.Vx - len(t["info"]["banned"][r]) < c.top_k and k.sum() == c.Vx - len(t["info"]["banned"][r]) for t, r, k in _kept(tr)),
    "ban_on_max_topp": lambda c, tr: c.top_p < 1 and all(
        t["info"]["smax"][r] in t["info"]["banned"][r] and k.sum() > 2 and
        t["info"]["tok"][r] != int(np.argmax(np.where(k, t["rows"][r], -np.inf))) for t, r, k in _kept(tr)),
    "minlen_bans_end": lambda c, tr: any(c.end in t["info"]["banned"][r] for t, r, _ in _kept(tr)),
    "end_drawn": lambda c, tr: any(tok == c.end for t in tr for tok in t["info"]["tok"].values()),
    "finished_row": lambda c, tr: any(t["st"]["finished"].any() and t["st"]["n_done"] < c.R for t in tr),
    "n_done_is_R": lambda c, tr: tr[0]["st"]["n_done"] == c.R and not tr[0]["info"]["written"],
    "pointer_entity": lambda c, tr: any(1 in t["info"]["next_mask"] for t in tr),
    "pointer_fact": lambda c, tr: any(2 in t["info"]["next_mask"] for t in tr),
    "seam_inside_quad": lambda c, tr: c.V % 4 != 0,
    "vx_not_multiple_of_4": lambda c, tr: c.Vx % 4 != 0,
    "last_of_ng4": lambda c, tr: c.Vx == 16384 and any(k[16383] for _, _, k in _kept(tr)),
    "first_of_ng16": lambda c, tr: c.Vx == 16385,
    "scripted": lambda c, tr: 3 <= len(tr) <= 5 and tr[-1]["pos"] == c.max_len - 1 and tr[0]["pos"] == 0,
}
SAMPLE_TAGS_REQUIRED = set(SAMPLE_TAGS)
SAMPLE_KERNELS = {("dec_sample_kernel", ng, r) for ng in (4, 16) for r in (False, True)}
