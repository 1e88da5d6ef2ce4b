"""Case table of the context, embedding and pointer kernels' envelope: the entity / fact encoders, the caption embedder,
the context indicators with the predicate gate (csrc/prefill.hip), their backward kernels (csrc/backward.hip from
caption_embed_bwd_kernel down to context_gate_bwd_kernel), the index rules all of them decode through
(csrc/context_index.h) and pointer_scores_kernel (csrc/score_head.hip).
tests/test_context_envelope_gpu.py runs every case against tests/context_ref.py; tests/test_context_ref_cpu.py checks
that the table reaches every hand-placed index it promises.

Shapes are the smallest that still reach an edge: four rows per workgroup (B L, B K, B F in {1, 3, 4, 5, 35}), the
64-lane fact count (F > 64), the 256-entry indicator tables (K, F > 256), the column blocks of 64 / 256 (d = 7, 64,
257, 300, 1100), the three pointer instantiations (d <= 320, <= 512, <= 1024), the pointer batches of 16 context rows
and the eight-row unroll of its backward (Kc = 1, 7, 8, 9, 16, 17, 71).  The tables are small (V = 23 words, 5 entity
types, 7 predicates unless stated) so that many sources meet in one destination row.

Indices are placed by hand on top of synth.make_batch (`gather_inputs`, `gate_inputs`); every one of them is inside the
documented clamping contract, so every address the kernels form is in bounds.  Values are finite and of order one.
"""
from dataclasses import dataclass

import torch

import ick_amd.synth as synth

V = 23                      # words; <pad> = 0
NTYPES = {"geo": 5, "knowledge": 5, "news": 4}
BIG = 2 ** 32


@dataclass(frozen=True)
class GatherCase:           # entity_encode / fact_encode / caption_embed and their backward kernels
    name: str
    variant: str
    B: int
    L: int
    K: int
    F: int                  # 0 for geo
    d: int
    num_pred: int = 7
    pos0: int = 0
    why: str = ""


GATHER = [
    GatherCase("geo_r1_d7", "geo", 1, 1, 1, 0, 7, why="one row everywhere, narrowest d of the entity encoder"),
    GatherCase("know_r3_r3_r1_d64", "knowledge", 1, 3, 3, 1, 64, why="B L = B K = 3, one fact"),
    GatherCase("news_r4_d64", "news", 2, 2, 2, 2, 64, pos0=3, why="exactly one workgroup of rows"),
    GatherCase("know_r5_d300", "knowledge", 1, 5, 5, 5, 300, why="one row past a workgroup"),
    GatherCase("news_r35_r5_r3_d300", "news", 1, 35, 5, 3, 300, why="B L = 35, B F = 3"),
    GatherCase("know_b7_r35_d7", "knowledge", 7, 5, 5, 5, 7, why="B = 7: 35 rows of every kind, d < 64"),
    GatherCase("geo_hand_d300", "geo", 3, 20, 20, 0, 300, pos0=2, why="hand-placed tokens, mask 2 without facts"),
    GatherCase("know_hand_d300", "knowledge", 3, 20, 20, 51, 300, why="every hand-placed index"),
    GatherCase("news_hand_d300", "news", 3, 20, 20, 51, 300, why="every hand-placed index, name words"),
    GatherCase("know_f65_d64", "knowledge", 1, 7, 5, 65, 64, why="fact count: one fact past the 64 lanes"),
    GatherCase("news_f130_d7", "news", 1, 4, 5, 130, 7, why="fact count: third trip of the lane loop"),
    GatherCase("news_k257_f257_d7", "news", 1, 4, 257, 257, 7, num_pred=300, why="K, F > 256"),
    GatherCase("know_k257_f3_d257", "knowledge", 1, 3, 257, 3, 257, why="second column block of the deterministic twins"),
]

# the one case with a fact subject of 2^32 + 1 and a predicate of 2^32 + 2: the encoders clamp them in int64 (to K - 1
# and num_pred - 1) and the fact count matches them to no entity; narrowing to int first would read rows 1 and 2
BIG_INDEX = GatherCase("know_big_index_d64", "knowledge", 2, 5, 5, 9, 64)


@dataclass(frozen=True)
class GateCase:             # context_indicators (+ dense predicate indicator) and context_gate_bwd
    name: str
    B: int
    L: int
    K: int
    F: int
    d: int
    num_pred: int = 7
    mode: int = 0
    bwd: bool = True
    why: str = ""


GATE = [
    GateCase("g_l1_k1_f1_d7", 1, 1, 1, 1, 7, why="first mention at the last position: act == T"),
    GateCase("g_l2_k5_f3_d64", 2, 2, 5, 3, 64),
    GateCase("g_hand_l20_d300", 3, 20, 20, 51, 300, why="every hand-placed subject / predicate, second column block"),
    GateCase("g_hand_mode1_d300", 3, 20, 20, 51, 300, mode=1, why="mode 1: T = 1, every mention counts"),
    GateCase("g_l63_k20_f65_d257", 1, 63, 20, 65, 257, why="largest T of the gate backward with K + 3 F <= 256"),
    GateCase("g_k257_f257_d64", 2, 20, 257, 257, 64, num_pred=300, why="K, F > 256: second trip of the table loops"),
    GateCase("g_f130_d1100", 1, 20, 5, 130, 1100, bwd=False, why="gate forward: 4 column blocks and a second trip"),
    GateCase("g_mode1_l2_f3_d257", 2, 2, 5, 3, 257, mode=1),
]
# (B, L, K, F, d): the gate backward's LDS holds T * 256 floats + K + 3 F ints; T = 64 is one row too many
GATE_BWD_REJECTED = (1, 64, 20, 65, 64)
# (B, L, K, F): the indicators' LDS holds K + 5 F + 1 ints
INDICATORS_REJECTED = (1, 1, 1, 3277)


@dataclass(frozen=True)
class PointerCase:          # pointer_scores (plain / out_gmap / packed) and pointer_scores_bwd (plain / packed)
    name: str
    B: int
    T: int
    Kc: int
    d: int
    lengths: tuple          # caption lengths of the packed form (length - 1 valid rows); 2 = one valid row
    why: str = ""


POINTER = [
    PointerCase("p_t1_k1_d64", 1, 1, 1, 64, (1,), why="smallest; packed: no valid row at T = 1"),
    PointerCase("p_t2_k7_d300", 2, 2, 7, 300, (2, 2), why="Kc < 8: the unroll's tail only"),
    PointerCase("p_t5_k8_d320", 3, 5, 8, 320, (5, 2, 3), why="last d of the 5-per-lane instantiation, one full unroll"),
    PointerCase("p_t3_k9_d321", 2, 3, 9, 321, (2, 3), why="first d of the 8-per-lane instantiation"),
    PointerCase("p_t20_k16_d512", 1, 20, 16, 512, (7,), why="last d of the 8-per-lane instantiation, one full batch"),
    PointerCase("p_t2_k17_d513", 2, 2, 17, 513, (2, 2), why="first d of the 16-per-lane instantiation, batch + 1"),
    PointerCase("p_t2_k71_d1024", 1, 2, 71, 1024, (2,), why="widest d"),
    PointerCase("p_t20_k71_d257", 2, 20, 71, 257, (2, 20), why="d not a multiple of 64, five 64-column blocks"),
    PointerCase("p_t7_k17_d7", 3, 7, 17, 7, (4, 2, 7), why="d < 64"),
    PointerCase("p_t4_k16_d64", 1, 4, 16, 64, (3,)),
]
POINTER_D_REJECTED = 1025                       # pointer forward: d > 64 * 16
POINTER_BWD_REJECTED = (1, 64, 252, 64)         # (B, T, Kc, d): T Kc + 260 floats just over the 64 KiB of LDS

# every hand-placed index the table promises; gather_inputs / gate_inputs return the labels they placed
CAPTION_LABELS = {"word", "ent_first", "ent_last", "fact_first", "fact_last", "beyond_all", "negative", "mask1_on_word",
                  "mask2_geo", "mask2_bad_fact", "mask3", "one_entity_everywhere", "pad_tail_zero_dx"}
ENTITY_LABELS = {"type_negative", "type_ntypes", "type_fraction", "name_negative", "name_vocab", "name_all_equal"}
FACT_LABELS = {"subj_negative", "subj_K", "subj_last", "subj_2^32+1", "subj_all_one", "pred_negative", "pred_num_pred",
               "pred_2^32+2", "pred_all_one_equal_act", "pred_two_subjects", "subj_first_at_0", "subj_first_at_last",
               "subj_never"}


def _fold(batch, c_variant, ntypes, num_pred):
    """synth draws types in [0, 500] and predicates in [0, 3000): fold them into this table's small tables."""
    batch["entities"][:, :, 4] = batch["entities"][:, :, 4] % ntypes
    if "facts" in batch:
        batch["facts"][:, :, 2] = batch["facts"][:, :, 2] % num_pred


def gather_inputs(c: GatherCase, big=False):
    """-> (batch dict of CPU tensors, set of labels placed).  Each index is placed where the shape has room for it.
    big: with the subject 2^32 + 1 and the predicate 2^32 + 2 (BIG_INDEX only, so that one test answers for them)."""
    seed = sum(map(ord, c.name))
    batch = synth.make_batch(c.variant, c.B, c.L, c.K, V, c.F, seed)
    nt = NTYPES[c.variant]
    _fold(batch, c.variant, nt, c.num_pred)
    caps, masks, ent = batch["captions"], batch["caption_masks"], batch["entities"]
    B, L, K, F = c.B, c.L, c.K, c.F
    done = set()
    facts_on = c.variant != "geo"
    # ---- caption tokens: sample 0, positions 1 .. (position 0 stays <start>)
    toks = [("word", 3, 0), ("ent_first", V, 1), ("ent_last", V + K - 1, 1), ("beyond_all", V + K + F + 5, 1),
            ("negative", -1, 0), ("mask1_on_word", 4, 1), ("mask3", 5, 3)]
    if facts_on:
        toks += [("fact_first", V + K, 2), ("fact_last", V + K + F - 1, 2), ("mask2_bad_fact", V + K + F + 5, 2),
                 ("negative_ent", -1, 1), ("word_mask2", 6, 2)]
    else:
        toks += [("mask2_geo", V + 1, 2)]
    for i, (label, tok, m) in enumerate(toks):
        b, l = divmod(i + 1, L)
        if b < B:
            caps[b, l], masks[b, l] = tok, m
            done.add(label)
    if B >= 2 and len(toks) + 1 <= L * (B - 1):
        caps[B - 1, :], masks[B - 1, :] = V + min(2, K - 1), 1      # every position of the last sample names one entity
        done.add("one_entity_everywhere")
    if B >= 3 and len(toks) + 1 <= L:
        caps[1, L // 2:], masks[1, L // 2:] = 0, 0                  # a <pad> tail; the test zeroes its dx rows
        batch["zero_dx"] = (1, L // 2)
        done.add("pad_tail_zero_dx")
    # ---- entity type / name words
    places = [("type_negative", -3.0), ("type_ntypes", float(nt)), ("type_fraction", 2.7)]
    for i, (label, v) in enumerate(places):
        b, k = divmod(i, K)
        if b < B:
            ent[b, k, 4] = v
            done.add(label)
    if c.variant == "news":
        for i, (label, v) in enumerate([("name_negative", -1.0), ("name_vocab", float(V)), ("name_all_equal", None)]):
            b, k = divmod(i + 1, K)
            if b < B:
                if v is None:
                    ent[b, k, 5:10] = 7.0
                else:
                    ent[b, k, 5 + i] = v
                done.add(label)
    # ---- fact subject / predicate
    if facts_on:
        done |= _place_facts(batch["facts"], B, K, F, c.num_pred, big)
    return batch, done


def _place_facts(facts, B, K, F, num_pred, big):
    done = set()
    places = [("subj_negative", 1, -1), ("subj_K", 1, K), ("subj_last", 1, K - 1),
              ("pred_negative", 2, -1), ("pred_num_pred", 2, num_pred)]
    if big:
        places += [("subj_2^32+1", 1, BIG + 1), ("pred_2^32+2", 2, BIG + 2)]
    for i, (label, col, v) in enumerate(places):
        b, j = divmod(i, F)
        if b < B:
            facts[b, j, col] = v
            done.add(label)
    if B >= 2 and len(places) <= F:
        facts[1, :, 1] = min(1, K - 1)          # every fact of sample 1 on one subject ...
        done.add("subj_all_one")
    if B >= 3:
        facts[2, :, 2] = 3 % num_pred           # ... and every fact of sample 2 on one predicate
    return done


def gate_inputs(c: GateCase):
    """-> (captions, facts, labels).  Samples: 0 carries the out-of-range subjects / predicates; 1 has every fact on one
    subject and one predicate (equal activation: the lowest index represents it); 2 has one predicate on two subjects
    first mentioned at different positions, and subjects first mentioned at position 0, at L - 1 and never."""
    seed = sum(map(ord, c.name))
    batch = synth.make_batch("knowledge", c.B, c.L, c.K, V, c.F, seed)
    _fold(batch, "knowledge", 5, c.num_pred)
    caps, facts = batch["captions"], batch["facts"]
    B, L, K, F = c.B, c.L, c.K, c.F
    done = set()
    caps[0, L // 2] = V + min(1, K - 1)                 # sample 0 mentions an entity
    facts[0, :, 1] = torch.where(torch.arange(F) % 2 == 0, torch.full((F,), min(1, K - 1)), facts[0, :, 1])
    done |= _place_facts(facts, 1, K, F, c.num_pred, True)
    if L == 1:
        caps[0, 0] = V                                  # the only position: act == 1 == T, nothing is active
        facts[0, 0, 1], facts[0, 0, 2] = 0, 0
        done.add("subj_first_at_last")
    if B >= 2 and K >= 2 and F >= 3:
        caps[1, :] = 1
        caps[1, 0] = V + 1
        facts[1, :, 1], facts[1, :, 2] = 1, 2 % c.num_pred
        done |= {"subj_all_one", "pred_all_one_equal_act", "subj_first_at_0"}
    if B >= 3 and K >= 5 and F >= 6 and L >= 4:
        caps[2, :] = 1
        caps[2, 0], caps[2, 2], caps[2, L - 1] = V + 0, V + 1, V + 2    # entity 3 is never mentioned
        caps[2, 3] = V + 0                                              # a second mention does not move the first
        facts[2, :, 1], facts[2, :, 2] = 3, torch.arange(F) % c.num_pred
        facts[2, 0, 1], facts[2, 0, 2] = 1, 4 % c.num_pred              # predicate 4: subject 1 (from position 3) ...
        facts[2, 1, 1], facts[2, 1, 2] = 0, 4 % c.num_pred              # ... and subject 0 (from position 1)
        facts[2, 2, 1], facts[2, 2, 2] = 2, 5 % c.num_pred              # first mentioned at L - 1: act == T
        facts[2, 3, 1], facts[2, 3, 2] = 0, 6 % c.num_pred
        facts[2, 4, 1], facts[2, 4, 2] = 1, 6 % c.num_pred              # predicate 6: the earlier index wins on act too
        done |= {"pred_two_subjects", "subj_first_at_0", "subj_first_at_last", "subj_never"}
    return caps, facts, done
