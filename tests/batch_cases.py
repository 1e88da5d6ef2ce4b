"""Case table of the BATCH shapes the suite runs the whole training step at (tests/test_batch_geometry_cpu.py,
tests/test_batch_geometry_gpu.py), the oracle steps both files compare with, and the batch sequences that change the shape
inside one TrainStep.

tests/model_cases.py varies the MODEL under one batch (B = 5, L = 9, K = 6, lengths 5..9).  Here the model is fixed at the
base geometry (d 300, H 10, FF 512 / 512, 3 layers, P = 196 image rows: the full tier, the path the bench replays) and the
batch varies: B = 1, a single valid row, ties in the length sort, valid rows that are no prefix of the batch, L = 2 and
L = 52, K = 1 and K = 200, a packed-row count on a tile edge, a memory longer than the matrix-core attention takes.  V = 152
(152 % 8 == 0: the Adam pass writes the re-laid-out weight images, DerivedWeights) unless a case says V = 150 (per-step
packing).

Per case the attention launch plans it is meant to reach are written out by hand in the notation of tests/train_cases.py
-- ("mfma", NQT, MAXT) for the matrix-core kernels, NQT = ceil(T / 16), MAXT = 1 (S <= 64), 4 (<= 256), 5 (<= 320),
8 (<= 512); ("general", DHP, chunks) for the general ones -- as (forward, backward) pairs of
  self   decoder self-attention, T = S = L, causal
  cross  cross-attention, T = L over S = 196 + K + Fn memory rows
  ent    the entity stack, T = S = K
  fact   the fact stack, T = S = Fn (None without facts)
all at head width 30 (d / H).  The CPU test holds them to ops.attention_plan.

No case is refused by the library (REFUSED is empty): every shape below runs through TrainStep at the base geometry.
"""
import math
from dataclasses import dataclass, replace

import ick_amd.synth as synth
import model_cases as MC
from dropout_ref import with_lengths

P_IMG, D, H, DH = 196, 300, 10, 30
SEED = 21
V_DERIVED, V_PLAIN = 152, 150
BASE = MC.BY_NAME["base"]


def _m(nqt, maxt):
    return ("mfma", nqt, maxt)


def _g(dhp, chunks=1):
    return ("general", dhp, chunks)


@dataclass(frozen=True)
class BatchCase:
    name: str
    variant: str
    B: int
    L: int
    K: int
    Fn: int
    lengths: tuple          # None: synth.make_captions' own (all equal to L where L <= 5)
    self_attn: tuple        # (forward plan, backward plan)
    cross: tuple
    ent: tuple
    fact: tuple = None
    V: int = V_DERIVED
    why: str = ""
    seed: int = SEED

    @property
    def Mp(self):
        """The packed row count: the valid caption rows of the batch, sum of max(0, length - 1)."""
        return sum(max(0, n - 1) for n in case_lengths(self))

    @property
    def S(self):
        return P_IMG + self.K + self.Fn

    @property
    def model(self):
        """The model_cases.Case (base geometry) of this case's variant and vocabulary: what MC.make_params,
        MC.oracle_config and MC.build_decoder take."""
        return replace(BASE, name="base_%s_v%d" % (self.variant, self.V), variant=self.variant, Fn=self.Fn, V=self.V,
                       derived=self.V % 8 == 0)

    @property
    def shapes(self):
        """name -> (T, S, causal) of the four attention problems of a step."""
        out = dict(self_attn=(self.L, self.L, True), cross=(self.L, self.S, False), ent=(self.K, self.K, False))
        if self.Fn:
            out["fact"] = (self.Fn, self.Fn, False)
        return out

    @property
    def plans(self):
        """name -> (forward plan, backward plan) as the table states them."""
        out = dict(self_attn=self.self_attn, cross=self.cross, ent=self.ent)
        if self.Fn:
            out["fact"] = self.fact
        return out


def _c(name, variant, B, L, K, Fn, lengths, self_attn, cross, ent, fact=None, V=V_DERIVED, why=""):
    pair = lambda p: None if p is None else (p if isinstance(p[0], tuple) else (p, p))      # noqa: E731
    return BatchCase(name, variant, B, L, K, Fn, None if lengths is None else tuple(lengths), pair(self_attn), pair(cross),
                     pair(ent), pair(fact), V, why)


INTERLEAVED = [9, 1, 9, 1, 2]
CASES = [
    _c("one_row", "geo", 1, 2, 1, 0, [2], _m(1, 1), _m(1, 4), _g(32),
       why="smallest batch the step accepts: Mp = 1, one entity (T = 1: the general kernels), cross-attention of 2 queries"),
    _c("one_caption", "geo", 1, 9, 6, 0, [9], _m(1, 1), _m(1, 4), _m(1, 1), why="B = 1 with a full caption"),
    _c("one_fact", "knowledge", 1, 2, 1, 1, [2], _m(1, 1), _m(1, 4), _g(32), _g(32),
       why="one entity, one fact: predicate gate and fact stack at T = 1"),
    _c("nearly_empty", "geo", 4, 6, 6, 0, [1, 1, 1, 2], _m(1, 1), _m(1, 4), _m(1, 1),
       why="Mp = 1 of 24 rows; three captions without a row"),
    _c("equal_lengths", "geo", 6, 9, 6, 0, [5] * 6, _m(1, 1), _m(1, 4), _m(1, 1),
       why="ties: the oracle's sort permutation against the step's unsorted batch"),
    _c("interleaved", "geo", 5, 9, 6, 0, INTERLEAVED, _m(1, 1), _m(1, 4), _m(1, 1),
       why="valid rows are not a prefix of the batch in either order"),
    _c("rows_64", "geo", 13, 6, 6, 0, [6] * 12 + [5], _m(1, 1), _m(1, 4), _m(1, 1),
       why="Mp = 64: exactly one 64-row tile of the packed head and the valid-row weight gradients"),
    _c("rows_65", "geo", 13, 6, 6, 0, [6] * 13, _m(1, 1), _m(1, 4), _m(1, 1), why="Mp = 65: one row past the tile"),
    _c("many_short", "geo", 64, 3, 2, 0, None, _m(1, 1), _m(1, 4), _m(1, 1),
       why="the bench's B with B L = 192 rows over 64 / 128-row tiles, Mp = 128"),
    _c("long_captions", "news", 3, 52, 20, 7, [52, 30, 2], _m(4, 1), _m(4, 4), _m(2, 1), _m(1, 1),
       why="T = 52: attention at NQT 4; position codes past 20; a 2-token caption next to a 52-token one"),
    _c("wide_context", "knowledge", 13, 5, 60, 40, None, _m(1, 1), _m(1, 5), _m(4, 1), _m(3, 1),
       why="context stacks at T = 60 / 40, S = 296 (MAXT 5), 100 pointer columns"),
    _c("past_matrix_core", "knowledge", 2, 4, 200, 120, [4, 2], _m(1, 1), _g(32), (_g(32, 2), _g(32, 4)), _g(32),
       why="S = 516 > 512: the general attention kernels inside the real model, entity stack at T = 200"),
    _c("base_v150", "geo", 5, 9, 6, 0, INTERLEAVED, _m(1, 1), _m(1, 4), _m(1, 1), V=V_PLAIN,
       why="the same interleaving without DerivedWeights (per-step packing)"),
]
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# (BatchCase, text the IckError must contain): shapes the library refuses by name.  None: every case above runs.
REFUSED = []


# ------------------------------------------------------------------------------------------------ inputs
_PARAMS = {}


def make_params(c):
    """One set of parameters per (variant, V), shared by every case and sequence of that model."""
    key = (c.variant, c.V)
    if key not in _PARAMS:
        _PARAMS[key] = MC.make_params(c.model)
    return _PARAMS[key]


def make_batch(variant, B, L, K, Fn, V, seed, lengths=None):
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    return batch if lengths is None else with_lengths(batch, list(lengths), V)


def make_inputs(c, seed=None, lengths="case"):
    """(batch, enc_out) of the case (lengths: another list of the case's B lengths)."""
    seed = c.seed if seed is None else seed
    lengths = c.lengths if lengths == "case" else lengths
    return make_batch(c.variant, c.B, c.L, c.K, c.Fn, c.V, seed, lengths), synth.make_enc_out(c.B, seed)


def case_lengths(c):
    if c.lengths is not None:
        return list(c.lengths)
    return synth.make_captions(c.variant, c.B, c.L, c.K, c.Fn, c.V, c.seed)[2].view(-1).tolist()


def oracle_step(c, f64, inputs=None):
    return MC.oracle_step(c.model, f64, make_params(c), inputs=make_inputs(c) if inputs is None else inputs)


# ------------------------------------------------------------------------------------------------ shape-change sequences
# A step of a sequence: (B, L, K, lengths or None, seed).  All geo, Fn = 0; V is the sequence's.
A_SHAPE, TAIL_SHAPE = (5, 9, 6), (2, 9, 6)


def _steps(shapes, seed0, lengths=None):
    lengths = lengths or {}
    return [(B, L, K, lengths.get(i), seed0 + i) for i, (B, L, K) in enumerate(shapes)]


# (a) an epoch with a ragged tail, twice: fresh seeds per batch
RAGGED = _steps([A_SHAPE, A_SHAPE, TAIL_SHAPE, A_SHAPE, A_SHAPE, TAIL_SHAPE], 100)
# (b) five distinct shapes -- one more than the graph cache holds -- and the first again.  Small shapes, but none with a
# single caption or a single row: with one_row / nearly_empty / one_caption as steps 2, 3 and 5 the float32 oracle's own
# loss strays up to 2.2e-6 (9.3e-6 at another seed) from the float64 one -- a step on one token's gradient is mostly
# Adam's +-lr on rounding noise -- which is more than the tenth of the 2e-5 bar the reference may use up.  With at least
# 12 tokens per batch it stays at 7.6e-7 (tests/test_batch_geometry_cpu.py).
EVICTION = _steps([A_SHAPE, (3, 5, 6), (4, 6, 6), TAIL_SHAPE, (6, 3, 2), A_SHAPE], 200, {2: (6, 1, 3, 2)})
# (c) capture against eager: A, tail, A, A's shape without a single valid row, a third shape, tail, A
BITWISE = _steps([A_SHAPE, TAIL_SHAPE, A_SHAPE, A_SHAPE, (4, 6, 6), TAIL_SHAPE, A_SHAPE], 300,
                 {3: (1,) * 5, 4: (6, 1, 3, 2)})
# ... and five distinct (B, L) for the scheduled-sampling buffers, then the first again
BITWISE_SS = _steps([A_SHAPE, TAIL_SHAPE, (4, 6, 6), (1, 9, 6), (3, 5, 6), A_SHAPE], 400, {2: (6, 1, 3, 2)})
# ... and the feature-map input at B = 3 -> 2 -> 3
BITWISE_CONV1 = _steps([(3, 9, 6), TAIL_SHAPE, (3, 9, 6), TAIL_SHAPE], 500, {1: (9, 1)})
SEQUENCES = dict(ragged=RAGGED, eviction=EVICTION)


CONV1_SEED = 21         # Encoder.conv1's parameters where a sequence feeds the (B, 2048, 14, 14) feature map


def sequence_inputs(steps, V, variant="geo", projected=False):
    """[(batch, enc_out)] of a sequence.  projected: enc_out is the float64 projection (R.feat_proj) of the step's feature
    map synth.make_feats(B, seed) through conv1's parameters of CONV1_SEED -- what the step computes from that map with
    encoder= -- in place of synth.make_enc_out's."""
    out = []
    for B, L, K, lengths, seed in steps:
        if projected:
            import torch
            from oracle import restatement as R
            cw, cb = synth.make_conv1(CONV1_SEED)
            with torch.no_grad():
                enc_out = R.feat_proj(synth.make_feats(B, seed).double(), cw.double(), cb.double())
        else:
            enc_out = synth.make_enc_out(B, seed)
        out.append((make_batch(variant, B, L, K, 0, V, seed, lengths), enc_out))
    return out


def sequence_model(V):
    return replace(BASE, name="base_geo_v%d" % V, V=V, derived=V % 8 == 0)


def sequence_params(V):
    if ("geo", V) not in _PARAMS:
        _PARAMS[("geo", V)] = MC.make_params(sequence_model(V))
    return _PARAMS[("geo", V)]


def distinct_shapes(steps):
    return len({s[:3] for s in steps})


def nqt(T):
    return math.ceil(T / 16)
