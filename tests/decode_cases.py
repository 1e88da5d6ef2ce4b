"""Case table of the fused decode envelope (csrc/decode.hip): every case names its sizes and the launch plan
(ick_decode_plan) it is meant to exercise.  tests/test_decode_plan_cpu.py checks that the table's plans together reach
every kernel instantiation, both score-head paths, the LN-on-load loop and a ragged last row group of every G > 1;
tests/test_decode_envelope_gpu.py runs each case against the float64 oracle (tests/decode_ref.py).

Baseline: geo, d = 300, H = 10, FF = 512, 3 layers, K = 20 entities, V = 1000, max_len = 16.  A case lists only what
differs.  S = 196 image rows + K (+ F) memory rows.
"""
from dataclasses import dataclass, field


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                  # "greedy" | "beam" | "sample"
    B: int
    rps: int = 1               # rows per sample: beam size or samples per caption
    variant: str = "geo"
    d: int = 300
    H: int = 10
    FF: int = 512
    layers: int = 3
    K: int = 20
    F: int = 0
    V: int = 1000
    max_len: int = 16
    seed: int = 1
    end_bias: float = 0.0      # added to the <end> (= last word) bias; negative: every row runs all steps, positive:
                               # <end> is chosen at some step (asserted)
    q_scale: float = 1.0       # cross-attention query rows of every decoder layer scaled: sharper attention
    plan: dict = field(default=None, compare=False, hash=False)
    why: str = ""

    @property
    def R(self):
        return self.B * self.rps

    @property
    def S(self):
        return 196 + self.K + self.F

    @property
    def Vx(self):
        return self.V + self.K + self.F


def P(g_self, g_cross, g_ffn, shared=0, merged=0, loop=0):
    return dict(g_self=g_self, g_cross=g_cross, g_ffn=g_ffn, cross_shared=shared, head_merged=merged, gather_loop=loop)


CASES = [
    # ---------------------------------------------------------------- greedy (fused selection, production sequence)
    Case("greedy_b3", "greedy", 3, plan=P(1, 1, 1, merged=1), why="G 1, merged head"),
    Case("greedy_b32", "greedy", 32, plan=P(2, 2, 1, merged=1), why="G 2 with the merged head"),
    Case("greedy_b33", "greedy", 33, plan=P(2, 2, 2), why="G 2, split head, ragged"),
    Case("greedy_b67", "greedy", 67, plan=P(4, 4, 4), why="G 4, ragged"),
    Case("greedy_b131", "greedy", 131, max_len=12, plan=P(8, 8, 8, loop=1), why="G 8, ragged, 5 vocab row blocks"),
    Case("greedy_wide_b3", "greedy", 3, d=320, H=16, FF=1024, V=2000, plan=P(1, 1, 1, loop=1),
         why="18 LN sources, split head at R <= 32, head width 20"),
    Case("greedy_wide_b40", "greedy", 40, d=320, H=16, FF=1024, max_len=12, plan=P(4, 4, 4, loop=1),
         why="d = 320 at G 4, ragged"),
    Case("greedy_small", "greedy", 3, d=64, H=2, FF=64, V=300, plan=P(1, 1, 1, merged=1), why="narrowest model"),
    Case("greedy_d260", "greedy", 33, d=260, H=13, FF=100, max_len=12, plan=P(2, 2, 1, loop=1),
         why="d4 = 65 (wide columns), 15 LN sources at G 2, a 36-unit last FFN chunk"),
    Case("greedy_h12", "greedy", 3, d=300, H=12, FF=644, plan=P(1, 1, 1, loop=1),
         why="head width 25, 11 FFN chunks: 13 sources, split head at R <= 32"),
    Case("greedy_s1024_geo", "greedy", 3, K=828, max_len=10, q_scale=8.0, plan=P(1, 1, 1, merged=1),
         why="S = 1024 memory rows; sharpened so that the last row alone moves the scores (test_decode_plan_cpu)"),
    Case("greedy_s1024_knowledge", "greedy", 3, variant="knowledge", K=400, F=428, max_len=10,
         plan=P(1, 1, 1, merged=1), why="S = 1024 with facts"),
    Case("greedy_ml128", "greedy", 3, max_len=128, V=300, end_bias=-30.0, plan=P(1, 1, 1, merged=1),
         why="every row runs all 128 cached positions"),
    Case("greedy_v47", "greedy", 5, V=47, K=6, plan=P(1, 1, 1, merged=1), why="vocabulary inside one 48-word tile"),
    Case("greedy_v16385", "greedy", 3, V=16385, end_bias=2.5, plan=P(1, 1, 1, merged=1),
         why="a partial last 48-word tile (16385 = 341 x 48 + 17); the last word (<end>) wins in every row"),
    Case("greedy_v49200", "greedy", 3, V=49200, end_bias=3.0, plan=P(1, 1, 1, merged=1),
         why="1025 vocabulary tiles: the selection's second 1024-tile sweep holds the last word (<end>), which wins"),
    Case("greedy_knowledge_b67", "greedy", 67, variant="knowledge", K=10, F=12, V=500, max_len=12,
         plan=P(4, 4, 4), why="facts at G 4"),
    Case("greedy_news_b67", "greedy", 67, variant="news", K=10, F=12, V=500, max_len=12, plan=P(4, 4, 4),
         why="news at G 4"),
    # ---------------------------------------------------------------- beam search
    Case("beam2_b20", "beam", 20, rps=2, max_len=10, plan=P(2, 2, 2, shared=1), why="shared cross G 2"),
    Case("beam4_b10", "beam", 10, rps=4, max_len=10, plan=P(2, 4, 2, shared=1), why="shared cross G 4"),
    Case("beam5_b12", "beam", 12, rps=5, max_len=10, plan=P(4, 5, 2, shared=1, loop=1), why="shared cross G 5"),
    Case("beam6_b6", "beam", 6, rps=6, max_len=10, plan=P(2, 3, 2, shared=1), why="shared cross G 3"),
    Case("beam7_b5", "beam", 5, rps=7, max_len=10, plan=P(2, 1, 2), why="unshared cross for a beam of 7"),
    Case("beam8_b20", "beam", 20, rps=8, max_len=8, plan=P(8, 8, 8, shared=1, loop=1), why="R = 160, shared G 8"),
    Case("beam8_vx65536", "beam", 1, rps=8, V=65516, K=20, max_len=6, plan=P(1, 8, 1, shared=1, merged=1, loop=1),
         why="largest vocabulary beam search takes"),
    # ---------------------------------------------------------------- sampling
    Case("sample4_b10", "sample", 10, rps=4, max_len=10, plan=P(2, 4, 2, shared=1)),
    Case("sample7_b5", "sample", 5, rps=7, max_len=10, plan=P(2, 1, 2)),
    Case("sample8_b4", "sample", 4, rps=8, max_len=10, plan=P(2, 8, 1, shared=1, merged=1, loop=1)),
    Case("sample16_b9", "sample", 9, rps=16, max_len=8, plan=P(8, 8, 8, shared=1, loop=1), why="R = 144"),
    Case("sample1_vx65536", "sample", 2, rps=1, V=65516, K=20, max_len=6, plan=P(1, 1, 1, merged=1),
         why="largest vocabulary sampling takes"),
]

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def shape_params(case, P):
    """The case's shaping of the synthetic parameters (in place on copies of the touched tensors)."""
    if case.end_bias:
        P["fc_vocab.bias"] = P["fc_vocab.bias"].clone()
        P["fc_vocab.bias"][case.V - 1] += case.end_bias
    if case.q_scale != 1.0:
        for li in range(case.layers):
            for k in ("weight", "bias"):
                name = "transformer_decoder.layers.%d.multihead_attn.in_proj_%s" % (li, k)
                P[name] = P[name].clone()
                P[name][:case.d] *= case.q_scale
    return P


# csrc/decode_select.h: kVocabTile; csrc/decode_select.hip: tiles per sweep of dec_select_kernel
VOCAB_TILE, SELECT_SWEEP_TILES = 48, 1024


def kernels_of(case, plan):
    """The instantiations and paths a run of `case` with launch plan `plan` reaches (strings)."""
    out = set()
    g = plan["g_self"]
    out.add("self<%d,false>" % g)                  # step 0 and every layer after the first
    if case.kind == "greedy" and plan["fsel"]:
        out.add("self<%d,true>" % g)               # the production greedy sequence fuses the selection at step >= 1
    out.add("cross<%d,%s>" % (plan["g_cross"], "shared" if plan["cross_shared"] else "unshared"))
    out.add("ffn<%d>" % plan["g_ffn"])
    out.add("head:merged" if plan["head_merged"] else "head:split")
    if plan["gather_loop"]:
        out.add("gather_loop")
    if case.kind == "greedy" and -(-case.V // VOCAB_TILE) > SELECT_SWEEP_TILES:
        out.add("select:second_sweep")             # dec_select_kernel reads the candidate tiles 1024 at a time
    for what in ("self", "ffn") + (() if plan["cross_shared"] else ("cross",)):
        gg = plan["g_" + what]
        if gg > 1 and case.R % gg:
            out.add("ragged:%s<%d>" % (what, gg))
    return out


REQUIRED = ({"self<%d,%s>" % (g, f) for g in (1, 2, 4, 8) for f in ("false", "true")}
            | {"cross<%d,unshared>" % g for g in (1, 2, 4, 8)}
            | {"cross<%d,shared>" % g for g in (2, 3, 4, 5, 8)}
            | {"ffn<%d>" % g for g in (1, 2, 4, 8)}
            | {"head:merged", "head:split", "gather_loop", "select:second_sweep"}
            | {"ragged:%s<%d>" % (k, g) for k in ("self", "cross", "ffn") for g in (2, 4, 8)})
