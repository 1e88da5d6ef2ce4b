"""Case table of the training-step kernels' envelope: attention forward / backward (csrc/attention.hip,
csrc/attention_mfma.hip), the row chains (csrc/rowchain.hip, csrc/rowchain_bwd.hip) and the LayerNorm backward
(csrc/backward.hip).  Every attention case names the launch plan (ick_attention_plan) it is meant to exercise in each
direction; tests/test_train_plan_cpu.py checks those plans against the library and that the table together reaches
every kernel instantiation, tests/test_train_envelope_gpu.py runs every case against float64 torch autograd.

Attention plans are written ("mfma", NQT, MAXT) for the matrix-core kernels and ("general", DHP, chunks) for the
general ones (chunks > 1: the backward accumulates dK / dV with float atomics).  Operands are head-major padded (row
stride DHP = 32 for dh <= 32, else 64), as the training step keeps them.
"""
from dataclasses import dataclass


@dataclass(frozen=True)
class AttnCase:
    name: str
    T: int
    S: int
    fwd: tuple
    bwd: tuple
    dh: int = 30
    H: int = 2
    B: int = 2
    causal: bool = False
    q_pos0: str = "0"         # "0" or "S-T" (the queries are the last T positions of the S keys)
    drop: float = 0.0         # attention-weight dropout probability
    why: str = ""

    @property
    def pos0(self):
        return 0 if self.q_pos0 == "0" else self.S - self.T

    @property
    def hp(self):             # row stride of the head-major buffers
        return 32 if self.dh <= 32 else 64

    @property
    def st2(self):
        """The matrix-core backward's 8-byte dK / dV stores (launch_bwd in attention_mfma.hip): dK / dV are the two
        column halves of one (B, S, 2 H dh) row-major buffer, so every stride is even and dV starts at an even offset
        exactly when H dh is even."""
        return self.dh % 2 == 0 and (self.H * self.dh) % 2 == 0


def _m(nqt, maxt):
    return ("mfma", nqt, maxt)


def _g(dhp, chunks=1):
    return ("general", dhp, chunks)


ATTN = [
    # matrix-core kernels: every (NQT, MAXT) instantiation.  NQT = ceil(T / 16); MAXT = 1 (S <= 64), 4 (<= 256),
    # 5 (<= 320), 8 (<= 512).  attn_mfma_shape_ok takes S <= 512 for T <= 48 and S <= 416 at T = 64 (the backward's
    # dS tile in LDS); both directions use the same predicate.
    AttnCase("m1x1_t2_s1", 2, 1, _m(1, 1), _m(1, 1), why="smallest shape of the path"),
    AttnCase("m1x1_t16_s64", 16, 64, _m(1, 1), _m(1, 1), causal=True, q_pos0="S-T", why="full tiles, causal offset"),
    AttnCase("m1x4_t16_s65", 16, 65, _m(1, 4), _m(1, 4), why="first S of MAXT 4"),
    AttnCase("m1x5_t2_s257", 2, 257, _m(1, 5), _m(1, 5), drop=0.1, why="first S of MAXT 5, dropout"),
    AttnCase("m1x8_t16_s512", 16, 512, _m(1, 8), _m(1, 8), why="largest S for NQT 1"),
    AttnCase("g_t16_s513", 16, 513, _g(32), _g(32), why="first S the matrix-core path rejects at NQT 1"),
    AttnCase("m2x1_t17_s17", 17, 17, _m(2, 1), _m(2, 1), causal=True, why="one row and one key past a tile"),
    AttnCase("m2x4_t32_s256", 32, 256, _m(2, 4), _m(2, 4), causal=True, q_pos0="S-T", why="last S of MAXT 4"),
    AttnCase("m2x5_t17_s320", 17, 320, _m(2, 5), _m(2, 5), why="last S of MAXT 5"),
    AttnCase("m2x8_t32_s321", 32, 321, _m(2, 8), _m(2, 8), drop=0.1, why="first S of MAXT 8, dropout"),
    AttnCase("m2x8_t32_s512", 32, 512, _m(2, 8), _m(2, 8), why="largest S for NQT 2"),
    AttnCase("g_t32_s513", 32, 513, _g(32), _g(32, 2), causal=True, q_pos0="S-T",
             why="first S the matrix-core path rejects at NQT 2"),
    AttnCase("m3x1_t33_s16", 33, 16, _m(3, 1), _m(3, 1), why="one query past two tiles, one key tile"),
    AttnCase("m3x4_t48_s65", 48, 65, _m(3, 4), _m(3, 4), causal=True, why="causal: keys beyond every query"),
    AttnCase("m3x5_t33_s300", 33, 300, _m(3, 5), _m(3, 5), drop=0.1, why="dropout"),
    AttnCase("m3x8_t48_s512", 48, 512, _m(3, 8), _m(3, 8), why="largest S for NQT 3"),
    AttnCase("g_t48_s513", 48, 513, _g(32, 2), _g(32, 4), why="first S the matrix-core path rejects at NQT 3"),
    AttnCase("m4x1_t49_s64", 49, 64, _m(4, 1), _m(4, 1), causal=True, drop=0.1, why="causal self-attention, dropout"),
    AttnCase("m4x4_t64_s200", 64, 200, _m(4, 4), _m(4, 4)),
    AttnCase("m4x5_t64_s320", 64, 320, _m(4, 5), _m(4, 5), causal=True, q_pos0="S-T", why="causal offset"),
    AttnCase("m4x8_t49_s512", 49, 512, _m(4, 8), _m(4, 8), why="largest S for NQT 4 at T = 49"),
    AttnCase("m4x8_t64_s416", 64, 416, _m(4, 8), _m(4, 8), causal=True, q_pos0="S-T",
             why="largest matrix-core shape at T = 64"),
    AttnCase("g_t64_s417", 64, 417, _g(32, 2), _g(32, 4), why="first S the matrix-core path rejects at T = 64"),
    # head widths on the matrix-core path
    AttnCase("m_dh8", 20, 40, _m(2, 1), _m(2, 1), dh=8, causal=True, why="narrow heads: 24 pad columns"),
    AttnCase("m_dh16", 33, 100, _m(3, 4), _m(3, 4), dh=16, drop=0.1),
    AttnCase("m_dh25_even_strides", 20, 216, _m(2, 4), _m(2, 4), dh=25,
             why="odd dh with even row strides: scalar dK / dV stores because of dh alone"),
    AttnCase("m_dh25_h12", 20, 20, _m(2, 1), _m(2, 1), dh=25, H=12, causal=True, why="a d = 300, H = 12 model"),
    AttnCase("m_dh32", 64, 300, _m(4, 5), _m(4, 5), dh=32, why="no pad columns"),
    # general kernels, DHP = 32: shapes the matrix-core path does not take
    AttnCase("g32_t1_s20", 1, 20, _g(32), _g(32), why="T = 1"),
    AttnCase("g32_t1_s814", 1, 814, _g(32), _g(32), why="largest S of the general backward at DHP 32"),
    AttnCase("g32_t257_s20", 257, 20, _g(32), _g(32), why="one chunk of more queries than threads"),
    AttnCase("g32_t300_s20", 300, 20, _g(32), _g(32), causal=True, why="one chunk of more queries than threads, causal"),
    AttnCase("g32_t300_s1", 300, 1, _g(32), _g(32), drop=0.1, why="one key, dropout"),
    AttnCase("g32_t80_s300", 80, 300, _g(32), _g(32, 2)),
    AttnCase("g32_t100_s600", 100, 600, _g(32, 4), _g(32, 15), drop=0.1, why="three key blocks, chunks both ways"),
    AttnCase("g32_t64_s512", 64, 512, _g(32, 2), _g(32, 4), causal=True, q_pos0="S-T",
             why="past the matrix-core LDS limit at T = 64"),
    # general kernels, DHP = 64 (33 <= dh <= 64)
    AttnCase("g64_dh33", 64, 64, _g(64), _g(64), dh=33, causal=True, why="one column past DHP 32"),
    AttnCase("g64_dh48_t20_s216", 20, 216, _g(64), _g(64), dh=48, drop=0.1),
    AttnCase("g64_dh64_t300_s20", 300, 20, _g(64), _g(64, 4), dh=64, causal=True, why="no pad columns, backward chunks"),
    AttnCase("g64_dh48_t100_s300", 100, 300, _g(64, 4), _g(64, 50), dh=48, why="two key blocks, chunks both ways"),
    AttnCase("g64_dh64_t1_s317", 1, 317, _g(64), _g(64), dh=64, why="largest S of the general backward at DHP 64"),
    AttnCase("g64_dh33_t257_s8", 257, 8, _g(64), _g(64, 2), dh=33, drop=0.1),
]

# just outside the documented limits: (direction, T, S, dh) the attention entry points reject with ICK_EINVAL
ATTN_REJECTED = [
    ("fwd", 2, 2, 65), ("bwd", 2, 2, 65),          # dh > 64
    ("fwd", 1, 1037, 30),                          # V does not fit the general forward's LDS even at one query
    ("fwd", 1, 556, 48),
    ("bwd", 1, 815, 30),                           # K + the staging tile do not fit the general backward's LDS
    ("bwd", 1, 318, 48),
]
# ... and just inside
ATTN_ACCEPTED = [("fwd", 1, 1036, 30), ("fwd", 1, 555, 48), ("bwd", 1, 814, 30), ("bwd", 1, 317, 48),
                 ("fwd", 2, 2, 64), ("bwd", 2, 2, 64)]


@dataclass(frozen=True)
class ChainCase:             # ick_rowchain_fwd
    name: str
    M: int
    K1: int
    d: int
    N2: int = 0
    relu: bool = False
    heads: tuple = None      # (nseg, H): y2 scattered head-major, T = M / B rows per sample
    B: int = 1
    slim: bool = False
    proj: bool = False       # ICK_CHAIN_PROJ: y2 = act(A W2^T + b2) only (K1 == d)
    drop1: float = 0.0
    drop2: float = 0.0
    why: str = ""


CHAIN = [
    ChainCase("f_m1_k16_d64_n64", 1, 16, 64, 64, why="narrowest"),
    ChainCase("f_m7_k300_d100_n65_relu", 7, 300, 100, 65, relu=True, drop1=0.2, why="ragged N2, d not a multiple of 64"),
    ChainCase("f_m8_k512_d320_n1024_slim", 8, 512, 320, 1024, slim=True, why="every limit at once, 8-wave form"),
    ChainCase("f_m9_k300_d320_n960_heads", 9, 300, 320, 960, heads=(3, 10), B=3, drop1=0.1,
              why="head-split y2 with dh = 32, one row past a workgroup"),
    ChainCase("f_m1280_k512_d256_n0", 1280, 512, 256, 0, why="norm only"),
    ChainCase("f_m1280_k300_d300_n1024_relu", 1280, 300, 300, 1024, relu=True, drop1=0.1, drop2=0.2),
    ChainCase("f_m9_k16_d64_n65_slim", 9, 16, 64, 65, relu=True, slim=True, drop2=0.3),
    ChainCase("f_proj_m7_d300_n65_relu", 7, 300, 300, 65, relu=True, proj=True, drop2=0.2, why="ICK_CHAIN_PROJ"),
    ChainCase("f_proj_m1280_d300_heads", 1280, 300, 300, 900, heads=(3, 10), B=64, proj=True,
              why="ICK_CHAIN_PROJ as the stack's first in_proj"),
    ChainCase("f_proj_m1_d64_n1024", 1, 64, 64, 1024, proj=True),
]


@dataclass(frozen=True)
class ChainBwdCase:          # ick_rowchain_bwd
    name: str
    M: int
    d: int
    K0: int = 0              # 0: no g0 W0 addend
    N1: int = 0              # 0: no FFN stage
    dzin: bool = True
    grouped: int = 0         # > 0: g0 is the (B, grouped, K0) context rows of a wider (B, S, K0) buffer (g0_grp)
    drop: float = 0.0        # dropout of both norms
    why: str = ""


CHAIN_BWD = [
    ChainBwdCase("b_m1_d64_k64", 1, 64, K0=64, why="narrowest"),
    ChainBwdCase("b_m7_d100_k0_n100", 7, 100, N1=100, why="no g0, ragged FFN"),
    ChainBwdCase("b_m9_d300_k1920_n512", 9, 300, K0=1920, N1=512, dzin=False, drop=0.2, why="widest K0 and N1"),
    ChainBwdCase("b_m160_d300_k1800_grp", 160, 300, K0=1800, grouped=20, drop=0.1,
                 why="the all-layer cross K/V gradient read through g0_grp"),
    ChainBwdCase("b_m160_d320_k900_n384", 160, 320, K0=900, N1=384, drop=0.3, why="widest d"),
    ChainBwdCase("b_m7_d64_k900_n512", 7, 64, K0=900, N1=512, dzin=False),
    ChainBwdCase("b_m160_d100_k64_n0", 160, 100, K0=64),
]


@dataclass(frozen=True)
class LnCase:                # ick_layernorm_bwd
    name: str
    rows: int
    d: int
    res: bool = True
    drop: float = 0.0
    atomics: bool = False    # partials == NULL: dgamma / dbeta accumulated with float atomics

    @property
    def nj(self):            # the layernorm_bwd_kernel<NJ> instantiation
        return 5 if self.d <= 320 else (8 if self.d <= 512 else 16)


LN = [
    LnCase("ln_d1_r7", 7, 1),
    LnCase("ln_d63_r9", 9, 63, res=False, drop=0.2),
    LnCase("ln_d300_r1280_atomics", 1280, 300, atomics=True),
    LnCase("ln_d320_r8", 8, 320, drop=0.1),
    LnCase("ln_d321_r1", 1, 321),
    LnCase("ln_d512_r9_atomics", 9, 512, drop=0.3, atomics=True),
    LnCase("ln_d513_r1280", 1280, 513, res=False),
    LnCase("ln_d1024_r7_atomics", 7, 1024, res=False, atomics=True),
    LnCase("ln_d1024_r8", 8, 1024, drop=0.1),
]

MFMA_INSTANTIATIONS = {(n, m) for n in (1, 2, 3, 4) for m in (1, 4, 5, 8)}
