"""Case table of the GEMM's envelope (csrc/gemm.hip, csrc/gemm_ps.hip; ick_gemm / ick_gemm_grouped).  Every case names
the kernel configuration ick_gemm_plan must report for it in each product mode (ick_set_gemm_split 0 / 1 / 2) as
(tile_m, tile_n, vec, split_bf16, presplit, split_k launched); tests/test_gemm_plan_cpu.py checks those plans against
the library and that the table together reaches every configuration the planner can choose,
tests/test_gemm_envelope_gpu.py runs every case against an exact integer reference and against float64.

Every case sits at the smallest shape that selects its configuration (make_plan): element-wise staging for ragged or
misaligned operands, 32 x 32 tiles below 512 tiles of 64 x 64, 64 x 64 from there on, 128 x 64 (eight waves) for long-K
narrow-N problems with a k-major A, 128 x 128 for split products from 512 such tiles on, and the three tiles of the
pre-split kernel (128 x 128, 64 x 160, 128 x 80).  WAVES gives the waves per workgroup ick_gemm_plan must report beside
each plan.  Grouped launches (ick_gemm_grouped) are not visible through ick_gemm_plan; GROUPED lists them by the plan
each member has alone.

Problem (below) lays a case out in memory exactly as include/ick_amd.h words the addressing, so both test modules build
the same ick_gemm_args: the CPU test on uninitialised host tensors (the planner looks at pointers, alignment and sizes
only), the GPU test on device copies with poisoned surroundings.
"""
from dataclasses import dataclass

EPILOGUES = ("bias", "relu", "alpha", "accumulate", "atomic", "drop", "gate", "headsplit", "c_gmap", "a_gmap", "colsum")
STAGINGS = ("vec", "ragged", "misaligned", "padded")


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    akm: bool                # A k-major (a_rs == 1)
    bkm: bool                # B k-major (b_rs == 1)
    want: tuple              # per product mode 0 / 1 / 2: (tile_m, tile_n, vec, split_bf16, presplit, split_k)
    split_k: int = 1
    staging: str = "vec"     # "vec" | "ragged" | "misaligned" (base one float off) | "padded" (NaN-padded leading dims)
    presplit: bool = False   # pass b_ps
    epi: tuple = ()          # out of EPILOGUES
    why: str = ""

    @property
    def layout(self):
        return (self.akm, self.bkm)

    @property
    def atomic(self):
        return "atomic" in self.epi or self.split_k > 1

    def modes(self):
        """The product modes to run: the first mode of every distinct plan."""
        return [m for m in (0, 1, 2) if self.want[m] not in self.want[:m]]


CC, MC, CM, MM = (False, False), (True, False), (False, True), (True, True)
LAYOUTS = (CC, MC, CM, MM)


def _w(tm, tn, vec=1, spl=0, ps=0, k=1):
    return (tm, tn, vec, spl, ps, k)


def _all(w):
    return (w, w, w)


def _elem(k=1):              # element-wise staging: always the exact 64 x 64 tile
    return _all(_w(64, 64, vec=0, k=k))


def _small(k=1):             # 32 x 32 tiles: always exact
    return _all(_w(32, 32, k=k))


def _big(layout, k=1):       # 64 x 64 tiles: split products in mode 1 when B is k-contiguous, in mode 2 always
    e, s = _w(64, 64, k=k), _w(64, 64, spl=1, k=k)
    return (e, e if layout[1] else s, s)


def _xl(layout):             # 128 x 128 tiles where the products are split, 64 x 64 exact tiles otherwise
    e, x = _w(64, 64), _w(128, 128, spl=1)
    return (e, e if layout[1] else x, x)


def _wide():                 # 128 x 64, eight waves (k-major A, k-contiguous B): split from mode 1 on
    return (_w(128, 64), _w(128, 64, spl=1), _w(128, 64, spl=1))


def _ps(tile, mode0, vec=1, k=1):
    p = _w(tile[0], tile[1], vec=vec, spl=1, ps=1, k=k)
    return (mode0, p, p)


# waves per workgroup by plan family: (tile_m, tile_n, presplit) -> waves.  Element-wise staging runs on the 64 x 64 tile.
WAVES = {
    (32, 32, 0): 4, (64, 64, 0): 4, (64, 160, 1): 4,
    (128, 64, 0): 8, (128, 128, 1): 8, (128, 80, 1): 8,
    (128, 128, 0): 4,        # stager-split: four waves of 64 x 64
}


def waves(w):
    """Waves per workgroup of a plan tuple (tile_m, tile_n, vec, split_bf16, presplit, split_k)."""
    return WAVES[(w[0], w[1], w[4])]


def C(name, shape, layout, want, **kw):
    M, N, K = shape
    return Case(name, M, N, K, layout[0], layout[1], want, **kw)


E1, E2 = (37, 53, 19), (36, 52, 20)
CASES = [
    # ---- element-wise staging (64 x 64 tile, exact in every mode): ragged sizes or a base pointer off 16-byte alignment
    C("e_cc_ragged", E1, CC, _elem(), staging="ragged", epi=("bias", "relu"), why="odd M, N, K; one partial slice"),
    C("e_cm_ragged", E1, CM, _elem(), staging="ragged", epi=("gate",)),
    C("e_mm_ragged", E1, MM, _elem(), staging="ragged", epi=("drop", "colsum")),
    C("e_cc_misaligned", E2, CC, _elem(), staging="misaligned", epi=("bias", "headsplit"),
      why="vector-legal sizes, base one float off"),
    C("e_mc_misaligned", E2, MC, _elem(), staging="misaligned", epi=("c_gmap", "a_gmap", "bias")),
    C("e_cm_misaligned", E2, CM, _elem(), staging="misaligned", epi=("a_gmap",)),
    C("e_mm_misaligned_k2", (36, 52, 68), MM, _elem(k=2), split_k=2, staging="misaligned", epi=("colsum",),
      why="odd slice count cut in two: 64 + 4"),
    C("e_cc_padded", E1, CC, _elem(), staging="padded", epi=("alpha", "accumulate"),
      why="NaN between the odd extents and the next multiple of 4"),
    C("e_mm_padded", E1, MM, _elem(), staging="padded", epi=("bias",)),
    C("e_mm_69x133x100_k3", (69, 133, 100), MM, _elem(k=2), split_k=3, staging="ragged", epi=("bias",),
      why="2 x 3 tiles (tiles_m <= tiles_n); 3 slices asked, chunks of 64 give 2"),
    C("e_mc_133x69x36", (133, 69, 36), MC, _elem(), staging="ragged", epi=("relu", "colsum"),
      why="3 x 2 tiles (tiles_m > tiles_n), two slices, column sums from the first tile column only"),
    C("e_cm_a_gmap_ragged", E1, CM, _elem(), staging="ragged", epi=("a_gmap", "c_gmap"), why="partial last group"),
    # ---- 32 x 32 vector tile (fewer than 512 tiles of 64 x 64; exact in every mode)
    C("s_cc", E2, CC, _small(), epi=("bias", "relu"), why="M, N one group of 4 past a tile; one partial slice"),
    C("s_mc", E2, MC, _small(), staging="padded", epi=("alpha", "accumulate", "colsum"), why="two tile columns: colsum once"),
    C("s_cm", E2, CM, _small(), staging="padded", epi=("gate",)),
    C("s_mm", E2, MM, _small(), epi=("drop",)),
    C("s_cc_headsplit", (36, 52, 36), CC, _small(), staging="padded", epi=("headsplit", "bias"), why="two slices"),
    C("s_mc_c_gmap", (36, 52, 68), MC, _small(), epi=("c_gmap", "a_gmap"), why="odd slice count"),
    C("s_cm_a_gmap", (36, 52, 100), CM, _small(), staging="padded", epi=("a_gmap",), why="four slices, tail of 4"),
    C("s_mm_k100_s8", (36, 52, 100), MM, _small(k=4), split_k=8, epi=("colsum", "bias"),
      why="8 slices asked, K = 100 gives 4: no split-major order"),
    C("s_mc_k100_s3", (36, 52, 100), MC, _small(k=2), split_k=3, epi=("alpha",), why="chunks of 64: 2 slices, short last"),
    C("s_cm_k228_s8", (36, 52, 228), CM, _small(k=8), split_k=8, epi=("drop",),
      why="split-major order over 4 tiles (not a multiple of 8), last slice of 4"),
    C("s_cc_k484_s16", (68, 36, 484), CC, _small(k=16), split_k=16, epi=("bias",),
      why="16 slices, split-major, 3 x 2 tiles (tiles_m > tiles_n)"),
    C("s_cc_below_512", (1412, 1348, 68), CC, _small(), why="23 x 22 = 506 tiles of 64 x 64: still 32 x 32 (1935 tiles)"),
    C("s_mm_below_512", (1412, 1348, 36), MM, _small(), staging="padded"),
    # ---- 64 x 64 vector tile (>= 512 tiles of 64 x 64 times split_k): exact, and split where the mode says so
    C("b_cc", (1412, 1412, 36), CC, _big(CC), staging="padded", epi=("bias", "relu"), why="23 x 23 = 529 tiles, ragged edges"),
    C("b_mc", (1412, 1412, 36), MC, _big(MC), staging="padded", epi=("alpha", "accumulate", "colsum"),
      why="column sums from registers on the split tile"),
    C("b_cm", (1412, 1412, 68), CM, _big(CM), staging="padded", epi=("gate",), why="ragged M and N on a mixed layout"),
    C("b_mm", (1412, 1412, 20), MM, _big(MM), staging="padded", epi=("drop", "colsum")),
    C("b_cc_headsplit", (1412, 1412, 100), CC, _big(CC), epi=("headsplit",)),
    C("b_mc_gmaps", (1412, 1412, 20), MC, _big(MC), epi=("c_gmap", "a_gmap", "bias")),
    C("b_cm_gmaps", (1412, 1412, 36), CM, _big(CM), staging="padded", epi=("c_gmap", "a_gmap")),
    C("b_cc_above_512", (1348, 1476, 20), CC, _big(CC), why="22 x 24 = 528 tiles: the other side of s_cc_below_512"),
    C("b_mc_k68_s3", (900, 836, 68), MC, _big(MC, k=3), split_k=3, epi=("colsum",), why="15 x 14 x 3 = 630; slices 32, 32, 4"),
    C("b_mm_k228_s8", (388, 580, 228), MM, _big(MM, k=8), split_k=8, epi=("colsum", "alpha"),
      why="split-major order over 7 x 10 = 70 tiles (not a multiple of 8)"),
    C("b_cm_k484_s16", (580, 260, 484), CM, _big(CM, k=16), split_k=16, staging="padded", epi=("drop",),
      why="16 slices over 10 x 5 tiles (tiles_m > tiles_n)"),
    C("b_cc_k100_s8", (452, 580, 100), CC, _big(CC, k=4), split_k=8, why="8 slices asked for the tile choice, 4 launched"),
    C("b_mc_wide_split_k", (6596, 260, 1028), MC, _big(MC, k=2), split_k=2, why="a K split keeps the 128 x 64 shape on 64 x 64"),
    C("b_cc_wide_layout", (6596, 260, 1028), CC, _big(CC), epi=("bias",), why="k-contiguous A keeps it on 64 x 64"),
    # ---- 128 x 64 eight-wave tile
    C("w_mc", (6596, 260, 1028), MC, _wide(), staging="padded", epi=("bias", "relu", "colsum"),
      why="M = 51 x 128 + 68, N = 4 x 64 + 4, K = 32 x 32 + 4"),
    C("w_mc_below_512", (6468, 260, 1028), MC, _small(), why="102 x 5 = 510 tiles of 64 x 64: 32 x 32 (M >= 4096 is implied)"),
    C("w_mc_below_k", (6596, 260, 1020), MC, _big(MC), why="K < 1024"),
    C("w_mc_above_n", (6596, 324, 1028), MC, _big(MC), why="N > 320"),
    # ---- 128 x 128 tile (split products, >= 512 tiles of 128 x 128, last tile column wastes at most N / 8)
    C("x_cc", (2820, 2948, 36), CC, _xl(CC), staging="padded", epi=("bias", "relu"), why="23 x 24 = 552 tiles"),
    C("x_mc", (2820, 2948, 20), MC, _xl(MC), staging="padded", epi=("alpha", "accumulate", "colsum")),
    C("x_cm", (2820, 2948, 68), CM, _xl(CM), staging="padded", epi=("gate",), why="mode 2 only: transposing reads of B"),
    C("x_mm", (2820, 2948, 100), MM, _xl(MM), epi=("drop",), why="mode 2 only: both operands through the 128-row block swap"),
    C("x_cc_headsplit", (2820, 2900, 36), CC, _xl(CC), epi=("headsplit", "a_gmap", "bias"),
      why="23 x 23 = 529 tiles; gathered rows into the head-major layout"),
    C("x_mm_gmaps", (2820, 2900, 36), MM, _xl(MM), staging="padded", epi=("c_gmap", "a_gmap", "colsum")),
    C("x_cc_below_512", (2820, 2692, 36), CC, _big(CC), why="23 x 22 = 506 tiles of 128 x 128: 64 x 64"),
    C("x_cc_n132", (32772, 132, 20), CC, _big(CC), why="257 x 2 tiles of 128 x 128 would waste 124 of 256 columns"),
    # ---- pre-split B (b_ps): csrc/gemm_ps.hip from mode 1 on; mode 0 never looks at the copy
    C("p128_cc", (1284, 644, 612), CC, _ps((128, 128), _w(32, 32)), presplit=True, staging="padded", epi=("bias", "relu", "drop"),
      why="flop just above 1e9; 11 x 6 tiles; K = 19 x 32 + 4"),
    C("p128_mc", (1284, 644, 612), MC, _ps((128, 128), _w(32, 32)), presplit=True, staging="padded", epi=("alpha", "accumulate")),
    C("p128_cc_gate", (1284, 644, 612), CC, _ps((128, 128), _w(32, 32)), presplit=True, epi=("gate",)),
    C("p128_mc_headsplit", (1284, 644, 612), MC, _ps((128, 128), _w(32, 32)), presplit=True, epi=("headsplit", "a_gmap", "bias")),
    C("p128_cc_gmaps", (1284, 644, 612), CC, _ps((128, 128), _w(32, 32)), presplit=True, staging="padded",
      epi=("c_gmap", "a_gmap")),
    C("p128_cc_k5", (260, 388, 9700), CC, _ps((128, 128), _w(32, 32, k=5), k=5), presplit=True, split_k=5, epi=("bias",),
      why="3 x 4 tiles x 5 slices of 1952, last 1892"),
    C("p128_mc_k5", (260, 388, 9700), MC, _ps((128, 128), _w(32, 32, k=5), k=5), presplit=True, split_k=5, staging="padded"),
    C("p128_below_flop", (1284, 644, 604), CC, _small(), presplit=True, why="flop just below 1e9: the copy is ignored"),
    C("p128_below_m", (252, 388, 9700), CC, _small(k=5), presplit=True, split_k=5, why="M < 256"),
    C("p128_below_n", (260, 124, 15600), CC, _small(k=5), presplit=True, split_k=5, why="N < 128"),
    C("p64x160_cc", (4100, 164, 772), CC, _ps((64, 160), _w(32, 32)), presplit=True, epi=("bias",),
      why="33 x 2 row tiles of 128 underfill the chip, 65 x 2 of 64 do not"),
    C("p64x160_mc", (4100, 164, 772), MC, _ps((64, 160), _w(32, 32)), presplit=True, staging="padded", epi=("alpha", "accumulate")),
    C("p64x160_below", (3972, 164, 772), CC, _small(), presplit=True, why="63 x 2 = 126 tiles of 64 x 160: too few"),
    C("p64x160_top", (11268, 164, 292), MC, _ps((64, 160), _w(64, 64)), presplit=True,
      why="89 x 2 = 178 tiles of 128 rows: the last underfilled size"),
    C("p128x80_cc", (11524, 164, 292), CC, _ps((128, 80), _w(64, 64)), presplit=True, staging="padded", epi=("bias", "relu"),
      why="91 x 2 = 182 tiles of 128 rows fill the chip"),
    C("p128x80_mc", (11524, 164, 292), MC, _ps((128, 80), _w(64, 64)), presplit=True, epi=("drop",)),
    C("p128x80_cc_k5", (260, 132, 14800), CC, _ps((128, 80), _w(32, 32, k=5), k=5), presplit=True, split_k=5, epi=("bias",),
      why="narrow split-K problem"),
    C("p128x80_mc_k5", (260, 132, 14800), MC, _ps((128, 80), _w(32, 32, k=5), k=5), presplit=True, split_k=5, staging="padded"),
]


@dataclass(frozen=True)
class GroupCase:             # one ick_gemm_grouped call
    name: str
    members: tuple           # Cases; `want` is the plan each has ALONE (ick_gemm_plan does not see the group)
    modes: tuple = (0,)
    rider: tuple = None      # (rows, cols, split_k): a plain column-sum problem (ICK_GEMM_COLSUM_ONLY) riding along
    promoted: bool = False   # the small both-k-major members together reach 512 tiles of 64 x 64: they run on 64 x 64
    why: str = ""


def _pair(tag, layout, big):
    """Two problems of one configuration: they share one grouped launch."""
    if big:
        shapes, want = ((1412, 1412, 20), (1348, 1476, 36)), _big(layout)
    else:
        shapes, want = ((36, 52, 20), (68, 36, 36)), _small()
    epi = (("colsum",) if layout[0] else ("bias",), ("alpha", "accumulate"))
    return tuple(C("%s_%d" % (tag, i), s, layout, want, epi=e, staging=("vec", "padded")[i])
                 for i, (s, e) in enumerate(zip(shapes, epi)))


GROUPED = [
    GroupCase("g32_cc", _pair("g32_cc", CC, False)),
    GroupCase("g32_mc", _pair("g32_mc", MC, False)),
    GroupCase("g32_cm", _pair("g32_cm", CM, False)),
    GroupCase("g64_cc", _pair("g64_cc", CC, True), modes=(0, 2)),
    GroupCase("g64_mc", _pair("g64_mc", MC, True), modes=(0, 2)),
    GroupCase("g64_cm", _pair("g64_cm", CM, True), modes=(0, 2)),
    GroupCase("g64_mm", _pair("g64_mm", MM, True), modes=(0, 2)),
    GroupCase("g_cut", tuple(C("g_cut_%d" % i, (36 + 4 * (i % 3), 52, 20 + 16 * (i % 2)), MM, _small(), epi=("colsum",))
                             for i in range(10)),
              why="ten problems of one configuration: launches of eight and two (kGroupMax)"),
    GroupCase("g_padding", (C("g_pad_0", (68, 36, 68), MM, _small(k=3), split_k=3, epi=("colsum",)),
                            C("g_pad_1", (36, 52, 228), MM, _small(k=8), split_k=8),
                            C("g_pad_2", (100, 36, 100), MM, _small(k=2), split_k=2, epi=("alpha",))),
              why="6 x 3 = 18, 4 x 8 = 32 (split-major) and 8 x 2 = 16 workgroups: padding workgroups behind the first"),
    GroupCase("g_promoted", tuple(C("g_prom_%d" % i, (644, 644 + 64 * i, 36 + 32 * i), MM, _small(k=1 + (i == 2)),
                                    split_k=1 + (i == 2), epi=("colsum",)) for i in range(4)),
              modes=(0, 2), promoted=True,
              why="11 x (11 + 12 + 13 x 2 + 14) = 693 tiles of 64 x 64 together: promoted to 64 x 64 (force_big)"),
    GroupCase("g_mix", (C("g_mix_cc32", (36, 52, 36), CC, _small(), epi=("bias", "relu")),
                        C("g_mix_mm32a", (36, 52, 100), MM, _small(k=4), split_k=4, epi=("colsum",)),
                        C("g_mix_elem", E1, MM, _elem(), staging="ragged", epi=("colsum",)),
                        C("g_mix_mm64", (1412, 1412, 20), MM, _big(MM)),
                        C("g_mix_mm32b", (68, 36, 20), MM, _small(), staging="padded"),
                        C("g_mix_cc32b", (68, 36, 68), CC, _small(), epi=("alpha", "accumulate"))),
              modes=(0, 2), rider=(228, 52, 2),
              why="three configurations, a single element-wise launch and a column-sum rider in one call"),
]

# arguments ick_gemm_plan must answer with ICK_EINVAL: (note, keyword overrides of a plain 64 x 64 x 64 problem)
REJECTED = [
    ("neither stride of A is 1", dict(a_rs=128, a_ks=2)),
    ("neither stride of B is 1", dict(b_rs=128, b_ks=2)),
    ("M = 0", dict(M=0)),
    ("N = 0", dict(N=0)),
    ("K = 0", dict(K=0)),
    ("split_k > 1 without atomic", dict(split_k=2)),
    ("gate with accumulate", dict(gate=True, accumulate=True)),
    ("gate with atomic", dict(gate=True, atomic=True)),
    ("gate with split_k", dict(gate=True, atomic=True, split_k=2)),
    ("gate with head split", dict(gate=True, headsplit=True)),
    ("colsum_a on a k-contiguous A", dict(colsum=True)),
    ("m_bound with dropout", dict(m_bound=True, drop=True)),
    ("m_bound with gate", dict(m_bound=True, gate=True)),
    ("m_bound with colsum_a", dict(m_bound=True, colsum=True, a_rs=1, a_ks=64)),
    ("ReLU with split_k > 1", dict(relu=True, atomic=True, split_k=2)),
]
# ... and their neighbours it must accept
ACCEPTED = [
    ("plain", dict()),
    ("split_k with atomic", dict(atomic=True, split_k=2)),
    ("ReLU without a split", dict(relu=True)),
    ("ReLU with atomic, one slice", dict(relu=True, atomic=True)),
    ("gate alone", dict(gate=True)),
    ("colsum_a on a k-major A", dict(colsum=True, a_rs=1, a_ks=64)),
    ("m_bound alone", dict(m_bound=True)),
]


# --------------------------------------------------------------------------------------------------- memory layout
GUARD = 1234.5               # value of the memory around an output
DROP_P, DROP_SITE = 0.5, 7   # keep scale 2: exact on integers
GATE_SCALE = 2.0


def ceil4(n):
    return (n + 3) // 4 * 4


def a_group(M):
    """Group size of the a_gmap cases: a multiple of 4 (vector staging of a k-major A) that is no multiple of a tile."""
    for g in (12, 20, 4):
        if M % g == 0:
            return g
    return 10


def c_group(M):
    return -(-M // 4)


def value_bound(c):
    """|output| of the exact-integer run is at most this (operands, bias and old values in -3 .. 3)."""
    return 9 * c.K * 2 * 2 * 2 + 3 + 3


class Operand:
    """One GEMM operand laid out as include/ick_amd.h addresses it: element (r, k) of the logical (rows, K) matrix lives
    at index[r, k] of the flat buffer, = off + goff(r) + (r % grp) * rs + k * ks.  Padding (between the logical extent of
    a line and its leading dimension, behind the last line, between groups) is NaN."""

    def __init__(self, torch, rows, K, kmajor, staging, pad, grp=0, gmap=None):
        self.rows, self.K, self.kmajor = rows, K, kmajor
        padded = staging == "padded"
        self.off = 1 if staging == "misaligned" else 0
        block = min(grp, rows) if grp else rows            # rows per group
        ngroups = -(-rows // grp) if grp else 1
        if kmajor:
            ld = ceil4(block) + pad if padded else block
            self.rs, self.ks = 1, ld
            lines, ext = K, block
        else:
            ld = ceil4(K) + pad if padded else K
            self.rs, self.ks = ld, 1
            lines, ext = block, K
        self.grp = grp
        self.gs = (lines * ld + (4 if padded else 0)) if grp else 0
        # the last line ends two floats behind its logical extent: the addressable extent ends mid-float4
        last = (lines - 1) * ld + ext + (2 if padded else 0)
        self.size = self.off + ((ngroups - 1) * self.gs + last if grp else last)
        r = torch.arange(rows, dtype=torch.long)
        if grp:
            g = r // grp
            goff = (gmap.long()[g] if gmap is not None else g) * self.gs
            r = r % grp
        else:
            goff = torch.zeros_like(r)
        self.index = (self.off + goff + r * self.rs).view(-1, 1) + torch.arange(K, dtype=torch.long).view(1, -1) * self.ks
        assert int(self.index.max()) < self.size

    def fill(self, torch, values, device):
        buf = torch.full((self.size,), float("nan"), dtype=torch.float32)
        buf[self.index.reshape(-1)] = values.reshape(-1).float()
        self.buf = buf.to(device)
        return self.view()

    def empty(self, torch):
        self.buf = torch.empty(self.size, dtype=torch.float32)
        return self.view()

    def view(self):
        return self.buf[self.off:]

    def matrix(self, torch):
        """The (rows, K) strided view (no groups)."""
        assert not self.grp
        return torch.as_strided(self.buf, (self.rows, self.K), (self.rs, self.ks), self.off)


class Output:
    """C inside a larger buffer: logical element (m, n) at index[m, n] of the flat buffer; guard floats in front and
    behind, a leading dimension larger than N, a guard row between row groups, head-split pad columns."""

    def __init__(self, torch, c, cmap):
        M, N = c.M, c.N
        m = torch.arange(M, dtype=torch.long)
        n = torch.arange(N, dtype=torch.long)
        self.c_grp = self.c_gs = self.c_rs = 0
        self.hs = None
        if "headsplit" in c.epi:
            assert M % 4 == 0 and N % 4 == 0
            nseg, H, dh = 2, 2, N // 4
            dhp, grp, s0 = dh + 3, M // 4, 2
            S = grp + s0 + 1
            assert (H * dh) % 16 != 0
            self.hs = (dh, dhp, H, S, s0)
            self.base = 7
            self.c_grp, self.c_gs = grp, nseg * H * S * dhp + 5
            g = m // grp
            row = (cmap.long()[g] if cmap is not None else g) * self.c_gs + (s0 + m % grp) * dhp
            seg, r = n // (H * dh), n % (H * dh)
            col = (seg * H + r // dh) * (S * dhp) + r % dh
            groups = 4
            self.size = self.base + groups * self.c_gs + 9
        else:
            ldc = N + 3
            self.c_rs = ldc
            self.base = 2 * ldc + 1
            if cmap is not None:
                grp = c_group(M)
                self.c_grp, self.c_gs = grp, (grp + 1) * ldc
                row = cmap.long()[m // grp] * self.c_gs + (m % grp) * ldc
                rows = len(cmap) * (grp + 1)
            else:
                row, rows = m * ldc, M
            col = n
            self.size = self.base + rows * ldc + 2 * ldc
        self.index = self.base + row.view(-1, 1) + col.view(1, -1)
        assert int(self.index.min()) >= self.base and int(self.index.max()) < self.size
        assert M * N > 1 << 16 or self.index.unique().numel() == M * N


class Problem:
    """One case in memory.  fill: None (uninitialised host tensors: the plan only), "int" (operands, bias and old values
    integers in -3 .. 3) or "float" (uniform operands as in tests/test_ops_gpu.py).  reference() is the float64 result of
    the documented formula, exact for the integer fill."""

    def __init__(self, torch, ops, c, fill=None, device="cpu", seed=0):
        self.c, self.torch, self.ops, self.filled = c, torch, ops, fill
        g = torch.Generator().manual_seed(seed)
        M, N, K = c.M, c.N, c.K
        perm = lambda n: torch.randperm(n, generator=g).int()
        if fill == "int":
            draw = lambda *s: torch.randint(-3, 4, s, generator=g).double()
            draw_b = draw
        else:
            draw = lambda *s: (torch.rand(*s, generator=g) * 2 - 1).float().double()
            draw_b = lambda *s: ((torch.rand(*s, generator=g) * 2 - 1) * 0.1).float().double()
        agrp = a_group(M) if "a_gmap" in c.epi else 0
        self.amap = perm(-(-M // agrp)) if agrp else None
        self.cmap = perm(4) if "c_gmap" in c.epi else None
        self.opA = Operand(torch, M, K, c.akm, c.staging, 4, agrp, self.amap)
        self.opB = Operand(torch, N, K, c.bkm, c.staging, 8)
        self.out = Output(torch, c, self.cmap)
        dev = lambda t: None if t is None else t.to(device)
        self.keep = []
        kw = dict(relu="relu" in c.epi, accumulate="accumulate" in c.epi, atomic=c.atomic, split_k=c.split_k,
                  alpha=2.0 if "alpha" in c.epi else 1.0)
        self.Am = self.Bm = self.bias = self.old = self.gate = self.cs_old = self.mask = None
        if fill is None:
            A, B = self.opA.empty(torch), self.opB.empty(torch)
            self.cbuf = torch.empty(self.out.size, dtype=torch.float32)
        else:
            self.Am, self.Bm = draw(M, K), draw_b(N, K)
            A, B = self.opA.fill(torch, self.Am, device), self.opB.fill(torch, self.Bm, device)
            init = torch.full((self.out.size,), GUARD, dtype=torch.float32)
            if "accumulate" in c.epi or c.atomic:
                self.old = draw(M, N)
                init[self.out.index.reshape(-1)] = self.old.reshape(-1).float()
            else:
                init[self.out.index.reshape(-1)] = float("nan")      # overwritten
            self.cinit = init
            self.cbuf = init.to(device)
        if "bias" in c.epi:
            self.bias = draw(N) if fill else torch.empty(N)
            kw["bias"] = dev(self.bias.float())
        if self.amap is not None:
            kw.update(a_grp=agrp, a_gs=self.opA.gs, a_gmap=dev(self.amap))
        if self.out.c_grp:
            kw.update(c_grp=self.out.c_grp, c_gs=self.out.c_gs, c_gmap=dev(self.cmap))
        if "gate" in c.epi:
            self.gate_rs = N + 7
            gbuf = torch.full((M, self.gate_rs), float("nan"))
            if fill:
                self.gate = torch.randint(-1, 3, (M, N), generator=g).double()      # zeros, negatives, positives
                gbuf[:, :N] = self.gate.float()
            kw.update(gate=dev(gbuf), gate_scale=GATE_SCALE)
        if "drop" in c.epi:
            self.drop = (DROP_P, 4321 + seed, DROP_SITE)
            kw["drop"] = self.drop
        if "colsum" in c.epi:
            cs = torch.full((M + 6,), GUARD)
            if fill:
                self.cs_old = draw(M)
                cs[3:3 + M] = self.cs_old.float()
            self.csbuf = dev(cs)
            kw["colsum_a"] = self.csbuf[3:]
        if c.presplit:
            self.b_ps = torch.empty(ops.presplit_bytes(N, K), dtype=torch.uint8, device=device)
            if fill:
                ops.presplit_weights([(self.opB.matrix(torch), self.b_ps)])
            kw["b_ps"] = self.b_ps
        self.keep.append(kw)
        self.args = ops.gemm_args(A, B, self.cbuf[self.out.base:], M, N, K, self.opA.rs, self.opA.ks, self.opB.rs,
                                  self.opB.ks, self.out.c_rs, **kw)
        if self.out.hs:
            a = self.args
            a.hs_dh, a.hs_dhp, a.hs_H, a.hs_S, a.hs_s0 = self.out.hs

    def plan(self):
        p = self.ops.gemm_plan(self.args)
        return (p["tile_m"], p["tile_n"], p["vec"], p["split_bf16"], p["presplit"], p["split_k"])

    def reference(self):
        """(C values (M, N), column sums (M) or None) in float64."""
        torch, c = self.torch, self.c
        v = self.Am @ self.Bm.t()
        if "alpha" in c.epi:
            v = v * 2.0
        if self.bias is not None:
            v = v + self.bias
        if "relu" in c.epi:
            v = v.relu()
        if "drop" in c.epi:
            if self.mask is None:
                self.mask = self.ops.dropout_mask(c.M, c.N, *self.drop).cpu().double()
            v = v * self.mask
        if self.gate is not None:
            v = torch.where(self.gate > 0, v * GATE_SCALE, torch.zeros_like(v))
        if self.old is not None:
            v = v + self.old
        cs = self.cs_old + self.Am.sum(1) if self.cs_old is not None else None
        return v, cs
