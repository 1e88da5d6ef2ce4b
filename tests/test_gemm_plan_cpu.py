"""Without a GPU: the GEMM envelope's case table (tests/gemm_cases.py) against the kernel configuration the library
reports (ick_gemm_plan, the function ick_gemm launches by) in all three product modes, its coverage of every
configuration the planner can choose, and the argument combinations the planner rejects.  The planner looks at
pointers, alignment and sizes only, so uninitialised host tensors stand in for the operands."""
import ctypes as C

import pytest
import torch

from gemm_cases import (ACCEPTED, CASES, CC, CM, EPILOGUES, GROUPED, LAYOUTS, MC, MM, REJECTED, STAGINGS, Problem,
                        a_group, value_bound, waves)


@pytest.fixture(scope="module")
def ops():
    import ick_amd.build as build
    build.build()
    import ick_amd.ops as ops
    before = ops.gemm_split_mode()
    yield ops
    ops.set_gemm_split(before)


def family(w):
    """Name of the kernel family behind a plan tuple (tile_m, tile_n, vec, split_bf16, presplit, split_k)."""
    tm, tn, vec, spl, ps, _ = w
    if ps:
        return "ps%dx%d" % (tm, tn)
    if not vec:
        return "elem"
    return "%dx%d%s" % (tm, tn, "s" if spl else "")


def features(c):
    """What a table row contributes: (plan family, layout, mode) and, per family it runs on, its epilogues, staging, K,
    requested -> launched K split; and its shape (the planner's thresholds are pinned by shape)."""
    f = {("shape", c.M, c.N, c.K, c.layout, c.split_k, c.presplit)}
    for mode in (0, 1, 2):
        fam = family(c.want[mode])
        f.add(("plan", fam, c.layout, mode))
        f.update(("epi", fam, e) for e in c.epi)
        f.add(("staging", fam, c.staging))
        f.add(("staging", fam, c.layout, c.staging))
        f.add(("K", fam, c.K))
        f.add(("K", fam, c.layout, c.K))
        f.add(("split", fam, c.split_k, c.want[mode][5]))
        f.add(("split", fam, c.layout, c.split_k, c.want[mode][5]))
        if "a_gmap" in c.epi:
            f.add(("a_gmap", fam, c.akm))
            if c.M % a_group(c.M):
                f.add(("a_gmap with a partial last group", fam))
        if "colsum" in c.epi and c.N > c.want[mode][1]:
            f.add(("colsum over tile columns", fam))
    return f


# ---- what the table must reach, written out ------------------------------------------------------------------------
def required():
    r = set()
    every = [(l, m) for l in LAYOUTS for m in (0, 1, 2)]
    # element-wise staging and the 32 x 32 tile: every layout, exact in every mode
    r.update(("plan", fam, l, m) for fam in ("elem", "32x32") for l, m in every)
    # 64 x 64: exact in mode 0, and in mode 1 for a k-major B; split in mode 1 for a k-contiguous B and in mode 2
    r.update(("plan", "64x64", l, 0) for l in LAYOUTS)
    r.update(("plan", "64x64", l, 1) for l in (CM, MM))
    r.update(("plan", "64x64s", l, 1) for l in (CC, MC))
    r.update(("plan", "64x64s", l, 2) for l in LAYOUTS)
    # 128 x 64, eight waves: k-major A with a k-contiguous B only
    r.update({("plan", "128x64", MC, 0), ("plan", "128x64s", MC, 1), ("plan", "128x64s", MC, 2)})
    # 128 x 128: the layouts mode 1 splits, all four in mode 2
    r.update(("plan", "128x128s", l, 1) for l in (CC, MC))
    r.update(("plan", "128x128s", l, 2) for l in LAYOUTS)
    # the pre-split tiles the planner picks itself: A both ways
    r.update(("plan", fam, l, m) for fam in ("ps128x128", "ps64x160", "ps128x80") for l in (CC, MC) for m in (1, 2))
    # every epilogue on the element-wise tile, 32 x 32, 64 x 64 exact and split, 128 x 128 and one pre-split tile
    epis = ("bias", "relu", "alpha", "accumulate", "gate", "drop", "headsplit", "c_gmap", "a_gmap")
    for fam in ("elem", "32x32", "64x64", "64x64s", "128x128s", "ps128x128"):
        r.update(("epi", fam, e) for e in epis)
    for fam in ("elem", "32x32", "64x64", "64x64s", "128x64", "128x64s", "128x128s"):
        r.add(("epi", fam, "colsum"))                 # (never beside b_ps: the planner then ignores the copy)
        r.add(("colsum over tile columns", fam))
    # operand views
    r.update(("staging", "elem", l, s) for l in LAYOUTS for s in ("ragged", "misaligned"))
    r.update(("staging", "elem", l, "padded") for l in (CC, MM))
    for fam in ("32x32", "64x64", "64x64s", "128x128s", "ps128x128", "ps64x160", "ps128x80"):
        r.update({("staging", fam, "vec"), ("staging", fam, "padded")})
    r.update({("staging", "128x64", "padded"), ("staging", "128x64s", "padded")})
    r.update(("staging", "32x32", l, "padded") for l in LAYOUTS)
    r.update(("staging", fam, l, "padded") for fam in ("64x64", "128x128s") for l in LAYOUTS)
    # gathered A rows (a_gmap) on a k-contiguous and on a k-major A
    r.update(("a_gmap", fam, akm) for fam in ("elem", "32x32", "64x64", "64x64s", "128x128s", "ps128x128")
             for akm in (False, True))
    r.add(("a_gmap with a partial last group", "elem"))
    # pipeline depth: one partial slice, two slices, an odd count, four slices with a tail of four
    for fam in ("elem", "32x32", "64x64", "64x64s", "128x128s"):
        r.update(("K", fam, k) for k in (20, 36, 68, 100))
    r.add(("K", "elem", 19))
    r.update(("K", "32x32", l, 20) for l in LAYOUTS)
    # two slices, an odd slice count and a tail of 4 away from the both-k-major layout
    r.update({("K", "32x32", CC, 36), ("K", "32x32", MC, 68), ("K", "32x32", CM, 100)})
    r.add(("K", "64x64s", MM, 20))                                   # one partial slice through both transposing reads
    # K split on the gemm.hip tiles: (requested, launched)
    r.update(("split", "elem", *s) for s in ((2, 2), (3, 2)))
    r.update(("split", "32x32", *s) for s in ((3, 2), (8, 4), (8, 8), (16, 16)))
    for fam in ("64x64", "64x64s"):
        r.update(("split", fam, *s) for s in ((2, 2), (3, 3), (8, 4), (8, 8), (16, 16)))
    r.update(("split", fam, l, k, k) for fam in ("ps128x128", "ps128x80") for l in (CC, MC) for k in (1, 5))
    # both sides of the planner's thresholds, by shape: (M, N, K, layout, split_k, presplit)
    r.update(("shape",) + s for s in (
        (1412, 1348, 68, CC, 1, False), (1348, 1476, 20, CC, 1, False),         # 506 / 528 tiles of 64 x 64
        (1412, 1348, 36, MM, 1, False),
        (6596, 260, 1028, MC, 1, False), (6468, 260, 1028, MC, 1, False),       # 128 x 64: 520 / 510 tiles,
        (6596, 260, 1020, MC, 1, False), (6596, 324, 1028, MC, 1, False),       # K below 1024, N above 320,
        (6596, 260, 1028, MC, 2, False), (6596, 260, 1028, CC, 1, False),       # a K split, a k-contiguous A
        (2820, 2900, 36, CC, 1, False), (2820, 2692, 36, CC, 1, False),         # 529 / 506 tiles of 128 x 128
        (32772, 132, 20, CC, 1, False),                                         # 128 x 128 refused for waste
        (1284, 644, 612, CC, 1, True), (1284, 644, 604, CC, 1, True),           # pre-split: flop above / below 1e9,
        (260, 388, 9700, CC, 5, True), (252, 388, 9700, CC, 5, True),           # M 260 / 252,
        (260, 132, 14800, CC, 5, True), (260, 124, 15600, CC, 5, True),         # N 132 / 124,
        (4100, 164, 772, CC, 1, True), (3972, 164, 772, CC, 1, True),           # 130 / 126 tiles of 64 x 160,
        (11268, 164, 292, MC, 1, True), (11524, 164, 292, CC, 1, True),         # 178 / 182 row tiles of 128
        (452, 580, 100, CC, 8, False),                                          # the requested split sizes the tile
    ))
    return r


def grouped_features(g):
    f = set()
    for c in g.members:
        for mode in g.modes:
            w = c.want[mode]
            fam = family(w)
            if g.promoted:
                fam = "64x64s" if mode == 2 else "64x64"
            uniform = all(o.layout == c.layout and o.want[mode][:5] == w[:5] for o in g.members)
            if uniform and len(g.members) > 1 and not g.promoted:
                f.add(("grouped", fam, c.layout))
            elif fam == "elem":
                f.add("single launch inside a call")
    by_cfg = {}
    for c in g.members:
        by_cfg.setdefault((c.layout, c.want[0][:5]), []).append(c)
    if any(len(v) > 8 for v in by_cfg.values()):
        f.add("cut at kGroupMax")
    if len([k for k, v in by_cfg.items() if len(v) > 1]) > 1:
        f.add("mix of configurations")
    if g.rider:
        f.add("column-sum rider")
    if g.promoted:
        f.add("promoted")
    # (a promoted group's tile counts are not those of the members' own plans)
    if not g.promoted and any(c.split_k > 1 and (-(-c.M // c.want[0][0]) * -(-c.N // c.want[0][1]) * c.want[0][5]) % 8
                              for c in g.members[:-1]):
        f.add("padding workgroups behind a split problem")
    return f


def grouped_required():
    r = {("grouped", "32x32", l) for l in LAYOUTS}
    r.update(("grouped", fam, l) for fam in ("64x64", "64x64s") for l in LAYOUTS)
    r.update({"cut at kGroupMax", "mix of configurations", "column-sum rider", "promoted", "padding workgroups behind a split problem",
              "single launch inside a call"})
    return r


# ---- the table itself ------------------------------------------------------------------------------------------------
def every_case():
    return CASES + [c for g in GROUPED for c in g.members]


def test_names_are_unique_and_fields_valid():
    names = [c.name for c in every_case()] + [g.name for g in GROUPED]
    assert len(names) == len(set(names))
    for c in every_case():
        assert c.staging in STAGINGS and set(c.epi) <= set(EPILOGUES), c.name
        assert len(c.want) == 3 and all(len(w) == 6 for w in c.want), c.name
        assert c.split_k == 1 or "relu" not in c.epi, c.name
        assert "colsum" not in c.epi or c.akm, c.name
        # the exact-integer run: every value stays an fp32 integer
        assert value_bound(c) < 2 ** 24, c.name
        assert 4 * max(c.M, c.N) * (c.K + 12) < 32 << 20, "%s: an operand above 32 MB" % c.name


@pytest.mark.parametrize("c", every_case(), ids=lambda c: c.name)
def test_case_plans_are_the_launchers(ops, c):
    p = Problem(torch, ops, c)
    for mode in (0, 1, 2):
        ops.set_gemm_split(mode)
        assert p.plan() == c.want[mode], (c.name, mode, p.plan(), c.why)
        assert ops.gemm_plan(p.args)["waves"] == waves(c.want[mode]), (c.name, mode)
    assert c.modes()[0] == 0


def test_table_covers_every_configuration():
    have = set().union(*(features(c) for c in CASES))
    missing = required() - have
    assert not missing, sorted(map(str, missing))
    have = set().union(*(grouped_features(g) for g in GROUPED))
    missing = grouped_required() - have
    assert not missing, sorted(map(str, missing))


def test_every_row_is_needed():
    """Deleting any row loses something the coverage test asks for."""
    req = required()
    for i, c in enumerate(CASES):
        rest = set().union(*(features(o) for j, o in enumerate(CASES) if j != i))
        assert req - rest, "%s adds nothing the coverage test asks for" % c.name
    req = grouped_required()
    for i, g in enumerate(GROUPED):
        rest = set().union(*(grouped_features(o) for j, o in enumerate(GROUPED) if j != i))
        assert req - rest, "%s adds nothing the coverage test asks for" % g.name


def test_tile_grids_reach_both_orders():
    for fam in ("elem", "32x32", "64x64"):
        grids = []
        for c in CASES:
            w = c.want[0]
            if family(w) == fam:
                grids.append((-(-c.M // w[0]), -(-c.N // w[1])))
        assert any(tm <= tn and tm * tn > 1 for tm, tn in grids) and any(tm > tn for tm, tn in grids), fam
        assert any((tm * tn) % 8 for tm, tn in grids), fam


# ---- rejected arguments ------------------------------------------------------------------------------------------------
def plain_args(ops, L, keep, M=64, N=64, K=64, a_rs=64, a_ks=1, b_rs=64, b_ks=1, gate=False, headsplit=False, colsum=False,
               m_bound=False, drop=False, **kw):
    t = lambda *s: keep.append(torch.empty(*s)) or keep[-1]
    if gate:
        kw["gate"] = t(64, 64)
    if colsum:
        kw["colsum_a"] = t(64)
    if drop:
        kw["drop"] = (0.5, 1, 2)
    a = ops.gemm_args(t(64 * 128), t(64 * 128), t(64 * 64), M, N, K, a_rs, a_ks, b_rs, b_ks, 64, **kw)
    if headsplit:
        a.hs_dh, a.hs_dhp, a.hs_H, a.hs_S, a.hs_s0 = 16, 16, 2, 64, 0
    if m_bound:
        a.m_bound = keep.append(torch.zeros(1, dtype=torch.int32)) or keep[-1].data_ptr()
    return a


def test_rejected_arguments(ops):
    import ick_amd.lib as L
    lib = L.load()
    for mode in (0, 1, 2):
        ops.set_gemm_split(mode)
        for note, kw in REJECTED + ACCEPTED:
            keep = []
            info = L.GemmPlanInfo()
            rc = lib.ick_gemm_plan(C.byref(plain_args(ops, L, keep, **kw)), C.byref(info))
            want = -1 if (note, kw) in REJECTED else 0          # ICK_EINVAL / ICK_OK
            assert rc == want, (note, mode, rc)
        assert lib.ick_gemm_plan(None, C.byref(L.GemmPlanInfo())) == -1
