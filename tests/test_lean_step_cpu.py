"""The lean step's entry points at the boundary, without a GPU: the header declares them, the binding
carries them with as many arguments as the header's prototypes, the library exports them, the structs the header shares
with the binding keep their sizes, and profiling.py gives each a class of its own choosing (no fall-through name)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NEW = ["ick_packed_ce_weighted_mean", "ick_packed_ce_packed_mean", "ick_packed_ce_smooth_mean",
       "ick_pointer_scores_bwd_fused", "ick_pointer_scores_bwd_fused_packed", "ick_adam_step", "ick_adam_step_derive"]
# each new entry takes the arguments of the entry it replaces plus these; the two Adam entries replaced every older one (none
# is left to compare with): their own argument counts
EXTRA = {"ick_packed_ce_weighted_mean": ("ick_packed_ce_weighted", 1), "ick_packed_ce_packed_mean": ("ick_packed_ce_packed", 1),
         "ick_packed_ce_smooth_mean": ("ick_packed_ce_smooth", 1), "ick_pointer_scores_bwd_fused": ("ick_pointer_scores_bwd", 0),
         "ick_pointer_scores_bwd_fused_packed": ("ick_pointer_scores_bwd_packed", 0)}
ADAM_ARGS = {"ick_adam_step": 26, "ick_adam_step_derive": 28}


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def prototypes():
    src = open(os.path.join(ROOT, "include", "ick_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return {m.group(1): [a for a in m.group(2).split(",") if a.strip() not in ("", "void")]
            for m in re.finditer(r"^int\s+(ick_[a-z0-9_]+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S)}


def test_header_binding_and_library_agree(built_lib):
    import ick_amd.lib as L
    protos = prototypes()
    lib = ctypes.CDLL(built_lib)
    for name in NEW:
        assert name in protos, "include/ick_amd.h does not declare %s" % name
        assert name in L.SIGNATURES, "lib.py does not bind %s" % name
        assert len(L.SIGNATURES[name]) == len(protos[name]), (name, len(L.SIGNATURES[name]), len(protos[name]))
        assert hasattr(lib, name), "libick_amd.so does not export %s" % name
        if name in ADAM_ARGS:
            assert len(L.SIGNATURES[name]) == ADAM_ARGS[name], name
            continue
        old, extra = EXTRA[name]
        assert len(L.SIGNATURES[name]) == len(L.SIGNATURES[old]) + extra, name
        assert L.SIGNATURES[name][:len(L.SIGNATURES[old]) - 1] == L.SIGNATURES[old][:-1], name
    # the flat and the derive form differ in what they run over only: n | items, blocks, n_blocks
    flat, derive = L.SIGNATURES["ick_adam_step"], L.SIGNATURES["ick_adam_step_derive"]
    assert flat[:5] == derive[:5] and flat[5:6] == [L.i64] and derive[5:8] == [L.vp, L.vp, L.i32] and flat[6:] == derive[8:]
    assert sorted(L.SIGNATURES) == sorted(protos)


def test_struct_sizes_unchanged(built_lib):
    # no struct gained a field: the sizes the parent commit's header gives (LP64)
    import ick_amd.lib as L
    assert ctypes.sizeof(L.RowChainArgs) == 272 and ctypes.sizeof(L.RowChainBwdArgs) == 296
    assert ctypes.sizeof(L.AdamItem) == 88 and ctypes.sizeof(L.AdamBlock) == 32 and ctypes.sizeof(L.LrSchedule) == 16


def test_profiling_classifies_the_new_entries():
    import ick_amd.profiling as prof
    args = [None] * 32
    for i in range(32):
        args[i] = 1
    for name in NEW:
        label = prof.classify(name, list(args))[0]
        assert label != name[4:].replace("_", " "), "profiling.classify has no class for %s" % name
    # the same class as the entry each one replaces, so by_kernel keeps one row per kind of work
    a = list(args)
    assert prof.classify("ick_packed_ce_packed_mean", a)[0] == prof.classify("ick_packed_ce_packed", a)[0]
    assert prof.classify("ick_packed_ce_smooth_mean", a)[0] == prof.classify("ick_packed_ce_smooth", a)[0]
    # the Adam entries: one class per set of options, (e, decay) by their pointers, in the flat and in the derive form
    labels = {(0, 0): "clamp + Adam", (0, 1): "clamp + Adam + weight decay", (1, 0): "clamp + Adam + EMA",
              (1, 1): "clamp + Adam + weight decay + EMA"}
    for (e, decay), label in labels.items():
        a = list(args)
        a[4], a[19] = e or None, decay or None
        assert prof.classify("ick_adam_step", a)[0] == label
        a = list(args)
        a[4], a[21] = e or None, decay or None
        assert prof.classify("ick_adam_step_derive", a)[0] == label + " + re-laid-out weight copies"
