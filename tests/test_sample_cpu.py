"""CPU checks of the sampled-decode boundary: ABI struct layout, exported symbols, the size check, and the numpy
Philox restatement the GPU tests use against its published known-answer vectors."""
import ctypes
import os
import subprocess
import tempfile

import numpy as np
import pytest

from sample_ref import gumbel, kept_set, philox4x32_10

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def built_lib():
    import ick_amd.build as build
    return build.build()


def test_sample_state_layout_matches_header(built_lib):
    import ick_amd.lib as L
    src = '#include <stdio.h>\n#include "ick_amd.h"\nint main(){printf("%zu", sizeof(ick_sample_state));}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "sz.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "sz")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        size = int(subprocess.check_output([exe]))
    assert ctypes.sizeof(L.SampleState) == size == 32


def test_library_exports_sample_symbols(built_lib):
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "ick_decode_select_sample") and hasattr(lib, "ick_decode_sample_supported")


def test_sample_supported_sizes(built_lib):
    import ick_amd.ops as ops
    assert ops.decode_sample_supported(50071, 1) and ops.decode_sample_supported(10020, 5)
    assert ops.decode_sample_supported(65536, 4096)
    assert not ops.decode_sample_supported(65537, 1) and not ops.decode_sample_supported(100000, 1)
    assert not ops.decode_sample_supported(10020, 0)


def test_select_sample_rejects_a_null_state(built_lib):
    import ick_amd.lib as L
    c = L.DecodeCtx()
    assert L.load().ick_decode_select_sample(ctypes.byref(c), None, 0, None) != 0


def test_philox_known_answers():
    got = philox4x32_10((0, 0, 0, 0), (0, 0))[0].tolist()
    assert got == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]
    m = 0xFFFFFFFF
    got = philox4x32_10((m, m, m, m), (m, m))[0].tolist()
    assert got == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_gumbel_is_finite_and_per_column():
    g = gumbel(123, 2, 1, 5, 4099)
    assert g.dtype == np.float32 and g.shape == (4099,) and np.isfinite(g).all()
    assert np.array_equal(gumbel(123, 2, 1, 5, 8)[:8], g[:8])       # a column's noise does not depend on the row width
    assert not np.array_equal(gumbel(124, 2, 1, 5, 8), g[:8])


def test_kept_set_rules():
    s = np.array([3.0, 1.0, 3.0, 2.0, 0.5], dtype=np.float32)
    keep, _ = kept_set(s, 1.0, 1, 1.0)
    assert keep.tolist() == [True, False, True, False, False]      # ties at the top-k boundary are all kept
    keep, _ = kept_set(s, 1.0, 3, 1.0)
    assert keep.tolist() == [True, False, True, True, False]
    keep, _ = kept_set(s, 1.0, 0, 0.3)                              # the two tied leaders: nothing strictly above them
    assert keep.tolist() == [True, False, True, False, False]
    keep, _ = kept_set(s, 1.0, 0, 1.0)
    assert keep.all()
