"""Host side of ick_conv1_wgrad (csrc/conv1_bwd.hip): the launch plan and the argument checks, which run no kernel."""
import ctypes

import pytest


@pytest.fixture(scope="module")
def lib():
    import ick_amd.build as build
    import ick_amd.lib as L
    build.build()
    return L.load()


def plan(lib, B, C, P, d):
    import ick_amd.lib as L
    p, floats = (L.i32 * 4)(), L.i64()
    rc = lib.ick_conv1_wgrad_plan(B, C, P, d, p, ctypes.byref(floats))
    return rc, tuple(p), floats.value


def test_plan_at_the_workload_shape(lib):
    rc, (groups, k_per_group, col_tiles, rows), floats = plan(lib, 64, 2048, 196, 300)
    assert rc == 0
    assert col_tiles == 32 and rows == 304              # 64 columns per workgroup, all 300 rows in one block
    assert groups * col_tiles == 512                    # two workgroups per CU
    assert k_per_group % 32 == 0 and (groups - 1) * k_per_group < 64 * 196 <= groups * k_per_group   # no empty group
    assert floats == groups * (300 * 2048 + 300)


@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (2, 100, 9, 300), (7, 33, 5, 17), (2, 2048, 196, 512), (1, 5, 3, 2000),
                                   (4096, 8, 196, 16)])
def test_plan_covers_the_reduction_without_an_empty_group(lib, shape):
    B, C, P, d = shape
    rc, (groups, k_per_group, col_tiles, rows), floats = plan(lib, *shape)
    assert rc == 0 and 1 <= groups <= 64
    assert (groups - 1) * k_per_group < B * P <= groups * k_per_group
    assert col_tiles == -(-C // 64) and rows in (64, 160, 304)
    assert floats == groups * (d * C + d)


def test_plan_refuses_bad_sizes(lib):
    for bad in [(0, 8, 8, 8), (8, 0, 8, 8), (8, 8, 0, 8), (8, 8, 8, 0), (-1, 8, 8, 8), (1 << 20, 8, 1 << 11, 8)]:
        assert plan(lib, *bad)[0] == -1, bad
    import ick_amd.lib as L
    assert lib.ick_conv1_wgrad_plan(1, 1, 1, 1, None, ctypes.byref(L.i64())) == -1
    assert lib.ick_conv1_wgrad_plan(1, 1, 1, 1, (L.i32 * 4)(), None) == -1


def test_entry_refuses_null_pointers_and_bad_sizes_without_a_launch(lib):
    """No GPU here: an ICK_EINVAL (-1) means the entry returned before it touched the runtime."""
    buf = (ctypes.c_float * 16)()
    p = ctypes.addressof(buf)
    ok = [p, p, p, p, 1, 1, 1, 1, p, 16, None]
    for i in (0, 1, 2, 3, 8):
        a = list(ok)
        a[i] = None
        assert lib.ick_conv1_wgrad(*a) == -1, i
    for i in (4, 5, 6, 7):
        for bad in (0, -2):
            a = list(ok)
            a[i] = bad
            assert lib.ick_conv1_wgrad(*a) == -1, (i, bad)
    a = list(ok)
    a[9] = 1                                            # the plan needs 2 floats of scratch
    assert lib.ick_conv1_wgrad(*a) == -1


@pytest.mark.parametrize("conflict", [dict(fine_tune_encoder=True), dict(scst=True), dict(fused=False)])
def test_train_conv1_flag_conflicts_raise(conflict):
    """train.main refuses the combinations before it touches a device or the dataset."""
    from ick_amd import train as tr
    assert tr.Config().train_conv1 is False
    with pytest.raises(ValueError, match="train_conv1"):
        tr.main(tr.Config(train_conv1=True, data_dir="/nonexistent", **conflict))
