"""Without a GPU: the training envelope's case table (tests/train_cases.py) against the launch plan the library reports
(ick_attention_plan, the function ick_attention / ick_attention_bwd launch by), its coverage of every kernel
instantiation, and the documented size limits of the attention entry points and the row chains."""
import os
import subprocess
import sys

import pytest

from train_cases import (ATTN, ATTN_ACCEPTED, ATTN_REJECTED, CHAIN, CHAIN_BWD, LN, MFMA_INSTANTIATIONS)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ops():
    import ick_amd.build as build
    build.build()
    import ick_amd.ops as ops
    return ops


def expected(plan):
    """ick_attention_plan's fields for a table entry ("mfma", NQT, MAXT) / ("general", DHP, chunks)."""
    if plan[0] == "mfma":
        return dict(mfma=1, nqt=plan[1], maxt=plan[2], dhp=0, chunks=1, overwrites=1)
    return dict(mfma=0, nqt=0, maxt=0, dhp=plan[1], chunks=plan[2])


def test_names_are_unique():
    for table in (ATTN, CHAIN, CHAIN_BWD, LN):
        names = [c.name for c in table]
        assert len(names) == len(set(names))


@pytest.mark.parametrize("c", ATTN, ids=lambda c: c.name)
def test_attention_case_plans_are_the_launchers(ops, c):
    for direction, want in (("fwd", c.fwd), ("bwd", c.bwd)):
        got = ops.attention_plan(direction, c.T, c.S, c.dh)
        assert got is not None, (c.name, direction)
        assert {k: got[k] for k in expected(want)} == expected(want), (c.name, direction, got)
        assert got["chunks"] == -(-c.T // got["tq"]), (c.name, direction, got)
        if direction == "fwd":
            assert got["overwrites"] == 1
        else:
            assert got["overwrites"] == (got["chunks"] == 1)
            assert ops.L.load_raw().ick_attention_bwd_overwrites(c.T, c.S, c.dh) == got["overwrites"]
    assert c.pos0 >= 0
    if c.dh <= 32:
        # the training layout is what routes these to the matrix-core kernels: without it the forward takes the
        # general kernel and the backward is rejected
        assert ops.attention_plan("fwd", c.T, c.S, c.dh, head_major=False)["mfma"] == 0
        assert ops.attention_plan("bwd", c.T, c.S, c.dh, head_major=False) is None


def test_attention_table_covers_every_instantiation(ops):
    seen = {"fwd": set(), "bwd": set()}
    general = set()
    for c in ATTN:
        for direction, plan in (("fwd", c.fwd), ("bwd", c.bwd)):
            if plan[0] == "mfma":
                seen[direction].add(plan[1:])
            else:
                general.add((direction, plan[1], plan[2] > 1 if direction == "bwd" else False))
    for direction in ("fwd", "bwd"):
        assert MFMA_INSTANTIATIONS - seen[direction] == set(), direction
    # both DHP instantiations of both general kernels; the backward's single-chunk (overwrite) and atomic forms of each
    for dhp in (32, 64):
        assert ("fwd", dhp, False) in general
        assert ("bwd", dhp, False) in general and ("bwd", dhp, True) in general
    # both dK / dV store forms of the matrix-core backward
    st2 = {c.st2 for c in ATTN if c.bwd[0] == "mfma"}
    assert st2 == {True, False}
    assert any(c.bwd[0] == "mfma" and not c.st2 and (c.H * c.dh) % 2 == 0 for c in ATTN), \
        "a case whose scalar stores come from dh alone"
    # the edges the table exists for
    assert {1, 2, 16, 17, 33, 48, 49, 64, 257, 300} <= {c.T for c in ATTN}
    assert {1, 16, 17, 64, 65, 256, 257, 320, 321, 416, 512} <= {c.S for c in ATTN}
    assert {8, 16, 25, 30, 32, 33, 48, 64} <= {c.dh for c in ATTN}
    assert any(c.causal and c.pos0 == 0 and c.T > 1 for c in ATTN)
    assert any(c.causal and c.pos0 > 0 for c in ATTN if c.bwd[0] == "mfma")
    assert any(c.causal and c.pos0 > 0 for c in ATTN if c.bwd[0] == "general")
    assert any(c.drop > 0 for c in ATTN if c.bwd[0] == "mfma") and any(c.drop > 0 for c in ATTN if c.bwd[0] == "general")
    # general backward chunks of more queries than the workgroup has threads
    assert any(c.bwd[0] == "general" and ops.attention_plan("bwd", c.T, c.S, c.dh)["tq"] > 256 for c in ATTN)


def test_largest_matrix_core_shapes(ops):
    """For each NQT the table holds the largest S the matrix-core path takes and the first it rejects (both
    directions share attn_mfma_shape_ok)."""
    for T in (16, 32, 48, 64):
        for direction in ("fwd", "bwd"):
            ok = [S for S in range(1, 600) if ops.attention_plan(direction, T, S, 30)["mfma"]]
            assert ok == list(range(1, ok[-1] + 1))
            names = {(c.T, c.S) for c in ATTN}
            assert (T, ok[-1]) in names and (T, ok[-1] + 1) in names, (T, ok[-1])
    assert max(S for S in range(1, 600) if ops.attention_plan("bwd", 64, S, 30)["mfma"]) == 416


def test_attention_limits(ops):
    for direction, T, S, dh in ATTN_REJECTED:
        assert ops.attention_plan(direction, T, S, dh) is None, (direction, T, S, dh)
    for direction, T, S, dh in ATTN_ACCEPTED:
        assert ops.attention_plan(direction, T, S, dh) is not None, (direction, T, S, dh)
    assert ops.attention_plan("fwd", 0, 4, 30) is None and ops.attention_plan("bwd", 4, 0, 30) is None


def test_no_mfma_switch_forces_the_general_kernels(ops):
    """ICK_ATTN_NO_MFMA: the plan follows the switch exactly as the launchers do (read once per process)."""
    code = ("import sys; sys.path.insert(0, %r); import ick_amd.ops as ops; from train_cases import ATTN\n"
            "for c in ATTN:\n"
            "    for d in ('fwd', 'bwd'):\n"
            "        p = ops.attention_plan(d, c.T, c.S, c.dh)\n"
            "        assert p['mfma'] == 0 and p['dhp'] == (32 if c.dh <= 32 else 64), (c.name, d, p)\n"
            "    assert ops.L.load_raw().ick_attention_bwd_overwrites(c.T, c.S, c.dh) == (p['chunks'] == 1)\n"
            "print('ok')\n" % ROOT)
    env = dict(os.environ, ICK_ATTN_NO_MFMA="1")
    r = subprocess.run([sys.executable, "-c", code], cwd=os.path.dirname(os.path.abspath(__file__)), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_row_chain_limits(ops):
    assert ops.rowchain_supported(512, 320, 1024)
    assert not ops.rowchain_supported(513, 320, 1024)
    assert not ops.rowchain_supported(512, 321, 1024)
    assert not ops.rowchain_supported(512, 320, 1025)
    assert not ops.rowchain_supported(0, 64, 0)
    assert ops.rowchain_bwd_supported(1920, 320, 512)
    assert not ops.rowchain_bwd_supported(1921, 320, 512)
    assert not ops.rowchain_bwd_supported(1920, 321, 512)
    assert not ops.rowchain_bwd_supported(1920, 320, 513)
    for c in CHAIN:
        assert ops.rowchain_supported(c.K1, c.d, c.N2), c.name
        assert not c.proj or c.K1 == c.d, c.name
    for c in CHAIN_BWD:
        assert ops.rowchain_bwd_supported(c.K0, c.d, c.N1), c.name
        assert c.M % max(1, c.grouped) == 0, c.name


def test_row_chain_tables_reach_the_edges():
    assert {16, 300, 512} <= {c.K1 for c in CHAIN if not c.proj}
    assert {64, 100, 256, 300, 320} <= {c.d for c in CHAIN}
    assert {0, 64, 65, 960, 1024} <= {c.N2 for c in CHAIN}
    assert {1, 7, 8, 9, 1280} <= {c.M for c in CHAIN}
    for flag in ("relu", "slim", "proj", "heads", "drop1", "drop2"):
        assert any(getattr(c, flag) for c in CHAIN), flag
    assert any(c.proj and c.heads for c in CHAIN)
    assert {0, 64, 900, 1800, 1920} <= {c.K0 for c in CHAIN_BWD}
    assert any(c.K0 == 1800 and c.grouped for c in CHAIN_BWD)
    assert {0, 100, 384, 512} <= {c.N1 for c in CHAIN_BWD}
    assert {64, 100, 300, 320} <= {c.d for c in CHAIN_BWD}
    assert {1, 7, 9, 160} <= {c.M for c in CHAIN_BWD}
    assert {True, False} == {c.dzin for c in CHAIN_BWD}
    assert any(c.drop > 0 and c.N1 > 0 for c in CHAIN_BWD) and any(c.drop == 0 for c in CHAIN_BWD)


def test_layernorm_table_covers_every_instantiation():
    assert {c.nj for c in LN} == {5, 8, 16}
    assert {1, 63, 300, 320, 321, 512, 513, 1024} <= {c.d for c in LN}
    assert {1, 7, 8, 9, 1280} <= {c.rows for c in LN}
    for nj in (5, 8, 16):
        assert {True, False} == {c.atomics for c in LN if c.nj == nj}, nj
    assert {True, False} == {c.res for c in LN} and {True, False} == {c.drop > 0 for c in LN}
