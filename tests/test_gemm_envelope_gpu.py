"""The GEMM across every kernel configuration its planner can choose (tests/gemm_cases.py; csrc/gemm.hip, csrc/gemm_ps.hip).
Every case asserts its plan first (ick_gemm_plan: tests/test_gemm_plan_cpu.py holds the table to the planner without a
GPU) and runs twice, in every product mode that gives it another plan:

exact integers   operands, bias and old C values are integers in -3 .. 3, alpha 1 or 2, dropout keep scale and gate scale
                 2: every product and partial sum is an fp32 integer below 2^24 on the exact MFMA and in the three-way bf16
                 split alike, and no order of atomics can change a sum.  The output must equal the reference BIT FOR BIT
                 (the reference is a float64 product: exact at these magnitudes).
rounding         uniform operands as in tests/test_ops_gpu.py against the float64 product.  Mode 0: that file's
                 2e-6 sqrt(K) of max(1, |ref|max), with atomic K slices 1e-5 sqrt(K) (tests/test_gemm_split_gpu.py, which
                 also bounds the fused column sums' float atomics); split and pre-split plans: that file's criterion, max
                 error at most 1.5 x and rms error at most 1.05 x the exact plan's on the same case.

Both runs poison the surroundings: C lies inside a buffer of sentinels (guard rows, a leading dimension above N, a guard
row between row groups, head-split pad columns) that must come back untouched, overwritten outputs start as NaN, the
padding of "padded" operands is NaN, "misaligned" operands start one float into their allocation."""
import ctypes as C
import math

import pytest
import torch

import ick_amd  # noqa: F401
import ick_amd.lib as L
from gemm_cases import CASES, GROUPED, GUARD, Problem

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ops():
    from ick_amd import ops as o
    before = o.gemm_split_mode()
    yield o
    o.set_gemm_split(before)


def seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


class Run:
    """A Problem on the device with its reference; reset() restores the output buffers between launches."""

    def __init__(self, ops, c, fill):
        self.c, self.fill = c, fill
        self.p = p = Problem(torch, ops, c, fill, "cuda", seed_of(c.name))
        self.ref, self.cs_ref = p.reference()
        if fill == "int":
            assert self.ref.abs().max().item() < 2 ** 24
        self.cs_init = p.csbuf.cpu() if p.cs_old is not None else None
        self.outside = torch.ones(p.out.size, dtype=torch.bool)
        self.outside[p.out.index.reshape(-1)] = False

    def reset(self):
        self.p.cbuf.copy_(self.p.cinit)
        if self.cs_init is not None:
            self.p.csbuf.copy_(self.cs_init)

    def check_exact(self, what):
        p = self.p
        got = p.cbuf.cpu()
        want = p.cinit.clone()
        want[p.out.index.reshape(-1)] = self.ref.reshape(-1).float()
        if not torch.equal(got, want):
            bad = ~((got == want) | (torch.isnan(got) & torch.isnan(want)))
            inside = bad[p.out.index]
            rows, cols = inside.any(1).nonzero().view(-1), inside.any(0).nonzero().view(-1)
            raise AssertionError("%s: %d wrong outputs (rows %s.., columns %s..), %d floats changed outside C" % (
                what, int(inside.sum()), rows[:4].tolist(), cols[:4].tolist(), int((bad & self.outside).sum())))
        if self.cs_ref is not None:
            want = self.cs_init.clone()
            want[3:3 + self.c.M] = self.cs_ref.float()
            assert torch.equal(p.csbuf.cpu(), want), "%s: column sums" % what

    def errors(self, what):
        """(max, rms) error of C against float64; everything outside C must be untouched, nothing non-finite inside."""
        p = self.p
        got = p.cbuf.cpu()
        assert torch.equal(got[self.outside], p.cinit[self.outside]), "%s: memory outside C changed" % what
        inside = got[p.out.index]
        assert torch.isfinite(inside).all(), "%s: non-finite outputs" % what
        e = inside.double() - self.ref
        return e.abs().max().item(), e.pow(2).mean().sqrt().item()

    def check_colsum(self, what):
        if self.cs_ref is None:
            return
        got = self.p.csbuf.cpu()
        assert (got[:3] == GUARD).all() and (got[3 + self.c.M:] == GUARD).all(), "%s: memory around the column sums" % what
        err = (got[3:3 + self.c.M].double() - self.cs_ref).abs().max().item()
        lim = 1e-5 * math.sqrt(self.c.K) * max(1.0, self.cs_ref.abs().max().item())
        print("%s: column sums max|err| %.3e (limit %.3e)" % (what, err, lim))
        assert err <= lim, "%s: column sums max|err| %.3e > %.3e" % (what, err, lim)


def check_rounding(run, what, split, launched, base):
    """The rounding run's bar for one launch; returns (max, rms).  base: the exact plan's errors on the same data."""
    emax, erms = run.errors(what)
    ref_max = max(1.0, run.ref.abs().max().item())
    if not split:
        tol = (1e-5 if launched > 1 else 2e-6) * math.sqrt(run.c.K)
        print("%s: max|err| %.3e rms %.3e (limit %.3e)" % (what, emax, erms, tol * ref_max))
        assert emax <= tol * ref_max, "%s max|err| %.3e > %.3e" % (what, emax, tol * ref_max)
    else:
        print("%s: max|err| %.3e rms %.3e (exact plan: %.3e, %.3e)" % (what, emax, erms, base[0], base[1]))
        assert emax <= 1.5 * base[0], "%s max|err| %.3e > 1.5 x %.3e of the exact plan" % (what, emax, base[0])
        assert erms <= 1.05 * base[1], "%s rms error %.3e > 1.05 x %.3e of the exact plan" % (what, erms, base[1])
    run.check_colsum(what)
    return emax, erms


def launch(ops, p):
    L.check(L.load().ick_gemm(C.byref(p.args), ops._stream()), "ick_gemm")
    torch.cuda.synchronize()


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_exact_integers(ops, c):
    run = Run(ops, c, "int")
    for mode in c.modes():
        ops.set_gemm_split(mode)
        assert run.p.plan() == c.want[mode], (mode, run.p.plan())
        run.reset()
        launch(ops, run.p)
        run.check_exact("%s mode %d" % (c.name, mode))


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.name)
def test_rounding(ops, c):
    run = Run(ops, c, "float")
    base = None
    for mode in c.modes():
        ops.set_gemm_split(mode)
        want = c.want[mode]
        assert run.p.plan() == want, (mode, run.p.plan())
        assert (mode == 0) == (want[3] == 0)
        run.reset()
        launch(ops, run.p)
        e = check_rounding(run, "%s mode %d" % (c.name, mode), want[3] == 1, want[5], base)
        if mode == 0:
            base = e


# ------------------------------------------------------------------------------------------------------- grouped launches
class Rider:
    """A plain column sum (ICK_GEMM_COLSUM_ONLY) riding in a grouped launch: out[n] += sum_m part[m, n]."""

    def __init__(self, ops, rows, cols, split_k, fill, seed):
        g = torch.Generator().manual_seed(seed)
        if fill == "int":
            self.part, self.old = (torch.randint(-3, 4, s, generator=g).double() for s in ((rows, cols), (cols,)))
        else:
            self.part, self.old = ((torch.rand(*s, generator=g) * 2 - 1).float().double() for s in ((rows, cols), (cols,)))
        self.rows = rows
        self.dpart = self.part.float().cuda()
        self.init = torch.full((cols + 6,), GUARD)
        self.init[3:3 + cols] = self.old.float()
        self.buf = self.init.cuda()
        self.args = ops.colsum_problem(self.dpart, self.buf[3:3 + cols], split_k=split_k)
        self.ref = self.old + self.part.sum(0)

    def check(self, exact, what):
        got, cols = self.buf.cpu(), self.ref.numel()
        want = self.init.clone()
        want[3:3 + cols] = self.ref.float()
        if exact:
            assert torch.equal(got, want), "%s: rider" % what
        else:
            assert torch.equal(got[:3], want[:3]) and torch.equal(got[3 + cols:], want[3 + cols:]), "%s: rider guards" % what
            err = (got[3:3 + cols].double() - self.ref).abs().max().item()
            assert err <= 1e-5 * math.sqrt(self.rows) * max(1.0, self.ref.abs().max().item()), "%s: rider %.3e" % (what, err)
        self.buf.copy_(self.init)


def grouped(ops, g, fill):
    runs = [Run(ops, c, fill) for c in g.members]
    rider = Rider(ops, *g.rider, fill, seed_of(g.name)) if g.rider else None
    base = {}
    for mode in g.modes:
        ops.set_gemm_split(mode)
        for r in runs:
            assert r.p.plan() == r.c.want[mode], (r.c.name, mode, r.p.plan())      # the plan each member has alone
            r.reset()
        ops.gemm_grouped([r.p.args for r in runs] + ([rider.args] if rider else []))
        torch.cuda.synchronize()
        for r in runs:
            what = "%s / %s mode %d" % (g.name, r.c.name, mode)
            if fill == "int":
                r.check_exact(what)
            else:
                split = r.c.want[mode][3] == 1 or (g.promoted and mode == 2)
                e = check_rounding(r, what, split, r.c.want[mode][5], base.get(r.c.name))
                if mode == 0:
                    base[r.c.name] = e
        if rider:
            rider.check(fill == "int", "%s mode %d" % (g.name, mode))


@pytest.mark.parametrize("g", GROUPED, ids=lambda g: g.name)
def test_grouped_exact_integers(ops, g):
    grouped(ops, g, "int")


@pytest.mark.parametrize("g", GROUPED, ids=lambda g: g.name)
def test_grouped_rounding(ops, g):
    grouped(ops, g, "float")
