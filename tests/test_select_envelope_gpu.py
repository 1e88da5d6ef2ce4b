"""The beam and sampled token selection kernels on inputs a test chose (csrc/decode_select.hip: dec_beam_partial_kernel +
dec_select_beam_kernel, plain / rules / diverse / forced; csrc/sample.hip: dec_sample_kernel<4|16, RULES>).  Every case
of tests/select_cases.py runs through its entry point on a hand-filled lib.DecodeCtx -- no decoder -- and the whole
outgoing state is held against the float64 reference of tests/select_ref.py after every step: tokens, parents, flags,
masks, lengths, met masks, histories, n_done and x0 exactly, cum and log_prob at 1e-4 (every decision is 1e-2 apart or
an intended tie; tests/test_select_cases_cpu.py checks that without a GPU).  NaN sits wherever the kernels must not
look, and every buffer ends in guard rows that must come back unchanged."""
import numpy as np
import pytest
import torch

import ick_amd.decoder as D
import ick_amd.lib as L
import ick_amd.ops as ops
import select_cases as SC

pytestmark = pytest.mark.gpu

GUARD_ROWS, GUARD_I, GUARD_F, POISON_I = 2, -77, 12345.0, -99
NAN = float("nan")


class Buf:
    """A device buffer of n rows followed by guard rows."""

    def __init__(self, n, tail, dtype, init):
        guard = GUARD_F if dtype.is_floating_point else GUARD_I
        self.full = torch.full((n + GUARD_ROWS,) + tuple(tail), guard, dtype=dtype, device="cuda")
        self.t = self.full[:n]
        self.guard = guard
        if isinstance(init, np.ndarray):
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)).to(dtype))
        else:
            self.t.fill_(init)

    def ptr(self):
        return self.full.data_ptr()

    def intact(self):
        return bool((self.full[self.t.shape[0]:] == self.guard).all())

    def np(self):
        return self.t.cpu().numpy()


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.int32),
                          np.ascontiguousarray(b, dtype=np.float32).view(np.int32))


class Harness:
    """lib.DecodeCtx over buffers of the harness's own: the fields the selection entry points read, and nothing else."""

    def __init__(self, case, rows_per_sample):
        R, V, P, Lm, d = case.R, case.V, case.K + case.F, case.max_len, case.d
        self.case, self.bufs = case, {}
        t = SC.tables(case)
        self.tables = t
        b = self.bufs
        b["word_emb"] = Buf(V, (d,), torch.float32, t["word_emb"])
        b["ee"] = Buf(case.B * case.K, (d,), torch.float32, t["ee"].reshape(-1, d))
        if case.F:
            b["fe"] = Buf(case.B * case.F, (d,), torch.float32, t["fe"].reshape(-1, d))
        b["pe"] = Buf(Lm, (d,), torch.float32, t["pe"])
        b["scores"] = Buf(R, (V + case.ld_pad,), torch.float32, NAN)
        b["ptr"] = Buf(R, (P,), torch.float32, NAN)
        b["x0"] = Buf(R, (d,), torch.float32, NAN)
        b["next_token"] = Buf(R, (), torch.int64, POISON_I)
        b["next_mask"] = Buf(R, (), torch.int64, POISON_I)
        b["n_done"] = Buf(1, (), torch.int32, 0)
        c = L.DecodeCtx()
        c.R, c.rows_per_sample, c.d, c.max_len, c.V, c.K, c.F = R, rows_per_sample, d, Lm, V, case.K, case.F
        c.end_token, c.pad_token, c.emb_scale, c.scores_ld = case.end, case.pad, t["emb_scale"], V + case.ld_pad
        for n in ("word_emb", "ee", "pe", "scores", "ptr", "x0", "next_token", "next_mask", "n_done"):
            setattr(c, n, b[n].ptr())
        c.fe = b["fe"].ptr() if case.F else None
        self.ctx = c

    def add(self, name, n, tail, dtype, init):
        self.bufs[name] = Buf(n, tail, dtype, init)
        return self.bufs[name]

    def write_rows(self, rows):
        """The step's raw rows; everything else is NaN: the columns past V of every row, and the whole score and
        pointer row of a row without scores."""
        s, p, V = self.bufs["scores"].t, self.bufs["ptr"].t, self.case.V
        s.fill_(NAN)
        p.fill_(NAN)
        for r, x in rows.items():
            x = torch.from_numpy(x).cuda()
            s[r, :V] = x[:V]
            p[r] = x[V:]

    def poison_outputs(self):
        self.bufs["x0"].t.fill_(NAN)
        self.bufs["next_token"].t.fill_(POISON_I)
        self.bufs["next_mask"].t.fill_(POISON_I)

    def check_next(self, info, written_rows, what):
        b = self.bufs
        assert np.array_equal(b["next_token"].np()[written_rows], info["next_token"][written_rows]), what
        assert np.array_equal(b["next_mask"].np()[written_rows], info["next_mask"][written_rows]), what
        assert (b["next_token"].np()[~written_rows] == POISON_I).all(), what

    def check_x0(self, info, written, what):
        x0 = self.bufs["x0"].np()
        assert same_bits(x0[written], info["x0"][written]), (what, x0[written], info["x0"][written])
        assert np.isnan(x0[~written]).all(), what

    def check_guards(self, what):
        for n, b in self.bufs.items():
            assert b.intact(), (what, n)


# ------------------------------------------------------------------------------------------------------------- beam
class BeamHarness(Harness):
    def __init__(self, case, st):
        super().__init__(case, case.beam)
        R, Lm = case.R, case.max_len
        nchunk = (case.Vx + 1023) // 1024
        self.add("cum", R, (), torch.float32, st["cum"].astype(np.float32))
        self.add("fin", R, (), torch.int32, st["fin"])
        self.add("rec", R * nchunk, (18,), torch.float32, NAN)
        self.seq = [self.add("seq%d" % q, R, (Lm,), torch.int64, st["seq"] if q == 0 else POISON_I) for q in range(2)]
        self.anc = [self.add("anc%d" % q, R, (Lm,), torch.int32, st["anc"] if q == 0 else POISON_I) for q in range(2)]
        self.cap = None
        if st["cap"] is not None:
            self.cap = [self.add("cap%d" % q, R, (Lm,), torch.int64, st["cap"] if q == 0 else POISON_I) for q in range(2)]
        self.bufs["n_done"].t.fill_(st["n_done"])
        bs = L.BeamState()
        bs.cum, bs.fin, bs.rec, bs.start_token = self.bufs["cum"].ptr(), self.bufs["fin"].ptr(), self.bufs["rec"].ptr(), case.start
        self.bs = bs
        self.rules = self.div = self.fc = None
        if case.rules is not None:
            ngram, min_len, alpha = case.rules
            self.rules_t = D.rules_tensor(Lm, alpha, ngram, min_len, "cuda")
            self.add("len", R, (), torch.int32, st["len"])
            self.rules = D._rules_struct(self.rules_t, self.bufs["len"].full)
        if case.form == "diverse":
            self.penalty = torch.tensor([case.lam], dtype=torch.float32, device="cuda")
            self.div = L.DecodeDiversity()
            self.div.groups, self.div.penalty = case.groups, self.penalty.data_ptr()
        if case.form == "forced":
            self.add("force", case.B, (8,), torch.int32, np.asarray(case.force, dtype=np.int32))
            self.add("met", R, (), torch.int32, st["met"])
            self.fc = L.DecodeConstraints()
            self.fc.force, self.fc.met = self.bufs["force"].ptr(), self.bufs["met"].ptr()

    def point(self, cur):
        nxt = cur ^ 1
        bs = self.bs
        bs.seq_in, bs.seq_out = self.seq[cur].ptr(), self.seq[nxt].ptr()
        bs.anc_in, bs.anc_out = self.anc[cur].ptr(), self.anc[nxt].ptr()
        if self.cap:
            bs.cap_in, bs.cap_out = self.cap[cur].ptr(), self.cap[nxt].ptr()
        for q in [self.seq[nxt], self.anc[nxt]] + ([self.cap[nxt]] if self.cap else []):
            q.t.fill_(POISON_I)
        return nxt

    def select(self, pos):
        ops.decode_select_beam(self.ctx, self.bs, pos, self.rules, self.div, self.fc)
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", SC.BEAM, ids=lambda c: c.name)
def test_beam_selection_matches_the_reference_step_by_step(case):
    trace = SC.beam_trace(case.name)
    h = BeamHarness(case, trace[0]["st"])
    k, R = case.beam, case.R
    lp_on = case.rules is not None and case.rules[2] != 0
    cur = 0
    for t in trace:
        pos, out, info = t["pos"], t["out"], t["info"]
        what = (case.name, pos)
        nxt = h.point(cur)
        h.write_rows(t["rows"])
        h.bufs["rec"].t.fill_(NAN)
        h.poison_outputs()
        h.select(pos)
        b = h.bufs
        cum, fin = b["cum"].np().astype(np.float64), b["fin"].np()
        print(what, "cum", cum, "want", out["cum"])
        dead = out["cum"] == SC.NEG
        assert np.array_equal(cum == SC.NEG, dead), what
        assert np.abs(cum[~dead] - out["cum"][~dead]).max(initial=0.0) < 1e-4, what
        assert np.array_equal(fin, out["fin"]), what
        if case.rules is not None:
            assert np.array_equal(b["len"].np(), out["len"]), what      # (untouched while the length penalty is off)
        if case.form == "forced":
            assert np.array_equal(b["met"].np(), out["met"]), what
        assert int(b["n_done"].np()[0]) == out["n_done"], (what, int(b["n_done"].np()[0]), out["n_done"])
        # the histories of every slot that holds a hypothesis (a dead slot's are not specified)
        keep = ~info["dead"]
        assert np.array_equal(h.seq[nxt].np()[keep], out["seq"][keep]), (what, h.seq[nxt].np(), out["seq"])
        assert np.array_equal(h.anc[nxt].np()[keep], out["anc"][keep]), (what, h.anc[nxt].np(), out["anc"])
        if h.cap:
            assert np.array_equal(h.cap[nxt].np()[keep], out["cap"][keep]), (what, h.cap[nxt].np(), out["cap"])
        h.check_next(info, np.ones(R, bool), what)
        h.check_x0(info, info["x0_written"], what)
        if pos == case.max_len - 1:
            assert not info["x0_written"].any()
        h.check_guards(what)
        cur = nxt


# --------------------------------------------------------------------------------------------------------- sampling
class SampleHarness(Harness):
    def __init__(self, case, st):
        super().__init__(case, case.rps)
        R, Lm = case.R, case.max_len
        self.add("output", R, (Lm,), torch.int64, st["output"])
        self.add("finished", R, (), torch.int32, st["finished"])
        self.add("log_prob", R, (Lm,), torch.float32, st["log_prob"].astype(np.float32))
        self.bufs["n_done"].t.fill_(st["n_done"])
        c = self.ctx
        c.output, c.finished = self.bufs["output"].ptr(), self.bufs["finished"].ptr()
        if st["cap_buf"] is not None:
            self.add("cap_buf", R, (Lm,), torch.int64, st["cap_buf"])
            c.cap_buf = self.bufs["cap_buf"].ptr()
        self.seed = torch.tensor([case.seed], dtype=torch.int64, device="cuda")
        self.tp = torch.tensor([case.T, case.top_p], dtype=torch.float32, device="cuda")
        self.tk = torch.tensor([case.top_k], dtype=torch.int32, device="cuda")
        s = L.SampleState()
        s.seed, s.temp_top_p, s.top_k = self.seed.data_ptr(), self.tp.data_ptr(), self.tk.data_ptr()
        s.log_prob = self.bufs["log_prob"].ptr()
        self.state = s
        self.rules = None
        if case.rules is not None:
            self.rules_t = D.rules_tensor(Lm, 0.0, case.rules[0], case.rules[1], "cuda")
            self.rules = D._rules_struct(self.rules_t)

    def select(self, pos):
        ops.decode_select_sample(self.ctx, self.state, pos, self.rules)
        torch.cuda.synchronize()


@pytest.mark.parametrize("case", SC.SAMPLE, ids=lambda c: c.name)
def test_sampled_selection_matches_the_reference_step_by_step(case):
    trace = SC.sample_trace(case.name)
    h = SampleHarness(case, trace[0]["st"])
    R = case.R
    for t in trace:
        pos, out, info = t["pos"], t["out"], t["info"]
        what = (case.name, pos)
        h.write_rows(t["rows"])
        h.poison_outputs()
        b = h.bufs
        live = np.array([r in t["rows"] for r in range(R)])
        if live.any():                          # what a live row's step overwrites
            rows = torch.from_numpy(np.nonzero(live)[0]).cuda()
            b["output"].t[rows, pos] = POISON_I
            b["log_prob"].t[rows, pos] = NAN
        h.select(pos)
        written = np.full(R, bool(info["written"]))
        print(what, "tokens", b["output"].np()[:, pos], "want", out["output"][:, pos], "log_prob", b["log_prob"].np()[:, pos])
        assert np.array_equal(b["output"].np(), out["output"]), (what, b["output"].np(), out["output"])
        assert np.array_equal(b["finished"].np(), out["finished"]), what
        assert int(b["n_done"].np()[0]) == out["n_done"], what
        assert np.abs(b["log_prob"].np().astype(np.float64) - out["log_prob"]).max() < 1e-4, what
        if "cap_buf" in b:
            assert np.array_equal(b["cap_buf"].np(), out["cap_buf"]), (what, b["cap_buf"].np(), out["cap_buf"])
        h.check_next(info, written, what)
        h.check_x0(info, written & (pos + 1 < case.max_len), what)
        h.check_guards(what)


# ------------------------------------------------------------------------------------------------------- rejections
def _ended_beam(B, beam, V, K, F, max_len, rules=None, form="plain", groups=1):
    """A harness whose hypotheses have all ended: an accepted call only moves the tables over."""
    case = SC.BeamCase("reject", form, B, beam, V, K, F, max_len, [(1, None)], rules=rules, groups=groups, lam=0.5,
                       force=[SC.NOF] * B, state0=[SC.hyp([SC.END], -1.0, fin=True)] * (B * beam))
    h = BeamHarness(case, SC.beam_state(case))
    h.point(0)
    return h


def refused(call):
    with pytest.raises(L.IckError, match="ICK_EINVAL"):
        call()
    torch.cuda.synchronize()


def test_beam_entry_points_refuse_what_they_do_not_support():
    """Host checks, before any launch; the matching just-inside call is accepted."""
    _ended_beam(1, 8, 50, 4, 0, 4).select(1)
    refused(lambda: _ended_beam(1, 9, 50, 4, 0, 4).select(1))                       # beam 9
    assert ops.decode_beam_supported(65536, 8) and not ops.decode_beam_supported(65537, 8)
    refused(lambda: _ended_beam(1, 8, 65521, 8, 8, 4).select(1))                    # beam 8 at Vx = 65 537
    _ended_beam(1, 4, 50, 4, 0, 4, form="diverse", groups=2).select(1)
    refused(lambda: _ended_beam(1, 4, 50, 4, 0, 4, form="diverse", groups=3).select(1))     # groups do not divide the beam
    _ended_beam(1, 2, 200, 4, 0, 128, rules=(1, 0, 0.0)).select(1)
    refused(lambda: _ended_beam(1, 2, 200, 4, 0, 129, rules=(1, 0, 0.0)).select(1))         # rules with max_len = 129
    h = _ended_beam(1, 2, 50, 4, 0, 4, rules=(1, 0, 0.0))
    h.select(1)
    h.rules.words += 4                                                              # rule words off a 16-byte boundary
    refused(lambda: h.select(1))
    h = _ended_beam(1, 2, 50, 4, 4, 4)
    h.select(1)
    h.bs.cap_out = None                                                             # cap_in without cap_out
    refused(lambda: h.select(1))
    h.check_guards("cap")


def _finished_sample(V, K, F):
    case = SC.SampleCase("reject", 1, 2, V, K, F, 4, [(1, None)], state0=[SC.srow([SC.END], fin=True)] * 2)
    return SampleHarness(case, SC.sample_state(case))


def test_sample_entry_points_refuse_what_they_do_not_support():
    _finished_sample(65520, 8, 8).select(1)
    assert ops.decode_sample_supported(65536, 2) and not ops.decode_sample_supported(65537, 2)
    refused(lambda: _finished_sample(65521, 8, 8).select(1))                        # Vx = 65 537
    h = _finished_sample(50, 4, 0)
    h.select(1)
    h.state.temp_top_p += 2                                                         # a knob pointer off a dword boundary
    refused(lambda: h.select(1))
    h.state.temp_top_p -= 2
    h.state.top_k += 1
    refused(lambda: h.select(1))
    h.check_guards("knobs")
