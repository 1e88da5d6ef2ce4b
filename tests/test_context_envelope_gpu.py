"""The context, embedding and pointer kernels across their envelope on the MI355X: the entity / fact encoders, the
caption embedder, the context indicators with the predicate gate, the pointer scores, and every backward kernel of
theirs in both the float-atomic and the deterministic form, each case of tests/context_cases.py against the float64
references of tests/context_ref.py.

Gathers are bit-exact.  Sums are held elementwise to |got - ref| <= (n + 4) 2^-24 A, A the reference's `*_abs`
evaluation of that element (the sum of |addends|) and n the largest addend count into any element of the tensor,
computed from the case's indices (context_ref.bound).  Backward outputs are pre-filled with seeded non-zero values (the
kernels add into buffers that already hold gradient; the prefill is one more addend) and sit between guard words that
must not change.
"""
import contextlib
import functools
import math
import zlib

import pytest
import torch

import context_ref as CR
from context_cases import (BIG_INDEX, GATE, GATE_BWD_REJECTED, GATHER, INDICATORS_REJECTED, NTYPES, POINTER,
                           POINTER_BWD_REJECTED, POINTER_D_REJECTED, V, GatherCase, gate_inputs, gather_inputs)

pytestmark = pytest.mark.gpu
PAD = 0
GUARD = 1024
SENTINEL = 12345.0


@pytest.fixture(scope="module")
def ops():
    import ick_amd.ops as ops
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return ops


@pytest.fixture(params=[False, True], ids=["atomics", "deterministic"])
def det(request, ops):
    with deterministic_mode(ops, request.param):
        yield request.param


@contextlib.contextmanager
def deterministic_mode(ops, on):
    before = ops.is_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(before)


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(zlib.crc32(str(seed).encode()))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def dev(x):
    return None if x is None else x.cuda()


def bits(x):
    return x.detach().contiguous().view(torch.int32)


class Out:
    """A device output pre-filled with `init` (CPU float32), between two runs of guard words."""

    def __init__(self, init):
        n = init.numel()
        self.init = init
        self.buf = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
        self.t = self.buf[GUARD:GUARD + n].view(init.shape)
        self.t.copy_(init)

    def guards_intact(self):
        n = self.init.numel()
        return bool((self.buf[:GUARD] == SENTINEL).all() and (self.buf[GUARD + n:] == SENTINEL).all())


def prefilled(*shape, seed):
    return Out(rnd(*shape, seed=seed, scale=0.5))


def held(out, grad, grad_abs, n, what):
    """out (Out or device tensor): prefill + grad within (n + 4) u A elementwise; n counts the prefill as an addend."""
    if isinstance(out, Out):
        assert out.guards_intact(), what + ": wrote outside its buffer"
        got, pre = out.t.cpu().double(), out.init.double()
    else:
        got, pre = out.cpu().double(), torch.zeros_like(grad)
    assert torch.isfinite(got).all(), what
    err = (got - (pre + grad)).abs()
    lim = CR.bound(n, pre.abs() + grad_abs)
    worst = (err / lim.clamp_min(1e-300)).max().item() if err.numel() else 0.0
    print("%s: n = %d, max |err| %.3e, max err / bound %.3f" % (what, n, err.max().item(), worst))
    assert (err <= lim).all(), "%s: max err / bound %.3f (n = %d)" % (what, worst, n)


def same_bits(a, b, what):
    assert torch.equal(bits(a), bits(b)), what


def max_count(keys):
    """Largest number of equal entries of a list of hashable destination keys."""
    seen = {}
    for k in keys:
        seen[k] = seen.get(k, 0) + 1
    return max(seen.values()) if seen else 0


# ============================================================================================ gathers: shared inputs
@functools.lru_cache(maxsize=None)
def gather_setup(c: GatherCase, big=False):
    """Inputs and float64 forward references of a gather case (computed once, never modified)."""
    batch, _ = gather_inputs(c, big)
    off = CR.TYPE_OFFSET[c.variant]
    s = dict(batch=batch, facts=batch.get("facts"), ent=batch["entities"],
             type_emb=rnd(NTYPES[c.variant], c.d - off, seed=c.name + "type"),
             word_emb=rnd(V, c.d, seed=c.name + "word"),
             pred_emb=rnd(c.num_pred, c.d, seed=c.name + "pred") if c.F else None,
             pe=rnd(c.pos0 + c.L, c.d, seed=c.name + "pe"))
    s["news_words"] = s["word_emb"] if c.variant == "news" else None
    s["ee_ref"] = CR.entity_encode(c.variant, s["ent"], s["type_emb"], c.d, s["facts"], s["news_words"])
    s["ee32"] = s["ee_ref"].float()
    s["fe32"] = CR.fact_encode(s["facts"], s["ee32"], s["pred_emb"]).float() if c.F else None
    return s


def run_entity_encode(ops, c, s):
    return ops.entity_encode(c.variant, dev(s["ent"]), dev(s["type_emb"]), c.d, facts=dev(s["facts"]),
                             word_emb=dev(s["news_words"]))


# ============================================================================================ gathers: forward
@pytest.mark.parametrize("c", GATHER, ids=lambda c: c.name)
def test_gather_forward(ops, c):
    s = gather_setup(c)
    caps, masks = s["batch"]["captions"], s["batch"]["caption_masks"]
    ee = run_entity_encode(ops, c, s)
    if c.variant == "news":     # float32 product of the encoding and a five-term average: the existing 1e-7
        err = (ee.cpu().double() - s["ee_ref"]).abs().max().item()
        assert err <= 1e-7 * max(1.0, s["ee_ref"].abs().max().item()), err
    else:
        same_bits(ee.cpu(), s["ee32"], "entity_encode")
    if c.F:
        fe = ops.fact_encode(dev(s["facts"]), dev(s["ee32"]), dev(s["pred_emb"]))
        same_bits(fe.cpu(), s["fe32"], "fact_encode")
    scale = math.sqrt(c.d)
    x_ref, emb_ref = CR.caption_embed(caps, masks, s["word_emb"], s["ee32"], s["fe32"], s["pe"], V, PAD, scale,
                                      pos0=c.pos0, round32=True)
    x, emb = ops.caption_embed(dev(caps), dev(masks), dev(s["word_emb"]), dev(s["ee32"]), dev(s["fe32"]), dev(s["pe"]), V,
                               PAD, scale, pos0=c.pos0, want_emb=True)
    same_bits(emb.cpu(), emb_ref.float(), "caption_embed emb_out")
    same_bits(x.cpu(), x_ref.float(), "caption_embed")
    x2 = ops.caption_embed(dev(caps), dev(masks), dev(s["word_emb"]), dev(s["ee32"]), dev(s["fe32"]), dev(s["pe"]), V, PAD,
                           scale, pos0=c.pos0)
    same_bits(x2.cpu(), x_ref.float(), "caption_embed without emb_out")


# ============================================================================================ gathers: backward
def caption_bwd_check(ops, c, s, det, drop=None, mask=None, combos=("all", "no_dword", "no_dfe")):
    caps, masks = s["batch"]["captions"], s["batch"]["caption_masks"]
    scale = math.sqrt(c.d)
    dx = rnd(c.B, c.L, c.d, seed=c.name + "dx")
    if "zero_dx" in s["batch"]:
        b, l0 = s["batch"]["zero_dx"]
        dx[b, l0:] = 0.0
    for combo in combos:
        with_fe = c.F > 0 and combo != "no_dfe"
        if combo == "no_dfe" and not c.F:
            continue
        fe = s["fe32"] if with_fe else None

        def fn(absval=False, word=None, ee=None, fe=None):
            return CR.caption_embed(caps, masks, word, ee, fe, s["pe"], V, PAD, scale, pos0=c.pos0, mask=mask,
                                    absval=absval)[0]
        leaves = dict(word=s["word_emb"], ee=s["ee32"])
        if with_fe:
            leaves["fe"] = fe
        g, ga = CR.grads(fn, leaves, dx), CR.grads(fn, leaves, dx, absval=True)
        kind, row = CR.caption_sources(caps, masks, V, c.K, c.F if with_fe else 0, PAD, with_fe)
        n = {k: 1 + max_count([(b if k != "word" else 0, int(row[b, l])) for b in range(c.B) for l in range(c.L)
                               if kind[b][l] == k]) for k in ("word", "ent", "fact")}
        runs = []
        for _ in range(2 if det else 1):
            dword = prefilled(V, c.d, seed=c.name + "dword") if combo != "no_dword" else None
            dee = prefilled(c.B, c.K, c.d, seed=c.name + "dee")
            dfe = prefilled(c.B, c.F, c.d, seed=c.name + "dfe") if with_fe else None
            ops.caption_embed_bwd(dev(dx), dev(caps), dev(masks), None if dword is None else dword.t, dee.t,
                                  None if dfe is None else dfe.t, V, PAD, scale, drop=drop)
            runs.append([o for o in (dword, dee, dfe) if o is not None])
        what = "caption_embed_bwd[%s] " % combo
        if dword is not None:
            held(dword, g["word"], ga["word"], n["word"], what + "dword")
        held(dee, g["ee"], ga["ee"], n["ent"], what + "dee")
        if dfe is not None:
            held(dfe, g["fe"], ga["fe"], n["fact"], what + "dfe")
        if det:
            for a, b2 in zip(*runs):
                same_bits(a.t, b2.t, what + "two deterministic runs")


def fact_bwd_check(ops, c, s, det):
    facts = s["facts"]
    up = rnd(c.B, c.F, c.d, seed=c.name + "dfe_up")

    def fn(absval=False, ee=None, pred=None):
        return CR.fact_encode(facts, ee, pred)
    leaves = dict(ee=s["ee32"], pred=s["pred_emb"])
    g, ga = CR.grads(fn, leaves, up), CR.grads(fn, leaves, up, absval=True)
    subj, pred = CR.clamp_facts(facts, c.K, c.num_pred)
    n_ee = 1 + max_count([(b, int(subj[b, j])) for b in range(c.B) for j in range(c.F)])
    n_pred = 1 + max_count([int(q) for q in pred.flatten()])
    runs = []
    for _ in range(2 if det else 1):
        dee = prefilled(c.B, c.K, c.d, seed=c.name + "dee2")
        dpred = prefilled(c.num_pred, c.d, seed=c.name + "dpred")
        ops.fact_encode_bwd(dev(up), dev(facts), dee.t, dpred.t)
        runs.append((dee, dpred))
    held(dee, g["ee"], ga["ee"], n_ee, "fact_encode_bwd dee")
    held(dpred, g["pred"], ga["pred"], n_pred, "fact_encode_bwd dpred")
    if det:
        for a, b2 in zip(*runs):
            same_bits(a.t, b2.t, "fact_encode_bwd: two deterministic runs")


def entity_bwd_check(ops, c, s, det):
    news = c.variant == "news"
    off = CR.TYPE_OFFSET[c.variant]
    up = rnd(c.B, c.K, c.d, seed=c.name + "dee_up")
    ee_dev = run_entity_encode(ops, c, s) if news else None    # the kernel recovers the encoding from ITS forward output

    def fn(absval=False, type_emb=None, word=None):
        return CR.entity_encode(c.variant, s["ent"], type_emb, c.d, s["facts"], word, absval=absval)
    leaves = dict(type_emb=s["type_emb"])
    if news:
        leaves["word"] = s["word_emb"]
    g, ga = CR.grads(fn, leaves, up), CR.grads(fn, leaves, up, absval=True)
    n_type = 1 + max_count([int(q) for q in CR.clamp_type(s["ent"], NTYPES[c.variant]).flatten()])
    n_word = 1 + max_count([int(q) for q in CR.clamp_names(s["ent"], V).flatten()]) if news else 0
    for combo in (("all", "no_dword") if news else ("all",)):
        runs = []
        for _ in range(2 if det else 1):
            dtype = prefilled(NTYPES[c.variant], c.d - off, seed=c.name + "dtype")
            dword = prefilled(V, c.d, seed=c.name + "dword2") if news and combo == "all" else None
            ops.entity_encode_bwd(c.variant, dev(up), dev(s["ent"]), ee_dev, dtype.t, word_emb=dev(s["news_words"]),
                                  dword=None if dword is None else dword.t)
            runs.append([o for o in (dtype, dword) if o is not None])
        held(dtype, g["type_emb"], ga["type_emb"], n_type, "entity_encode_bwd[%s] dtype_emb" % combo)
        if dword is not None:
            held(dword, g["word"], ga["word"], n_word, "entity_encode_bwd dword")
        if det:
            for a, b2 in zip(*runs):
                same_bits(a.t, b2.t, "entity_encode_bwd: two deterministic runs")


@pytest.mark.parametrize("c", GATHER, ids=lambda c: c.name)
def test_gather_backward(ops, det, c):
    s = gather_setup(c)
    caption_bwd_check(ops, c, s, det)
    if c.F:
        fact_bwd_check(ops, c, s, det)
    entity_bwd_check(ops, c, s, det)


def test_fact_index_beyond_int32(ops):
    """A fact subject of 2^32 + 1 and a predicate of 2^32 + 2 are out of range: the fact encoder and its backward (both
    forms) clamp them to the last rows, the fact count matches them to no entity."""
    c = BIG_INDEX
    s = gather_setup(c, True)
    assert (s["facts"] > 2 ** 32).sum().item() == 2
    same_bits(run_entity_encode(ops, c, s).cpu(), s["ee32"], "entity_encode (fact count)")
    fe = ops.fact_encode(dev(s["facts"]), dev(s["ee32"]), dev(s["pred_emb"]))
    same_bits(fe.cpu(), s["fe32"], "fact_encode")
    for mode in (False, True):
        with deterministic_mode(ops, mode):
            fact_bwd_check(ops, c, s, mode)


# ============================================================================================ dropout site
def test_caption_embed_dropout_site(ops, det):
    """The PositionEncoder dropout of the caption embedder: forward and backward index the same mask."""
    c = GatherCase("drop_know_d300", "knowledge", 2, 9, 5, 4, 300)
    s = gather_setup(c)
    caps, masks = s["batch"]["captions"], s["batch"]["caption_masks"]
    drop = (0.3, 977, 4)
    mask = ops.dropout_mask(c.B * c.L, c.d, *drop).cpu()
    keep = (mask > 0).float().mean().item()
    assert 0.6 < keep < 0.8 and abs(mask.max().item() - 1 / 0.7) < 1e-6
    scale = math.sqrt(c.d)
    x_ref, _ = CR.caption_embed(caps, masks, s["word_emb"], s["ee32"], s["fe32"], s["pe"], V, PAD, scale, mask=mask,
                                round32=True)
    x = ops.caption_embed(dev(caps), dev(masks), dev(s["word_emb"]), dev(s["ee32"]), dev(s["fe32"]), dev(s["pe"]), V, PAD,
                          scale, drop=drop)
    same_bits(x.cpu(), x_ref.float(), "caption_embed with dropout")
    caption_bwd_check(ops, c, s, det, drop=drop, mask=mask, combos=("all",))


# ============================================================================================ indicators and gate
@functools.lru_cache(maxsize=None)
def gate_setup(c):
    caps, facts, _ = gate_inputs(c)
    weight = rnd(c.d, c.num_pred, seed=c.name + "w", scale=0.5)        # fc_predicate.weight
    bias = rnd(c.d, seed=c.name + "b")
    eib, gate, pi = CR.context_indicators(caps, facts, c.K, V, weight, bias, c.mode)
    return dict(caps=caps, facts=facts, weight=weight, bias=bias, eib=eib, gate=gate, pi=pi)


@pytest.mark.parametrize("c", GATE, ids=lambda c: c.name)
def test_context_indicators_forward(ops, c):
    s = gate_setup(c)
    wt = s["weight"].t().contiguous()
    eib, gate = ops.context_indicators(dev(s["caps"]), dev(s["facts"]), c.K, V, dev(wt), dev(s["bias"]), mode=c.mode)
    same_bits(eib.cpu(), s["eib"].float(), "entity_idx_before")
    _, gate_abs, _ = CR.context_indicators_abs(s["caps"], s["facts"], c.K, V, s["weight"], s["bias"], c.mode)
    n = 1 + int(s["pi"].sum(-1).max().item())
    held(gate, s["gate"], gate_abs, n, "gate")
    eib2, dense = ops.context_indicators(dev(s["caps"]), dev(s["facts"]), c.K, V, mode=c.mode, dense_pred=c.num_pred)
    same_bits(eib2.cpu(), s["eib"].float(), "entity_idx_before (dense call)")
    same_bits(dense.cpu(), s["pi"].float(), "dense predicate indicator")


@pytest.mark.parametrize("c", [c for c in GATE if c.bwd], ids=lambda c: c.name)
def test_context_gate_backward(ops, det, c):
    s = gate_setup(c)
    T = c.L if c.mode == 0 else 1
    dgate = rnd(c.B, T, c.d, seed=c.name + "dgate")

    def fn(absval=False, weight=None, bias=None):
        return CR.context_indicators(s["caps"], s["facts"], c.K, V, weight, bias, c.mode)[1]
    leaves = dict(weight=s["weight"], bias=s["bias"])
    g, ga = CR.grads(fn, leaves, dgate), CR.grads(fn, leaves, dgate, absval=True)
    runs = []
    for _ in range(2 if det else 1):
        dw, dbias = prefilled(c.d, c.num_pred, seed=c.name + "dw"), prefilled(c.d, seed=c.name + "dbias")
        ops.context_gate_bwd(dev(s["caps"]), dev(s["facts"]), dev(dgate), dw.t, dbias.t, c.K, V, mode=c.mode)
        runs.append((dw, dbias))
    n = c.B * T + 1
    held(dw, g["weight"], ga["weight"], n, "context_gate_bwd dw")
    held(dbias, g["bias"], ga["bias"], n, "context_gate_bwd dbias")
    if det:
        for a, b2 in zip(*runs):
            same_bits(a.t, b2.t, "context_gate_bwd: two deterministic runs")


# ============================================================================================ pointer scores
COL0, TAIL = 5, 3           # the pointer columns sit at [COL0, COL0 + Kc) of rows COL0 + Kc + TAIL wide


@functools.lru_cache(maxsize=None)
def pointer_setup(c):
    s = dict(h=rnd(c.B, c.T, c.d, seed=c.name + "h"), ctx=rnd(c.B, c.Kc, c.d, seed=c.name + "ctx"),
             w=rnd(1, c.d, seed=c.name + "w", scale=0.5), bias=rnd(1, seed=c.name + "bias"),
             ind=(rnd(c.B, c.T, c.Kc, seed=c.name + "ind") > -0.3).float())
    s["ref"] = CR.pointer_scores(s["h"], s["ctx"], s["w"], s["bias"], s["ind"])
    s["abs"] = CR.pointer_scores_abs(s["h"], s["ctx"], s["w"], s["bias"], s["ind"])
    # packed form: the valid rows (b, t), t < min(T - 1, length - 1), in sample order
    s["valid"] = [(b, t) for b in range(c.B) for t in range(max(0, min(c.T - 1, c.lengths[b] - 1)))]
    return s


@pytest.mark.parametrize("form", ["plain", "out_gmap", "packed"])
@pytest.mark.parametrize("c", POINTER, ids=lambda c: c.name)
def test_pointer_scores_forward(ops, c, form):
    s = pointer_setup(c)
    ld = COL0 + c.Kc + TAIL
    args = (dev(s["h"]), dev(s["ctx"]), dev(s["w"]), dev(s["bias"]))
    nan = float("nan")
    if form == "packed":
        pack = ops.HeadRows(torch.tensor(c.lengths, dtype=torch.int64, device="cuda"), c.B, c.T)
        assert pack.count.item() == len(s["valid"])
        out = torch.full((c.B * c.T, ld), nan, device="cuda")
        ops.pointer_scores(*args, out, COL0, ind=dev(s["ind"]), pack=pack)
        rows = [(m, b, t) for m, (b, t) in enumerate(s["valid"])]
        out = out.cpu()
    else:
        gmap = list(reversed(range(1, c.B + 1))) if form == "out_gmap" else list(range(c.B))   # sample b -> row block
        out = torch.full((c.B + 1, c.T, ld), nan, device="cuda")
        ops.pointer_scores(*args, out, COL0, ind=dev(s["ind"]),
                           out_gmap=torch.tensor(gmap, dtype=torch.int32, device="cuda") if form == "out_gmap" else None)
        rows = [(gmap[b] * c.T + t, b, t) for b in range(c.B) for t in range(c.T)]
        out = out.cpu().view((c.B + 1) * c.T, ld)
    written = torch.zeros(out.shape[0], dtype=torch.bool)
    if rows:
        m_idx = torch.tensor([r[0] for r in rows])
        written[m_idx] = True
        pick = lambda x: torch.stack([x[b, t] for _, b, t in rows])      # noqa: E731
        held(out[m_idx, COL0:COL0 + c.Kc], pick(s["ref"]), pick(s["abs"]), c.d + 1, "pointer_scores[%s]" % form)
        assert torch.isnan(out[m_idx, :COL0]).all() and torch.isnan(out[m_idx, COL0 + c.Kc:]).all(), \
            "columns outside [col0, col0 + Kc) were written"
    assert torch.isnan(out[~written]).all(), "rows beyond the valid ones were written"


@pytest.mark.parametrize("form", ["plain", "packed"])
@pytest.mark.parametrize("c", POINTER, ids=lambda c: c.name)
def test_pointer_scores_backward(ops, det, c, form):
    s = pointer_setup(c)
    ld = COL0 + c.Kc + TAIL
    ds = rnd(c.B * c.T, ld, seed=c.name + "ds")
    up = torch.zeros(c.B, c.T, c.Kc)
    pack = None
    if form == "packed":
        pack = ops.HeadRows(torch.tensor(c.lengths, dtype=torch.int64, device="cuda"), c.B, c.T)
        ds[len(s["valid"]):] = float("nan")                  # packed rows beyond the valid count are never read
        for m, (b, t) in enumerate(s["valid"]):
            up[b, t] = ds[m, COL0:COL0 + c.Kc]
    else:
        up = ds.view(c.B, c.T, ld)[:, :, COL0:COL0 + c.Kc].clone()

    def fn(absval=False, h=None, ctx=None, w=None, bias=None):
        return CR.pointer_scores(h, ctx, w, bias, s["ind"], absval=absval)
    leaves = dict(h=s["h"], ctx=s["ctx"], w=s["w"], bias=s["bias"])
    g, ga = CR.grads(fn, leaves, up), CR.grads(fn, leaves, up, absval=True)
    dsd = dev(ds) if form == "packed" else dev(ds).view(c.B, c.T, ld)
    runs = []
    for _ in range(2 if det else 1):
        outs = dict(h=prefilled(c.B, c.T, c.d, seed=c.name + "dh"), ctx=prefilled(c.B, c.Kc, c.d, seed=c.name + "dctx"),
                    w=prefilled(1, c.d, seed=c.name + "dw"), bias=prefilled(1, seed=c.name + "dbias"))
        ops.pointer_scores_bwd(dsd, COL0, dev(s["h"]), dev(s["ctx"]), dev(s["w"]), dev(s["ind"]), outs["h"].t,
                               outs["ctx"].t, outs["w"].t, outs["bias"].t, pack=pack)
        runs.append(outs)
    total = c.B * c.T * c.Kc + 1
    for k, n in (("h", c.Kc + 1), ("ctx", c.T + 1), ("w", total), ("bias", total)):
        held(outs[k], g[k], ga[k], n, "pointer_scores_bwd[%s] d%s" % (form, k))
    if det:
        for k in outs:
            same_bits(runs[0][k].t, runs[1][k].t, "pointer_scores_bwd d%s: two deterministic runs" % k)


# ============================================================================================ rejections
def _rejected(ops, call, outs, what):
    """The call raises and every output buffer is bit for bit what it was."""
    before = [o.clone() for o in outs]
    with pytest.raises(ops.L.IckError, match="EINVAL"):
        call()
    torch.cuda.synchronize()
    for i, (o, b) in enumerate(zip(outs, before)):
        same_bits(o, b, "%s: output %d changed by a rejected call" % (what, i))


def test_pointer_scores_rejects_d_1025(ops):
    B, T, Kc, d = 1, 2, 3, POINTER_D_REJECTED
    h, ctx, w, b = (dev(rnd(*sh, seed="rej%d" % i)) for i, sh in enumerate([(B, T, d), (B, Kc, d), (1, d), (1,)]))
    out = dev(rnd(B, T, Kc, seed="rejout"))
    _rejected(ops, lambda: ops.pointer_scores(h, ctx, w, b, out, 0), [out], "pointer_scores")
    pack = ops.HeadRows(torch.tensor([2], dtype=torch.int64, device="cuda"), B, T)
    _rejected(ops, lambda: ops.pointer_scores(h, ctx, w, b, out.view(B * T, Kc), 0, pack=pack), [out],
              "pointer_scores packed")


def test_pointer_scores_bwd_rejects_past_its_lds(ops):
    """Plain and packed, in both modes: dh, dctx, dw and dbias all stay as they were."""
    B, T, Kc, d = POINTER_BWD_REJECTED
    h, ctx, w = dev(rnd(B, T, d, seed="rh")), dev(rnd(B, Kc, d, seed="rc")), dev(rnd(1, d, seed="rw"))
    ds = dev(rnd(B, T, Kc, seed="rds"))
    outs = [dev(rnd(*sh, seed="ro%d" % i)) for i, sh in enumerate([(B, T, d), (B, Kc, d), (1, d), (1,)])]
    for mode in (False, True):
        for form in ("plain", "packed"):
            pack = ops.HeadRows(torch.tensor([T], dtype=torch.int64, device="cuda"), B, T) if form == "packed" else None
            dsd = ds.view(B * T, Kc) if pack is not None else ds
            with deterministic_mode(ops, mode):
                _rejected(ops, lambda: ops.pointer_scores_bwd(dsd, 0, h, ctx, w, None, *outs, pack=pack), outs,
                          "pointer_scores_bwd[%s]" % form)


def test_context_gate_bwd_rejects_t_64(ops, det):
    B, L, K, F, d = GATE_BWD_REJECTED
    caps = torch.full((B, L), V + 1, dtype=torch.int64, device="cuda")
    facts = torch.ones(B, F, 3, dtype=torch.int64, device="cuda")
    outs = [dev(rnd(d, 7, seed="gdw")), dev(rnd(d, seed="gdb"))]
    _rejected(ops, lambda: ops.context_gate_bwd(caps, facts, dev(rnd(B, L, d, seed="gdg")), outs[0], outs[1], K, V),
              outs, "context_gate_bwd")


def test_context_indicators_rejects_past_its_lds(ops):
    B, L, K, F = INDICATORS_REJECTED
    caps = torch.full((B, L), V, dtype=torch.int64, device="cuda")
    facts = torch.zeros(B, F, 3, dtype=torch.int64, device="cuda")
    d, num_pred = 8, 7
    wt, bias = dev(rnd(num_pred, d, seed="iw")), dev(rnd(d, seed="ib"))
    outs = [dev(rnd(B, L, F, seed="ie")), dev(rnd(B, L, d, seed="ig"))]
    _rejected(ops, lambda: ops.context_indicators(caps, facts, K, V, wt, bias, eib=outs[0], gate=outs[1]), outs,
              "context_indicators")
