"""Scheduled sampling on the MI355X: ick_sched_sample_mix alone against tests/sched_sample_ref.py on score rows of exact
eighths, and TrainStep(scheduled_sampling=) against the float64 oracle (tests/sched_sample_cases.py).

Bars.  Kernel alone, argmax mode: tokens, masks and `replaced` equal the restatement exactly (eighths: no rounding).  Sample
mode: equal too; a token may differ only where the restatement's perturbed margin is below test_sample_gpu.py's MARGIN
(1e-4), at most once per case, and not at all where the float32 and float64 restatements agree -- which they do on every
case here (test_sched_sample_cpu.py).  Draw distribution: total variation <= 0.03 over 4096 counter values of a
23-column row, test_sample_gpu.py's bound.  Step level: the mixed inputs equal the oracle's exactly (its top-two margin is
>= 1e-3 at every eligible position, test_sched_sample_cpu.py); loss 2e-5 and gradients 2e-3 of max(1e-3, |ref|max) with
the ReLU-flip allowance -- dropout_ref's bars, the ones test_model_geometry_gpu.py applies to the plain captured step."""
import contextlib

import numpy as np
import pytest
import torch

import dropout_ref as DR
import ick_amd.ops as ops
import ick_amd.synth as synth
import model_cases as MC
import sched_sample_cases as SC
import sched_sample_ref as SR
from ick_amd.lib import IckError

pytestmark = pytest.mark.gpu

MARGIN = 1e-4
VX_CASES = ["v52", "v161", "v10026", "v50071"]
OTHER_CASES = [s[0] for s in SC.KERNEL_SHAPES if s[0] not in VX_CASES]
KERNEL_PARAMS = [(n, lay) for n in VX_CASES for lay in SC.LAYOUTS] + [(n, "padded") for n in OTHER_CASES]
kernel_cases = pytest.mark.parametrize("name,layout", KERNEL_PARAMS, ids=["%s-%s" % p for p in KERNEL_PARAMS])


# ------------------------------------------------------------------------------------------------ helpers
def words(prob, T, seed, step):
    seed &= (1 << 64) - 1
    return (torch.tensor([prob], dtype=torch.float32, device="cuda"), torch.tensor([T], dtype=torch.float32, device="cuda"),
            torch.tensor([seed - (1 << 64) if seed >= 1 << 63 else seed], dtype=torch.int64, device="cuda"),
            torch.tensor([step], dtype=torch.int32, device="cuda"))


def device_scores(k, layout, rows=None, fill=float("nan")):
    """The (B, L, Vx) view the packed head would have written: the case's rows at the top of a B * L-row buffer, `fill`
    (NaN: a row the kernel must not read) everywhere else.  tight: ld = Vx; padded: ld a multiple of 4 on a 16-byte
    boundary; offset: that, one float off the boundary."""
    B, L, Vx = k["B"], k["L"], k["Vx"]
    rows = k["rows"] if rows is None else rows
    ld = Vx if layout == "tight" else (Vx + 3) // 4 * 4
    off = 1 if layout == "offset" else 0
    buf = torch.full((B * L * ld + 4,), fill, device="cuda")
    scores = buf[off:off + B * L * ld].view(B, L, ld)[:, :, :Vx]
    if k["M"]:
        scores.view(B * L, Vx)[:k["M"]] = rows.cuda()       # (a view of a strided view: row m of the B * L)
    return scores


def run_mix(k, scores, prob, T=1.0, seed=SC.KERNEL_SEED, step=SC.KERNEL_STEP, mode="argmax", w=None):
    pack = ops.HeadRows(torch.tensor(k["lengths"], dtype=torch.int64, device="cuda"), k["B"], k["L"])
    w = words(prob, T, seed, step) if w is None else w
    out = ops.sched_sample_mix(scores, pack, k["captions"].cuda(), k["masks"].cuda(), k["V"], k["K"], k["F"], k["start"],
                               k["pad"], *w, mode=mode)
    return [t.cpu().numpy() for t in out]


def restate(k, prob, T=1.0, seed=SC.KERNEL_SEED, step=SC.KERNEL_STEP, argmax=True, rows=None, dtype=np.float32):
    rows = k["rows"] if rows is None else rows
    return SR.mix(rows.numpy(), k["lengths"], k["captions"].numpy(), k["masks"].numpy(), k["V"], k["K"], k["F"], k["start"],
                  k["pad"], prob, T, seed, step, argmax, dtype=dtype)


@contextlib.contextmanager
def deterministic_mode():
    try:
        yield
    finally:
        ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ 1. the kernel alone
@kernel_cases
def test_argmax_mode_is_exact(name, layout):
    k = SC.kernel_case(name)
    scores = device_scores(k, layout)
    assert (scores.data_ptr() % 16 == 0) == (layout != "offset")
    for prob in (0.0, 0.5, 1.0):
        ci, mi, rep = run_mix(k, scores, prob)
        rc, rm, rr, _ = restate(k, prob)
        assert np.array_equal(ci, rc) and np.array_equal(mi, rm) and np.array_equal(rep, rr), (name, layout, prob)
        if prob == 0.0:
            assert np.array_equal(ci, k["captions"].numpy()) and np.array_equal(mi, k["masks"].numpy()) and not rep.any()
        if prob == 1.0:
            n, _ = SR.valid_rows(k["lengths"], k["L"])
            assert int(rep.sum()) == int(np.maximum(n - 1, 0).sum())         # every eligible position, no other
            assert not np.isin(ci[rep == 1], (k["start"], k["pad"])).any()   # both hold every row's maximum, and lose
    print("%s %s: %d packed rows, %d replaced at prob 1" % (name, layout, k["M"], int(rep.sum())))


@pytest.mark.parametrize("T", [0.7, 1.0])
@kernel_cases
def test_sample_mode_equals_the_restatement(name, layout, T):
    k = SC.kernel_case(name)
    scores = device_scores(k, layout)
    ci, mi, rep = run_mix(k, scores, 0.5, T=T, mode="sample")
    rc, rm, rr, margins = restate(k, 0.5, T=T, argmax=False)
    r64 = restate(k, 0.5, T=T, argmax=False, dtype=np.float64)
    agree = all(np.array_equal(a, b) for a, b in zip((rc, rm, rr), r64[:3]))
    assert np.array_equal(rep, rr)
    diff = [(b, q) for b, q in zip(*np.nonzero(ci != rc))]
    print("%s %s T %.1f: %d draws, %d differ, smallest restated margin %.3e"
          % (name, layout, T, int(rr.sum()), len(diff), min(margins.values()) if margins else float("inf")))
    assert len(diff) <= (0 if agree else 1), diff
    for b, q in diff:
        assert margins[(b, q)] < MARGIN, (b, q, margins[(b, q)])
    same = ci == rc
    assert np.array_equal(mi[same], rm[same])
    for b, q in diff:
        assert mi[b, q] == SR.token_mask(int(ci[b, q]), k["V"], k["K"])


@pytest.mark.parametrize("mode", ["argmax", "sample"])
def test_rows_that_are_not_replaced_are_not_read(mode):
    """NaN in every packed row whose position loses its coin or is not eligible (the last row of each caption predicts
    position n_b, which is never fed back): the outputs are the clean rows' outputs."""
    k = SC.kernel_case("rows130")
    clean = restate(k, 0.5, argmax=mode == "argmax")
    n, rowstart = SR.valid_rows(k["lengths"], k["L"])
    poisoned = k["rows"].clone()
    kept = 0
    for b in range(k["B"]):
        for t in range(int(n[b])):                    # packed row rowstart[b] + t predicts position t + 1
            if t + 1 > n[b] - 1 or not clean[2][b, t + 1]:
                poisoned[rowstart[b] + t] = float("nan")
            else:
                kept += 1
    assert 0 < kept < k["M"] and kept == int(clean[2].sum())
    ci, mi, rep = run_mix(k, device_scores(k, "padded", rows=poisoned), 0.5, mode=mode)
    assert np.array_equal(ci, clean[0]) and np.array_equal(mi, clean[1]) and np.array_equal(rep, clean[2])


def test_same_bits_twice_and_new_words_without_a_rebuild():
    k = SC.kernel_case("rows130")
    scores = device_scores(k, "padded")
    w = words(0.5, 1.0, 77, 0)
    a = run_mix(k, scores, None, mode="sample", w=w)
    b = run_mix(k, scores, None, mode="sample", w=w)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    w[3].fill_(1)                                     # the counter word: the same launch arguments, new coins
    c = run_mix(k, scores, None, mode="sample", w=w)
    assert np.array_equal(c[2], restate(k, 0.5, seed=77, step=1, argmax=False)[2]) and not np.array_equal(c[2], a[2])
    w[2].fill_(78)                                    # the seed word
    d = run_mix(k, scores, None, mode="sample", w=w)
    assert np.array_equal(d[2], restate(k, 0.5, seed=78, step=1, argmax=False)[2]) and not np.array_equal(d[2], c[2])
    w[0].fill_(1.0)                                   # the probability word
    assert int(run_mix(k, scores, None, mode="sample", w=w)[2].sum()) == int(np.maximum(SR.valid_rows(k["lengths"], k["L"])[0] - 1, 0).sum())


@pytest.mark.parametrize("T", [0.7, 1.0])
def test_draw_distribution(T):
    """One 23-column row (20 words, 3 entities; <start> and <pad> banned), position (0, 1) of one caption of length 3,
    over 4096 values of the counter word: the drawn columns against softmax(s / T) over the allowed columns."""
    V, K, n = 20, 3, 4096
    start, pad = V - 2, 0
    s = torch.tensor([((7 * i) % 23) / 4.0 - 3.0 for i in range(23)])
    scores = torch.zeros(1, 3, 24, device="cuda")[:, :, :23]
    scores[0, 0] = s.cuda()
    caps = torch.tensor([[start, 3, V - 1]], device="cuda")
    masks = torch.zeros_like(caps)
    pack = ops.HeadRows(torch.tensor([3], device="cuda"), 1, 3)
    prob, temp, seed, _ = words(1.0, T, 4242, 0)
    steps = torch.arange(n, dtype=torch.int32, device="cuda")
    outs = (torch.empty(n, 1, 3, dtype=torch.int64, device="cuda"), torch.empty(n, 1, 3, dtype=torch.int64, device="cuda"),
            torch.empty(n, 1, 3, dtype=torch.int32, device="cuda"))
    for i in range(n):
        ops.sched_sample_mix(scores, pack, caps, masks, V, K, 0, start, pad, prob, temp, seed, steps[i:i + 1], mode="sample",
                             out=tuple(o[i] for o in outs))
    drawn = outs[0][:, 0, 1].cpu().numpy()
    assert bool((outs[2][:, 0, 1] == 1).all()) and bool((outs[0][:, 0, 0] == start).all())
    z = (s / T).double().numpy()
    p = np.exp(z - z.max())
    p[[start, pad]] = 0.0
    p /= p.sum()
    tv = 0.5 * np.abs(np.bincount(drawn, minlength=23) / n - p).sum()
    print("T %.1f: total variation %.4f over %d draws" % (T, tv, n))
    assert not np.isin(drawn, (start, pad)).any()
    assert tv <= 0.03, tv


def test_limits_return_einval_without_a_launch():
    import ick_amd.lib as L
    k = SC.kernel_case("v52")
    scores = device_scores(k, "padded")
    pack = ops.HeadRows(torch.tensor(k["lengths"], dtype=torch.int64, device="cuda"), k["B"], k["L"])
    caps, masks = k["captions"].cuda(), k["masks"].cuda()
    w = words(1.0, 1.0, 1, 0)
    outs = [torch.full((k["B"], k["L"]), -7, dtype=torch.int64, device="cuda") for _ in range(2)] + \
           [torch.full((k["B"], k["L"]), -7, dtype=torch.int32, device="cuda")]
    p = lambda t: None if t is None else t.data_ptr()      # noqa: E731

    def call(B=k["B"], Lc=k["L"], V=k["V"], K=k["K"], F=k["F"], ld=scores.stride(1), prob=w[0], temp=w[1], seed=w[2],
             step=w[3], sc=scores, out0=outs[0]):
        return L.load().ick_sched_sample_mix(p(sc), ld, p(pack.rowstart), p(pack.decode_len), p(caps), p(masks), B, Lc, V, K,
                                             F, k["start"], k["pad"], p(prob), p(temp), p(seed), p(step), 1, p(out0),
                                             p(outs[1]), p(outs[2]), None)
    bad = [dict(Lc=1), dict(B=0), dict(B=1 << 20, Lc=1 << 12), dict(V=(1 << 24) - 10), dict(ld=k["Vx"] - 1), dict(prob=None),
           dict(temp=None), dict(seed=None), dict(step=None), dict(sc=None), dict(out0=None)]
    for kw in bad:
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert all(bool((o == -7).all()) for o in outs)
    assert call() == 0
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), restate(k, 1.0, seed=1, step=0)[0])
    with pytest.raises(IckError, match="unknown mode"):
        ops.sched_sample_mix(scores, pack, caps, masks, k["V"], k["K"], k["F"], k["start"], k["pad"], *w, mode="greedy")
    with pytest.raises(IckError, match="one-element"):
        ops.sched_sample_mix(scores, pack, caps, masks, k["V"], k["K"], k["F"], k["start"], k["pad"], 0.5, *w[1:])


# ------------------------------------------------------------------------------------------------ 2. the training step
step_cases = pytest.mark.parametrize("c", SC.CASES, ids=[c.name for c in SC.CASES])
ARGMAX_ALL = dict(prob=1.0, mode="argmax")


def train_decoder(c, P):
    from test_training_gpu import zero_dropout
    return zero_dropout(MC.build_decoder(c, P).train())


def make_step(c, P, ss, **kw):
    from ick_amd.training import TrainStep
    return TrainStep(train_decoder(c, P), lr=MC.LR, grad_clip=MC.CLIP, scheduled_sampling=ss, **kw)


def inputs_of(c, seed=SC.SEED):
    return MC.step_args(*MC.make_inputs(c, seed))


@step_cases
def test_prob_one_argmax_step_vs_oracle(c):
    o = SC.oracle(c)
    ts = make_step(c, o["P"], ARGMAX_ALL)
    loss = ts(*inputs_of(c))
    assert ts.use_graph and len(ts._graphs) == 1 and ts.derived is not None
    ci, mi, rep = (t.cpu() for t in ts.sampled_inputs())
    assert torch.equal(rep, o["replaced"]) and torch.equal(ci, o["captions_in"]) and torch.equal(mi, o["masks_in"])
    if c.variant != "geo":
        # pointer tokens were fed back: the context indicators / predicate gate and their backward follow the mixed input
        assert int((mi[rep == 1] > 0).sum()) >= 1
    print("%s: %d replaced (%d pointer tokens), loss %.6f, oracle %.6f (err %.2e)"
          % (c.name, int(rep.sum()), int((mi[rep == 1] > 0).sum()), loss.item(), o["loss"], abs(loss.item() - o["loss"])))
    assert abs(loss.item() - o["loss"]) < DR.LOSS_BAR, (loss.item(), o["loss"])
    mine = {k: ts.grads[id(p)] for k, p in ts.dec.named_parameters() if id(p) in ts.grads}
    DR.check_grads(mine, o["grads"], "%s scheduled sampling" % c.name, clamp=MC.CLIP)


@step_cases
def test_prob_zero_is_the_plain_step_bit_for_bit(c):
    """Three steps on alternating batches in deterministic mode (the default mode's float atomics differ from run to run,
    with or without the feature): loss, parameters and moments equal those of a step built without the argument."""
    P = MC.make_params(c)
    runs = []
    with deterministic_mode():
        for ss in (None, dict(prob=0.0, mode="sample")):
            ts = make_step(c, P, ss, deterministic=True)
            losses = [ts(*inputs_of(c, s)).item() for s in SC.STEP_SEEDS]
            assert ts.use_graph
            runs.append((losses, ts.flat_p.clone(), ts.flat_m.clone(), ts.flat_v.clone()))
            if ss is not None:
                assert not bool(ts.sampled_inputs()[2].any())
    assert runs[0][0] == runs[1][0]
    for a, b in zip(runs[0][1:], runs[1][1:]):
        assert torch.equal(a, b)


@step_cases
def test_three_captured_steps_equal_the_eager_twin(c):
    """Deterministic mode, prob 0.5, mode "sample": the captured step and its use_graph=False twin are bit-identical over
    the batches of seeds 25, 26, 25 -- a first pass on a stale weight image would part them at step 2 --, the coins of
    steps 1 and 3 (same batch, another counter) differ, and the setters replay the one graph."""
    P = MC.make_params(c)
    runs = []
    with deterministic_mode():
        for use_graph in (True, False):
            ts = make_step(c, P, dict(prob=0.5, mode="sample", seed=5), deterministic=True, use_graph=use_graph)
            seen = []
            for i, s in enumerate(SC.STEP_SEEDS):
                loss = ts(*inputs_of(c, s)).item()
                seen.append((loss,) + tuple(t.clone() for t in ts.sampled_inputs()))
                if i == 0:
                    graph = next(iter(ts._graphs.values()))[0] if use_graph else None
                    ts.set_sampling_prob(0.5)
                    ts.set_sampling_temperature(1.0)
            if use_graph:
                assert ts.use_graph and len(ts._graphs) == 1 and next(iter(ts._graphs.values()))[0] is graph
            assert int(ts.counter.item()) == 3
            runs.append((seen, ts.flat_p.clone(), ts.flat_m.clone()))
    (g, gp, gm), (e, ep, em) = runs
    for i, (a, b) in enumerate(zip(g, e)):
        assert a[0] == b[0], ("loss of step %d" % (i + 1), a[0], b[0])
        assert all(torch.equal(x, y) for x, y in zip(a[1:], b[1:])), "mixed inputs of step %d" % (i + 1)
    assert torch.equal(gp, ep) and torch.equal(gm, em)
    assert 0 < int(g[0][3].sum()) and not torch.equal(g[0][3], g[2][3])


def test_setters_change_the_draw_without_a_capture():
    c = SC.CASES[0]
    ts = make_step(c, MC.make_params(c), dict(prob=1.0, mode="sample", temperature=1.0))
    args = inputs_of(c)
    ts(*args)
    graph = next(iter(ts._graphs.values()))[0]
    n_el = int(ts.sampled_inputs()[2].sum())
    ts.set_sampling_prob(0.0)
    ts(*args)
    assert int(ts.sampled_inputs()[2].sum()) == 0 and torch.equal(ts.sampled_inputs()[0], args[0])
    ts.set_sampling_prob(1.0)
    ts.set_sampling_temperature(1e-4)         # the noise no longer matters: the draw is the argmax of the scores
    ts(*args)
    assert int(ts.sampled_inputs()[2].sum()) == n_el
    assert len(ts._graphs) == 1 and next(iter(ts._graphs.values()))[0] is graph


def test_split_step_and_optimizer_options(monkeypatch):
    """The two-graph step (ICK_SPLIT_ALLREDUCE=1) feeds and trains on the same mixed inputs as the single graph, and a
    step with every optimizer option on runs its three steps on one capture."""
    c = SC.CASES[1]
    o = SC.oracle(c)
    monkeypatch.setenv("ICK_SPLIT_ALLREDUCE", "1")
    ts = make_step(c, o["P"], ARGMAX_ALL)
    assert ts.split
    loss = ts(*inputs_of(c))
    assert ts.use_graph and next(iter(ts._graphs.values()))[3] is not None
    assert torch.equal(ts.sampled_inputs()[0].cpu(), o["captions_in"]) and abs(loss.item() - o["loss"]) < DR.LOSS_BAR
    monkeypatch.delenv("ICK_SPLIT_ALLREDUCE")
    ts = make_step(c, o["P"], dict(prob=0.5, mode="sample"), label_smoothing=0.1, max_grad_norm=1.0, ema_decay=0.99,
                   weight_decay=0.01, lr_schedule=dict(kind="constant", warmup_steps=2))
    losses = [ts(*inputs_of(c, s)).item() for s in SC.STEP_SEEDS]
    assert not ts.split and ts.use_graph and len(ts._graphs) == 1 and all(np.isfinite(losses))
    assert int(ts.counter.item()) == 3 and float(ts.grad_norm.item()) > 0


def conv1_case():
    from test_conv1_train_gpu import small_case
    return small_case("geo", 5)


def test_feature_map_with_an_attached_encoder():
    """One step from the 4-D feature map (Encoder.conv1 inside both passes) against one from the encoder's output."""
    from ick_amd.training import TrainStep
    from test_bench_sizes_gpu import make_encoder
    from test_conv1_train_gpu import step_args
    from test_forward_gpu import build_decoder
    from test_training_gpu import zero_dropout
    cfg, P, batch, feats, cw, cb = conv1_case()
    got = []
    for four_d in (True, False):
        enc, _, _ = make_encoder(31)
        dec = zero_dropout(build_decoder(cfg.variant, cfg.vocab_size, P).train())
        ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP, encoder=enc, scheduled_sampling=ARGMAX_ALL, lazy_update=True)
        args = step_args(batch, feats)
        if not four_d:
            with torch.no_grad():
                args[1] = enc(feats.cuda())
        loss = ts(*args)
        assert ts.use_graph and not ts._pending and int(ts.counter.item()) == 1       # lazy_update defers nothing here
        got.append((loss.item(), [t.clone() for t in ts.sampled_inputs()]))
    assert abs(got[0][0] - got[1][0]) < DR.LOSS_BAR
    assert int(got[0][1][2].sum()) > 0 and all(torch.equal(a, b) for a, b in zip(got[0][1], got[1][1]))


def test_train_conv1_step_vs_oracle():
    """train_conv1=True at B = 5 (tests/test_conv1_train_gpu.py's case): loss and every gradient, conv1's included, against
    the oracle run on the step's mixed inputs and the gold targets; the mixed inputs against the oracle's own argmax
    wherever its top-two margin is at least 1e-3."""
    from oracle import restatement as R
    from test_conv1_train_gpu import CLIP, build_step, check_gradients, step_args
    cfg, P, batch, feats, cw, cb = conv1_case()
    ts, dec, enc = build_step(cfg, P, 31, scheduled_sampling=ARGMAX_ALL)
    loss = ts(*step_args(batch, feats))
    assert ts.use_graph and len(ts._graphs) == 1
    ci, mi, rep = (t.cpu() for t in ts.sampled_inputs())
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
    conv = {"conv1.weight": cw.clone().requires_grad_(True), "conv1.bias": cb.clone().requires_grad_(True)}
    enc_out = R.feat_proj(feats, conv["conv1.weight"], conv["conv1.bias"])
    with torch.no_grad():
        st = {}
        s1, _, _ = R.forward(cfg, Pr, batch["captions"], enc_out, batch["caption_masks"], batch["caption_lengths"],
                             batch["entities"], stages=st)
    wm = synth.make_word_map(cfg.vocab_size)
    lengths = batch["caption_lengths"].view(-1).tolist()
    checked = 0
    for r, b in enumerate(st["sort_ind"].tolist()):
        for q in range(1, lengths[b] - 1):
            s = s1[r, q - 1].clone()
            s[wm["<start>"]] = s[wm["<pad>"]] = float("-inf")
            top = s.topk(2)
            assert rep[b, q] == 1
            if top.values[0] - top.values[1] >= SC.MIN_MARGIN:
                assert ci[b, q] == top.indices[0] and mi[b, q] == (0 if ci[b, q] < cfg.vocab_size else 1)
                checked += 1
    assert checked >= 1 and int(rep.sum()) == sum(max(0, n - 2) for n in lengths)
    scores, _, dl = R.forward(cfg, Pr, ci, enc_out, mi, batch["caption_lengths"], batch["entities"])
    ref = R.packed_ce_loss(cfg, scores, batch["captions"][st["sort_ind"]], dl)
    ref.backward()
    assert abs(loss.item() - ref.item()) < 2e-5, (loss.item(), ref.item())
    grads = {k: v.grad if v.grad is not None else torch.zeros_like(v) for k, v in list(Pr.items()) + list(conv.items())}
    check_gradients(ts, dec, grads, "train_conv1 + scheduled sampling")
    assert CLIP == MC.CLIP


def test_refusals():
    from ick_amd.scst import SelfCriticalStep
    from ick_amd.training import TrainStep
    c = SC.CASES[0]
    P = MC.make_params(c)
    dec = train_decoder(c, P)
    for bad, text in ((dict(prob=-0.01), "prob must lie"), (dict(prob=1.01), "prob must lie"),
                      (dict(temperature=0.0), "temperature must be"), (dict(temperature=-2.0), "temperature must be"),
                      (dict(mode="beam"), "unknown mode"), (dict(p=0.5), "must be a dict of")):
        with pytest.raises(IckError, match=text):
            TrainStep(dec, scheduled_sampling=bad)
    ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP, scheduled_sampling=dict(prob=0.25))
    args = inputs_of(c)
    with pytest.raises(IckError, match="no caption_weights and no image_index"):
        ts(*args, caption_weights=torch.ones(MC.B, device="cuda"))
    with pytest.raises(IckError, match="no caption_weights and no image_index"):
        ts(*args, image_index=torch.arange(MC.B, device="cuda"))
    with pytest.raises(IckError, match="scheduled_sampling"):
        SelfCriticalStep(ts, lambda tokens: [0.0] * len(tokens))
    for bad in (-0.5, 1.5, float("nan")):
        with pytest.raises(IckError, match="prob must lie"):
            ts.set_sampling_prob(bad)
    with pytest.raises(IckError, match="temperature must be"):
        ts.set_sampling_temperature(0)
    with pytest.raises(IckError, match="no step has run"):
        ts.sampled_inputs()
    assert int(ts.counter.item()) == 0 and not ts._graphs            # nothing was launched
    plain = TrainStep(train_decoder(c, P), lr=MC.LR, grad_clip=MC.CLIP)
    assert plain.ss is None and plain._ss_words is None and not plain._ss_bufs
    for call in (lambda: plain.set_sampling_prob(0.5), lambda: plain.set_sampling_temperature(1.0), plain.sampled_inputs):
        with pytest.raises(IckError, match="needs a TrainStep built with scheduled_sampling="):
            call()


@pytest.mark.parametrize("prefetch", [True, False], ids=["pipelined_loop", "plain_loop"])
def test_train_main_with_scheduled_sampling(tmp_path, prefetch):
    from ick_amd import train as tr
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    torch.manual_seed(0)
    cfg = tr.Config(variant="geo", data_dir=data_dir, data_name="toy", batch_size=8, workers=0, print_freq=1000, fused=True,
                    seed=3, out_dir=str(tmp_path), prefetch=prefetch, epochs=2, scheduled_sampling_start=0,
                    scheduled_sampling_increase_every=1, scheduled_sampling_increase_prob=0.2,
                    scheduled_sampling_max_prob=0.3)
    hist = tr.main(cfg)
    assert len(hist) == 2 and all(np.isfinite(h[0]) for h in hist)
    assert tr.STATS["sampling_prob"] == pytest.approx(0.3)           # epoch 1: min(0.3, 0.2 * 2)
