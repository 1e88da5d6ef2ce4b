"""The exponential moving average of the parameters inside the fused Adam pass on the GPU:
  * ick_adam_step with e alone on raw buckets: p, g, m, v are the bits of the call without e, e is the float32
    restatement (tests/ema_ref.py) of the new p, at every size where a kernel path begins or ends;
  * ick_adam_step_derive with e over a real decoder's cover: the flat form's bits, the images of the call without e;
  * TrainStep(ema_decay=) against a twin without it: the same loss, parameters and moments, and the average of every
    parameter is the restatement folded over the twin's parameter snapshots;
  * set_ema_decay replays, lazy_update, ema_weights(), the state round trip, and the training script.
Twins are compared bit for bit in deterministic mode: outside it the weight gradients' float atomics are unordered and
two runs of the SAME step differ (tests/test_adam_derive_gpu.py compares such runs with a tolerance)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
from ema_ref import decay_at32, ema_fold32, ema_update32
from ick_amd.lib import OPT_WORDS, IckError
from ick_amd.training import DerivedWeights, TrainStep
from test_bench_sizes_gpu import make_encoder
from test_forward_gpu import build_decoder
from test_label_smoothing_gpu import STEP_CASES, _count_captures, same_bits, step_args, step_case
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu

DECAY = 0.9
SENTINEL = 12345.0


@pytest.fixture()
def det_off_after():
    yield
    ops.set_deterministic(False)


def decay_word(d=DECAY):
    return torch.full((1,), d, device="cuda")


# ------------------------------------------------------------------------------------------------ the kernel alone
# 1, 3, 4095: the scalar kernel only; 4096: the float4 kernel only; 4099: float4 plus a scalar tail; "offset": a bucket
# that starts one float behind a 16-byte boundary (scalar kernel at a float4 size); 2^22 + 4100: the float4 kernel's
# 4096 workgroups of 256 lanes make a second trip of the grid-stride loop
SIZES = [1, 3, 4095, 4096, 4096 + 3, "offset", (1 << 22) + 4100]
MODES = ["plain", "words", "warmup_step1", "warmup_step1000", "no_tokens"]
_BUCKETS = {}


def bucket(n, offset):
    """Five arrays p, g, m, v, e of n floats behind `offset` floats, sentinels on both sides (shared: tests clone)."""
    key = (n, offset)
    if key not in _BUCKETS:
        _BUCKETS.clear()
        gen = torch.Generator(device="cuda").manual_seed(n)
        arrays = []
        for scale, positive in ((1.0, False), (4.0, False), (0.01, False), (1e-3, True), (1.0, False)):
            buf = torch.full((offset + n + 4,), SENTINEL, device="cuda")
            x = torch.rand(n, device="cuda", generator=gen) if positive else torch.randn(n, device="cuda", generator=gen)
            buf[offset:offset + n] = x * scale
            arrays.append(buf)
        _BUCKETS[key] = arrays
    return [b.clone() for b in _BUCKETS[key]]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_kernel_keeps_adams_bits_and_the_restatements_average(size, mode):
    n, offset = (4096 + 3, 1) if size == "offset" else (size, 0)
    step0 = 999 if mode == "warmup_step1000" else 0
    warm = mode.startswith("warmup")
    counter = torch.full((1,), step0, device="cuda", dtype=torch.int32)
    den = torch.tensor([0.0 if mode == "no_tokens" else 7.0], device="cuda")
    rate = dict(lr=4e-4)
    if mode == "words":
        w = torch.zeros(OPT_WORDS, device="cuda")
        w[0], w[3] = 4e-4, 0.25
        rate = dict(words=w, schedule=dict(kind="cosine", warmup_steps=2, total_steps=9, min_lr_ratio=0.1))
    common = dict(clip=0.5, gscale=1.0, step_tensor=counter, gscale_den=den)
    ref, mine = bucket(n, offset), bucket(n, offset)
    view = lambda bufs: [b[offset:offset + n] for b in bufs]          # noqa: E731
    if mode == "words":
        rate_ref = dict(rate, words=rate["words"].clone())
    else:
        rate_ref = rate
    ops.adam_update(*view(ref)[:4], 1, **common, **rate_ref)
    word = decay_word()
    ops.adam_update(*view(mine)[:4], 1, **common, **rate, ema=view(mine)[4], ema_decay_word=word, ema_warmup=warm)
    torch.cuda.synchronize()
    for a, b, what in zip(mine[:4], ref[:4], "pgmv"):
        assert same_bits(a, b), (what, size, mode)                     # (whole buffers: the sentinels are intact too)
    e0 = ref[4]
    assert all(float(b[offset + n:].min()) == SENTINEL == float(b[offset + n:].max()) for b in mine)
    assert offset == 0 or all(float(b[0]) == SENTINEL for b in mine)
    if mode == "no_tokens":
        assert same_bits(mine[4], e0) and same_bits(mine[0], bucket(n, offset)[0])      # nothing is written, e included
        return
    assert not same_bits(mine[0], bucket(n, offset)[0])
    want = ema_update32(e0[offset:offset + n].cpu().numpy(), mine[0][offset:offset + n].cpu().numpy(), step0 + 1, DECAY,
                        warm)
    got = mine[4][offset:offset + n].cpu().numpy()
    assert np.array_equal(got.view(np.int32), want.view(np.int32)), (size, mode, np.abs(got - want).max())
    if warm:      # the ramp binds at step 1 (2/11 < 0.9) and no longer at step 1000 (1001/1010 > 0.9)
        assert (decay_at32(step0 + 1, DECAY, True) < np.float32(DECAY)) == (step0 == 0)
    if mode == "words":
        assert rate["words"][4].item() == rate_ref["words"][4].item() != 0.0            # the rate word is written as before


# ------------------------------------------------------------------------------------------------ the cover
def _images(dw):
    wi = dw.owner
    out = {"pk": wi.flat["chain"], "pkb": wi.flat["chain_t"], "kvT": wi.chain_t[("kv", "T")], "wkv": wi.wkv, "bkv": wi.bkv,
           "wkv_ps": wi.kv_ps, "vocab_ps": wi.vocab_ps, "vocab_t_ps": wi.vocab_t_ps}
    if wi.pred_wt is not None:
        out["pred_wt"] = wi.pred_wt
    return out


@pytest.mark.parametrize("rate", ["lr", "words"])
@pytest.mark.parametrize("variant,V", [("geo", 200), ("knowledge", 160)])
def test_derive_form_has_the_flat_forms_bits_and_the_plain_covers_images(variant, V, rate):
    dec = build_decoder(variant, V, synth.make_params(variant, V, 3)).train()
    kw = dict(max_grad_norm=1e9, lr_schedule=dict(kind="linear", warmup_steps=2, total_steps=20)) if rate == "words" else {}
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, ema_decay=DECAY, ema_warmup=True, **kw)
    ts.derived = dw = DerivedWeights.build(ts)
    assert dw is not None and dw.n_blocks > 50
    dw.refresh()
    gen = torch.Generator(device="cuda").manual_seed(1)
    n = ts.n
    used = torch.zeros(n, dtype=torch.bool, device="cuda")              # (the pads between the parameters stay zero)
    for p in ts.params:
        off = (p.data_ptr() - ts.flat_p.data_ptr()) // 4
        used[off:off + p.numel()] = True
    rnd = lambda: torch.randn(n, device="cuda", generator=gen) * used    # noqa: E731
    ts.flat_g[:n] = rnd() * 40.0                                         # some elements beyond the clamp (5 x 7 tokens)
    ts.flat_g[n], ts.flat_g[n + 1] = 3.5, 7.0
    ts.flat_m.copy_(rnd() * 0.01)
    ts.flat_v.copy_(rnd().abs() * 1e-3)
    ts.flat_e.copy_(ts.flat_p + rnd() * 0.01)
    ts.counter.fill_(4)
    start = [t.clone() for t in (ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v, ts.flat_e)]
    ts._adam()                                                                   # ick_adam_step_derive, e != NULL
    torch.cuda.synchronize()
    mine = [t.clone() for t in (ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v, ts.flat_e)]
    images = {k: v.clone() for k, v in _images(dw).items()}
    # the flat form on copies
    flat = [t.clone() for t in start]
    words = dict(words=ts._words, schedule=ts._sched) if rate == "words" else dict(lr=4e-4)
    common = dict(clip=5.0, gscale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, step_tensor=ts.counter,
                  gscale_den=ts.flat_g[n + 1:])
    ops.adam_update(flat[0], flat[1][:n], flat[2], flat[3], 1, **common, **words, ema=flat[4], ema_decay_word=ts._ema_word,
                    ema_warmup=True)
    for a, b, what in zip(mine, flat, "pgmve"):
        assert same_bits(a[:n], b[:n]), (what, variant, rate)
    assert not same_bits(mine[4], start[4]) and not same_bits(mine[0], start[0])
    # the cover without the average, from the same start: the same images (images of p, not of e)
    for t, s in zip((ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v), start):
        t.copy_(s)
    ops.adam_update(ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v, 1, cover=dw, **common, **words)
    torch.cuda.synchronize()
    assert same_bits(ts.flat_p, mine[0])
    for k, v in _images(dw).items():
        assert same_bits(images[k], v), (variant, k)
    # pads between the parameters stay zero in the average
    assert float(mine[4][~used].abs().max()) == 0.0 and int((~used).sum()) > 0


# ------------------------------------------------------------------------------------------------ TrainStep against a twin
def run_twin(name, nsteps=4, dropout=True, deterministic=True, conv1=False, **kw):
    """nsteps steps; after every step the loss and copies of the parameters, moments (and the averages)."""
    variant, V, P, cfg, batch, enc_out = step_case(name)
    dec = build_decoder(variant, V, P).train()
    if not dropout:
        zero_dropout(dec)
    args = step_args(variant, batch, enc_out)
    if conv1:
        enc, _, _ = make_encoder(17)
        kw.update(encoder=enc, train_conv1=True, encoder_lr=1e-3)
        args[1] = synth.make_feats(batch["captions"].shape[0], 17).cuda()
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, seed=11, deterministic=deterministic, **kw)
    e0 = [t.clone() for t in (ts.flat_e, ts.enc_e) if t is not None]
    log = []
    for _ in range(nsteps):
        loss = ts(*args).clone()
        state = [ts.flat_p, ts.flat_m, ts.flat_v] + ([ts.enc_p, ts.enc_m, ts.enc_v] if conv1 else [])
        avg = [t for t in (ts.flat_e, ts.enc_e) if t is not None]
        log.append((loss, [t.clone() for t in state], [t.clone() for t in avg]))
    return ts, dec, args, log, e0


def check_against_twin(with_ema, twin, decay=DECAY, warmup=False):
    (ts, _, _, log, e0), (ts0, _, _, log0, _) = with_ema, twin
    assert ts0.flat_e is None and ts0._ema_word is None and ts.flat_e is not None
    snaps = [[] for _ in e0]
    for i, ((loss, state, avg), (loss0, state0, _)) in enumerate(zip(log, log0)):
        assert same_bits(loss, loss0), i
        assert all(same_bits(a, b) for a, b in zip(state, state0)), i
        for k in range(len(e0)):
            snaps[k].append(state0[3 * k].cpu().numpy())                # flat_p[, enc_p] of the twin
            want = ema_fold32(e0[k].cpu().numpy(), snaps[k], decay, warmup)
            got = avg[k].cpu().numpy()
            assert np.array_equal(got.view(np.int32), want.view(np.int32)), (i, k, np.abs(got - want).max())
    assert not same_bits(log[-1][2][0], e0[0]) and not same_bits(log[-1][2][0], log[-1][1][0])     # it moved, and lags p


@pytest.mark.parametrize("derive", ["cover", "no_cover"])
@pytest.mark.parametrize("name", ["geo", "knowledge"])
def test_four_steps_equal_the_twin_and_the_folded_restatement(name, derive, monkeypatch, det_off_after):
    monkeypatch.setenv("ICK_ADAM_DERIVE", "1" if derive == "cover" else "0")
    a = run_twin(name, ema_decay=DECAY)
    assert a[0].use_graph and (a[0].derived is not None) == (derive == "cover")
    check_against_twin(a, run_twin(name))


def test_with_clip_schedule_and_warmup(det_off_after):
    kw = dict(max_grad_norm=0.5, lr_schedule=dict(kind="cosine", warmup_steps=2, total_steps=8, min_lr_ratio=0.1))
    check_against_twin(run_twin("geo", ema_decay=DECAY, ema_warmup=True, **kw), run_twin("geo", **kw), warmup=True)


def test_with_train_conv1_and_the_same_bits_twice(det_off_after):
    a = run_twin("geo", conv1=True, ema_decay=DECAY)
    assert a[0].enc_e is not None and a[0].enc_e.numel() == a[0].ne
    check_against_twin(a, run_twin("geo", conv1=True))
    b = run_twin("geo", conv1=True, ema_decay=DECAY)                     # deterministic mode: the same bits twice
    assert all(same_bits(x, y) for (_, _, ax), (_, _, bx) in zip(a[3], b[3]) for x, y in zip(ax, bx))


def test_default_step_allocates_nothing_and_refuses_the_methods():
    variant, V, P, cfg, batch, enc_out = step_case("geo")
    dec = build_decoder(variant, V, P).train()
    ts = TrainStep(dec)
    assert ts.ema_decay is None and ts.flat_e is None and ts.enc_e is None and ts._ema_word is None
    for call in (ts.ema_state_dict, lambda: ts.load_ema_state_dict({}), lambda: ts.ema_weights().__enter__(),
                 lambda: ts.set_ema_decay(0.9)):
        with pytest.raises(IckError):
            call()
    ts.set_ema_decay(None)                                               # (off stays off)
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(IckError):
            TrainStep(dec, ema_decay=bad)
    ts2 = TrainStep(dec, ema_decay=0.5)
    with pytest.raises(IckError):
        ts2.set_ema_decay(None)                                          # ... and on stays on
    for bad in (-0.1, 1.0, float("nan")):
        with pytest.raises(IckError):
            ts2.set_ema_decay(bad)
    assert ts2.ema_decay == 0.5 and ts2._ema_word.item() == 0.5 and "ema" not in "".join(ts2.state_dict())


# ------------------------------------------------------------------------------------------------ graphs, lazy update
def test_set_ema_decay_replays_the_captured_graphs(det_off_after):
    ts, dec, args, log, e0 = run_twin("geo", nsteps=1, ema_decay=DECAY)
    graphs = dict(ts._graphs)
    calls = _count_captures(ts)
    ts.set_ema_decay(0.5)
    e1, = log[0][2]
    ts(*args)
    assert ts._graphs == graphs and not calls and ts.use_graph
    want = ema_update32(e1.cpu().numpy(), ts.flat_p.cpu().numpy(), 2, 0.5)
    assert np.array_equal(ts.flat_e.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not np.array_equal(want, ema_update32(e1.cpu().numpy(), ts.flat_p.cpu().numpy(), 2, DECAY))


def test_lazy_update_keeps_the_average_with_the_deferred_update():
    """lazy_update needs the two-stream step, which deterministic mode excludes, so the eager twin's gradients differ by
    the float atomics' order (tests/test_adam_derive_gpu.py).  What is exact: after call i + 1 the bucket holds update i,
    so the run's own snapshots fold to its own average, bit for bit -- the deferred launch keeps the average like the
    eager one.  Against the eager twin: the existing lazy test's tolerance."""
    variant, V, P, cfg, batch, enc_out = step_case("geo")
    enc, _, _ = make_encoder(13)
    args = step_args(variant, batch, enc_out)
    args[1] = synth.make_feats(batch["captions"].shape[0], 13).cuda()
    out = []
    for lazy in (True, False):
        dec = zero_dropout(build_decoder(variant, V, P).train())
        ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, encoder=enc, lazy_update=lazy, ema_decay=DECAY, deterministic=False)
        e0, snaps = ts.flat_e.clone(), []
        for i in range(4):
            ts(*args)
            torch.cuda.synchronize()
            if not lazy or i > 0:
                snaps.append(ts.flat_p.cpu().numpy().copy())
        if lazy:
            assert ts._pending and ts._lazy_active(args[1]) and int(ts.counter.item()) == 3
            assert same_bits(ts.flat_e, torch.from_numpy(ema_fold32(e0.cpu().numpy(), snaps, DECAY)).cuda())
        sd = ts.ema_state_dict()                                         # flushes
        assert not ts._pending and int(ts.counter.item()) == 4
        if lazy:
            snaps.append(ts.flat_p.cpu().numpy().copy())
        assert len(snaps) == 4
        want = ema_fold32(e0.cpu().numpy(), snaps, DECAY)
        assert np.array_equal(ts.flat_e.cpu().numpy().view(np.int32), want.view(np.int32)), lazy
        assert all(same_bits(t, ts._slot(ts.flat_e, p)) for t, p in zip(sd["params"], ts._adam_order()))
        out.append(ts.flat_e.clone())
    assert (out[0] - out[1]).abs().max().item() <= 4 * 4e-4 + 1e-6
    assert ((out[0] - out[1]).abs() > 1e-4).float().mean().item() < 0.02


# ------------------------------------------------------------------------------------------------ ema_weights()
def _fresh_with(ts, dec, name, tensors):
    """A fresh decoder whose trained parameters hold `tensors` (ema_state_dict()["params"] order)."""
    variant, V = STEP_CASES[name][0], STEP_CASES[name][1]
    sd = {k: v.detach().clone() for k, v in dec.state_dict().items() if k != "pos_encoder.pe"}
    avg = {id(p): t for p, t in zip(ts._adam_order(), tensors)}
    for k, p in dec.named_parameters(remove_duplicate=False):           # (a shared parameter has several names)
        if id(p) in avg:
            sd[k] = avg[id(p)].clone()
    return build_decoder(variant, V, sd)


@pytest.mark.parametrize("raises", [False, True], ids=["plain_exit", "body_raises"])
def test_ema_weights_shows_the_average_and_restores_the_parameters(raises, det_off_after):
    name = "knowledge"
    ts, dec, args, log, _ = run_twin(name, nsteps=3, dropout=False, ema_decay=DECAY)
    twin, _, _, _, _ = run_twin(name, nsteps=3, dropout=False, ema_decay=DECAY)
    avg = ts.ema_state_dict()
    fresh = _fresh_with(ts, dec, name, avg["params"]).eval()
    p_before, e_before = ts.flat_p.clone(), ts.flat_e.clone()
    tail = args[2:]
    with torch.no_grad():
        want_scores = fresh(args[0], args[1], *tail)[0].clone()
        want_seq = fresh.predict(args[1], 8, *args[4:]).clone()
    dec.eval()
    with (pytest.raises(ZeroDivisionError) if raises else contextlib.nullcontext()):
        with ts.ema_weights():
            assert same_bits(ts.flat_p, e_before) and same_bits(ts.flat_e, p_before)
            with torch.no_grad():
                got_scores = dec(args[0], args[1], *tail)[0]
                print("scores inside ema_weights() against the fresh decoder's: max |diff| %.3g"
                      % (got_scores - want_scores).abs().max().item())
                assert same_bits(got_scores, want_scores)
                assert torch.equal(dec.predict(args[1], 8, *args[4:]), want_seq)
            with pytest.raises(IckError, match="ema_weights"):
                ts(*args)
            with pytest.raises(IckError):
                ts.ema_weights().__enter__()
            with pytest.raises(IckError, match="ema_weights"):          # the buckets are exchanged: no state from in here
                ts.ema_state_dict()
            if raises:
                1 / 0
    assert same_bits(ts.flat_p, p_before) and same_bits(ts.flat_e, e_before) and not ts._ema_swapped
    with torch.no_grad():
        assert not same_bits(dec(args[0], args[1], *tail)[0], want_scores)            # the raw weights again
    dec.train()
    loss, loss_twin = ts(*args).clone(), twin(*args).clone()                            # the weight images are current
    assert same_bits(loss, loss_twin) and same_bits(ts.flat_p, twin.flat_p) and same_bits(ts.flat_e, twin.flat_e)


def test_ema_weights_exchanges_conv1_and_the_next_step_equals_the_twin(det_off_after):
    """train_conv1: conv1's pair is exchanged too, the encoder's pre-split copy follows the weights in and out of the
    context (enc(feats) equals, bit for bit, a fresh encoder's with the averaged / the raw conv1), and the step after the
    context equals the twin that never swapped."""
    ts, dec, args, _, _ = run_twin("geo", nsteps=2, dropout=False, conv1=True, ema_decay=DECAY)
    twin = run_twin("geo", nsteps=2, dropout=False, conv1=True, ema_decay=DECAY)[0]
    enc, feats = ts.enc, args[1]
    p_before, e_before = ts.enc_p.clone(), ts.enc_e.clone()
    assert not same_bits(p_before, e_before)
    sd = ts.ema_state_dict()
    assert [tuple(t.shape) for t in sd["encoder_params"]] == [tuple(p.shape) for p in ts.enc_params]
    fresh, _, _ = make_encoder(17)
    with torch.no_grad():
        fresh.conv1.weight.copy_(sd["encoder_params"][0])
        fresh.conv1.bias.copy_(sd["encoder_params"][1])
        want, raw_out = fresh(feats).clone(), enc(feats).clone()
    assert not same_bits(want, raw_out)
    with ts.ema_weights():
        assert same_bits(ts.enc_p, e_before) and same_bits(ts.enc_e, p_before)
        assert same_bits(enc.conv1.weight.detach(), sd["encoder_params"][0])
        with torch.no_grad():
            assert same_bits(enc(feats), want)
    assert same_bits(ts.enc_p, p_before) and same_bits(ts.enc_e, e_before)
    with torch.no_grad():
        assert same_bits(enc(feats), raw_out)
    loss, loss_twin = ts(*args).clone(), twin(*args).clone()
    assert same_bits(loss, loss_twin)
    for a, b, what in ((ts.flat_p, twin.flat_p, "p"), (ts.flat_e, twin.flat_e, "e"), (ts.enc_p, twin.enc_p, "conv1"),
                       (ts.enc_e, twin.enc_e, "conv1's average"), (ts.enc_m, twin.enc_m, "conv1's moment")):
        assert same_bits(a, b), what


# ------------------------------------------------------------------------------------------------ state
def test_state_round_trip_and_resume(det_off_after):
    name = "geo"
    ts, dec, args, log, _ = run_twin(name, nsteps=2, ema_decay=DECAY, ema_warmup=True)
    sd, opt = ts.ema_state_dict(), ts.state_dict()
    assert sd["decay"] == DECAY and sd["warmup"] is True and len(sd["params"]) == len(ts._adam_order())
    assert all(tuple(t.shape) == tuple(p.shape) for t, p in zip(sd["params"], ts._adam_order()))
    assert sd["params"][0].data_ptr() != ts._slot(ts.flat_e, ts._adam_order()[0]).data_ptr()       # copies
    weights = {k: v.detach().clone() for k, v in dec.state_dict().items() if k != "pos_encoder.pe"}
    ts(*args)
    after = (ts.flat_p.clone(), ts.flat_e.clone())
    # a fresh step from the checkpointed weights, optimizer state and average continues to the same bits
    dec2 = build_decoder(STEP_CASES[name][0], STEP_CASES[name][1], weights).train()
    ts2 = TrainStep(dec2, lr=4e-4, grad_clip=5.0, seed=11, deterministic=True, ema_decay=0.5)
    ts2.load_state_dict(opt)
    ts2.load_ema_state_dict(sd)
    assert ts2.ema_decay == DECAY and ts2.ema_warmup is True and ts2._ema_word.item() == np.float32(DECAY)
    back = ts2.ema_state_dict()
    assert all(same_bits(a, b) for a, b in zip(back["params"], sd["params"]))
    ts2(*args)
    assert same_bits(ts2.flat_p, after[0]) and same_bits(ts2.flat_e, after[1])
    # mismatches are refused
    with pytest.raises(IckError):
        ts2.load_ema_state_dict(dict(sd, params=sd["params"][:-1]))
    wrong = list(sd["params"])
    wrong[0] = torch.zeros(3, 3, device="cuda")
    with pytest.raises(IckError):
        ts2.load_ema_state_dict(dict(sd, params=wrong))
    with pytest.raises(IckError):
        ts2.load_ema_state_dict(dict(sd, encoder_params=[torch.zeros(1)]))


# ------------------------------------------------------------------------------------------------ the training script
@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_train_main_keeps_checkpoints_and_validates_on_the_average(tmp_path, fused, monkeypatch):
    from ick_amd import eval as ev, train as tr, utils as ut
    from ick_amd.datasets import CaptionDataset
    # main()'s own step / average and what it hands to validate(), kept for the run by hand below
    seen, real_validate = {}, tr.validate

    class Step(tr.TrainStep):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["owner"] = self

    class Ema(tr.TorchEma):
        def __init__(self, *a, **k):
            super().__init__(*a, **k)
            seen["owner"] = self

    def validate(loader, encoder, decoder, criterion, cfg, device, cider=None):
        seen["args"] = (loader, encoder, decoder, criterion, cfg, device)
        seen["weights"] = [p.detach().clone() for p in decoder.parameters() if p.requires_grad]
        return real_validate(loader, encoder, decoder, criterion, cfg, device, cider=cider)

    monkeypatch.setattr(tr, "TrainStep", Step)
    monkeypatch.setattr(tr, "TorchEma", Ema)
    monkeypatch.setattr(tr, "validate", validate)
    data_dir = str(tmp_path / "data")
    wm = synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    base = dict(variant="geo", data_dir=data_dir, data_name="toy", batch_size=8, workers=0, print_freq=1000, fused=fused,
                seed=3, out_dir=str(tmp_path))
    torch.manual_seed(0)
    hist = tr.main(tr.Config(epochs=2, ema_decay=0.8, ema_warmup=True, **base))
    assert len(hist) == 2 and all(math.isfinite(h[1]) for h in hist)
    # With ema_validate the reported loss EQUALS validate() run by hand inside main()'s own ema_weights() (fused:
    # TrainStep.ema_weights(); unfused: TorchEma.weights()), on main()'s own loader, modules and criterion
    owner = seen["owner"]
    assert isinstance(owner, Step if fused else Ema)
    with (owner.ema_weights() if fused else owner.weights()):
        by_hand = real_validate(*seen["args"])
        inside = [p.detach().clone() for p in seen["args"][2].parameters() if p.requires_grad]
    print("validation loss reported %.9g, by hand inside ema_weights() %.9g" % (hist[-1][1], by_hand))
    assert by_hand == hist[-1][1]
    assert all(torch.equal(a, b) for a, b in zip(seen["weights"], inside))              # main() validated these very bits
    ck = ut.load_checkpoint(str(tmp_path / "checkpoint_toy.pth.tar"), map_location="cuda")
    assert set(ck) == {"epoch", "epochs_since_improvement", "loss", "encoder", "decoder", "encoder_optimizer",
                       "decoder_optimizer", "decoder_ema"}
    ema = ck["decoder_ema"]
    dec, enc = ck["decoder"].cuda(), ck["encoder"].cuda()
    trained = [p for p in dec.parameters() if p.requires_grad]
    assert ema["decay"] == 0.8 and ema["warmup"] is True and len(ema["params"]) == len(trained)
    raw = [p.detach().clone() for p in trained]
    assert any(not torch.equal(a, b) for a, b in zip(raw, ema["params"]))                # the average lags the weights
    # the reported validation loss is validate() on the averaged weights
    crit = tr.make_criteria(wm["<pad>"])[1].cuda()
    dev = torch.device("cuda", torch.cuda.current_device())
    val = lambda: torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "VAL"), batch_size=8, shuffle=False)   # noqa: E731
    loss_raw = tr.validate(val(), enc, dec, crit, tr.Config(**base), dev)
    ut.load_ema_weights(dec, ema, encoder=enc)
    assert all(torch.equal(p.detach(), t) for p, t in zip(trained, ema["params"]))
    loss_avg = tr.validate(val(), enc, dec, crit, tr.Config(**base), dev)
    print("validation loss reported %.7f, on the average %.7f, on the raw weights %.7f" % (hist[-1][1], loss_avg, loss_raw))
    assert all(torch.equal(a, b) for a, b in zip(inside, ema["params"]))                 # ... which the checkpoint carries
    assert loss_avg == hist[-1][1] and ck["loss"] == hist[-1][1]                         # the same bits, the same loss
    assert abs(loss_raw - loss_avg) > 1e-4
    caps, seqs = ev.evaluate(enc.eval(), dec.eval(), torch.utils.data.DataLoader(CaptionDataset(data_dir, "toy", "TEST"),
                                                                                 batch_size=2, shuffle=False),
                             wm, max_caption_len=10, out_csv=str(tmp_path / "generated_captions.csv"))
    assert len(caps) == 4
    # resume restores the average.  The resumed epoch runs with a decay of 1 - 1e-6: its three steps move the average by
    # at most 3e-6 of its distance to the weights, so it must end where the checkpoint had it -- an average that was lost
    # would have restarted at the checkpoint's raw weights instead
    tr.main(tr.Config(epochs=3, ema_decay=0.999999, checkpoint=str(tmp_path / "checkpoint_toy.pth.tar"), **base))
    c2 = ut.load_checkpoint(str(tmp_path / "checkpoint_2_toy.pth.tar"), map_location="cuda")
    assert c2["epoch"] == 2 and len(c2["decoder_ema"]["params"]) == len(trained) and c2["decoder_ema"]["warmup"] is False
    moved = max((a - b).abs().max().item() for a, b in zip(c2["decoder_ema"]["params"], ema["params"]))
    lag = max((a - b).abs().max().item() for a, b in zip(raw, ema["params"]))
    print("resumed average moved %.3g, the checkpoint's average lagged its weights by %.3g" % (moved, lag))
    assert lag > 1e-4 and moved < 0.01 * lag
    # a default run keeps the seven keys
    (tmp_path / "plain").mkdir()
    tr.main(tr.Config(epochs=1, **dict(base, out_dir=str(tmp_path / "plain"))))
    c3 = ut.load_checkpoint(str(tmp_path / "plain" / "checkpoint_0_toy.pth.tar"), map_location="cuda")
    assert set(c3) == set(ck) - {"decoder_ema"}
