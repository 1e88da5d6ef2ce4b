"""Weight decay inside the fused Adam pass on the GPU:
  * ick_adam_step with decay alone on raw buckets, bit for bit against the same entry without it run on inputs prepared with the float32
    restatement (tests/weight_decay_ref.py), at every size where a kernel path begins or ends and for masks that cross
    them;
  * ick_adam_step_derive with decay over a real decoder's cover: the flat form's bits, and images of the updated parameters;
  * TrainStep(weight_decay=) against a twin without it (deterministic mode: bit for bit), and against the float64 oracle
    with torch.optim.AdamW / Adam(weight_decay=) over the same per-parameter groups;
  * the setters, lazy_update, the default step, the state round trip, SelfCriticalStep and the training script."""
import math

import numpy as np
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
from decode_ref import float64_default
from ick_amd.lib import OPT_WORDS, IckError
from ick_amd.training import DerivedWeights, TrainStep, default_decay_filter
from oracle import restatement as R
from test_bench_sizes_gpu import make_encoder
from test_ema_gpu import SENTINEL, SIZES, _images, bucket
from test_forward_gpu import build_decoder
from test_label_smoothing_gpu import STEP_CASES, _count_captures, compare_with_oracle, same_bits, step_args, step_case
from test_training_gpu import zero_dropout
from weight_decay_ref import adam_l2_step64, adamw_step64, clamped_grad32, coupled_grad32, decoupled_factor32, shrink32

pytestmark = pytest.mark.gpu

LR = 4e-4
WD = {True: 2.5, False: 0.1}          # decoupled: wd * lr = 1e-3; coupled: wd of order 0.1
FORMS = [True, False]                 # decoupled_weight_decay


@pytest.fixture()
def det_off_after():
    yield
    ops.set_deterministic(False)


def word(x):
    return torch.full((1,), x, device="cuda")


# ------------------------------------------------------------------------------------------------ the kernel alone
MASKS = ["ones", "zeros", "alternating", "last"]
MODES = ["plain", "words", "step1000", "no_tokens"]
SCHEDULE = dict(kind="cosine", warmup_steps=2, total_steps=9, min_lr_ratio=0.1)
DEN, CLIP, COEF = 7.0, 0.5, 0.25


def granule_mask(n, kind):
    """One byte per 64 floats of an n-float bucket; "last": only the last (for these sizes partial) granule."""
    gr = (n + 63) // 64
    m = torch.zeros(gr, dtype=torch.uint8)
    if kind == "ones":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "last":
        m[-1] = 1
    return m


def run_entry(bufs, offset, n, mode, step0, den, decay=None, clip=CLIP, coef=COEF, ema=False):
    """One optimizer launch over the n floats behind `offset` of the five buffers; -> the optimizer words (or None)."""
    view = [b[offset:offset + n] for b in bufs]
    counter = torch.full((1,), step0, device="cuda", dtype=torch.int32)
    rate, w = dict(lr=LR), None
    if mode == "words":
        w = torch.zeros(OPT_WORDS, device="cuda")
        w[0], w[3] = LR, coef
        rate = dict(words=w, schedule=SCHEDULE)
    kw = dict(ema=view[4], ema_decay_word=word(0.9)) if ema else {}
    ops.adam_update(*view[:4], 1, clip=clip, gscale=1.0, step_tensor=counter, gscale_den=torch.tensor([den], device="cuda"),
                    **rate, **kw, **(decay or {}))
    torch.cuda.synchronize()
    return w


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("mask_kind", MASKS)
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_kernel_has_the_plain_entries_bits_on_prepared_inputs(size, mask_kind, mode):
    """Everything here is bit-exact.  Decoupled: p, m, v are the plain entry's on a copy whose selected granules were
    multiplied by the restatement's float32 f (words mode: lr_t read back from words[4]).  Coupled: p, m, v are the plain
    entry's, run with clip = 0, a denominator of 1 and a coefficient of 1, on a copy whose gradient is the restatement's
    clamped gradient plus wd * p in the selected granules.  The written g is the plain entry's from the original inputs;
    wd = 0 is the plain entry; without tokens nothing is written; the sentinels stay.  "offset": the bucket starts one
    float behind a 16-byte boundary and the mask still counts from the bucket's start."""
    n, offset = (4096 + 3, 1) if size == "offset" else (size, 0)
    step0 = 999 if mode == "step1000" else 0
    den = 0.0 if mode == "no_tokens" else DEN
    ema = mode == "step1000"                       # (one mode also keeps the moving average: <kEma, kDecay> instantiations)
    mask = granule_mask(n, mask_kind)
    sel = mask.bool().repeat_interleave(64)[:n].numpy()
    mask_dev = mask.cuda()
    orig = bucket(n, offset)
    plain = bucket(n, offset)
    run_entry(plain, offset, n, mode, step0, den, ema=ema)          # the plain entry on the original inputs
    lo, hi = offset, offset + n
    for decoupled in FORMS:
        wd = WD[decoupled]
        mine = bucket(n, offset)
        decay = dict(decay_word=word(wd), decay_mask=mask_dev, decoupled=decoupled)
        w = run_entry(mine, offset, n, mode, step0, den, decay, ema=ema)
        assert all(float(b[hi:].min()) == SENTINEL == float(b[hi:].max()) for b in mine)
        assert offset == 0 or all(float(b[0]) == SENTINEL for b in mine)
        if mode == "no_tokens":
            assert all(same_bits(a, b) for a, b in zip(mine, orig)), decoupled
            continue
        assert same_bits(mine[1], plain[1]), ("g", decoupled)
        ref = bucket(n, offset)
        p0 = orig[0][lo:hi].cpu().numpy()
        if decoupled:
            lr_t = w[4].item() if mode == "words" else LR
            assert lr_t > 0
            ref[0][lo:hi] = torch.from_numpy(np.where(sel, shrink32(p0, decoupled_factor32(lr_t, wd)), p0)).cuda()
            run_entry(ref, offset, n, mode, step0, den, ema=ema)
        else:
            x = clamped_grad32(orig[1][lo:hi].cpu().numpy(), DEN, CLIP, coef=COEF if mode == "words" else None)
            assert np.array_equal(x.view(np.int32), plain[1][lo:hi].cpu().numpy().view(np.int32))      # the restatement's x
            ref[1][lo:hi] = torch.from_numpy(np.where(sel, coupled_grad32(x, p0, wd), x)).cuda()
            run_entry(ref, offset, n, mode, step0, 1.0, clip=0.0, coef=1.0, ema=ema)
        for k, what in ((0, "p"), (2, "m"), (3, "v")) + (((4, "e"),) if ema else ()):
            assert same_bits(mine[k], ref[k]), (what, decoupled, size, mask_kind, mode)
        if sel.any():
            assert not same_bits(mine[0], plain[0]), decoupled                      # the decay did something
        else:
            assert same_bits(mine[0], plain[0]) and same_bits(mine[2], plain[2])
        # wd = 0: the plain entry's bits
        zero = bucket(n, offset)
        run_entry(zero, offset, n, mode, step0, den, dict(decay, decay_word=word(0.0)), ema=ema)
        assert all(same_bits(a, b) for a, b in zip(zero, plain)), ("wd = 0", decoupled)


# ------------------------------------------------------------------------------------------------ the cover
@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
@pytest.mark.parametrize("ema", [False, True], ids=["no_ema", "ema"])
@pytest.mark.parametrize("rate", ["lr", "words"])
@pytest.mark.parametrize("variant,V", [("geo", 200), ("knowledge", 160)])
def test_derive_form_has_the_flat_forms_bits_and_images_of_the_new_parameters(variant, V, rate, ema, decoupled):
    dec = build_decoder(variant, V, synth.make_params(variant, V, 3)).train()
    kw = dict(max_grad_norm=1e9, lr_schedule=dict(kind="linear", warmup_steps=2, total_steps=20)) if rate == "words" else {}
    if ema:
        kw.update(ema_decay=0.9, ema_warmup=True)
    wd = WD[decoupled]
    ts = TrainStep(dec, lr=LR, grad_clip=5.0, weight_decay=wd, decoupled_weight_decay=decoupled, **kw)
    ts.derived = dw = DerivedWeights.build(ts)
    assert dw is not None and dw.n_blocks > 50
    dw.refresh()
    n = ts.n
    mask = ts._wd_mask
    assert mask.numel() == n // 64 and 0 < int(mask.sum()) < mask.numel()        # the step's own mask: a mixed selection
    gen = torch.Generator(device="cuda").manual_seed(1)
    used = torch.zeros(n, dtype=torch.bool, device="cuda")              # (the pads between the parameters stay zero)
    for p in ts.params:
        off = (p.data_ptr() - ts.flat_p.data_ptr()) // 4
        used[off:off + p.numel()] = True
    rnd = lambda: torch.randn(n, device="cuda", generator=gen) * used    # noqa: E731
    ts.flat_g[:n] = rnd() * 40.0                                         # some elements beyond the clamp (5 x 7 tokens)
    ts.flat_g[n], ts.flat_g[n + 1] = 3.5, 7.0
    ts.flat_m.copy_(rnd() * 0.01)
    ts.flat_v.copy_(rnd().abs() * 1e-3)
    state = [ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v] + ([ts.flat_e] if ema else [])
    if ema:
        ts.flat_e.copy_(ts.flat_p + rnd() * 0.01)
    ts.counter.fill_(4)
    start = [t.clone() for t in state]
    ts._adam()                                                                   # ick_adam_step_derive, decay != NULL
    torch.cuda.synchronize()
    mine = [t.clone() for t in state]
    images = {k: v.clone() for k, v in _images(dw).items()}
    # the flat form on copies
    flat = [t.clone() for t in start]
    words = dict(words=ts._words, schedule=ts._sched) if rate == "words" else dict(lr=LR)
    common = dict(clip=5.0, gscale=1.0, beta1=0.9, beta2=0.999, eps=1e-8, step_tensor=ts.counter,
                  gscale_den=ts.flat_g[n + 1:], decay_word=ts._wd_word, decay_mask=mask, decoupled=decoupled)
    avg = dict(ema=flat[4], ema_decay_word=ts._ema_word, ema_warmup=True) if ema else {}
    ops.adam_update(flat[0], flat[1][:n], flat[2], flat[3], 1, **common, **words, **avg)
    # ... and the flat form without decay, to see that the decay reached the selected granules and only those
    nodecay = [t.clone() for t in start]
    del common["decay_word"], common["decay_mask"], common["decoupled"]
    ops.adam_update(nodecay[0], nodecay[1][:n], nodecay[2], nodecay[3], 1, **common, **words)
    torch.cuda.synchronize()
    for a, b, what in zip(mine, flat, "pgmve"):
        assert same_bits(a[:n], b[:n]), (what, variant, rate)
    sel = mask.bool().repeat_interleave(64)
    assert same_bits(mine[0][~sel], nodecay[0][~sel]) and not same_bits(mine[0][sel], nodecay[0][sel])
    assert same_bits(mine[1][:n], nodecay[1][:n])                                 # the gradient stays without the term
    # every image is an image of the updated parameters
    dw.refresh()
    torch.cuda.synchronize()
    for k, v in _images(dw).items():
        assert same_bits(images[k], v), (variant, k)
    # pads between the parameters stay zero
    assert int((~used).sum()) > 0 and all(float(t[:n][~used].abs().max()) == 0.0 for t in mine)


# ------------------------------------------------------------------------------------------------ TrainStep against a twin
def build_step(name, conv1=False, dropout=True, deterministic=True, **kw):
    variant, V, P, cfg, batch, enc_out = step_case(name)
    dec = build_decoder(variant, V, P).train()
    if not dropout:
        zero_dropout(dec)
    args = step_args(variant, batch, enc_out)
    if conv1:
        enc, _, _ = make_encoder(17)
        kw.update(encoder=enc, train_conv1=True, encoder_lr=1e-3)
        args[1] = synth.make_feats(batch["captions"].shape[0], 17).cuda()
    return TrainStep(dec, lr=LR, grad_clip=5.0, seed=11, deterministic=deterministic, **kw), dec, args


def slots(ts, flat, enc_flat=None):
    out = {n: ts._slot(flat, p) for n, p in ts.dec.named_parameters() if id(p) in ts.grads}
    if enc_flat is not None:
        out.update({"encoder.conv1.weight": ts._enc_bucket.slot(enc_flat, ts.enc_params[0]),
                    "encoder.conv1.bias": ts._enc_bucket.slot(enc_flat, ts.enc_params[1])})
    return out


@pytest.mark.parametrize("conv1", [False, True], ids=["decoder", "with_conv1"])
@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
@pytest.mark.parametrize("name", ["geo", "knowledge"])
def test_one_step_against_a_twin_without_decay(name, decoupled, conv1, det_off_after):
    wd = WD[decoupled]
    kw = dict(encoder_weight_decay=wd) if conv1 else {}
    ts, dec, args = build_step(name, conv1=conv1, weight_decay=wd, decoupled_weight_decay=decoupled, **kw)
    twin, _, _ = build_step(name, conv1=conv1)
    assert same_bits(ts.flat_p, twin.flat_p)
    loss, loss0 = ts(*args).clone(), twin(*args).clone()
    assert ts.use_graph and same_bits(loss, loss0)
    chosen = set(ts.decayed_parameter_names())
    want = {n for n, p in dec.named_parameters() if id(p) in ts.grads and p.ndim >= 2}
    assert chosen == want | ({"encoder.conv1.weight"} if conv1 else set()) and want
    enc = (lambda t: (t.enc_p, t.enc_m, t.enc_v)) if conv1 else (lambda t: (None, None, None))      # noqa: E731
    for k, (mine, theirs) in enumerate(zip((ts.flat_p, ts.flat_m, ts.flat_v), (twin.flat_p, twin.flat_m, twin.flat_v))):
        a, b = slots(ts, mine, enc(ts)[k]), slots(twin, theirs, enc(twin)[k])
        assert set(a) == set(b) and chosen <= set(a)
        for n in a:
            same = same_bits(a[n], b[n])
            if n not in chosen or (decoupled and k > 0):
                assert same, ("pmv"[k], n)             # unselected: the twin's bits; decoupled: all moments are the twin's
            elif k == 0:
                assert not same, ("p", n)              # every selected parameter moved
    assert same_bits(ts.flat_g, twin.flat_g)           # the gradient stays without the term


def test_without_the_cover_and_inside_ema_weights(monkeypatch, det_off_after):
    """ICK_ADAM_DERIVE=0 (the flat entry inside the step) ends on the cover's bits, and ema_weights() around a decayed step
    shows the average and gives the training bits back: the next step equals the twin's that never swapped."""
    kw = dict(weight_decay=WD[True], ema_decay=0.9)
    runs = {}
    for derive in ("1", "0"):
        monkeypatch.setenv("ICK_ADAM_DERIVE", derive)
        ts, dec, args = build_step("knowledge", **kw)
        ts(*args)
        ts(*args)
        assert ts.use_graph and (ts.derived is not None) == (derive == "1")
        runs[derive] = ts
    a, b = runs["1"], runs["0"]
    for x, y, what in ((a.flat_p, b.flat_p, "p"), (a.flat_m, b.flat_m, "m"), (a.flat_v, b.flat_v, "v"), (a.flat_e, b.flat_e, "e")):
        assert same_bits(x, y), what
    p_before, e_before = a.flat_p.clone(), a.flat_e.clone()
    with a.ema_weights():
        assert same_bits(a.flat_p, e_before) and same_bits(a.flat_e, p_before)
        with pytest.raises(IckError, match="ema_weights"):
            a(*args)
    assert same_bits(a.flat_p, p_before) and same_bits(a.flat_e, e_before)
    a(*args)
    b(*args)
    assert same_bits(a.flat_p, b.flat_p) and same_bits(a.flat_e, b.flat_e)


def test_weight_decay_none_is_todays_step(det_off_after):
    """Nothing allocated, every launch the plain instantiation's (no option pointer given), the twin's bits over four steps, and the setters refuse."""
    launched = []
    real = ops.L.load

    class Spy:
        def __getattr__(self, name):
            fn = getattr(real(), name)
            if not name.startswith("ick_adam"):
                return fn

            def record(*a):
                launched.append((name, a))
                return fn(*a)
            return record

    ts, dec, args = build_step("geo", weight_decay=None)
    twin, _, _ = build_step("geo")
    assert ts.weight_decay is None and ts._wd_word is None and ts._wd_mask is None and ts._enc_wd_word is None
    assert ts.decayed_parameter_names() == []
    ops.L.load = Spy
    try:
        losses = [ts(*args).clone() for _ in range(4)]
    finally:
        ops.L.load = real
    assert launched and {name for name, _ in launched} == \
        {"ick_adam_step_derive" if ts.derived is not None else "ick_adam_step"}
    for name, a in launched:                 # every launch selects <kOpt, kEma, kDecay> = <0, 0, 0>: the plain instantiation
        over = 2 if name == "ick_adam_step_derive" else 0
        e, words, (decay, mask, granules) = a[4], a[9 + over], a[19 + over:22 + over]
        assert e is None and words is None and decay is None and mask is None and granules == 0, (name, a)
    losses0 = [twin(*args).clone() for _ in range(4)]
    assert all(same_bits(a, b) for a, b in zip(losses, losses0))
    assert same_bits(ts.flat_p, twin.flat_p) and same_bits(ts.flat_m, twin.flat_m) and same_bits(ts.flat_v, twin.flat_v)
    sd = ts.state_dict()
    assert len(sd["param_groups"]) == 1 and sd["param_groups"][0]["weight_decay"] == 0
    assert type(ts.as_torch_optimizer()) is torch.optim.Adam
    for call in (lambda: ts.set_weight_decay(0.1), lambda: ts.set_encoder_weight_decay(0.1)):
        with pytest.raises(IckError):
            call()
    ts.set_weight_decay(None)                                            # (off stays off)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(IckError):
            TrainStep(dec, weight_decay=bad)
    with pytest.raises(IckError):
        TrainStep(dec, encoder_weight_decay=0.1)                         # needs train_conv1
    ts2 = TrainStep(dec, weight_decay=0.5)
    with pytest.raises(IckError):
        ts2.set_weight_decay(None)                                       # ... and on stays on
    with pytest.raises(IckError):
        ts2.set_weight_decay(-1.0)
    assert ts2.weight_decay == 0.5 and ts2._wd_word.item() == 0.5


def test_custom_filter_selects_by_name():
    variant, V, P, cfg, batch, enc_out = step_case("geo")
    dec = build_decoder(variant, V, P).train()
    seen = []
    ts = TrainStep(dec, weight_decay=0.1, decay_filter=lambda n, p: (seen.append((n, p)), n.endswith("bias"))[1])
    names = ts.decayed_parameter_names()
    assert names and all(n.endswith("bias") for n in names)
    assert len(seen) == len(ts.params) and all(isinstance(n, str) and dict(dec.named_parameters())[n] is p for n, p in seen)
    chosen = [p for n, p in dec.named_parameters() if n in set(names)]
    assert torch.equal(ts._wd_mask, ts._dec_bucket.decay_mask(chosen))
    assert default_decay_filter("x", torch.zeros(2, 2)) and not default_decay_filter("x", torch.zeros(2))


# ------------------------------------------------------------------------------------------------ against the float64 oracle
# wd for the oracle comparison.  The condition below (the oracle with decay and the oracle without differ by at least 20 x
# the tolerance on every selected tensor) decides the size.  Decoupled: three steps shrink an element by 3 * wd * lr * |p|,
# and the selected tensor with the smallest weights has max |p| of about 0.07, so wd * lr = 1e-3 moves it by 2e-4, 1.3 x
# the parameter tolerance of 1.5e-4 (measured on the CPU oracle); wd * lr = 3e-2 moves it by 4e-3 (Adam's own steps
# take part of the shrink back).  Coupled: wd = 0.1.
ORACLE_WD = {True: 75.0, False: 0.1}
ORACLE_STEPS = 3
TOL_P_ANY, TOL_P_WELL, TOL_M, TOL_V = 3 * 8.5e-4, 3 * 5e-5, 2e-3, 4e-3      # tests/test_conv1_train_gpu.py, three steps
_ORACLE = {}


def oracle_steps(name, decoupled):
    """Three optimizer steps of the reference sequence on the CPU oracle in float64, with torch.optim.AdamW / Adam over
    one param group per parameter (decoupled None: plain Adam, no decay).  -> the first step's loss and gradients, the
    starting parameters, and after the last step the parameters and the optimizer.  Once per case."""
    key = (name, decoupled)
    if key in _ORACLE:
        return _ORACLE[key]
    variant, V, P, cfg, batch, enc_out = step_case(name)
    Pr = {k: v.double().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
    if cfg.has_facts:
        Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
    names = [k for k in Pr if not k.startswith("fact_encoder.")]
    start = {k: Pr[k].detach().clone() for k in names}
    selected = [k for k in names if default_decay_filter(k, Pr[k])]
    wd = 0.0 if decoupled is None else ORACLE_WD[decoupled]
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([dict(params=[Pr[k]], weight_decay=wd if k in selected else 0.0) for k in names], lr=LR, weight_decay=0.0)
    out = {}
    for s in range(ORACLE_STEPS):
        opt.zero_grad()
        with float64_default():          # (the oracle allocates its tables and masks with the default dtype)
            scores, caps, dl = R.forward(cfg, Pr, batch["captions"], enc_out.double(), batch["caption_masks"],
                                         batch["caption_lengths"], batch["entities"], batch.get("facts"))
            loss = R.packed_ce_loss(cfg, scores, caps, dl)
            loss.backward()
        if s == 0:
            out["loss"] = loss.item()
            out["grads"] = {k: Pr[k].grad.clone() for k in names}
        for k in names:
            Pr[k].grad.clamp_(-5.0, 5.0)
        opt.step()
    out.update(names=names, selected=selected, start=start, params=Pr, opt=opt, wd=wd)
    _ORACLE[key] = out
    return out


def check_condition(name, decoupled):
    """The tolerance cannot hide a missing decay: from the oracle alone, with and without decay, on every selected tensor.
    Decoupled: the parameters differ by at least 20 x their (well-conditioned) tolerance.  Coupled: both moments, which the
    term wd * p enters directly, differ by at least 20 x their tolerances; the parameters cannot -- Adam moves an element
    by at most about lr per step, so two runs differ by at most 2 * 3 * lr = 2.4e-3 = 16 x the tolerance whatever wd is --
    and are held to half of that bound.  Unselected tensors see the decay only through the later steps' gradients."""
    with_, without = oracle_steps(name, decoupled), oracle_steps(name, None)
    assert with_["selected"] and len(with_["selected"]) < len(with_["names"])
    worst = {}
    for k in with_["selected"]:
        a, b = with_["params"][k], without["params"][k]
        sa, sb = with_["opt"].state[a], without["opt"].state[b]
        dp = (a - b).abs().max().item()
        dm = ((sa["exp_avg"] - sb["exp_avg"]).abs().max() / sb["exp_avg"].abs().max()).item()
        dv = ((sa["exp_avg_sq"] - sb["exp_avg_sq"]).abs().max() / sb["exp_avg_sq"].abs().max()).item()
        for what, d in (("p", dp), ("m", dm), ("v", dv)):
            worst[what] = min(worst.get(what, (math.inf, None)), (d, k))
        if decoupled:
            assert dp >= 20 * TOL_P_WELL, (k, dp)
        else:
            assert dm >= 20 * TOL_M and dv >= 20 * TOL_V, (k, dm, dv)
            assert dp >= 0.5 * 2 * ORACLE_STEPS * LR, (k, dp)
    print("%s %s: smallest difference over the selected tensors, with against without decay:" %
          (name, "decoupled" if decoupled else "coupled"), worst)


@pytest.mark.parametrize("head", ["packed_head", "no_packed_head"])
@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
@pytest.mark.parametrize("name", ["geo", "knowledge"])
def test_three_steps_match_the_oracle(name, decoupled, head, gemm_split, monkeypatch):
    """Loss and every gradient of step 1 to compare_with_oracle's bounds (tests/test_grad_norm_gpu.py's one-step
    comparison), then parameters and moments after three steps to tests/test_conv1_train_gpu.py's three-step bounds:
    any element within 3 * 8.5e-4, well-conditioned elements within 3 * 5e-5 (at least 98 % of the elements whose first
    Adam input is at least 1e-6 must be: ours within 5 % of the oracle's), exp_avg within 2e-3 and exp_avg_sq within 4e-3
    of their maxima, with that test's allowance for ReLU units that flip (at most two hidden units of a linear1, in at
    most two tensors).  The Adam input is the clamped gradient, plus wd * p in the coupled form."""
    if head == "no_packed_head":
        monkeypatch.setenv("ICK_NO_PACKED_HEAD", "1")
    check_condition(name, decoupled)
    ref = oracle_steps(name, decoupled)
    wd = ORACLE_WD[decoupled]
    variant, V, P, cfg, batch, enc_out = step_case(name)
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=LR, grad_clip=5.0, weight_decay=wd, decoupled_weight_decay=decoupled)
    assert ts.packed_head == (head == "packed_head")
    args = step_args(variant, batch, enc_out)
    named = dict(dec.named_parameters())
    assert sorted(ts.decayed_parameter_names()) == sorted(ref["selected"])
    loss = ts(*args)
    assert ts.use_graph, "hipGraph capture failed: the captured step was not exercised"
    compare_with_oracle(ts, dec, loss.item(), ref["loss"], {k: g.float() for k, g in ref["grads"].items()})
    g1 = {k: ts.grads[id(named[k])].detach().cpu().double().clone() for k in ref["names"]}
    for _ in range(ORACLE_STEPS - 1):
        ts(*args)
    sd = ts.state_dict()
    assert [g["weight_decay"] for g in sd["param_groups"]] == \
        [wd if id(p) in {id(named[k]) for k in ref["selected"]} else 0.0 for p in ts._adam_order()]
    order = {id(p): i for i, p in enumerate(ts._adam_order())}
    worst, units, flipped = {}, {}, 0
    for k in ref["names"]:
        pr = ref["params"][k]
        st_ref, st = ref["opt"].state[pr], sd["state"][order[id(named[k])]]
        assert float(st["step"]) == float(st_ref["step"]) == float(ORACLE_STEPS)
        diff = (named[k].detach().cpu().double() - pr.detach()).abs()
        term = wd * ref["start"][k] if (k in ref["selected"] and not decoupled) else 0.0
        aref = ref["grads"][k].clamp(-5.0, 5.0) + term               # the first Adam input
        big = aref.abs() >= 1e-6
        well = big & ((g1[k].view(aref.shape) + term - aref).abs() <= 0.05 * aref.abs())
        keep = torch.ones(diff.shape[0], dtype=torch.bool)
        if k.endswith("linear1.bias") and k[:-4] in units:      # the units set aside in this Linear's weight: its bias too
            keep[units[k[:-4]]] = False
            flipped += 1
        if k.endswith(("linear1.weight", "linear1.bias")) and well.any() and (diff * well).max().item() >= TOL_P_WELL:
            rows = (diff * well).view(diff.shape[0], -1).max(dim=1).values
            bad = rows.topk(2).indices[rows.topk(2).values >= TOL_P_WELL]
            flipped += bool(keep.all())
            keep[bad] = False
            units[k.rsplit(".", 1)[0] + "."] = bad
            print("set aside as flipped ReLU units:", k, bad.tolist(), rows[bad].tolist())
        diff, well = diff[keep], well[keep]
        for mk, tol in (("exp_avg", TOL_M), ("exp_avg_sq", TOL_V)):
            mref = st_ref[mk]
            err = (st[mk].cpu().double() - mref)[keep].abs().max().item() / max(1e-12, mref.abs().max().item())
            worst[mk] = max(worst.get(mk, (0, None)), (err, k))
            assert err < tol, (mk, k, err)
        assert diff.max().item() <= TOL_P_ANY, ("parameter (any element)", k, diff.max().item())
        if big.any():
            assert well.sum().item() >= 0.98 * big[keep].sum().item(), ("too few well-conditioned elements", k)
        if well.any():
            err = diff[well].max().item()
            worst["param"] = max(worst.get("param", (0, None)), (err, k))
            assert err < TOL_P_WELL, ("parameter", k, err)
    assert flipped <= 2, "more than two tensors with flipped ReLU units"
    print("%s %s after three steps, worst" % (name, "decoupled" if decoupled else "coupled"), worst)


# ------------------------------------------------------------------------------------------------ graphs, lazy update
def test_set_weight_decay_replays_the_captured_graphs(det_off_after):
    """After one step, set_weight_decay writes the device word only: no capture, the same graphs, and the next update is
    the one a twin that had the new value from the start makes from the same state (deterministic mode: bit for bit) --
    and not the one under the old value."""
    ts, dec, args = build_step("geo", weight_decay=2.5)
    old, _, _ = build_step("geo", weight_decay=2.5)
    ts(*args)
    old(*args)
    assert same_bits(ts.flat_p, old.flat_p)
    graphs = dict(ts._graphs)
    calls = _count_captures(ts)
    ts.set_weight_decay(25.0)
    assert ts.weight_decay == 25.0 and ts._wd_word.item() == 25.0
    ts(*args)
    old(*args)
    assert ts._graphs == graphs and not calls and ts.use_graph
    assert not same_bits(ts.flat_p, old.flat_p)
    # the decoupled update from the same state: the shrunk copy under the new value through the plain entry
    fresh, _, _ = build_step("geo", weight_decay=2.5)
    fresh(*args)
    fresh.set_weight_decay(25.0)
    fresh._graphs.clear()                                                 # a fresh capture reads the same word
    fresh(*args)
    assert same_bits(ts.flat_p, fresh.flat_p) and same_bits(ts.flat_m, fresh.flat_m)
    sel = ts._wd_mask.bool().repeat_interleave(64)
    ratio = (ts.flat_p[sel] - old.flat_p[sel]).abs().max().item()
    assert ratio > 0.5 * (25.0 - 2.5) * LR * old.flat_p[sel].abs().max().item()       # the new factor reached the weights


def test_lazy_update_applies_the_decay_with_the_deferred_update():
    """tests/test_adam_derive_gpu.py's lazy test with weight decay, to its tolerances (lazy_update needs the two-stream
    step, whose float atomics are unordered: no bit comparison with the eager twin)."""
    variant, B, L, K, V, seed = "geo", 6, 9, 6, 160, 13
    P = synth.make_params(variant, V, seed)
    enc, _, _ = make_encoder(seed)
    batches = []
    for s_ in (seed, seed + 1):
        b = synth.make_batch(variant, B, L, K, V, 0, s_)
        batches.append([b["captions"].cuda(), synth.make_feats(B, s_).cuda(), b["caption_masks"].cuda(),
                        b["caption_lengths"].cuda(), b["entities"]])

    def run(lazy, wd):
        dec = zero_dropout(build_decoder(variant, V, P).train())
        ts = TrainStep(dec, lr=LR, grad_clip=5.0, encoder=enc, lazy_update=lazy, weight_decay=wd, deterministic=False)
        losses = [ts(*batches[i % 2]).item() for i in range(5)]
        assert ts.use_graph and ts.derived is not None and ts._pending == lazy
        assert int(ts.counter.item()) == (4 if lazy else 5)
        ts.set_weight_decay(wd)                                           # flushes first
        assert not ts._pending and int(ts.counter.item()) == 5
        return ts, losses

    ts1, l1 = run(True, 25.0)
    ts0, l0 = run(False, 25.0)
    plain, _ = run(False, 0.0)
    for a, b_ in zip(l1, l0):
        assert abs(a - b_) < 2e-4 * max(1.0, abs(b_)), (l1, l0)
    assert (ts1.flat_p - ts0.flat_p).abs().max().item() <= 5 * LR + 1e-6
    assert ((ts1.flat_p - ts0.flat_p).abs() > 1e-4).float().mean().item() < 0.02
    # five decayed updates shrink a weight by 1 - (1 - 25 * 4e-4)^5 = 4.9 %: the largest selected weight of the run without
    # decay (about 0.13) predicts the distance between the two; half of it is asked for, and it lies beyond the
    # lazy-against-eager tolerance above, so that tolerance cannot hide a deferred update that forgot the decay
    sel = ts1._wd_mask.bool().repeat_interleave(64)
    predicted = (1 - (1 - 25.0 * LR) ** 5) * plain.flat_p[sel].abs().max().item()
    assert 0.5 * predicted > 5 * LR + 1e-6
    assert (ts1.flat_p[sel] - plain.flat_p[sel]).abs().max().item() > 0.5 * predicted


def test_with_clip_schedule_and_ema_together(det_off_after):
    """max_grad_norm + lr_schedule + ema_decay + weight_decay: unselected parameters, the norm and the rate are the twin's
    without decay after one step; over three steps the decoupled factor follows the scheduled rate (lr_now)."""
    kw = dict(max_grad_norm=0.5, lr_schedule=dict(kind="cosine", warmup_steps=2, total_steps=8, min_lr_ratio=0.1),
              ema_decay=0.9)
    ts, dec, args = build_step("knowledge", weight_decay=25.0, **kw)
    twin, _, _ = build_step("knowledge", **kw)
    ts(*args)
    twin(*args)
    sel = ts._wd_mask.bool().repeat_interleave(64)
    assert same_bits(ts.flat_p[~sel], twin.flat_p[~sel]) and not same_bits(ts.flat_p[sel], twin.flat_p[sel])
    assert same_bits(ts.flat_m, twin.flat_m) and same_bits(ts.flat_v, twin.flat_v) and same_bits(ts._words, twin._words)
    assert same_bits(ts.flat_e[~sel], twin.flat_e[~sel]) and not same_bits(ts.flat_e[sel], twin.flat_e[sel])
    assert ts.clip_coef.item() < 1.0
    # step 3 by hand from the state after step 2: shrink by the float32 f at the scheduled rate, then the plain words entry
    ts(*args)
    before = [t.clone() for t in (ts.flat_p, ts.flat_m, ts.flat_v, ts.flat_e)]
    ts(*args)
    lr_t = ts.lr_now.item()
    assert 0 < lr_t < np.float32(LR)                                         # (the cosine has left the base rate)
    p0 = before[0].cpu().numpy()
    ref_p = torch.from_numpy(np.where(sel.cpu().numpy(), shrink32(p0, decoupled_factor32(lr_t, 25.0)), p0)).cuda()
    # ts.flat_g holds the clamped gradient of step 3 (what Adam consumed): feed it back with no scale, clip or coefficient
    w = ts._words.clone()
    w[3] = 1.0
    counter = ts.counter - 1
    ops.adam_update(ref_p, ts.flat_g[:ts.n].clone(), before[1], before[2], 1, words=w, schedule=ts._sched, clip=0.0,
                    gscale=1.0, step_tensor=counter, ema=before[3], ema_decay_word=ts._ema_word)
    assert same_bits(ref_p, ts.flat_p) and same_bits(before[1], ts.flat_m) and same_bits(before[3], ts.flat_e)


# ------------------------------------------------------------------------------------------------ state
@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
def test_state_round_trip_and_resume_across_decay_on_and_off(decoupled, det_off_after):
    name, wd = "geo", ORACLE_WD[decoupled]
    ts, dec, args = build_step(name, weight_decay=wd, decoupled_weight_decay=decoupled)
    ts(*args)
    ts(*args)
    sd = ts.state_dict()
    order = ts._adam_order()
    chosen = {id(p) for n, p in dec.named_parameters() if n in set(ts.decayed_parameter_names())}
    assert [g["params"] for g in sd["param_groups"]] == [[i] for i in range(len(order))]
    assert [g["weight_decay"] for g in sd["param_groups"]] == [wd if id(p) in chosen else 0.0 for p in order]
    assert all(g["decoupled_weight_decay"] is decoupled and g["lr"] == LR for g in sd["param_groups"])
    opt = ts.as_torch_optimizer()
    assert type(opt) is (torch.optim.AdamW if decoupled else torch.optim.Adam)
    assert opt.state_dict()["param_groups"] == sd["param_groups"]
    weights = {k: v.detach().clone() for k, v in dec.state_dict().items() if k != "pos_encoder.pe"}
    ts(*args)
    after = (ts.flat_p.clone(), ts.flat_m.clone())
    variant, V = STEP_CASES[name][0], STEP_CASES[name][1]
    # a fresh step with decay, loaded from that state (whose decay values it ignores: its own value holds)
    for stored in (sd, dict(sd, param_groups=[dict(g, weight_decay=123.0) for g in sd["param_groups"]])):
        ts2 = TrainStep(build_decoder(variant, V, weights).train(), lr=LR, grad_clip=5.0, seed=11, deterministic=True,
                        weight_decay=wd, decoupled_weight_decay=decoupled)
        ts2.load_state_dict(stored)
        assert ts2.weight_decay == wd and ts2._wd_word.item() == np.float32(wd)
        ts2(*args)
        assert same_bits(ts2.flat_p, after[0]) and same_bits(ts2.flat_m, after[1])
    # decay on -> off: a step without decay loads the per-parameter layout and continues as a plain step from there
    off = TrainStep(build_decoder(variant, V, weights).train(), lr=LR, grad_clip=5.0, seed=11, deterministic=True)
    off.load_state_dict(sd)
    one_group = off.state_dict()
    assert len(one_group["param_groups"]) == 1 and one_group["param_groups"][0]["weight_decay"] == 0
    assert all(torch.equal(one_group["state"][i]["exp_avg"], sd["state"][i]["exp_avg"]) for i in range(len(order)))
    off(*args)
    assert int(off.counter.item()) == 3 and not same_bits(off.flat_p, after[0])
    # decay off -> on: the one-group layout loads into a step with decay and continues to the decayed run's bits
    on = TrainStep(build_decoder(variant, V, weights).train(), lr=LR, grad_clip=5.0, seed=11, deterministic=True,
                   weight_decay=wd, decoupled_weight_decay=decoupled)
    on.load_state_dict(one_group)
    on(*args)
    assert same_bits(on.flat_p, after[0]) and same_bits(on.flat_m, after[1])


@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
def test_torch_optimizer_steps_like_the_float64_restatement(decoupled, det_off_after):
    """as_torch_optimizer() / as_torch_encoder_optimizer() carry the groups: one .step() of theirs on cloned CPU state in
    float64 equals the restatement's step (1e-12 of each tensor's largest magnitude)."""
    wd = WD[decoupled]
    ts, dec, args = build_step("geo", conv1=True, weight_decay=wd, encoder_weight_decay=wd,
                               decoupled_weight_decay=decoupled)
    ts(*args)
    ts(*args)
    names = set(ts.decayed_parameter_names())
    assert "encoder.conv1.weight" in names and "encoder.conv1.bias" not in names
    eopt = ts.as_torch_encoder_optimizer()
    assert type(eopt) is (torch.optim.AdamW if decoupled else torch.optim.Adam)
    assert [g["weight_decay"] for g in eopt.param_groups] == [wd, 0.0] and eopt.param_groups[0]["lr"] == 1e-3
    step = adamw_step64 if decoupled else adam_l2_step64
    for opt, lr, decayed in ((ts.as_torch_optimizer(), LR, {id(p) for n, p in dec.named_parameters() if n in names}),
                             (eopt, 1e-3, {id(ts.enc_params[0])})):
        sd = opt.state_dict()
        live = [p for g in opt.param_groups for p in g["params"]]
        clones = [torch.nn.Parameter(p.detach().cpu().double()) for p in live]
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        cpu = cls([dict(params=[c], weight_decay=g["weight_decay"]) for c, g in zip(clones, sd["param_groups"])], lr=lr,
                  weight_decay=0.0)
        cpu.load_state_dict(sd)
        gen = torch.Generator().manual_seed(5)
        before = [(c.detach().numpy().copy(), cpu.state[c]["exp_avg"].numpy().copy(),
                   cpu.state[c]["exp_avg_sq"].numpy().copy()) for c in clones]
        assert all(b[1].dtype == np.float64 for b in before)
        grads = [torch.randn(c.shape, generator=gen, dtype=torch.float64) * 0.01 for c in clones]
        for c, g in zip(clones, grads):
            c.grad = g.clone()
        cpu.step()
        for c, p, g, (p0, m0, v0) in zip(clones, live, grads, before):
            want = step(p0, g.numpy(), m0, v0, 3, lr, wd, decay=id(p) in decayed)
            for a, b in zip(want, (c.detach(), cpu.state[c]["exp_avg"], cpu.state[c]["exp_avg_sq"])):
                assert np.abs(a - b.numpy()).max() <= 1e-12 * max(np.abs(a).max(), 1e-30)


def test_self_critical_step_over_a_decayed_train_step():
    from ick_amd.scst import SelfCriticalStep
    from test_sample_gpu import make_case
    dec, cfg, P, ents, facts, enc = make_case("knowledge", 3, 5, 40, 4, 21, end_bias=1.5)
    ts = TrainStep(dec.train(), lr=LR, grad_clip=5.0, weight_decay=25.0)
    step = SelfCriticalStep(ts, lambda toks, img: (toks % 7).sum(1).double(), num_samples=3, baseline="mean", max_len=8,
                            seed=3)
    sel = ts._wd_mask.bool().repeat_interleave(64)
    norm0 = ts.flat_p[sel].double().norm().item()
    for _ in range(2):
        out = step(enc.cuda(), ents, facts.cuda())
        assert math.isfinite(out.loss.item())
    assert int(ts.counter.item()) == 2
    # two shrinks of 1 %; Adam's own two steps of at most lr per element cannot give that back (weights of about 0.1)
    assert ts.flat_p[sel].double().norm().item() < norm0 * (1 - 0.25 * 2 * 25.0 * LR)


# ------------------------------------------------------------------------------------------------ the training script
def _main_runner(tmp_path, decoupled, wd):
    from ick_amd import train as tr, utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=16, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam

    def run(out, fused, epochs, weight_decay=wd, checkpoint=None):
        (tmp_path / out).mkdir(exist_ok=True)
        torch.manual_seed(0)
        cfg = tr.Config(variant="geo", data_dir=data_dir, data_name="toy", epochs=epochs, batch_size=8, workers=0,
                        print_freq=1000, fused=fused, seed=3, out_dir=str(tmp_path / out), max_batches=2,
                        weight_decay=weight_decay, decoupled_weight_decay=decoupled, checkpoint=checkpoint)
        hist = tr.main(cfg)
        assert all(math.isfinite(h[0]) and math.isfinite(h[1]) for h in hist)
        path = str(tmp_path / out / ut.checkpoint_name("toy", epochs - 1))
        return path, ut.load_checkpoint(path, map_location="cuda")

    def check_groups(ck, steps, decayed=True):
        opt = ck["decoder_optimizer"]
        trained = [p for p in ck["decoder"].parameters() if p.requires_grad]
        if not decayed:
            assert type(opt) is torch.optim.Adam and len(opt.param_groups) == 1 and opt.param_groups[0]["weight_decay"] == 0
        else:
            assert type(opt) is cls and len(opt.param_groups) == len(trained)
            assert [g["params"][0] is p for g, p in zip(opt.param_groups, trained)] == [True] * len(trained)
            assert [g["weight_decay"] for g in opt.param_groups] == [wd if p.ndim >= 2 else 0.0 for p in trained]
            assert all(g["decoupled_weight_decay"] is decoupled for g in opt.param_groups)
        assert {int(float(st["step"])) for st in opt.state.values()} == {steps}

    return run, check_groups


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
@pytest.mark.parametrize("decoupled", FORMS, ids=["decoupled", "coupled"])
def test_train_main_checkpoints_load_into_the_other_path(tmp_path, decoupled, fused):
    """train.main with weight_decay: the saved decoder_optimizer is AdamW / Adam over one group per parameter with the
    decay on the ndim >= 2 ones, and the other path resumes from it and keeps the layout (two steps per epoch)."""
    run, check_groups = _main_runner(tmp_path, decoupled, 0.5)
    path, ck = run("first", fused, 1)
    check_groups(ck, 2)
    _, ck = run("resumed", not fused, 2, checkpoint=path)
    assert ck["epoch"] == 1
    check_groups(ck, 4)


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_train_main_resumes_across_decay_on_and_off(tmp_path, fused):
    """A checkpoint written with decay resumes in a run without it and the reverse: the moments carry over (the step
    count continues), the decay and the group layout come from the Config."""
    run, check_groups = _main_runner(tmp_path, True, 0.5)
    with_decay, ck = run("with", fused, 1)
    check_groups(ck, 2)
    without, ck = run("off", fused, 2, weight_decay=None, checkpoint=with_decay)
    check_groups(ck, 4, decayed=False)
    _, ck = run("on", fused, 3, checkpoint=without)
    check_groups(ck, 6)
