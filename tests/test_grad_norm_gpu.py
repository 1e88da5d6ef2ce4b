"""Global-norm gradient clipping and the device-side learning-rate schedule on the GPU:
  * ick_grad_sqnorm alone: exact on buckets whose every partial sum is an fp32 number, at the sizes where a path of the
    kernel begins or ends; against float64 on normal data; the same bits twice; the token-count rule; the coefficient;
  * ick_adam_step / ick_adam_step_derive with the words against the same entry without, bit for bit, with a coefficient
    of 1 and of 0.25; the scalar kernel against the float4 kernel on the same elements (csrc/adam.hip: one adam1, three
    kernels that address differently);
  * one TrainStep(max_grad_norm=) step against the CPU oracle with torch's clip_grad_norm_ and clamp_, in every product
    mode and both head modes; with a bound that never binds, the default step's bits;
  * the schedule inside captured steps: the rate of every step, no further capture, set_lr, resume from state_dict();
  * eager, lazy_update, SelfCriticalStep and train.main over the new arguments."""
import math
import types

import numpy as np
import pytest
import torch

import ick_amd.ops as ops
import ick_amd.synth as synth
from grad_norm_ref import clip_coef
from ick_amd.lib import OPT_WORDS, IckError
from ick_amd.training import DerivedWeights, TrainStep, lr_at
from oracle import restatement as R
from test_bench_sizes_gpu import make_encoder, reference_train_step_cached
from test_forward_gpu import build_decoder
from test_label_smoothing_gpu import (STEP_CASES, _count_captures, compare_with_oracle, run_steps, same_bits, step_args,
                                       step_case)
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu

W_BASE, W_MAX, W_NORM, W_COEF, W_LR, W_SQ = range(6)


def make_words(base_lr=0.0, max_norm=0.0, fill=0.0):
    w = torch.full((OPT_WORDS,), fill, device="cuda")
    w[W_BASE], w[W_MAX], w[W_COEF] = base_lr, max_norm, 1.0
    return w


@pytest.fixture()
def det_off_after():
    yield
    ops.set_deterministic(False)


# ------------------------------------------------------------------------------------------------ the norm kernel alone
def _plan_edge():
    wgs, per_wg, scratch = ops.grad_sqnorm_plan(1 << 30)
    assert wgs == scratch                               # a large bucket gets the most workgroups the plan has
    return wgs * per_wg                                 # above it the grid-stride loop makes a second trip


EXACT_SIZES = [1, 3, 4, 5, 255, 256, 1024, 4096 + 64, "edge-4", "edge+4100", (1 << 20) + 64]


@pytest.mark.parametrize("offset", [0, 4])
@pytest.mark.parametrize("n", EXACT_SIZES, ids=str)
def test_sqnorm_is_exact_on_exactly_summable_buckets(n, offset):
    """Values from {0, +-1, +-2} / 8: every square is a multiple of 1/64, and while 64 * sum < 2^24 every partial sum in
    any order is an fp32 number -- the kernel's sum of squares must be numpy's integer sum.  The norm word is one
    correctly rounded sqrtf of it (<= 2^-24 relative; 2^-23 allowed)."""
    if isinstance(n, str):
        n = _plan_edge() + int(n[4:])
    g = torch.Generator().manual_seed(n)
    ints = torch.randint(-2, 3, (n,), generator=g)
    exact64 = int((ints.long() ** 2).sum())
    assert 0 < exact64 < 2 ** 24 or n < 8
    buf = torch.zeros(n + offset + 4, device="cuda")
    buf[offset:offset + n] = (ints.float() * 0.125).cuda()
    buf[offset + n:] = 1000.0                            # what lies behind the bucket is not read
    if offset:
        buf[:offset] = 1000.0
    words = ops.grad_sqnorm(buf[offset:offset + n], make_words())
    wgs, per_wg, _ = ops.grad_sqnorm_plan(n)
    assert wgs == max(1, min(-(-(n // 4) // (per_wg // 4)), ops.grad_sqnorm_plan(n)[2]))
    w = words.cpu().double().numpy()
    assert w[W_SQ] * 64 == exact64, (n, w[W_SQ] * 64, exact64)
    assert abs(w[W_NORM] - math.sqrt(exact64 / 64)) <= 2.0 ** -23 * math.sqrt(exact64 / 64)
    assert w[W_COEF] == 1.0                             # max_norm word 0: the clip is off


def test_sqnorm_on_normal_data_and_bit_reproducible():
    """1e-5 relative: a chain of c fp32 additions of non-negative terms errs by at most c * 2^-24 relative; the kernel's
    chains (16 squares per thread and trip, an 8-level tree, 4 partials per thread and the tree again) stay far below the
    ~160 that bound allows."""
    n = 1_000_000
    g = torch.randn(n, generator=torch.Generator().manual_seed(5))
    ref = math.sqrt(float((g.double() ** 2).sum()))
    gd = g.cuda()
    runs = [ops.grad_sqnorm(gd, make_words()).clone() for _ in range(2)]
    got = runs[0][W_NORM].item()
    print("norm %.9g, float64 %.9g, relative error %.3g" % (got, ref, abs(got - ref) / ref))
    assert abs(got - ref) <= 1e-5 * ref
    assert same_bits(runs[0], runs[1])
    ops.set_deterministic(True)
    try:
        assert same_bits(ops.grad_sqnorm(gd, make_words()), runs[0])        # the same order in deterministic mode
    finally:
        ops.set_deterministic(False)


def test_sqnorm_without_tokens_leaves_the_words_alone():
    g = torch.ones(5000, device="cuda")
    words = make_words(4e-4, 1.0, fill=77.0)
    before = words.clone()
    for count in (0.0, -1.0, float("nan")):
        ops.grad_sqnorm(g, words, gscale_den=torch.tensor([count], device="cuda"))
        assert same_bits(words, before)
    ops.grad_sqnorm(g, words, gscale_den=torch.tensor([2.0], device="cuda"))
    assert words[W_SQ].item() == 5000.0 and words[W_BASE].item() == before[W_BASE].item()


@pytest.mark.parametrize("max_norm,den", [(0.5, None), (150.0, None), (3.0, 7.0), (1e-3, 7.0), (20.0, 7.0)])
def test_coef_word(max_norm, den):
    """coef is 1.0 exactly when the norm is within the bound, max_norm / (norm + 1e-6) otherwise: against float64 within
    1e-6 relative (the norm's rounding, one addition, one division in fp32)."""
    n = 10_001
    g = torch.randn(n, generator=torch.Generator().manual_seed(9))
    norm = math.sqrt(float((g.double() ** 2).sum())) / (den or 1.0)         # ~100, ~14.3 over 7 tokens
    words = ops.grad_sqnorm(g.cuda(), make_words(0.0, max_norm),
                            gscale_den=None if den is None else torch.tensor([den], device="cuda"))
    got_norm, got = words[W_NORM].item(), words[W_COEF].item()
    assert abs(got_norm - norm) <= 1e-5 * norm
    want = clip_coef(norm, max_norm)
    if norm <= max_norm:
        assert want == 1.0 and got == 1.0
    else:
        assert got < 1.0 and abs(got - want) <= 1e-6 * want


def test_wrappers_refuse_host_words():
    t = [torch.zeros(4096, device="cuda") for _ in range(4)]
    for bad in (4e-4, torch.zeros(OPT_WORDS), torch.zeros(OPT_WORDS - 1, device="cuda"),
                torch.zeros(OPT_WORDS, device="cuda", dtype=torch.float64)):
        with pytest.raises(IckError):
            ops.grad_sqnorm(t[0], bad)
        with pytest.raises(IckError):
            ops.adam_update(*t, 1, words=bad)
    with pytest.raises(IckError):        # the schedule's shape is checked by the library too
        ops.adam_update(*t, 1, words=make_words(4e-4), schedule=dict(kind="cosine", warmup_steps=3, total_steps=3))


# ------------------------------------------------------------------------------------------------ the Adam entries
def _bucket(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(n, device="cuda", generator=g) * 0.1, torch.randn(n, device="cuda", generator=g) * 400.0,
            torch.randn(n, device="cuda", generator=g) * 0.01, torch.rand(n, device="cuda", generator=g) * 1e-3]


@pytest.mark.parametrize("n", [1001, 4096 * 3 + 5, 8192])
@pytest.mark.parametrize("coef", [1.0, 0.25])
def test_adam_opt_is_adam_clamp_bit_for_bit(n, coef):
    """coef 1 and a constant schedule: the existing entry's bits.  coef 0.25 (a power of two: the product is exact):
    the existing entry called with gscale * 0.25."""
    counter = torch.full((1,), 4, device="cuda", dtype=torch.int32)
    den = torch.tensor([7.0], device="cuda")
    ref, mine = _bucket(n, n), _bucket(n, n)
    ops.adam_update(*ref, 1, 4e-4, clip=5.0, gscale=coef, beta1=0.9, beta2=0.999, eps=1e-8, step_tensor=counter,
                    gscale_den=den)
    words = make_words(4e-4, 1.0)
    words[W_COEF] = coef
    ops.adam_update(*mine, 1, words=words, clip=5.0, gscale=1.0, step_tensor=counter, gscale_den=den)
    for a, b, what in zip(mine, ref, "pgmv"):
        assert same_bits(a, b), what
    assert ref[1].abs().max().item() == 5.0                         # the clamp was exercised
    assert words[W_LR].item() == np.float32(4e-4)
    # without tokens nothing moves, the rate word included
    words[W_LR] = 0.0
    before = [t.clone() for t in mine]
    ops.adam_update(*mine, 1, words=words, step_tensor=counter, gscale_den=torch.zeros(1, device="cuda"))
    assert all(same_bits(a, b) for a, b in zip(mine, before)) and words[W_LR].item() == 0.0


@pytest.mark.parametrize("form", ["lr", "words"])
def test_scalar_kernel_is_float4_kernel_bit_for_bit(form):
    """The two flat kernels on the SAME elements (the other tests compare them on disjoint ranges only): one bucket of
    4099 floats in arrays that start one float past a 16-byte boundary, which sends all of it through adam_clamp_kernel,
    and the same contents aligned, where adam_clamp_vec4_kernel takes 4096 and the scalar kernel the tail of 3.  Plain
    rate, and the words form with coefficient 0.25 at step 5 of a cosine schedule."""
    n = 4099
    counter = torch.full((1,), 4, device="cuda", dtype=torch.int32)
    den = torch.tensor([7.0], device="cuda")
    vec, odd = _bucket(n, n), []
    for t in _bucket(n, n):
        buf = torch.empty(n + 1, device="cuda")
        buf[1:] = t
        odd.append(buf[1:])
    assert all(t.data_ptr() % 16 == 0 for t in vec) and all(t.data_ptr() % 16 == 4 for t in odd)
    assert all(same_bits(a, b) for a, b in zip(odd, vec))

    def rate():
        if form == "lr":
            return dict(lr=4e-4)
        words = make_words(4e-4, 1.0)
        words[W_COEF] = 0.25
        return dict(words=words, schedule=dict(kind="cosine", warmup_steps=3, total_steps=9))

    rates = rate(), rate()
    for arrays, r in zip((vec, odd), rates):
        ops.adam_update(*arrays, 1, clip=5.0, gscale=1.0, step_tensor=counter, gscale_den=den, **r)
    for a, b, what in zip(odd, vec, "pgmv"):
        assert same_bits(a, b), what
    assert vec[1].abs().max().item() == 5.0                         # the clamp was exercised
    if form == "words":
        assert same_bits(*(r["words"] for r in rates)) and 0.0 < rates[0]["words"][W_LR].item() < 4e-4


def _images(dw):
    wi = dw.owner
    out = {"pk": wi.flat["chain"], "pkb": wi.flat["chain_t"], "kvT": wi.chain_t[("kv", "T")], "wkv": wi.wkv, "bkv": wi.bkv,
           "wkv_ps": wi.kv_ps, "vocab_ps": wi.vocab_ps, "vocab_t_ps": wi.vocab_t_ps}
    if wi.pred_wt is not None:
        out["pred_wt"] = wi.pred_wt
    return out


@pytest.mark.parametrize("coef", [1.0, 0.25])
def test_adam_opt_derive_is_adam_clamp_derive_bit_for_bit(coef):
    """The bucket and cover of tests/test_adam_derive_gpu.py (knowledge, V = 1000): parameters, gradients, moments and
    every image."""
    variant, V = "knowledge", 1000
    dec = build_decoder(variant, V, synth.make_params(variant, V, 3)).train()
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0)
    ts.derived = dw = DerivedWeights.build(ts)
    assert dw is not None and dw.n_blocks > 100
    dw.refresh()
    n = ts.n
    g = torch.Generator(device="cuda").manual_seed(1)
    ts.flat_g[:n] = torch.randn(n, device="cuda", generator=g) * 400.0
    ts.flat_g[n], ts.flat_g[n + 1] = 3.5, 7.0
    ts.flat_m.copy_(torch.randn(n, device="cuda", generator=g) * 0.01)
    ts.flat_v.copy_(torch.rand(n, device="cuda", generator=g) * 1e-3)
    ts.counter.fill_(4)
    den = ts.flat_g[n + 1:].clone()
    images0 = {k: v.clone() for k, v in _images(dw).items()}
    start = [t.clone() for t in (ts.flat_p, ts.flat_g, ts.flat_m, ts.flat_v)]
    ref = [t.clone() for t in start]
    ops.adam_update(*ref, 1, 4e-4, cover=dw, clip=5.0, gscale=coef, beta1=0.9, beta2=0.999, eps=1e-8,
                    step_tensor=ts.counter, gscale_den=den)
    ref_images = {k: v.clone() for k, v in _images(dw).items()}
    for k, v in _images(dw).items():                    # back to the images of the weights before the update
        v.copy_(images0[k])
    mine = [t.clone() for t in start]
    words = make_words(4e-4, 1.0)
    words[W_COEF] = coef
    ops.adam_update(*mine, 1, words=words, cover=dw, clip=5.0, gscale=1.0, step_tensor=ts.counter, gscale_den=den)
    for a, b, what in zip(mine, ref, "pgmv"):
        assert same_bits(a[:n], b[:n]), what
    assert not torch.equal(mine[0], start[0]) and words[W_LR].item() == np.float32(4e-4)
    for k, v in _images(dw).items():
        assert same_bits(v, ref_images[k]) and not same_bits(v, images0[k]), k


@pytest.mark.parametrize("kind", ["constant", "inverse_sqrt", "cosine", "linear"])
def test_adam_opt_rate_word_follows_the_schedule(kind):
    """The rate the kOpt instantiation reports over the steps 1 .. N + 3 of each kind: 1e-6 relative (a few fp32 roundings) plus
    1e-6 * lr absolute (the cosine near its zero)."""
    sch = dict(kind=kind, warmup_steps=3, total_steps=9, min_lr_ratio=0.1)
    t4 = [torch.zeros(256, device="cuda") for _ in range(4)]
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    words = make_words(4e-4)
    for t in range(1, 13):
        ops.adam_update(*t4, 1, words=words, schedule=sch, step_tensor=counter)
        ops.counter_add(counter, 1)
        want = lr_at(t, float(np.float32(4e-4)), sch)
        assert abs(words[W_LR].item() - want) <= 1e-6 * want + 1e-6 * 4e-4, (kind, t)


# ------------------------------------------------------------------------------------------------ one step vs the oracle
CASES = dict(STEP_CASES, news=("news", 40, 4))
del CASES["geo_aligned"]


_ORACLE = {}


def oracle_case(name):
    """(variant, V, P, batch, enc_out, loss, the oracle's gradients before any clip, their global norm), once per case."""
    if name not in _ORACLE:
        _ORACLE[name] = _oracle_case(name)
    return _ORACLE[name]


def _oracle_case(name):
    variant, V, Fn = CASES[name]
    Bs, L, K, seed = 4, 8, 5, 17
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    batch = synth.make_batch(variant, Bs, L, K, V, Fn, seed)
    enc_out = synth.make_enc_out(Bs, seed)
    loss, grads, _ = reference_train_step_cached(("grad_norm", name), cfg, P, batch, enc_out)
    holders = [torch.nn.Parameter(torch.zeros_like(g)) for g in grads.values()]
    for h, g in zip(holders, grads.values()):
        h.grad = g.clone()
    norm = torch.nn.utils.clip_grad_norm_(holders, 1e30, norm_type=2).item()      # torch's own norm, nothing clipped
    return variant, V, P, batch, enc_out, loss, grads, norm


@pytest.mark.parametrize("head", ["packed_head", "no_packed_head"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_clipped_train_step_matches_oracle(name, head, gemm_split, monkeypatch):
    """max_grad_norm = half the ORACLE's norm of this step, so the clip binds: the norm word, the written-back gradients
    and the first moment against the oracle's gradients after torch's clip_grad_norm_ and clamp_(+-5).  (Not the
    parameters: Adam's first update is lr * g / |g|, which no clip changes.)"""
    if head == "no_packed_head":
        monkeypatch.setenv("ICK_NO_PACKED_HEAD", "1")
    variant, V, P, batch, enc_out, loss_ref, grads, norm_ref = oracle_case(name)
    m = 0.5 * norm_ref
    holders = {k: torch.nn.Parameter(torch.zeros_like(g)) for k, g in grads.items()}
    for k, g in grads.items():
        holders[k].grad = g.clone()
    torch.nn.utils.clip_grad_norm_(list(holders.values()), m, norm_type=2)
    clipped = {k: h.grad for k, h in holders.items()}               # (compare_with_oracle applies the +-5 clamp)
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, max_grad_norm=m)
    assert ts.packed_head == (head == "packed_head")
    loss = ts(*step_args(variant, batch, enc_out))
    assert ts.use_graph, "hipGraph capture failed: the captured step was not exercised"
    got_norm, got_coef = ts.grad_norm.item(), ts.clip_coef.item()
    print("%s: norm %.7g, oracle %.7g, coef %.7g" % (name, got_norm, norm_ref, got_coef))
    assert abs(got_norm - norm_ref) <= 2e-3 * norm_ref
    assert abs(got_coef - m / (got_norm + 1e-6)) <= 1e-6 * got_coef and got_coef < 0.51
    compare_with_oracle(ts, dec, loss.item(), loss_ref, clipped)
    c1 = 1.0 - 0.9
    first_moment = types.SimpleNamespace(grads={id(p): ts._slot(ts.flat_m, p) / c1 for p in ts.params})
    compare_with_oracle(first_moment, dec, loss.item(), loss_ref, clipped)


def test_a_bound_that_never_binds_is_the_default_step(det_off_after):
    """m = 10 x the oracle's norm: coef is exactly 1, and (deterministic mode) parameters, moments and losses after three
    steps are the bits of a TrainStep without the argument."""
    norm_ref = oracle_case("knowledge")[-1]
    ts0, _, _, l0 = run_steps("knowledge", 3)
    ts1, _, _, l1 = run_steps("knowledge", 3, max_grad_norm=10.0 * norm_ref)
    assert ts0._words is None and ts1.clip_coef.item() == 1.0 and ts1.grad_norm.item() > 0
    assert all(same_bits(a, b) for a, b in zip(l0, l1))
    for a, b in ((ts0.flat_p, ts1.flat_p), (ts0.flat_m, ts1.flat_m), (ts0.flat_v, ts1.flat_v), (ts0.flat_g, ts1.flat_g)):
        assert same_bits(a, b)
    assert set(ts0.state_dict()) == set(ts1.state_dict())
    assert ts0.state_dict()["param_groups"][0].keys() == ts1.state_dict()["param_groups"][0].keys()
    with pytest.raises(IckError):
        ts0.grad_norm


def test_no_clamp_with_grad_clip_none():
    """grad_clip=None: no element clamp -- the written-back gradient is the oracle's times the coefficient, elements
    beyond what +-0.01 would have left included."""
    variant, V, P, batch, enc_out, loss_ref, grads, norm_ref = oracle_case("geo")
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=4e-4, grad_clip=None, max_grad_norm=0.5 * norm_ref)
    ts(*step_args(variant, batch, enc_out))
    big = max(g.abs().max().item() for g in grads.values())
    assert abs(ts.flat_g[:ts.n].abs().max().item() - 0.5 * big) <= 2e-3 * big
    dec2 = zero_dropout(build_decoder(variant, V, P).train())
    ts2 = TrainStep(dec2, lr=4e-4, grad_clip=0.01 * big, max_grad_norm=0.5 * norm_ref)
    ts2(*step_args(variant, batch, enc_out))
    assert ts2.flat_g[:ts2.n].abs().max().item() == np.float32(0.01 * big)


def test_bad_arguments():
    variant, V, _ = CASES["geo"]
    dec = build_decoder(variant, V, synth.make_params(variant, V, 17)).train()
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(IckError):
            TrainStep(dec, max_grad_norm=bad)
    for bad in (dict(kind="exponential"), dict(kind="cosine", warmup_steps=4, total_steps=4),
                dict(kind="inverse_sqrt", warmup_steps=0)):
        with pytest.raises(IckError):
            TrainStep(dec, lr_schedule=bad)
    ts = TrainStep(dec, max_grad_norm=2.0)
    for bad in (0.0, float("nan")):
        with pytest.raises(IckError):
            ts.set_max_grad_norm(bad)
    assert ts.max_grad_norm == 2.0 and ts._words[W_MAX].item() == 2.0


# ------------------------------------------------------------------------------------------------ the schedule in the step
CONSTANT4 = dict(kind="constant", warmup_steps=4)
COSINE = dict(kind="cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1)


@pytest.mark.parametrize("sch", [CONSTANT4, COSINE], ids=["constant_w4", "cosine_w2_n6"])
def test_schedule_over_captured_steps(sch, det_off_after):
    """Eight captured steps: the rate word after each is lr_at(t) (1e-6 relative plus 1e-6 * lr absolute), and nothing
    is captured after the first step -- not by the steps, not by set_lr(lr * 0.8), not by set_max_grad_norm."""
    lr = 4e-4
    ts, dec, args, _ = run_steps("geo", 1, lr_schedule=sch, max_grad_norm=1.0)
    assert ts.use_graph and len(ts._graphs) == 1
    calls = _count_captures(ts)
    graphs = dict(ts._graphs)
    rates = [ts.lr_now.item()]
    for t in range(2, 9):
        ts(*args)
        rates.append(ts.lr_now.item())
    for t, got in enumerate(rates, start=1):
        want = lr_at(t, float(np.float32(lr)), sch)
        assert abs(got - want) <= 1e-6 * want + 1e-6 * lr, (t, got, want)
    ts.set_lr(lr * 0.8)
    ts(*args)
    want = lr_at(9, float(np.float32(lr * 0.8)), sch)
    assert abs(ts.lr_now.item() - want) <= 1e-6 * want + 1e-6 * lr
    ts.set_max_grad_norm(1e-3)
    ts(*args)
    assert ts.clip_coef.item() < 1.0 and abs(ts.clip_coef.item() * (ts.grad_norm.item() + 1e-6) - 1e-3) <= 1e-9
    assert not calls and ts._graphs == graphs and int(ts.counter.item()) == 10
    assert ts.state_dict()["param_groups"][0]["lr"] == lr * 0.8        # the BASE rate; the position is the step count


def test_warmup_step_is_the_default_step_at_that_rate(det_off_after):
    """Step 1 of the W = 4 warmup (deterministic mode) leaves the bits of a default TrainStep built at the rate the word
    reports: the schedule changes the step size and nothing else."""
    ts, _, _, (l1,) = run_steps("geo", 1, lr_schedule=CONSTANT4)
    rate = float(ts.lr_now)
    assert rate == np.float32(np.float32(4e-4) * np.float32(0.25))
    variant, V, P, _, batch, enc_out = step_case("geo")
    ref = TrainStep(build_decoder(variant, V, P).train(), lr=rate, grad_clip=5.0, seed=11, deterministic=True)
    l0 = ref(*step_args(variant, batch, enc_out)).clone()
    assert same_bits(l0, l1) and same_bits(ref.flat_p, ts.flat_p) and same_bits(ref.flat_m, ts.flat_m)


def test_set_lr_then_resume_from_state_dict(det_off_after):
    """After three steps and set_lr(lr * 0.8), the next step is, bit for bit (deterministic mode), that of a fresh
    TrainStep built at the new base rate with the same schedule and bound and loaded from state_dict(): no state beyond
    the base rate and the step count places a run in its schedule."""
    lr = 4e-4
    kw = dict(lr_schedule=COSINE, max_grad_norm=0.05)
    ts, dec, args, _ = run_steps("geo", 3, **kw)
    calls = _count_captures(ts)
    ts.set_lr(lr * 0.8)
    state = ts.state_dict()
    snap = {k: v.detach().clone() for k, v in dec.state_dict().items() if k != "pos_encoder.pe"}
    l4 = ts(*args).clone()
    assert not calls and ts.clip_coef.item() < 1.0
    variant, V, _ = STEP_CASES["geo"]
    fresh_dec = build_decoder(variant, V, snap).train()
    fresh = TrainStep(fresh_dec, lr=lr * 0.8, grad_clip=5.0, seed=11, deterministic=True, **kw)
    fresh.load_state_dict(state)
    lf = fresh(*args)
    assert same_bits(lf, l4) and same_bits(fresh.flat_p, ts.flat_p) and same_bits(fresh.flat_g, ts.flat_g)
    assert same_bits(fresh._words, ts._words)
    # a loaded state with another rate writes the word and keeps the graphs; other betas capture again
    graphs = dict(fresh._graphs)
    state["param_groups"][0]["lr"] = 1e-4
    fresh.load_state_dict(state)
    assert fresh._graphs == graphs and fresh._words[W_BASE].item() == np.float32(1e-4)
    state["param_groups"][0]["betas"] = (0.8, 0.999)
    fresh.load_state_dict(state)
    assert not fresh._graphs


def test_eager_equals_captured(det_off_after):
    kw = dict(lr_schedule=COSINE, max_grad_norm=0.05)
    ts0, _, _, l0 = run_steps("knowledge", 3, **kw)
    ts1, _, _, l1 = run_steps("knowledge", 3, use_graph=False, **kw)
    assert ts0._graphs and not ts1._graphs
    assert all(same_bits(a, b) for a, b in zip(l0, l1))
    assert same_bits(ts0.flat_p, ts1.flat_p) and same_bits(ts0.flat_g, ts1.flat_g) and same_bits(ts0._words, ts1._words)
    assert ts0.clip_coef.item() < 1.0


def test_lazy_update_with_clip_and_schedule():
    """tests/test_adam_derive_gpu.py's lazy test with the new arguments, to its tolerances: the same optimizer steps in
    the same order, the words of the last update once flush() applied it."""
    variant, B, L, K, V, seed = "geo", 6, 9, 6, 160, 13
    P = synth.make_params(variant, V, seed)
    enc, _, _ = make_encoder(seed)
    batches = []
    for s_ in (seed, seed + 1):
        b = synth.make_batch(variant, B, L, K, V, 0, s_)
        batches.append([b["captions"].cuda(), synth.make_feats(B, s_).cuda(), b["caption_masks"].cuda(),
                        b["caption_lengths"].cuda(), b["entities"]])
    sch = dict(kind="linear", warmup_steps=2, total_steps=8, min_lr_ratio=0.1)

    def run(lazy):
        dec = zero_dropout(build_decoder(variant, V, P).train())
        ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, encoder=enc, lazy_update=lazy, max_grad_norm=0.05, lr_schedule=sch)
        losses = [ts(*batches[i % 2]).item() for i in range(5)]
        assert ts.use_graph and ts.derived is not None and ts._pending == lazy
        assert int(ts.counter.item()) == (4 if lazy else 5)
        ts.flush()
        assert int(ts.counter.item()) == 5
        return ts, losses

    ts1, l1 = run(True)
    ts0, l0 = run(False)
    for a, b_ in zip(l1, l0):
        assert abs(a - b_) < 2e-4 * max(1.0, abs(b_)), (l1, l0)
    assert (ts1.flat_p - ts0.flat_p).abs().max().item() <= 5 * 4e-4 + 1e-6
    assert ((ts1.flat_p - ts0.flat_p).abs() > 1e-4).float().mean().item() < 0.02
    assert ts1.lr_now.item() == ts0.lr_now.item() and abs(ts1.lr_now.item() - lr_at(5, 4e-4, sch)) <= 2e-6 * 4e-4
    assert ts1.clip_coef.item() < 1.0 and abs(ts1.grad_norm.item() - ts0.grad_norm.item()) <= 2e-3 * ts0.grad_norm.item()


def test_self_critical_step_over_a_clipped_train_step():
    from ick_amd.scst import SelfCriticalStep
    from test_sample_gpu import make_case
    dec, cfg, P, ents, facts, enc = make_case("knowledge", 3, 5, 40, 4, 21, end_bias=1.5)
    ts = TrainStep(dec.train(), lr=4e-4, grad_clip=5.0, max_grad_norm=1.0)
    step = SelfCriticalStep(ts, lambda toks, img: (toks % 7).sum(1).double(), num_samples=3, baseline="mean", max_len=8,
                            seed=3)
    for _ in range(2):
        out = step(enc.cuda(), ents, facts.cuda())
        norm, coef = ts.grad_norm.item(), ts.clip_coef.item()
        assert math.isfinite(out.loss.item()) and math.isfinite(norm) and norm > 0 and 0 < coef <= 1.0
        assert coef == 1.0 or abs(coef * (norm + 1e-6) - 1.0) <= 1e-6


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_train_main_with_clip_and_schedule(tmp_path, fused):
    """train.main over both Config fields, two batches per epoch, three epochs = six optimizer steps: finite losses, the
    logged norm, and a checkpoint whose optimizer carries the BASE rate (fused) / the scheduled rate beside it (unfused)."""
    from ick_amd import train as tr, utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    sch = dict(kind="cosine", warmup_steps=2, total_steps=6, min_lr_ratio=0.1)
    cfg = tr.Config(variant="geo", data_dir=data_dir, data_name="toy", epochs=3, batch_size=8, workers=0, print_freq=1000,
                    fused=fused, out_dir=str(tmp_path), max_batches=2, max_grad_norm=0.5, lr_schedule=sch)
    torch.manual_seed(0)
    tr.STATS.pop("last_grad_norm", None)
    hist = tr.main(cfg)
    assert len(hist) == 3 and all(math.isfinite(h[0]) and math.isfinite(h[1]) for h in hist)
    assert math.isfinite(tr.STATS["last_grad_norm"]) and tr.STATS["last_grad_norm"] > 0
    ck = ut.load_checkpoint(str(tmp_path / "checkpoint_2_toy.pth.tar"), map_location="cuda")
    group = ck["decoder_optimizer"].param_groups[0]
    assert int(float(next(iter(ck["decoder_optimizer"].state.values()))["step"])) == 6
    if fused:
        assert group["lr"] == cfg.decoder_lr
    else:
        assert group["base_lr"] == cfg.decoder_lr and abs(group["lr"] - lr_at(6, cfg.decoder_lr, sch)) <= 1e-12
