"""The training step across BATCH shapes (tests/batch_cases.py) on the MI355X against the float64 oracle, and batch shapes
that change inside one TrainStep.

Per case, at the base geometry (the full tier, DerivedWeights at V = 152): the eval forward, and one captured TrainStep in
every GEMM product mode -- loss, every gradient, Adam's closed form on every element, the weights after the step -- with
the launches the table promises read back from the test hooks: the decoder layers' weight gradients reduced through the
valid-row maps over K = B L rows (ops.GROUP_LOG), and the attention problems of the case's (T, S) on the kernels the
table names (ops.ATTN_LOG -> ops.attention_plan).  A batch without a single valid row is a no-op on every piece of state.

Bars (none new): scores dropout_ref.SCORE_BAR = 2e-4 * max(1, |ref|max); loss 2e-5; gradients 2e-3 of max(1e-3, |ref|max)
with the ReLU-flip allowance; Adam's closed form and the post-step weights as
tests/test_bench_sizes_gpu.py::run_train_step_vs_oracle; every loss of a sequence 2e-5, the bar of
tests/test_model_geometry_gpu.py::test_three_steps_on_alternating_batches.

Measured on the MI355X, worst over the three GEMM product modes, next to the oracle's own float32 floor
(tests/test_batch_geometry_cpu.py: scores <= 2.5e-6, loss <= 9.8e-7, gradients <= 2.2e-6):

  case               Mp    scores   loss     gradient (tensor)
  one_row            1     1.6e-06  7.5e-07  1.3e-06 (entities.layers.1.self_attn.out_proj.weight)
  one_caption        8     1.9e-06  2.9e-07  2.7e-06 (entities.layers.0.norm1.weight)
  one_fact           1     5.3e-08  2.2e-07  7.8e-07 (fc_entity.weight)
  nearly_empty       1     1.8e-06  2.4e-07  8.1e-07 (entities.layers.0.self_attn.in_proj_weight)
  equal_lengths      24    2.3e-06  4.7e-07  6.7e-07 (entities.layers.0.self_attn.in_proj_bias)
  interleaved        17    3.1e-06  2.9e-08  8.0e-07 (entity_encoder.type_embedding.weight)
  rows_64            64    2.7e-06  1.1e-07  6.2e-07 (entities.layers.0.self_attn.in_proj_weight)
  rows_65            65    2.7e-06  3.2e-07  6.6e-07 (entities.layers.1.self_attn.in_proj_weight)
  many_short         128   3.2e-06  2.5e-08  5.7e-07 (decoder.layers.0.self_attn.out_proj.weight)
  long_captions      81    1.6e-07  2.6e-07  6.6e-07 (entities.layers.0.self_attn.in_proj_bias)
  wide_context       52    1.4e-06  1.6e-08  1.1e-06 (fc_fact.weight)
  past_matrix_core   4     4.1e-07  6.2e-07  1.6e-06 (entities.layers.0.norm2.weight)
  base_v150          17    2.2e-06  4.5e-07  7.2e-07 (entity_encoder.type_embedding.weight)

No case needed the ReLU-flip allowance, every capture succeeded, no case is refused: the device sits at the oracle's float32
floor at every batch shape, two to three orders below the bars.  Worst sequence losses: ragged 2.9e-6 (eager update),
3.3e-6 (lazy_update), 1.3e-6 (V = 150); eviction 8.2e-6 (V = 152), 3.6e-6 (V = 150) -- the small batches of that sequence
are the ones on which Adam turns rounding noise into whole +-lr steps -- against 2e-5.

One bug found and fixed (training.py, TrainStep._part_b): the eager update advanced the step counter on a batch without a
single valid row, although it applies no update then (the deferred update of lazy_update never did): bias correction,
the schedule's position, state_dict()'s step and the dropout stream ran one ahead of the moments from there on.  It
failed test_batch_without_a_single_valid_row_changes_nothing (counter 2 against 1) and step 4 of
test_capture_is_invisible_bit_for_bit (counter 4 against 3 applied updates).

Shape changes inside one TrainStep (every new shape: flush of a deferred update, eviction at the fifth key, an eager
warm-up of part B that is a real optimizer step, the snapshot and rewind of [counter] + bucket.tensors(), re-staling
DerivedWeights, conv1's pre-split copy, zeroing the token count):
  (a) an epoch with a ragged tail, twice -- shapes A A tail A A tail -- against the float64 oracle sequence with torch
      Adam; with the eager update, with lazy_update on the feature-map input (where it really defers: it needs
      encoder=, the two-stream captured step and DerivedWeights) and at V = 150 (per-step packing);
  (b) five shapes, one more than the graph cache holds, then the first again, against the oracle sequence;
  (c) a captured TrainStep against a use_graph=False twin in deterministic mode with dropout on and every optimizer
      option on at once, bit for bit after every step: loss, parameters, both moments, the average, the counter, the
      optimizer words, and at the end the weight images against a fresh re-layout of the final weights.  Legs: the
      options alone; lazy_update=True on the feature map (deterministic mode keeps the update where it was --
      TrainStep._lazy_active -- so this leg pins that the flag is inert there and flush() harmless; the deferral itself
      is (a)'s); encoder= with train_conv1=True at B = 3 -> 2, conv1's bucket and pre-split copy included;
      scheduled_sampling over five distinct (B, L), which evicts _ss_bufs and with them the graphs;
  (d) train.main on 20 samples at batch size 8 (batches 8, 8, 4), two epochs, both loops, twice: the loss falls and both
      runs write the same bits.

What breaking the code shows (local experiments on the MI355X, one change at a time; not part of the suite):
  * the snapshot without the moving average `e` (ParamBucket.tensors): all four legs of (c) that existed then fail at
    `step 1 e`, 2.0e-5 apart; (a), (b), (d) pass -- nothing else reads the average.
  * the rewind without re-staling DerivedWeights: (a) and (b) at V = 152 fail `step 1 loss` by 1.7 to 1.9 (the first
    replay runs on images of the warm-up's weights), every leg of (c) at `step 1 loss`, (d) by its falling-loss check;
    the V = 150 legs pass (per-step packing).
  * the snapshot without the counter: every test fails -- (a) ends at counter 8 for 6 steps, (b) at 12, (c) at `step 1
    loss` (other dropout masks), (d) with optimizer step 8.0 in the checkpoint.
  * no flush() before a capture (the pending update dropped): only (a) with lazy_update fails, counter 5 for 6 steps.
  * not zeroing the token count behind the warm-up: nothing fails; the replay path zeroes it again when lazy_update is
    active and nothing is pending, and no other path reads it before the next loss writes it.
  * not re-splitting conv1's pre-split copy behind the rewind: nothing fails, not even in the split-bf16 leg; at 588
    image rows the projection is supposed not to read the copy (not verified here) -- the B = 64 path has
    tests/test_conv1_train_gpu.py::test_presplit_copy_is_fresh_after_steps, which changes no shape.  NOT COVERED.
"""
import os

import pytest
import torch

import batch_cases as BC
import dropout_ref as DR
import ick_amd.synth as synth
import model_cases as MC
from decode_ref import float64_default, params64

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", BC.CASES, ids=[c.name for c in BC.CASES])
SEQ_BAR = 2e-5

_ORACLE = {}


def oracle(c):
    """The case's float64 oracle step, computed once: parameters, loss, scores, gradients, the weights after torch Adam."""
    if c.name not in _ORACLE:
        P = BC.make_params(c)
        o = BC.oracle_step(c, True)
        with float64_default():
            Pa = {k: v.clone().requires_grad_(True) for k, v in params64(P).items() if not k.startswith("fact_encoder.")}
            for k, v in Pa.items():
                v.grad = o["grads"][k].clamp(-MC.CLIP, MC.CLIP)
            torch.optim.Adam(list(Pa.values()), lr=MC.LR).step()
        o.update(P=P, P_after={k: v.detach() for k, v in Pa.items()})
        _ORACLE[c.name] = o
    return _ORACLE[c.name]


def oracle_sequence(name, steps, V, projected=False):
    key = ("sequence", name, V, projected)
    if key not in _ORACLE:
        _ORACLE[key] = MC.oracle_loss_sequence(BC.sequence_model(V), BC.sequence_params(V),
                                               inputs=BC.sequence_inputs(steps, V, projected=projected))
    return _ORACLE[key]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(-1).view(torch.uint8), b.contiguous().view(-1).view(torch.uint8))


def train_decoder(model, P, dropout=False):
    from test_training_gpu import zero_dropout
    dec = MC.build_decoder(model, P).train()
    return dec if dropout else zero_dropout(dec)


@pytest.fixture()
def launch_logs():
    import ick_amd.ops as ops
    ops.GROUP_LOG, ops.ATTN_LOG = [], []
    yield ops
    ops.GROUP_LOG = ops.ATTN_LOG = None


@pytest.fixture()
def det_off_after():
    import ick_amd.ops as ops
    yield
    ops.set_deterministic(False)


def test_no_case_is_refused():
    """batch_cases.REFUSED lists the shapes the library refuses by name; each must still be refused with that message."""
    from ick_amd.lib import IckError
    from ick_amd.training import TrainStep
    for c, text in BC.REFUSED:
        ts = TrainStep(train_decoder(c.model, BC.make_params(c)), lr=MC.LR, grad_clip=MC.CLIP)
        with pytest.raises(IckError, match=text):
            ts(*MC.step_args(*BC.make_inputs(c)))
    assert len(BC.CASES) + len(BC.REFUSED) >= 13


# ------------------------------------------------------------------------------------------------ eval forward
@cases
def test_eval_forward_vs_oracle(c, gemm_split):
    o = oracle(c)
    dec = MC.build_decoder(c.model, o["P"])
    with torch.no_grad():
        scores, caps, dl = dec(*MC.step_args(*BC.make_inputs(c)))
    assert dl == o["decode_lengths"] and sum(dl) == c.Mp
    assert tuple(scores.shape)[::2] == (c.B, c.V + c.K + c.Fn)
    DR.check_scores(scores, o, "%s eval forward" % c.name)


# ------------------------------------------------------------------------------------------------ captured train step
def _plan_note(p):
    return ("mfma", p["nqt"], p["maxt"]) if p["mfma"] else ("general", p["dhp"], p["chunks"])


@cases
def test_captured_train_step_vs_oracle(c, gemm_split, launch_logs):
    from test_bench_sizes_gpu import run_train_step_vs_oracle
    from test_valid_row_wgrad_gpu import _mapped
    ops = launch_logs
    o = oracle(c)
    ts, _ = run_train_step_vs_oracle(c.variant, c.B, c.L, c.K, c.V, c.Fn, c.seed, None, float64=True,
                                     reference=lambda cfg, P, batch, enc_out: (o["loss"], o["grads"], o["P_after"]),
                                     inputs=BC.make_inputs(c), params=o["P"])
    assert ts.use_graph and ts._graphs
    assert (ts.derived is not None) == (c.V % 8 == 0)
    # the decoder layers' weight gradients took the valid-row maps: 6 Linear problems in each of the 3 layers per traced run
    on = _mapped(ops.GROUP_LOG, c.B * c.L)
    assert len(on) >= 18 and len(on) % 18 == 0, len(on)
    assert sorted({(a.M, a.N) for a in on}) == sorted({(300, 512), (512, 300), (300, 300), (900, 300)})
    # the attention problems of the case's shapes ran, both ways, and their launch plan is the table's
    seen = {(d, T, S) for d, T, S, dh, causal in ops.ATTN_LOG if dh == BC.DH}
    for name, (T, S, causal) in c.shapes.items():
        for d, want in zip(("fwd", "bwd"), c.plans[name]):
            assert (d, T, S) in seen, (c.name, name, d, sorted(seen))
            assert _plan_note(ops.attention_plan(d, T, S, BC.DH)) == want, (c.name, name, d)


@pytest.mark.parametrize("V", [BC.V_DERIVED, BC.V_PLAIN])
def test_batch_without_a_single_valid_row_changes_nothing(V, gemm_split):
    """nearly_empty's shape with every length 1, behind one real step (so that moments, images and counter are not at their
    initial values): loss 0, the gradient bucket all zero, parameters, moments, weight images and the counter keep their bits."""
    from dataclasses import replace
    from ick_amd.training import TrainStep
    from test_weight_images_gpu import _buffers
    c = replace(BC.BY_NAME["nearly_empty"], V=V)
    P = BC.make_params(c)
    dec = train_decoder(c.model, P)
    ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP)
    l1 = ts(*MC.step_args(*BC.make_inputs(c))).item()
    assert l1 > 0 and int(ts.counter.item()) == 1 and ts.use_graph and (ts.derived is not None) == (V % 8 == 0)
    state = dict(p=ts.flat_p, m=ts.flat_m, v=ts.flat_v, counter=ts.counter)
    if ts.derived is not None:
        state.update({"image %s %s" % k: b for k, b in _buffers(dec.weight_images()).items()})
    before = {k: t.clone() for k, t in state.items()}
    assert before["m"].abs().max().item() > 0
    loss = ts(*MC.step_args(*BC.make_inputs(c, lengths=[1] * c.B)))
    assert loss.item() == 0.0 and len(ts._graphs) == 1
    assert not ts.flat_g[:ts.n].any() and ts.flat_g[ts._t + 1].item() == 0.0
    for k, t in state.items():
        assert same_bits(t, before[k]), k
    # ... and the step after it is a step again
    l3 = ts(*MC.step_args(*BC.make_inputs(c))).item()
    assert 0 < l3 < l1 and int(ts.counter.item()) == 2


# ------------------------------------------------------------------------------------------------ (a), (b): sequences
def _count_captures(ts):
    from test_label_smoothing_gpu import _count_captures as count
    return count(ts)


def _feature_inputs(steps, V):
    """The sequence with the (B, 2048, 14, 14) feature maps in place of enc_out."""
    return [(batch, synth.make_feats(s[0], s[4])) for s, (batch, _) in zip(steps, BC.sequence_inputs(steps, V))]


def _run_sequence(name, steps, V, lazy=False):
    from ick_amd.training import TrainStep
    from test_bench_sizes_gpu import make_encoder
    ref = oracle_sequence(name, steps, V, projected=lazy)
    enc = None
    if lazy:        # the deferred update needs the feature-map input: Encoder.conv1 (frozen) inside the step
        enc, cw, cb = make_encoder(BC.CONV1_SEED)
        inputs = _feature_inputs(steps, V)
    else:
        inputs = BC.sequence_inputs(steps, V)
    ts = TrainStep(train_decoder(BC.sequence_model(V), BC.sequence_params(V)), lr=MC.LR, grad_clip=MC.CLIP, encoder=enc,
                   lazy_update=lazy)
    calls = _count_captures(ts)
    losses = []
    for batch, x in inputs:
        losses.append(ts(*MC.step_args(batch, x)).item())
        if lazy:
            assert ts._pending and ts._lazy_active(x.cuda())
    ts.flush()
    errs = [abs(a - b) for a, b in zip(losses, ref)]
    print("%s V %d lazy %s: losses %s, oracle %s, errors %s"
          % (name, V, lazy, ["%.6f" % x for x in losses], ["%.6f" % x for x in ref], ["%.1e" % e for e in errs]))
    assert ts.use_graph and (ts.derived is not None) == (V % 8 == 0)
    return ts, calls, ref, errs


@pytest.mark.parametrize("leg", ["eager_update", "lazy_update", "v150"])
def test_epoch_with_a_ragged_tail_vs_oracle(leg):
    V = BC.V_PLAIN if leg == "v150" else BC.V_DERIVED
    ts, calls, ref, errs = _run_sequence("ragged", BC.RAGGED, V, lazy=leg == "lazy_update")
    assert len(ts._graphs) == 2 and int(ts.counter.item()) == 6 and ts.step_count == 6
    assert len(calls) == 2 * 2                        # two shapes captured, each as graph A and graph B; the rest replays
    assert abs(ref[3] - ref[0]) > 1e-3 and abs(ref[4] - ref[0]) > 1e-3, "a later A step must see the updates"
    for i, e in enumerate(errs):
        assert e < SEQ_BAR, ("step %d loss" % (i + 1), e)


@pytest.mark.parametrize("V", [BC.V_DERIVED, BC.V_PLAIN])
def test_more_shapes_than_the_graph_cache_holds_vs_oracle(V):
    assert BC.distinct_shapes(BC.EVICTION[:5]) == 5 and BC.EVICTION[5][:3] == BC.EVICTION[0][:3]
    ts, calls, ref, errs = _run_sequence("eviction", BC.EVICTION, V)
    # the fifth shape emptied the cache, so the first shape was captured a second time: six captures of two graphs each,
    # and two keys left
    assert len(calls) == 2 * 6 and len(ts._graphs) == 2
    assert int(ts.counter.item()) == 6 and ts.step_count == 6
    assert abs(ref[5] - ref[0]) > 1e-3
    for i, e in enumerate(errs):
        assert e < SEQ_BAR, ("step %d loss" % (i + 1), e)


# ------------------------------------------------------------------------------------------------ (c): capture is invisible
ALL_OPTIONS = dict(max_grad_norm=1.0, lr_schedule=dict(kind="cosine", warmup_steps=3, total_steps=12, min_lr_ratio=0.1),
                   ema_decay=0.9, ema_warmup=True, weight_decay=0.05, decoupled_weight_decay=True, label_smoothing=0.1)
BITWISE_LEGS = {
    "options": dict(steps=BC.BITWISE),
    "lazy_update": dict(steps=BC.BITWISE, feats=True, lazy_update=True),
    "train_conv1": dict(steps=BC.BITWISE_CONV1, feats=True, train_conv1=True, encoder_weight_decay=0.05, gemm=0),
    # ... in the product mode where Encoder.conv1 multiplies with the pre-split copy of its weight (none in mode 0)
    "train_conv1_split_bf16": dict(steps=BC.BITWISE_CONV1, feats=True, train_conv1=True, encoder_weight_decay=0.05, gemm=1),
    "scheduled_sampling": dict(steps=BC.BITWISE_SS, scheduled_sampling=dict(prob=0.5, mode="sample")),
}


def _state(ts):
    out = dict(p=ts.flat_p, m=ts.flat_m, v=ts.flat_v, e=ts.flat_e, counter=ts.counter, words=ts._words, lr_now=ts.lr_now)
    if ts.train_conv1:
        out.update(conv1_p=ts.enc_p, conv1_m=ts.enc_m, conv1_v=ts.enc_v, conv1_e=ts.enc_e)
    if ts.ss is not None:
        out.update(zip(("ss_captions", "ss_masks", "ss_replaced"), ts.sampled_inputs()))
    return out


@pytest.mark.parametrize("leg", sorted(BITWISE_LEGS))
def test_capture_is_invisible_bit_for_bit(leg, det_off_after):
    """A captured TrainStep and a use_graph=False twin from the same parameters through the same batches: the twin never
    warms up, snapshots or rewinds, so whatever the rewind misses shows as a different bit."""
    import ick_amd.ops as ops
    kw = dict(BITWISE_LEGS[leg])
    steps, feats, gemm = kw.pop("steps"), kw.pop("feats", False), kw.pop("gemm", None)
    V = BC.V_DERIVED
    mode_before = ops.gemm_split_mode()
    if gemm is not None:
        ops.set_gemm_split(gemm)
    try:
        _capture_is_invisible(leg, kw, steps, feats, V)
    finally:
        ops.set_gemm_split(mode_before)


def _capture_is_invisible(leg, kw, steps, feats, V):
    from ick_amd.training import TrainStep
    from test_bench_sizes_gpu import make_encoder
    from test_weight_images_gpu import _buffers
    inputs = _feature_inputs(steps, V) if feats else BC.sequence_inputs(steps, V)
    twins = []
    for use_graph in (True, False):
        dec = train_decoder(BC.sequence_model(V), BC.sequence_params(V), dropout=True)
        enc = make_encoder(BC.CONV1_SEED)[0] if feats else None
        ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP, seed=11, deterministic=True, use_graph=use_graph, encoder=enc,
                       **ALL_OPTIONS, **kw)
        twins.append((ts, dec, enc))
    (cap, dec_c, enc_c), (eag, _, _) = twins
    calls = _count_captures(cap)
    applied = 0
    for i, ((batch, x), s) in enumerate(zip(inputs, steps)):
        args = MC.step_args(batch, x)
        losses = []
        for ts, _, _ in twins:
            losses.append(ts(*args).clone())
            assert not ts._pending              # (deterministic mode never defers the update)
            ts.flush()
        applied += int(any(n > 1 for n in batch["caption_lengths"].view(-1).tolist()))
        assert same_bits(*losses), ("step %d loss" % (i + 1), [x.item() for x in losses])
        a, b = _state(cap), _state(eag)
        for k in a:
            assert same_bits(a[k], b[k]), ("step %d %s" % (i + 1, k), (a[k].float() - b[k].float()).abs().max().item())
        assert int(cap.counter.item()) == applied          # a batch without a valid row is no optimizer step
    assert cap.use_graph and not eag._graphs and cap.derived is not None and eag.derived is not None
    shapes = BC.distinct_shapes(steps)
    if leg == "scheduled_sampling":
        # the fifth (B, L) evicted the mix buffers and every graph: six captures (A, B; the first pass goes through
        # ops.capture itself), two keys and two buffer sets left
        assert shapes == 5 and len(calls) == 2 * 6 and len(cap._graphs) == 2 and len(cap._ss_bufs) == 2
    else:
        assert len(calls) == 2 * shapes and len(cap._graphs) == shapes
    assert applied == len(steps) - sum(1 for s in steps if s[3] is not None and set(s[3]) == {1})
    assert (cap.flat_p - cap.flat_e).abs().max().item() > 0 and cap.flat_m.abs().max().item() > 0
    # the weight images (and conv1's pre-split copy) are what a fresh re-layout of the final weights gives -- compared
    # inside each step's own buffers: bytes no kernel writes differ between two allocations
    for ts, dec, enc in twins:
        bufs = _buffers(dec.weight_images())
        before = {k: b.clone() for k, b in bufs.items()}
        ts.derived.refresh()
        for k, b in bufs.items():
            assert same_bits(b, before[k]), ("weight image", k, ts.use_graph)
        assert not ts.train_conv1 or (enc.conv1_presplit() is not None) == (leg == "train_conv1_split_bf16")
        if ts.train_conv1 and enc.conv1_presplit() is not None:
            ps = enc.conv1_presplit()
            was = ps.clone()
            ts._conv1_resplit()
            assert same_bits(ps, was), ("conv1 pre-split copy", ts.use_graph)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ (d): the training script
@pytest.mark.parametrize("prefetch", [True, False], ids=["pipelined_loop", "plain_loop"])
def test_train_main_with_a_smaller_last_batch(tmp_path, prefetch, det_off_after):
    """20 samples at batch size 8: every epoch ends in a batch of 4 (the loaders keep it: drop_last=False).  V = 64: the
    step's Adam pass maintains the weight images.  Deterministic mode: two runs end in the same bits."""
    from ick_amd import train as tr, utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=20, n_val=8, n_test=4, L=12, K=6, V=64, F=0)
    finals = []
    for run in ("a", "b"):
        out_dir = str(tmp_path / run)
        os.makedirs(out_dir)
        cfg = tr.Config(variant="geo", data_dir=data_dir, data_name="toy", epochs=2, batch_size=8, workers=0, print_freq=1000,
                        fused=True, seed=3, out_dir=out_dir, prefetch=prefetch, deterministic=True)
        torch.manual_seed(0)
        hist = tr.main(cfg)
        assert len(hist) == 2 and all(h[0] == h[0] and h[1] == h[1] for h in hist)
        assert hist[-1][0] < hist[0][0]                                                # it trains
        ck = ut.load_checkpoint(os.path.join(out_dir, "checkpoint_toy.pth.tar"), map_location="cuda")
        assert ck["epoch"] == 1
        opt = ck["decoder_optimizer"].state_dict()
        assert {float(st["step"]) for st in opt["state"].values()} == {6.0}            # 2 epochs x (8 + 8 + 4)
        finals.append((hist, {k: v.detach().clone() for k, v in ck["decoder"].state_dict().items()}, opt["state"]))
    (h0, d0, o0), (h1, d1, o1) = finals
    assert [h[0] for h in h0] == [h[0] for h in h1]                                    # the epochs' training losses
    assert d0.keys() == d1.keys() and o0.keys() == o1.keys()
    for k in d0:
        assert same_bits(d0[k], d1[k]), k
    for i in o0:
        assert same_bits(o0[i]["exp_avg"], o1[i]["exp_avg"]) and same_bits(o0[i]["exp_avg_sq"], o1[i]["exp_avg_sq"]), i
