"""The model-level paths across model geometries (tests/model_cases.py) on the MI355X, against the float64 oracle.

The geometry alone selects the path here -- no __dict__ overrides, no environment switches: forward row chains with the
unfused backward and the staged per-step packing (deep_*), chains off by the decoder's or the entity stack's feed-forward
width or by emb_dim, the exact limits of both chain kernels and of the fused decode in one model (limit_*), a single
layer, widths that are no multiple of 4, news through the captured step, 49 image rows.  Per case: the tier the model
takes, eval-mode scores, one captured TrainStep (loss, every gradient, Adam's closed form, the weights after it), three
captured steps on two alternating batches (what makes a stale re-laid-out weight image show), greedy decode, and -- where
the fused decode kernels run -- beam search; in the mixed tier also the autograd bridge and bit reproducibility of the
deterministic mode with dropout on.  A head wider than 32 is refused by name at every entry point.

Bars: scores 2e-4 * max(1, |ref|max) (dropout_ref.SCORE_BAR); loss 2e-5, gradients 2e-3 of max(1e-3, |ref|max) with the
ReLU-flip allowance, Adam and weights as tests/test_bench_sizes_gpu.py::run_train_step_vs_oracle; every loss of the
three-step sequence 2e-5, the bar test_training_gpu.py::test_train_step_matches_reference_sequence_and_dp_split holds one
step's loss to (a stale image leaves step 2 on weights one Adam step = 4e-4 per element behind: off in the second digit).

Measured on the MI355X, worst over the three GEMM product modes, next to the oracle's own float32 noise floor
(tests/test_model_geometry_cpu.py: scores <= 3.1e-6, loss <= 8.7e-7, gradients <= 2.2e-6; no ReLU-flip unit):

  case                 tier       derived  scores   loss     gradient (tensor)                                 3-step loss
  base                 full       no       2.2e-06  3.7e-08  8.5e-07 (entities.layers.2.norm1.weight)          5.2e-07
  deep_geo             mixed      no       2.3e-06  4.5e-07  1.9e-06 (entities.layers.0.norm2.weight)          6.5e-07
  deep_knowledge       mixed      no       7.2e-07  8.4e-08  1.7e-06 (decoder.layers.2.multihead_attn.in_proj_bias) 3.1e-07
  single_layer         full       no       1.1e-06  3.3e-07  8.9e-07 (decoder.layers.0.multihead_attn.in_proj_bias) 5.4e-07
  limit_geo            full       no       2.8e-06  1.1e-07  6.8e-07 (entities.layers.2.linear1.weight)        1.6e-06
  limit_knowledge      full       no       7.2e-07  3.5e-08  1.0e-06 (decoder.layers.1.linear1.weight)         2.9e-07
  wide_ffn             no_chains  no       6.9e-07  4.8e-08  1.3e-06 (decoder.layers.0.self_attn.in_proj_weight) 3.0e-07
  wide_ctx             no_chains  no       2.7e-06  5.2e-07  8.2e-07 (entities.layers.0.self_attn.in_proj_weight) 5.2e-07
  wide_model           none       no       2.6e-06  3.6e-08  7.8e-07 (entities.layers.0.self_attn.in_proj_weight) 1.6e-06
  news_small           full       no       8.9e-08  5.0e-07  4.0e-07 (decoder.layers.0.self_attn.out_proj.bias) 5.0e-07
  odd_head             full       no       1.0e-06  2.7e-07  5.7e-07 (entities.layers.1.linear1.weight)        1.3e-06
  unaligned            partial    no       1.0e-06  3.9e-07  6.0e-07 (entities.layers.0.norm1.weight)          1.3e-06
  base_v152            full       yes      -        5.0e-07  8.8e-07 (decoder.layers.0.multihead_attn.in_proj_weight) 5.0e-07
  single_layer_v152    full       yes      -        1.8e-07  1.9e-06 (decoder.layers.0.norm1.weight)           1.8e-07
  limit_geo_v152       full       yes      -        4.7e-07  8.0e-07 (decoder.layers.0.self_attn.out_proj.weight) 9.8e-07
  limit_knowledge_v152 full       yes      -        1.4e-07  1.1e-06 (decoder.layers.0.self_attn.out_proj.weight) 3.8e-07
  news_small_v152      full       yes      -        2.2e-07  4.8e-07 (decoder.layers.0.norm1.weight)           2.8e-07
  odd_head_v152        full       yes      -        5.7e-07  5.9e-07 (entities.layers.0.self_attn.in_proj_bias) 8.2e-07

No case needed the ReLU-flip allowance (no hidden unit set aside), every capture succeeded, and the tiers observed on the
device are the table's.  Greedy step scores on the fused kernels stay within 3.8e-6 of the oracle's; tokens are identical
in every case, beam search included.  So the device sits at the oracle's own float32 floor, two to three orders below the
bars.  (V = 150 keeps DerivedWeights from all twelve geometries -- 150 % 8 != 0, weights.py -- hence the *_v152 rows.)

What the three-step check is there for, shown by breaking the code (not part of the suite): with the staged second-stage
`chain` refresh skipped inside the captured step, deep_geo's step-2 loss is off by 5.2e-1; with the Adam pass no longer
writing DerivedWeights' images, base_v152's by 1.9e-1.  Both fail `step 2 loss`; the one-step checks cannot see either.
"""
import pytest
import torch

import model_cases as MC
from decode_ref import float64_default, params64
from model_cases import B, K, L, MAX_LEN, SEED
from oracle import restatement as R

pytestmark = pytest.mark.gpu

cases = pytest.mark.parametrize("c", MC.CASES, ids=[c.name for c in MC.CASES])
# ... and the geometries that admit DerivedWeights again at the aligned vocabulary, for what a TrainStep does
step_cases = pytest.mark.parametrize("c", MC.ALL_CASES, ids=[c.name for c in MC.ALL_CASES])

_ORACLE = {}


def oracle(c):
    """The case's float64 oracle step, computed once: parameters, loss, scores, gradients, the weights after torch Adam."""
    if c.name not in _ORACLE:
        P = MC.make_params(c)
        o = MC.oracle_step(c, True, P)
        with float64_default():
            Pa = {k: v.clone().requires_grad_(True) for k, v in params64(P).items() if not k.startswith("fact_encoder.")}
            for k, v in Pa.items():
                v.grad = o["grads"][k].clamp(-MC.CLIP, MC.CLIP)
            torch.optim.Adam(list(Pa.values()), lr=MC.LR).step()
        o.update(P=P, P_after={k: v.detach() for k, v in Pa.items()})
        _ORACLE[c.name] = o
    return _ORACLE[c.name]


def train_decoder(c, P, dropout=False):
    from test_training_gpu import zero_dropout
    dec = MC.build_decoder(c, P).train()
    return dec if dropout else zero_dropout(dec)


# ------------------------------------------------------------------------------------------------ which path runs
@step_cases
def test_tier_is_the_tables(c):
    import ick_amd.ops as ops
    from ick_amd.training import TrainStep, forward_with_tape
    o = oracle(c)
    dec = train_decoder(c, o["P"])
    assert dec.chain_supported() == c.chain
    assert dec.chain_bwd_supported() == c.chain_bwd
    assert ops.decode_supported(c.d, c.H, c.FF_dec, c.S, MAX_LEN) == c.decode
    batch, enc_out = MC.make_inputs(c)
    ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP)
    ts(*MC.step_args(batch, enc_out))
    assert (ts.derived is not None) == c.derived
    assert ts.use_graph and ts._graphs, "hipGraph capture failed in tier %s" % c.tier
    lengths, sort_ind = batch["caption_lengths"].squeeze(1).sort(descending=True)
    sd = sort_ind.cuda()
    facts = batch["facts"].cuda()[sd].contiguous() if "facts" in batch else None
    scores, tape = forward_with_tape(dec, batch["captions"].cuda()[sd].contiguous(),
                                     batch["caption_masks"].cuda()[sd].contiguous(),
                                     batch["entities"].cuda()[sd].contiguous(), facts,
                                     enc_out.cuda().permute(0, 2, 1).contiguous(), sd.to(torch.int32))
    assert (tape.misc.get("pkb") is not None) == c.chain_bwd
    assert tuple(scores.shape) == (B, L, c.V + K + c.Fn)
    print("%s: tier %s (chain %s, chain_bwd %s, decode %s, derived %s)"
          % (c.name, c.tier, dec.chain_supported(), dec.chain_bwd_supported(), c.decode, ts.derived is not None))


# ------------------------------------------------------------------------------------------------ eval forward
@cases
def test_eval_forward_vs_oracle(c, gemm_split):
    import dropout_ref as DR
    o = oracle(c)
    dec = MC.build_decoder(c, o["P"])
    batch, enc_out = MC.make_inputs(c)
    with torch.no_grad():
        scores, caps, dl = dec(*MC.step_args(batch, enc_out))
    assert dl == o["decode_lengths"]
    DR.check_scores(scores, o, "%s eval forward" % c.name)


# ------------------------------------------------------------------------------------------------ captured train step
@step_cases
def test_captured_train_step_vs_oracle(c, gemm_split):
    from test_bench_sizes_gpu import run_train_step_vs_oracle
    o = oracle(c)
    ts, _ = run_train_step_vs_oracle(c.variant, B, L, K, c.V, c.Fn, SEED, None, geometry=c.geometry, float64=True,
                                     reference=lambda cfg, P, batch, enc_out: (o["loss"], o["grads"], o["P_after"]))
    assert ts.use_graph and ts._graphs
    assert (ts.derived is not None) == c.derived and ts.dec.chain_bwd_supported() == c.chain_bwd


@step_cases
def test_three_steps_on_alternating_batches(c):
    """The loss sequence over the batches of seeds 21, 22, 21 against the oracle's (torch Adam, float64).  Steps 2 and 3 run
    on what step 1's optimizer pass left in the re-laid-out weight images: re-packed by the staged per-step launches in
    the mixed tier, written by the Adam pass itself with DerivedWeights, only the gathered cross K/V weight without
    chains."""
    from ick_amd.training import TrainStep
    o = oracle(c)
    key = c.name + "/sequence"
    if key not in _ORACLE:
        _ORACLE[key] = MC.oracle_loss_sequence(c, o["P"])
    ref = _ORACLE[key]
    assert abs(ref[0] - o["loss"]) < 1e-12
    ts = TrainStep(train_decoder(c, o["P"]), lr=MC.LR, grad_clip=MC.CLIP)
    losses = [ts(*MC.step_args(*MC.make_inputs(c, seed))).item() for seed in MC.STEP_SEEDS]
    assert ts.use_graph and len(ts._graphs) == 1
    errs = [abs(a - b) for a, b in zip(losses, ref)]
    print("%s three steps: losses %s, oracle %s, errors %s" % (c.name, losses, ref, ["%.1e" % e for e in errs]))
    assert abs(ref[2] - ref[0]) > 1e-3, "the third step must see the update, or the sequence shows nothing"
    for i, e in enumerate(errs):
        assert e < 2e-5, ("step %d loss" % (i + 1), losses[i], ref[i])


# ------------------------------------------------------------------------------------------------ mixed tier only
MIXED = [c for c in MC.CASES if c.tier == "mixed"]
mixed = pytest.mark.parametrize("c", MIXED, ids=[c.name for c in MIXED])


@mixed
def test_mixed_tier_autograd_bridge_vs_oracle(c):
    """dec(*args) -> cross_entropy -> backward() through DecoderGraphFn, dropout off: forward chains, unfused backward."""
    import dropout_ref as DR
    from torch.nn.utils.rnn import pack_padded_sequence
    o = oracle(c)
    dec = train_decoder(c, o["P"])
    assert dec.chain_supported() and not dec.chain_bwd_supported()
    batch, enc_out = MC.make_inputs(c)
    scores, caps, dl = dec(*MC.step_args(batch, enc_out))
    DR.check_scores(scores, o, "%s bridge forward" % c.name)
    sp = pack_padded_sequence(scores, dl, batch_first=True).data
    tp = pack_padded_sequence(caps[:, 1:], dl, batch_first=True).data
    loss = torch.nn.functional.cross_entropy(sp, tp, ignore_index=0)
    assert abs(loss.item() - o["loss"]) < DR.LOSS_BAR
    loss.backward()
    mine = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in dec.named_parameters()}
    DR.check_grads(mine, o["grads"], "%s bridge" % c.name)


@mixed
def test_mixed_tier_deterministic_steps_are_bit_reproducible(c):
    import ick_amd.ops as ops
    from ick_amd.training import TrainStep
    P = oracle(c)["P"]
    runs = []
    try:
        for _ in range(2):
            ts = TrainStep(train_decoder(c, P, dropout=True), lr=MC.LR, grad_clip=MC.CLIP, seed=11, deterministic=True)
            losses = [ts(*MC.step_args(*MC.make_inputs(c, seed))).item() for seed in MC.STEP_SEEDS[:2]]
            assert ts.use_graph and ts.derived is None
            runs.append((losses, ts.flat_g.clone()))
    finally:
        ops.set_deterministic(False)
    (l0, g0), (l1, g1) = runs
    assert l0 == l1
    assert torch.equal(g0, g1), (g0 - g1).abs().max().item()
    assert g0[:-2].abs().max().item() > 0


# ------------------------------------------------------------------------------------------------ decode
def decode_inputs(c, n=3):
    batch, enc_out = MC.make_inputs(c)
    facts = batch["facts"][:n] if "facts" in batch else None
    return enc_out[:n], batch["entities"][:n], facts


@cases
def test_greedy_decode_vs_oracle(c):
    """As tests/test_decode_gpu.py::test_fused_decode_other_model_sizes: tokens equal R.predict's per sample, and -- on the
    fused kernels, which keep every step's score row -- the step scores within 2e-4; without them predict() must give
    the same tokens through the per-op launches, and beam search / sampling must say what they need."""
    import ick_amd.ops as ops
    from ick_amd.lib import IckError
    o = oracle(c)
    dec = MC.build_decoder(c, o["P"])
    cfg = MC.oracle_config(c)
    enc, ents, facts = decode_inputs(c)
    fargs = [] if facts is None else [facts.cuda()]
    assert ops.decode_supported(c.d, c.H, c.FF_dec, c.S, MAX_LEN) == c.decode
    seqs = dec.predict(enc.cuda(), MAX_LEN, ents, *fargs)
    assert tuple(seqs.shape) == (MAX_LEN, enc.shape[0])
    out = scores = None
    if c.decode:
        from test_decode_gpu import fused_steps
        out, scores, _ = fused_steps(dec, enc.cuda(), ents, None if facts is None else facts.cuda(), MAX_LEN)
        assert torch.equal(seqs.t().contiguous(), out)
    worst = 0.0
    for b in range(enc.shape[0]):
        with torch.no_grad():
            seq, ref = R.predict(cfg, o["P"], enc[b:b + 1], MAX_LEN, ents[b:b + 1],
                                 None if facts is None else facts[b:b + 1], return_scores=True)
        assert seqs[:, b].cpu().tolist() == seq.view(-1).tolist(), (c.name, b)
        if scores is not None:
            n = ref.shape[0]
            err = (scores[b, :n].cpu() - ref).abs().max().item()
            worst = max(worst, err)
            assert err < 2e-4, (c.name, b, err)
    print("%s greedy: fused %s, worst step score error %.3e" % (c.name, c.decode, worst))
    if not c.decode:
        with pytest.raises(IckError, match="sizes the fused decode kernels support"):
            dec.predict_beam(enc.cuda(), MAX_LEN, ents, *fargs, beam_size=3)
        with pytest.raises(IckError, match="sizes the fused decode kernels support"):
            dec.predict_sample(enc.cuda(), MAX_LEN, ents, *fargs, num_samples=2, seed=1)


@pytest.mark.parametrize("name", MC.BEAM_CASES)
def test_beam_search_vs_cpu_beam_reference(name):
    """The check of tests/test_decode_gpu.py::test_beam_search_vs_cpu_beam_reference for one sample, beam 3."""
    c = MC.BY_NAME[name]
    assert c.decode
    o = oracle(c)
    P, cfg = o["P"], MC.oracle_config(c)
    dec = MC.build_decoder(c, P)
    enc, ents, facts = decode_inputs(c, 1)
    args = [enc.cuda(), MAX_LEN, ents] + ([facts.cuda()] if facts is not None else [])
    seq, score, allseq, allscore = dec.predict_beam(*args, beam_size=3, return_all=True)
    with torch.no_grad():
        ref_seq, ref_score, _ = R.predict_beam(cfg, P, enc, MAX_LEN, ents, facts, 3)
        mine = seq[:, 0].cpu().tolist()
        own = R.sequence_logprob(cfg, P, enc, ents, facts, mine, MAX_LEN)
    assert abs(score.item() - own) < 1e-3
    if mine == ref_seq.tolist():
        assert abs(score.item() - ref_score) < 1e-3
    else:
        assert own > ref_score - 1e-3, (mine, ref_seq.tolist())


# ------------------------------------------------------------------------------------------------ refused geometry
@pytest.mark.parametrize("geo", MC.REFUSED, ids=lambda g: "%s_d%d_H%d" % g[:3])
def test_head_wider_than_32_is_refused_by_name(geo):
    """Each entry point on its own, on a fresh model: the refusal comes before anything is launched."""
    from ick_amd.lib import IckError
    from ick_amd.training import TrainStep
    variant, d, H, FF_dec, FF_enc, NL = geo
    text = r"head width %d .*limit of 32" % (d // H)
    batch = MC.synth.make_batch(variant, B, L, K, MC.V, 0, SEED)
    enc_out = MC.synth.make_enc_out(B, SEED, emb_dim=d)
    with pytest.raises(IckError, match=text):
        MC.build_model(*geo)(*MC.step_args(batch, enc_out))
    with pytest.raises(IckError, match=text):
        MC.build_model(*geo).predict(enc_out.cuda(), MAX_LEN, batch["entities"])
    dec = MC.build_model(*geo).train()
    ts = TrainStep(dec, lr=MC.LR, grad_clip=MC.CLIP)
    with pytest.raises(IckError, match=text):
        ts(*MC.step_args(batch, enc_out))
    torch.cuda.synchronize()
