"""Without a GPU: the model-geometry case table (tests/model_cases.py) -- that its tier columns are what the library's
predicates say, that every tier and both exact limits are in it, and that every case sits where the oracle's float32 and
float64 evaluations agree without any ReLU-flip allowance, so that the allowance the GPU comparison grants (at most two
hidden units of a linear1, in at most two tensors: tests/test_bench_sizes_gpu.py::run_train_step_vs_oracle) has nothing
of the reference's own to hide.

Float32 oracle step (R.forward, R.packed_ce_loss, backward; as reference_train_step runs it) against the float64 one,
measured on the CPU, worst over the case's tensors; gradients relative to max(1e-3, |ref|max), no hidden unit set aside:

  case             scores     loss       gradient (tensor)
  base             2.3e-06    4.4e-07    9.1e-07 (transformer_encoder_entities.layers.0.norm2.weight)
  deep_geo         2.1e-06    4.5e-07    8.2e-07 (transformer_decoder.layers.1.linear1.weight)
  deep_knowledge   9.0e-07    5.6e-07    1.2e-06 (transformer_decoder.layers.2.self_attn.in_proj_bias)
  single_layer     6.7e-07    6.3e-07    1.0e-06 (transformer_decoder.layers.0.linear2.weight)
  limit_geo        2.4e-06    1.1e-07    9.0e-07 (transformer_encoder_entities.layers.2.norm2.weight)
  limit_knowledge  1.5e-06    4.4e-07    1.1e-06 (transformer_encoder_entities.layers.1.self_attn.in_proj_weight)
  wide_ffn         1.6e-06    4.8e-08    1.1e-06 (transformer_decoder.layers.1.self_attn.in_proj_bias)
  wide_ctx         3.1e-06    4.7e-08    7.0e-07 (transformer_decoder.layers.0.multihead_attn.in_proj_weight)
  wide_model       1.8e-06    5.1e-07    5.5e-07 (transformer_encoder_entities.layers.1.norm1.weight)
  news_small       8.3e-08    4.6e-07    4.6e-07 (fc_entity.bias)
  odd_head         1.1e-06    2.7e-07    5.2e-07 (transformer_encoder_entities.layers.0.linear1.weight)
  unaligned        1.1e-06    8.7e-07    6.3e-07 (transformer_decoder.layers.1.norm3.weight)
  base_v152        3.0e-06    4.5e-07    9.5e-07 (transformer_decoder.layers.1.multihead_attn.in_proj_weight)
  single_layer_v152 9.6e-07   1.8e-07    2.2e-06 (transformer_decoder.layers.0.norm3.weight)
  limit_geo_v152   3.1e-06    5.4e-09    8.9e-07 (transformer_encoder_entities.layers.2.norm1.weight)
  limit_knowledge_v152 1.1e-06 6.1e-07   1.1e-06 (transformer_decoder.layers.0.self_attn.in_proj_weight)
  news_small_v152  8.0e-08    2.2e-07    4.9e-07 (transformer_decoder.layers.0.self_attn.in_proj_weight)
  odd_head_v152    1.1e-06    8.9e-08    5.1e-07 (transformer_encoder_entities.layers.1.norm2.weight)

(*_v152: the geometries that admit TrainStep's DerivedWeights, again at a vocabulary of 152 words; V = 150 admits none.)

The bars are a few times the worst of each column: scores 1e-5, loss 3e-6, gradients 5e-6.  They are two to three orders
below the GPU bars (2e-4, 2e-5, 2e-3).  (A 5-layer news model at this seed does flip one unit, 8.9e-5: not in the table.)
"""
import pytest
import torch

import model_cases as MC

SCORE_FLOOR, LOSS_FLOOR, GRAD_FLOOR = 1e-5, 3e-6, 5e-6


@pytest.fixture(scope="module")
def ops():
    import ick_amd.build as build
    build.build()
    import ick_amd.ops as ops
    return ops


def test_every_case_has_the_fixed_batch():
    import ick_amd.synth as synth
    assert all(c.V == MC.V for c in MC.CASES) and len(MC.CASES) == 12
    for c in MC.ALL_CASES:
        batch, enc_out = MC.make_inputs(c)
        assert batch["caption_lengths"].view(-1).tolist() == MC.LENGTHS
        assert tuple(enc_out.shape) == (MC.B, c.d, c.P)
        assert (("facts" in batch) == (c.variant != "geo")) and (c.Fn > 0) == (c.variant != "geo")
        assert c.d % c.H == 0 and c.d // c.H <= MC.MAX_HEAD
        shapes = synth.param_shapes(c.variant, c.V, d=c.d, decoder_dim=c.FF_dec, encoder_dim=c.FF_enc, num_layers=c.NL)
        assert shapes["transformer_decoder.layers.%d.linear1.weight" % (c.NL - 1)] == (c.FF_dec, c.d)
        assert shapes["transformer_encoder_entities.layers.0.linear1.weight"] == (c.FF_enc, c.d)
    for variant, d, H, FF_dec, FF_enc, NL in MC.REFUSED:
        assert d % H == 0 and d // H > MC.MAX_HEAD


@pytest.mark.parametrize("c", MC.ALL_CASES, ids=lambda c: c.name)
def test_tier_columns_by_hand(c):
    """The columns against the limits as this file's reader can check them (model_cases.py's docstring)."""
    chain = c.ff <= MC.MAX_K and c.d <= MC.MAX_D and max(3 * c.d, c.ff) <= MC.MAX_N2
    chain_bwd = chain and c.K0 <= MC.MAX_K0
    decode = c.d % 4 == 0 and 64 <= c.d <= 320 and c.H <= 16 and c.d // c.H <= 32 and c.FF_dec % 4 == 0 and \
        c.FF_dec <= 1024 and c.S <= 1024 and MC.MAX_LEN <= 128
    assert (c.chain, c.chain_bwd, c.decode) == (chain, chain_bwd, decode)
    # DerivedWeights._tables: every weight's row length % 4, fc_vocab's rows (its transposed planes) % 8
    assert c.derived == (c.chain_bwd and c.d % 4 == 0 and c.FF_dec % 4 == 0 and c.FF_enc % 4 == 0 and c.V % 8 == 0)


@pytest.mark.parametrize("c", MC.ALL_CASES, ids=lambda c: c.name)
def test_tier_columns_are_the_librarys(ops, c):
    """As DecoderTransformer.chain_supported() / chain_bwd_supported() ask (ff: the widest of both stacks)."""
    assert c.chain == ops.rowchain_supported(c.ff, c.d, max(3 * c.d, c.ff))
    assert c.chain_bwd == (c.chain and ops.rowchain_bwd_supported(max(3, 2 * c.NL) * c.d, c.d, c.ff))
    assert c.decode == bool(ops.L.load_raw().ick_decode_supported(c.d, c.H, c.FF_dec, c.S, MC.MAX_LEN))


def test_every_tier_and_both_limits_are_present(ops):
    tiers = {c.tier for c in MC.CASES}
    assert tiers == {"full", "mixed", "no_chains", "none", "partial"}, tiers
    # the vocabulary of the twelve keeps DerivedWeights away from all of them: the same geometries at an aligned one
    assert not any(c.derived for c in MC.CASES)
    assert {c.name for c in MC.DERIVED_CASES} == {n + "_v152" for n in ("base", "single_layer", "limit_geo",
                                                                       "limit_knowledge", "news_small", "odd_head")}
    assert all(c.derived and c.tier == "full" for c in MC.DERIVED_CASES)
    assert {c.name for c in MC.CASES if c.tier == "mixed"} == {"deep_geo", "deep_knowledge"}
    assert {c.name for c in MC.CASES if c.tier == "partial"} == {"unaligned"}
    assert {c.variant for c in MC.CASES} == {"geo", "knowledge", "news"}
    assert any(c.NL == 1 for c in MC.CASES) and any(c.P != 196 for c in MC.CASES)
    assert any(c.FF_dec == 1024 and c.decode for c in MC.CASES)        # 16 FFN chunks of the fused decode
    for name in ("limit_geo", "limit_knowledge"):
        c = MC.BY_NAME[name]
        assert c.tier == "full" and c.d == MC.MAX_D and c.K0 == MC.MAX_K0 and c.d // c.H == MC.MAX_HEAD
        # ... exactly ON the limits: one more column, or one more unit of width, and the library says no.  If a limit
        # constant moves, this fails: move the limit_* cases (and model_cases.MAX_*) with it.
        assert ops.rowchain_bwd_supported(c.K0, c.d, c.ff) and not ops.rowchain_bwd_supported(c.K0 + 1, c.d, c.ff)
        assert ops.rowchain_supported(c.ff, c.d, 3 * c.d) and not ops.rowchain_supported(c.ff, c.d + 1, 3 * c.d)
        assert ops.L.load_raw().ick_decode_supported(c.d, c.H, c.FF_dec, c.S, MC.MAX_LEN)
        assert not ops.L.load_raw().ick_decode_supported(c.d + 4, c.H, c.FF_dec, c.S, MC.MAX_LEN)
    assert ops.rowchain_supported(MC.MAX_K, 300, 900) and not ops.rowchain_supported(MC.MAX_K + 1, 300, 900)
    assert ops.DHP == MC.MAX_HEAD


@pytest.mark.parametrize("c", MC.ALL_CASES, ids=lambda c: c.name)
def test_float32_oracle_needs_no_relu_flip_allowance(c):
    P = MC.make_params(c)
    # (deterministic algorithms: the scatter-add behind a repeated embedding lookup otherwise sums in a changing order)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = MC.oracle_step(c, False, P)
        b = MC.oracle_step(c, True, P)
    finally:
        torch.use_deterministic_algorithms(before)
    assert a["decode_lengths"] == b["decode_lengths"] == sorted((n - 1 for n in MC.LENGTHS), reverse=True)
    v = b["valid"]
    s_err = (a["scores"].double()[v] - b["scores"][v]).abs().max().item()
    l_err = abs(a["loss"] - b["loss"])
    assert a["grads"].keys() == b["grads"].keys()
    worst = (0.0, None)
    for k, gr in b["grads"].items():
        scale = max(1e-3, gr.abs().max().item())
        err = (a["grads"][k].double() - gr).abs().max().item() / scale
        if err > worst[0]:
            worst = (err, k)
    print("%-16s %.1e    %.1e    %.1e (%s)" % (c.name, s_err, l_err, worst[0], worst[1]))
    assert s_err < SCORE_FLOOR, ("scores", s_err)
    assert l_err < LOSS_FLOOR, ("loss", l_err)
    assert worst[0] < GRAD_FLOOR, ("gradient",) + worst
