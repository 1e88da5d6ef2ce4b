"""Without a GPU: the decode envelope's case table (tests/decode_cases.py) against the launch plan the library reports
(ick_decode_plan, the function ick_decode_layers launches by), its coverage of every kernel instantiation, the size
limits, and -- on the float64 oracle only -- that the edge elements the envelope cases exist for move a checked score
by at least 10x the GPU test's tolerance when dropped (so a kernel that dropped them would fail those cases)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ick_amd.synth as synth
from oracle import restatement as R
from decode_cases import BY_NAME, CASES, REQUIRED, kernels_of, shape_params
from decode_ref import Fp64Decode, float64_default

TOL = 2e-4           # tests/test_decode_envelope_gpu.py: raw scores against fp64


@pytest.fixture(scope="module")
def ops():
    import ick_amd.build as build
    build.build()
    import ick_amd.ops as ops
    return ops


def test_case_plans_are_the_launchers(ops):
    for c in CASES:
        got = ops.decode_plan(c.R, c.rps, c.d, c.H, c.FF)
        assert {k: got[k] for k in c.plan} == c.plan, (c.name, got)
        assert got["fsel"] == (c.rps == 1)
        assert ops.decode_supported(c.d, c.H, c.FF, c.S, c.max_len), c.name
        if c.kind == "beam":
            assert ops.decode_beam_supported(c.Vx, c.rps), c.name
        if c.kind == "sample":
            assert ops.decode_sample_supported(c.Vx, c.rps), c.name


def test_table_covers_every_instantiation(ops):
    seen = {}
    for c in CASES:
        for k in kernels_of(c, ops.decode_plan(c.R, c.rps, c.d, c.H, c.FF)):
            seen.setdefault(k, []).append(c.name)
    missing = sorted(REQUIRED - set(seen))
    assert not missing, missing


def test_plan_edges(ops):
    # pick_group: the smallest G with H * ceil(R / G) <= 256 CUs
    assert [ops.decode_plan(R, 1, 300, 10, 512)["g_self"] for R in (25, 26, 50, 51, 100, 101)] == [1, 2, 2, 4, 4, 8]
    # the merged head takes at most 32 rows and 10 FFN chunks
    assert ops.decode_plan(32, 1, 300, 10, 640)["head_merged"] == 1
    assert ops.decode_plan(33, 1, 300, 10, 512)["head_merged"] == 0
    assert ops.decode_plan(3, 1, 300, 10, 644)["head_merged"] == 0
    # beams without a shared divisor read K / V per row
    assert ops.decode_plan(7, 7, 300, 10, 512)["cross_shared"] == 0
    assert ops.decode_plan(10, 10, 300, 10, 512)["g_cross"] == 5
    from ick_amd.lib import IckError
    for bad in ((0, 1, 300, 10, 512), (6, 4, 300, 10, 512), (3, 1, 324, 12, 512), (3, 1, 300, 7, 512),
                (3, 1, 300, 10, 1028), (3, 1, 300, 10, 0)):
        with pytest.raises(IckError):
            ops.decode_plan(*bad)


def test_envelope_limits(ops):
    assert ops.decode_supported(320, 16, 1024, 1024, 128)
    assert not ops.decode_supported(300, 10, 512, 1025, 16)
    assert not ops.decode_supported(300, 10, 512, 216, 129)
    assert not ops.decode_supported(324, 12, 512, 216, 16)
    assert ops.decode_beam_supported(65536, 8) and not ops.decode_beam_supported(65537, 8)
    assert not ops.decode_beam_supported(1000, 9)
    assert ops.decode_sample_supported(65536, 16) and not ops.decode_sample_supported(65537, 1)


# ------------------------------------------------------------------------------------------------ sensitivity
def case_model(name):
    c = BY_NAME[name]
    P = shape_params(c, synth.make_params(c.variant, c.V, c.seed, d=c.d, decoder_dim=c.FF, num_layers=c.layers))
    cfg = R.config_from_word_map(c.variant, synth.make_word_map(c.V), emb_dim=c.d, num_heads=c.H, num_layers=c.layers)
    ents = synth.make_entities(c.variant, c.B, c.K, c.V, c.seed)
    facts = synth.make_facts(c.variant, c.B, c.F, c.K, c.seed) if c.variant != "geo" else None
    enc = synth.make_enc_out(c.B, c.seed, emb_dim=c.d)
    return c, P, cfg, ents, facts, enc


def fed_words(c, steps, seed=0):
    """Teacher-forced input: <start>, then ordinary words (the scores of any fed prefix are checked the same way)."""
    g = torch.Generator().manual_seed(seed)
    fed = torch.randint(1, c.V - 3, (c.B, steps), generator=g)
    fed[:, 0] = c.V - 2
    return fed


def moved(a, b):
    return float(np.abs(a - b).max())


def test_sensitivity_last_memory_row():
    """S = 1024 (greedy_s1024_geo): the memory rows after LayerNorm all have the same norm and the random projections
    spread attention nearly evenly over 1024 keys -- dropping the last one moved the scores by only ~1.7e-3.  The case
    therefore scales the decoder's cross-attention queries by 8 (sharper attention): the drop then moves them by ~4.7e-3."""
    c, P, cfg, ents, facts, enc = case_model("greedy_s1024_geo")
    ref = Fp64Decode(cfg, P, enc, ents, facts)
    fed = fed_words(c, c.max_len)
    img = torch.arange(c.B)
    full = ref.scores(fed, img)
    ref.mem = ref.mem[:, :-1]
    assert moved(full, ref.scores(fed, img)) > 10 * TOL


def test_sensitivity_position_zero_from_the_last_step():
    """max_len = 128 (greedy_ml128): the key / value of position 0 as seen by the query of step 127.  Position 0 holds
    <start>, an embedding unlike any word's; its removal from the last query's causal window alone (every other query
    keeps it) moves step 127's scores by more than 10x the tolerance."""
    c, P, cfg, ents, facts, enc = case_model("greedy_ml128")
    ref = Fp64Decode(cfg, P, enc, ents, facts)
    fed = fed_words(c, c.max_len)
    img = torch.arange(c.B)
    full = ref.scores(fed, img, first=c.max_len - 1)
    mha = R.mha

    def mha_drop(xq, xkv, in_w, in_b, out_w, out_b, H, causal):
        if not causal:
            return mha(xq, xkv, in_w, in_b, out_w, out_b, H, causal)
        B, T, d = xq.shape
        dh = d // H
        q = F.linear(xq, in_w[:d], in_b[:d]).view(B, T, H, dh).transpose(1, 2) * (1.0 / math.sqrt(dh))
        k = F.linear(xkv, in_w[d:2 * d], in_b[d:2 * d]).view(B, T, H, dh).transpose(1, 2)
        v = F.linear(xkv, in_w[2 * d:], in_b[2 * d:]).view(B, T, H, dh).transpose(1, 2)
        neg = torch.full((T, T), float("-inf")).triu(1)
        neg[T - 1, 0] = float("-inf")                  # the last query does not see position 0
        att = (q @ k.transpose(-1, -2) + neg).softmax(dim=-1)
        return F.linear((att @ v).transpose(1, 2).reshape(B, T, d), out_w, out_b)

    R.mha = mha_drop
    try:
        dropped = ref.scores(fed, img, first=c.max_len - 1)
    finally:
        R.mha = mha
    assert moved(full, dropped) > 10 * TOL


def test_sensitivity_last_ffn_chunk():
    """FF = 100 (greedy_d260): the last chunk's 36 hidden units of every decoder layer (linear1 rows 64..99 -> 0)."""
    c, P, cfg, ents, facts, enc = case_model("greedy_d260")
    fed, img = fed_words(c, c.max_len), torch.arange(c.B)
    full = Fp64Decode(cfg, P, enc, ents, facts).scores(fed, img)
    Q = dict(P)
    for li in range(c.layers):
        pre = "transformer_decoder.layers.%d.linear1." % li
        Q[pre + "weight"] = P[pre + "weight"].clone()
        Q[pre + "weight"][64:] = 0
        Q[pre + "bias"] = P[pre + "bias"].clone()
        Q[pre + "bias"][64:] = 0
    assert moved(full, Fp64Decode(cfg, Q, enc, ents, facts).scores(fed, img)) > 10 * TOL


@pytest.mark.parametrize("block", ["self_attn", "multihead_attn"])
def test_sensitivity_last_head(block):
    """H = 16 (greedy_wide_b3): the last head's slice of the attention output (out_proj columns 300..319 -> 0) in every
    decoder layer."""
    c, P, cfg, ents, facts, enc = case_model("greedy_wide_b3")
    fed, img = fed_words(c, c.max_len), torch.arange(c.B)
    full = Fp64Decode(cfg, P, enc, ents, facts).scores(fed, img)
    dh = c.d // c.H
    Q = dict(P)
    for li in range(c.layers):
        name = "transformer_decoder.layers.%d.%s.out_proj.weight" % (li, block)
        Q[name] = P[name].clone()
        Q[name][:, c.d - dh:] = 0
    assert moved(full, Fp64Decode(cfg, Q, enc, ents, facts).scores(fed, img)) > 10 * TOL


def test_float64_default_is_restored():
    before = torch.get_default_dtype()
    with pytest.raises(RuntimeError):
        with float64_default():
            assert torch.get_default_dtype() == torch.float64
            raise RuntimeError("inside")
    assert torch.get_default_dtype() == before
