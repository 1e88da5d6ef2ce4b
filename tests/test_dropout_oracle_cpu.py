"""The masked oracle (oracle/restatement.py, drop=) on the CPU: that it changes nothing when it drops nothing, that it
drops where torch drops -- against oracle/stock.py's stock torch modules with their nn.Dropout replaced by modules that
play given masks back, and against F.multi_head_attention_forward for the attention-weight site --, and that the cases of
tests/test_dropout_oracle_gpu.py sit where float32 and float64 agree (no ReLU input within rounding of zero beyond the
allowance the GPU comparison grants)."""
import pytest
import torch
import torch.nn.functional as F
from torch import nn

import dropout_ref as DR
from decode_ref import float64_default, params64
from oracle import restatement as R
from oracle.stock import StockDecoder


def torch_masks(case, seed):
    """Random 0 or 1 / (1 - p) masks in float64, one per site, in the oracle's shapes."""
    g = torch.Generator().manual_seed(seed)
    masks = {}
    for e in DR.expected_table(case["variant"], case["B"], case["Fn"], case["rates"], 0):
        p = case["rates"][e["name"]]
        keep = torch.rand(e["shape"], generator=g, dtype=torch.float64) >= p
        masks[e["name"]] = keep.double() / (1.0 - p)
    return masks


@pytest.mark.parametrize("name", ["geo", "knowledge", "news"])
def test_all_ones_masks_change_nothing(name):
    """drop= with all-ones masks == drop=None, bit for bit: scores and every gradient (float32, as the goldens run it)."""
    case = DR.make_case(name)
    ones = {e["name"]: torch.ones(e["shape"], dtype=torch.float64)
            for e in DR.expected_table(case["variant"], case["B"], case["Fn"], case["rates"], 0)}
    # (deterministic algorithms: the scatter-add behind a repeated embedding lookup -- the news variant's name words --
    # otherwise sums in an order that changes from one run to the next, with or without masks)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        a = DR.masked_reference(case, None, torch.float32)
        b = DR.masked_reference(case, ones, torch.float32)
    finally:
        torch.use_deterministic_algorithms(before)
    assert torch.equal(a["scores"], b["scores"]) and a["loss"] == b["loss"]
    assert a["grads"].keys() == b["grads"].keys()
    for k in a["grads"]:
        assert torch.equal(a["grads"][k], b["grads"][k]), k


class Playback(nn.Module):
    """Stands where an nn.Dropout stood and multiplies by a given mask.  The stock modules are sequence-major
    ((T, B, d)); the masks are the oracle's, batch-major."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.transpose(0, 1)


def stock_with_playback(case, masks):
    m = StockDecoder(case["variant"], case["wm"], dropout=0.5, dropout_pos=0.1)
    with float64_default():
        m = m.double()
        m.load_reference_params(params64(case["P"]))
    m.train()
    m.pos_dropout = Playback(masks["pos"])
    stacks = [("e", m.transformer_encoder_entities), ("d", m.transformer_decoder)]
    if case["variant"] != "geo":
        stacks.append(("f", m.transformer_encoder_facts))
    for tag, stack in stacks:
        for li, layer in enumerate(stack.layers):
            layer.self_attn.dropout = 0.0            # attention dropout off: the fused attention cannot play a mask back
            if tag == "d":
                layer.multihead_attn.dropout = 0.0
            layer.dropout = Playback(masks[(tag, li, "ff")])
            for s in ("1", "2") + (("3",) if tag == "d" else ()):
                setattr(layer, "dropout" + s, Playback(masks[(tag, li, s)]))
    assert not any(isinstance(mod, nn.Dropout) for mod in m.modules())
    return m


@pytest.mark.parametrize("name", ["geo", "knowledge", "news", "geo_distinct_rates"])
def test_masked_oracle_equals_stock_modules_playing_the_masks_back(name):
    """Scores and every parameter gradient to 1e-10 relative, in float64, train mode.  The attention-weight sites are
    covered by test_attention_weight_site_is_where_torch_drops."""
    case = DR.make_case(name)
    masks = {k: v for k, v in torch_masks(case, 5).items() if k == "pos" or k[2] not in ("att", "sa", "ca")}
    ref = DR.masked_reference(case, masks)
    m = stock_with_playback(case, masks)
    b = case["batch"]
    with float64_default():
        scores, caps, dl = m(b["captions"], case["enc_out"].double(), b["caption_masks"], b["caption_lengths"],
                             b["entities"], b.get("facts"))
        loss = R.packed_ce_loss(case["cfg"], scores, caps, dl)
        loss.backward()
    assert dl == ref["decode_lengths"]
    err = (scores.detach() - ref["scores"]).abs().max().item()
    assert err <= 1e-10 * max(1.0, ref["scores"].abs().max().item()), err
    assert abs(loss.item() - ref["loss"]) <= 1e-10
    named = dict(m.named_parameters())
    rename = {"entity_encoder.type_embedding.weight": "type_embedding.weight"}
    # the masks must matter: the same model with nothing dropped gives other scores
    plain = DR.masked_reference(case, None)
    assert (plain["scores"] - ref["scores"]).abs().max().item() > 1e-2
    for k, gr in ref["grads"].items():
        got = named[rename.get(k, k)].grad
        assert got is not None, k
        e = (got - gr).abs().max().item()
        assert e <= 1e-10 * max(1e-3, gr.abs().max().item()), (k, e)


@pytest.mark.parametrize("causal", [False, True])
def test_attention_weight_site_is_where_torch_drops(monkeypatch, causal):
    """R.mha under a mask against F.multi_head_attention_forward(need_weights=True, training=True) with
    torch.nn.functional.dropout patched to play the same mask back: with need_weights=True torch computes
    softmax(q k^T) itself and calls the module-level dropout() on it before bmm(weights, v).  The patch asserts it was
    reached; a torch that routes this path elsewhere fails here instead of passing untested."""
    B, T, S, d, Hh, p = 3, 5, 7, 40, 4, 0.3
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    xq, xkv = r(B, T, d), (r(B, S, d) if not causal else None)
    if causal:
        xkv, S = xq, T
    in_w, in_b, out_w, out_b = (r(3 * d, d) / d ** 0.5).requires_grad_(True), r(3 * d).requires_grad_(True), \
        (r(d, d) / d ** 0.5).requires_grad_(True), r(d).requires_grad_(True)
    mask = (torch.rand(B, Hh, T, S, generator=g, dtype=torch.float64) >= p).double() / (1 - p)
    dy = r(B, T, d)
    calls = []

    def playback(x, p=0.5, training=True, inplace=False):
        calls.append(tuple(x.shape))
        assert tuple(x.shape) == (B * Hh, T, S) and training
        return x * mask.view(B * Hh, T, S)

    monkeypatch.setattr(F, "dropout", playback)
    attn_mask = torch.full((T, S), float("-inf"), dtype=torch.float64).triu(1) if causal else None
    out, _ = F.multi_head_attention_forward(
        xq.transpose(0, 1), xkv.transpose(0, 1), xkv.transpose(0, 1), d, Hh, in_w, in_b, None, None, False, p, out_w,
        out_b, training=True, need_weights=True, attn_mask=attn_mask)
    assert calls == [(B * Hh, T, S)]
    out.transpose(0, 1).backward(dy)
    ref_grads = [t.grad.clone() for t in (in_w, in_b, out_w, out_b)]
    for t in (in_w, in_b, out_w, out_b):
        t.grad = None
    with float64_default():
        mine = R.mha(xq, xkv, in_w, in_b, out_w, out_b, Hh, causal, drop=DR.player({"site": mask}), site="site")
    mine.backward(dy)
    assert (mine.detach() - out.detach().transpose(0, 1)).abs().max().item() < 1e-12
    for t, gr in zip((in_w, in_b, out_w, out_b), ref_grads):
        assert (t.grad - gr).abs().max().item() <= 1e-10 * max(1e-3, gr.abs().max().item())
    # the mask matters
    with float64_default():
        early = R.mha(xq, xkv, in_w, in_b, out_w, out_b, Hh, causal)
    assert (early.detach() - mine.detach()).abs().max().item() > 1e-2


def test_hash_mask_statistics():
    """The numpy restatement of ick_dropout_mask (compared with the kernel bit for bit on the GPU): keep rate, scale."""
    m = DR.hash_mask(1280, 300, 0.5, 1234, 7)
    assert set(m.unique().tolist()) == {0.0, 2.0} and abs((m > 0).float().mean().item() - 0.5) < 0.01
    m = DR.hash_mask(1280, 300, 0.1, 99, 1)
    assert abs((m > 0).float().mean().item() - 0.9) < 0.01 and abs(m.max().item() - 1 / 0.9) < 1e-6
    assert not torch.equal(DR.hash_mask(64, 64, 0.5, 1234, 7), DR.hash_mask(64, 64, 0.5, 1235, 7))
    assert torch.equal(DR.hash_mask(64, 64, 0.5, 1235, 7), DR.hash_mask(64, 64, 0.5, 1234 + 1, 7))


@pytest.mark.parametrize("name,seed,epochs", DR.GPU_POINTS, ids=lambda v: v if isinstance(v, str) else None)
def test_gpu_cases_sit_where_float32_and_float64_agree(name, seed, epochs):
    """The flip allowance of the GPU comparison is a cap, not an expectation: for every case, seed and counter value the
    GPU tests use, the float32 evaluation of the masked oracle on the CPU (the real masks, from hash_mask) already
    agrees with the float64 one within the GPU bars -- loss 2e-5, scores 2e-4, gradients 2e-3 with the allowance."""
    case = DR.make_case(name)
    for ep in epochs:
        table = DR.expected_table(case["variant"], case["B"], case["Fn"], case["rates"], seed)
        masks = DR.masks_from_table(table, ep, DR.hash_mask)
        r64 = DR.masked_reference(case, masks)
        r32 = DR.masked_reference(case, masks, torch.float32)
        what = "%s seed %#x counter %d (float32 oracle)" % (name, seed, ep)
        assert abs(r32["loss"] - r64["loss"]) < DR.LOSS_BAR, (what, r32["loss"], r64["loss"])
        DR.check_scores(r32["scores"], r64, what)
        DR.check_grads(r32["grads"], r64["grads"], what)
