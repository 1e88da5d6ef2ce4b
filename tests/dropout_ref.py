"""Shared pieces of the dropout-on comparisons with the masked oracle (tests/test_dropout_oracle_cpu.py and
tests/test_dropout_oracle_gpu.py): the cases, the table of dropout sites of a step in the kernels' logical layouts, the
name -> float64 mask dictionary the oracle's drop= callable plays back, the masked reference step, and the comparisons.

Layouts (what the kernels index their masks by; element (row, col) of a site is hash index row * cols + col):
  "pos"                 rows b * L + t,            cols d      caption_embed / caption_embed_bwd
  (stack, li, "att")    rows (b * H + h) * T + t,  cols T      context-encoder self-attention, T = K or Fn
  ("d", li, "sa")       rows (b * H + h) * L + t,  cols L      decoder self-attention
  ("d", li, "ca")       rows (b * H + h) * L + t,  cols S      cross-attention over S = P + K + Fn memory rows
  (stack, li, "1|2|3")  rows b * T + t,            cols d      the add & norm launches / row chains
  (stack, li, "ff")     rows b * T + t,            cols FF     linear1's ReLU epilogue / the row chains' second GEMM
"""
from collections import OrderedDict

import numpy as np
import torch

import ick_amd.synth as synth
from decode_ref import float64_default, params64
from oracle import restatement as R

# The smallest model shapes the suite runs the whole model at.
D, H, FF, NL, P_IMG, L, K, V = 300, 10, 512, 3, 196, 9, 6, 160
LENGTHS = [9, 7, 5, 3, 2]           # strictly descending: the oracle's length sort is the identity

# name -> variant, Fn, seed of parameters and batch, caption lengths, rates: "reference" (dropout_dec = dropout_enc = 0.5,
# dropout_pos = 0.1, geo-aware/models.py:219) or "distinct"
CASES = {
    "geo": dict(variant="geo", Fn=0, seed=41, lengths=LENGTHS, rates="reference"),
    "knowledge": dict(variant="knowledge", Fn=5, seed=42, lengths=LENGTHS, rates="reference"),
    "news": dict(variant="news", Fn=5, seed=43, lengths=LENGTHS, rates="reference"),
    "geo_distinct_rates": dict(variant="geo", Fn=0, seed=44, lengths=LENGTHS, rates="distinct"),
    "geo_length1": dict(variant="geo", Fn=0, seed=45, lengths=[9, 7, 5, 3, 1], rates="reference"),
    # second batches of the TrainStep cases: the partner's parameters (pseed), a batch of their own
    "geo_b": dict(variant="geo", Fn=0, seed=46, pseed=41, lengths=[8, 6, 5, 4, 3], rates="reference"),
    "knowledge_b": dict(variant="knowledge", Fn=5, seed=47, pseed=42, lengths=[8, 6, 5, 4, 3], rates="reference"),
    "geo_length1_b": dict(variant="geo", Fn=0, seed=48, pseed=45, lengths=[8, 6, 4, 2, 1], rates="reference"),
    # the benchmark's composition: the (B, 2048, 14, 14) feature map through Encoder.conv1 inside the step
    "bench": dict(variant="geo", Fn=0, seed=49, lengths=[9, 7, 5, 3], rates="reference", feats=True),
    "bench_b": dict(variant="geo", Fn=0, seed=50, pseed=49, lengths=[8, 6, 4, 2], rates="reference", feats=True),
}


# The seeds the GPU tests run at.  Level A hands forward_with_tape a literal seed and a counter holding 3; the autograd
# bridge derives its seed from the module's call count (DecoderGraphFn.forward) and has no counter; TrainStep(seed=s)
# hands the kernels s * 2654435761 and its device counter.
TAPE_SEED, TAPE_EPOCH = 0x5EED1234, 3
STEP_SEED = 11


def bridge_seed(call, drop_seed=0x1234567):
    return (drop_seed * 2654435761 + call) & 0xFFFFFFFF


def step_seed(s=STEP_SEED):
    return s * 2654435761 & 0xFFFFFFFF


# (case, seed the kernels get, counter values the case's forward passes see): every point the GPU tests compare at.
# TrainStep runs batch a, b, a: the first case of a pair sees the counter at 0 and 2, the second at 1.
GPU_POINTS = [(n, TAPE_SEED, (TAPE_EPOCH,)) for n in ("geo", "knowledge", "news", "geo_distinct_rates")] + \
    [("geo", bridge_seed(1), (0,)), ("geo", bridge_seed(2), (0,))] + \
    [p for a, b in (("geo", "geo_b"), ("knowledge", "knowledge_b"), ("geo_length1", "geo_length1_b"), ("bench", "bench_b"))
     for p in ((a, step_seed(), (0, 2)), (b, step_seed(), (1,)))]


def with_lengths(batch, lengths, V):
    """The batch with its captions cut to the given lengths: <end> at length - 1, <pad> behind it, masks 0 from there on
    (what synth.make_captions writes for a caption of that length)."""
    caps, masks = batch["captions"].clone(), batch["caption_masks"].clone()
    B, Lc = caps.shape
    assert len(lengths) == B and max(lengths) <= Lc and min(lengths) >= 1
    lens = torch.tensor(lengths, dtype=torch.long).view(B, 1)
    pos = torch.arange(Lc).view(1, Lc)
    fresh = torch.randint(1, V - 4, (B, Lc), generator=torch.Generator().manual_seed(7))
    caps = torch.where((caps == 0) | (caps == V - 1), fresh, caps)     # positions the longer caption now reaches
    caps[:, 0] = V - 2
    caps = torch.where(pos == lens - 1, torch.full_like(caps, V - 1), caps)
    caps = torch.where(pos > lens - 1, torch.zeros_like(caps), caps)
    masks = torch.where(pos >= lens - 1, torch.zeros_like(masks), masks)
    masks = torch.where(caps < V, torch.zeros_like(masks), masks)
    out = dict(batch)
    out.update(captions=caps, caption_masks=masks, caption_lengths=lens)
    return out


def make_case(name):
    """-> dict(cfg, P, wm, batch, enc_out, rates, ...): parameters and one batch of a case, on the CPU in float32.  A
    feature-map case has feats (B, 2048, 14, 14) and conv1 = (weight, bias) instead of enc_out."""
    c = CASES[name]
    B = len(c["lengths"])
    pseed = c.get("pseed", c["seed"])
    P = synth.make_params(c["variant"], V, pseed)
    wm = synth.make_word_map(V)
    cfg = R.config_from_word_map(c["variant"], wm)
    batch = with_lengths(synth.make_batch(c["variant"], B, L, K, V, c["Fn"], c["seed"]), c["lengths"], V)
    out = dict(name=name, cfg=cfg, P=P, wm=wm, batch=batch, rates=rates_of(c["variant"], c["rates"]), B=B, Fn=c["Fn"],
               variant=c["variant"], pseed=pseed)
    if c.get("feats"):
        out.update(feats=synth.make_feats(B, c["seed"]), conv1=synth.make_conv1(pseed))
    else:
        out["enc_out"] = synth.make_enc_out(B, c["seed"])
    return out


# ------------------------------------------------------------------------------------------------ site names and rates
def site_names(variant):
    """The oracle's site names in the order the forward pass reaches them."""
    names = []
    for tag in ("e",) + (("f",) if variant != "geo" else ()):
        for li in range(NL):
            names += [(tag, li, "att"), (tag, li, "1"), (tag, li, "ff"), (tag, li, "2")]
    names.append("pos")
    for li in range(NL):
        names += [("d", li, s) for s in ("sa", "1", "ca", "2", "ff", "3")]
    return names


def rates_of(variant, kind):
    """name -> p.  "reference": 0.5 in every layer, 0.1 at the position encoder.  "distinct": every module its own rate,
    spread over 0.05 .. 0.6 so that neighbouring sites lie far apart (a swapped rate or keep-scale changes the numbers)."""
    names = site_names(variant)
    if kind == "reference":
        return OrderedDict((n, 0.1 if n == "pos" else 0.5) for n in names)
    n = len(names)
    assert n == 31      # 11 is coprime to it: the rates below are a permutation of 31 evenly spaced values
    return OrderedDict((nm, round(0.05 + 0.55 * ((i * 11) % n) / (n - 1), 3)) for i, nm in enumerate(names))


def _slot(dec, name):
    """(object, attribute) holding the rate of a site in a DecoderTransformer / its torch layers."""
    if name == "pos":
        return dec.pos_encoder.dropout, "p"
    tag, li, s = name
    stack = {"e": "transformer_encoder_entities", "f": "transformer_encoder_facts", "d": "transformer_decoder"}[tag]
    layer = getattr(dec, stack).layers[li]
    if s in ("att", "sa"):
        return layer.self_attn, "dropout"
    if s == "ca":
        return layer.multihead_attn, "dropout"
    if s == "ff":
        return layer.dropout, "p"
    return getattr(layer, "dropout" + s), "p"


def set_rates(dec, rates):
    for name, p in rates.items():
        obj, attr = _slot(dec, name)
        setattr(obj, attr, p)
    assert {n: getattr(*_slot(dec, n)) for n in rates} == dict(rates)      # no two names share a module
    return dec


# ------------------------------------------------------------------------------------------------ the site table
def _layouts(variant, B, Fn):
    """name -> (rows, cols, shape of the mask as the oracle multiplies it)."""
    S = P_IMG + K + Fn
    out = OrderedDict()
    for name in site_names(variant):
        if name == "pos":
            out[name] = (B * L, D, (B, L, D))
            continue
        tag, li, s = name
        T = {"e": K, "f": Fn, "d": L}[tag]
        if s in ("att", "sa"):
            out[name] = (B * H * T, T, (B, H, T, T))
        elif s == "ca":
            out[name] = (B * H * T, S, (B, H, T, S))
        elif s == "ff":
            out[name] = (B * T, FF, (B, T, FF))
        else:
            out[name] = (B * T, D, (B, T, D))
    return out


def _entry(name, drop, lay):
    return dict(name=name, drop=drop, rows=lay[0], cols=lay[1], shape=lay[2])


def table_from_tape(tape, variant, B, Fn):
    """The sites a forward_with_tape call handed out, read from its tape: [dict(name, drop, rows, cols, shape)], with
    drop = the (p, seed, site[, epoch tensor]) tuple the kernels got (None: the site's rate is 0)."""
    lay = _layouts(variant, B, Fn)
    key = {"att": "d_att", "sa": "d_sa", "ca": "d_ca", "ff": "d_ff", "1": "d1", "2": "d2", "3": "d3"}
    table = []
    for name in site_names(variant):
        if name == "pos":
            drop = tape.misc["d_pos"]
        else:
            tag, li, s = name
            t = tape.dec_layers[li] if tag == "d" else tape.enc_layers["entities" if tag == "e" else "facts"][li]
            drop = t[key[s]]
        table.append(_entry(name, drop, lay[name]))
    return table


def expected_table(variant, B, Fn, rates, seed):
    """The same table without a GPU, from the order DropSites hands ids out in (1, 2, ... along site_names()): what the
    CPU checks of a case's seeds use."""
    lay = _layouts(variant, B, Fn)
    table, nxt = [], 0
    for name in site_names(variant):
        p = rates[name]
        drop = None
        if p > 0.0:
            nxt += 1
            drop = (float(p), seed, nxt)
        table.append(_entry(name, drop, lay[name]))
    return table


def triples(table):
    return [(e["name"], None if e["drop"] is None else tuple(e["drop"][:3])) for e in table]


def assert_sites_distinct(table):
    ids = [e["drop"][2] for e in table if e["drop"] is not None]
    assert len(ids) == len(set(ids)), ("two dropout sites of one step share an id", ids)
    seeds = {e["drop"][1] for e in table if e["drop"] is not None}
    assert len(seeds) == 1, seeds


def hash_mask(rows, cols, p, seed, site, device=None):
    """ick_dropout_mask restated with numpy (csrc/common.h: drop_hash, make_dropout): keep iff
    murmur3_finaliser(idx * 0x9E3779B1 ^ (seed + site * 0x85EBCA6B)) >= uint32(p * 2^32), kept elements 1 / (1 - p) in
    float32.  The GPU tests check it against the kernel; the CPU tests draw the cases' real masks with it."""
    p32 = np.float32(p)
    thr = np.uint32(min(np.float32(p32 * np.float32(4294967296.0)), np.float32(4294967040.0)))
    scale = np.float32(1.0) / (np.float32(1.0) - p32)
    idx = np.arange(rows * cols, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    key = np.uint64((int(seed) + int(site) * 0x85EBCA6B) & 0xFFFFFFFF)
    x = ((idx * np.uint64(0x9E3779B1)) & m32) ^ key
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & m32
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & m32
    x ^= x >> np.uint64(16)
    out = np.where(x >= np.uint64(thr), scale, np.float32(0.0)).astype(np.float32)
    return torch.from_numpy(out).view(rows, cols)


def masks_from_table(table, epoch_value, mask_fn):
    """name -> float64 mask (CPU) in the oracle's shape.  mask_fn(rows, cols, p, seed, site) is ops.dropout_mask on the
    GPU or hash_mask; the effective seed is seed + the step counter's value (epoch_seed() in csrc/common.h)."""
    masks = {}
    for e in table:
        if e["drop"] is None:
            continue
        p, seed, site = e["drop"][:3]
        m = mask_fn(e["rows"], e["cols"], p, (seed + epoch_value) & 0xFFFFFFFF, site)
        masks[e["name"]] = m.detach().cpu().double().view(e["shape"])
    return masks


def player(masks):
    """The oracle's drop= callable: multiplies by the site's mask (a site without one is left alone)."""
    def drop(name, x):
        m = masks.get(name)
        return x if m is None else x * m.to(x.dtype)
    return drop


# ------------------------------------------------------------------------------------------------ the masked reference
def masked_reference(case, masks, dtype=torch.float64):
    """One forward + packed cross entropy + backward of the masked oracle.  -> dict(loss, scores (B, L, Vx), dscores
    (the gradient of the token-mean loss with respect to the scores), grads name -> tensor, decode_lengths, valid (B, L)
    bool: the positions the loss reads).  A feature-map case goes through R.feat_proj in the same precision."""
    cfg, batch = case["cfg"], case["batch"]
    if "feats" in case:
        with torch.no_grad():
            enc_out = R.feat_proj(case["feats"].to(dtype), case["conv1"][0].to(dtype), case["conv1"][1].to(dtype))
    else:
        enc_out = case["enc_out"]
    P = case["P"] if dtype == torch.float32 else params64(case["P"])
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
    if cfg.has_facts:
        Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
    stages = {}

    def run():
        scores, caps, dl = R.forward(cfg, Pr, batch["captions"], enc_out.to(dtype), batch["caption_masks"],
                                     batch["caption_lengths"], batch["entities"], batch.get("facts"), stages,
                                     drop=player(masks) if masks is not None else None)
        scores.retain_grad()
        loss = R.packed_ce_loss(cfg, scores, caps, dl)
        loss.backward()
        return scores, dl, loss

    if dtype == torch.float64:
        with float64_default():
            scores, dl, loss = run()
    else:
        scores, dl, loss = run()
    B = scores.shape[0]
    assert torch.equal(stages["sort_ind"], torch.arange(B)), "the case's lengths must be strictly descending"
    valid = torch.arange(scores.shape[1]).view(1, -1) < torch.tensor(dl).view(B, 1)
    grads = {k: (v.grad if v.grad is not None else torch.zeros_like(v)).detach()
             for k, v in Pr.items() if not k.startswith("fact_encoder.")}
    return dict(loss=loss.item(), scores=scores.detach(), dscores=scores.grad.detach(), grads=grads,
                decode_lengths=dl, valid=valid)


# ------------------------------------------------------------------------------------------------ the comparisons
LOSS_BAR, GRAD_BAR, SCORE_BAR = 2e-5, 2e-3, 2e-4


def check_scores(got, ref, what):
    """Scores at every valid position: |got - ref| < 2e-4 * max(1, |ref|max)."""
    v = ref["valid"]
    r = ref["scores"][v].double()
    err = (got.detach().cpu().double()[v] - r).abs().max().item() if v.any() else 0.0
    bar = SCORE_BAR * max(1.0, r.abs().max().item() if v.any() else 0.0)
    print("%s: scores max err %.3e (bar %.3e)" % (what, err, bar))
    assert err < bar, (what, "scores", err, bar)


def check_grads(mine, ref_grads, what, clamp=None):
    """Every parameter gradient: max |mine - ref| / max(1e-3, |ref|max) < 2e-3 per tensor.  The allowance of
    tests/test_bench_sizes_gpu.py::run_train_step_vs_oracle for a ReLU input within rounding of zero: in at most two
    linear1 tensors, at most two hidden units (rows) are set aside, and the tensor must still agree in norm to 5e-3.
    mine: name -> tensor (any device); clamp: the element clamp both sides went through (TrainStep's grad_clip)."""
    flipped, worst = {}, (0.0, None)
    for k, gr in ref_grads.items():
        got = mine[k].detach().cpu().double()
        gr = gr.double()
        if clamp is not None:
            gr = gr.clamp(-clamp, clamp)
        d = (got - gr).abs()
        scale = max(1e-3, gr.abs().max().item())
        if d.max().item() / scale >= GRAD_BAR and k.endswith(("linear1.weight", "linear1.bias")):
            rows = d.view(d.shape[0], -1).max(dim=1).values
            top = rows.topk(2)
            bad = top.indices[top.values / scale >= GRAD_BAR]
            flipped[k] = bad.tolist()
            d = d.clone()
            d[bad] = 0
            assert (got - gr).norm().item() <= 5e-3 * gr.norm().item(), (what, "gradient norm", k)
        err = d.max().item() / scale
        if err > worst[0]:
            worst = (err, k)
        assert err < GRAD_BAR, (what, "gradient", k, err)
    print("%s: worst gradient rel err %.3e (%s), set aside %s" % (what, worst[0], worst[1], flipped))
    assert len(flipped) <= 2, (what, flipped)
    return flipped
