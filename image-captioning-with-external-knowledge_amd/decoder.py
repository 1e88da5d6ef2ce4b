"""Encoder / DecoderTransformer engine shared by the three drop-in `models` modules.

Mirrors the reference's operator interface for the hot path:
    models.Encoder(encoded_image_size=14, emb_dim=300, encoder_dim=2048)         geo-aware/models.py:9-60
    models.DecoderTransformer(word_map, emb_dim, decoder_dim, encoder_dim, num_heads, num_layers,
                              dropout_dec=0.5, dropout_enc=0.5, dropout_pos=0.1)  geo-aware/models.py:212-254
    decoder(captions, encoder_out, caption_masks, caption_lengths, entities[, facts])
        -> (scores (B,L,V+K[+F]) in length-sorted order, captions_sorted, decode_lengths)   :315-361
    decoder.predict(encoder_out, max_pred_len, entities[, facts]) -> LongTensor (max_pred_len, B) :363-443
The module tree (sub-module and parameter names) is the reference's, so its whole-object
checkpoints (geo-aware/utils.py:32-49) unpickle into these classes and state_dicts interchange.
torch.nn modules are used ONLY as parameter containers; every forward computation below runs
in libick_amd.so (HIP, gfx950) through ops.py.  There is no CPU / PyTorch fallback.
"""
import dataclasses
import math
import os
import struct
import weakref
from typing import NamedTuple, Optional

import torch
from torch import nn

from . import ops
from .lib import IckError
from .weights import WeightImages, vocab_planes_wanted

VARIANT_TYPE_OFFSET = {"geo": 4, "knowledge": 6, "news": 5}
VARIANT_NUM_TYPES = {"geo": 1000, "knowledge": 1000, "news": 20}
VARIANT_NUM_PREDICATES = {"geo": 0, "knowledge": 3000, "news": 3500}


def _sinusoid_table(max_len, d):
    """PositionEncoder buffer (geo-aware/models.py:199-205), shape (max_len, 1, d)."""
    pos = torch.arange(max_len, dtype=torch.float32).unsqueeze(1)
    freq = torch.exp(torch.arange(0, d, 2, dtype=torch.float32) * (-math.log(10000.0) / d))
    table = torch.zeros(max_len, d)
    table[:, 0::2] = torch.sin(pos * freq)
    table[:, 1::2] = torch.cos(pos * freq)
    return table.unsqueeze(1)


class _GraphedCall:
    """hipGraph capture of a pure-device function of static-shaped tensors (torch.cuda.CUDAGraph is the
    HIP graph API on ROCm).  The kernels are launched through ctypes on torch's current stream, which is the
    capture stream inside torch.cuda.graph(), so the whole launch sequence -- ~75 kernels for a teacher-forced
    forward, ~900 for a 20-step greedy decode -- replays from one hipGraphLaunch with no host work in between."""

    def __init__(self, fn, example_inputs):
        self.static_in = [None if t is None else t.contiguous().clone() for t in example_inputs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):            # warm-up off the capture: lazy hipFuncSetAttribute, caches
            for _ in range(2):
                fn(*self.static_in)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        with ops.capture(self.graph):
            self.static_out = fn(*self.static_in)

    def __call__(self, *inputs):
        copy_inputs(self.static_in, inputs)
        self.graph.replay()
        return self.static_out


def copy_inputs(static, inputs):
    """Refresh a graph's input buffers: one foreach call instead of a Python-level copy_ per tensor (the host is
    on the critical path here: forward() has just synchronised for the length sort)."""
    # an input that IS its static buffer (the caller filled it in place) needs no copy
    pairs = [(d, s) for d, s in zip(static, inputs) if d is not None and not (
        s.is_cuda and s.data_ptr() == d.data_ptr() and s.shape == d.shape and s.dtype == d.dtype)]
    if not pairs:
        return
    dst = [d for d, _ in pairs]
    src = [s for _, s in pairs]
    if all(s.is_cuda and s.shape == d.shape and s.dtype == d.dtype and s.is_contiguous() for d, s in zip(dst, src)):
        ops.copy_batch(dst, src)          # one launch for all of them
    elif all(s.is_cuda and s.shape == d.shape for d, s in zip(dst, src)):
        torch._foreach_copy_(dst, src, non_blocking=True)
    else:
        for d, s in zip(dst, src):
            d.copy_(s, non_blocking=True)


class DropSites:
    """Hands out (p, seed, site) triples: one site id per dropout call site of a step, so the backward
    kernels regenerate exactly the masks the forward used (ick_dropout_mask in include/ick_amd.h)."""

    def __init__(self, seed, enabled, epoch=None):
        self.seed, self.enabled, self.next, self.epoch = seed, enabled, 0, epoch

    def site(self, p):
        if not self.enabled or p <= 0.0:
            return None
        self.next += 1
        return (float(p), self.seed, self.next, self.epoch) if self.epoch is not None else \
            (float(p), self.seed, self.next)


_NO_DROPOUT = DropSites(0, False)

# return_attention: the largest weight buffer a decode call may allocate, (max_len, rows, layers, H, S) fp32
ATTENTION_MAX_BYTES = 1 << 30


class _BeamResult(NamedTuple):
    """What DecoderTransformer._predict_beam_device returns; None: not part of this search."""
    best: torch.Tensor                  # (B, max_len) the best hypothesis of every caption
    score: torch.Tensor                 # (B) its log-probability
    all: torch.Tensor                   # (B, beam, max_len) every final hypothesis
    all_scores: torch.Tensor            # (B, beam)
    attn: Optional[torch.Tensor] = None             # cross-attention weights of the best (attention=True)
    all_attn: Optional[torch.Tensor] = None         # ... of every final hypothesis
    group: Optional[torch.Tensor] = None            # (B * G, max_len) the best of each group (groups > 1)
    group_score: Optional[torch.Tensor] = None      # (B * G)
    group_attn: Optional[torch.Tensor] = None


def _attention_check(what, max_len, rows, layers, H, S):
    nbytes = 4 * max_len * rows * layers * H * S
    if nbytes > ATTENTION_MAX_BYTES:
        raise IckError("%s(return_attention=True) would need a %.0f MB weight buffer (max_len %d x rows %d x layers %d x "
                       "heads %d x S %d fp32); the limit is ATTENTION_MAX_BYTES = %d MB"
                       % (what, nbytes / 2 ** 20, max_len, rows, layers, H, S, ATTENTION_MAX_BYTES >> 20))


def _zero_after_end(attn, tokens, end_token):
    """Zero, in place, the steps of every row after its first <end> in tokens (rows, max_len); attn (max_len, rows, ...).
    The <end> step itself keeps the weights that chose it."""
    is_end = (tokens == end_token).to(torch.int32)
    live = (torch.cumsum(is_end, dim=1) - is_end) == 0            # no <end> before this step
    attn.mul_(live.t().to(attn.dtype).reshape(live.shape[1], live.shape[0], *([1] * (attn.dim() - 2))))
    return attn


def split_attention(attn, P, K, F=0):
    """Views of a cross-attention weight tensor (..., S) along its memory axis S = P + K + F, in the decode K/V order
    [image ; entities ; facts]: {"image": (..., P), or (..., h, w) when P = h * w is a perfect square (the encoder's
    h x w grid, row-major), "entities": (..., K), "facts": (..., F)}."""
    if attn.shape[-1] != P + K + F:
        raise IckError("split_attention: the last axis has %d rows, P + K + F = %d" % (attn.shape[-1], P + K + F))
    img = attn[..., :P]
    side = math.isqrt(P)
    if side * side == P:
        img = img.unflatten(-1, (side, side))
    return {"image": img, "entities": attn[..., P:P + K], "facts": attn[..., P + K:]}


RULES_MAX_NGRAM = 8


def length_penalty_table(alpha, max_len):
    """GNMT length penalty lp[L] = ((5 + L) / 6) ** alpha for L = 0 .. max_len, computed in float64 and rounded to
    fp32 (lp[0] = 1 is never a real length: it keeps an unused beam slot's key at -inf)."""
    lp = [((5.0 + L) / 6.0) ** float(alpha) for L in range(max_len + 1)]
    lp[0] = 1.0
    return torch.tensor(lp, dtype=torch.float64).to(torch.float32)


def check_rules(what, max_len, Vx, length_penalty=0.0, no_repeat_ngram_size=0, min_len=0):
    """Validate the decoding rules of predict_beam / predict_sample (IckError); True when any rule is on."""
    if isinstance(length_penalty, bool) or not isinstance(length_penalty, (int, float)) or \
            not math.isfinite(length_penalty) or length_penalty < 0:
        raise IckError("%s needs a finite length_penalty >= 0 (0 = off)" % what)
    if isinstance(no_repeat_ngram_size, bool) or not isinstance(no_repeat_ngram_size, int) or \
            not 0 <= no_repeat_ngram_size <= RULES_MAX_NGRAM:
        raise IckError("%s needs an integer no_repeat_ngram_size in 0..%d (0 = off)" % (what, RULES_MAX_NGRAM))
    if isinstance(min_len, bool) or not isinstance(min_len, int) or not 0 <= min_len <= max_len:
        raise IckError("%s needs an integer min_len in 0..max_pred_len (0 = off)" % what)
    on = length_penalty != 0 or no_repeat_ngram_size != 0 or min_len != 0
    if on and Vx <= max_len:
        raise IckError("%s: decoding rules need V+K+F (%d) > max_pred_len (%d), so that some token stays allowed"
                       % (what, Vx, max_len))
    return on


def check_diversity(what, beam_size, num_beam_groups=1, diversity_penalty=0.0):
    """Validate the diverse beam search arguments of predict_beam (IckError); True when there is more than one group."""
    if isinstance(num_beam_groups, bool) or not isinstance(num_beam_groups, int) or num_beam_groups < 1 or \
            (num_beam_groups > 1 and (num_beam_groups > beam_size or beam_size % num_beam_groups != 0)):
        raise IckError("%s needs an integer num_beam_groups in 1..beam_size that divides beam_size (%d)"
                       % (what, beam_size))
    if isinstance(diversity_penalty, bool) or not isinstance(diversity_penalty, (int, float)) or \
            not math.isfinite(diversity_penalty) or diversity_penalty < 0:
        raise IckError("%s needs a finite diversity_penalty >= 0" % what)
    return num_beam_groups > 1


FORCE_MAX = 8


def check_force(what, B, Vx, special, force_tokens=None, num_beam_groups=1):
    """Validate predict_beam's force_tokens (IckError): None, or an integer tensor / nested list (B, C), C in 1..8, of
    column ids in [0, Vx) with -1 for an empty slot; `special` holds the ids that cannot be forced (<start>, <end>,
    <pad>).  Returns None, or the int32 CPU tensor (B, 8) padded with -1 that becomes the device input."""
    if force_tokens is None:
        return None
    if isinstance(num_beam_groups, int) and num_beam_groups > 1:
        raise IckError("%s: force_tokens does not compose with num_beam_groups > 1" % what)
    ft = force_tokens
    if not torch.is_tensor(ft):
        try:
            ft = torch.tensor(ft)
        except (TypeError, ValueError, RuntimeError):
            raise IckError("%s needs force_tokens as an integer tensor or nested list (B, 1..%d)" % (what, FORCE_MAX))
    if ft.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or ft.dim() != 2 or \
            ft.shape[0] != B or not 1 <= ft.shape[1] <= FORCE_MAX:
        raise IckError("%s needs force_tokens as an integer tensor or nested list (B = %d, 1..%d)"
                       % (what, B, FORCE_MAX))
    ft = ft.detach().to("cpu", torch.int64)                  # one small read-back per call
    if bool((ft < -1).any()) or bool((ft >= Vx).any()):
        raise IckError("%s: force_tokens holds column ids in [0, V+K+F = %d) or -1 for an empty slot" % (what, Vx))
    for tok in special:
        if bool((ft == tok).any()):
            raise IckError("%s: <start>, <end> and <pad> cannot be forced" % what)
    out = torch.full((B, FORCE_MAX), -1, dtype=torch.int32)
    out[:, :ft.shape[1]] = ft.to(torch.int32)
    return out


BIAS_MAX = 64


def bias_tensors(B, ids, vals):
    """The device inputs of a column bias as CPU tensors: int32 ids (B, 64) padded with -1 and fp32 values (B, 64), 0 in
    every empty slot; ids (B, C) or (C,) integer and vals of the same shape, C <= 64 (a (C,) pair goes to every caption)."""
    ids = torch.as_tensor(ids).to(torch.int64)
    vals = torch.as_tensor(vals).to(torch.float32)
    if ids.dim() == 1:
        ids, vals = ids.view(1, -1).expand(B, -1), vals.view(1, -1).expand(B, -1)
    out_i = torch.full((B, BIAS_MAX), -1, dtype=torch.int32)
    out_v = torch.zeros(B, BIAS_MAX, dtype=torch.float32)
    out_i[:, :ids.shape[1]] = ids.to(torch.int32)
    out_v[:, :ids.shape[1]] = torch.where(ids >= 0, vals, torch.zeros_like(vals))
    return out_i, out_v


def _bias_input(bias, device):
    """bias_tensors()' pair as ONE int32 (2, B, 64) device tensor, ids over the values' bits: one host-to-device copy per
    call, one static input of the decode graph."""
    return torch.stack([bias[0], bias[1].view(torch.int32)]).to(device)


def _bias_views(packed):
    """The (B, 64) ids and values of a _bias_input()."""
    return packed[0], packed[1].view(torch.float32)


def check_column_bias(what, B, Vx, word_map, column_bias=None, num_beam_groups=1, force_tokens=None):
    """Validate the column_bias of predict_beam / predict_sample (IckError): None; a dict {column id or word of
    word_map: value} for every caption; or a pair (ids, values) of an integer tensor / nested list (B, C) or (C,), C in
    1..64, and a float one of the same shape.  Ids are force_tokens' columns, -1 = an empty slot (its value is ignored);
    a value is a finite float or -inf.  Returns None or bias_tensors()' padded (B, 64) pair."""
    if column_bias is None:
        return None
    if isinstance(num_beam_groups, int) and num_beam_groups > 1:
        raise IckError("%s: column_bias does not compose with num_beam_groups > 1" % what)
    if force_tokens is not None:
        raise IckError("%s: column_bias does not compose with force_tokens" % what)
    shape_msg = "%s needs column_bias as a dict {column: value} or a pair (ids, values) of shape (B = %d, 1..%d) or " \
                "(1..%d,)" % (what, B, BIAS_MAX, BIAS_MAX)
    if isinstance(column_bias, dict):
        ids, vals = [], []
        for key, v in column_bias.items():
            if isinstance(key, str):
                if key not in word_map:
                    raise IckError("%s: column_bias names the unknown word %r" % (what, key))
                key = word_map[key]
            if isinstance(key, bool) or not isinstance(key, int) or isinstance(v, bool) or \
                    not isinstance(v, (int, float)):
                raise IckError(shape_msg)
            ids.append(key)
            vals.append(float(v))
        if len(set(ids)) != len(ids):
            raise IckError("%s: column_bias names a column twice" % what)
        column_bias = (ids, vals)
    if not isinstance(column_bias, (tuple, list)) or len(column_bias) != 2:
        raise IckError(shape_msg)
    ids, vals = column_bias
    try:
        ids = ids if torch.is_tensor(ids) else torch.tensor(ids)
        vals = vals if torch.is_tensor(vals) else torch.tensor(vals, dtype=torch.float32)
    except (TypeError, ValueError, RuntimeError):
        raise IckError(shape_msg)
    if ids.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or \
            not (vals.dtype.is_floating_point or vals.dtype in (torch.int32, torch.int64)) or \
            ids.dim() not in (1, 2) or tuple(vals.shape) != tuple(ids.shape) or \
            (ids.dim() == 2 and ids.shape[0] != B) or not 1 <= ids.shape[-1] <= BIAS_MAX:
        raise IckError(shape_msg)
    ids = ids.detach().to("cpu", torch.int64)                # one small read-back per call
    vals = vals.detach().to("cpu", torch.float32)
    if bool((ids < -1).any()) or bool((ids >= Vx).any()):
        raise IckError("%s: column_bias holds column ids in [0, V+K+F = %d) or -1 for an empty slot" % (what, Vx))
    used = ids >= 0
    if bool((used & (torch.isnan(vals) | (vals == float("inf")))).any()):
        raise IckError("%s: a column_bias value is a finite float or -inf" % what)
    rows = ids.view(1, -1) if ids.dim() == 1 else ids
    vrows = vals.view(1, -1) if vals.dim() == 1 else vals
    never = {word_map[w] for w in ("<start>", "<pad>") if w in word_map and 0 <= word_map[w] < Vx}
    for row, vrow in zip(rows.tolist(), vrows.tolist()):
        cols = [c for c in row if c >= 0]
        if len(set(cols)) != len(cols):
            raise IckError("%s: column_bias names a column twice in one caption's row" % what)
        if len(never | {c for c, v in zip(row, vrow) if c >= 0 and v == float("-inf")}) >= Vx:
            raise IckError("%s: column_bias bans every column of a caption" % what)
    return bias_tensors(B, ids, vals)


def check_prefix(what, B, Vx, max_len, word_map, prefix=None, force_tokens=None, bias=None):
    """Validate the prefix of predict_beam / predict_sample (IckError): None, or an integer tensor / nested list (B, Pn) or
    (Pn,), 1 <= Pn <= max_len (a (Pn,) value goes to every caption), of column ids in [0, Vx) numbered as force_tokens
    numbers them, -1 padding a shorter prefix at its end; in nested lists a string is a word of word_map, and rows of
    unequal length are padded.  <start>, <end> and <pad> cannot be given.  bias: check_column_bias()'s pair or None -- a
    -inf bias on a column of the same caption's prefix is refused.  Returns None, or the device form as a CPU tensor:
    int32 (B, max_len), the forced column of every step and -1 for a free step (its shape does not depend on Pn)."""
    if prefix is None:
        return None
    if force_tokens is not None:
        raise IckError("%s: prefix does not compose with force_tokens" % what)
    shape_msg = "%s needs prefix as an integer tensor or nested list (B = %d, 1..max_pred_len = %d) or " \
                "(1..%d,)" % (what, B, max_len, max_len)
    px = prefix
    if not torch.is_tensor(px):
        def word(v):
            if isinstance(v, str):
                if v not in word_map:
                    raise IckError("%s: prefix names the unknown word %r" % (what, v))
                return word_map[v]
            return v
        if isinstance(px, (list, tuple)) and len(px) > 0 and all(isinstance(r, (list, tuple)) for r in px):
            width = max(len(r) for r in px)
            px = [[word(v) for v in r] + [-1] * (width - len(r)) for r in px]
        elif isinstance(px, (list, tuple)):
            px = [word(v) for v in px]
        try:
            px = torch.tensor(px)
        except (TypeError, ValueError, RuntimeError):
            raise IckError(shape_msg)
    if px.dtype not in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8) or px.dim() not in (1, 2) or \
            (px.dim() == 2 and px.shape[0] != B) or not 1 <= px.shape[-1] <= max_len:
        raise IckError(shape_msg)
    px = px.detach().to("cpu", torch.int64)                  # one small read-back per call
    if px.dim() == 1:
        px = px.view(1, -1).expand(B, -1)
    if bool((px < -1).any()) or bool((px >= Vx).any()):
        raise IckError("%s: prefix holds column ids in [0, V+K+F = %d), or -1 behind a shorter prefix" % (what, Vx))
    for w in ("<start>", "<end>", "<pad>"):
        if w in word_map and bool((px == word_map[w]).any()):
            raise IckError("%s: %s cannot be part of a prefix" % (what, w))
    free = px < 0
    if bool((free[:, :-1] & ~free[:, 1:]).any()):
        raise IckError("%s: prefix holds a column id behind a -1 (-1 only pads a prefix at its end)" % what)
    if bias is not None:
        never = torch.where(bias[1] == float("-inf"), bias[0].to(torch.int64), torch.full_like(bias[0], -2, dtype=torch.int64))
        clash = (px.unsqueeze(2) == never.unsqueeze(1)).any(dim=2)                          # (B, Pn)
        if bool(clash.any()):
            b, t = [int(v) for v in clash.nonzero()[0]]
            raise IckError("%s: column_bias bans (-inf) column %d, which caption %d's prefix holds at step %d"
                           % (what, int(px[b, t]), b, t))
    out = torch.full((B, max_len), -1, dtype=torch.int32)
    out[:, :px.shape[1]] = px.to(torch.int32)
    return out


def check_score_args(what, has_facts, captions, encoder_out, caption_masks, caption_lengths, entities, facts=None,
                     image_index=None, top_k=5):
    """Validate the arguments of score_captions (IckError); shapes only, so it runs on tensors of any device.  Returns
    (R, L, n_img): captions, caption length, image rows."""
    if isinstance(top_k, bool) or not isinstance(top_k, int) or top_k < 1:
        raise IckError("%s needs an integer top_k >= 1" % what)
    if captions.dim() != 2 or captions.shape[0] < 1 or captions.shape[1] < 2:
        raise IckError("%s needs captions (R, L) with R >= 1 and L >= 2, got %s" % (what, tuple(captions.shape)))
    R, Lc = captions.shape
    if tuple(caption_masks.shape) != (R, Lc):
        raise IckError("%s: caption_masks must have the captions' shape (%d, %d), got %s"
                       % (what, R, Lc, tuple(caption_masks.shape)))
    if caption_lengths.numel() != R:
        raise IckError("%s: caption_lengths must hold %d lengths, got %s" % (what, R, tuple(caption_lengths.shape)))
    if encoder_out.dim() not in (3, 4):
        raise IckError("%s needs a token-major encoder_out (B, d, P) or a 4-D feature map" % what)
    n_img = encoder_out.shape[0]
    if entities.dim() != 3 or entities.shape[0] != n_img:
        raise IckError("%s: entities must be (%d, K, features), got %s" % (what, n_img, tuple(entities.shape)))
    if has_facts and (facts is None or facts.dim() != 3 or facts.shape[0] != n_img or facts.shape[2] != 3):
        raise IckError("%s: facts must be (%d, F, 3)" % (what, n_img))
    if image_index is None:
        if n_img != R:
            raise IckError("%s: %d captions over %d image rows need image_index" % (what, R, n_img))
    else:
        if encoder_out.dim() == 4:
            raise IckError("image_index needs a token-major encoder_out (B, d, P), not a 4-D feature map")
        if not torch.is_tensor(image_index) or image_index.dtype not in (torch.int32, torch.int64) or \
                tuple(image_index.shape) != (R,):
            raise IckError("image_index must be an integer tensor of shape (%d,)" % R)
    return R, Lc, n_img


@dataclasses.dataclass
class CaptionScores:
    """score_captions' result, device tensors in the caller's caption order: log_prob (R,) = sum of the caption's token
    log-probabilities, tokens (R,) int32 = how many were scored, token_log_probs / rank / best (R, L-1) per position
    (0 / -1 / -1 past the caption; rank 0 = the target is the argmax, best = the argmax column), and the totals over all
    captions loss_sum (= -sum of log-probabilities), count, top1_hits, topk_hits, (1,) float32 each."""
    log_prob: torch.Tensor
    tokens: torch.Tensor
    token_log_probs: torch.Tensor
    rank: torch.Tensor
    best: torch.Tensor
    loss_sum: torch.Tensor
    count: torch.Tensor
    top1_hits: torch.Tensor
    topk_hits: torch.Tensor


def _caption_scores(flat, R, T):
    """CaptionScores as views of one flat float32 buffer of 3 * R * T + 2 * R + 4 words (one allocation, one copy out of
    a graph's static result)."""
    n = R * T
    i32 = flat.view(torch.int32)
    return CaptionScores(log_prob=flat[3 * n:3 * n + R], tokens=i32[3 * n + R:3 * n + 2 * R],
                         token_log_probs=flat[:n].view(R, T), rank=i32[n:2 * n].view(R, T),
                         best=i32[2 * n:3 * n].view(R, T), loss_sum=flat[3 * n + 2 * R:][0:1],
                         count=flat[3 * n + 2 * R:][1:2], top1_hits=flat[3 * n + 2 * R:][2:3],
                         topk_hits=flat[3 * n + 2 * R:][3:4])


def rules_tensor(max_len, length_penalty=0.0, no_repeat_ngram_size=0, min_len=0, device="cuda"):
    """The device input of the rules (lib.DecodeRules): int32 (4 + max_len + 1) = the rule words
    {no_repeat_ngram_size, min_len, length penalty on, 0} followed by the fp32 bits of length_penalty_table()."""
    words = torch.tensor([no_repeat_ngram_size, min_len, int(length_penalty != 0), 0], dtype=torch.int32)
    lp = length_penalty_table(length_penalty, max_len).view(torch.int32)
    return torch.cat([words, lp]).to(device)


def _rules_struct(rules, lens=None):
    """lib.DecodeRules over a rules_tensor() (and a beam's (R) int32 length buffer)."""
    from . import lib as L
    r = L.DecodeRules()
    r.words, r.lp = rules.data_ptr(), rules.data_ptr() + 16
    r.len = None if lens is None else lens.data_ptr()
    return r


def _wb(linear):
    return linear.weight.detach(), linear.bias.detach()


def _ln(norm):
    """The (gamma, beta, eps) arguments of ops.add_layernorm / ops.rowchain_fwd."""
    return norm.weight.detach(), norm.bias.detach(), norm.eps


def _with_stats(r, save):
    """ops.add_layernorm's result as (out, mean, rstd); the statistics are None unless save_stats was set."""
    return r if save else (r, None, None)


class PositionEncoder(nn.Module):
    """Holds the sinusoid buffer `pe` and the dropout rate; applied inside ick_caption_embed."""

    def __init__(self, emb_dim, dropout, max_len=5000):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.register_buffer("pe", _sinusoid_table(max_len, emb_dim))


class EntityEncoder(nn.Module):
    """Parameter holder for the entity-type embedding (computation: ick_entity_encode)."""

    def __init__(self, emb_dim, type_embedding):
        super().__init__()
        self.emb_dim = emb_dim
        self.type_embedding = type_embedding


class FactEncoder(nn.Module):
    """Parameter holder for the predicate embedding (computation: ick_fact_encode)."""

    def __init__(self, emb_dim, predicate_embedding):
        super().__init__()
        self.emb_dim = emb_dim
        self.predicate_embedding = predicate_embedding


class CaptionEmbedder(nn.Module):
    def __init__(self, vocab_size):
        super().__init__()
        self.vocab_size = vocab_size


# Device-side caches a module keeps in its __dict__ (captured graphs, packed / pre-split weight copies, pinned staging):
# never part of a pickle (checkpoints pickle whole modules, geo-aware/utils.py:32-46) or of a deep copy -- they are rebuilt
# on first use.
_CACHE_KEYS = ("_graphs", "_images", "_len_pin", "_idx_pin", "_plist", "_pin_ev", "_chain_ok", "_chain_bwd_ok", "_ps_cache",
               "_last_static", "_enc", "_score_gmap_checked")


def _state_without_caches(module):
    return {k: v for k, v in module.__dict__.items() if k not in _CACHE_KEYS}


class _Conv1Fn(torch.autograd.Function):
    """Encoder.conv1 (1x1 convolution = GEMM over the NCHW map) with its backward on the same HIP GEMM:
    dW = dY^T . X, db = column sums of dY (riding on that GEMM), dX = dY . W (only when the trunk is being
    fine-tuned).  Used when gradients are wanted (fine_tune_encoder=True, geo-aware/train.py:93-100,282-294)."""

    @staticmethod
    def forward(ctx, feats, weight, bias, w_ps=None):
        B, Cc, Hh, Ww = feats.shape
        P, d = Hh * Ww, weight.shape[0]
        out = torch.empty(B, P, d, device=feats.device, dtype=torch.float32)
        ops.gemm_raw(feats, weight.detach().view(d, Cc), out, B * P, d, Cc, 1, P, Cc, 1, d, bias=bias, a_grp=P, a_gs=Cc * P,
                     b_ps=w_ps)
        ctx.save_for_backward(feats, weight)
        return out

    @staticmethod
    def backward(ctx, dout):
        feats, weight = ctx.saved_tensors
        B, Cc, Hh, Ww = feats.shape
        P, d = Hh * Ww, weight.shape[0]
        dy = dout.contiguous().view(B * P, d)
        dw = db = dx = None
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[2]:
            # token-major copy of the map: the reduction index (sample, position) of dW needs one uniform stride
            xt = feats.view(B, Cc, P).permute(0, 2, 1).contiguous().view(B * P, Cc)
            dw = torch.zeros(d, Cc, device=feats.device, dtype=torch.float32)
            db = torch.zeros(d, device=feats.device, dtype=torch.float32)
            ops.gemm_raw(dy, xt, dw, d, Cc, B * P, 1, d, 1, Cc, Cc, atomic=True, split_k=ops.wgrad_split(B * P, d, Cc),
                         colsum_a=db)
            dw = dw.view_as(weight)
        if ctx.needs_input_grad[0]:
            dxt = torch.empty(B * P, Cc, device=feats.device, dtype=torch.float32)
            w2 = weight.view(d, Cc)
            ops.gemm_raw(dy, w2, dxt, B * P, Cc, d, d, 1, 1, Cc, Cc)           # dX = dY . W  (B k-major)
            dx = dxt.view(B, P, Cc).permute(0, 2, 1).reshape(B, Cc, Hh, Ww)
        return dx, dw, db, None


class Encoder(nn.Module):
    """Image encoder (geo-aware/models.py:9-60): [ResNet-101 trunk -> AdaptiveAvgPool2d(14)] -> conv1 (1x1,
    2048 -> emb_dim) -> view (B, emb_dim, 196).

    The hot path starts at the 14x14x2048 feature map (BASELINE configs use precomputed ResNet-101 features):
    forward() takes either that map (B, 2048, H, W) -- conv1 runs as a HIP GEMM straight off the NCHW layout -- or
    raw images (B, 3, H, W), which first go through the trunk (stock torch.nn / MIOpen, resnet.py; built on first
    use or with with_trunk=True; there is no network here, so pretrained weights come from load_state_dict /
    resnet.load_torchvision_state_dict).  Returns (B, emb_dim, 196) like the reference; the storage is token-major
    (B, 196, emb_dim) -- the layout the decoder's cross-attention K/V projection streams -- exposed through a
    permuted view, so the decoder consumes it without a copy."""

    def __init__(self, encoded_image_size=14, emb_dim=300, encoder_dim=2048, with_trunk=None):
        super().__init__()
        self.emb_dim = emb_dim
        self.encoder_dim = encoder_dim
        self.encoded_image_size = encoded_image_size
        self.with_trunk = with_trunk
        if with_trunk:
            self._build_trunk()
        self.conv1 = nn.Conv2d(encoder_dim, emb_dim, 1)
        self.fine_tune()

    def _build_trunk(self):
        from .resnet import resnet101_trunk
        dev = self.conv1.weight.device if "conv1" in self._modules else None
        self.resnet = resnet101_trunk()
        self.adaptive_pool = nn.AdaptiveAvgPool2d((self.encoded_image_size, self.encoded_image_size))
        if dev is not None:
            self.resnet.to(dev)
        self.resnet.train(self.training)
        # a trunk built on first use takes the fine_tune() setting that was asked for before it existed.  Its
        # parameters are new, so an optimizer built earlier does not hold them: train.py builds the trunk up front
        # (with_trunk=True) whenever fine_tune_encoder is set.
        self.fine_tune(self.__dict__.get("_fine_tune", True))

    def features(self, images):
        """images (B, 3, H, W) -> (B, 2048, 14, 14): trunk + adaptive pooling (geo-aware/models.py:42-43)."""
        if "resnet" not in self._modules:
            if self.with_trunk is False:
                raise IckError("this Encoder was built with with_trunk=False: pass the (B, %d, H, W) feature map"
                               % self.encoder_dim)
            self._build_trunk()
        return self.adaptive_pool(self.resnet(images))

    def forward(self, feats):
        if feats.dim() == 4 and feats.shape[1] == 3 and self.encoder_dim != 3:
            feats = self.features(feats)
        if feats.dim() != 4 or feats.shape[1] != self.encoder_dim:
            raise IckError("Encoder.forward expects images (B, 3, H, W) or the (B, %d, H, W) feature map"
                           % self.encoder_dim)
        if feats.dtype != torch.float32:          # a float16 feature file: the kernels read float32
            feats = feats.float()
        feats = feats.contiguous()
        B, Cc, Hh, Ww = feats.shape
        P = Hh * Ww
        d = self.emb_dim
        if torch.is_grad_enabled() and (feats.requires_grad or self.conv1.weight.requires_grad):
            return _Conv1Fn.apply(feats, self.conv1.weight, self.conv1.bias, self.conv1_presplit()).permute(0, 2, 1)
        out = torch.empty(B, P, d, device=feats.device, dtype=torch.float32)
        w = self.conv1.weight.detach().view(d, Cc)
        ops.gemm_raw(feats, w, out, B * P, d, Cc, 1, P, Cc, 1, d, bias=self.conv1.bias.detach(),
                     a_grp=P, a_gs=Cc * P, b_ps=self.conv1_presplit())
        return out.permute(0, 2, 1)

    def __getstate__(self):
        return _state_without_caches(self)

    def conv1_presplit(self):
        """The pre-split copy of conv1's (emb_dim, encoder_dim) weight for ick_gemm's b_ps (refreshed in place when the
        weight changes; None in the exact-fp32 product mode)."""
        w = self.conv1.weight
        return ops.presplit_cached(self, "conv1", w.detach().view(w.shape[0], -1),
                                   (w._version, w.data_ptr(), self.__dict__.get("_param_epoch", 0)))

    def invalidate_caches(self):
        """Call after conv1's weight was written behind torch's version counters (through .data, a fused optimizer): the
        pre-split copy is rebuilt on the next use and graphs that captured this encoder are re-captured."""
        self.__dict__["_param_epoch"] = self.__dict__.get("_param_epoch", 0) + 1

    def fine_tune(self, fine_tune=True):
        """Convolutional blocks 2-4 of the trunk train iff fine_tune (geo-aware/models.py:49-60); conv1 is left
        as the reference leaves it (always requires_grad).  Without a trunk the setting is remembered and applied when
        the trunk is built."""
        self.__dict__["_fine_tune"] = bool(fine_tune)
        if "resnet" not in self._modules:
            return
        for p in self.resnet.parameters():
            p.requires_grad = False
        for c in list(self.resnet.children())[5:]:
            for p in c.parameters():
                p.requires_grad = fine_tune


class DecoderTransformer(nn.Module):
    variant = "geo"
    use_hip_graphs = True   # inference forward / predict replay a captured hipGraph per input shape
    fused_decode = True     # predict(): fused per-block decode kernels (csrc/decode.hip) when the sizes allow
    fuse_select = True      # ... with the greedy selection folded into the next step's first launch

    def __init__(self, word_map, emb_dim, decoder_dim, encoder_dim, num_heads, num_layers, dropout_dec=0.5,
                 dropout_enc=0.5, dropout_pos=0.1):
        super().__init__()
        v = self.variant
        self.word_map = word_map
        self.vocab_size = len(word_map)
        self.emb_dim = emb_dim
        self.softmax = nn.Softmax(dim=-1)
        self.lookahead_mask = None
        self.pos_encoder = PositionEncoder(emb_dim, dropout_pos)
        self.transformer_decoder = nn.TransformerDecoder(
            nn.TransformerDecoderLayer(emb_dim, num_heads, decoder_dim, dropout_dec), num_layers)
        self.transformer_encoder_entities = nn.TransformerEncoder(
            nn.TransformerEncoderLayer(emb_dim, num_heads, encoder_dim, dropout_enc), num_layers,
            enable_nested_tensor=False)
        if v != "geo":
            self.transformer_encoder_facts = nn.TransformerEncoder(
                nn.TransformerEncoderLayer(emb_dim, num_heads, encoder_dim, dropout_enc), num_layers,
                enable_nested_tensor=False)
        self.word_embedding = nn.Embedding(self.vocab_size, emb_dim)
        self.entity_encoder = EntityEncoder(
            emb_dim, nn.Embedding(VARIANT_NUM_TYPES[v], emb_dim - VARIANT_TYPE_OFFSET[v]))
        if v != "geo":
            self.num_predicates = VARIANT_NUM_PREDICATES[v]
            self.predicate_embedding = nn.Embedding(self.num_predicates, emb_dim)
            self.fact_encoder = FactEncoder(emb_dim, self.predicate_embedding)
        self.caption_embedder = CaptionEmbedder(self.vocab_size)
        self.fc_vocab = nn.Linear(emb_dim, self.vocab_size)
        self.fc_entity = nn.Linear(emb_dim, 1)
        if v != "geo":
            self.fc_fact = nn.Linear(emb_dim, 1)
            self.fc_predicate = nn.Linear(self.num_predicates, emb_dim)
        self.init_weights()

    # ------------------------------------------------------------------ reference API surface
    def init_weights(self):
        """U(-0.1, 0.1) weights / zero bias on the score-head linears (geo-aware/models.py:264-272)."""
        heads = [self.fc_vocab, self.fc_entity]
        if self.variant != "geo":
            heads += [self.fc_fact, self.fc_predicate]
        with torch.no_grad():
            for m in heads:
                m.bias.zero_()
                m.weight.uniform_(-0.1, 0.1)

    def load_pretrained_embeddings(self, embeddings):
        self.word_embedding.weight = nn.Parameter(embeddings)
        self.invalidate_caches()      # a new Parameter object: cached parameter list, packed weights, graphs

    def fine_tune_embeddings(self, fine_tune=True):
        for p in self.word_embedding.parameters():
            p.requires_grad = fine_tune

    def _generate_square_subsequent_mask(self, sz):
        """Kept for API parity (geo-aware/models.py:256-262); the HIP attention kernel applies the
        causal mask from indices and never reads this tensor."""
        return torch.full((sz, sz), float("-inf")).triu(1)

    # ------------------------------------------------------------------ helpers
    @property
    def has_facts(self):
        return self.variant != "geo"

    @property
    def num_heads(self):
        return self.transformer_decoder.layers[0].self_attn.num_heads

    def _dropout_rates(self):
        return (self.pos_encoder.dropout.p, self.transformer_decoder.layers[0].dropout.p,
                self.transformer_encoder_entities.layers[0].dropout.p)

    def _wants_grad(self):
        return torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())

    def __getstate__(self):
        return _state_without_caches(self)

    def invalidate_caches(self):
        """Call after parameters were modified outside torch's version tracking (the fused Adam kernel
        writes the flat bucket directly): every captured graph is dropped and the re-laid-out weight copies
        (weight_images) become stale -- they keep their buffers, which captured training and SCST graphs write."""
        self.__dict__["_param_epoch"] = self.__dict__.get("_param_epoch", 0) + 1
        for k in ("_graphs", "_plist", "_last_static"):
            self.__dict__.pop(k, None)

    def _token_major(self, encoder_out):
        """(B, d, P) -> contiguous (B, P, d) storage.  Our Encoder already stores token-major."""
        B, d, P = encoder_out.shape
        if encoder_out.stride() == (P * d, 1, d):
            return encoder_out.permute(0, 2, 1)
        return encoder_out.permute(0, 2, 1).contiguous()

    def attach_encoder(self, encoder):
        """Let forward() / predict() / predict_beam() take the (B, 2048, 14, 14) feature map in place of encoder_out:
        Encoder.conv1 then runs INSIDE the captured graph, on the main stream beside the context-encoder chain on the
        side stream -- instead of a stand-alone launch the graph (and with it the context chain, which never reads the
        image) has to wait for.  Same kernels, same numbers (tests/test_round4_gpu.py); cfg2 forward 0.76 -> ~0.6 ms,
        cfg5 greedy 2.15 -> ~1.9 ms.  encoder_out tensors (B, emb_dim, 196) keep working as before.  The encoder is not
        registered as a submodule (state_dict / parameters() of the decoder stay the reference's)."""
        self.__dict__["_enc"] = encoder
        return self

    def _image_input(self, encoder_out):
        """-> (enc_in, P): the token-major (B, P, d) view of an encoder output, or -- with an attached Encoder and the
        hipGraph paths on -- the float32 feature map itself (4-D) for _encode_context to project inside the graph."""
        if encoder_out.dim() == 4:
            enc = self.__dict__.get("_enc")
            if enc is None:
                raise IckError("a 4-D input is a feature map: attach_encoder(encoder) first, or pass encoder(feats)")
            if self.use_hip_graphs and not self._wants_grad() and not os.environ.get("ICK_NO_FUSED_ENCODER") and \
                    encoder_out.shape[1] == enc.encoder_dim:
                feats = encoder_out if encoder_out.dtype == torch.float32 else encoder_out.float()
                enc.conv1_presplit()       # refreshed in place, outside the captured graph, if conv1's weight changed
                return feats.contiguous(), feats.shape[2] * feats.shape[3]
            encoder_out = enc(encoder_out)
        t = self._token_major(encoder_out)
        return t, t.shape[1]

    def weight_images(self):
        """The owner of every re-laid-out copy of this decoder's weights (weights.WeightImages).  One object per parameter
        storage: when a parameter has moved (.to(), a replaced Parameter) a new one is built and the captured graphs,
        which read the old one's buffers, go with it."""
        wi = self.__dict__.get("_images")
        if wi is None or not wi.matches():
            if wi is not None:
                self.__dict__.get("_graphs", {}).clear()       # (in place: _graphed may be holding the dictionary)
            wi = self.__dict__["_images"] = WeightImages(self)
        return wi

    def _packed_cross_kv(self):
        """[K_0;V_0;K_1;V_1;...] rows of the layers' cross-attention in_proj (weight, bias): one GEMM projects the memory."""
        wi = self.weight_images().current("kv")
        return wi.wkv, wi.bkv

    def _vocab_presplit(self, rows):
        """Pre-split copy of fc_vocab's weight for the vocabulary GEMM over `rows` rows (None below 256 rows)."""
        return self.weight_images().planes("vocab_ps", rows)

    def _pred_wt(self):
        return self.weight_images().current("pred_wt").pred_wt

    def _decode_pack(self):
        """Transposed out_proj / linear2 weights of the decoder layers for the fused decode kernels (one input
        feature per row, so a workgroup's slice of the out-projection is read coalesced)."""
        return self.weight_images().current("decode").decode

    def chain_supported(self):
        """Do the layer widths fit the row-chain kernel (ick_rowchain_supported)?  ICK_NO_ROWCHAIN=1 turns it off."""
        cached = self.__dict__.get("_chain_ok")
        if cached is None:
            d = self.emb_dim
            ff = max(l.linear1.out_features for st in (self.transformer_decoder, self.transformer_encoder_entities)
                     for l in st.layers)
            cached = (not os.environ.get("ICK_NO_ROWCHAIN")) and ops.rowchain_supported(ff, d, max(3 * d, ff))
            self.__dict__["_chain_ok"] = cached
        return cached

    def chain_bwd_supported(self):
        cached = self.__dict__.get("_chain_bwd_ok")
        if cached is None:
            d = self.emb_dim
            ff = max(l.linear1.out_features for st in (self.transformer_decoder, self.transformer_encoder_entities)
                     for l in st.layers)
            cached = self.chain_supported() and not os.environ.get("ICK_NO_ROWCHAIN_BWD") and \
                ops.rowchain_bwd_supported(max(3, 2 * len(self.transformer_decoder.layers)) * d, d, ff)
            self.__dict__["_chain_bwd_ok"] = cached
        return cached

    def _encode_context(self, enc_tok, entities, facts, gmap):
        """Entity / fact encoders, context transformers and the all-layer cross K/V projection.
        Returns (entities_encoded, facts_encoded, kv, contexts); kv is head-major
        (B, 2*layers, H, S, 32): segment 2i = keys of decoder layer i, 2i+1 = its values, over the
        memory rows [196 image positions ; entity rows ; fact rows]."""
        d = self.emb_dim
        H = self.num_heads
        feats = None
        if enc_tok.dim() == 4:
            # the feature map itself (attach_encoder): Encoder.conv1 runs below, beside the context chain
            feats, enc = enc_tok, self.__dict__["_enc"]
            B, Cc = feats.shape[:2]
            P = feats.shape[2] * feats.shape[3]
            enc_tok = torch.empty(B, P, d, device=feats.device, dtype=torch.float32)
        else:
            B, P, _ = enc_tok.shape
        K = entities.shape[1]
        Fn = facts.shape[1] if self.has_facts else 0
        ee, fe = self._encode_entities(entities, facts)
        # refreshed (if stale) on the main stream, before the side stream forks
        wi = self.weight_images().current("kv", *(("chain",) if self.chain_supported() else ()))
        wkv, bkv, wkv_ps = wi.wkv, wi.bkv, wi.planes("kv_ps")
        pk = wi.chain if self.chain_supported() else None
        nseg = wkv.shape[0] // d
        S = P + K + Fn
        kv = torch.empty(B, nseg, H, S, ops.DHP, device=enc_tok.device, dtype=torch.float32)
        # The context-encoder chain (small, latency-bound kernels) runs on a second stream beside the
        # large image-row projection; both write disjoint key/value rows of `kv`.  The caller joins the
        # side stream before the first cross-attention (`side.join()`).
        side = ops.SideStream(priority=-1)
        ctx = [None, None]
        # (Measured and removed in round 4: only layer 0's image K/V in front of the decoder and the later layers' on the side
        # stream behind the context chain -- forward 0.695 -> 0.826 ms, a second fork / join pair makes the hipGraph
        # executor start the context chain only after conv1)

        def entity_chain():
            ops.stamp("side: context chain starts")
            # beside Encoder.conv1 / the image K/V projection: the 8-wave form finds room on a CU that hosts bulk GEMM
            # workgroups (as in the training step)
            ctx[0] = self._context_stack(self.transformer_encoder_entities, ee, pk, "e", slim=True)
            ops.project_heads(ctx[0], wkv, bkv, nseg, H, S, out=kv, s0=P, grp=K)
            side.signal("ctx")
            ops.stamp("side: context chain done")

        def fact_chain():
            ctx[1] = self._context_stack(self.transformer_encoder_facts, fe, pk, "f")
            ops.project_heads(ctx[1], wkv, bkv, nseg, H, S, out=kv, s0=P + K, grp=Fn)

        # dependency point now, enqueued after the main stream's next kernel: in a captured graph the main chain
        # must be the first child of the fork node (see SideStream)
        side.submit(entity_chain, ee, fe, kv, wkv, bkv)

        def conv1():
            c1 = enc.conv1
            ops.gemm_raw(feats, c1.weight.detach().view(d, Cc), enc_tok, B * P, d, Cc, 1, P, Cc, 1, d,
                         bias=c1.bias.detach(), a_grp=P, a_gs=Cc * P, b_ps=enc.conv1_presplit())

        if self.has_facts:
            # the fact chain runs on the main stream beside the entity chain (two chains of small kernels overlap well,
            # a chain beside the large projection does not: cfg4 forward 1.84 -> 1.72 ms), the image rows follow
            fact_chain()
            side.flush()
            if feats is not None:
                conv1()
            ops.project_heads(enc_tok, wkv, bkv, nseg, H, S, out=kv, s0=0, grp=P, a_gmap=gmap, a_gs=enc_tok.stride(0),
                              w_ps=wkv_ps)
        else:
            # image rows (gathered through gmap = sort order)
            if feats is not None:
                conv1()
                side.flush()       # the context chain starts beside Encoder.conv1
            ops.project_heads(enc_tok, wkv, bkv, nseg, H, S, out=kv, s0=0, grp=P, a_gmap=gmap, a_gs=enc_tok.stride(0),
                              w_ps=wkv_ps)
            side.flush()
        ops.stamp("main: image K/V projection done")
        ctx_e, ctx_f = ctx
        return ee, fe, kv, (ctx_e, ctx_f), side

    # ------------------------------------------------------------------ layer forward (inference and training.py)
    # Shared by the inference forward and training.forward_with_tape.  pk: the packed row-chain weights (weight_images().chain) ->
    # each out-projection / linear2 runs in one ops.rowchain_fwd launch together with its add & norm and the next
    # projection; pk None -> the separate GEMM / add & norm kernels.  ds hands out the dropout sites (training only).
    # save: keep what the backward pass needs -- o_out, the norm statistics and the attention lse -- in the layer's dict.
    def _encode_entities(self, entities, facts):
        """-> (entities_encoded (B, K, d), facts_encoded (B, F, d) or None)."""
        ee = ops.entity_encode(self.variant, entities, self.entity_encoder.type_embedding.weight.detach(), self.emb_dim,
                               facts=facts if self.has_facts else None,
                               word_emb=self.word_embedding.weight.detach() if self.variant == "news" else None)
        fe = ops.fact_encode(facts, ee, self.predicate_embedding.weight.detach()) if self.has_facts else None
        return ee, fe

    def _context_stack(self, stack, x, pk, tag, out=None, slim=False, ds=_NO_DROPOUT, tape=None):
        """Post-LN encoder stack (entities: tag "e", facts: "f") on x (B, T, d).  With pk, two row-chain launches per
        layer: out-projection + norm1 + linear1, linear2 + norm2 + the next layer's in_proj.  `out`: (B, T, d) view (rows
        of the memory buffer) that receives the last layer's output.  slim: the chains' 8-wave form.  tape: a list ->
        each layer's dict is appended to it."""
        H, d = self.num_heads, self.emb_dim
        B, T, _ = x.shape
        save = tape is not None
        n = len(stack.layers)
        qkv = None
        for li, layer in enumerate(stack.layers):
            t = {"x": x, "d_att": ds.site(layer.self_attn.dropout), "d1": ds.site(layer.dropout1.p),
                 "d_ff": ds.site(layer.dropout.p), "d2": ds.site(layer.dropout2.p)}
            if qkv is None:
                qkv = ops.project_heads(x, layer.self_attn.in_proj_weight.detach(), layer.self_attn.in_proj_bias.detach(),
                                        3, H, T)
            t["qkv"] = qkv
            t["sa"] = torch.empty_like(x)
            t["lse"] = torch.empty(B * H * T, device=x.device, dtype=torch.float32) if save else None
            ops.attention_heads(t["qkv"], t["qkv"], t["sa"], H, d // H, T, T, 0, 1, 2, lse=t["lse"], drop=t["d_att"])
            last = li == n - 1
            x, qkv = self._layer_tail(layer, t, "sa", layer.self_attn.out_proj, "so", 1, pk, (tag, li),
                                      None if last else stack.layers[li + 1], save, slim=slim, out=out if last else None)
            if save:
                tape.append(t)
        return x

    def _layer_tail(self, layer, t, att, out_proj, oname, i, pk, at, nxt, save, slim=False, out=None):
        """What follows an attention in a post-LN layer of either kind of stack: out-projection of t[att] + add & norm
        number i + linear1 (ReLU, dropout), then linear2 + add & norm number i + 1.  i fixes the keys of t: the residual
        going in is t["x"] (i = 1) or t["x%d" % (i - 1)]; o, x, m, r, d of i and o, m, r, d of i + 1 are read / written.
        With pk, two row-chain launches (at = (tag, li) names the layer's packed images, oname the out-projection's), the
        second also projecting the rows into the head-major q|k|v of nxt, the next layer if any; without pk, the separate
        kernels.  out: a (B, T, d) view that receives the output.  Returns (x, that q|k|v or None)."""
        H = self.num_heads
        res = t["x%d" % (i - 1)] if i > 1 else t["x"]
        B, T, _ = res.shape
        norm_a, norm_b = getattr(layer, "norm%d" % i), getattr(layer, "norm%d" % (i + 1))
        o_a, x_a, m_a, r_a, d_a = ("%s%d" % (k, i) for k in "oxmrd")
        o_b, m_b, r_b, d_b = ("%s%d" % (k, i + 1) for k in "omrd")
        if pk is None:
            t[o_a] = ops.linear(t[att], *_wb(out_proj))
            t[x_a], t[m_a], t[r_a] = _with_stats(ops.add_layernorm(
                t[o_a], res, *_ln(norm_a), save_stats=save, drop=t[d_a]), save)
            t["f"] = ops.linear(t[x_a], *_wb(layer.linear1), relu=True, drop=t["d_ff"])
            t[o_b] = ops.linear(t["f"], *_wb(layer.linear2))
            x, t[m_b], t[r_b] = _with_stats(ops.add_layernorm(
                t[o_b], t[x_a], *_ln(norm_b), save_stats=save, drop=t[d_b]), save)
            if out is not None:
                out.copy_(x)
                x = out
            return x, None
        tag, li = at
        t[x_a] = torch.empty_like(res)
        t[o_a], t[o_b] = (torch.empty_like(res), torch.empty_like(res)) if save else (None, None)
        t["f"] = torch.empty(B, T, layer.linear1.out_features, device=res.device, dtype=torch.float32)
        t[m_a], t[r_a] = ops.rowchain_fwd(
            t[att], pk[(tag, li, oname)], out_proj.bias.detach(), res, *_ln(norm_a), t[x_a], drop1=t[d_a], o_out=t[o_a],
            save_stats=save, w2p=pk[(tag, li, "l1")], b2=layer.linear1.bias.detach(), y2=t["f"], relu=True,
            drop2=t["d_ff"], slim=slim)
        x = out if out is not None else torch.empty_like(res)
        qkv = None if nxt is None else torch.empty(B, 3, H, T, ops.DHP, device=res.device, dtype=torch.float32)
        t[m_b], t[r_b] = ops.rowchain_fwd(
            t["f"], pk[(tag, li, "l2")], layer.linear2.bias.detach(), t[x_a], *_ln(norm_b), x, drop1=t[d_b],
            o_out=t[o_b], save_stats=save, w2p=None if nxt is None else pk[(tag, li + 1, "si")],
            b2=None if nxt is None else nxt.self_attn.in_proj_bias.detach(), y2=qkv,
            heads=None if nxt is None else (3, H, T, 0, T), slim=slim)
        return x, qkv

    def _decoder_self_block(self, li, layer, x, pk, qkv=None, ds=_NO_DROPOUT, save=False, qkv_buf=None, pos=None):
        """Self-attention block of decoder layer li on x (B, T, d), up to the cross-attention query: in_proj (unless
        qkv, this layer's head-major q|k|v, came with the previous layer's last launch), causal attention, out-projection
        + norm1 + q-projection (with pk: one row-chain launch).  Nothing here reads the memory.  With qkv_buf
        (B, 3, H, max_len, 32) and no pk it is one KV-cached decode step: the new q|k|v row is written at position `pos`
        and attends to [0, pos].  ds hands out the six dropout sites of the layer.  Returns the layer's dict."""
        H, d = self.num_heads, self.emb_dim
        dh = d // H
        B, T, _ = x.shape
        sa_w, sa_b = layer.self_attn.in_proj_weight.detach(), layer.self_attn.in_proj_bias.detach()
        t = {"x": x, "d_sa": ds.site(layer.self_attn.dropout), "d1": ds.site(layer.dropout1.p),
             "d_ca": ds.site(layer.multihead_attn.dropout), "d2": ds.site(layer.dropout2.p),
             "d_ff": ds.site(layer.dropout.p), "d3": ds.site(layer.dropout3.p)}
        t["sa"] = torch.empty_like(x)
        if qkv_buf is None:
            t["qkv"] = qkv if qkv is not None else ops.project_heads(x, sa_w, sa_b, 3, H, T)
            t["lse_s"] = torch.empty(B * H * T, device=x.device, dtype=torch.float32) if save else None
            ops.attention_heads(t["qkv"], t["qkv"], t["sa"], H, dh, T, T, 0, 1, 2, causal=True, lse=t["lse_s"],
                                drop=t["d_sa"])
        else:
            ops.project_heads(x, sa_w, sa_b, 3, H, qkv_buf.shape[3], out=qkv_buf, s0=pos, grp=1)
            ops.attention_heads(qkv_buf, qkv_buf, t["sa"], H, dh, 1, pos + 1, 0, 1, 2, q_t0=pos)
        ca_w, ca_b = layer.multihead_attn.in_proj_weight.detach(), layer.multihead_attn.in_proj_bias.detach()
        if pk is not None:
            t["x1"] = torch.empty_like(x)
            t["o1"] = torch.empty_like(x) if save else None
            t["qc"] = torch.empty(B, 1, H, T, ops.DHP, device=x.device, dtype=torch.float32)
            t["m1"], t["r1"] = ops.rowchain_fwd(
                t["sa"], pk[("d", li, "so")], layer.self_attn.out_proj.bias.detach(), x, *_ln(layer.norm1), t["x1"],
                drop1=t["d1"], o_out=t["o1"], save_stats=save, w2p=pk[("d", li, "cq")], b2=ca_b[:d], y2=t["qc"],
                heads=(1, H, T, 0, T))
        else:
            t["o1"] = ops.linear(t["sa"], *_wb(layer.self_attn.out_proj))
            t["x1"], t["m1"], t["r1"] = _with_stats(ops.add_layernorm(
                t["o1"], x, *_ln(layer.norm1), save_stats=save, drop=t["d1"]), save)
            t["qc"] = ops.project_heads(t["x1"], ca_w[:d], ca_b[:d], 1, H, T)
        return t

    def _decoder_cross_block(self, li, layer, t, kv, S, pk, save=False):
        """The rest of decoder layer li after _decoder_self_block returned t: cross-attention over the S memory rows of
        kv (head-major keys / values of layer li in segments 2li, 2li+1), out-projection + norm2 + linear1, linear2 +
        norm3 (with pk: two row-chain launches, the second also projecting the next layer's q|k|v).  The caller makes
        the main stream wait for the side stream's rows of kv first.  Returns (x, that q|k|v or None)."""
        H, d = self.num_heads, self.emb_dim
        dh = d // H
        x = t["x"]
        B, T, _ = x.shape
        t["ca"] = torch.empty_like(x)
        t["lse_c"] = torch.empty(B * H * T, device=x.device, dtype=torch.float32) if save else None
        ops.attention_heads(t["qc"], kv, t["ca"], H, dh, T, S, 0, 2 * li, 2 * li + 1, lse=t["lse_c"], drop=t["d_ca"])
        layers = self.transformer_decoder.layers
        return self._layer_tail(layer, t, "ca", layer.multihead_attn.out_proj, "co", 2, pk, ("d", li),
                                layers[li + 1] if li + 1 < len(layers) else None, save)

    def _score_head(self, h, ee, fe, eib, hv, out, vocab_ps=None, pack=None):
        """get_scores into `out`, a (B, T, V+K[+F]) view with any row stride: the vocabulary logits of hv (facts
        variants: h times the predicate gate; None: h) through fc_vocab (vocab_ps: its pre-split copy) and the pointer
        scores of h.  pack (ops.HeadRows; the fused training step): only the valid rows are computed -- gathered through
        pack.rowmap, written to the first pack.count rows of `out` (row m of the B * T, not position (b, t))."""
        B, T, d = h.shape
        V, K = self.vocab_size, ee.shape[1]
        gather = {} if pack is None else dict(a_grp=1, a_gs=d, a_gmap=pack.rowmap, m_bound=pack.count)
        ops.gemm_raw(h if hv is None else hv, self.fc_vocab.weight.detach(), out, B * T, V, d, d, 1, d, 1, out.stride(1),
                     bias=self.fc_vocab.bias.detach(), b_ps=vocab_ps, **gather)
        ops.pointer_scores(h, ee, *_wb(self.fc_entity), out, V, pack=pack)
        if self.has_facts:
            ops.pointer_scores(h, fe, *_wb(self.fc_fact), out, V + K, ind=eib, pack=pack)

    # ------------------------------------------------------------------ public score-head methods
    @torch.no_grad()
    def get_context_indicators(self, captions, facts, entity_context_size, out_length):
        """knowledge-aware/models.py:380-418 (news: same): captions (B, L) token indices, facts (B, F, 3) ->
        (entity_idx_before (B, out_length, F, 1), predicate_indicator (B, out_length, num_predicates, 1)), dense 0/1
        float tensors like the reference's.  out_length == 1 is predict()'s form ("mentioned anywhere in the buffer"),
        otherwise position p sees the mentions strictly before p.  One launch of ick_context_indicators (forward()
        itself never builds the dense predicate indicator: it uses the kernel's fused fc_predicate form)."""
        if not self.has_facts:
            raise AttributeError("the geo variant has no get_context_indicators (geo-aware/models.py)")
        dev = self.fc_vocab.weight.device
        captions = captions.to(device=dev, dtype=torch.int64)
        facts = facts.to(device=dev, dtype=torch.int64).contiguous()
        B, Lc = captions.shape
        mode = 1 if out_length == 1 else 0
        if mode == 0 and out_length > Lc:      # positions past the caption see every mention: pad with <pad> tokens
            captions = torch.cat([captions, captions.new_full((B, out_length - Lc), self.word_map["<pad>"])], dim=1)
        eib, pi = ops.context_indicators(captions.contiguous(), facts, entity_context_size, self.vocab_size, mode=mode,
                                         dense_pred=self.num_predicates)
        return eib[:, :out_length].unsqueeze(3), pi[:, :out_length].unsqueeze(3)

    @torch.no_grad()
    def get_scores(self, h, entities_encoded, facts_encoded=None, entity_idx_before=None, predicate_indicator=None):
        """geo-aware/models.py:291-313 / knowledge-aware/models.py:420-455: h (L, B, d) decoder states,
        entities_encoded (B, K, d) [, facts_encoded (B, F, d), entity_idx_before (B, L, F, 1), predicate_indicator
        (B, L, num_predicates, 1)] -> scores (L, B, V+K[+F]).  Runs the score-head kernels (vocabulary GEMM written in
        place + pointer-score kernels; the predicate gate from the DENSE indicator is one more GEMM).  Inference
        helper: gradients flow through forward() only."""
        dev = self.fc_vocab.weight.device
        hb = h.detach().to(dev, torch.float32).permute(1, 0, 2).contiguous()           # (B, L, d) rows
        ee = entities_encoded.detach().to(dev, torch.float32).contiguous()
        B, T, d = hb.shape
        fe = eib = hv = None
        if self.has_facts:
            if facts_encoded is None or entity_idx_before is None or predicate_indicator is None:
                raise IckError("%s variant: get_scores(h, entities_encoded, facts_encoded, entity_idx_before, "
                               "predicate_indicator)" % self.variant)
            fe = facts_encoded.detach().to(dev, torch.float32).contiguous()
            eib = entity_idx_before.detach().to(dev, torch.float32).reshape(B, T, fe.shape[1]).contiguous()
            pi = predicate_indicator.detach().to(dev, torch.float32).reshape(B * T, self.num_predicates).contiguous()
            gate = ops.linear(pi, self.fc_predicate.weight.detach(), self.fc_predicate.bias.detach()).view(B, T, d)
            hv = ops.mul(hb, gate)
        out = torch.empty(B, T, self.vocab_size + ee.shape[1] + (0 if fe is None else fe.shape[1]), device=dev,
                          dtype=torch.float32)
        self._score_head(hb, ee, fe, eib, hv, out, self._vocab_presplit(B * T))
        return out.permute(1, 0, 2)

    def _prepare_inputs(self, encoder_out, entities, facts):
        dev = self.fc_vocab.weight.device
        if dev.type != "cuda":
            raise IckError("DecoderTransformer parameters must live on the GPU (decoder.to('cuda'))")
        dh = self.emb_dim // self.num_heads
        if dh > ops.DHP:
            # the head-major q / k / v buffers hold ops.DHP floats per head: refused here, before anything is launched
            raise IckError("head width %d (emb_dim %d / %d heads) is above the limit of %d the head-major attention "
                           "buffers hold" % (dh, self.emb_dim, self.num_heads, ops.DHP))
        entities = entities.to(device=dev, dtype=torch.float32)
        if self.has_facts:
            if facts is None:
                raise IckError("%s variant needs the facts tensor" % self.variant)
            facts = facts.to(device=dev, dtype=torch.int64)
        return encoder_out.to(dev), entities, facts

    # ------------------------------------------------------------------ forward (teacher forced)
    def _forward_device(self, captions, caption_masks, entities, facts, enc_tok, gmap, stages=None, head=None):
        """Device-only part of forward() on length-sorted inputs (no host synchronisation inside).  head: callable
        (h, ee, fe, eib, hv) -> result that takes the place of the dense score head (score_captions)."""
        d, V = self.emb_dim, self.vocab_size
        K = entities.shape[1]
        ops.stamp("forward: start")
        pe = self.pos_encoder.pe.view(-1, d)

        def embed(ee, fe):
            return ops.caption_embed(captions, caption_masks, self.word_embedding.weight.detach(), ee, fe, pe, V,
                                     self.word_map["<pad>"], math.sqrt(d), want_emb=True)

        # (Measured and removed in round 4: layer 0's caption embedding + in_proj at the head of the side stream -- it delays
        # the context chain, which is what the first cross-attention waits for: forward 0.694 -> 0.715 ms.)
        ee, fe, kv, ctx, side = self._encode_context(enc_tok, entities, facts, gmap)
        x, emb = embed(ee, fe)
        pk = self.weight_images().current("chain").chain if self.chain_supported() else None    # as _encode_context refreshed it
        qkv = None
        S = kv.shape[3]
        for li, layer in enumerate(self.transformer_decoder.layers):
            t = self._decoder_self_block(li, layer, x, pk, qkv=qkv)
            if li == 0:
                side.join()       # entity / fact rows of kv come from the side stream
            x, qkv = self._decoder_cross_block(li, layer, t, kv, S, pk)
            ops.stamp("main: decoder layer %d done" % li)
        side.join()
        B, T, _ = x.shape
        eib = gate = hv = None
        if self.has_facts:
            eib, gate = ops.context_indicators(captions, facts, K, V, self._pred_wt(),
                                               self.fc_predicate.bias.detach(), mode=0)
            hv = ops.mul(x, gate)
        if head is not None:
            return head(x, ee, fe, eib, hv)
        scores = torch.empty(B, T, V + K + (0 if fe is None else fe.shape[1]), device=x.device, dtype=torch.float32)
        self._score_head(x, ee, fe, eib, hv, scores, self._vocab_presplit(B * T))
        ops.stamp("forward: scores done")
        if stages is not None:
            stages.update(entities_encoded=ee, facts_encoded=fe, embeddings=emb, entity_context=ctx[0],
                          fact_context=ctx[1], h=x, kv=kv, eib=eib, gate=gate)
        return scores

    def _enc_key(self, enc_in):
        """Graph-key part for a feature-map input: the attached encoder's conv1 is read through its device pointers."""
        if enc_in.dim() != 4:
            return ()
        enc = self.__dict__["_enc"]
        c1 = enc.conv1
        return (c1.weight.data_ptr(), c1.bias.data_ptr(), c1.weight._version, c1.bias._version,
                enc.__dict__.get("_param_epoch", 0))

    def input_buffers(self):
        """The static input tensors of the graph the last forward() / predict() / predict_beam() / score_captions() call
        replayed (None before the first graphed call), in that call's order -- forward: [captions, caption_masks,
        entities, facts, image input]; predict*: [image input, entities, facts]; score_captions: [captions,
        caption_masks, lengths, entities, facts, image input, image_index].  A loader that copies the next batch
        straight into them and passes them back in saves the device-to-device input copy of every call (the feature map
        is 103 MB at B = 64)."""
        return self.__dict__.get("_last_static")

    def _graphed(self, kind, key, fn, inputs):
        """Replay (capturing on first use) the hipGraph of `fn` for this shape key; parameters are read
        through their device pointers, so in-place weight updates are seen, re-allocation is not
        (the key includes the parameters' storage pointers)."""
        cache = self.__dict__.setdefault("_graphs", {})
        plist = self.__dict__.get("_plist")
        if plist is None:       # the module tree is fixed after construction; invalidate_caches() drops this list
            plist = self.__dict__["_plist"] = list(self.parameters())
        pkey = (self.__dict__.get("_param_epoch", 0),) + tuple(p._version for p in plist) + \
            tuple(p.data_ptr() for p in plist)
        # the product mode of the large GEMM tiles is baked into a capture (and decides whether the pre-split weight copies a
        # graph reads are being refreshed at all): a graph is only replayed in the mode it was captured in
        full = (kind, key, pkey, ops.gemm_split_mode())
        g = cache.get(full)
        if g is None:
            if len(cache) >= 8:
                cache.clear()
            g = cache[full] = _GraphedCall(fn, inputs)
        self.__dict__["_last_static"] = g.static_in
        return g(*inputs)

    def forward(self, captions, encoder_out, caption_masks, caption_lengths, entities, facts=None, stages=None):
        encoder_out, entities, facts = self._prepare_inputs(encoder_out, entities, facts)
        dev = encoder_out.device
        captions = captions.to(dev)
        caption_masks = caption_masks.to(dev)
        if encoder_out.dim() == 4 and not (stages is None and not self._wants_grad() and self.use_hip_graphs):
            encoder_out = self.__dict__["_enc"](encoder_out) if "_enc" in self.__dict__ else encoder_out
        enc_tok, _ = self._image_input(encoder_out)

        def sorted_inputs(c, m, e, f, sd):
            """Batch permutation into length order (reference: geo-aware/models.py:330-336), on the device."""
            return (c.index_select(0, sd), m.index_select(0, sd), e.index_select(0, sd),
                    None if f is None else f.index_select(0, sd), sd.to(torch.int32))

        if stages is None and not self._wants_grad() and self.use_hip_graphs:
            # Samples are independent, so the captured graph runs the batch in the caller's order and only the results
            # are permuted into length order.  That takes the host's length sort off the device's critical path: the
            # lengths start their way to the host, the graph is launched, and while it runs the host sorts and enqueues
            # the two gathers behind it.  (Launching the graph after a blocking .cpu() left the GPU idle for ~160 us.)
            lens_dev = caption_lengths.detach().reshape(-1)
            ev = None
            if lens_dev.is_cuda:
                pin = self.__dict__.get("_len_pin")
                if pin is None or pin.shape != lens_dev.shape or pin.dtype != lens_dev.dtype:
                    pin = self.__dict__["_len_pin"] = torch.empty(lens_dev.shape, dtype=lens_dev.dtype, pin_memory=True)
                pin.copy_(lens_dev, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record()
            key = (tuple(captions.shape), tuple(enc_tok.shape), tuple(entities.shape),
                   None if facts is None else tuple(facts.shape)) + self._enc_key(enc_tok)
            scores_raw = self._graphed("fwd", key, lambda c, m, e, f, t: self._forward_device(c, m, e, f, t, None),
                                       [captions, caption_masks, entities, facts, enc_tok])
            if ev is not None:
                ev.synchronize()
                lens_host = pin.clone()
            else:
                lens_host = lens_dev
            lengths, sort_ind = lens_host.sort(dim=0, descending=True)
            # through pinned memory: a host-to-device copy from pageable memory blocks the host until the stream
            # (the whole graph) has drained
            pidx = self.__dict__.get("_idx_pin")
            if pidx is None or pidx.shape != sort_ind.shape:
                pidx = self.__dict__["_idx_pin"] = torch.empty(sort_ind.shape, dtype=torch.int64, pin_memory=True)
            prev = self.__dict__.get("_pin_ev")
            if prev is not None:
                prev.synchronize()    # the previous call's asynchronous copy out of this pinned buffer has executed
            pidx.copy_(sort_ind)
            sort_dev = pidx.to(dev, non_blocking=True)
            prev = self.__dict__["_pin_ev"] = torch.cuda.Event()
            prev.record()
            return scores_raw.index_select(0, sort_dev), captions.index_select(0, sort_dev), (lengths - 1).tolist()
        # length sort on the host, like the reference's CPU path (the result feeds a Python list anyway)
        lengths, sort_ind = caption_lengths.detach().reshape(-1).cpu().sort(dim=0, descending=True)
        decode_lengths = (lengths - 1).tolist()
        sort_dev = sort_ind.to(dev, non_blocking=True)
        captions, caption_masks, entities, facts, gmap = sorted_inputs(captions, caption_masks, entities, facts, sort_dev)
        if self._wants_grad() and stages is None:
            # autograd bridge: the HIP backward pass runs when the caller's loss.backward() reaches us
            from . import training
            scores = training.DecoderGraphFn.apply(self, captions, caption_masks, entities, facts, enc_tok, gmap,
                                                   *training.unique_parameters(self))
            return scores, captions, decode_lengths
        return self._forward_device(captions, caption_masks, entities, facts, enc_tok, gmap, stages), captions, \
            decode_lengths

    # ------------------------------------------------------------------ scoring of given captions
    def _score_device(self, captions, caption_masks, lengths, entities, facts, enc_tok, gmap, top_k):
        """Device-only part of score_captions, in the caller's order: forward()'s layers, then the packed score head over
        the valid rows (ops.HeadRows from the device lengths) and the two reduction launches.  -> the flat result buffer of
        _caption_scores.  gmap (R,) int32: caption r reads image / entity / fact row gmap[r] (gathered copies)."""
        if gmap is not None:
            idx = gmap.long()
            enc_tok, entities = enc_tok.index_select(0, idx), entities.index_select(0, idx)
            facts = None if facts is None else facts.index_select(0, idx)
        R, Lc = captions.shape
        V, K = self.vocab_size, entities.shape[1]

        def head(x, ee, fe, eib, hv):
            pack = ops.HeadRows(lengths, R, Lc)
            Vx = V + K + (0 if fe is None else fe.shape[1])
            ld = (Vx + 3) // 4 * 4          # 16-byte aligned rows for the reduction's float4 loads
            scores = torch.empty(R, Lc, ld, device=x.device, dtype=torch.float32)[:, :, :Vx]
            self._score_head(x, ee, fe, eib, hv, scores, self._vocab_presplit(R * Lc), pack=pack)
            ops.stamp("score: packed scores done")
            T = Lc - 1
            flat = torch.empty(3 * R * T + 2 * R + 4, device=x.device, dtype=torch.float32)
            v = _caption_scores(flat, R, T)
            ops.row_logprob_rank(scores, captions, pack, self.word_map["<pad>"], out=(v.token_log_probs, v.rank, v.best))
            ops.caption_score_sums(pack, v.token_log_probs, v.rank, v.best, top_k,
                                   out=(v.log_prob, v.tokens, flat[3 * R * T + 2 * R:]))
            return flat

        return self._forward_device(captions, caption_masks, entities, facts, enc_tok, None, head=head)

    @torch.no_grad()
    def score_captions(self, captions, encoder_out, caption_masks, caption_lengths, entities, facts=None,
                       image_index=None, top_k=5):
        """How likely the GIVEN captions are (teacher forced, forward()'s argument order) -> CaptionScores, in the caller's
        caption order: per caption the summed log-probability and token count, per position the target's
        log-probability, its rank among the V+K[+F] columns (0 = argmax) and the argmax column, and the batch totals a
        validation loop accumulates (loss_sum, count, top1_hits, topk_hits with rank < top_k).
        Runs without dropout and without gradients whatever the module's mode.  No length sort and no host
        synchronisation: the lengths stay on the device, the score head runs over the valid positions only
        (ops.HeadRows) and each packed score row is read once (ick_row_logprob_rank); the (R, L, V+K+F) score matrix is
        never returned.  image_index (R,) int: caption r reads row image_index[r] of a token-major encoder_out, of
        entities and of facts (several captions of one image; as TrainStep's image_index).  With use_hip_graphs the call
        replays a captured graph per input shape (kind "score"); the result tensors are the caller's own."""
        R, Lc, n_img = check_score_args("score_captions", self.has_facts, captions, encoder_out, caption_masks,
                                        caption_lengths, entities, facts, image_index, top_k)
        if image_index is not None:
            # range check as TrainStep's: skipped for the very tensor object validated last time, unmodified
            ok = self.__dict__.get("_score_gmap_checked")
            if ok is None or ok[0]() is not image_index or ok[1:] != (image_index._version, n_img):
                lo, hi = (int(v) for v in torch.aminmax(image_index.reshape(-1)))
                if lo < 0 or hi >= n_img:
                    raise IckError("image_index values must lie in [0, %d), got [%d, %d]" % (n_img, lo, hi))
                self.__dict__["_score_gmap_checked"] = (weakref.ref(image_index), image_index._version, n_img)
        return self._score_captions(captions, encoder_out, caption_masks, caption_lengths, entities, facts, image_index,
                                    top_k)

    def _score_captions(self, captions, encoder_out, caption_masks, caption_lengths, entities, facts, image_index, top_k):
        """score_captions behind its argument checks (image_index is known to be in range)."""
        R, Lc = captions.shape
        encoder_out, entities, facts = self._prepare_inputs(encoder_out, entities, facts)
        dev = encoder_out.device
        gmap = None if image_index is None else image_index.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
        captions = captions.to(dev, torch.int64, non_blocking=True).contiguous()
        caption_masks = caption_masks.to(dev, torch.int64, non_blocking=True).contiguous()
        lengths = caption_lengths.detach().reshape(-1).to(dev, torch.int64, non_blocking=True).contiguous()
        enc_tok, _ = self._image_input(encoder_out)
        inputs = [captions, caption_masks, lengths, entities, facts, enc_tok, gmap]
        fn = lambda c, m, l, e, f, t, g: self._score_device(c, m, l, e, f, t, g, top_k)     # noqa: E731
        if self.use_hip_graphs:
            key = tuple(None if t is None else tuple(t.shape) for t in inputs) + (top_k,) + self._enc_key(enc_tok)
            flat = self._graphed("score", key, fn, inputs).clone()      # the graph's static result stays the graph's
        else:
            flat = fn(*inputs)
        return _caption_scores(flat, R, Lc - 1)

    @torch.no_grad()
    def score_tokens(self, tokens, encoder_out, entities, facts=None, samples_per_image=1, top_k=5):
        """score_captions of decode output: tokens (max_len, R) int64 as predict / predict_beam / predict_sample return
        them, column b * n + j belonging to image b (n = samples_per_image).  The rows become teacher-forcing captions
        [<start>, w_1 .. <end>, <pad> ..] on the device (ops.samples_to_captions); position t of the result scores w_{t+1}."""
        n = samples_per_image
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise IckError("score_tokens needs an integer samples_per_image >= 1")
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.shape[1] != encoder_out.shape[0] * n:
            raise IckError("score_tokens needs tokens (max_len, %d images x %d), got %s"
                           % (encoder_out.shape[0], n, tuple(tokens.shape) if torch.is_tensor(tokens) else type(tokens)))
        dev = self.fc_vocab.weight.device
        rows = tokens.to(dev, torch.int64).t().contiguous()
        wm = self.word_map
        caps, masks, lengths = ops.samples_to_captions(rows, self.vocab_size, entities.shape[1], self.has_facts,
                                                       wm["<start>"], wm["<end>"], wm["<pad>"])
        index = torch.arange(rows.shape[0], device=dev, dtype=torch.int32) // n if n > 1 else None
        check_score_args("score_tokens", self.has_facts, caps, encoder_out, masks, lengths, entities, facts, index, top_k)
        return self._score_captions(caps, encoder_out, masks, lengths, entities, facts, index, top_k)

    # ------------------------------------------------------------------ greedy decode (KV cached)
    def _refresh_decode_copies(self, rows):
        """Re-derive IN PLACE, from the live parameters, every re-laid-out weight copy the decode paths (predict,
        predict_sample over `rows` rows) read: the gathered cross K/V weight and bias, _decode_pack's transposed
        out_proj / linear2, the transposed predicate weight, the context encoders' packed row-chain images and the
        pre-split planes.  One ick_pack_weights launch (+ one ick_presplit_weights launch in the split product modes), so
        it can open a captured decode graph that must stay valid across optimizer steps which update the parameters
        behind torch's version counters (SelfCriticalStep)."""
        groups = ("kv", "decode", "pred_wt") + (("chain",) if self.chain_supported() else ())
        if ops.gemm_split_mode() != 0:
            groups += ("kv_ps",)
            if not self.fused_decode and vocab_planes_wanted(rows):      # the unfused greedy path's score head
                groups += ("vocab_ps",)
        # only the context encoders' chain images: the decode kernels read the layers directly
        self.weight_images().refresh(*groups, subset=lambda k: k[0] != "d")

    def _decode_ctx(self, kv, ee, fe, rows_per_sample, max_len, S, anc=None, want_scores=False, fuse_select=False,
                    n_done_init=0):
        """lib.DecodeCtx over freshly allocated state buffers for R = B * rows_per_sample rows (+ the tensors, kept
        alive by the caller).  See include/ick_amd.h (ick_decode_ctx)."""
        from . import lib as L
        dev = kv.device
        d, H, V = self.emb_dim, self.num_heads, self.vocab_size
        layers = self.transformer_decoder.layers
        nl = len(layers)
        B, K = ee.shape[0], ee.shape[1]
        Fn = fe.shape[1] if fe is not None else 0
        R = B * rows_per_sample
        FF = layers[0].linear1.out_features
        nch = (FF + 63) // 64
        ntiles = (V + 15) // 16
        f32 = dict(device=dev, dtype=torch.float32)
        # state buffers are initialised by ops.decode_init (one launch; they were eight fills, an embedding and a copy)
        t = {"x0": torch.empty(R, d, **f32), "xa": torch.empty(R, d, **f32), "xb": torch.empty(R, d, **f32),
             "xc": torch.empty(R, d, **f32), "p1": torch.empty(R, H, d, **f32), "p2": torch.empty(R, H, d, **f32),
             "p3": torch.empty(R, nch, d, **f32), "hfin": torch.empty(R, d, **f32), "hv": torch.empty(R, d, **f32),
             "ptr": torch.empty(R, K + Fn, **f32), "cand": torch.empty(R, ntiles, 4, **f32),
             "self_kv": torch.empty(nl, 2, R, H, max_len, ops.DHP, **f32),
             "output": torch.empty((R, max_len), dtype=torch.long, device=dev),
             "hist": torch.empty(R, max_len, dtype=torch.int32, device=dev),
             "finished": torch.empty(R, dtype=torch.int32, device=dev),
             "n_done": torch.empty(1, dtype=torch.int32, device=dev),
             "next_token": torch.empty(R, dtype=torch.long, device=dev),
             "next_mask": torch.empty(R, dtype=torch.long, device=dev),
             "pack": self._decode_pack(), "kv": kv, "ee": ee, "fe": fe, "anc": anc}
        if fuse_select:
            t["sel_state"] = torch.empty(2, R, 12, dtype=torch.int32, device=dev)
        if want_scores:
            t["scores"] = torch.empty(R, V, **f32)
        if self.has_facts:
            t["gate"] = torch.empty(R, 1, d, **f32)
            t["eib"] = torch.empty(R, 1, Fn, **f32)
            t["cap_buf"] = torch.empty((R, max_len), dtype=torch.long, device=dev)
        c = L.DecodeCtx()
        c.R, c.rows_per_sample, c.d, c.H, c.FF, c.layers, c.S, c.max_len = R, rows_per_sample, d, H, FF, nl, S, max_len
        c.V, c.K, c.F = V, K, Fn
        c.end_token, c.pad_token = self.word_map["<end>"], self.word_map["<pad>"]
        c.ln_eps, c.emb_scale = layers[0].norm1.eps, math.sqrt(d)
        c.kv_bs = kv.stride(0)
        seg = H * S * ops.DHP * 4      # bytes per (segment) of the memory projection
        pk = t["pack"]
        for li, l in enumerate(layers):
            w = c.layer[li]
            w.sa_in_w, w.sa_in_b = l.self_attn.in_proj_weight.data_ptr(), l.self_attn.in_proj_bias.data_ptr()
            w.sa_out_wt, w.sa_out_b = pk[3 * li].data_ptr(), l.self_attn.out_proj.bias.data_ptr()
            w.n1_g, w.n1_b = l.norm1.weight.data_ptr(), l.norm1.bias.data_ptr()
            w.ca_in_w, w.ca_in_b = l.multihead_attn.in_proj_weight.data_ptr(), l.multihead_attn.in_proj_bias.data_ptr()
            w.ca_out_wt, w.ca_out_b = pk[3 * li + 1].data_ptr(), l.multihead_attn.out_proj.bias.data_ptr()
            w.n2_g, w.n2_b = l.norm2.weight.data_ptr(), l.norm2.bias.data_ptr()
            w.w1, w.b1 = l.linear1.weight.data_ptr(), l.linear1.bias.data_ptr()
            w.w2t, w.b2 = pk[3 * li + 2].data_ptr(), l.linear2.bias.data_ptr()
            w.n3_g, w.n3_b = l.norm3.weight.data_ptr(), l.norm3.bias.data_ptr()
            w.self_k, w.self_v = t["self_kv"][li, 0].data_ptr(), t["self_kv"][li, 1].data_ptr()
            w.cross_k, w.cross_v = kv.data_ptr() + 2 * li * seg, kv.data_ptr() + (2 * li + 1) * seg
        c.anc = None if anc is None else anc.data_ptr()
        c.wv, c.bv = self.fc_vocab.weight.data_ptr(), self.fc_vocab.bias.data_ptr()
        c.we, c.be = self.fc_entity.weight.data_ptr(), self.fc_entity.bias.data_ptr()
        if self.has_facts:
            c.wf, c.bf = self.fc_fact.weight.data_ptr(), self.fc_fact.bias.data_ptr()
            c.fe, c.gate, c.eib, c.cap_buf = fe.data_ptr(), t["gate"].data_ptr(), t["eib"].data_ptr(), t["cap_buf"].data_ptr()
        c.ee = ee.data_ptr()
        c.word_emb, c.pe = self.word_embedding.weight.data_ptr(), self.pos_encoder.pe.data_ptr()
        for name in ("x0", "xa", "xb", "xc", "p1", "p2", "p3", "hfin", "hv", "ptr", "cand", "output", "hist", "finished",
                     "n_done", "next_token", "next_mask"):
            setattr(c, name, t[name].data_ptr())
        if want_scores:
            c.scores, c.scores_ld = t["scores"].data_ptr(), V
        if fuse_select:
            c.sel_state = t["sel_state"].data_ptr()
        ops.decode_init(c, self.word_map["<start>"], n_done_init)
        return c, t

    def _decode_front(self, what, encoder_out, entities, facts, max_pred_len, rows=1, attention=False, needs=None,
                      fits=None):
        """The front end predict(), predict_beam() and predict_sample() share: the inputs as the device loops read them,
        S_all = P + K + F memory rows and Vx = V + K + F score columns.  needs: the IckError text of a call the fused
        decode kernels cannot run -- their own size limits, or fits(B, Vx), the caller's -- or None for no such check;
        attention: the weight buffer of `rows` rows per caption must fit.  Returns (enc_tok, entities, facts, S_all, Vx)."""
        encoder_out, entities, facts = self._prepare_inputs(encoder_out, entities, facts)
        entities = entities.contiguous()
        enc_tok, P = self._image_input(encoder_out)
        enc_tok = enc_tok.contiguous()
        S_all = P + entities.shape[1] + (facts.shape[1] if facts is not None else 0)
        Vx = self.vocab_size + S_all - P
        FF = self.transformer_decoder.layers[0].linear1.out_features
        if needs is not None and not (fits(enc_tok.shape[0], Vx) and
                                      ops.decode_supported(self.emb_dim, self.num_heads, FF, S_all, max_pred_len)):
            raise IckError(needs)
        if attention:
            _attention_check(what, max_pred_len, enc_tok.shape[0] * rows, len(self.transformer_decoder.layers),
                             self.num_heads, S_all)
        return enc_tok, entities, facts, S_all, Vx

    def _decode_step(self, c, t, cap, facts, K, i, attn=None, part=0):
        """The layers of decode step i on the fused kernels (part: as ops.decode_layers_part, 0 = the whole step): the
        context indicators of the caption buffer `cap` (a model with facts), then the decoder stack and the score head,
        which also writes the step's cross-attention weights when attn is given."""
        if self.has_facts:
            ops.context_indicators(cap, facts, K, self.vocab_size, self._pred_wt(), self.fc_predicate.bias.detach(),
                                   mode=1, eib=t["eib"], gate=t["gate"])
        if attn is not None:
            ops.decode_layers_attn(c, attn, i, part)
        elif part:
            ops.decode_layers_part(c, i, part)
        else:
            ops.decode_layers(c, i)

    def _predict_fused(self, enc_tok, entities, facts, max_pred_len, attention=False):
        """predict() on the fused decode kernels (csrc/decode.hip): 12 launches per token (13 with facts).  attention:
        also return the cross-attention weights (max_len, B, layers, H, S), zero after each row's <end>."""
        B = enc_tok.shape[0]
        K = entities.shape[1]
        ee, fe, kv, _, side = self._encode_context(enc_tok, entities, facts, None)
        side.join()
        S = kv.shape[3]
        # the token of step i - 1 is chosen inside the first launch of step i (csrc/decode.hip: fused_select); only the
        # last step needs the selection kernel of its own: 11 launches per token (12 with facts)
        fuse = self.fuse_select
        c, t = self._decode_ctx(kv, ee, fe, 1, max_pred_len, S, fuse_select=fuse)
        attn = torch.zeros(max_pred_len, B, c.layers, c.H, S, device=kv.device) if attention else None
        for i in range(max_pred_len):
            fused = fuse and i > 0
            if fused:
                ops.decode_layers_part(c, i, 1)           # selection of step i - 1 + first self-attention block
            self._decode_step(c, t, t.get("cap_buf"), facts, K, i, attn, 2 if fused else 0)
            if not fuse or i == max_pred_len - 1:
                ops.decode_select_greedy(c, i)
        if attention:
            return t["output"], _zero_after_end(attn, t["output"], self.word_map["<end>"])
        return t["output"]

    def _predict_beam_device(self, enc_tok, entities, facts, max_pred_len, beam, attention=False, rules=None, groups=1,
                             penalty=None, force=None, bias=None, prefix=None):
        """Beam search on the fused decode kernels: R = B * beam rows share their caption's cross K/V; the
        self-attention cache is never reordered -- an ancestry table says which cache row holds position p of a
        hypothesis.  Returns a _BeamResult: the best sequence (B, max_len), its log-probability (B), all sequences, all
        scores; with attention also the cross-attention weights of the best (max_len, B, layers, H, S) and of every
        final hypothesis (max_len, B, beam, layers, H, S).  rules: a rules_tensor() (device input read at run time) or
        None; with it the best hypothesis is the argmax of cum / lp[length].  groups > 1: diverse beam search (DESIGN.md
        §3.2f) with the penalty lambda read from the (1) fp32 device tensor `penalty`; every group starts from the
        <start> hypothesis, and the result also holds the best hypothesis of each group (by the unpenalised key): its
        sequence (B * G, max_len), its log-probability (B * G), and with attention its weights (max_len, B * G, layers,
        H, S).  force: the (B, 8) int32
        device tensor of check_force() (read at run time) or None; with it the search is the constrained one of
        DESIGN.md §3.2g and the best hypothesis is the best by (met slots, key).  bias: the (B, 64) int32 ids and fp32
        values of check_column_bias() on the device (read at run time) or None; with it every hypothesis carries the sum
        of the biases it has emitted and the best hypothesis is the best by the key with that sum.
        prefix: the (B, max_len) int32 table of check_prefix() on the device (read at run time) or None; with it a caption
        keeps one live hypothesis (one per group) through its forced steps, and a slot that was never
        used is returned with a -inf score and a <pad> row."""
        from . import lib as L
        B = enc_tok.shape[0]
        d, V, K = self.emb_dim, self.vocab_size, entities.shape[1]
        dev = enc_tok.device
        ee, fe, kv, _, side = self._encode_context(enc_tok, entities, facts, None)
        side.join()
        S = kv.shape[3]
        R = B * beam
        anc = [torch.zeros(R, max_pred_len, dtype=torch.int32, device=dev) for _ in range(2)]
        c, t = self._decode_ctx(kv, ee, fe, beam, max_pred_len, S, anc=anc[0], want_scores=True,
                                n_done_init=B * (beam - groups))        # the unused slots count as ended
        seq = [torch.full((R, max_pred_len), self.word_map["<pad>"], dtype=torch.long, device=dev) for _ in range(2)]
        cum = torch.full((B, beam), float("-inf"), device=dev)
        kg = beam // groups
        cum[:, ::kg] = 0.0                                # one live hypothesis per caption (per group) at the start
        fin = torch.zeros(R, dtype=torch.int32, device=dev)
        facts_r = cap = None
        if self.has_facts:
            facts_r = facts.repeat_interleave(beam, dim=0).contiguous()
            cap = [torch.full((R, max_pred_len), self.word_map["<start>"], dtype=torch.long, device=dev)
                   for _ in range(2)]
        bs = L.BeamState()
        bs.cum, bs.fin, bs.start_token = cum.data_ptr(), fin.data_ptr(), self.word_map["<start>"]
        Vx = V + K + (fe.shape[1] if fe is not None else 0)
        rec = torch.empty(R, (Vx + 1023) // 1024, 18, device=dev, dtype=torch.float32)
        bs.rec = rec.data_ptr()
        attn = torch.zeros(max_pred_len, R, c.layers, c.H, S, device=dev) if attention else None
        rs = dv = fc = None
        if rules is not None:
            lens = torch.zeros(R, dtype=torch.int32, device=dev)
            rs = _rules_struct(rules, lens)
        if groups > 1:
            dv = L.DecodeDiversity()
            dv.groups, dv.penalty = groups, penalty.data_ptr()
        if force is not None:
            met = torch.zeros(R, dtype=torch.int32, device=dev)
            fc = L.DecodeConstraints()
            fc.force, fc.met = force.data_ptr(), met.data_ptr()
        cb = None
        if bias is not None:
            bsum = torch.zeros(R, dtype=torch.float32, device=dev)
            cb = L.DecodeBias()
            cb.cols, cb.vals, cb.sum = bias[0].data_ptr(), bias[1].data_ptr(), bsum.data_ptr()
        px = None
        if prefix is not None:
            px = L.DecodePrefix()
            px.cols = prefix.data_ptr()
        for i in range(max_pred_len):
            cur, nxt = i & 1, (i + 1) & 1
            c.anc = anc[cur].data_ptr()
            if self.has_facts:
                bs.cap_in, bs.cap_out = cap[cur].data_ptr(), cap[nxt].data_ptr()
            self._decode_step(c, t, cap and cap[cur], facts_r, K, i, attn)
            bs.seq_in, bs.seq_out = seq[cur].data_ptr(), seq[nxt].data_ptr()
            bs.anc_in, bs.anc_out = anc[cur].data_ptr(), anc[nxt].data_ptr()
            ops.decode_select_beam(c, bs, i, rs, dv, fc, cb, px)
        final = seq[max_pred_len & 1].view(B, beam, max_pred_len)
        if prefix is not None:                            # a slot no hypothesis ever filled: a <pad> row
            final = final.masked_fill((cum == float("-inf")).view(B, beam, 1), self.word_map["<pad>"])
        key = cum if bias is None else cum + bsum.view(B, beam)       # the kernel's ranking key
        if rules is None:
            best = key.argmax(dim=1)                      # ties: the lower hypothesis
        else:                                             # over the length penalty; ties: the lower hypothesis
            lp = rules[4:].view(torch.float32)
            key = key / lp[lens.view(B, beam).long()]
            best = key.argmax(dim=1)
        if force is not None:                             # bank first: the key ranks among the most-met hypotheses
            bank = ((met.view(B, beam, 1) >> torch.arange(FORCE_MAX, device=dev, dtype=torch.int32)) & 1).sum(dim=2)
            top = bank == bank.max(dim=1, keepdim=True).values
            best = torch.where(top, key, torch.full_like(key, float("-inf"))).argmax(dim=1)
        rows = torch.arange(B, device=dev)
        res = _BeamResult(final[rows, best], cum.gather(1, best.view(B, 1)).view(B), final, cum)
        if groups > 1:                                    # the best of each group by the same key (no penalty)
            gbest = key.view(B, groups, kg).argmax(dim=2) + torch.arange(0, beam, kg, device=dev)      # (B, G)
            bidx = rows.view(B, 1)
            res = res._replace(group=final[bidx, gbest].reshape(B * groups, max_pred_len),
                               group_score=cum.gather(1, gbest).reshape(B * groups))
        if not attention:
            return res
        # rows are never reordered: position p of a final hypothesis was computed by row anc[hyp, p] (global row index)
        anc_fin = anc[max_pred_len & 1].t().long()                                        # (max_len, R)
        steps = torch.arange(max_pred_len, device=dev).view(-1, 1)
        hyp = _zero_after_end(attn[steps, anc_fin], final.view(R, max_pred_len), self.word_map["<end>"])
        hyp = hyp.view(max_pred_len, B, beam, *hyp.shape[2:])
        if groups > 1:
            res = res._replace(group_attn=hyp[:, bidx, gbest].reshape(max_pred_len, B * groups, *hyp.shape[3:]))
        return res._replace(attn=hyp[:, rows, best], all_attn=hyp)

    @torch.no_grad()
    def predict_beam(self, encoder_out, max_pred_len, entities, facts=None, beam_size=5, return_all=False,
                     return_attention=False, length_penalty=0.0, no_repeat_ngram_size=0, min_len=0, num_beam_groups=1,
                     diversity_penalty=0.0, return_groups=False, force_tokens=None, column_bias=None, prefix=None):
        """Beam-search decode (north_star cfg5: beam 5, batch 32).  The reference decodes greedily only
        (geo-aware/eval.py:61,83), so beam > 1 has no reference output to pin against ("parity-unpinned"); the tests
        check it against a CPU beam search written to the same rules.  beam_size == 1 IS predict(): the pinned greedy path with
        its n-gram clean-up.  Hypotheses are scored by their summed log-probability (log_softmax over the V+K+F
        scores); an ended hypothesis keeps competing with its final score; the best of the beam is returned as
        LongTensor (max_pred_len, B), <pad> after <end>.  return_all adds (best log-probability (B), every final
        hypothesis (B, beam, max_len), their log-probabilities (B, beam)).  return_attention appends the cross-attention
        weights of the best hypothesis, float32 (max_pred_len, B, layers, H, S) (see predict()), and with return_all
        those of every final hypothesis, (max_pred_len, B, beam, layers, H, S).

        Decoding rules (0 = off, the default, which gives the bits of a call without them):
        length_penalty = alpha >= 0 ranks hypotheses by log-probability / ((5 + L) / 6) ** alpha, L = generated tokens
        including <end> (max_pred_len for one that never ended); no_repeat_ngram_size = n in 0..8 bans every token that
        would repeat an n-gram of the hypothesis; min_len = m bans <end> before step m.  Bans remove candidates only:
        the returned log-probabilities stay the model's untruncated ones.  The rules are a device input of the
        captured decode graph (a new value replays it); beam_size == 1 with a rule on runs the beam kernels with one
        hypothesis (predict()'s clean-up is not applied).

        Diverse beam search (Vijayakumar et al., AAAI 2018): num_beam_groups = G splits the beam into G
        groups of beam_size / G hypotheses (G divides beam_size; group g holds hypotheses g*k_g .. (g+1)*k_g - 1), each
        starting from <start>.  At every step the groups choose in order, and group g ranks a candidate token w by its
        key (with the rules above) minus diversity_penalty * (the number of hypotheses of groups 0 .. g-1 expanded with
        w at this step).  The penalty only ranks: every returned log-probability stays the model's.  diversity_penalty
        is a device input of the captured graph (a new value replays it); G = 1, the default, is the call without
        groups, bit for bit.  The best hypothesis is the best of all groups by the unpenalised key, and return_all
        lists every hypothesis group-major.  return_groups=True returns the best hypothesis of each group instead of
        the best of the caption: (max_pred_len, B * G), column b * G + g for group g of caption b; with return_all
        their log-probabilities (B * G) come second (the (B, beam, ...) values follow unchanged), and with
        return_attention their weights are (max_pred_len, B * G, layers, H, S).

        Constrained beam search (dynamic beam allocation, Post & Vilar, NAACL 2018): force_tokens is
        an integer tensor or nested list (B, C), C in 1..8, of columns every caption must contain: a word id, V + k for
        entity slot k, V + K + j for fact j, or -1 for an empty slot (<start>, <end> and <pad> cannot be forced).  A
        hypothesis cannot end before it has emitted all its caption's columns, and at every step the beam is shared
        out between the hypotheses by how many they have emitted, so that the furthest always keeps a slot; the
        returned caption contains every forced column whenever max_pred_len >= their number.  The ids are a device
        input of the captured graph (new ids, or another C, replay it); scores stay the model's log-probabilities, the
        rules compose, and return shapes do not change.  A caption whose slots are all empty gets the plain search, bit
        for bit; None, the default, is the call without the argument.  Not with num_beam_groups > 1.

        Column bias: column_bias adds a value to chosen score columns, -inf meaning "never".  It is a
        dict {column: value} for every caption (a key is a column id or a word of word_map, e.g. {"<unk>":
        float("-inf")}), or a pair (ids, values) of an integer tensor or nested list (B, C) and a float one of the same
        shape, C in 1..64 (a (C,) pair goes to every caption); columns are force_tokens' and -1 is an empty slot.  A
        hypothesis carries the sum of the biases of the columns it has emitted, and candidates are ranked by the key
        above plus that sum (an expansion with its column's bias); a -inf column leaves the candidate pool as a banned
        one does, and a rule ban wins over a bias.  Every returned score stays the model's log-probability.  Ids and
        values are device inputs of the captured graph (new values, ids or another C replay it); all slots empty or all
        values 0 give the bits of the call without the argument.  The rules compose; not with num_beam_groups > 1 or
        force_tokens.  beam_size == 1 with a bias runs the beam kernels with one hypothesis.

        Caption prefixes (elsewhere decoder_input_ids or a forced prefix): prefix starts every caption
        from tokens the caller already has.  It is an integer tensor or nested list (B, Pn), 1 <= Pn <= max_pred_len, of
        columns numbered as force_tokens numbers them (a word id, V + k for entity slot k, V + K + j for fact j); -1
        pads a shorter prefix at its end, a (Pn,) value goes to every caption, and in nested lists a string is a word of
        word_map (rows of unequal length are padded).  <start>, <end> and <pad> cannot be given.  With p_b the number of
        leading non-negative entries of caption b: at step t < p_b the only candidate of a live hypothesis is column
        prefix[b][t] -- it wins over the rule bans and over finite biases -- while the log-softmax still runs over every
        raw column, so a returned score is the model's log-probability of the WHOLE returned caption, prefix included,
        and score_tokens() of the result agrees with it.  Through its prefix a caption has one live hypothesis (one
        per group); step p_b fans out from it as step 0 of the plain search does, and from there on the call is the
        call without a prefix.  The prefix tokens count as generated tokens everywhere: n-gram history, min_len, the
        length L of the length penalty, the bias sum, the fact-aware caption buffer and the attention maps.  With
        p_b = max_pred_len nothing fans out: under return_all the other beam_size - 1 (beam_size - G) slots come back
        unused, with a -inf score and a <pad> row.  The table is a device input of the captured graph and its shape
        does not depend on Pn: new ids and new lengths replay it.  A caption whose row is all -1 gets the search
        without a prefix, bit for bit; None, the default, is the call without the argument.  It composes with the
        rules, num_beam_groups / return_groups, column_bias (a -inf bias on a column of the same caption's prefix is
        refused), return_all and return_attention; not with force_tokens.  beam_size == 1 with a prefix runs the beam
        kernels with one hypothesis; predict() does not take the argument.  "One caption per entity" is
        prefix=[[V + k]] for k in turn.  The attention maps of a GIVEN caption -- where the model looks for each
        of its words -- are a whole-caption prefix with return_attention:
            toks = caption[:, 1:1 + max_pred_len]            # the tokens after <start>, before <end>
            _, attn = decoder.predict_beam(enc, max_pred_len, entities, beam_size=1, prefix=toks, return_attention=True)
        (attn[t, b] belongs to the step that produced toks[b][t]; split_attention() splits its S axis)."""
        P_ = entities.shape[1] + (facts.shape[1] if facts is not None else 0)
        rules_on = check_rules("predict_beam", max_pred_len, self.vocab_size + P_, length_penalty,
                               no_repeat_ngram_size, min_len)
        diverse = check_diversity("predict_beam", beam_size, num_beam_groups, diversity_penalty)
        force = check_force("predict_beam", encoder_out.shape[0], self.vocab_size + P_,
                            [self.word_map[w] for w in ("<start>", "<end>", "<pad>")], force_tokens, num_beam_groups)
        bias = check_column_bias("predict_beam", encoder_out.shape[0], self.vocab_size + P_, self.word_map, column_bias,
                                 num_beam_groups, force_tokens)
        ptab = check_prefix("predict_beam", encoder_out.shape[0], self.vocab_size + P_, max_pred_len, self.word_map,
                            prefix, force_tokens, bias)
        if beam_size == 1 and not rules_on and force is None and bias is None and ptab is None:
            return DecoderTransformer.predict(self, encoder_out, max_pred_len, entities, facts,
                                              return_attention=return_attention)
        enc_tok, entities, facts, _, _ = self._decode_front(
            "predict_beam", encoder_out, entities, facts, max_pred_len, beam_size, return_attention,
            "predict_beam needs 1 <= beam_size <= 8, beam_size^2 * ceil((V+K+F)/1024) <= 4096 and sizes the fused decode "
            "kernels support", lambda B, Vx: 1 <= beam_size <= 8 and ops.decode_beam_supported(Vx, beam_size))
        rules = rules_tensor(max_pred_len, length_penalty, no_repeat_ngram_size, min_len, enc_tok.device) \
            if rules_on else None
        G = num_beam_groups
        forced = force is not None
        # the variant's own device input: the forced columns, or the diversity penalty
        extra = force.to(enc_tok.device) if forced else \
            torch.tensor([diversity_penalty], dtype=torch.float32).to(enc_tok.device) if diverse else None
        inputs = [enc_tok, entities, facts] + ([rules, extra] if extra is not None else [rules] if rules_on else [])
        if bias is not None:
            inputs = [enc_tok, entities, facts, rules, _bias_input(bias, enc_tok.device)]
        if ptab is not None:        # (rules and the variant's input may be None: every prefix call has the same arity)
            inputs = [enc_tok, entities, facts, rules, inputs[4] if len(inputs) > 4 else None, ptab.to(enc_tok.device)]

        def run(t, e, f, r=None, x=None, p=None):
            return self._predict_beam_device(t, e, f, max_pred_len, beam_size, return_attention, r, G,
                                             x if diverse else None, x if forced else None,
                                             _bias_views(x) if bias is not None else None, p)

        if self.use_hip_graphs:
            key = (tuple(enc_tok.shape), tuple(entities.shape), None if facts is None else tuple(facts.shape),
                   max_pred_len, beam_size) + self._enc_key(enc_tok) + ((G,) if diverse else ())
            kind = "beam" + ("_prefix" if ptab is not None else "") + ("_force" if forced else "_div" if diverse else "_bias" if bias is not None else "") + \
                ("_rules" if rules_on else "") + \
                ("_attn" if return_attention else "")
            res = self._graphed(kind, key, run, inputs)
        else:
            res = run(*inputs)
        seq, score, attn = res.best, res.score, res.attn
        if return_groups and diverse:       # the best of each group in place of the best of the caption
            seq, score, attn = res.group, res.group_score, res.group_attn
        out = seq.t().contiguous()
        if not return_attention:
            return (out, score, res.all, res.all_scores) if return_all else out
        if return_all:
            return out, score, res.all, res.all_scores, attn.clone(), res.all_attn.clone()
        return out, attn.clone()

    def _predict_sample_device(self, enc_tok, entities, facts, knobs, max_pred_len, n, attention=False, rules=None,
                               bias=None, prefix=None):
        """Sampled decode on the fused decode kernels: R = B * n rows, the n samples of a caption share its cross K/V
        and keep their own self-attention caches.  knobs: int64 (3) device tensor [seed, temperature | top_p << 32
        (two fp32 words), top_k] -- read by the selection kernel, so a replay sees whatever was copied into it.
        rules: a rules_tensor() (read the same way) or None; bias: the (B, 64) ids and values of check_column_bias() on
        the device (read the same way) or None; prefix: the (B, max_len) int32 table of check_prefix() on the device (read
        the same way) or None.  Returns (tokens (R, max_len), log-probabilities (R, max_len)[, cross-attention weights (max_len, R, layers, H,
        S)])."""
        from . import lib as L
        dev = enc_tok.device
        K = entities.shape[1]
        ee, fe, kv, _, side = self._encode_context(enc_tok, entities, facts, None)
        side.join()
        c, t = self._decode_ctx(kv, ee, fe, n, max_pred_len, kv.shape[3], want_scores=True)
        log_prob = torch.zeros(c.R, max_pred_len, device=dev, dtype=torch.float32)
        facts_r = facts.repeat_interleave(n, dim=0).contiguous() if self.has_facts else None
        st = L.SampleState()
        base = knobs.data_ptr()
        st.seed, st.temp_top_p, st.top_k, st.log_prob = base, base + 8, base + 16, log_prob.data_ptr()
        attn = torch.zeros(max_pred_len, c.R, c.layers, c.H, c.S, device=dev) if attention else None
        rs = None if rules is None else _rules_struct(rules)
        cb = None
        if bias is not None:
            cb = L.DecodeBias()
            cb.cols, cb.vals = bias[0].data_ptr(), bias[1].data_ptr()
        px = None
        if prefix is not None:
            px = L.DecodePrefix()
            px.cols = prefix.data_ptr()
        for i in range(max_pred_len):
            self._decode_step(c, t, t.get("cap_buf"), facts_r, K, i, attn)
            ops.decode_select_sample(c, st, i, rs, cb, px)
        if attention:
            return t["output"], log_prob, _zero_after_end(attn, t["output"], self.word_map["<end>"])
        return t["output"], log_prob

    @torch.no_grad()
    def predict_sample(self, encoder_out, max_pred_len, entities, facts=None, num_samples=1, temperature=1.0, top_k=0,
                       top_p=1.0, seed=None, return_log_probs=False, return_attention=False, no_repeat_ngram_size=0,
                       min_len=0, column_bias=None, prefix=None):
        """Stochastic decode: `num_samples` captions per image drawn from the model's distribution, with temperature,
        top-k and nucleus (top-p) truncation.  Per row and step over the V+K+F raw scores s: z = s / temperature;
        top-k keeps s >= the k-th largest s (ties at the boundary all kept); top-p then keeps the tokens whose
        strictly-greater mass (weights exp(z - max z) over the kept set) is < top_p of the kept mass; the token is
        argmax(z + Gumbel noise) over the kept set, the noise drawn by Philox-4x32-10 from (seed, caption, sample, step,
        column) -- so the samples of a caption do not depend on the rest of the batch (csrc/sample.hip).
        The reference's repeated n-gram clean-up (a greedy heuristic on the runner-up token) is NOT applied: top_k=1 is
        plain argmax decoding and differs from predict() wherever that clean-up fires.

        Returns LongTensor (max_pred_len, B * num_samples), column b * num_samples + j = sample j of caption b, <pad>
        after <end>; with return_log_probs also a float tensor of the same shape: the model's log-probability
        (log_softmax of the raw scores, T = 1, untruncated) of every generated token, 0 after <end>.  seed=None draws a
        63-bit seed from torch's default CPU generator; an integer seed makes the call bit-reproducible.  The knobs
        and the seed are inputs of the captured decode graph: changing them replays it without a new capture.
        return_attention appends the cross-attention weights, float32 (max_pred_len, B * num_samples, layers, H, S) (see
        predict()); the tokens and log-probabilities are the same bits as without it.

        Decoding rules (as predict_beam; 0 = off, the default): no_repeat_ngram_size = n in 0..8 bans every token that
        would repeat an n-gram of the row, min_len = m bans <end> before step m.  A banned token is absent before top-k
        and top-p (not counted in k, no mass); its Gumbel noise is unchanged, so a step where no ban fires draws the
        same token as without rules.  return_log_probs stays the untruncated log-probability.

        Column bias (as predict_beam's column_bias): everything that selects runs on s' = s + b -- the
        top-k threshold, z = s' / temperature, the top-p weights and the Gumbel arg-max; a -inf column is absent like a
        banned one.  The noise of a column does not change, so a step at which no biased column is near the draw draws
        the token it drew before; return_log_probs stays log_softmax of the raw scores.  A bias on <end> is the length
        control of sampling.  Ids and values are inputs of the captured graph.

        Caption prefixes (as predict_beam's prefix): every sample of caption b starts with prefix[b].
        A forced step draws nothing -- no top-k, no top-p, no noise -- and wins over the rule bans and the bias;
        return_log_probs holds the model's log-probability of the prefix tokens as well.  The noise is keyed by (seed,
        caption, sample, step, column), so the later steps draw what they would have drawn: feeding back the first p
        tokens of a sample with the seed it was drawn with reproduces that sample.  num_samples continuations of one
        opening are prefix=opening with num_samples > 1.  The table is an input of the captured graph (new ids and
        lengths replay it); a row of -1 gets the draw without a prefix, bit for bit.  The attention maps of a given
        caption are a whole-caption prefix with return_attention (see predict_beam)."""
        P_ = entities.shape[1] + (facts.shape[1] if facts is not None else 0)
        rules_on = check_rules("predict_sample", max_pred_len, self.vocab_size + P_, 0.0, no_repeat_ngram_size, min_len)
        bias = check_column_bias("predict_sample", encoder_out.shape[0], self.vocab_size + P_, self.word_map,
                                 column_bias)
        ptab = check_prefix("predict_sample", encoder_out.shape[0], self.vocab_size + P_, max_pred_len, self.word_map,
                            prefix, None, bias)
        if not (isinstance(num_samples, int) and num_samples >= 1):
            raise IckError("predict_sample needs num_samples >= 1")
        if not (math.isfinite(temperature) and temperature > 0):
            raise IckError("predict_sample needs a finite temperature > 0")
        if not (isinstance(top_k, int) and top_k >= 0):
            raise IckError("predict_sample needs an integer top_k >= 0 (0 = off)")
        if not (0 < top_p <= 1):
            raise IckError("predict_sample needs 0 < top_p <= 1")
        enc_tok, entities, facts, _, _ = self._decode_front(
            "predict_sample", encoder_out, entities, facts, max_pred_len, num_samples, return_attention,
            "predict_sample needs B * num_samples <= 65535, V+K+F <= 65536 and sizes the fused decode kernels support",
            lambda B, Vx: B * num_samples <= 65535 and ops.decode_sample_supported(Vx, num_samples))
        if seed is None:
            seed = int(torch.randint(0, 2 ** 63 - 1, (), dtype=torch.int64))
        seed = int(seed) & (2 ** 64 - 1)
        seed = seed - 2 ** 64 if seed >= 2 ** 63 else seed          # the same 64 bits as an int64
        tp = struct.unpack("<q", struct.pack("<ff", temperature, top_p))[0]
        knobs = torch.tensor([seed, tp, min(top_k, 2 ** 31 - 1)], dtype=torch.int64).to(enc_tok.device)
        rules = rules_tensor(max_pred_len, 0.0, no_repeat_ngram_size, min_len, enc_tok.device) if rules_on else None
        inputs = [enc_tok, entities, facts, knobs] + ([rules] if rules_on else [])
        if bias is not None:
            inputs = [enc_tok, entities, facts, knobs, rules, _bias_input(bias, enc_tok.device)]
        if ptab is not None:
            inputs = [enc_tok, entities, facts, knobs, rules, inputs[5] if bias is not None else None,
                      ptab.to(enc_tok.device)]

        def run(t, e, f, k, r=None, x=None, p=None):
            return self._predict_sample_device(t, e, f, k, max_pred_len, num_samples, return_attention, r,
                                               None if x is None else _bias_views(x), p)

        if self.use_hip_graphs:
            key = (tuple(enc_tok.shape), tuple(entities.shape), None if facts is None else tuple(facts.shape),
                   max_pred_len, num_samples) + self._enc_key(enc_tok)
            kind = "sample" + ("_prefix" if ptab is not None else "") + ("_bias" if bias is not None else "") + ("_rules" if rules_on else "") + \
                ("_attn" if return_attention else "")
            res = self._graphed(kind, key, run, inputs)
        else:
            res = run(*inputs)
        out = res[0].t().contiguous()
        ret = (out, res[1].t().contiguous()) if return_log_probs else (out,)
        if return_attention:
            ret += (res[2].clone(),)
        return ret if len(ret) > 1 else out

    def _predict_device(self, enc_tok, entities, facts, max_pred_len, attention=False):
        """Whole greedy decode on the device: every step's token choice, clean-up and stop flag are computed
        by kernels (no host round trip), so the loop can be captured as one hipGraph."""
        dev = enc_tok.device
        B = enc_tok.shape[0]
        d, V, K = self.emb_dim, self.vocab_size, entities.shape[1]
        P = enc_tok.shape[1] if enc_tok.dim() == 3 else enc_tok.shape[2] * enc_tok.shape[3]
        S_all = P + K + (facts.shape[1] if facts is not None else 0)
        FF = self.transformer_decoder.layers[0].linear1.out_features
        if self.fused_decode and ops.decode_supported(d, self.num_heads, FF, S_all, max_pred_len):
            return self._predict_fused(enc_tok, entities, facts, max_pred_len, attention)
        if attention:
            raise IckError("return_attention needs the fused decode kernels")
        ee, fe, kv, _, side = self._encode_context(enc_tok, entities, facts, None)
        side.join()
        S = kv.shape[3]
        pe = self.pos_encoder.pe.view(-1, d)
        nl = len(self.transformer_decoder.layers)
        qkv_cache = [torch.empty(B, 3, self.num_heads, max_pred_len, ops.DHP, device=dev, dtype=torch.float32)
                     for _ in range(nl)]
        output = torch.full((B, max_pred_len), self.word_map["<pad>"], dtype=torch.long, device=dev)
        hist = torch.zeros(B, max_pred_len, dtype=torch.int32, device=dev)
        finished = torch.zeros(B, dtype=torch.int32, device=dev)
        tok = torch.full((B, 1), self.word_map["<start>"], dtype=torch.long, device=dev)
        msk = torch.zeros(B, 1, dtype=torch.long, device=dev)
        cap_buf = torch.full((B, max_pred_len), self.word_map["<start>"], dtype=torch.long, device=dev)
        Fn = fe.shape[1] if fe is not None else 0
        scores = torch.empty(B, 1, V + K + Fn, device=dev, dtype=torch.float32)
        wemb = self.word_embedding.weight.detach()
        for i in range(max_pred_len):
            x = ops.caption_embed(tok, msk, wemb, ee, fe, pe, V, self.word_map["<pad>"], math.sqrt(d), pos0=i)
            for li, layer in enumerate(self.transformer_decoder.layers):
                t = self._decoder_self_block(li, layer, x, None, qkv_buf=qkv_cache[li], pos=i)
                x, _ = self._decoder_cross_block(li, layer, t, kv, S, None)
            eib = hv = None
            if self.has_facts:
                eib, gate = ops.context_indicators(cap_buf, facts, K, V, self._pred_wt(),
                                                   self.fc_predicate.bias.detach(), mode=1)
                hv = ops.mul(x, gate)
            self._score_head(x, ee, fe, eib, hv, scores, self._vocab_presplit(B))
            ops.greedy_select(scores.view(B, -1), output, hist, finished, tok.view(-1), msk.view(-1), i, V, K,
                              self.has_facts, self.word_map["<end>"])
            if self.has_facts and i + 1 < max_pred_len:
                cap_buf[:, i + 1] = tok.view(-1)
        return output

    @torch.no_grad()
    def predict(self, encoder_out, max_pred_len, entities, facts=None, return_attention=False):
        """Greedy decode with the reference's semantics per caption (argmax, <end> stop, repeated
        n-gram clean-up, pointer masks), KV-cached: step i only projects position i.  Works for any
        batch size (B independent captions); returns LongTensor (max_pred_len, B), <pad> after <end>.

        return_attention=True also returns the decoder's cross-attention weights, float32 on the device,
        (max_pred_len, B, layers, H, S): softmax(q . k / sqrt(dh)) of the query at step i (the one that produced output
        token i) over the S = P + K + F memory rows [image ; entities ; facts] (split_attention() cuts that axis).  Steps
        after a row's <end> are zero (the <end> step keeps the weights that chose it).  Needs the fused decode kernels
        and a buffer of at most ATTENTION_MAX_BYTES; the tokens are the same bits as without it."""
        enc_tok, entities, facts, _, _ = self._decode_front(
            "predict", encoder_out, entities, facts, max_pred_len, 1, return_attention,
            "predict(return_attention=True) needs fused_decode and sizes the fused decode kernels support"
            if return_attention else None, lambda B, Vx: self.fused_decode)
        if self.use_hip_graphs:
            key = (tuple(enc_tok.shape), tuple(entities.shape), None if facts is None else tuple(facts.shape),
                   max_pred_len) + self._enc_key(enc_tok)
            res = self._graphed("greedy_attn" if return_attention else "greedy", key,
                                lambda t, e, f: self._predict_device(t, e, f, max_pred_len, return_attention),
                                [enc_tok, entities, facts])
        else:
            res = self._predict_device(enc_tok, entities, facts, max_pred_len, return_attention)
        if return_attention:
            return res[0].t().contiguous(), res[1].clone()
        return res.t().contiguous()
