"""Training step of the caption decoder on MI355X.

Reference call surface (geo-aware/train.py:269-292):
    scores, caps_sorted, decode_lengths = decoder(captions, imgs, masks, lengths, entities[, facts])
    loss = CrossEntropyLoss(ignore_index=<pad>)(pack_padded(scores), pack_padded(caps_sorted[:, 1:]))
    decoder_optimizer.zero_grad(); loss.backward(); clip_gradient(optimizer, 5.0); optimizer.step()

Two ways in:
  * drop-in: in train() mode DecoderTransformer.forward routes through DecoderGraphFn, a
    torch.autograd.Function whose backward runs the hand-written HIP backward pass, so the
    reference's train.py works unchanged (its loss / optimizer stay torch objects);
  * fused: TrainStep owns one flat fp32 bucket for parameters, gradients and Adam moments, runs
    forward -> packed cross entropy -> backward -> (RCCL all-reduce of the bucket) -> clamp + Adam,
    all in HIP kernels, one collective per step (data parallel over the GPUs of a node).
Dropout: the reference constructs the decoder with dropout 0.5/0.5/0.1; the masks come from a
counter-based generator (see ick_dropout) and cannot be bit-identical to torch's CPU stream, so
parity of the training math is pinned with dropout disabled (p = 0 / eval-mode fixtures).
"""
import collections
import contextlib
import functools
import math
import os
import weakref

import torch

from . import dp, ops
from .bucket import ParamBucket
from .decoder import DropSites
from .lib import IckError
from .weights import DerivedWeights, first_stage, vocab_planes_wanted      # noqa: F401  (DerivedWeights is also imported from here)


class Tape:
    """Activations kept from the forward pass for the backward pass."""

    def __init__(self):
        self.enc_layers = {}   # stack name -> list of per-layer dicts
        self.dec_layers = []
        self.misc = {}


def _p(x):
    return x.detach()


# ----------------------------------------------------------------------------------------------
# forward with saved activations
# ----------------------------------------------------------------------------------------------
def forward_with_tape(dec, captions, caption_masks, entities, facts, enc_tok, gmap, seed=0, epoch=None,
                      fresh_pack=False, overlap=False, feats=None, conv1=None, side_tail=None, derived=None, pre_side=None,
                      head_rows=None, pre_main=None):
    """Teacher-forced forward on already length-sorted inputs; returns (scores, tape).  Dropout is
    active iff the module is in train() mode (masks derive from `seed` + the device counter `epoch`).
    fresh_pack: rebuild the packed cross-K/V / transposed predicate weights from the live parameters
    (needed when they are updated behind torch's version counters, and inside captured graphs).
    derived: TrainStep's persistent re-laid-out copies of the weights (DerivedWeights: packed row-chain copies, forward
    and transposed, the gathered cross K/V weight / bias and the bf16 planes of the large GEMMs' weights), kept current by
    the optimizer kernel itself -- no packing launch at all in this pass.
    overlap: run the context-encoder chain (small, latency-bound kernels) on a second stream beside the
    image-row K/V projection and the first self-attention block (for captured graphs; eager launches are
    host-bound and gain nothing).
    feats + conv1 = (weight, bias): instead of enc_tok, the (B, 2048, 14, 14) feature map; Encoder.conv1 then runs
    here and writes the image rows straight into the memory buffer (no (B, 196, d) intermediate, no copy).
    side_tail: work of the caller that nothing in the forward pass waits for (TrainStep: zeroing the gradient bucket,
    the decode lengths); with `overlap` it runs on the side stream once the context chain is done, else right away.
    pre_side (needs overlap, feats and derived): work of the caller that must run BEFORE anything here reads a parameter
    -- TrainStep's deferred optimizer update of the previous step.  It opens the side stream, beside Encoder.conv1 on the
    main stream (frozen weights, input features: the one large kernel of the step that reads no trainable parameter);
    the entity / fact encoders follow it there and the main stream waits for that point behind conv1.
    pre_main: work of the caller that must run on the MAIN stream before Encoder.conv1 and before the side stream opens --
    TrainStep's deferred update of a trained conv1 (it reads the step counter the side stream's update then advances).
    head_rows: callable -> ops.HeadRows or None, asked when the score head is reached (TrainStep makes the row list in its
    side tail): the head then runs over the packed list of valid rows only and `scores` holds packed rows."""
    tape = Tape()
    m = tape.misc
    if pre_main is not None:
        pre_main()
    ds = DropSites(seed, dec.training, epoch)
    d, V, H = dec.emb_dim, dec.vocab_size, dec.num_heads
    B, L = captions.shape
    P = feats.shape[2] * feats.shape[3] if feats is not None else enc_tok.shape[1]
    K = entities.shape[1]
    dev = captions.device
    Fn = facts.shape[1] if dec.has_facts else 0
    nseg = 2 * len(dec.transformer_decoder.layers)
    S = P + K + Fn
    # memory rows [image ; entities ; facts], kept contiguous (B, S, d) for the weight gradient of the K/V
    # projection; its three row groups are projected separately (disjoint rows of the head-major kv buffer)
    mem = torch.empty(B, S, d, device=dev, dtype=torch.float32)
    kv = torch.empty(B, nseg, H, S, ops.DHP, device=dev, dtype=torch.float32)
    tape.enc_layers["entities"] = []
    if dec.has_facts:
        tape.enc_layers["facts"] = []
    side = ops.SideStream(priority=-1) if overlap else None
    if side is None and side_tail is not None:
        side_tail()

    chain = dec.chain_supported()
    chain_t = chain and dec.chain_bwd_supported()
    staged = chain and fresh_pack and overlap and derived is None
    split_on = ops.gemm_split_mode() >= 1 and not ops.is_deterministic()

    lazy = pre_side is not None and side is not None and feats is not None and derived is not None
    if pre_side is not None and not lazy:
        pre_side()
    ee, fe = (None, None) if lazy else dec._encode_entities(entities, facts)
    # The re-laid-out weight copies.  `derived` keeps them current itself; a captured step without it (fresh_pack) re-fills
    # them, the packed row-chain images in three launches placed where they cost least: the context encoders' now (the side
    # chain needs them first; the cross K/V weight and bias ride along), the decoder layers' after Encoder.conv1 has been
    # enqueued, the transposed images of the backward chains on the side stream once the context chain is done.
    wi = dec.weight_images()
    fill = None if derived is not None else wi.refresh if fresh_pack else wi.current
    if staged:
        wi.refresh("kv", "chain", subset=first_stage)
    elif fill is not None:
        fill("kv", *(("chain",) if chain else ()))
    wkv, bkv = wi.wkv, wi.bkv
    pk = wi.chain if chain else None

    def kv_presplit():
        # pre-split copy (three bf16 planes) of the all-layer cross K/V weight for the image rows' projection (ick_gemm's
        # b_ps, csrc/gemm_ps.hip); with a side stream it is made behind the fork: only the main stream reads it
        if split_on:
            if fill is not None:
                fill("kv_ps")
            m["wkv_ps"] = wi.kv_ps

    if side is None:
        kv_presplit()

    def vocab_presplit():
        # fc_vocab's pre-split copies: nothing needs them before the score head, so they are made where the side stream
        # idles.  The transposed one is the B operand of the data gradient dh = dscores @ W on the pre-split kernel (128 x 80
        # tile, 40 tiles x 12 K slices: cfg2 train step 1.770 -> 1.741 ms, profiles/r04_y_ab_vocab_dgrad_ps.txt)
        if split_on and vocab_planes_wanted(B * L):
            groups = ("vocab_ps", "vocab_t_ps") if derived is not None or fresh_pack else ("vocab_ps",)
            if fill is not None:
                fill(*groups)
            for g in groups:
                m[g] = getattr(wi, g)

    head = {}

    def entity_chain():
        nonlocal ee, fe
        if lazy:
            ops.stamp("side: deferred optimizer update starts")
            pre_side()
            ee, fe = head["ee"], head["fe"] = dec._encode_entities(entities, facts)
            side.signal("head")
        ops.stamp("side: context chain starts")
        # the stack's last add & norm writes the entity rows of the memory buffer directly; beside Encoder.conv1 and the
        # image K/V projection the chain runs in its 8-wave form, which finds room on the CUs the bulk GEMMs occupy
        ctx_e = dec._context_stack(dec.transformer_encoder_entities, ee, pk, "e", out=mem[:, P:P + K], slim=overlap, ds=ds,
                                   tape=tape.enc_layers["entities"])
        ops.project_heads(ctx_e, wkv, bkv, nseg, H, S, out=kv, s0=P, grp=K)
        if side is not None:
            side.signal("ctx")      # the first cross-attention waits for this point, not for the packing / zeroing below
        ops.stamp("side: context chain done")
        # bulk work nothing waits for before the score head / the backward pass
        if staged and chain_t:
            wi.refresh("chain_t")
        vocab_presplit()
        if side is not None and side_tail is not None:
            side_tail()

    def fact_chain():
        ctx_f = dec._context_stack(dec.transformer_encoder_facts, fe, pk, "f", out=mem[:, P + K:], slim=overlap, ds=ds,
                                   tape=tape.enc_layers["facts"])
        ops.project_heads(ctx_f, wkv, bkv, nseg, H, S, out=kv, s0=P + K, grp=Fn)

    pe = dec.pos_encoder.pe.view(-1, d)
    if feats is not None:
        img = mem[:, :P]
    else:
        img = enc_tok.index_select(0, gmap.long()) if gmap is not None else enc_tok
    if side is not None:
        side.submit(entity_chain, ee, fe, mem, kv, wkv, bkv, img, entities, facts)
    else:
        entity_chain()
    if feats is not None:
        cw, cb = conv1[0], conv1[1]
        Cc = feats.shape[1]
        ops.gemm_raw(feats, cw.view(d, Cc), mem, B * P, d, Cc, 1, P, Cc, 1, d, bias=cb, a_grp=P, a_gs=Cc * P,
                     c_grp=P, c_gs=S * d, b_ps=conv1[2] if len(conv1) > 2 else None)
    else:
        mem[:, :P].copy_(img)
    if side is not None:
        side.flush()     # enqueued after the main stream's next kernel (see SideStream)
        if lazy:
            side.wait("head")      # from here on the main stream reads parameters (and the encoded entity / fact rows)
            ee, fe = head["ee"], head["fe"]
        kv_presplit()
    if staged:
        wi.refresh("chain", subset=lambda k: not first_stage(k))
    elif fill is not None and chain_t:
        fill("chain_t")
    if chain_t:
        m["pkb"] = wi.chain_t
    if dec.has_facts:
        # on the main stream, beside the entity chain on the side stream: two chains of small kernels overlap well
        # (a chain beside the large projection below does not)
        fact_chain()
    # One GEMM for the image rows of every layer.  Projecting the later layers' rows on the side stream after the
    # chain was measured (device time stamps): the chain ends 70 us earlier, the first decoder layer 90 us later --
    # a 5000-workgroup GEMM beside a chain of small kernels delays the chain by about its own duration either way.
    ops.project_heads(img, wkv, bkv, nseg, H, S, out=kv, s0=0, grp=P, w_ps=m.get("wkv_ps"))
    ops.stamp("fwd: image K/V projection done")
    m["d_pos"] = ds.site(dec.pos_encoder.dropout.p)
    x = ops.caption_embed(captions, caption_masks, _p(dec.word_embedding.weight), ee, fe, pe, V,
                          dec.word_map["<pad>"], math.sqrt(d), drop=m["d_pos"])
    qkv = None
    for li, layer in enumerate(dec.transformer_decoder.layers):
        t = dec._decoder_self_block(li, layer, x, pk, qkv=qkv, ds=ds, save=True)
        ops.stamp("fwd: layer %d reaches cross-attention" % li)
        if side is not None and li == 0:
            side.wait_or_join("ctx")    # the context rows of kv come from the side stream (its tail may still run)
        x, qkv = dec._decoder_cross_block(li, layer, t, kv, S, pk, save=True)
        tape.dec_layers.append(t)
    if side is not None:
        side.join()
    ops.stamp("fwd: decoder layers done")
    eib = gate = hv = None
    if dec.has_facts:
        if fill is not None:
            fill("pred_wt")
        eib, gate = ops.context_indicators(captions, facts, K, V, wi.pred_wt, _p(dec.fc_predicate.bias), mode=0)
        hv = ops.mul(x, gate)
    Vx = V + K + Fn
    # rows padded to a multiple of 4 floats (knowledge: 50 000 + 20 + 51 = 50 071 columns): the vocabulary's data- and
    # weight-gradient GEMMs read the score gradients with 16-byte loads only from aligned rows (645 -> ~470 us)
    ld = (Vx + 3) // 4 * 4
    scores = torch.empty(B, L, ld, device=x.device, dtype=torch.float32)[:, :, :Vx]
    m["pack"] = head_rows() if head_rows is not None else None
    dec._score_head(x, ee, fe, eib, hv, scores, m.get("vocab_ps"), pack=m["pack"])
    m.update(ee=ee, fe=fe, mem=mem, kv=kv, h=x, hv=hv, eib=eib, gate=gate, captions=captions, masks=caption_masks,
             entities=entities, facts=facts, P=P, K=K, Fn=Fn, S=S, wkv=wkv)
    return scores, tape


# ----------------------------------------------------------------------------------------------
# backward
# ----------------------------------------------------------------------------------------------
def _keep_scale(drop):
    return 1.0 if drop is None else 1.0 / (1.0 - drop[0])


def _g(grads, param):
    """Gradient buffer of a parameter (None when it is frozen)."""
    return grads.get(id(param))


def _lin_bwd(grads, dy2, x2, lin_w, lin_b, w_rows=None, need_dx=True, dx=None, acc=False, group_now=False,
             gate=None, gate_scale=1.0, wt_ps=None, xt_ps=None, pack=None, valid=None):
    """Backward of a Linear whose weight is `lin_w` (optionally the row slice w_rows of it)."""
    gw, gb = _g(grads, lin_w), _g(grads, lin_b)
    w = _p(lin_w)
    if w_rows is not None:
        w = w[w_rows]
        gw = gw[w_rows] if gw is not None else None
        gb = gb[w_rows] if gb is not None else None
    return ops.linear_bwd(dy2, x2, w, gw, gb, need_dx=need_dx, dx=dx, accumulate_dx=acc, group_now=group_now,
                          gate=gate, gate_scale=gate_scale, wt_ps=wt_ps, xt_ps=xt_ps, pack=pack, valid=valid)


def _prezeroed(dec, captions, entities, facts):
    """Accumulation targets of the backward pass's first kernels (the vocabulary data gradient's split-K sum, the
    gradient of the encoded entity / fact rows), zeroed where nothing waits for it -- the forward pass's side stream --
    instead of between the loss and the first backward GEMM (two fills + a gap: ~13 us of the step's critical path)."""
    B, L = captions.shape[0], captions.shape[1]
    d, dev = dec.emb_dim, captions.device
    pre = {"dhv": torch.zeros(B * L, d, device=dev, dtype=torch.float32),
           "dee": torch.zeros(B, entities.shape[1], d, device=dev, dtype=torch.float32)}
    if facts is not None:
        pre["dfe"] = torch.zeros(B, facts.shape[1], d, device=dev, dtype=torch.float32)
    return pre


# A post-LN layer's backward, written once for the context-encoder stacks and the decoder stack and for both kernel
# paths.  What differs between the layers arrives as data: an add & norm site = (LayerNorm module, its index in the
# layer's tape dict, the key of its residual operand), the attention's module and tape keys, the packed images' names.
# When the side stream's queued work goes out is each stack's own choreography: the stacks below call ops.SIDE's flushes
# between the pieces, no piece calls one (ops.layernorm_bwd flushes behind its own kernel, whoever calls it).
Dims = collections.namedtuple("Dims", "B T M d H dh dev")       # of a stack whose activations are (B, T, d); M = B * T


def _dims(dec, x):
    B, T, d = x.shape
    return Dims(B, T, B * T, d, dec.num_heads, d // dec.num_heads, x.device)


def _norm_args(t, site, D):
    """The saved forward tensors of an add & norm site + fresh outputs, as ops.rowchain_bwd wants them."""
    norm, i, res = site
    return dict(o=t["o%d" % i], res=t[res], mean=t["m%d" % i], rstd=t["r%d" % i], gamma=_p(norm.weight),
                drop=t["d%d" % i], do=torch.empty(D.M, D.d, device=D.dev, dtype=torch.float32),
                part=ops.ln_partials(D.M, D.d, D.dev), norm=norm)


def _norm_param_grads(grads, n):
    ops.ln_partials_reduce(n["part"], _g(grads, n["norm"].weight), _g(grads, n["norm"].bias))


def _ffn_chain_launch(layer, t, hi, lo, out_img, pkb, at, state, D):
    """One ops.rowchain_bwd launch: [the hand-down g0 @ W0 + dzin] + norm' (site hi) + linear2' + ReLU' + linear1' +
    norm' (site lo) + the out-projection' below it.  state = (dz, g0, w0p): the residual-path gradient of the layer's
    output and the gradient whose data gradient rides on this launch.  at = (tag, li) names the layer's packed transposed
    images, out_img the out-projection's.  Returns (n_hi, n_lo, dpre, datt, dz_out): the norms' argument dicts, the
    gradients of linear1's and of the attention's output, the residual-path gradient below site lo."""
    dz, g0, w0p = state
    n_hi, n_lo = _norm_args(t, hi, D), _norm_args(t, lo, D)
    dpre = torch.empty(D.M, layer.linear1.out_features, device=D.dev, dtype=torch.float32)
    datt = torch.empty(D.M, D.d, device=D.dev, dtype=torch.float32)
    dz_out = torch.empty(D.M, D.d, device=D.dev, dtype=torch.float32)
    ops.rowchain_bwd(D.M, D.d, n_hi, pkb[at + (out_img,)], datt, dz_out, g0=g0, w0p=w0p, dzin=dz,
                     ffn=dict(w1p=pkb[at + ("l2T",)], w2p=pkb[at + ("l1T",)], act=t["f"],
                              gate_scale=_keep_scale(t["d_ff"]), t_out=dpre), norm2=n_lo)
    return n_hi, n_lo, dpre, datt, dz_out


def _ffn_chain_param_grads(grads, layer, t, n_hi, n_lo, dpre, out_proj, att, valid, D):
    """What goes with _ffn_chain_launch: the parameter gradients of the two norms, linear2, linear1 and the out-projection
    fed by t[att].  valid (ops.HeadRows, below a packed score head): the weight gradients reduce over the valid caption
    rows only -- every other row of their dy operands is exactly zero."""
    _norm_param_grads(grads, n_hi)
    _norm_param_grads(grads, n_lo)
    _lin_bwd(grads, n_hi["do"], t["f"].view(D.M, -1), layer.linear2.weight, layer.linear2.bias, need_dx=False, valid=valid)
    _lin_bwd(grads, dpre, n_hi["res"].view(D.M, D.d), layer.linear1.weight, layer.linear1.bias, need_dx=False, valid=valid)
    _lin_bwd(grads, n_lo["do"], t[att].view(D.M, D.d), out_proj.weight, out_proj.bias, need_dx=False, valid=valid)


def _norm_bwd(grads, t, site, dx):
    norm, i, res = site
    return ops.layernorm_bwd(dx, t["o%d" % i], t[res], _p(norm.weight), t["m%d" % i], t["r%d" % i],
                             _g(grads, norm.weight), _g(grads, norm.bias), drop=t["d%d" % i])


def _ffn_plain_bwd(grads, layer, t, dx, hi, valid, D):
    """The feed-forward sublayer with the add & norm above it (site hi) on separate kernels -> gradient of its input."""
    dz, do = _norm_bwd(grads, t, hi, dx)
    dpre = _lin_bwd(grads, do.view(D.M, D.d), t["f"].view(D.M, -1), layer.linear2.weight, layer.linear2.bias,
                    gate=t["f"].view(D.M, -1), gate_scale=_keep_scale(t["d_ff"]),       # ReLU' (+ dropout) fused
                    valid=valid)
    return _lin_bwd(grads, dpre, t[hi[2]].view(D.M, D.d), layer.linear1.weight, layer.linear1.bias, dx=dz.view(D.M, D.d),
                    acc=True, valid=valid)


def _out_proj_plain_bwd(grads, t, dx, site, out_proj, att, valid, D):
    """An attention's out-projection with its add & norm on separate kernels -> (residual-path gradient, that of t[att])."""
    dz, do = _norm_bwd(grads, t, site, dx)
    return dz, _lin_bwd(grads, do.view(D.M, D.d), t[att].view(D.M, D.d), out_proj.weight, out_proj.bias, valid=valid)


def _self_attn_bwd(t, datt, lse, drop, causal, D):
    """Backward of a layer's self-attention over its head-major q|k|v -> the (M, 3 d) gradient of in_proj's output."""
    B, T, d = D.B, D.T, D.d
    dqkv = ops.attention_bwd_buffer((B, T, 3 * d), T, T, D.dh, D.dev)
    ops.attention_heads_bwd(t["qkv"], t["qkv"], t["sa"], datt.view(B, T, d), t[lse], dqkv[:, :, :d],
                            dqkv[:, :, d:2 * d], dqkv[:, :, 2 * d:], D.H, D.dh, T, T, 0, 1, 2, causal=causal, drop=t[drop])
    return dqkv.view(D.M, 3 * d)


def _in_proj_bwd(grads, attn, t, dqkv, dz, valid, D, hand_down=None):
    """Backward of a self-attention's in_proj -> the state (dz, g0, w0p) for what comes next.  hand_down (the packed
    in_proj_weight.T; chain path, a layer below exists): parameter gradients only, the data gradient dqkv @ W rides on
    that layer's first launch.  Else it is accumulated into dz."""
    args = (grads, dqkv, t["x"].view(D.M, D.d), attn.in_proj_weight, attn.in_proj_bias)
    if hand_down is not None:
        _lin_bwd(*args, need_dx=False, valid=valid)
        return dz, dqkv, hand_down
    return _lin_bwd(*args, dx=dz.view(D.M, D.d), acc=True, valid=valid), None, None


def _context_encoder_bwd_chain(dec, stack, tapes, grads, pkb, tag, g0, w0p):
    """A context encoder on the row chains (pkb: dec.weight_images().chain_t): one ops.rowchain_bwd launch per layer
    instead of six kernels.  The incoming gradient is g0 @ W0 (g0: a rows view, w0p: packed W0^T), no dx tensor."""
    layers = list(stack.layers)
    D = _dims(dec, tapes[0]["x"])
    state = (None, g0, w0p)
    for li in reversed(range(len(layers))):
        layer, t = layers[li], tapes[li]
        n2, n1, dpre, dsa, dz_out = _ffn_chain_launch(layer, t, (layer.norm2, 2, "x1"), (layer.norm1, 1, "x"), "soT", pkb,
                                                      (tag, li), state, D)
        if ops.SIDE is not None:
            ops.SIDE.flush()
        _ffn_chain_param_grads(grads, layer, t, n2, n1, dpre, layer.self_attn.out_proj, "sa", None, D)
        if ops.SIDE is not None and li > 0:
            # everything queued so far only needs the chain launch above: it goes out now, beside the attention
            # backward (the in_proj weight gradient follows with the next group) -- the side stream's last group,
            # which nothing on the main stream overlaps any more, shrinks to one problem
            ops.SIDE.flush_group()
        dqkv = _self_attn_bwd(t, dsa, "lse", "d_att", False, D)
        if ops.SIDE is not None:
            ops.SIDE.flush()
        state = _in_proj_bwd(grads, layer.self_attn, t, dqkv, dz_out, None, D, pkb[(tag, li, "siT")] if li > 0 else None)
        if ops.SIDE is not None and li == 0:
            # the stack's first layer is the last thing the backward pass computes: the main stream has
            # nothing left while the side stream still works off the layers above -- its weight gradients
            # run here instead of queueing behind them
            ops.SIDE.flush_group_here()
    return state[0].view(D.B, D.T, D.d)


def _context_encoder_bwd(dec, stack, tapes, dx, grads):
    """A context encoder on the separate GEMM / LayerNorm-backward kernels; dx (B, T, d): the gradient of its output."""
    D = _dims(dec, dx)
    for layer, t in zip(reversed(list(stack.layers)), reversed(tapes)):
        dx1 = _ffn_plain_bwd(grads, layer, t, dx, (layer.norm2, 2, "x1"), None, D)
        dz, dsa = _out_proj_plain_bwd(grads, t, dx1, (layer.norm1, 1, "x"), layer.self_attn.out_proj, "sa", None, D)
        dqkv = _self_attn_bwd(t, dsa, "lse", "d_att", False, D)
        dx = _in_proj_bwd(grads, layer.self_attn, t, dqkv, dz, None, D)[0]
        if ops.SIDE is not None:
            ops.SIDE.flush_group()      # this layer's weight gradients: one grouped launch
    return dx.view(D.B, D.T, D.d)


def _cross_attn_bwd(li, t, dca, dkv_rows, kv, S, D):
    """Backward of decoder layer li's cross-attention (K / V gradients: the layer's columns of dkv_rows) -> dq (B, T, d)."""
    dq = torch.empty(D.B, D.T, D.d, device=D.dev, dtype=torch.float32)
    c0 = 2 * li * D.d
    ops.attention_heads_bwd(t["qc"], kv, t["ca"], dca.view(D.B, D.T, D.d), t["lse_c"], dq, dkv_rows[:, :, c0:c0 + D.d],
                            dkv_rows[:, :, c0 + D.d:c0 + 2 * D.d], D.H, D.dh, D.T, S, 0, 2 * li, 2 * li + 1, drop=t["d_ca"])
    return dq


def _decoder_layer_bwd_chain(li, layer, t, state, dkv_rows, kv, S, grads, pkb, mem2, mem_t_ps, valid, D):
    """Backward of decoder layer li as two ops.rowchain_bwd launches around the cross-attention backward + the
    self-attention backward.  state = (dz, g0, w0p): the residual-path gradient of this layer's output, and -- from the
    layer above -- the in_proj gradient whose data gradient rides on this layer's first launch.  Returns the state
    for the layer below.  valid: see _ffn_chain_param_grads."""
    M, d = D.M, D.d
    n3, n2, dpre, dca, dz_a = _ffn_chain_launch(layer, t, (layer.norm3, 3, "x2"), (layer.norm2, 2, "x1"), "coT", pkb,
                                                ("d", li), state, D)
    if ops.SIDE is not None:
        ops.SIDE.flush()
    _ffn_chain_param_grads(grads, layer, t, n3, n2, dpre, layer.multihead_attn.out_proj, "ca", valid, D)
    # The layer's weight gradients go out in two grouped launches: linear2 / linear1 / cross out-projection + the two
    # norms' partials right behind the chain launch above, the rest at the layer's end (the side stream finishes last:
    # starting its work earlier shortens the step, 651 -> 654 k decode-steps/s; a third launch right behind the
    # cross-attention backward -- the K/V-projection weight gradient behind its operand -- costs more in fork points than
    # it gains: round 2 645 k, round 5 1.733 -> 1.739 ms, profiles/r05_x_ab_kv_wgrad_subgroups.txt)
    if ops.SIDE is not None:
        ops.SIDE.flush_group()
    dq = _cross_attn_bwd(li, t, dca, dkv_rows, kv, S, D)
    if ops.SIDE is not None:
        ops.SIDE.flush()
    _kv_proj_param_grads(layer, li, dkv_rows, mem2, grads, d, mem_t_ps)
    n1 = _norm_args(t, (layer.norm1, 1, "x"), D)
    dsa = torch.empty(M, d, device=D.dev, dtype=torch.float32)
    dz_b = torch.empty(M, d, device=D.dev, dtype=torch.float32)
    ops.rowchain_bwd(M, d, n1, pkb[("d", li, "soT")], dsa, dz_b, g0=dq.view(M, d), w0p=pkb[("d", li, "cqT")], dzin=dz_a)
    if ops.SIDE is not None:
        ops.SIDE.flush()
    _norm_param_grads(grads, n1)
    _lin_bwd(grads, dq.view(M, d), t["x1"].view(M, d), layer.multihead_attn.in_proj_weight,
             layer.multihead_attn.in_proj_bias, w_rows=slice(0, d), need_dx=False, valid=valid)
    _lin_bwd(grads, n1["do"], t["sa"].view(M, d), layer.self_attn.out_proj.weight, layer.self_attn.out_proj.bias,
             need_dx=False, valid=valid)
    dqkv = _self_attn_bwd(t, dsa, "lse_s", "d_sa", True, D)
    state = _in_proj_bwd(grads, layer.self_attn, t, dqkv, dz_b, valid, D, pkb[("d", li, "siT")] if li > 0 else None)
    if ops.SIDE is not None:
        ops.SIDE.flush_group()          # this layer's weight gradients: one grouped launch
    return state


def _decoder_layer_bwd(li, layer, t, dx, dkv_rows, kv, S, grads, mem2, mem_t_ps, valid, D):
    """Backward of decoder layer li on the separate kernels: the gradient dx of its output -> that of its input."""
    M, d = D.M, D.d
    dx2 = _ffn_plain_bwd(grads, layer, t, dx, (layer.norm3, 3, "x2"), valid, D)
    dz, dca = _out_proj_plain_bwd(grads, t, dx2, (layer.norm2, 2, "x1"), layer.multihead_attn.out_proj, "ca", valid, D)
    dq = _cross_attn_bwd(li, t, dca, dkv_rows, kv, S, D)
    # this layer's columns of the K/V-projection gradient are complete: its weight (and bias) gradient over
    # all B * S memory rows joins this layer's group instead of waiting for the whole decoder stack
    _kv_proj_param_grads(layer, li, dkv_rows, mem2, grads, d, mem_t_ps)
    dx1 = _lin_bwd(grads, dq.view(M, d), t["x1"].view(M, d), layer.multihead_attn.in_proj_weight,
                   layer.multihead_attn.in_proj_bias, w_rows=slice(0, d), dx=dz.view(M, d), acc=True, valid=valid)
    dz, dsa = _out_proj_plain_bwd(grads, t, dx1, (layer.norm1, 1, "x"), layer.self_attn.out_proj, "sa", valid, D)
    dqkv = _self_attn_bwd(t, dsa, "lse_s", "d_sa", True, D)
    dx0 = _in_proj_bwd(grads, layer.self_attn, t, dqkv, dz, valid, D)[0]
    if ops.SIDE is not None:
        ops.SIDE.flush_group()          # this layer's weight gradients: one grouped launch
    return dx0


def _kv_proj_param_grads(layer, li, dkv_rows, mem2, grads, d, mem_t_ps=None):
    """dW[d:3d] += dkv[:, layer columns].T @ memory, db[d:3d] += column sums (fused), for one decoder layer.
    mem_t_ps: the pre-split copy of memory^T (d x rows; made once per backward pass on the side stream): the product then
    runs on the LDS-DMA kernel of csrc/gemm_ps.hip (600 x 300 outputs over 13 824 rows: 75-88 -> ~50 us per layer) and the
    bias gradient becomes a plain column sum in the same side-stream group."""
    gw, gb = _g(grads, layer.multihead_attn.in_proj_weight), _g(grads, layer.multihead_attn.in_proj_bias)
    rows = mem2.shape[0]
    sl = dkv_rows.view(rows, -1)[:, 2 * li * d:(2 * li + 2) * d]
    if gw is not None:
        if mem_t_ps is not None:
            # 5 x 4 tiles of 128 x 80: K slices so that ~160 workgroups exist -- 8 slices, one per XCD (the kernel deals the
            # (slice, tile) pairs to the XCDs slice-major), half the float atomics of 16 slices and one workgroup per CU,
            # which leaves the CU's other slot to the main stream's kernels.  Sweeps inside the step: round 4
            # (profiles/r04_y_ab_bwd_splits.txt) 16 slices 1.695-1.705 ms against 12 / 24 / 32 at 1.711-1.720; round 5
            # (profiles/r05_x_ab_kv_wgrad_slices.txt) 8 slices 1.703-1.726 against 16 at 1.727-1.743 on the same boxes,
            # 4 / 6 / 10 / 24 slices 1.85 / 1.77 / 1.76 / 1.74-1.75
            split = max(1, min(32, 160 // (((2 * d + 127) // 128) * ((d + 79) // 80)), rows // 256))
            wg = ops.gemm_args(sl, mem2, gw[d:], 2 * d, d, rows, 1, sl.stride(0), 1, d, d, atomic=True, split_k=split,
                               b_ps=mem_t_ps)
            extra = [] if gb is None else [ops.colsum_problem(sl, gb[d:], split_k=max(1, min(16, rows // 512)))]
        else:
            wg = ops.gemm_args(sl, mem2, gw[d:], 2 * d, d, rows, 1, sl.stride(0), 1, d, d, atomic=True,
                               split_k=1 if ops.is_deterministic() else 16,
                               colsum_a=None if gb is None else gb[d:])
            extra = []
        if ops.SIDE is not None:
            ops.SIDE.add_problem(wg, dkv_rows, mem2, mem_t_ps)
            for e in extra:
                ops.SIDE.add_problem(e, dkv_rows)
        else:
            ops.gemm_grouped([wg] + extra)
    elif gb is not None:
        ops.colsum(sl, gb[d:])


def _memory_t_presplit(m, B, S, d):
    """Pre-split copy of memory^T (csrc/gemm_ps.hip's B operand for the cross K/V weight gradients), made where the side
    stream starts its backward work; None in the exact / deterministic modes."""
    if ops.gemm_split_mode() < 1 or ops.is_deterministic() or B * S < 2048:
        return None
    mem2 = m["mem"].view(B * S, d)
    buf = ops.presplit_buffer(d, B * S, mem2.device)

    def make():
        ops.presplit_weights([(mem2.t(), buf)])

    if ops.SIDE is not None:
        ops.SIDE.submit(make, mem2, buf)
    else:
        make()
    return buf


def _rows_t_presplit(x2, pack=None):
    """Pre-split copy of x2^T (x2: (rows, d) activations): the B operand of a weight gradient dW = dy^T @ x2 on
    csrc/gemm_ps.hip's kernel -- the vocabulary's (10 000 x 300 outputs over the 1 280 caption rows), made on the side
    stream in front of that gradient; None in the exact / deterministic modes and for few rows.
    pack (ops.HeadRows): the rows are gathered through pack.rowmap -- column m of the copy is the m-th valid row -- and
    only the pack.count valid ones are split (zeros up to the end of the last 32-row slice)."""
    rows, d = x2.shape
    if ops.gemm_split_mode() < 1 or ops.is_deterministic() or rows < 1024:
        return None
    buf = ops.presplit_buffer(d, rows, x2.device)

    def make():
        if pack is None:
            ops.presplit_weights([(x2.t(), buf)])
        else:
            ops.presplit_weights([(x2.t(), buf)], k_map=pack.rowmap, k_bound=pack.count)

    if ops.SIDE is not None:
        ops.SIDE.submit(make, x2, buf)
    else:
        make()
    return buf


def backward_from_tape(dec, tape, dscores, grads, overlap=True, want_image_grad=False, image_grad_sink=None):
    """Accumulate parameter gradients of `dec` into `grads` (dict id(param) -> zero-initialised
    tensor shaped like the parameter; frozen parameters are simply absent).  With `overlap` the weight /
    bias gradients of the Linear layers run on a second HIP stream beside the data-gradient chain.
    want_image_grad: also return the gradient of the (length-sorted) image memory rows (B, P, d) -- what
    fine_tune_encoder=True back-propagates into Encoder.conv1; the default step skips that 13.5 GFLOP GEMM because
    the reference never uses the result (geo-aware/train.py:93-100,283-284).
    image_grad_sink: callable(d_img) that consumes that gradient for the optimizer alone (TrainStep's conv1 weight
    gradient): with `overlap` the image-row gradient and the sink both run on the side stream, beside the context
    encoders' backward."""
    bp = BackwardPass(dec, tape, dscores, grads, overlap, want_image_grad, image_grad_sink)
    bp.early(join=False)     # one pass: the side stream is only joined at the very end
    bp.late()
    return tape.misc.get("d_img")


def early_parameters(dec):
    """Parameters whose gradients are complete after BackwardPass.early(): the score head and the decoder stack
    (54 % of the geo model's bytes).  The rest -- context encoders, embeddings -- completes in late()."""
    mods = [dec.fc_vocab, dec.fc_entity, dec.transformer_decoder]
    for name in ("fc_fact", "fc_predicate"):
        if getattr(dec, name, None) is not None:
            mods.append(getattr(dec, name))
    seen, out = set(), []
    for mod in mods:
        for prm in mod.parameters():
            if id(prm) not in seen:
                seen.add(id(prm))
                out.append(prm)
    return out


class BackwardPass:
    """The backward pass in two phases, so that a data-parallel step can start reducing the first half of the
    gradient bucket while the second half is still being computed (TrainStep with more than one rank):
    early() = score head + decoder stack, with the side stream joined at its end; late() = context encoders and
    embeddings.  The two phases may be captured into two hipGraphs."""

    def __init__(self, dec, tape, dscores, grads, overlap=True, want_image_grad=False, image_grad_sink=None):
        self.side = ops.SideStream() if overlap else None
        self.gen = _backward_phases(dec, tape, dscores, grads, want_image_grad, image_grad_sink)

    def _run(self, join):
        ops.SIDE = self.side
        try:
            next(self.gen, None)
        finally:
            ops.SIDE = None
            if self.side is not None and join:
                self.side.join()

    def early(self, join=True):
        self._run(join)
        self.joined = join

    def late(self):
        if self.side is not None and getattr(self, "joined", False):
            # the two phases may be captured into two graphs: each graph gets a side stream of its own (one stream
            # object forked into two captures made every kernel of both graphs run ~2.5x slower on ROCm 7.2)
            self.retired = self.side          # keeps the tensors the first phase's side work read alive
            self.side = ops.SideStream()
        self._run(True)


def _backward_phases(dec, tape, dscores, grads, want_image_grad=False, image_grad_sink=None):
    m = tape.misc
    V = dec.vocab_size
    h, ee, fe = m["h"], m["ee"], m["fe"]
    dims = _dims(dec, h)
    B, L, M, d, H, _, dev = dims
    # frozen parameters (other than the word embedding, whose scatter is simply skipped) get a scratch
    # buffer so every kernel has somewhere to accumulate; the scratch is dropped afterwards
    grads = dict(grads)
    for prm in unique_parameters(dec):
        if id(prm) not in grads and prm is not dec.word_embedding.weight:
            grads[id(prm)] = torch.zeros_like(prm)
    P, K, Fn, S = m["P"], m["K"], m["Fn"], m["S"]
    Vx = dscores.shape[2]
    dsc2 = dscores.view(M, Vx)
    pre = m.get("prezero") or {}

    def zeroed(name, like):
        t = pre.get(name)
        return t if t is not None and t.shape == like.shape else torch.zeros_like(like)

    dee = zeroed("dee", ee)
    dfe = zeroed("dfe", fe) if fe is not None else None
    # ---- score head
    hv = m["hv"] if dec.has_facts else h
    # the vocabulary weight gradient is a large problem of its own: it starts beside its data gradient
    dhv0 = pre.get("dhv")
    pack = m.get("pack")        # packed score head: dscores holds the valid rows only, packed at its top
    # below a packed head the gradient at every padded position is exactly zero all the way down the decoder stack: the
    # layers' weight gradients reduce over the valid rows only (ICK_NO_VALID_ROW_WGRAD=1: over all B * L).
    # Not in deterministic mode: there every gradient below the head is pinned bit-identical to the unpacked head's
    # (tests/test_packed_head_gpu.py), and packed rows fall into other 4-row MFMA groups than logical ones
    valid = pack if os.environ.get("ICK_NO_VALID_ROW_WGRAD", "0") in ("", "0") and not ops.is_deterministic() else None
    hv_t_ps = _rows_t_presplit(hv.view(M, d), pack) if _g(grads, dec.fc_vocab.weight) is not None else None
    # The data gradient's target.  Packed head: M' rows of data gradient, scattered into a zeroed logical buffer (the padded
    # positions stay exactly zero).  Else split-K partial sums add into the buffer the forward pass's side stream zeroed,
    # where there is one (not in deterministic mode: no split-K there); without a target the GEMM makes its own output
    if dhv0 is not None and (dhv0.shape != (M, d) or (pack is None and ops.is_deterministic())):
        dhv0 = None
    if dhv0 is None and pack is not None:
        dhv0 = torch.zeros(M, d, device=dev, dtype=torch.float32)
    dhv = _lin_bwd(grads, dsc2[:, :V], hv.view(M, d), dec.fc_vocab.weight, dec.fc_vocab.bias, dx=dhv0,
                   acc=dhv0 is not None, group_now=True, wt_ps=m.get("vocab_t_ps"), xt_ps=hv_t_ps, pack=pack).view(B, L, d)
    if dec.has_facts:
        dh = ops.mul(dhv, m["gate"])
        dgate = ops.mul(dhv, h)
        gw, gb = _g(grads, dec.fc_predicate.weight), _g(grads, dec.fc_predicate.bias)
        if gw is not None:
            ops.context_gate_bwd(m["captions"], m["facts"], dgate, gw, gb, K, V, mode=0)
    else:
        dh = dhv

    def gbuf(param):
        return _g(grads, param)

    ops.pointer_scores_bwd(dscores, V, h, ee, _p(dec.fc_entity.weight), None, dh, dee, gbuf(dec.fc_entity.weight),
                           gbuf(dec.fc_entity.bias), pack=pack, fused=True)
    if dec.has_facts:
        ops.pointer_scores_bwd(dscores, V + K, h, fe, _p(dec.fc_fact.weight), m["eib"], dh, dfe,
                               gbuf(dec.fc_fact.weight), gbuf(dec.fc_fact.bias), pack=pack, fused=True)
    # ---- decoder stack
    layers = list(dec.transformer_decoder.layers)
    nseg = 2 * len(layers)
    dkv_rows = ops.attention_bwd_buffer((B, S, nseg * d), L, S, d // H, dev)
    ops.stamp("bwd: head done")
    # the packed transposed weights exist only when dec.chain_bwd_supported() holds, and that covers a hand-down of
    # max(3, nseg) * d columns: pkb => the K/V projection's data gradient (nseg * d columns) fits the context encoders'
    # first chain launch as well
    pkb = m.get("pkb")
    mem_t_ps = _memory_t_presplit(m, B, S, d)
    mem2 = m["mem"].view(B * S, d)
    dx, state = dh, (dh.view(M, d), None, None)
    for li in reversed(range(len(layers))):
        if pkb is not None:
            state = _decoder_layer_bwd_chain(li, layers[li], tape.dec_layers[li], state, dkv_rows, m["kv"], S, grads,
                                             pkb, mem2, mem_t_ps, valid, dims)
            dx = state[0]
        else:
            dx = _decoder_layer_bwd(li, layers[li], tape.dec_layers[li], dx, dkv_rows, m["kv"], S, grads, mem2,
                                    mem_t_ps, valid, dims)
        ops.stamp("bwd: decoder layer %d done" % li)
    yield    # ---- end of the early phase: every gradient of early_parameters() has been enqueued
    # ---- cross K/V projection: the weight gradients went out with the decoder layers; data gradient for the
    # context rows only (the image rows' gradient would be Encoder.conv1's, which the reference never uses)
    nctx = K + Fn
    dkv_ctx = dkv_rows[:, P:]                       # (B, nctx, 2 * layers * d) view of the K/V gradient rows
    if pkb is None:
        # K = 2 * layers * d = 1800 over only B * nctx x d outputs: split the reduction (40 -> ~15 us with the fill)
        ksplit = max(1, min(8, (nseg * d) // 450)) if B * nctx * d <= 1280 * 512 else 1
        if ops.is_deterministic():
            ksplit = 1
        dctx = (torch.zeros if ksplit > 1 else torch.empty)(B, nctx, d, device=dev, dtype=torch.float32)
        ops.gemm_raw(dkv_ctx, m["wkv"], dctx, B * nctx, d, nseg * d, nseg * d, 1, 1, d, d, a_grp=nctx,
                     a_gs=S * nseg * d, atomic=ksplit > 1, split_k=ksplit)
    if want_image_grad:
        # image rows: d mem[:, :P] = dK/dV rows @ packed K/V weight (the data gradient of the all-layer projection)
        d_img = torch.empty(B, P, d, device=dev, dtype=torch.float32)

        def image_grad():
            ops.gemm_raw(dkv_rows, m["wkv"], d_img, B * P, d, nseg * d, nseg * d, 1, 1, d, d, a_grp=P, a_gs=S * nseg * d)
            if image_grad_sink is not None:
                image_grad_sink(d_img)

        # with a sink nothing on the main stream reads d_img: both launches go to the side stream (enqueued at the next
        # flush, behind the context encoders' first launch); ICK_CONV1_BWD_MAIN=1 keeps them on the main stream (A/B runs)
        if image_grad_sink is not None and ops.SIDE is not None and not os.environ.get("ICK_CONV1_BWD_MAIN"):
            ops.SIDE.submit(image_grad, dkv_rows, m["wkv"], d_img)
        else:
            image_grad()
        m["d_img"] = d_img
    # ---- context encoders.  With the row chains the data gradient of the K/V projection for the context rows rides on
    # the first launch of each context encoder's backward (its rows are read straight out of the K/V gradient buffer)
    ops.stamp("bwd: context gradient ready")

    def context_encoder_bwd(stack, name, tag, rows):
        if pkb is not None:
            return _context_encoder_bwd_chain(dec, stack, tape.enc_layers[name], grads, pkb, tag, dkv_ctx[:, rows],
                                              pkb[("kv", "T")])
        return _context_encoder_bwd(dec, stack, tape.enc_layers[name], dctx[:, rows].contiguous(), grads)

    dee_enc = context_encoder_bwd(dec.transformer_encoder_entities, "entities", "e", slice(0, K))
    ops.stamp("bwd: entity context encoder done")
    dee += dee_enc
    if dec.has_facts:
        dfe += context_encoder_bwd(dec.transformer_encoder_facts, "facts", "f", slice(K, None))
    # ---- caption embedding, fact encoder, entity encoder
    gword = _g(grads, dec.word_embedding.weight)
    ops.caption_embed_bwd(dx, m["captions"], m["masks"], gword, dee, dfe, V, dec.word_map["<pad>"], math.sqrt(d),
                          drop=m["d_pos"])
    if dec.has_facts:
        ops.fact_encode_bwd(dfe, m["facts"], dee, gbuf(dec.predicate_embedding.weight))
    ops.entity_encode_bwd(dec.variant, dee, m["entities"], ee, gbuf(dec.entity_encoder.type_embedding.weight),
                          word_emb=_p(dec.word_embedding.weight) if dec.variant == "news" else None,
                          dword=gword if dec.variant == "news" else None)


# ----------------------------------------------------------------------------------------------
# autograd bridge (drop-in for the reference's train.py)
# ----------------------------------------------------------------------------------------------
class DecoderGraphFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dec, captions, masks, entities, facts, enc_tok, gmap, *params):
        dec.__dict__["_drop_step"] = dec.__dict__.get("_drop_step", 0) + 1
        seed = (dec.__dict__.get("_drop_seed", 0x1234567) * 2654435761 + dec.__dict__["_drop_step"]) & 0xFFFFFFFF
        scores, tape = forward_with_tape(dec, captions, masks, entities, facts, enc_tok.detach(), gmap, seed=seed)
        ctx.dec, ctx.tape, ctx.params, ctx.gmap = dec, tape, params, gmap
        ctx.enc_shape = enc_tok.shape
        return scores

    @staticmethod
    def backward(ctx, dscores):
        dec, params = ctx.dec, ctx.params
        grads = {id(p): torch.zeros_like(p) for p in params if p.requires_grad}
        want_img = ctx.needs_input_grad[5]      # fine_tune_encoder=True: the loss reaches Encoder.conv1 through enc_tok
        d_img = backward_from_tape(dec, ctx.tape, dscores.contiguous(), grads, overlap=not ops.is_deterministic(),
                                   want_image_grad=want_img)
        d_enc = None
        if want_img:                            # the forward gathered the samples into length order through gmap
            d_enc = torch.empty(ctx.enc_shape, device=d_img.device, dtype=torch.float32)
            d_enc.index_copy_(0, ctx.gmap.long(), d_img) if ctx.gmap is not None else d_enc.copy_(d_img)
        return (None,) * 5 + (d_enc, None) + tuple(grads.get(id(p)) for p in params)


def unique_parameters(dec):
    seen, out = set(), []
    for p in dec.parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out.append(p)
    return out


# ----------------------------------------------------------------------------------------------
# learning-rate schedule and global-norm clip: the definitions
# ----------------------------------------------------------------------------------------------
LR_KINDS = ("constant", "inverse_sqrt", "cosine", "linear")


def check_lr_schedule(schedule):
    """dict(kind=, warmup_steps=W, total_steps=N, min_lr_ratio=r) -> the same with every key present and checked
    (None stays None).  W >= 0; inverse_sqrt needs W >= 1; cosine and linear need N > W; 0 <= r <= 1."""
    if schedule is None:
        return None
    if not isinstance(schedule, dict) or set(schedule) - {"kind", "warmup_steps", "total_steps", "min_lr_ratio"}:
        raise IckError("lr_schedule must be a dict of kind, warmup_steps, total_steps, min_lr_ratio; got %r" % (schedule,))
    kind = schedule.get("kind", "constant")
    if kind not in LR_KINDS:
        raise IckError("unknown lr_schedule kind %r (one of %s)" % (kind, ", ".join(LR_KINDS)))
    W, N, r = schedule.get("warmup_steps", 0), schedule.get("total_steps", 0), float(schedule.get("min_lr_ratio", 0.0))
    if int(W) != W or int(N) != N or W < 0 or not 0 <= N < 2 ** 31 or W >= 2 ** 31:
        raise IckError("lr_schedule: warmup_steps and total_steps must be integers >= 0, got %r, %r" % (W, N))
    if kind == "inverse_sqrt" and W < 1:
        raise IckError("lr_schedule inverse_sqrt needs warmup_steps >= 1")
    if kind in ("cosine", "linear") and not N > W:
        raise IckError("lr_schedule %s needs total_steps > warmup_steps, got %r <= %r" % (kind, N, W))
    if not 0.0 <= r <= 1.0:           # (NaN fails both compares)
        raise IckError("lr_schedule: min_lr_ratio must lie in [0, 1], got %r" % (r,))
    return dict(kind=kind, warmup_steps=int(W), total_steps=int(N), min_lr_ratio=r)


def lr_at(t, lr, schedule):
    """The learning rate of the 1-based optimizer step t under `schedule` with base rate lr, in float64: the definition
    the device schedule (csrc/opt_words.h) and the unfused path follow.
      constant      lr * min(1, t / W)                    (W = 0: lr)
      inverse_sqrt  lr * min(t / W, sqrt(W / t))
      cosine        t < W: lr * t / W, else lr * (r + (1 - r) * 0.5 * (1 + cos(pi * (min(t, N) - W) / (N - W))))
      linear        t < W: lr * t / W, else lr * (r + (1 - r) * (N - min(t, N)) / (N - W))"""
    sch = check_lr_schedule(schedule)
    t, lr = float(t), float(lr)
    if sch is None:
        return lr
    kind, W, N, r = sch["kind"], float(sch["warmup_steps"]), float(sch["total_steps"]), sch["min_lr_ratio"]
    if kind == "inverse_sqrt":
        return lr * min(t / W, math.sqrt(W / t))
    if t < W:
        return lr * (t / W)
    if kind == "constant":
        return lr
    tt = min(t, N)
    if kind == "cosine":
        return lr * (r + (1.0 - r) * 0.5 * (1.0 + math.cos(math.pi * (tt - W) / (N - W))))
    return lr * (r + (1.0 - r) * (N - tt) / (N - W))


def check_ema_decay(d):
    """None (no moving average) or a float in [0, 1)."""
    if d is None:
        return None
    d = float(d)
    if not 0.0 <= d < 1.0:            # (NaN fails both compares)
        raise IckError("ema_decay must lie in [0, 1) (None: off), got %r" % (d,))
    return d


def ema_decay_at(t, decay, warmup=False):
    """The decay d_t of the moving average at the 1-based optimizer step t, in float64: the definition the optimizer
    kernels (csrc/adam.hip, in float32) and the unfused path follow.  Without warmup the decay itself; with it
    min(decay, (1 + t) / (10 + t)), so the average follows the first steps' weights instead of the initial ones."""
    decay, t = float(decay), float(t)
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def check_weight_decay(wd):
    """None (no weight decay) or a finite float >= 0."""
    if wd is None:
        return None
    wd = float(wd)
    if not (wd >= 0.0 and math.isfinite(wd)):       # (NaN fails the compare)
        raise IckError("weight_decay must be a finite float >= 0 (None: off), got %r" % (wd,))
    return wd


def default_decay_filter(name, param):
    """What weight decay covers by default: matrices and embedding tables (ndim >= 2), not biases, norm scales or the
    1-element parameters."""
    return param.ndim >= 2


def check_max_grad_norm(m):
    if m is None:
        return None
    m = float(m)
    if not m > 0.0:                   # (NaN fails the compare)
        raise IckError("max_grad_norm must be a float > 0 (None: off), got %r" % (m,))
    return m


# ----------------------------------------------------------------------------------------------
# scheduled sampling: the definitions
# ----------------------------------------------------------------------------------------------
SAMPLING_MODES = ops.SCHED_SAMPLE_MODES


def check_sampling_prob(p):
    p = float(p)
    if not 0.0 <= p <= 1.0:           # (NaN fails both compares)
        raise IckError("scheduled_sampling: prob must lie in [0, 1], got %r" % (p,))
    return p


def check_sampling_temperature(T):
    T = float(T)
    if not (T > 0.0 and math.isfinite(T)):
        raise IckError("scheduled_sampling: temperature must be a finite float > 0, got %r" % (T,))
    return T


def check_scheduled_sampling(ss):
    """dict(prob=0.25, mode="sample" | "argmax", temperature=1.0, seed=None) -> the same with every key present and
    checked (None stays None).  0 <= prob <= 1, temperature > 0; seed None: the step's own seed."""
    if ss is None:
        return None
    if not isinstance(ss, dict) or set(ss) - {"prob", "mode", "temperature", "seed"}:
        raise IckError("scheduled_sampling must be a dict of prob, mode, temperature, seed; got %r" % (ss,))
    mode = ss.get("mode", "sample")
    if mode not in SAMPLING_MODES:
        raise IckError("scheduled_sampling: unknown mode %r (one of %s)" % (mode, ", ".join(SAMPLING_MODES)))
    seed = ss.get("seed")
    if seed is not None and (isinstance(seed, bool) or int(seed) != seed or not -2 ** 63 <= seed < 2 ** 64):
        raise IckError("scheduled_sampling: seed must be an integer of at most 64 bits or None, got %r" % (seed,))
    return dict(prob=check_sampling_prob(ss.get("prob", 0.25)), mode=mode,
                temperature=check_sampling_temperature(ss.get("temperature", 1.0)), seed=None if seed is None else int(seed))


def sampling_prob_at(epoch, start, increase_every, increase_prob, max_prob):
    """The usual staircase of the scheduled-sampling probability over the epochs: 0 before `start` (and for start < 0:
    off), then min(max_prob, increase_prob * ((epoch - start) // increase_every + 1))."""
    if increase_every < 1:
        raise IckError("sampling_prob_at: increase_every must be an integer >= 1, got %r" % (increase_every,))
    if start < 0 or epoch < start:
        return 0.0
    return min(float(max_prob), float(increase_prob) * ((int(epoch) - int(start)) // int(increase_every) + 1))


# ----------------------------------------------------------------------------------------------
# fused data-parallel training step
# ----------------------------------------------------------------------------------------------
class TrainStep:
    """forward -> packed CE -> backward -> all-reduce -> clamp + Adam over one flat fp32 bucket.

    Gradient semantics equal the single-process full-batch step of the reference: every rank
    contributes the SUM of its token losses' gradients plus its token count; after the
    all-reduce(sum) the bucket is divided by the global token count, clamped to +-grad_clip
    (geo-aware/train.py:287-288 clamps the full-batch gradient) and fed to Adam (lr 4e-4).

    With use_graph the device work is two captured hipGraphs around the (eager) collective:
      A  zero the bucket, forward with saved activations, packed cross entropy, backward -- the
         weight / bias gradients run on a second stream beside the data-gradient chain (fork/join
         edges of the graph);
      B  divide by the reduced token count, clamp, Adam, bump the step counter.
    The step counter lives on the device: it seeds the dropout masks and Adam's bias correction, so
    replays advance without re-capturing."""

    def __init__(self, decoder, lr=4e-4, grad_clip=5.0, betas=(0.9, 0.999), eps=1e-8, process_group=None, seed=0,
                 use_graph=True, encoder=None, deterministic=None, lazy_update=False, label_smoothing=0.0,
                 max_grad_norm=None, lr_schedule=None, train_conv1=False, encoder_lr=1e-4, ema_decay=None,
                 ema_warmup=False, weight_decay=None, decoupled_weight_decay=True, decay_filter=None,
                 encoder_weight_decay=None, scheduled_sampling=None):
        self.dec = decoder
        # scheduled_sampling (dict(prob=0.25, mode="sample" | "argmax", temperature=1.0, seed=None); None: off; DESIGN.md
        # 3.1l): the two-pass scheduled sampling of a Transformer decoder.  Part A starts with a FIRST PASS -- the inference
        # layers on the gold captions, without dropout whatever the module's mode (the decoder as it will decode, the
        # choice score_captions makes), the packed score head over the valid rows and ick_sched_sample_mix, which replaces
        # each fed token with the model's own prediction for that position with probability prob (drawn through Gumbel
        # noise at `temperature`, or the argmax).  The existing pass then runs on the mixed captions / masks -- embedding,
        # context indicators, predicate gate and every backward kernel that reads the fed tokens follow them -- against the
        # GOLD targets.  prob, temperature and the seed (None: the step's own) live in device words (set_sampling_prob /
        # set_sampling_temperature replay the captured graphs); the coin and the noise take the step's device counter, so
        # every replay draws anew; whether there is sampling and its mode are part of the graph key.  sampled_inputs()
        # hands out the last step's (captions_in, masks_in, replaced).  The first pass has to see the newest weights: such
        # a step applies its update eagerly, lazy_update does not defer it (_lazy_active is false).  It reads the weight
        # images the second pass of the same step reads.  The mix is rank-local: no collective changes.  Not with
        # caption_weights or image_index (SelfCriticalStep trains on sampled captions already).  None: nothing is
        # allocated, the same launches.
        self.ss = check_scheduled_sampling(scheduled_sampling)
        self._ss_words = self._ss_out = None
        self._ss_bufs, self._ss_first = {}, {}        # (B, L) -> the mix kernel's outputs; graph key -> the first pass's graph
        self._ss_inline = os.environ.get("ICK_SS_ONE_GRAPH", "0") not in ("", "0")
        # weight_decay (finite float >= 0; None: off): weight decay inside the optimizer launch, on the
        # decoder's parameters that decay_filter(name, param) selects (default: param.ndim >= 2 -- matrices and embedding
        # tables, not biases, norm scales or 1-element parameters).  decoupled_weight_decay=True is torch.optim.AdamW
        # (p *= 1 - lr_t * wd ahead of the update, lr_t the rate the update uses, scheduled or not); False is
        # torch.optim.Adam(weight_decay=): wd * p joins the clamped gradient the moments see; max_grad_norm keeps
        # measuring the gradient without the term and flat_g keeps it without the term.  encoder_weight_decay (needs
        # train_conv1): the same for conv1.weight (never conv1.bias), at encoder_lr.  The values live in one-float device
        # words (set_weight_decay / set_encoder_weight_decay replay the captured graphs); whether there is decay, its form
        # and the selection are fixed at construction.  A step without tokens applies no update and so no decay (torch
        # would decay on such a step; here the step does not exist).  Decay is a function of replicated state: no
        # collective.  A hyper-parameter like grad_clip: state_dict() reports it per parameter, load_state_dict ignores
        # stored values.  None: nothing is allocated, the same launches.
        self.weight_decay = check_weight_decay(weight_decay)
        self.encoder_weight_decay = check_weight_decay(encoder_weight_decay)
        self.decoupled_weight_decay = bool(decoupled_weight_decay)
        self._decay_filter = decay_filter if decay_filter is not None else default_decay_filter
        self._wd_word = self._wd_mask = self._enc_wd_word = self._enc_wd_mask = None
        self._decayed = []
        if self.encoder_weight_decay is not None and not train_conv1:
            raise IckError("encoder_weight_decay needs train_conv1=True: the step trains no encoder parameter without it")
        # ema_decay (float in [0, 1); None: off): an exponential moving average of every trained parameter
        # (conv1's with train_conv1), e += (1 - d_t) (p - e) after each applied update, kept by the optimizer launch itself
        # in flat_e / enc_e, laid out like flat_p / enc_p and starting as copies of them.  d_t = ema_decay, or with
        # ema_warmup min(ema_decay, (1 + t) / (10 + t)) on the optimizer step t.  The decay lives in a one-float device word
        # (set_ema_decay replays the captured graphs); whether there is an average is fixed at construction.  The average
        # is a function of parameters that are identical on every rank, so it needs no collective.  ema_state_dict() /
        # load_ema_state_dict() carry it; state_dict() is unchanged.  None: nothing is allocated, the same launches.
        self.ema_decay = check_ema_decay(ema_decay)
        self.ema_warmup = bool(ema_warmup)
        self.flat_e = self.enc_e = self._ema_word = None
        self._ema_swapped = False
        # train_conv1 (needs encoder= and the 4-D feature map as encoder_out): Encoder.conv1 is trained
        # inside the step as the reference's fine_tune_encoder=True trains it (geo-aware/train.py:93-100,283-294): the
        # backward pass also produces the image rows' gradient and ick_conv1_wgrad reduces it against the feature map;
        # conv1's gradient travels behind the decoder's in the same bucket (one all-reduce), is divided by the same token
        # count, clamped by grad_clip and fed to an Adam of its own (encoder_lr, this step's betas / eps and step counter).
        # max_grad_norm and lr_schedule keep covering the decoder's parameters only.  False: nothing changes.
        self.train_conv1 = bool(train_conv1)
        self.encoder_lr = float(encoder_lr)
        if self.train_conv1 and encoder is None:
            raise IckError("train_conv1=True needs encoder=: the step cannot reach Encoder.conv1 without it")
        # max_grad_norm (float > 0; None: off): torch.nn.utils.clip_grad_norm_(params, m, norm_type=2) on the
        # token-mean gradient of the global batch, BEFORE the element clamp grad_clip (grad_clip=None: no clamp).
        # lr_schedule (dict(kind=, warmup_steps=, total_steps=, min_lr_ratio=), see lr_at; None: the fixed rate lr): the
        # rate of optimizer step t = device step counter + 1.  With either one the base rate, max_norm, the norm, the clip
        # coefficient and the rate used live in a few device words (self._words) that the optimizer kernels read and
        # write: set_lr() / set_max_grad_norm() / a warmup replay the captured graphs, and grad_norm, clip_coef, lr_now
        # read the last applied update's values without a host synchronisation.  With neither, nothing changes: the same
        # kernels, graphs and set_lr as before.  Hyper-parameters like grad_clip: not part of state_dict() -- the position
        # in the schedule follows from the step count.
        self.max_grad_norm = check_max_grad_norm(max_grad_norm)
        self.lr_schedule = check_lr_schedule(lr_schedule)
        self._words = self._norm_scratch = None
        # label_smoothing (0 <= eps < 1): the loss of torch's CrossEntropyLoss(label_smoothing=eps), and
        # the returned loss is that smoothed loss.  Exactly 0.0 launches the plain cross entropy; a non-zero value lives
        # in a one-float device word the smoothed kernel reads, so set_label_smoothing() between two non-zero values
        # replays the captured graphs.  With caption_weights (SelfCriticalStep) the row's smoothed loss and gradient are
        # multiplied by the caption's weight, the count stays unweighted.  A hyper-parameter like grad_clip: not part of
        # state_dict().
        self.label_smoothing = self._check_smoothing(label_smoothing)
        self._eps_word = None
        # lazy_update: the optimizer update of step i runs at the head of step i + 1's graph, on the side stream beside
        # Encoder.conv1 (see forward_with_tape's pre_side) instead of as a graph of its own at the end of step i, where
        # nothing overlaps its ~85 us of HBM streaming.  Between two calls the parameters then lag one update behind the
        # gradients: flush() applies the pending update (state_dict / load_state_dict / set_lr / as_torch_optimizer do it
        # themselves; call it before reading the decoder's parameters, validating or checkpointing).  Same arithmetic,
        # same order of optimizer steps; needs the captured two-stream step with the feature-map input (encoder=) and the
        # optimizer-maintained weight images, else the update stays where it was.
        self.lazy = bool(lazy_update)
        # the score head over the packed list of valid caption rows; ICK_NO_PACKED_HEAD=1 restores the
        # head over all B * L positions (A/B runs)
        self.packed_head = os.environ.get("ICK_NO_PACKED_HEAD", "0") in ("", "0")
        self._pending = False
        self._gb = None
        # deterministic (default: ICK_DETERMINISTIC=1 in the environment): the library's fixed-order reductions, no
        # split GEMMs, everything on one stream -- two runs of the same steps end bit-identical (cost: DESIGN.md)
        # None inherits the library's current mode (ick_get_deterministic: ICK_DETERMINISTIC in the environment unless
        # ops.set_deterministic was called); only an explicit True / False changes the process-wide flag, and a step
        # refuses to run when the flag no longer is what its graphs were captured under.
        if deterministic is None:
            deterministic = ops.is_deterministic()
        else:
            ops.set_deterministic(bool(deterministic))
        self.deterministic = bool(deterministic)
        # with an encoder the step also accepts the (B, 2048, 14, 14) feature map: Encoder.conv1 (frozen, as in the
        # reference's default fine_tune_encoder=False) then runs inside graph A straight into the memory buffer
        self.enc = encoder
        self.seed = seed  # dropout mask stream; give every rank its own seed
        self.lr, self.clip, self.betas, self.eps = lr, (0.0 if grad_clip is None else grad_clip), betas, eps
        self.pg = process_group
        self.use_graph = use_graph
        self.step_count = 0
        params = [p for p in unique_parameters(decoder) if p.requires_grad]
        # bucket order: the parameters whose gradients are complete first come first, so that with several ranks
        # their part of the bucket can be all-reduced while the rest of the backward pass still runs
        early_ids = {id(p) for p in early_parameters(decoder)}
        params = [p for p in params if id(p) in early_ids] + [p for p in params if id(p) not in early_ids]
        dev = params[0].device
        if self.train_conv1 and encoder.conv1.weight.device != dev:
            raise IckError("train_conv1=True: the encoder must be on the decoder's device (%s)" % dev)
        # The state lives in ParamBuckets (bucket.py: the layout, the parameters as views of it): the decoder's and, with
        # train_conv1, one over [conv1.weight, conv1.bias].  The flat_* / enc_* names are those buckets' tensors.
        self._dec_bucket = db = ParamBucket(params, IckError)
        self._buckets = [db]
        self.params, self.n = params, db.n
        self.n_early = db.offsets[sum(id(p) in early_ids for p in params)]      # the early parameters come first
        self.flat_p, self.flat_m, self.flat_v = db.p, db.m, db.v
        # train_conv1: conv1's extent lies between the decoder's n floats and the trailing words, so the one all-reduce
        # carries it; self.n stays the decoder's size
        self.ne = 0
        if self.train_conv1:
            c1 = encoder.conv1
            self._enc_bucket = eb = ParamBucket([c1.weight, c1.bias], IckError)
            self._buckets.append(eb)
            self.enc_params, self.ne = eb.params, eb.n
            self.enc_p, self.enc_m, self.enc_v = eb.p, eb.m, eb.v
            encoder.invalidate_caches()          # the weight moved: its pre-split copy is made again on first use
        # one gradient allocation: [decoder n | conv1 ne | sum of token losses, token count]
        self._t = self.n + self.ne              # where [sum of token losses, token count] start in flat_g
        self.flat_g = torch.zeros(self._t + 2, device=dev, dtype=torch.float32)
        self.grads = db.grad_views(self.flat_g[:self.n])
        if self.train_conv1:
            self.enc_g = self.flat_g[self.n:self._t]
            eg = eb.grad_views(self.enc_g)
            self._c1_gw, self._c1_gb = eg[id(c1.weight)].view(c1.weight.shape[0], -1), eg[id(c1.bias)]
        self.counter = torch.zeros(1, device=dev, dtype=torch.int32)   # steps done (read as uint32 by the kernels)
        # this rank's token-mean loss, written by the loss's reduction launch: __call__ returns it at world
        # size 1 -- the step's own buffer, written again by the next step (clone() to keep a value)
        self._mean = torch.zeros(1, device=dev, dtype=torch.float32)
        self._adam_ticket = ops.adam_ticket(dev)      # the deferred update's (it runs on the side stream: a word of its own)
        self.one = torch.ones(1, device=dev, dtype=torch.float32)
        if self.max_grad_norm is not None or self.lr_schedule is not None:
            self._make_words()
        if self.label_smoothing != 0.0:
            self._eps_word = torch.full((1,), self.label_smoothing, device=dev, dtype=torch.float32)
        if self.ema_decay is not None:
            self._ema_word = torch.full((1,), self.ema_decay, device=dev, dtype=torch.float32)
        if self.ss is not None:
            sd = (self.seed if self.ss["seed"] is None else self.ss["seed"]) & (2 ** 64 - 1)
            self._ss_words = (torch.full((1,), self.ss["prob"], device=dev, dtype=torch.float32),
                              torch.full((1,), self.ss["temperature"], device=dev, dtype=torch.float32),
                              torch.tensor([sd - 2 ** 64 if sd >= 2 ** 63 else sd], device=dev, dtype=torch.int64))
        if self.weight_decay is not None:
            names = {}
            for name, p in decoder.named_parameters():
                names.setdefault(id(p), name)
            self._decayed = [(names[id(p)], p) for p in params if self._decay_filter(names[id(p)], p)]
            self._wd_word = torch.full((1,), self.weight_decay, device=dev, dtype=torch.float32)
            self._wd_mask = db.decay_mask(p for _, p in self._decayed)
        if self.encoder_weight_decay is not None:
            self._enc_wd_word = torch.full((1,), self.encoder_weight_decay, device=dev, dtype=torch.float32)
            self._enc_wd_mask = eb.decay_mask([encoder.conv1.weight])
        self._graphs = {}
        # the re-laid-out copies of the weights (packed row-chain images, cross K/V gather, bf16 planes) that the optimizer
        # kernel keeps current itself: built on the first call (DerivedWeights); ICK_ADAM_DERIVE=0 keeps the per-step
        # packing launches of rounds 2-4 instead (A/B runs, and the fallback for layer widths the images do not cover)
        self.derived = None
        self._derived_tried = False
        # several ranks: every replica starts from rank 0's weights (a freshly built decoder is randomly initialised
        # per process; the reference has a single process, geo-aware/train.py:16-18).  One broadcast of the bucket.
        # (the moments start at zero everywhere, and the averages start at the broadcast parameters)
        for b in self._buckets:
            dp.broadcast_bucket(b.p, self.pg)
            if self.ema_decay is not None:
                b.start_average()
        self.flat_e = self._dec_bucket.e
        if self.train_conv1:
            self.enc_e = self._enc_bucket.e
        # Several ranks, ICK_SPLIT_ALLREDUCE=1: the step runs as two graphs around two all-reduces -- the early half of
        # the bucket (score head, decoder stack: gradients complete first) travels while the late half (cross K/V
        # projection, context encoders, embeddings) is computed, and only the late half's all-reduce is exposed.  Measured
        # on one GPU the split itself costs ~130 us (a join in the middle of the backward pass, one more graph launch),
        # and nothing has been measured on a multi-GPU node to win that back, so the DEFAULT IS OFF (one all-reduce
        # between graph A and graph B) until a scaling run shows the gain; same bits either way
        # (tests/test_deterministic_gpu.py).  ICK_SPLIT_ALLREDUCE=auto decides from a timed all-reduce of the bucket at
        # construction (split when the collective costs more than twice what the split does; every rank takes the
        # max-reduced time, so every rank decides alike).  allreduce_probe_ms keeps that measurement for bench.py.
        env = os.environ.get("ICK_SPLIT_ALLREDUCE", "0")
        self.allreduce_probe_ms = None
        if dp.world_size(self.pg) > 1 and (env == "auto" or os.environ.get("ICK_ALLREDUCE_PROBE") == "1"):
            self.allreduce_probe_ms = dp.time_all_reduce(self.flat_g, self.pg)
        if env == "auto":
            self.split = self.allreduce_probe_ms is not None and self.allreduce_probe_ms > 0.26
        else:
            self.split = env not in ("", "0")       # an explicit 1 also splits a single rank's step (tests, A/B runs)

    # ---- device-only halves -------------------------------------------------------------------
    def _overlap(self, off_switch):
        """Second-stream work (context chains beside the image projection, weight gradients beside the data-gradient
        chain): in captured steps, unless switched off -- and never in deterministic mode, where every buffer must
        receive its terms in one fixed order."""
        if self.deterministic:
            return False
        return bool((self.use_graph or os.environ.get("ICK_GROUP_SAME_STREAM")) and not os.environ.get(off_switch))

    def _enc_kwargs(self, enc_in):
        if enc_in.dim() == 4:
            c1 = self.enc.conv1
            return dict(enc_tok=None, feats=enc_in, conv1=(c1.weight.detach(), c1.bias.detach(), self.enc.conv1_presplit()))
        return dict(enc_tok=enc_in)

    @staticmethod
    def _check_smoothing(eps):
        eps = float(eps)
        if not 0.0 <= eps < 1.0:          # (NaN fails both compares)
            raise IckError("label_smoothing must lie in [0, 1), got %r" % (eps,))
        return eps

    def set_label_smoothing(self, eps):
        """A new label-smoothing value.  Between two non-zero values only the device word is written and the captured
        graphs replay; moving between zero and non-zero changes the loss kernel, which is part of the graph key, so the
        next step captures once for the new kind (graphs of the other kind are kept).  No flush(): eps shapes the
        gradients of the steps to come, not a pending update."""
        eps = self._check_smoothing(eps)
        if eps != 0.0:
            if self._eps_word is None:
                self._eps_word = torch.empty(1, device=self.flat_p.device, dtype=torch.float32)
            self._eps_word.fill_(eps)
        self.label_smoothing = eps

    # ---- global-norm clip and learning-rate schedule: the optimizer words --------
    def _make_words(self):
        """The optimizer words (include/ick_amd.h: base lr, max_norm, norm, coef, lr used, sum of squares) and the norm
        pass's scratch.  From here on _adam() gives ick_adam_step[_derive] the words, which then hold the rate."""
        dev = self.flat_p.device
        if self._words is None:
            w = [0.0] * 8
            w[0], w[1], w[3] = float(self.lr), self.max_grad_norm or 0.0, 1.0
            self._words = torch.tensor(w, device=dev, dtype=torch.float32)
            self._sched = ops.lr_schedule_struct(self.lr_schedule)
        if self.max_grad_norm is not None and self._norm_scratch is None:
            self._norm_scratch = torch.empty(ops.grad_sqnorm_plan(self.n)[2], device=dev, dtype=torch.float32)

    def _word(self, i, what):
        if self._words is None:
            raise IckError("%s needs a TrainStep built with max_grad_norm= or lr_schedule=" % what)
        return self._words[i:i + 1]

    @property
    def grad_norm(self):
        """1-element device tensor: the L2 norm of the token-mean gradient of the last applied update, before any clip
        (a view of the optimizer words: clone() to keep a value; 0 until max_grad_norm is on and an update ran)."""
        return self._word(2, "grad_norm")

    @property
    def clip_coef(self):
        """1-element device tensor: min(1, max_grad_norm / (grad_norm + 1e-6)) of the last applied update."""
        return self._word(3, "clip_coef")

    @property
    def lr_now(self):
        """1-element device tensor: the learning rate the last applied update used (base rate times the schedule)."""
        return self._word(4, "lr_now")

    def set_max_grad_norm(self, m):
        """A new bound of the global-norm clip.  Between two positive values only the device word is written and the
        captured graphs replay; switching the clip on or off (None) adds or removes the norm pass, so the next step
        captures again.  A pending (lazy_update) update is applied first, under the old bound."""
        m = check_max_grad_norm(m)
        self.flush()
        if (m is None) != (self.max_grad_norm is None):
            self._graphs.clear()
        self.max_grad_norm = m
        if m is None and self._words is None:
            return
        self._make_words()
        self._words[1:2].fill_(m or 0.0)
        if m is None:
            self._words[3:4].fill_(1.0)       # nothing recomputes the coefficient any more

    def _loss(self, scores, captions, decode_len, weights, pack=None):
        """Packed cross entropy into the tail of the gradient bucket (it was zeroed by the side tail; nothing else touches
        those two floats); with per-caption weights (SelfCriticalStep's advantages) the weighted form.  pack: the scores
        are the packed rows of the valid positions, and so are the score gradients.  With label smoothing on, the
        smoothed entry in the same layout."""
        tail = dict(want_grad=True, out_sum=self.flat_g[self._t:self._t + 1], out_count=self.flat_g[self._t + 1:],
                    mean=self._mean)
        pad = self.dec.word_map["<pad>"]
        if self.label_smoothing != 0.0:
            return ops.packed_ce_smooth(scores, captions, pack if pack is not None else decode_len, pad, self._eps_word,
                                        weights=weights, **tail)
        if pack is not None:
            return ops.packed_ce_rows(scores, captions, pack, pad, weights=weights, **tail)
        if weights is None:
            return ops.packed_ce(scores, captions, decode_len, pad, **tail)
        return ops.packed_ce_weighted(scores, captions, decode_len, weights, pad, **tail)

    def _side_tail(self, box, captions, entities, facts, lengths):
        """Work of a step that nothing in the forward pass waits for (forward_with_tape runs it on the side stream behind
        the context chain): zeroing the gradient bucket and the backward pass's accumulation targets, and the decode
        lengths -- with the packed score head (the default; ICK_NO_PACKED_HEAD=1: every position runs through the head,
        as before) one row-map launch that also lists the valid rows."""
        def tail():
            self.flat_g.zero_()
            if self.packed_head:
                box["pack"] = ops.HeadRows(lengths, captions.shape[0], captions.shape[1])
                box["decode_len"] = box["pack"].decode_len
            else:
                box["decode_len"] = (lengths.reshape(-1) - 1).to(torch.int32)
            box["prezero"] = _prezeroed(self.dec, captions, entities, facts)

        return tail

    def _forward_and_loss(self, captions, caption_masks, entities, facts, enc_in, gmap, lengths, weights=None):
        """Part A up to the backward pass, for the one-graph and the split step alike: the side tail, the forward pass with
        saved activations and the loss -> the (args, kwargs) of the backward pass, which _part_a runs in one go and
        _part_a1 / _part_a2 in two phases.  The lazy hooks are None in the split step (_lazy_active is false there)."""
        box = {}
        lazy = self._lazy_active(enc_in)
        fed, fed_masks = captions, caption_masks      # the targets stay `captions`, whatever is fed
        if self.ss is not None:
            # the first pass has written the mixed inputs: in a graph of its own in front of this one, or (A/B runs) here
            if self._ss_inline:
                self._first_pass(captions, caption_masks, entities, facts, enc_in, gmap, lengths)
            fed, fed_masks = self._ss_bufs[tuple(captions.shape)][:2]
        scores, tape = forward_with_tape(self.dec, fed, fed_masks, entities, facts, gmap=gmap,
                                         seed=self.seed * 2654435761 & 0xFFFFFFFF, epoch=self.counter, fresh_pack=True,
                                         overlap=self._overlap("ICK_NO_FWD_OVERLAP"),
                                         side_tail=self._side_tail(box, captions, entities, facts, lengths),
                                         derived=self.derived, pre_side=self._deferred_update if lazy else None,
                                         pre_main=self._adam_conv1 if self.train_conv1 and lazy else None,
                                         head_rows=lambda: box.get("pack"), **self._enc_kwargs(enc_in))
        tape.misc["prezero"] = box.get("prezero")
        ops.stamp("fwd: scores done")
        ce = self._loss(scores, captions, box["decode_len"], weights, box.get("pack"))
        ops.stamp("CE done")
        return (self.dec, tape, ce[2], self.grads), dict(self._conv1_bwd_kwargs(enc_in),
                                                         overlap=self._overlap("ICK_NO_BWD_OVERLAP"))

    # ---- scheduled sampling (scheduled_sampling=) ---------------------------------
    def _first_pass(self, captions, caption_masks, entities, facts, enc_in, gmap, lengths, weights=None):
        """The first pass of a step with scheduled sampling (part A's argument list), into the step's (captions_in, masks_in,
        replaced) buffers: the inference layers on the gold prefix (no dropout, nothing saved), a head hook that lists the
        valid rows, runs the packed score head over them and the mix kernel.  The pass reads the re-laid-out weights
        through dec.weight_images(), the very buffers the second pass reads: with DerivedWeights the optimizer launch has
        just written them (they are stamped current, no launch); without, they are filled here from the live parameters,
        unconditionally -- a launch whose presence must not depend on what the host believes while a graph is captured.
        Captured steps replay it as a graph of its own in front of graph A, the structure of score_captions' graph (cfg2
        step 4.95 ms; 5.17 ms with the pass captured inside graph A, which ICK_SS_ONE_GRAPH=1 keeps for A/B runs; DESIGN.md
        3.1l)."""
        dec = self.dec
        B, Lc = captions.shape
        V, K = dec.vocab_size, entities.shape[1]
        Fn = facts.shape[1] if dec.has_facts else 0
        wm = dec.word_map
        wi = dec.weight_images()
        groups = ["kv"] + (["chain"] if dec.chain_supported() else []) + (["pred_wt"] if dec.has_facts else [])
        if ops.gemm_split_mode() != 0:
            groups += ["kv_ps"] + (["vocab_ps"] if vocab_planes_wanted(B * Lc) else [])
        if self.derived is not None:
            wi.adopt(*groups)
        else:
            wi.refresh(*groups)
        out = self._ss_bufs[(B, Lc)]

        def head(x, ee, fe, eib, hv):
            pack = ops.HeadRows(lengths, B, Lc)
            Vx = V + K + Fn
            ld = (Vx + 3) // 4 * 4          # 16-byte aligned rows for the mix kernel's float4 loads
            scores = torch.empty(B, Lc, ld, device=x.device, dtype=torch.float32)[:, :, :Vx]
            dec._score_head(x, ee, fe, eib, hv, scores, dec._vocab_presplit(B * Lc), pack=pack)
            ops.stamp("first pass: packed scores done")
            prob, temp, seed = self._ss_words
            return ops.sched_sample_mix(scores, pack, captions, caption_masks, V, K, Fn, wm["<start>"], wm["<pad>"], prob,
                                        temp, seed, self.counter, mode=self.ss["mode"], out=out)

        with torch.no_grad():
            # (a feature map goes through Encoder.conv1 here and again in the second pass, which writes the rows straight
            # into its memory buffer)
            enc_tok = dec._token_major(self.enc(enc_in)) if enc_in.dim() == 4 else enc_in
            dec._forward_device(captions, caption_masks, entities, facts, enc_tok, None, head=head)
        ops.stamp("first pass: mixed inputs done")

    def _need_sampling(self, what):
        if self.ss is None:
            raise IckError("%s needs a TrainStep built with scheduled_sampling=" % what)

    def set_sampling_prob(self, p):
        """A new replacement probability, from the next step on: only the device word is written, the captured graphs
        replay.  Whether there is scheduled sampling is fixed at construction."""
        self._need_sampling("set_sampling_prob")
        self.ss["prob"] = check_sampling_prob(p)
        self._ss_words[0].fill_(self.ss["prob"])

    def set_sampling_temperature(self, T):
        """A new temperature of the draw (mode "sample"), from the next step on: only the device word is written."""
        self._need_sampling("set_sampling_temperature")
        self.ss["temperature"] = check_sampling_temperature(T)
        self._ss_words[1].fill_(self.ss["temperature"])

    def sampled_inputs(self):
        """The last step's (captions_in, masks_in int64, replaced int32), each (B, L) on the device: what its second pass
        was fed and where the model's own prediction took gold's place.  No synchronisation; the tensors are the step's
        own buffers, written again by the next step of the same shape (clone() to keep them)."""
        self._need_sampling("sampled_inputs")
        if self._ss_out is None:
            raise IckError("sampled_inputs: no step has run yet")
        return self._ss_out

    def _part_a(self, *inputs):
        ops.stamp("A: start")
        args, kwargs = self._forward_and_loss(*inputs)
        backward_from_tape(*args, **kwargs)
        ops.stamp("A: end (after join)")

    def _lazy_active(self, enc_in):
        # (not with scheduled sampling: its first pass has to see this step's weights, so the update is never deferred)
        return bool(self.lazy and self.ss is None and self.use_graph and self.derived is not None and not self.split
                    and not self.deterministic
                    and enc_in is not None and enc_in.dim() == 4 and self._overlap("ICK_NO_FWD_OVERLAP"))

    def _conv1_bwd_kwargs(self, enc_in):
        """train_conv1: the backward pass also makes the image rows' gradient and hands it to ick_conv1_wgrad, which writes
        conv1's extent of the bucket (overwriting what the side tail zeroed)."""
        if not self.train_conv1:
            return {}

        def sink(d_img):
            ops.stamp("conv1 weight gradient starts")
            ops.conv1_wgrad(d_img, enc_in, self._c1_gw, self._c1_gb)
            ops.stamp("conv1 weight gradient done")

        return dict(want_image_grad=True, image_grad_sink=sink)

    def _ema_kwargs(self, e):
        if self.ema_decay is None:
            return {}
        return dict(ema=e, ema_decay_word=self._ema_word, ema_warmup=self.ema_warmup)

    def _decay_kwargs(self, word, mask):
        if word is None:
            return {}
        return dict(decay_word=word, decay_mask=mask, decoupled=self.decoupled_weight_decay)

    def _adam_conv1(self):
        """conv1's own update: the same division by the global token count, the element clamp, Adam with encoder_lr and
        the step counter the decoder's update of the same step reads (so it runs before the counter advances) -- then the
        pre-split copy of the new weight, into the buffer Encoder.conv1_presplit() hands out and captured graphs read in
        place.  A no-op on the parameters while the token count is zero, as the decoder's update."""
        ops.adam_update(self.enc_p, self.enc_g, self.enc_m, self.enc_v, 1, lr=self.encoder_lr, clip=self.clip, gscale=1.0,
                        beta1=self.betas[0], beta2=self.betas[1], eps=self.eps, step_tensor=self.counter,
                        gscale_den=self.flat_g[self._t + 1:], **self._ema_kwargs(self.enc_e),
                        **self._decay_kwargs(self._enc_wd_word, self._enc_wd_mask))
        self._conv1_resplit()

    def _conv1_resplit(self):
        ps = self.enc.conv1_presplit()            # (current by its key: no launch of its own)
        if ps is not None:
            w = self.enc.conv1.weight.detach()
            ops.presplit_weights([(w.view(w.shape[0], -1), ps)])

    def _deferred_update(self):
        """The previous step's clamp + Adam and step counter, at the head of this step's graph.  Both are no-ops while the
        token count in the gradient bucket's tail is zero: the very first step, and the step after a flush().  (A trained
        conv1's update has run on the main stream by now: forward_with_tape's pre_main.)"""
        self._adam(bump=(1, self._adam_ticket))       # (the counter moves inside the launch, by counter_add_if's rule)

    def flush(self):
        """Apply a pending (lazy_update) optimizer update now; afterwards the parameters, moments, step counter and weight
        images are what the eager order would have left."""
        if not self._pending:
            return
        if self._gb is not None:
            self._gb.replay()
        else:
            self._part_b()
        self.flat_g[self._t + 1:].zero_()      # the next step's leading update finds nothing to apply
        self._pending = False
        self.dec.invalidate_caches()
        if self.derived is not None:
            self.derived.mark_current()

    def _adam(self, bump=None):
        # divide by the global token count (device-resident), clamp, Adam with the device step counter -- and, with
        # self.derived, the re-laid-out copies of the updated weights in the same pass (the cover runs over the whole
        # bucket).  With the optimizer words the rate comes from them and the schedule, else from self.lr.
        den = self.flat_g[self._t + 1:]
        if self._words is not None and self.max_grad_norm is not None:
            # The norm is taken here, behind the all-reduce, so every rank gets the same value.  It runs over [0, n): the
            # alignment pads between the parameters lie inside, and they are zero -- _side_tail zeroes the whole bucket,
            # the backward pass writes through self.grads (views of the parameters' own extents), the all-reduce adds
            # zeros, and the optimizer kernels write back clamp(0 * scale) = 0.  The trailing [loss sum, token count] at
            # n, n + 1 are outside.
            ops.grad_sqnorm(self.flat_g[:self.n], self._words, self._norm_scratch, gscale=1.0, gscale_den=den)
        rate = dict(lr=self.lr) if self._words is None else dict(words=self._words, schedule=self._sched)
        # (the update runs over flat_p's n floats or the cover: flat_g's two trailing words stay outside without a view)
        ops.adam_update(self.flat_p, self.flat_g, self.flat_m, self.flat_v, 1, cover=self.derived,
                        clip=self.clip, gscale=1.0, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                        step_tensor=self.counter, gscale_den=den, **rate, **self._ema_kwargs(self.flat_e),
                        **self._decay_kwargs(self._wd_word, self._wd_mask), bump=bump)

    # ---- the same step in two halves (several ranks: the early half's all-reduce overlaps the late half) ----
    def _part_a1(self, *inputs):
        args, kwargs = self._forward_and_loss(*inputs)
        self._bp = BackwardPass(*args, **kwargs)
        self._bp.early(join=True)

    def _part_a2(self):
        self._bp.late()

    def _part_b(self):
        # divide by the global token count (device-resident), clamp, Adam with the device step counter
        ops.stamp("B: start")
        self._adam()
        if self.train_conv1:
            self._adam_conv1()
        # the counter counts APPLIED updates: a batch without a token leaves it, as it leaves the parameters and moments
        # (the deferred update's rule, _deferred_update) -- else Adam's bias correction, the schedule's position and
        # state_dict()'s step run ahead of the moments, and lazy_update and the eager order part ways
        ops.counter_add_if(self.counter, 1, self.flat_g[self._t + 1:])
        ops.stamp("B: end")

    @staticmethod
    def _warm_static(fn, inputs):
        """Static clones of the inputs and one run of fn on them off the capture, on a side stream (lazy kernel
        attributes); the warm-up steps touch the gradient bucket only."""
        static = [None if t is None else t.contiguous().clone() for t in inputs]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn(*static)
        torch.cuda.current_stream().wait_stream(side)
        return static

    @staticmethod
    def _after(first, fn):
        """fn, behind `first` on the same arguments when there is one (the warm-up run of a step with scheduled sampling:
        part A reads what the first pass wrote)."""
        return fn if first is None else lambda *s: (first(*s), fn(*s))

    def _capture(self, fn, inputs, first=None):
        static = self._warm_static(self._after(first, fn), inputs)
        g = torch.cuda.CUDAGraph()
        with ops.capture(g):
            fn(*static)
        return g, static

    def _capture_split(self, inputs, first=None):
        """Graphs A1 (forward, CE, early backward) and A2 (late backward) over one memory pool: A2 reads what A1 left
        in the tape."""
        static = self._warm_static(self._after(first, lambda *s: (self._part_a1(*s), self._part_a2())), inputs)
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with ops.capture(g1):
            self._part_a1(*static)
        with ops.capture(g2):   # own pool: the tape keeps A1's tensors alive
            self._part_a2()
        return g1, static, g2

    # ---- optimizer state in torch.optim.Adam's layout ------------------------------------------
    def _adam_order(self):
        """Trainable parameters in the order the reference hands them to torch.optim.Adam
        (geo-aware/train.py:85-88: filter(requires_grad, decoder.parameters()))."""
        mine = {id(p) for p in self.params}
        return [p for p in unique_parameters(self.dec) if id(p) in mine]

    def _slot(self, flat, p):
        """Decoder parameter p's extent of flat_m / flat_v / flat_e / flat_g (or a tensor laid out like them)."""
        return self._dec_bucket.slot(flat, p)

    def _step(self):
        return int(self.counter.item()) & 0xFFFFFFFF

    def state_dict(self):
        """The optimizer state as torch.optim.Adam.state_dict() would report it (exp_avg / exp_avg_sq / step per
        parameter, one param group), so checkpoints interchange with the reference's `decoder_optimizer`
        (geo-aware/utils.py:32-46) and with the fused=False path.  Tensors are copies."""
        self.flush()
        self._check_views()
        order = self._adam_order()
        return self._dec_bucket.adam_state(order, self._step(), self.lr, self.betas, self.eps,
                                           **self._decay_groups(order, self.weight_decay, self._decayed))

    def _decay_groups(self, order, wd, decayed):
        """adam_state's decay arguments: with decay on, one value per parameter of `order` (0 where it is not selected)."""
        if wd is None:
            return {}
        chosen = {id(p) for _, p in decayed}
        return dict(decay=[wd if id(p) in chosen else 0.0 for p in order], decoupled=self.decoupled_weight_decay)

    def _torch_optimizer(self, order, lr, wd, decayed):
        """torch.optim.Adam over `order`, or with decay on AdamW / Adam over one param group per parameter."""
        kw = dict(lr=lr, betas=tuple(self.betas), eps=self.eps)
        if wd is None:
            return torch.optim.Adam(order, **kw)
        groups = self._decay_groups(order, wd, decayed)["decay"]
        cls = torch.optim.AdamW if self.decoupled_weight_decay else torch.optim.Adam
        return cls([dict(params=[p], weight_decay=w) for p, w in zip(order, groups)], weight_decay=0.0, **kw)

    def load_state_dict(self, sd):
        """Restore Adam moments, step count (which also positions the dropout stream) and learning rate from a
        torch.optim.Adam-layout state dict: ours, the reference's, or the fused=False path's -- one param group or one per
        parameter.  Stored weight-decay values are ignored: decay is a hyper-parameter like grad_clip, and the
        constructor's (or set_weight_decay's) value holds."""
        self.flush()
        self._check_views()
        order = self._adam_order()
        steps, group = self._dec_bucket.load_adam_state(sd, order, "optimizer state",
                                                        "the decoder has %d trainable ones" % len(order))
        if len(steps) > 1:
            raise IckError("per-parameter Adam step counts differ (%s): not representable in the fused step" % steps)
        self.counter.fill_(steps.pop() if steps else 0)
        # (base_lr: the unfused path of train.py keeps the schedule's base rate there, "lr" then is the scheduled one)
        lr = float(group.get("base_lr", group["lr"]))
        betas, eps = tuple(group.get("betas", self.betas)), float(group.get("eps", self.eps))
        if self._words is None or betas != tuple(self.betas) or eps != self.eps:
            self._graphs.clear()      # betas / eps (and, without the optimizer words, lr) are baked into the captured graph
        self.lr, self.betas, self.eps = lr, betas, eps
        if self._words is not None:
            self._words[0:1].fill_(lr)
        self.dec.invalidate_caches()
        self.parameters_changed()

    def parameters_changed(self):
        """Tell the step that parameter VALUES were written from outside it (through .data, a raw kernel, a restored
        checkpoint): the re-laid-out copies the optimizer kernel maintains are rebuilt before the next step.  In-place
        torch operations on the parameters are noticed without this call (their version counters move)."""
        self.flush()
        if self.derived is not None:
            self.derived.stale = True

    def as_torch_optimizer(self):
        """A live torch.optim.Adam over the decoder's parameters carrying this step's state: what goes into the
        checkpoint under 'decoder_optimizer', exactly the kind of object the reference pickles there."""
        opt = self._torch_optimizer(self._adam_order(), self.lr, self.weight_decay, self._decayed)
        opt.load_state_dict(self.state_dict())
        return opt

    # ---- conv1's optimizer state (train_conv1), torch.optim.Adam's layout over [conv1.weight, conv1.bias] ----
    def _need_conv1(self, what):
        if not self.train_conv1:
            raise IckError("%s needs a TrainStep built with train_conv1=True" % what)
        self.flush()
        self._check_views()

    def encoder_state_dict(self):
        """conv1's Adam state as torch.optim.Adam.state_dict() reports it for the reference's `encoder_optimizer` over a
        feature-file encoder's trainable parameters [conv1.weight, conv1.bias] (geo-aware/train.py:93-100).  Both optimizers
        step together: the step count is the decoder's.  Tensors are copies; state_dict() is unchanged."""
        self._need_conv1("encoder_state_dict")
        return self._enc_bucket.adam_state(self.enc_params, self._step(), self.encoder_lr, self.betas, self.eps,
                                           **self._decay_groups(self.enc_params, self.encoder_weight_decay,
                                                                self._enc_decayed()))

    def load_encoder_state_dict(self, sd):
        """Restore conv1's moments and rate from a torch.optim.Adam-layout state dict over [conv1.weight, conv1.bias].  The
        step count is the decoder's (load_state_dict sets it): a state whose step differs from it is refused."""
        self._need_conv1("load_encoder_state_dict")
        steps, group = self._enc_bucket.load_adam_state(
            sd, self.enc_params, "encoder optimizer state", "the step trains conv1.weight and conv1.bias (a state that "
            "also covers trunk blocks belongs to fine_tune_encoder=True)")
        mine = self._step()
        if steps - {mine}:
            raise IckError("encoder optimizer state is at step %d, the decoder's at %d: both step together (load "
                           "the decoder's state first)" % (min(steps - {mine}), mine))
        self.encoder_lr = float(group["lr"])
        self._graphs.clear()              # the rate is baked into the captured optimizer launches

    def as_torch_encoder_optimizer(self):
        """A live torch.optim.Adam over [conv1.weight, conv1.bias] carrying conv1's state: what goes into the checkpoint
        under 'encoder_optimizer', the kind of object the reference pickles there."""
        sd = self.encoder_state_dict()
        opt = self._torch_optimizer(self.enc_params, self.encoder_lr, self.encoder_weight_decay, self._enc_decayed())
        opt.load_state_dict(sd)
        return opt

    # ---- weight decay (weight_decay= / encoder_weight_decay=) -----------------------
    def _enc_decayed(self):
        return [("conv1.weight", self.enc_params[0])] if self.encoder_weight_decay is not None else []

    def decayed_parameter_names(self):
        """The names of the parameters weight decay covers: the decoder's (named_parameters() names, bucket order), then
        "encoder.conv1.weight" with encoder_weight_decay.  Empty without decay."""
        return [n for n, _ in self._decayed] + ["encoder." + n for n, _ in self._enc_decayed()]

    def _set_decay(self, wd, what, attr, word):
        if (wd is None) != (word is None):
            raise IckError("weight decay cannot be switched %s after construction: build the TrainStep with%s %s="
                           % (("off", "out", what) if wd is None else ("on", "", what)))
        if wd is None:
            return
        wd = check_weight_decay(wd)
        self.flush()
        setattr(self, attr, wd)
        word.fill_(wd)

    def set_weight_decay(self, wd):
        """A new weight-decay value for the decoder's selected parameters, applied from the next update on: only the
        device word is written, the captured graphs replay.  A pending (lazy_update) update is applied first, under the
        old value.  Whether there is decay is fixed at construction: None here, or a value for a step built without it,
        is refused."""
        self._set_decay(wd, "weight_decay", "weight_decay", self._wd_word)

    def set_encoder_weight_decay(self, wd):
        """set_weight_decay for conv1.weight's decay (encoder_weight_decay=)."""
        self._set_decay(wd, "encoder_weight_decay", "encoder_weight_decay", self._enc_wd_word)

    # ---- the moving average of the parameters (ema_decay=) -------------------------
    def _need_ema(self, what):
        if self.ema_decay is None:
            raise IckError("%s needs a TrainStep built with ema_decay=" % what)
        self.flush()
        self._check_views()

    def set_ema_decay(self, d):
        """A new decay of the moving average, applied from the next update on: only the device word is written, the
        captured graphs replay.  A pending (lazy_update) update is applied first, under the old decay.  Whether there is
        an average at all is fixed at construction: None here, or a value for a step built without one, is refused."""
        if (d is None) != (self.ema_decay is None):
            raise IckError("the moving average cannot be switched %s after construction: build the TrainStep with%s "
                           "ema_decay=" % (("off", "out") if d is None else ("on", "")))
        if d is None:
            return
        d = check_ema_decay(d)
        self.flush()
        self.ema_decay = d
        self._ema_word.fill_(d)

    def _ema_params(self):
        """(parameter, its slot of the average) in ema_state_dict()'s order: _adam_order(), then conv1's two."""
        orders = [self._adam_order()] + ([self.enc_params] if self.train_conv1 else [])
        return [(p, b.slot(b.e, p)) for b, order in zip(self._buckets, orders) for p in order]

    def ema_state_dict(self):
        """The moving average: {"decay", "warmup", "params": one tensor per parameter in _adam_order()'s order[,
        "encoder_params": conv1.weight's and conv1.bias's with train_conv1]}.  Tensors are copies; a pending update is
        applied first.  Refused inside ema_weights(), where the two buckets are exchanged and flat_e holds the training
        weights."""
        self._need_ema("ema_state_dict")
        if self._ema_swapped:
            raise IckError("ema_state_dict inside ema_weights(): the buckets are exchanged there; leave the context first")
        n = len(self._adam_order())
        avg = [e.clone() for _, e in self._ema_params()]
        sd = {"decay": self.ema_decay, "warmup": self.ema_warmup, "params": avg[:n]}
        if self.train_conv1:
            sd["encoder_params"] = avg[n:]
        return sd

    def load_ema_state_dict(self, sd):
        """Restore the moving average (and its decay and warmup flag) from ema_state_dict()'s layout."""
        self._need_ema("load_ema_state_dict")
        if self._ema_swapped:
            raise IckError("load_ema_state_dict inside ema_weights(): leave the context first")
        mine = self._ema_params()
        theirs = list(sd["params"]) + list(sd.get("encoder_params", ()))
        if len(theirs) != len(mine) or len(sd["params"]) != len(self._adam_order()):
            raise IckError("the moving average holds %d (+ %d encoder) tensors, the step trains %d (+ %d)" %
                           (len(sd["params"]), len(sd.get("encoder_params", ())), len(self._adam_order()),
                            len(mine) - len(self._adam_order())))
        for i, ((p, _), t) in enumerate(zip(mine, theirs)):
            if tuple(t.shape) != tuple(p.shape):
                raise IckError("moving average %d has shape %s, the parameter has %s" % (i, tuple(t.shape), tuple(p.shape)))
        decay = check_ema_decay(sd.get("decay", self.ema_decay))
        if decay is None:
            raise IckError("the moving average's state carries no decay")
        with torch.no_grad():
            for (_, e), t in zip(mine, theirs):
                e.copy_(t)
        self.ema_decay = decay
        self._ema_word.fill_(decay)
        if bool(sd.get("warmup", self.ema_warmup)) != self.ema_warmup:
            self.ema_warmup = not self.ema_warmup
            self._graphs.clear()          # the flag is an argument of the captured optimizer launches

    def _ema_exchange(self):
        for b in self._buckets:
            b.exchange_average()
        self.dec.invalidate_caches()
        if self.enc is not None:
            self.enc.invalidate_caches()
        self.parameters_changed()

    @contextlib.contextmanager
    def ema_weights(self):
        """Inside the context the parameters hold the averaged weights: forward, predict*, score_captions, validate see
        them through the parameters' own views of the bucket.  A pending update is applied first; the contents of flat_p
        and flat_e (and of conv1's pair) are exchanged, every cache of re-laid-out weights is invalidated, and on the way
        out -- also when the body raises -- they are exchanged back and invalidated again, so the next step trains the
        very bits it left.  A training step inside the context is refused."""
        self._need_ema("ema_weights")
        if self._ema_swapped:
            raise IckError("ema_weights() is already in effect")
        self._ema_exchange()
        self._ema_swapped = True
        try:
            yield self
        finally:
            self._ema_swapped = False
            self._ema_exchange()

    def input_buffers(self):
        """The static input tensors of the most recently captured graphs, in __call__'s argument order
        (captions, encoder_out-or-features, caption_masks, caption_lengths, entities[, facts]).  A loader that writes
        the next batch straight into them (pinned host-to-device copies) and calls the step with these very tensors
        skips the per-step device-to-device copy of the inputs."""
        st = getattr(self, "_last_static", None)
        if st is None:
            raise IckError("no captured graph yet: run one step first")
        captions, masks, entities, facts, enc_in, _, lengths = st[:7]
        return (captions, enc_in, masks, lengths, entities) + ((facts,) if facts is not None else ())

    def set_lr(self, lr):
        self.flush()                  # a pending update was computed under the old rate
        self.lr = float(lr)
        if self._words is not None:
            self._words[0:1].fill_(self.lr)       # the base rate word: the captured graphs replay, the schedule multiplies it
        else:
            self._graphs.clear()      # baked into the captured optimizer graph

    def set_encoder_lr(self, lr):
        """A new rate for conv1's Adam (train_conv1), applied from the next update on.  As set_lr without the optimizer
        words: a pending update is applied first, under the old rate, and the rate is baked into the captured optimizer
        launches, so the next step captures again."""
        if not self.train_conv1:
            raise IckError("set_encoder_lr needs a TrainStep built with train_conv1=True")
        self.flush()
        self.encoder_lr = float(lr)
        self._graphs.clear()

    def _check_views(self):
        """The decoder's parameters must still be views of the flat bucket: decoder.to() / .cuda() /
        load_pretrained_embeddings() re-allocate them and the step would then update memory the module no longer
        reads (silently).  Two pointer compares per bucket and call (ParamBucket.resident)."""
        if not self._dec_bucket.resident():
            raise IckError("the decoder's parameters no longer live in TrainStep's bucket (module moved or a "
                           "Parameter was replaced after TrainStep was built): build a new TrainStep")
        if self.train_conv1:
            c1 = self.enc.conv1
            if c1.weight is not self.enc_params[0] or c1.bias is not self.enc_params[1] or not self._enc_bucket.resident():
                raise IckError("Encoder.conv1 no longer lives in TrainStep's storage (encoder moved or a Parameter was "
                               "replaced after TrainStep was built): build a new TrainStep")

    def _row_inputs(self, caption_weights, image_index, R, n_img, dev):
        """Validated device copies of the optional per-caption inputs (None stays None).  The image index is checked
        against the encoder rows (an index outside [0, n_img) would make the gather read outside encoder_out); a call
        that passes the very tensor object validated last time, unmodified (same version counter), skips the check."""
        w = gm = None
        if caption_weights is not None:
            if tuple(caption_weights.shape) != (R,):
                raise IckError("caption_weights must have shape (%d,), got %s" % (R, tuple(caption_weights.shape)))
            w = caption_weights.to(device=dev, dtype=torch.float32, non_blocking=True).contiguous()
        if image_index is not None:
            if tuple(image_index.shape) != (R,):
                raise IckError("image_index must have shape (%d,), got %s" % (R, tuple(image_index.shape)))
            ok = getattr(self, "_gmap_checked", None)
            if ok is None or ok[0]() is not image_index or ok[1:] != (image_index._version, n_img):
                lo, hi = (int(v) for v in torch.aminmax(image_index.reshape(-1)))
                if lo < 0 or hi >= n_img:
                    raise IckError("image_index values must lie in [0, %d), got [%d, %d]" % (n_img, lo, hi))
                self._gmap_checked = (weakref.ref(image_index), image_index._version, n_img)
            gm = image_index.to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
        return w, gm

    def __call__(self, captions, encoder_out, caption_masks, caption_lengths, entities, facts=None,
                 caption_weights=None, image_index=None):
        """One training step; returns the token-mean loss (device scalar; at world size 1 the step's own one-element buffer,
        which the next step writes again: .item() or .clone() it to keep a value; 0 for a batch without a token).
        caption_weights (R,) fp32: per-caption
        weights of the loss (the weighted packed cross entropy; SelfCriticalStep's advantages), still divided by the
        token count.  image_index (R,) int: caption row r reads row image_index[r] of a token-major encoder_out with
        fewer rows (several captions of one image share its encoder output); not with a 4-D feature map.  Both are
        inputs of the captured graphs (new values replay, never re-capture); their presence is part of the graph key."""
        dec = self.dec
        if self._ema_swapped:
            raise IckError("a training step inside ema_weights(): the parameters hold the averaged weights there; leave "
                           "the context first")
        self._check_views()
        encoder_out, entities, facts = dec._prepare_inputs(encoder_out, entities, facts)
        dev = encoder_out.device
        if image_index is not None and encoder_out.dim() == 4:
            raise IckError("image_index needs a token-major encoder_out (B, d, P), not a 4-D feature map")
        if self.ss is not None and (caption_weights is not None or image_index is not None):
            raise IckError("scheduled_sampling: a step built with it takes no caption_weights and no image_index (its inputs "
                           "are mixed per caption row; SelfCriticalStep trains on sampled captions already)")
        if self.train_conv1 and (encoder_out.dim() != 4 or image_index is not None):
            raise IckError("train_conv1=True needs the 4-D feature map as encoder_out and no image_index: from a token-major "
                           "encoder_out the step cannot reach Encoder.conv1")
        weights, gmap = self._row_inputs(caption_weights, image_index, captions.shape[0], encoder_out.shape[0], dev)
        # No length sort and no host round trip here: the loss is a sum over tokens, so the batch order does
        # not matter, and the lengths are only read on the device (packed cross entropy).  The reference sorts
        # because pack_padded_sequence wants it (geo-aware/models.py:330-336); forward() keeps doing so.
        captions = captions.to(dev, non_blocking=True)
        caption_masks = caption_masks.to(dev, non_blocking=True)
        if encoder_out.dim() == 4:
            if self.enc is None:
                raise IckError("TrainStep got a (B, C, H, W) feature map but was built without encoder=")
            enc_in = encoder_out
            self.enc.conv1_presplit()      # refreshed in place, OUTSIDE the captured graphs, if conv1's weight changed
        else:
            enc_in = dec._token_major(encoder_out)
        lengths = caption_lengths.to(dev, non_blocking=True)
        inputs = [captions, caption_masks, entities, facts, enc_in, gmap, lengths]
        if weights is not None:
            inputs.append(weights)
        if ops.is_deterministic() != self.deterministic:
            raise IckError("the library's deterministic mode is %s but this TrainStep was built with %s: captured graphs "
                           "keep the mode they were captured in (call ops.set_deterministic before building the step)"
                           % (ops.is_deterministic(), self.deterministic))
        # the large GEMM tiles' product mode is baked into a capture as well
        key = tuple(None if t is None else tuple(t.shape) for t in inputs) + (ops.gemm_split_mode(),)
        if self.label_smoothing != 0.0:
            key += ("label_smoothing",)     # another loss kernel; the value itself is read from the device word
        if self.ss is not None:
            key += ("scheduled_sampling", self.ss["mode"])      # the first pass; prob / temperature / seed are device words
            B, Lc = captions.shape
            if (B, Lc) not in self._ss_bufs:    # the mix kernel's outputs: the step's own, outside every graph's pool
                if len(self._ss_bufs) >= 4:
                    self._ss_bufs.clear()
                    self._graphs.clear()
                self._ss_bufs[(B, Lc)] = (torch.zeros(B, Lc, device=dev, dtype=torch.int64),
                                          torch.zeros(B, Lc, device=dev, dtype=torch.int64),
                                          torch.zeros(B, Lc, device=dev, dtype=torch.int32))
            self._ss_out = self._ss_bufs[(B, Lc)]
        if not self._derived_tried:
            self._derived_tried = True
            if os.environ.get("ICK_ADAM_DERIVE", "1") != "0":
                self.derived = DerivedWeights.build(self)
                self._graphs.clear()
        if self.derived is not None:
            self.derived.ensure_current(check=key not in self._graphs)
        if self.use_graph and key not in self._graphs:
            self.flush()                  # the warm-up runs below must not find gradients waiting to be applied
            if len(self._graphs) >= 4:
                self._graphs.clear()
            # the eager warm-up run of part B is a real optimizer step: snapshot and rewind its state
            state = [self.counter] + [t for b in self._buckets for t in b.tensors()]
            snap = [t.clone() for t in state]
            try:
                first = self._first_pass if self.ss is not None and not self._ss_inline else None
                if self.split:
                    ga, static, ga2 = self._capture_split(inputs, first)
                else:
                    ga, static = self._capture(self._part_a, inputs, first)
                    ga2 = None
                if first is not None:         # the first pass over the same static inputs, a graph of its own
                    g0 = torch.cuda.CUDAGraph()
                    with ops.capture(g0):
                        first(*static)
                    if not self._graphs:
                        self._ss_first.clear()
                    self._ss_first[key] = g0
                gb, _ = self._capture(self._part_b, [])
                self._gb = gb
                self._graphs[key] = (ga, static, gb, ga2)
                self._last_static = static
            except RuntimeError as e:   # capture refused (driver / collective library state): run eagerly
                import warnings
                warnings.warn("ick_amd TrainStep: hipGraph capture failed (%s); continuing without graphs" % e)
                torch.cuda.synchronize()
                self.use_graph = False
            for t, sv in zip(state, snap):
                t.copy_(sv)
            if self.derived is not None:      # the warm-up's optimizer step wrote the images of weights that were just rewound
                self.derived.stale = True
                self.derived.ensure_current()
            if self.train_conv1:              # ... and the pre-split copy of conv1's
                self._conv1_resplit()
            self.flat_g[self._t + 1:].zero_()  # (lazy_update: the warm-up's gradients are not a pending update)
        # how the parts of this step run: replays of the captured graphs, or the Python functions on the inputs
        if self.use_graph:
            ga, static, gb, ga2 = self._graphs[key]
            if self._lazy_active(enc_in) and not self._pending:
                # nothing is waiting to be applied (first step, or the update was flushed / applied eagerly): the leading
                # update of the graph must find a zero token count
                self.flat_g[self._t + 1:].zero_()
            from .decoder import copy_inputs
            copy_inputs(static, inputs)
            part_a, part_a2, part_b = ga.replay, None if ga2 is None else ga2.replay, gb.replay
            first = self._ss_first[key].replay if self.ss is not None and not self._ss_inline else None
        else:
            part_a = functools.partial(self._part_a1 if self.split else self._part_a, *inputs)
            part_a2, part_b = self._part_a2 if self.split else None, self._part_b
            first = functools.partial(self._first_pass, *inputs) if self.ss is not None and not self._ss_inline else None
        if first is not None:
            first()
        part_a()
        if part_a2 is None:
            dp.allreduce_bucket(self.flat_g, self.pg)
        else:
            # [early gradients] travel while part A2 computes [late gradients | loss_sum, count]
            w1 = dp.allreduce_bucket(self.flat_g[:self.n_early], self.pg, async_op=True)
            part_a2()
            w2 = dp.allreduce_bucket(self.flat_g[self.n_early:], self.pg, async_op=True)
            for w in (w1, w2):
                if w is not None:
                    w.wait()
        if self._lazy_active(enc_in):     # (captured steps only)
            self._pending = True          # applied at the head of the next step's graph (or by flush())
        else:
            part_b()
        self.step_count += 1
        dec.invalidate_caches()   # the update went around torch's version counters
        if self.derived is not None:
            self.derived.mark_current()
        # token-mean loss of the global batch, still on the device: at world size 1 the loss launch has written it (0 for a
        # batch without a token); several ranks divide the all-reduced sums
        if dp.world_size(self.pg) == 1:
            return self._mean
        return self.flat_g[self._t:self._t + 1] / self.flat_g[self._t + 1:]
