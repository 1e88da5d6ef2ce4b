"""Float64 cross-attention weights of the decoder stack, teacher-forced over the tokens every decode row was fed.

The stack is restated on the oracle's pieces (R.caption_embed, R.build_memory through decode_ref.Fp64Decode, the layer
weights of the state dict); the multi-head attention below is written for this test so that it can hand back the
cross-attention probabilities softmax(q . k / sqrt(dh)) of every layer and head.  With the causal self-attention,
position i of one teacher-forced pass is decode step i.
"""
import math

import torch
import torch.nn.functional as F

from oracle import restatement as R
from decode_ref import feed_masks, float64_default


def attention(xq, xkv, in_w, in_b, out_w, out_b, H, causal):
    """-> (output (B, T, d), probabilities (B, H, T, S))."""
    B, T, d = xq.shape
    S, dh = xkv.shape[1], d // H
    q = (xq @ in_w[:d].t() + in_b[:d]).view(B, T, H, dh).permute(0, 2, 1, 3)
    k = (xkv @ in_w[d:2 * d].t() + in_b[d:2 * d]).view(B, S, H, dh).permute(0, 2, 3, 1)
    v = (xkv @ in_w[2 * d:].t() + in_b[2 * d:]).view(B, S, H, dh).permute(0, 2, 1, 3)
    logits = torch.matmul(q, k) / math.sqrt(dh)
    if causal:
        logits = logits.masked_fill(torch.ones(T, S, dtype=torch.bool).triu(1), float("-inf"))
    p = torch.softmax(logits, dim=-1)
    ctx = torch.matmul(p, v).permute(0, 2, 1, 3).reshape(B, T, d)
    return ctx @ out_w.t() + out_b, p


def _norm(x, P, name):
    return F.layer_norm(x, (x.shape[-1],), P[name + ".weight"], P[name + ".bias"], R.LN_EPS)


def cross_weights(fp64, fed, img):
    """fp64: decode_ref.Fp64Decode of the batch; fed (R, n) int64 tokens row r was fed at positions 0..n-1; img (R,)
    image of each row.  Returns float64 (R, n, layers, H, S): the cross-attention weights of every step."""
    cfg, P, K = fp64.cfg, fp64.P, fp64.K
    fed = torch.as_tensor(fed, dtype=torch.long).cpu()
    img = torch.as_tensor(img, dtype=torch.long).cpu()
    n = fed.shape[1]
    H = cfg.num_heads
    with float64_default(), torch.no_grad():
        ee = fp64.ee[img]
        fe = fp64.fe[img] if fp64.fe is not None else None
        x = R.caption_embed(cfg, P, fed, feed_masks(cfg, fed, K), ee, fe) * math.sqrt(cfg.emb_dim) + \
            R.pe_table(n, cfg.emb_dim).unsqueeze(0)
        mem = fp64.mem[img]
        out = []
        for li in range(cfg.num_layers):
            pre = "transformer_decoder.layers.%d." % li
            a, _ = attention(x, x, P[pre + "self_attn.in_proj_weight"], P[pre + "self_attn.in_proj_bias"],
                             P[pre + "self_attn.out_proj.weight"], P[pre + "self_attn.out_proj.bias"], H, True)
            x = _norm(x + a, P, pre + "norm1")
            c, p = attention(x, mem, P[pre + "multihead_attn.in_proj_weight"], P[pre + "multihead_attn.in_proj_bias"],
                             P[pre + "multihead_attn.out_proj.weight"], P[pre + "multihead_attn.out_proj.bias"], H, False)
            out.append(p)                                                   # (R, H, n, S)
            x = _norm(x + c, P, pre + "norm2")
            f = F.relu(x @ P[pre + "linear1.weight"].t() + P[pre + "linear1.bias"]) @ P[pre + "linear2.weight"].t() + \
                P[pre + "linear2.bias"]
            x = _norm(x + f, P, pre + "norm3")
        return torch.stack(out, dim=1).permute(0, 3, 1, 2, 4).numpy()      # (R, n, layers, H, S)


def prefix_feeds(seqs, start, end):
    """Feeds of rows that were fed their own output: <start> + the row's tokens before its <end> (or all of them).
    seqs: (R, max_len) int64.  Returns (fed (R, max_len), live steps per row)."""
    seqs = torch.as_tensor(seqs).cpu()
    Rn, T = seqs.shape
    fed = torch.full((Rn, T), start, dtype=torch.long)
    fed[:, 1:] = seqs[:, :-1]
    live = []
    for r in range(Rn):
        t = seqs[r].tolist()
        live.append(t.index(end) + 1 if end in t else T)
    return fed, live
