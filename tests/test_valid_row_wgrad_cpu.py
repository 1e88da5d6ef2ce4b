"""The premise of the valid-row weight gradients of the decoder layers, pinned on the oracle's own
arithmetic and without a GPU: with the packed cross entropy of the reference (geo-aware/train.py:275-281) the gradient at
the output of EVERY Linear and LayerNorm of the decoder stack (geo-aware/models.py:241-244, 315-361) is exactly 0.0 at
every caption position t >= caption_length[b] - 1.  The loss reads the positions below that only, the self-attention is
causal and has no key-padding mask, cross-attention and everything else is row-wise, and LayerNorm' of a zero row is zero
-- so every weight gradient dW += dy^T x of a decoder layer adds rows of exact zeros for the padded positions, and
leaving them out of the reduction changes nothing but the order of the sum.

torch.nn.MultiheadAttention applies its projections through torch.nn.functional.linear, not through Linear modules, so
the hooks are put on the outputs of F.linear and F.layer_norm while transformer_decoder runs: that covers linear1 /
linear2, the three norms, both out-projections, the packed self-attention in-projection and the cross-attention query
projection of every layer.  (The cross-attention K/V projection has memory rows, not caption rows: not part of this.)"""
import pytest
import torch
import torch.nn.functional as F

import ick_amd.synth as synth
from oracle import restatement as R
from oracle.stock import StockDecoder

CASES = [("geo", 4, 6, 4, 0, [6, 1, 2, 4]), ("knowledge", 3, 5, 4, 5, [5, 1, 2]), ("news", 4, 5, 5, 6, [2, 5, 1, 3])]


@pytest.mark.parametrize("dropout", [False, True], ids=["dropout_off", "dropout_on"])
@pytest.mark.parametrize("variant,B,L,K,Fn,lengths", CASES, ids=[c[0] for c in CASES])
def test_gradient_is_exactly_zero_at_padded_rows_of_every_decoder_layer_output(monkeypatch, variant, B, L, K, Fn,
                                                                                lengths, dropout):
    V, seed = 60, 7
    assert 1 in lengths and 2 in lengths and L in lengths
    P = synth.make_params(variant, V, seed)
    wm = synth.make_word_map(V)
    cfg = R.config_from_word_map(variant, wm)
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    batch["caption_lengths"] = torch.tensor(lengths, dtype=torch.int64).view(B, 1)
    enc_out = synth.make_enc_out(B, seed)
    m = StockDecoder(variant, wm).load_reference_params(P)
    m = m.train() if dropout else m.eval()
    torch.manual_seed(seed)

    kept, inside = [], [False]
    real_linear, real_layer_norm = F.linear, F.layer_norm

    def keep(name, out):
        # caption-row tensors are (L, B, *) inside the stack -- the attention out-projections run on the (L * B, d) view of
        # it, position-major -- and the cross K/V projection's rows are memory rows
        rows = (out.dim() == 3 and out.shape[:2] == (L, B)) or (out.dim() == 2 and out.shape[0] == L * B)
        if inside[0] and rows and out.requires_grad:
            out.retain_grad()
            kept.append((name, out))
        return out

    monkeypatch.setattr(F, "linear", lambda x, w, b=None: keep("linear %s" % (tuple(w.shape),), real_linear(x, w, b)))
    monkeypatch.setattr(F, "layer_norm", lambda x, *a, **k: keep("layer_norm", real_layer_norm(x, *a, **k)))
    m.transformer_decoder.register_forward_pre_hook(lambda mod, inp: inside.__setitem__(0, True))
    m.transformer_decoder.register_forward_hook(lambda mod, inp, out: inside.__setitem__(0, False))

    args = [batch["captions"], enc_out, batch["caption_masks"], batch["caption_lengths"], batch["entities"]]
    if variant != "geo":
        args.append(batch["facts"])
    scores, caps, dl = m(*args)
    S = enc_out.shape[1] + K + Fn
    assert S != L, "memory rows must be told from caption rows by their count"
    loss = R.packed_ce_loss(cfg, scores, caps, dl)
    loss.backward()

    layers = len(m.transformer_decoder.layers)
    d = kept[0][1].shape[-1] // 3
    # per layer: self in-proj (3d), self out-proj, norm1, cross q in-proj, cross out-proj, norm2, linear1, linear2, norm3
    assert len(kept) >= 9 * layers, [n for n, _ in kept]
    names = [n for n, _ in kept]
    assert names.count("layer_norm") >= 3 * layers
    assert sum(1 for _, t in kept if t.shape[-1] == 3 * d) == layers         # packed self-attention q | k | v
    assert sorted(dl, reverse=True) == dl and 0 in dl and 1 in dl and L - 1 in dl
    nonzero = 0
    for name, t in kept:
        assert t.grad is not None, name
        g = t.grad.view(L, B, -1)
        for b in range(B):
            pad = g[dl[b]:, b]
            assert torch.equal(pad, torch.zeros_like(pad)), (name, b, dl[b], pad.abs().max().item())
            nonzero += int(g[:dl[b], b].abs().sum().item() > 0.0)
    assert nonzero > 0, "the valid rows must carry a gradient"
