"""The packed score head of the fused training step, the parts that need no GPU:
  * the row list ick_head_rowmap builds (csrc/score_head.hip), restated in Python thread by thread, against the
    bookkeeping of pack_padded_sequence as the reference's loss uses it (geo-aware/train.py:275-281);
  * the premise that makes skipping the padded rows exact: the gradient of the packed loss with respect to the decoder's
    output is exactly zero at and beyond every sample's decode length -- the decoder's self-attention is causal and has
    no key-padding mask (geo-aware/models.py:315-361), so no valid position reads a padded one.
"""
import pytest
import torch
from torch.nn.utils.rnn import pack_padded_sequence

import ick_amd.synth as synth
from oracle import restatement as R


def rowmap_ref(lengths, L, threads=256):
    """head_rowmap_kernel, thread by thread: every thread owns `per` consecutive samples, thread 0 scans the partial
    sums, every thread then lists its samples' valid rows.  -> (decode_len, rowstart (B + 1), rowmap (B * L))."""
    B = len(lengths)
    per = (B + threads - 1) // threads
    valid = lambda n: min(L - 1, max(0, n - 1))     # noqa: E731
    decode_len = [n - 1 for n in lengths]
    part = []
    for tid in range(threads):
        b0 = min(B, tid * per)
        part.append(sum(valid(lengths[b]) for b in range(b0, min(B, b0 + per))))
    run, start = 0, []
    for v in part:
        start.append(run)
        run += v
    total = run
    rowstart, rowmap = [0] * (B + 1), [0] * (B * L)
    rowstart[B] = total
    for tid in range(threads):
        b0 = min(B, tid * per)
        run = start[tid]
        for b in range(b0, min(B, b0 + per)):
            n = valid(lengths[b])
            rowstart[b] = run
            for t in range(n):
                rowmap[run + t] = b * L + t
            run += n
    return decode_len, rowstart, rowmap, total


CASES = {
    "all_full": (8, [8] * 6),
    "all_two": (8, [2] * 6),
    "mixed": (8, [8, 5, 7, 2, 6, 3]),
    "one_of_length_one": (8, [4, 1, 8, 3]),
    "more_samples_than_threads": (5, [(i * 7) % 5 + 1 for i in range(600)]),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rowmap_restatement_vs_pack_padded_bookkeeping(name):
    L, lengths = CASES[name]
    B = len(lengths)
    decode_len, rowstart, rowmap, total = rowmap_ref(lengths, L)
    dl = torch.tensor([n - 1 for n in lengths])
    assert decode_len == dl.tolist() and total == int(dl.clamp(0, L - 1).sum())
    # sample-major, position ascending: exactly the positions t < decode_len[b]
    expect = [b * L + t for b in range(B) for t in range(min(L - 1, max(0, lengths[b] - 1)))]
    assert rowmap[:total] == expect and all(v == 0 for v in rowmap[total:])
    assert rowstart[:B] == [sum(dl.clamp(0, L - 1)[:b].tolist()) for b in range(B)]
    # pack_padded_sequence keeps the same rows (time-major, and it refuses samples without a single row)
    keep = dl > 0
    if keep.any():
        idx = torch.arange(B * L).view(B, L)
        packed = pack_padded_sequence(idx[keep], dl[keep], batch_first=True, enforce_sorted=False).data
        assert sorted(packed.tolist()) == sorted(expect)
    else:
        assert total == 0


def test_loss_gradient_is_exactly_zero_on_padded_decoder_rows():
    """oracle/stock.py (torch.nn's Transformer stacks), geo variant, B = 6, L = 8: dLoss/dh of the packed cross entropy is
    non-zero on exactly sum(decode_len) rows and exactly 0.0 on every row at or beyond a sample's decode length."""
    from oracle.stock import StockDecoder
    variant, B, L, K, V, seed = "geo", 6, 8, 5, 60, 3
    P = synth.make_params(variant, V, seed)
    wm = synth.make_word_map(V)
    cfg = R.config_from_word_map(variant, wm)
    batch = synth.make_batch(variant, B, L, K, V, 0, seed)
    enc_out = synth.make_enc_out(B, seed)
    m = StockDecoder(variant, wm).load_reference_params(P).eval()
    kept = {}

    def hook(mod, inp, out):
        out.retain_grad()
        kept["h"] = out             # (L, B, d), samples in the length-sorted order of forward()

    m.transformer_decoder.register_forward_hook(hook)
    scores, caps, dl = m(batch["captions"], enc_out, batch["caption_masks"], batch["caption_lengths"], batch["entities"])
    loss = R.packed_ce_loss(cfg, scores, caps, dl)
    loss.backward()
    g = kept["h"].grad.permute(1, 0, 2)         # (B, L, d)
    assert len(set(dl)) > 1 and min(dl) < L - 1, "the case must contain padded rows"
    nonzero_rows = 0
    for b in range(B):
        for t in range(L):
            row = g[b, t]
            if t < dl[b]:
                assert row.abs().max().item() > 0.0, (b, t)
                nonzero_rows += 1
            else:
                assert torch.equal(row, torch.zeros_like(row)), (b, t, row.abs().max().item())
    assert nonzero_rows == sum(dl)
