#!/usr/bin/env python3
"""Caption scoring at cfg2 and cfg4: DecoderTransformer.score_captions against the route to the same numbers without it
-- forward() followed by torch log_softmax + gather + topk(5) over the (B, L, V+K+F) matrix -- and the row kernel
(ick_row_logprob_rank) alone against its one-read floor.  Both routes run in one process on one GPU, in alternating
blocks between HIP events; the figures are medians over the blocks.
    python tools/score_captions_bench.py [--out profiles/score_captions_bench.json] [--blocks 9] [--calls 20]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes/s, MI355X


def median(xs):
    return sorted(xs)[len(xs) // 2]


def timed_block(fn, calls):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls       # ms per call


def run(name, blocks, calls):
    import torch
    import ick_amd
    import ick_amd.synth as synth
    from ick_amd import ops
    c = synth.CONFIGS[name]
    variant, B, L, K, V, Fn = c["variant"], c["B"], c["L"], c["K"], c["V"], c["F"]
    P = synth.make_params(variant, V, 1)
    dec = ick_amd.load_models(variant).DecoderTransformer(word_map=synth.make_word_map(V), emb_dim=300, decoder_dim=512,
                                                          encoder_dim=512, num_heads=10, num_layers=3)
    dec.load_state_dict(P, strict=False)
    dec = dec.cuda().eval()
    batch = synth.make_batch(variant, B, L, K, V, Fn, 1)
    caps, masks, lens = (batch[k].cuda() for k in ("captions", "caption_masks", "caption_lengths"))
    ents = batch["entities"].cuda()
    facts = batch["facts"].cuda() if "facts" in batch else None
    enc = synth.make_enc_out(B, 1).cuda()
    pad = dec.word_map["<pad>"]
    Vx = V + K + Fn
    pos = torch.arange(L - 1, device="cuda").view(1, -1)

    def scored():
        return dec.score_captions(caps, enc, masks, lens, ents, facts, top_k=5)

    def dense():
        with torch.no_grad():
            scores, caps_sorted, dl = dec(caps, enc, masks, lens, ents, *([facts] if facts is not None else []))
            s = scores[:, :-1]
            tgt = caps_sorted[:, 1:]
            keep = (pos < torch.tensor(dl, device="cuda").view(-1, 1)) & (tgt != pad)
            tlp = torch.log_softmax(s, -1).gather(2, tgt.unsqueeze(2)).squeeze(2)
            top5 = s.topk(5, -1).indices
            hit5 = (top5 == tgt.unsqueeze(2)).any(-1) & keep
            hit1 = (top5[..., 0] == tgt) & keep
            return -(tlp * keep).sum(), keep.sum(), hit1.sum(), hit5.sum()

    a, b = scored(), dense()          # warm-up: captures both graphs; and the two routes agree
    torch.cuda.synchronize()
    agree = dict(loss_sum=[a.loss_sum.item(), b[0].item()], count=[a.count.item(), b[1].item()],
                 top1_hits=[a.top1_hits.item(), b[2].item()], top5_hits=[a.topk_hits.item(), b[3].item()])
    for _ in range(3):
        scored(); dense()
    ta, tb = [], []
    for _ in range(blocks):           # alternating blocks
        ta.append(timed_block(scored, calls))
        tb.append(timed_block(dense, calls))

    # the row kernel alone, over packed rows of this shape (the training step's padded row stride)
    ld = (Vx + 3) // 4 * 4
    scores = (torch.randn(B, L, ld, device="cuda") * 2)[:, :, :Vx]
    pack = ops.HeadRows(lens.view(-1), B, L)
    rows = int(pack.count.item())
    out = (torch.empty(B, L - 1, device="cuda"), torch.empty(B, L - 1, dtype=torch.int32, device="cuda"),
           torch.empty(B, L - 1, dtype=torch.int32, device="cuda"))
    junk = torch.empty(96 * 1024 * 1024, device="cuda")           # 384 MB: flushes L2 and the Infinity Cache

    def kernel():
        ops.row_logprob_rank(scores, caps, pack, pad, out=out)

    kernel()
    hot = median([timed_block(kernel, 20) for _ in range(blocks)])
    cold = []
    for _ in range(blocks):
        junk.fill_(1.0)
        cold.append(timed_block(kernel, 1))
    cold = median(cold)
    nbytes = 4.0 * rows * Vx
    res = dict(config=name, variant=variant, B=B, L=L, Vx=Vx, valid_rows=rows, blocks=blocks, calls_per_block=calls,
               score_captions_ms=median(ta), score_captions_ms_min_max=[min(ta), max(ta)],
               forward_plus_torch_ms=median(tb), forward_plus_torch_ms_min_max=[min(tb), max(tb)],
               routes_agree=agree,
               row_kernel=dict(bytes_one_read=nbytes, hot_us=hot * 1e3, cold_us=cold * 1e3,
                               hot_bytes_per_s=nbytes / (hot * 1e-3), cold_bytes_per_s=nbytes / (cold * 1e-3),
                               floor_us_at_hbm_peak=nbytes / HBM_PEAK * 1e6,
                               cold_share_of_hbm_peak=nbytes / (cold * 1e-3) / HBM_PEAK))
    print(json.dumps(res), flush=True)
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_captions_bench.json"))
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--configs", default="cfg2,cfg4")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("score_captions_bench needs a GPU")
    results = [run(n, args.blocks, args.calls) for n in args.configs.split(",")]
    with open(args.out, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), hbm_peak_bytes_per_s=HBM_PEAK, results=results), f, indent=1)
        f.write("\n")
