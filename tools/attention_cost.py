"""Cost of return_attention on the fused decode: greedy (32 captions x 20 tokens, V = 10 k, K = 20, the cfg5 sizes) and
beam 5 over the same batch, each timed with and without the cross-attention weights.  The two calls alternate after
warm-up and every call is timed by device events, so both see the same clocks and caches.

    python tools/attention_cost.py [--reps 30] [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.synth as synth  # noqa: E402


def build(B, V, K, seed=1):
    P = synth.make_params("geo", V, seed)
    dec = ick_amd.load_models("geo").DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)
    dec.load_state_dict(P, strict=False)
    return dec.cuda().eval(), synth.make_enc_out(B, seed).cuda(), synth.make_entities("geo", B, K, V, seed)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    B, V, K, T = 32, 10000, 20, 20
    dec, enc, ents = build(B, V, K)
    runs = {
        "greedy": (lambda: dec.predict(enc, T, ents), lambda: dec.predict(enc, T, ents, return_attention=True)),
        "beam5": (lambda: dec.predict_beam(enc, T, ents, beam_size=5),
                  lambda: dec.predict_beam(enc, T, ents, beam_size=5, return_attention=True)),
    }
    out = {}
    for name, (plain, attn) in runs.items():
        for _ in range(args.warmup):
            plain()
            attn()
        tp, ta = [], []
        for _ in range(args.reps):
            tp.append(timed(plain))
            ta.append(timed(attn))
        mp, ma = statistics.median(tp), statistics.median(ta)
        out[name] = dict(plain_ms=mp, attention_ms=ma, overhead_pct=100.0 * (ma - mp) / mp,
                         plain_min_ms=min(tp), attention_min_ms=min(ta), reps=args.reps)
        print("%-6s plain %.3f ms  attention %.3f ms  (+%.1f %%)  [min %.3f / %.3f]"
              % (name, mp, ma, out[name]["overhead_pct"], min(tp), min(ta)), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
