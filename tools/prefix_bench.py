"""Cost of caption prefixes at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo), in one process:

  predict_beam(beam_size=5)   plain; an all-empty table (every step free: the prefix kernels on the path of the plain
                              call); a 3-word prefix; a prefix over all 20 steps
  predict_sample              the same four legs, at T = 1 and at top_p = 0.9 (5 samples per caption)

The prefix tokens are a caption's own greedy tokens (no <end> among them), so that a prefixed search runs its 20 steps.
The legs are interleaved block by block (each block = `--reps` calls of one leg, timed with HIP events) and the median
block per leg is reported as ms per call with [min, max] of its blocks and the ratio to its plain leg; a prefix leg says
whether its median lies inside the spread (min .. max) of the plain leg's blocks.

    python tools/prefix_bench.py [--blocks 9] [--reps 10] [--out profiles/prefix_bench.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=9)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--legs", default=None, help="comma-separated subset of the legs")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    variant, B, K, V, Lm, seed = "geo", 32, 20, 10000, 20, 52
    P = synth.make_params(variant, V, seed)
    m = ick_amd.load_models(variant)
    wm = synth.make_word_map(V)
    dec = m.DecoderTransformer(wm, 300, 512, 512, 10, 3)
    dec.load_state_dict(P, strict=False)
    dec = dec.cuda().eval()
    ents = synth.make_entities(variant, B, K, V, seed).cuda()
    enc = synth.make_enc_out(B, seed).cuda()
    # a caption of 20 ordinary columns per image: its greedy tokens, <start> / <end> / <pad> replaced by a word
    own = dec.predict(enc, Lm, ents).t().contiguous().cpu()
    special = torch.tensor([wm["<start>"], wm["<end>"], wm["<pad>"]])
    own = torch.where(torch.isin(own, special), torch.full_like(own, 7), own)
    empty = torch.full((B, Lm), -1, dtype=torch.long)
    three = empty.clone()
    three[:, :3] = own[:, :3]
    tables = {"empty": empty, "prefix3": three, "prefix20": own}
    legs = {"beam5": lambda: dec.predict_beam(enc, Lm, ents, beam_size=5)}
    base_of = {}
    for name, t in tables.items():
        legs["beam5_" + name] = lambda t=t: dec.predict_beam(enc, Lm, ents, beam_size=5, prefix=t)
        base_of["beam5_" + name] = "beam5"
    for tag, kw in (("sample_t1", {}), ("sample_p09", dict(top_p=0.9))):
        legs[tag] = lambda kw=kw: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3, **kw)
        for name, t in tables.items():
            legs[tag + "_" + name] = lambda kw=kw, t=t: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3, prefix=t, **kw)
            base_of[tag + "_" + name] = tag
    if a.legs:
        legs = {k: legs[k] for k in a.legs.split(",")}
    for f in legs.values():          # capture + warm
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.blocks):
        for k, f in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) / a.reps)
    import ick_amd.build as build
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20 beam=5 / 5 samples; prefix: the caption's own greedy tokens",
           "build_id": build.source_id(), "blocks": a.blocks, "reps": a.reps, "legs": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        leg = {"ms_per_call": round(med[k], 4), "min_max_ms": [round(min(v), 4), round(max(v), 4)],
               "blocks_ms": [round(x, 4) for x in v]}
        b = base_of.get(k)
        if b in med:
            leg["vs_" + b] = round(med[k] / med[b], 4)
            leg["inside_spread_of_" + b] = bool(min(times[b]) <= med[k] <= max(times[b]))
        res["legs"][k] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
