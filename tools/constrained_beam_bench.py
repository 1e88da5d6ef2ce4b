"""Cost of constrained beam search at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo, beam 5),
in one process: the plain beam, the constrained search with every slot empty (it decodes the plain beam's tokens, so
its ratio to the plain leg is the cost of the FORCED selection kernels and nothing else), and three forced columns per
caption (an entity pointer and two words).  The legs are interleaved block by block (each block = `--reps` graph
replays of one leg, timed with HIP events) and the median block per leg is reported as ms per call, with the ratio to
the plain beam of the same run.

    python tools/constrained_beam_bench.py [--blocks 9] [--reps 10] [--out profiles/constrained_beam_bench.json]
    python tools/constrained_beam_bench.py --legs beam5,beam5_empty --blocks 1 --reps 3   # a profiler run
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
    variant, B, K, V, L, seed = "geo", 32, 20, 10000, 20, 52
    P = synth.make_params(variant, V, seed)
    m = ick_amd.load_models(variant)
    dec = m.DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)
    dec.load_state_dict(P, strict=False)
    dec = dec.cuda().eval()
    ents = synth.make_entities(variant, B, K, V, seed).cuda()
    enc = synth.make_enc_out(B, seed).cuda()
    g = torch.Generator().manual_seed(seed)
    empty = torch.full((B, 3), -1)
    three = torch.stack([V + torch.randint(0, K, (B,), generator=g), torch.randint(10, V - 10, (B,), generator=g),
                         torch.randint(10, V - 10, (B,), generator=g)], dim=1)
    legs = {
        "beam5": lambda: dec.predict_beam(enc, L, ents, beam_size=5),
        "beam5_empty": lambda: dec.predict_beam(enc, L, ents, beam_size=5, force_tokens=empty),
        "beam5_c3": lambda: dec.predict_beam(enc, L, ents, beam_size=5, force_tokens=three),
    }
    if a.legs:
        legs = {k: legs[k] for k in a.legs.split(",")}
    for f in legs.values():          # capture + warm
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    if "beam5" in legs and "beam5_empty" in legs:
        assert torch.equal(legs["beam5"]().clone(), legs["beam5_empty"]()), "the all-empty leg decodes the plain tokens"
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
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20 beam=5", "build_id": build.source_id(), "blocks": a.blocks,
           "reps": a.reps, "legs": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        leg = {"ms_per_call": round(med[k], 4), "blocks_ms": [round(x, 4) for x in v]}
        if k != "beam5" and "beam5" in med:
            leg["vs_beam5"] = round(med[k] / med["beam5"], 4)
        res["legs"][k] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
