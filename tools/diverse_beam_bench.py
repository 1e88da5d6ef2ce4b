"""Cost of diverse beam search at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo), in one
process: beam 6 plain and in 3 groups (diversity_penalty 0.5), beam 8 plain and in 4 groups, and beam 6 in 3 groups
with the decoding rules on (no_repeat_ngram_size 3, length_penalty 0.6, min_len 5) next to beam 6 with the same rules
and no groups.  The legs are interleaved block by block (each block = `--reps` graph replays of one leg, timed with
HIP events) and the median block per leg is reported as ms per call, with the ratio to the same-width plain beam.

    python tools/diverse_beam_bench.py [--blocks 9] [--reps 10] [--out profiles/diverse_beam_bench.json]
    python tools/diverse_beam_bench.py --legs beam6,beam6_g3 --blocks 1 --reps 3   # a profiler run
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

RULES = dict(length_penalty=0.6, no_repeat_ngram_size=3, min_len=5)
TWIN = {"beam6_g3": "beam6", "beam8_g4": "beam8", "beam6_g3_rules": "beam6_rules"}


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
    legs = {
        "beam6": lambda: dec.predict_beam(enc, L, ents, beam_size=6),
        "beam6_g3": lambda: dec.predict_beam(enc, L, ents, beam_size=6, num_beam_groups=3, diversity_penalty=0.5),
        "beam8": lambda: dec.predict_beam(enc, L, ents, beam_size=8),
        "beam8_g4": lambda: dec.predict_beam(enc, L, ents, beam_size=8, num_beam_groups=4, diversity_penalty=0.5),
        "beam6_rules": lambda: dec.predict_beam(enc, L, ents, beam_size=6, **RULES),
        "beam6_g3_rules": lambda: dec.predict_beam(enc, L, ents, beam_size=6, num_beam_groups=3, diversity_penalty=0.5,
                                                   **RULES),
    }
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
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20", "diversity_penalty": 0.5, "rules": RULES,
           "build_id": build.source_id(), "blocks": a.blocks, "reps": a.reps, "legs": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        leg = {"ms_per_call": round(med[k], 4), "blocks_ms": [round(x, 4) for x in v]}
        if TWIN.get(k) in med:
            leg["vs_" + TWIN[k]] = round(med[k] / med[TWIN[k]], 4)
        res["legs"][k] = leg
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
