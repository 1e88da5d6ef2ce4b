"""Cost of the decoding rules at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo), in one
process: beam 5 without rules, with the rules given explicitly at their defaults, and with (no_repeat_ngram_size 3,
length_penalty 0.6, min_len 5); 5 samples per caption without and with (no_repeat_ngram_size 3, min_len 5).  The legs
are interleaved block by block (each block = `--reps` graph replays of one leg, timed with HIP events) and the median
block per leg is reported as ms per call, with the ratio to the leg's rule-free twin.

    python tools/decode_rules_bench.py [--blocks 9] [--reps 10] [--out profiles/decode_rules_bench.json]
    python tools/decode_rules_bench.py --legs beam5_rules,sample5_rules --blocks 1 --reps 3   # a profiler run
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

DEFAULTS = dict(length_penalty=0.0, no_repeat_ngram_size=0, min_len=0)
BEAM_RULES = dict(length_penalty=0.6, no_repeat_ngram_size=3, min_len=5)
SAMPLE_RULES = dict(no_repeat_ngram_size=3, min_len=5)
TWIN = {"beam5_defaults": "beam5", "beam5_rules": "beam5", "sample5_rules": "sample5"}


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
        "beam5": lambda: dec.predict_beam(enc, L, ents, beam_size=5),
        "beam5_defaults": lambda: dec.predict_beam(enc, L, ents, beam_size=5, **DEFAULTS),
        "beam5_rules": lambda: dec.predict_beam(enc, L, ents, beam_size=5, **BEAM_RULES),
        "sample5": lambda: dec.predict_sample(enc, L, ents, num_samples=5, seed=1),
        "sample5_rules": lambda: dec.predict_sample(enc, L, ents, num_samples=5, seed=1, **SAMPLE_RULES),
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
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20", "beam_rules": BEAM_RULES, "sample_rules": SAMPLE_RULES,
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
