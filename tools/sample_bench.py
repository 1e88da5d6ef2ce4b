"""Sampled decode at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo) against greedy predict() and beam 5, in
one process: the legs are interleaved block by block (each block = `--reps` graph replays of one leg, timed with
HIP events) and the median block per leg is reported as ms per call and us per generated position.

    python tools/sample_bench.py [--blocks 9] [--reps 10] [--out profiles/sample_bench.json]
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
        "greedy": lambda: dec.predict(enc, L, ents),
        "beam5": lambda: dec.predict_beam(enc, L, ents, beam_size=5),
        "sample_T1_n1": lambda: dec.predict_sample(enc, L, ents, temperature=1.0, seed=1),
        "sample_p0.9_n1": lambda: dec.predict_sample(enc, L, ents, top_p=0.9, seed=1),
        "sample_T1_n5": lambda: dec.predict_sample(enc, L, ents, num_samples=5, seed=1),
    }
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
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20", "blocks": a.blocks, "reps": a.reps, "legs": {}}
    g = statistics.median(times["greedy"])
    for k, v in times.items():
        med = statistics.median(v)
        res["legs"][k] = {"ms_per_call": round(med, 4), "us_per_position": round(1000 * med / L, 2),
                          "vs_greedy": round(med / g, 3), "blocks_ms": [round(x, 4) for x in v]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
