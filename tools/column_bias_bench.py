"""Cost of the column bias at cfg5 (32 captions x 20 tokens, V = 10 000, K = 20, geo), in one process:

  predict_beam(beam_size=5)   plain, with a rule on (no_repeat_ngram_size = 2), and with <unk> banned plus the 20 entity
                              pointers at +1.0, rules off and on
  predict_sample              T = 1 and top_p = 0.9, with and without the same bias
  the selection alone         ick_decode_select_beam_rules / _biased (two launches) and ick_decode_select_sample_rules /
                              _biased (one) on a context of the same sizes, outside any graph (each call also
                              resets the state it changes with a few fills, the same on both sides)

The legs are interleaved block by block (each block = `--reps` calls of one leg, timed with HIP events) and the median
block per leg is reported as ms per call with the ratio to its plain leg; every leg also carries its own blocks, and a
biased leg says whether its median lies inside the spread (min .. max) of the plain leg's blocks.

    python tools/column_bias_bench.py [--blocks 9] [--reps 10] [--out profiles/column_bias_bench.json]
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
import ick_amd.decoder as D  # noqa: E402
import ick_amd.lib as L  # noqa: E402
import ick_amd.ops as ops  # noqa: E402
import ick_amd.synth as synth  # noqa: E402


def selection_legs(B, beam, V, K, Lm, d, bias_cpu, seed):
    """The selection entry points on buffers of their own: random score rows, every hypothesis live at step 3."""
    g = torch.Generator().manual_seed(seed)
    dev = "cuda"
    legs = {}

    def ctx_of(R, rps):
        t = dict(word_emb=torch.randn(V, d, generator=g).to(dev), ee=torch.randn(B * K, d, generator=g).to(dev),
                 pe=torch.randn(Lm, d, generator=g).to(dev), scores=torch.randn(R, V, generator=g).to(dev),
                 ptr=torch.randn(R, K, generator=g).to(dev), x0=torch.zeros(R, d, device=dev),
                 next_token=torch.zeros(R, dtype=torch.long, device=dev), next_mask=torch.zeros(R, dtype=torch.long, device=dev),
                 n_done=torch.zeros(1, dtype=torch.int32, device=dev))
        c = L.DecodeCtx()
        c.R, c.rows_per_sample, c.d, c.max_len, c.V, c.K, c.F = R, rps, d, Lm, V, K, 0
        c.end_token, c.pad_token, c.emb_scale, c.scores_ld = 1, 0, 1.0, V
        for n, x in t.items():
            setattr(c, n, x.data_ptr())
        return c, t

    cols, vals = (x.to(dev) for x in bias_cpu)
    rules_t = D.rules_tensor(Lm, 0.0, 0, 0, dev)
    # beam
    R = B * beam
    c, t = ctx_of(R, beam)
    st = dict(cum=torch.zeros(R, device=dev), fin=torch.zeros(R, dtype=torch.int32, device=dev),
              rec=torch.empty(R, (V + K + 1023) // 1024, 18, device=dev), lens=torch.zeros(R, dtype=torch.int32, device=dev),
              bsum=torch.zeros(R, device=dev),
              seq=[torch.zeros(R, Lm, dtype=torch.long, device=dev) for _ in range(2)],
              anc=[torch.zeros(R, Lm, dtype=torch.int32, device=dev) for _ in range(2)])
    bs = L.BeamState()
    bs.cum, bs.fin, bs.rec, bs.start_token = st["cum"].data_ptr(), st["fin"].data_ptr(), st["rec"].data_ptr(), 2
    bs.seq_in, bs.seq_out = st["seq"][0].data_ptr(), st["seq"][1].data_ptr()
    bs.anc_in, bs.anc_out = st["anc"][0].data_ptr(), st["anc"][1].data_ptr()
    rs = D._rules_struct(rules_t, st["lens"])
    cb = L.DecodeBias()
    cb.cols, cb.vals, cb.sum = cols.data_ptr(), vals.data_ptr(), st["bsum"].data_ptr()

    def beam_sel(bias):
        def f():
            st["cum"].zero_()
            st["fin"].zero_()
            st["bsum"].zero_()
            t["n_done"].zero_()
            ops.decode_select_beam(c, bs, 3, rs, bias=bias)
        return f

    legs["select_beam_rules"] = beam_sel(None)
    legs["select_beam_biased"] = beam_sel(cb)
    # sampling
    R2 = B * beam
    c2, t2 = ctx_of(R2, beam)
    out = torch.zeros(R2, Lm, dtype=torch.long, device=dev)
    fin2 = torch.zeros(R2, dtype=torch.int32, device=dev)
    c2.output, c2.finished = out.data_ptr(), fin2.data_ptr()
    knobs = [torch.tensor([7], dtype=torch.int64, device=dev), torch.tensor([1.0, 0.9], device=dev),
             torch.tensor([0], dtype=torch.int32, device=dev)]
    ss = L.SampleState()
    ss.seed, ss.temp_top_p, ss.top_k = (k.data_ptr() for k in knobs)
    rs2 = D._rules_struct(rules_t)
    cb2 = L.DecodeBias()
    cb2.cols, cb2.vals = cols.data_ptr(), vals.data_ptr()

    def samp_sel(bias):
        def f():
            fin2.zero_()
            t2["n_done"].zero_()
            ops.decode_select_sample(c2, ss, 3, rs2, bias)
        return f

    legs["select_sample_rules"] = samp_sel(None)
    legs["select_sample_biased"] = samp_sel(cb2)
    return legs, (t, st, t2, out, fin2, knobs, cols, vals, rules_t)


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
    dec = m.DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)
    dec.load_state_dict(P, strict=False)
    dec = dec.cuda().eval()
    ents = synth.make_entities(variant, B, K, V, seed).cuda()
    enc = synth.make_enc_out(B, seed).cuda()
    bias = {"<unk>": float("-inf")}
    bias.update({V + k: 1.0 for k in range(K)})
    rule = dict(no_repeat_ngram_size=2)
    legs = {
        "beam5": lambda: dec.predict_beam(enc, Lm, ents, beam_size=5),
        "beam5_rules": lambda: dec.predict_beam(enc, Lm, ents, beam_size=5, **rule),
        "beam5_bias": lambda: dec.predict_beam(enc, Lm, ents, beam_size=5, column_bias=bias),
        "beam5_rules_bias": lambda: dec.predict_beam(enc, Lm, ents, beam_size=5, column_bias=bias, **rule),
        "sample_t1": lambda: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3),
        "sample_t1_bias": lambda: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3, column_bias=bias),
        "sample_p09": lambda: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3, top_p=0.9),
        "sample_p09_bias": lambda: dec.predict_sample(enc, Lm, ents, num_samples=5, seed=3, top_p=0.9, column_bias=bias),
    }
    base_of = {"beam5_rules": "beam5", "beam5_bias": "beam5", "beam5_rules_bias": "beam5", "sample_t1_bias": "sample_t1",
               "sample_p09_bias": "sample_p09", "select_beam_biased": "select_beam_rules",
               "select_sample_biased": "select_sample_rules"}
    sel, keep = selection_legs(B, 5, V, K, Lm, 300, D.check_column_bias("bench", B, V + K, dec.word_map, bias), seed)
    legs.update(sel)
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
    res = {"config": "cfg5 geo B=32 L=20 V=10000 K=20 beam=5 / 5 samples; bias: <unk> banned, 20 pointers +1.0",
           "build_id": build.source_id(), "blocks": a.blocks, "reps": a.reps, "legs": {}}
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        leg = {"ms_per_call": round(med[k], 4), "blocks_ms": [round(x, 4) for x in v]}
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
