"""The geo-reference counts (ick_geo_reference_counts, GeoReferenceMetric) at cfg5's evaluation shape, in one run:

  launch     one GeoReferenceMetric call (clearing the histograms, the launch) on 32 rows x 30 tokens, K = 20 entities
             (one evaluation batch) and on 320 rows, and the same call plus the device add of two batches' counts;
  host       the plain-Python restatement (tests/geo_metric_ref.py) of the same rows on the host, in turn with it;
  evaluate   an eval.evaluate() pass (batches of 32, 30 tokens, no CSV) over a synthetic TEST split with and without
             geo_metric.  The synthetic decoder's greedy captions hold no pointer, so the pass samples (one caption per
             image, temperature 3) and the words it puts in front of pointers are named as the prepositions.

The sides of every comparison run in turn, `--blocks` blocks each; a block times `--reps` calls between two HIP events
(host, evaluate: the host clock; an evaluate pass ends in a synchronisation).  Every figure is the median over the blocks
with the smallest and the largest block beside it.  The bin edges and the train distribution are the test fixture's
(tests/golden/geo_metric_data.npz).

    python tools/geo_metric_bench.py [--blocks 7] [--reps 200] [--out profiles/geo_metric_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.geo_metric import GeoReferenceMetric  # noqa: E402

V, T, K, BATCH = 10000, 30, 20, 32
GEO_WORDS = ["near", "along", "across", "in", "north_of", "south_of", "east_of", "west_of", "of", "the", "a"]


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def in_turn(sides, blocks, timed):
    out = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            out[k].append(timed(fn))
    return {k: spread(v) for k, v in out.items()}


def events_per_call(reps):
    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        return 1000.0 * e0.elapsed_time(e1) / reps          # microseconds per call
    return timed


def host_clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1000.0 * (time.perf_counter() - t0)              # milliseconds


def geo_word_map():
    """The synthetic vocabulary with its first words named as the prepositions and links."""
    wm = synth.make_word_map(V)
    rename = {"w%d" % (i + 1): w for i, w in enumerate(GEO_WORDS)}
    return {rename.get(w, w): i for w, i in wm.items()}


def caption_rows(n, wm, seed=1):
    """n caption rows of T tokens: <start>, then phrases of a few words, a preposition, a link and a pointer (about
    two geo references per caption), <end>, <pad>; one image of K entities per 1 row, a quarter of them <unk_ent>."""
    rng = np.random.default_rng(seed)
    links = [[], ["the"], ["a"], ["of", "the"], ["of"]]
    rows = np.full((n, T), wm["<pad>"], np.int64)
    for r in range(n):
        toks = [wm["<start>"]]
        for _ in range(rng.integers(1, 4)):
            toks += list(rng.integers(12, V - 3, rng.integers(1, 5)))
            toks.append(wm[GEO_WORDS[rng.integers(8)]])
            toks += [wm[w] for w in links[rng.integers(len(links))]]
            toks.append(V + rng.integers(K + 1))
        toks = (toks + [wm["<end>"]])[:T]
        rows[r, :len(toks)] = toks
    ent = rng.uniform(0, 2.5, (n, K, 5)).astype(np.float32)
    ent[:, :, 2] = rng.uniform(-180, 200, (n, K))
    ent[:, :, 4] = rng.integers(0, 986, (n, K))
    names = np.full((n, K, 52), 124, np.int64)
    for b in range(n):
        for k in range(K):
            text = "<unk_ent>" if rng.random() < 0.25 else "entity %d" % k
            names[b, k, :2] = k, len(text)
            names[b, k, 2:2 + len(text)] = [ord(c) for c in text]
    return rows, np.arange(n), ent, names


def bench_launch(a, fx, res):
    import geo_metric_ref
    wm = geo_word_map()
    m = GeoReferenceMetric(wm, fx.bins_d, fx.bins_a, fx.n_types, fx.train, seed=1)
    for n in (BATCH, 10 * BATCH):
        rows, idx, ent, names = caption_rows(n, wm)
        d = [torch.from_numpy(x).cuda() for x in (rows, idx, ent, names)]
        first = m(*d)
        want = geo_metric_ref.run(rows, idx, ent, names, wm, fx.bins_d, fx.bins_a, fx.n_types, seed=1)
        assert np.array_equal(first.generated.cpu().numpy(), want[0]) and np.array_equal(first.marks.cpu().numpy(), want[2])
        sides = {"metric_call_us": lambda: m(*d), "metric_call_and_add_us": lambda: first + m(*d)}
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        r = in_turn(sides, a.blocks, events_per_call(a.reps))
        host = []
        for _ in range(max(3, a.blocks)):
            host.append(host_clock(lambda: geo_metric_ref.run(rows, idx, ent, names, wm, fx.bins_d, fx.bins_a, fx.n_types,
                                                              seed=1)))
            events_per_call(a.reps)(sides["metric_call_us"])            # in turn with the device side
        r["host_restatement_ms"] = spread(host, 2)
        r["geo_references"] = int(want[0][:, 0].sum())
        res["launch_%d_rows" % n] = r


def observed_word_map(seqs, wm):
    """The synthetic decoder knows no prepositions: name the words it did put in front of pointers, most frequent first,
    so that the timed pass counts references."""
    special = {wm["<pad>"], wm["<start>"], wm["<end>"], wm["<unk>"]}
    seen = {}
    for s in seqs:
        for i in range(1, len(s)):
            if V <= s[i] < V + K and s[i - 1] < V and s[i - 1] not in special:
                seen[s[i - 1]] = seen.get(s[i - 1], 0) + 1
    ranked = sorted(seen, key=lambda t: (-seen[t], t))
    rename = dict(zip(ranked, GEO_WORDS))
    return {rename.get(i, w): i for w, i in wm.items()}


def bench_evaluate(a, fx, res):
    import ick_amd.eval as ev
    from ick_amd.datasets import CaptionDataset
    with tempfile.TemporaryDirectory() as d:
        synth.write_dataset(d, "bench", "geo", n_train=4, n_val=4, n_test=4 * BATCH, L=22, K=K, V=V)
        wm = synth.make_word_map(V)
        models = ick_amd.load_models("geo")
        dec = models.DecoderTransformer(wm, 300, 512, 512, 10, 3)
        dec.load_state_dict(synth.make_params("geo", V, 52), strict=False)
        dec, enc = dec.cuda().eval(), models.Encoder(emb_dim=300).cuda().eval()
        ds = CaptionDataset(d, "bench", "TEST")

        def run(**kw):
            loader = torch.utils.data.DataLoader(ds, batch_size=BATCH, shuffle=False)
            return ev.evaluate(enc, dec, loader, wm, max_caption_len=T, out_csv=None,
                               sample=dict(num_samples=1, seed=3, temperature=3.0), **kw)

        m = GeoReferenceMetric(observed_word_map(run()[1], wm), fx.bins_d, fx.bins_a, fx.n_types, fx.train, seed=1)
        sides = {"plain": lambda: run(), "with_geo_metric": lambda: run(geo_metric=m)}
        for fn in sides.values():
            fn()
        res["evaluate_pass_ms"] = dict(in_turn(sides, a.blocks, host_clock), captions=4 * BATCH, batch_size=BATCH,
                                       max_caption_len=T, decode="sampled, temperature 3")
        geo = run(geo_metric=m)[2]["geo_js"]["generated"]
        res["evaluate_pass_ms"]["geo_references"] = sum(v["n_occurrences"] for v in geo.values())


def main():
    import geo_metric_ref
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    fx = geo_metric_ref.Fixture(os.path.join(ROOT, "tests", "golden"))
    res = {"config": "cfg5 evaluation shape: rows of %d tokens, K=%d, V=%d, geo, batches of %d; blocks=%d reps=%d"
           % (T, K, V, BATCH, a.blocks, a.reps), "device": torch.cuda.get_device_name(0)}
    bench_launch(a, fx, res)
    bench_evaluate(a, fx, res)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
