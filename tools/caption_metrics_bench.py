"""The device caption metrics (ick_caption_metrics) at cfg2's SCST shape, beside their yardsticks, in one run:

  launch     the metrics launch in SCST layout (64 images x 5 samples + 64 greedy rows, T = 20; M = 1 and M = 5
             references per image) and ick_cider_d on the same rows, and the totals launch (ick_caption_metric_sums);
  host       the plain-Python restatement (tests/metrics_ref.py) of the same rows on the host;
  scst       SelfCriticalStep with reward(cider=c, bleu=(0, 0, 0, 0.5)) against the CiderD-only step (cfg2, geo);
  validate   a train.validate() pass over a synthetic VAL split with and without Config.val_caption_metrics.

The two sides of every comparison run in turn, `--blocks` blocks each; a block times `--reps` launches (or `--steps`
steps) between two HIP events (validate: the host clock around the pass, which ends in a synchronisation).  Every
figure is the median over the blocks with the smallest and the largest block beside it.

    python tools/caption_metrics_bench.py [--blocks 7] [--reps 200] [--steps 10] [--out profiles/caption_metrics_bench.json]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.cider import CiderD  # noqa: E402
from ick_amd.metrics import CaptionMetrics  # noqa: E402
from ick_amd.scst import SelfCriticalStep  # noqa: E402
from ick_amd.training import TrainStep  # noqa: E402
from scst_bench import synthetic_corpus  # noqa: E402

V, B, N_S, T, K = 10000, 64, 5, 20, 20


def spread(xs, digits=4):
    return {"median": round(statistics.median(xs), digits), "min": round(min(xs), digits), "max": round(max(xs), digits)}


def in_turn(sides, blocks, timed):
    """sides: name -> callable; every block runs each side once, in turn; timed(fn) -> one figure."""
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


def scst_rows(corpus, M, seed=1):
    """References (B, M, 22) from the corpus and 384 candidate rows of T tokens: each a reference of its image with a
    third of its words redrawn (overlap as SCST samples have it), <end> kept, <pad> after it."""
    wm = synth.make_word_map(V)
    rng = np.random.default_rng(seed)
    refs = corpus[:B * M].reshape(B, M, -1).clone()
    img = np.concatenate([np.repeat(np.arange(B), N_S), np.arange(B)])
    rows = refs[torch.from_numpy(img), torch.from_numpy(rng.integers(0, M, size=img.size))][:, 1:T + 1].numpy().copy()
    redraw = (rng.random(rows.shape) < 0.33) & (rows != wm["<end>"]) & (rows != wm["<pad>"])
    rows[redraw] = rng.integers(1, V - 3, size=int(redraw.sum()))
    return torch.from_numpy(rows), torch.from_numpy(img), refs


def bench_launch(a, cider, corpus, res):
    import metrics_ref
    wm = synth.make_word_map(V)
    m = CaptionMetrics(wm, pointer_base=V)
    mixed = m.reward(cider=cider, bleu=(0, 0, 0, 0.5))
    for M in (1, 5):
        rows, img, refs = scst_rows(corpus, M)
        rows_d, refs_d = rows.cuda(), refs.cuda()
        idx = img.cuda().to(torch.int32)
        base = cider.scst(rows_d, refs_d, N_S, "greedy")[0]
        out = m(rows_d, idx, refs_d)
        sides = {
            "ick_cider_d_us": lambda: cider.scst(rows_d, refs_d, N_S, "greedy"),
            "ick_caption_metrics_us": lambda: ick_amd.ops.caption_metrics(
                rows_d, refs_d, m.start, m.end, m.pad, (), V, 1.2, num_samples=N_S, baseline="greedy",
                base_rewards=base, weights=mixed.weights),
            "cider_then_metrics_us": lambda: mixed.scst(rows_d, refs_d, N_S, "greedy"),
            "ick_caption_metric_sums_us": lambda: m.totals(out),
        }
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        r = in_turn(sides, a.blocks, events_per_call(a.reps))
        host = []
        for _ in range(3):
            t0 = time.perf_counter()
            metrics_ref.caption_rows(rows.numpy(), img.numpy(), [list(x) for x in refs.numpy()], m.start, m.end, m.pad, (), V)
            host.append(1000.0 * (time.perf_counter() - t0))
        r["host_restatement_ms"] = spread(host, 2)
        res["launch_M%d" % M] = r


def bench_scst(a, cider, corpus, res):
    wm = synth.make_word_map(V)
    refs = corpus[:B].clone().cuda()
    rewards = {"cider": cider, "cider_plus_half_bleu4": CaptionMetrics(wm, pointer_base=V).reward(cider=cider, bleu=(0, 0, 0, 0.5))}
    steps = {}
    for name, reward in rewards.items():
        dec = ick_amd.load_models("geo").DecoderTransformer(wm, 300, 512, 512, 10, 3)
        dec.load_state_dict(synth.make_params("geo", V, 52), strict=False)
        dec = dec.cuda().train()
        ents, enc = synth.make_entities("geo", B, K, V, 52).cuda(), synth.make_enc_out(B, 52).cuda()
        step = SelfCriticalStep(TrainStep(dec), reward, num_samples=N_S, baseline="greedy", max_len=T)
        steps[name] = (lambda s=step, e=enc, n=ents: s(e, n, refs=refs))
        for _ in range(3):
            steps[name]()
    torch.cuda.synchronize()
    timed = events_per_call(a.steps)
    res["scst_step_ms"] = {k: {kk: round(vv / 1000.0, 4) for kk, vv in v.items()}
                           for k, v in in_turn(steps, a.blocks, timed).items()}


def bench_validate(a, res):
    import ick_amd.train as tr
    from ick_amd.datasets import CaptionDataset
    with tempfile.TemporaryDirectory() as d:
        wm = synth.write_dataset(d, "bench", "geo", n_train=4, n_val=128, n_test=4, L=22, K=K, V=V)
        m = ick_amd.load_models("geo")
        dec = m.DecoderTransformer(word_map=wm, emb_dim=300, decoder_dim=512, encoder_dim=512, num_heads=10, num_layers=3).cuda()
        enc = m.Encoder(emb_dim=300).cuda()
        dev = torch.device("cuda", torch.cuda.current_device())
        crit = tr.make_criteria(wm["<pad>"])[1].to(dev)
        ds = CaptionDataset(d, "bench", "VAL")
        base = dict(variant="geo", data_dir=d, data_name="bench", batch_size=32)

        def run(**kw):
            loader = torch.utils.data.DataLoader(ds, batch_size=32, shuffle=False)
            return tr.validate(loader, enc, dec, crit, tr.Config(**base, **kw), dev)

        sides = {"loss_only": lambda: run(), "with_caption_metrics": lambda: run(val_caption_metrics=True),
                 "token_metrics": lambda: run(val_token_metrics=True),
                 "token_and_caption_metrics": lambda: run(val_token_metrics=True, val_caption_metrics=True)}
        for fn in sides.values():
            fn()

        def timed(fn):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            return 1000.0 * (time.perf_counter() - t0)

        stdout, sys.stdout = sys.stdout, open(os.devnull, "w")      # (validate prints its lines)
        try:
            res["validate_pass_ms"] = dict(in_turn(sides, a.blocks, timed), captions=128, batch_size=32)
        finally:
            sys.stdout = stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=7)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    corpus = synthetic_corpus(V)
    cider = CiderD(corpus, synth.make_word_map(V))
    res = {"config": "cfg2 SCST shape: 64 images x 5 samples + 64 greedy rows, T=20, V=10000, geo; blocks=%d reps=%d steps=%d"
           % (a.blocks, a.reps, a.steps), "device": torch.cuda.get_device_name(0)}
    bench_launch(a, cider, corpus, res)
    bench_scst(a, cider, corpus, res)
    bench_validate(a, res)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
