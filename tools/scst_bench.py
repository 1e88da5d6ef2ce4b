"""SelfCriticalStep at cfg2 (B = 64 images, n = 5 samples each, max_len 20, V = 10 000, K = 20, geo; greedy
baseline; a trivial reward): per-phase times of a step -- sample (320 rows), greedy (64 rows), device-to-host copy,
host reward + advantages, samples -> captions, the weighted training step on 320 captions -- as the median over
`--steps` timed steps after `--warmup` (HIP events at the phase boundaries; the host phases also by the host clock).
Also reports the decode-graph captures after the first step and after the last one, and the weighted loss kernel
alone (ick_packed_ce_weighted on the step's 320 x 21 x 10 020 scores, graph-free, with its gradient).

    python tools/scst_bench.py [--steps 20] [--warmup 3] [--reward trivial] [--out profiles/scst_bench.json]

--reward picks the reward: trivial (the default, the output above), cider (ick_amd.CiderD on the device, refs = the
batch's captions), cider-host (the plain-Python CIDEr-D restatement of tests/cider_ref.py as a host reward_fn) or all
(the three in one run, one JSON line keyed by reward).  Both CIDEr-D rewards use the same df table, built from a
synthetic 100 000-caption corpus (power-law words, 8-20 words per caption); the 64 images' references are its first 64
captions.  The cider rewards also time the reward launch alone (ick_cider_d in SCST layout, 384 rows, HIP events).
"""
import argparse
import json
import time
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.ops as ops  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.scst import SelfCriticalStep  # noqa: E402
from ick_amd.training import TrainStep  # noqa: E402

REWARDS = ("trivial", "cider", "cider-host")


def synthetic_corpus(V, N=100000, L=22, seed=0, a=0.9):
    """N caption rows [<start>, 8..20 words, <end>, <pad>..] of width L, word ranks drawn with p(r) ~ r^-a."""
    import numpy as np
    wm = synth.make_word_map(V)
    rng = np.random.default_rng(seed)
    ranks = np.arange(1, V - 3)
    p = 1.0 / ranks.astype(np.float64) ** a
    words = rng.choice(ranks, size=(N, L), p=p / p.sum()).astype(np.int64)
    nw = rng.integers(8, L - 1, size=N)
    c = np.full((N, L), wm["<pad>"], dtype=np.int64)
    c[:, 0] = wm["<start>"]
    j = np.arange(L)[None, :]
    body = (j >= 1) & (j <= nw[:, None])
    c[body] = words[body]
    c[j == nw[:, None] + 1] = wm["<end>"]
    return torch.from_numpy(c)


def cider_setup(V, B):
    from ick_amd.cider import CiderD
    wm = synth.make_word_map(V)
    corpus = synthetic_corpus(V)
    t0 = time.perf_counter()
    cider = CiderD(corpus, wm)
    torch.cuda.synchronize()
    info = {"corpus_captions": corpus.shape[0], "df_entries": cider.size,
            "df_table_mb": round(cider.size * 20 / 1e6, 1), "df_build_s": round(time.perf_counter() - t0, 2)}
    return cider, corpus[:B].clone(), info


def host_cider(cider, refs, wm):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from cider_ref import cider_rows, table_to_dict
    keys, counts, lrl = cider.table()
    df = table_to_dict(keys, counts)
    rows = [[list(r)] for r in refs.numpy()]

    def reward(toks, img):
        return cider_rows(toks.numpy(), img.numpy(), rows, df, lrl, wm["<start>"], wm["<end>"], wm["<pad>"])
    return reward


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reward", choices=REWARDS + ("all",), default="trivial")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.reward == "all":
        cider = cider_setup(10000, 64)
        res = {"corpus": cider[2], "rewards": {}}
        for name in REWARDS:
            r = run(a, name, cider)
            r.pop("corpus", None)
            res["rewards"][name] = r
    else:
        res = run(a, a.reward, cider_setup(10000, 64) if a.reward != "trivial" else None)
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


def run(a, reward_name, cider_parts):
    variant, B, n, K, V, T, seed = "geo", 64, 5, 20, 10000, 20, 52
    P = synth.make_params(variant, V, seed)
    wm = synth.make_word_map(V)
    m = ick_amd.load_models(variant)
    dec = m.DecoderTransformer(wm, 300, 512, 512, 10, 3)
    dec.load_state_dict(P, strict=False)
    dec = dec.cuda().train()
    ents = synth.make_entities(variant, B, K, V, seed).cuda()
    enc = synth.make_enc_out(B, seed).cuda()
    end = wm["<end>"]

    def reward(toks, img):      # trivial: shorter captions score higher
        return -(toks != 0).sum(1).double()

    kw = {}
    if reward_name != "trivial":
        cider, refs, corpus_info = cider_parts
        if reward_name == "cider":
            reward = cider
            kw = {"refs": refs.cuda()}
        else:
            reward = host_cider(cider, refs, wm)
    step = SelfCriticalStep(TrainStep(dec), reward, num_samples=n, baseline="greedy", max_len=T)
    step(enc, ents, **kw)
    torch.cuda.synchronize()
    captures_first = step.captures
    for _ in range(a.warmup):
        step(enc, ents, **kw)
    torch.cuda.synchronize()
    phases = {}
    host = {}
    for _ in range(a.steps):
        step.marks = []
        step(enc, ents, **kw)
        torch.cuda.synchronize()
        mk = step.marks
        for (_, e0, h0), (name, e1, h1) in zip(mk, mk[1:]):
            phases.setdefault(name, []).append(e0.elapsed_time(e1))
            host.setdefault(name, []).append(1000.0 * (h1 - h0))
        phases.setdefault("total", []).append(mk[0][1].elapsed_time(mk[-1][1]))
    step.marks = None
    # the weighted loss alone at the step's size (rows of 10 020 scores, 21 positions, 320 captions)
    Vx, Lc, Rr = V + K, T + 1, B * n
    sc = torch.randn(Rr, Lc, Vx, device="cuda")
    caps = torch.randint(1, V, (Rr, Lc), device="cuda")
    dl = torch.randint(1, Lc, (Rr,), device="cuda", dtype=torch.int32)
    w = torch.randn(Rr, device="cuda")
    ce = []
    for i in range(a.steps + a.warmup):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.packed_ce_weighted(sc, caps, dl, w, 0, want_grad=True)
        e1.record()
        e1.synchronize()
        if i >= a.warmup:
            ce.append(e0.elapsed_time(e1))
    res = {"config": "cfg2 geo B=64 n=5 max_len=20 V=10000 K=20 baseline=greedy", "steps": a.steps,
           "warmup": a.warmup, "captures_after_first_step": captures_first, "captures_after_last_step": step.captures,
           "phases_ms_device": {k: round(statistics.median(v), 4) for k, v in phases.items()},
           "phases_ms_host": {k: round(statistics.median(v), 4) for k, v in host.items()},
           "weighted_ce_alone_ms": round(statistics.median(ce), 4),
           "mean_sampled_length_last_step": float((step(enc, ents, **kw).samples != 0).sum(1).double().mean()),
           "end_token": end}
    if reward_name != "trivial":
        res["reward"] = reward_name
        res["corpus"] = corpus_info
        last = step(enc, ents, **kw)
        res["mean_sample_reward_last_step"] = float(torch.as_tensor(last.rewards).double().mean())
    if reward_name == "cider":
        rows = torch.cat([last.samples, last.greedy])
        refs_d = kw["refs"]
        ck = []
        for i in range(a.steps + a.warmup):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            cider.scst(rows, refs_d, n, "greedy")
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ck.append(e0.elapsed_time(e1))
        res["cider_launch_alone_ms"] = round(statistics.median(ck), 4)
    return res


if __name__ == "__main__":
    main()
