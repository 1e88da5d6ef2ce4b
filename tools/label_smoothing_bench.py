"""What label smoothing costs: the smoothed loss launch against the plain one, and the whole captured
train step with eps 0 against eps 0.1 -- plain and smoothed INTERLEAVED in one run, HIP-event times of repeated blocks,
the median over the blocks and their spread (min .. max) for each side.

  * the loss launch alone (with its gradient) over the PACKED rows of cfg2 (geo, 64 x 20 positions, 10 020 columns) and
    of cfg4 (knowledge, 64 x 20 positions, 50 071 columns, row stride 50 072): ick_packed_ce_packed against
    ick_packed_ce_smooth with 0.1 in the device word, on the same scores, captions and row list;
  * the captured train step at cfg2 as bench.py builds it (feature-map input, Encoder.conv1 inside the step,
    lazy_update) with label_smoothing 0 and 0.1: one TrainStep per child process, the two kinds of process in turn
    (see train_step() for why they do not share a process).

    python tools/label_smoothing_bench.py [--blocks 15] [--launches 50] [--steps 20] [--rounds 3]
                                          [--out profiles/label_smoothing_bench.json]
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
import ick_amd.ops as ops  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.training import TrainStep  # noqa: E402


def timed_block(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def interleaved(sides, blocks, n, before=None):
    """sides: {name: fn}.  Every round times one block of n calls of each side, in turn -> per side the per-call median,
    min and max over the blocks (ms)."""
    for fn in sides.values():                   # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in sides}
    for _ in range(blocks):
        for k, fn in sides.items():
            if before is not None:
                before(k)
            times[k].append(timed_block(fn, n))
    return {k: {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}
            for k, v in times.items()}


def compare(res, a="plain", b="smoothed"):
    res["smoothed_over_plain"] = round(res[b]["median_ms"] / res[a]["median_ms"], 4)
    res["plain_spread"] = round((res[a]["max_ms"] - res[a]["min_ms"]) / res[a]["median_ms"], 4)
    return res


def loss_launch(cfgname, blocks, n):
    c = synth.CONFIGS[cfgname]
    B, L, Vx = c["B"], c["L"], c["V"] + c["K"] + c["F"]
    ld = (Vx + 3) // 4 * 4                      # the training step's padded row stride
    batch = synth.make_batch(c["variant"], B, L, c["K"], c["V"], c["F"], 100)
    caps = batch["captions"].cuda()
    pack = ops.HeadRows(batch["caption_lengths"].cuda(), B, L)
    g = torch.Generator().manual_seed(1)
    scores = torch.randn(B, L, ld, generator=g).cuda()[:, :, :Vx]
    eps = torch.full((1,), 0.1, device="cuda")
    pad = 0
    sides = {"plain": lambda: ops.packed_ce_rows(scores, caps, pack, pad, want_grad=True),
             "smoothed": lambda: ops.packed_ce_smooth(scores, caps, pack, pad, eps, want_grad=True)}
    res = compare(interleaved(sides, blocks, n))
    res.update(config=cfgname, rows=int(pack.count.item()), columns=Vx, row_stride=ld, launches_per_block=n, blocks=blocks)
    return res


def train_step_child(eps, blocks, n):
    """One TrainStep at cfg2 as bench.py builds it, the only one of this process: the per-step times of `blocks` blocks of
    n steps (ms), the last loss, and whether the steps replayed captured graphs."""
    c = synth.CONFIGS["cfg2"]
    variant, B, L, K, V, Fn = c["variant"], c["B"], c["L"], c["K"], c["V"], c["F"]
    m = ick_amd.load_models(variant)
    batch = {k: v.cuda() for k, v in synth.make_batch(variant, B, L, K, V, Fn, 100).items()}
    feats = synth.make_feats(B, 100).cuda()
    args = (batch["captions"], feats, batch["caption_masks"], batch["caption_lengths"], batch["entities"])
    dec = m.DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)
    dec.load_state_dict(synth.make_params(variant, V, 0), strict=False)
    enc = m.Encoder(emb_dim=300)
    cw, cb = synth.make_conv1(0)
    with torch.no_grad():
        enc.conv1.weight.copy_(cw)
        enc.conv1.bias.copy_(cb)
    ts = TrainStep(dec.cuda().train(), lr=4e-4, grad_clip=5.0, encoder=enc.cuda().eval(), lazy_update=True,
                   label_smoothing=eps)
    last = {}

    def step():
        last["loss"] = ts(*args)

    for _ in range(5):
        step()
    times = []
    for _ in range(blocks):
        ts.flush()
        torch.cuda.synchronize()
        times.append(timed_block(step, n))
    loss = float(last["loss"])                  # (read before the flush zeroes the token count)
    ts.flush()
    return {"eps": eps, "block_ms_per_step": [round(t, 5) for t in times], "last_loss": round(loss, 5),
            "captured": bool(ts.use_graph)}


def train_step(rounds, blocks, n):
    """eps 0 and eps 0.1 in turn, each in a fresh child process, `rounds` times: a second TrainStep built in one process
    replays ~1.8x slower than the first whatever its loss (two plain steps: 1.60 / 2.97 ms), so the two sides cannot
    share a process; alternating the processes still puts both sides under the same box and the same drift."""
    import subprocess
    runs = {"plain": [], "smoothed": []}
    for _ in range(rounds):
        for name, eps in (("plain", 0.0), ("smoothed", 0.1)):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(eps), "--blocks", str(blocks),
                                  "--steps", str(n)], capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("child run failed:\n" + out.stderr[-2000:])
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {}
    for name, rs in runs.items():
        v = [t for r in rs for t in r["block_ms_per_step"]]
        res[name] = {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
                     "process_medians_ms": [round(statistics.median(r["block_ms_per_step"]), 5) for r in rs],
                     "last_loss": rs[-1]["last_loss"]}
    compare(res)
    res.update(config="cfg2", steps_per_block=n, blocks_per_process=blocks, processes_per_side=rounds,
               captured=all(r["captured"] for rs in runs.values() for r in rs))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--child", type=float, default=None, help="(internal) one train-step process at this eps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "label_smoothing_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.child is not None:
        print(json.dumps(train_step_child(a.child, a.blocks, a.steps)))
        return
    res = {"loss_launch": {name: loss_launch(name, a.blocks, a.launches) for name in ("cfg2", "cfg4")},
           "train_step": train_step(a.rounds, a.blocks, a.steps), "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
