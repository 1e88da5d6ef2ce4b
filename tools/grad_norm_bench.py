"""What global-norm clipping and the device-side learning-rate schedule cost -- the sides of every
comparison INTERLEAVED in one run, HIP-event times of repeated blocks, the median over the blocks and their spread
(min .. max) for each side.

  * the norm pass alone (ick_grad_sqnorm: partial + finalise launch) over a bucket of cfg2's and of cfg4's size, as us
    and as a share of the HBM rate for 4 * n bytes -- over ONE bucket, which the 256 MB last-level cache keeps ("warm",
    what the step sees: the backward pass and the all-reduce have just written the gradients), and rotating over enough
    copies to exceed that cache ("cold");
  * the captured train step at cfg2 as bench.py builds it (feature-map input, Encoder.conv1 inside the step,
    lazy_update) with the feature off, with max_grad_norm, and with max_grad_norm and a cosine schedule: one TrainStep
    per child process, the kinds of process in turn (a second TrainStep in one process replays slower than the first,
    tools/label_smoothing_bench.py);
  * with --parent-root (a built checkout of the parent commit): the default step of that tree against the default step
    of this one, child processes of the two trees in turn.

    python tools/grad_norm_bench.py [--blocks 15] [--launches 50] [--steps 20] [--rounds 3] [--parent-root DIR]
                                    [--out profiles/grad_norm_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:                        # (internal) a child process that imports another tree's package
    sys.path.insert(0, os.path.abspath(sys.argv[sys.argv.index("--root") + 1]))
else:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.ops as ops  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.training import TrainStep  # noqa: E402

HBM_PEAK = 8.0e12        # bytes/s, MI355X
LLC_BYTES = 256 << 20    # the last-level cache a repeatedly read bucket stays in
COSINE = dict(kind="cosine", warmup_steps=100, total_steps=100000, min_lr_ratio=0.1)
KINDS = {"off": {}, "clip": dict(max_grad_norm=1.0), "clip_schedule": dict(max_grad_norm=1.0, lr_schedule=COSINE)}


def timed_block(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / n


def summary(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5),
            "spread": round((max(v) - min(v)) / med, 4)}


def bucket_floats(cfgname):
    """The floats of the gradient bucket TrainStep builds for a config of synth.CONFIGS (alignment pads included)."""
    c = synth.CONFIGS[cfgname]
    m = ick_amd.load_models(c["variant"])
    dec = m.DecoderTransformer(synth.make_word_map(c["V"]), 300, 512, 512, 10, 3)
    return TrainStep(dec.cuda().train()).n


def norm_pass(cfgname, blocks, n_launch):
    n = bucket_floats(cfgname)
    copies = LLC_BYTES * 2 // (4 * n) + 2
    g = torch.Generator(device="cuda").manual_seed(1)
    bufs = [torch.randn(n, device="cuda", generator=g) for _ in range(copies)]
    words = torch.zeros(8, device="cuda")
    words[1], words[3] = 1.0, 1.0
    scratch = torch.empty(ops.grad_sqnorm_plan(n)[2], device="cuda")
    den = torch.full((1,), 1280.0, device="cuda")
    turn = [0]

    def warm():
        ops.grad_sqnorm(bufs[0], words, scratch, gscale_den=den)

    def cold():
        turn[0] = (turn[0] + 1) % copies
        ops.grad_sqnorm(bufs[turn[0]], words, scratch, gscale_den=den)

    for fn in (warm, cold):
        for _ in range(copies + 3):
            fn()
    torch.cuda.synchronize()
    times = {"warm": [], "cold": []}
    for _ in range(blocks):
        for k, fn in (("warm", warm), ("cold", cold)):
            times[k].append(timed_block(fn, n_launch))
    res = {"config": cfgname, "floats": n, "bytes": 4 * n, "copies_rotated": copies, "launches_per_block": n_launch,
           "blocks": blocks, "workgroups": ops.grad_sqnorm_plan(n)[0]}
    for k, v in times.items():
        res[k] = summary(v)
        res[k]["median_us"] = round(res[k]["median_ms"] * 1e3, 2)
        res[k]["share_of_hbm_rate"] = round(4.0 * n / (res[k]["median_ms"] * 1e-3) / HBM_PEAK, 4)
    return res


def train_step_child(kind, blocks, n):
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
    ts = TrainStep(dec.cuda().train(), lr=4e-4, grad_clip=5.0, encoder=enc.cuda().eval(), lazy_update=True, **KINDS[kind])
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
    out = {"kind": kind, "block_ms_per_step": [round(t, 5) for t in times], "last_loss": round(loss, 5),
           "captured": bool(ts.use_graph), "bucket_floats": ts.n}
    if kind != "off":
        out.update(grad_norm=float(ts.grad_norm), clip_coef=float(ts.clip_coef), lr_now=float(ts.lr_now))
    return out


def run_children(sides, rounds, blocks, n):
    """sides: [(name, kind, root)] in turn, each in a fresh child process, `rounds` times."""
    runs = {name: [] for name, _, _ in sides}
    for _ in range(rounds):
        for name, kind, root in sides:
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kind, "--blocks", str(blocks), "--steps", str(n)]
            if root:
                cmd += ["--root", root]
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
            if out.returncode != 0:
                raise RuntimeError("child run failed:\n" + out.stderr[-2000:])
            runs[name].append(json.loads(out.stdout.strip().splitlines()[-1]))
    res = {}
    for name, rs in runs.items():
        res[name] = summary([t for r in rs for t in r["block_ms_per_step"]])
        res[name]["process_medians_ms"] = [round(statistics.median(r["block_ms_per_step"]), 5) for r in rs]
        res[name]["last"] = {k: v for k, v in rs[-1].items() if k != "block_ms_per_step"}
    first = sides[0][0]
    for name in list(res)[1:]:
        res[name]["over_" + first] = round(res[name]["median_ms"] / res[first]["median_ms"], 4)
    res.update(config="cfg2", steps_per_block=n, blocks_per_process=blocks, processes_per_side=rounds,
               captured=all(r["captured"] for rs in runs.values() for r in rs))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its default step is timed "
                                                        "in turn with this tree's")
    ap.add_argument("--child", default=None, help="(internal) one train-step process of this kind")
    ap.add_argument("--root", default=None, help="(internal) the tree a child imports ick_amd from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grad_norm_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.child is not None:
        print(json.dumps(train_step_child(a.child, a.blocks, a.steps)))
        return
    res = {"norm_pass": {name: norm_pass(name, a.blocks, a.launches) for name in ("cfg2", "cfg4")},
           "train_step": run_children([(k, k, None) for k in KINDS], a.rounds, a.blocks, a.steps),
           "device": torch.cuda.get_device_name(0)}
    if a.parent_root:
        res["default_step_vs_parent"] = run_children([("parent", "off", a.parent_root), ("this_tree", "off", ROOT)],
                                                     a.rounds, a.blocks, a.steps)
    else:
        res["default_step_vs_parent"] = "not measured (no --parent-root)"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
