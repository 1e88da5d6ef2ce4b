"""What weight decay inside the optimizer launch costs -- the sides of every comparison INTERLEAVED in
one run, HIP-event times of repeated blocks, the median over the blocks and their spread (min .. max) for each side.

  * the optimizer launch alone over cfg2's and cfg4's bucket, in the flat form (ick_adam_step) and in the derive
    form over the decoder's cover (ick_adam_step_derive), each without and with decay != NULL: plain, with decay (the
    TrainStep's own mask: parameters with ndim >= 2), and plain followed by a separate torch mul_ over the decayed
    extents -- what a user has today, one more launch per decayed parameter.  Over ONE set of arrays ("warm") and
    rotating over enough sets to exceed the 256 MB last-level cache ("cold"; the derive form rotates p, g, m, v under one
    cover, whose images are written in place every time);
  * the captured train step at cfg2 as bench.py builds it (feature-map input, Encoder.conv1 inside the step, lazy_update)
    without and with weight_decay: one TrainStep per child process, the kinds of process in turn;
  * with --parent-root (a built checkout of the parent commit): the default step of that tree (the `off_lazy` child of its
    tools/ema_bench.py) against the default step of this one, child processes of the two trees in turn:
        mkdir parent && git archive HEAD~1 | tar -x -C parent
        (cd parent && python -c "import __graft_entry__ as g; g.build()")

    python tools/weight_decay_bench.py [--blocks 15] [--launches 30] [--steps 20] [--rounds 3] [--parent-root DIR]
                                       [--only launch|step|parent] [--out profiles/weight_decay_bench.json]
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
from ick_amd.training import DerivedWeights, TrainStep  # noqa: E402

LLC_BYTES = 256 << 20    # the last-level cache a repeatedly streamed bucket stays in
WD = 0.01
KINDS = {"off_lazy": dict(lazy_update=True), "decay_lazy": dict(lazy_update=True, weight_decay=WD)}
SIDES = ("plain", "decay", "plain_then_mul")


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


def adam_launch(cfgname, form, blocks, n_launch):
    """The three sides over one config's bucket, flat or derive form, warm and cold."""
    c = synth.CONFIGS[cfgname]
    m = ick_amd.load_models(c["variant"])
    dec = m.DecoderTransformer(synth.make_word_map(c["V"]), 300, 512, 512, 10, 3)
    ts = TrainStep(dec.cuda().train(), weight_decay=WD)
    cover = None
    if form == "derive":
        cover = DerivedWeights.build(ts)
        if cover is None:
            return {"config": cfgname, "form": form, "skipped": "no cover for this decoder"}
        cover.refresh()
    n, mask, word = ts.n, ts._wd_mask, ts._wd_word
    extents = [(ts._dec_bucket._off[id(p)], p.numel()) for _, p in ts._decayed]
    torch.cuda.empty_cache()
    sets = LLC_BYTES * 2 // (4 * 4 * n) + 2
    gen = torch.Generator(device="cuda").manual_seed(1)

    def make(first):
        p = ts.flat_p if first else torch.randn(n, device="cuda", generator=gen) * 0.05
        g = torch.randn(n, device="cuda", generator=gen) * 1e-3
        return [p, g, torch.zeros_like(p), torch.zeros_like(p)]

    arrays = [make(i == 0) for i in range(sets)]
    views = [[a[0][o:o + k] for o, k in extents] for a in arrays]
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    den = torch.full((1,), 1.0, device="cuda")
    common = dict(lr=4e-4, clip=5.0, step_tensor=counter, gscale_den=den, cover=cover)
    factor = 1.0 - 4e-4 * WD
    turn = [0]

    def side(kind, rotate):
        def fn():
            if rotate:
                turn[0] = (turn[0] + 1) % sets
            i = turn[0] if rotate else 0
            p, g, mm, v = arrays[i]
            if kind == "decay":
                ops.adam_update(p, g, mm, v, 1, decay_word=word, decay_mask=mask, **common)
            else:
                ops.adam_update(p, g, mm, v, 1, **common)
                if kind == "plain_then_mul":
                    for t in views[i]:
                        t.mul_(factor)
        return fn

    sides = [(k, r, side(k, r == "cold")) for r in ("warm", "cold") for k in SIDES]
    for _, _, fn in sides:
        for _ in range(sets + 3):
            fn()
    torch.cuda.synchronize()
    times = {(k, r): [] for k, r, _ in sides}
    for _ in range(blocks):
        for k, r, fn in sides:
            times[(k, r)].append(timed_block(fn, n_launch))
    res = {"config": cfgname, "form": form, "floats": n, "bucket_bytes": 4 * n, "granules": int(mask.numel()),
           "granules_selected": int(mask.sum()), "decayed_parameters": len(extents), "sets_rotated": sets,
           "launches_per_block": n_launch, "blocks": blocks}
    for (k, r), v in times.items():
        s = summary(v)
        s["median_us"] = round(s["median_ms"] * 1e3, 2)
        res.setdefault(r, {})[k] = s
    for r in ("warm", "cold"):
        res[r]["decay_over_plain"] = round(res[r]["decay"]["median_ms"] / res[r]["plain"]["median_ms"], 4)
        res[r]["decay_over_plain_then_mul"] = round(res[r]["decay"]["median_ms"] / res[r]["plain_then_mul"]["median_ms"], 4)
        res[r]["decay_inside_plains_spread"] = bool(res[r]["plain"]["min_ms"] <= res[r]["decay"]["median_ms"] <=
                                                    res[r]["plain"]["max_ms"])
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
    ts = TrainStep(dec.cuda().train(), lr=4e-4, grad_clip=5.0, encoder=enc.cuda().eval(), **KINDS[kind])
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
    return {"kind": kind, "block_ms_per_step": [round(t, 5) for t in times], "last_loss": round(loss, 5),
            "captured": bool(ts.use_graph), "bucket_floats": ts.n}


def run_children(sides, rounds, blocks, n):
    """sides: [(name, kind, root)] in turn, each in a fresh child process, `rounds` times."""
    runs = {name: [] for name, _, _ in sides}
    for _ in range(rounds):
        for name, kind, root in sides:
            tool = os.path.join(root, "tools", "ema_bench.py") if root else os.path.abspath(__file__)
            cmd = [sys.executable, tool, "--child", kind, "--blocks", str(blocks), "--steps", str(n)]
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
    res.update(config="cfg2", steps_per_block=n, blocks_per_process=blocks, processes_per_side=rounds,
               captured=all(r["captured"] for rs in runs.values() for r in rs))
    return res


def inside(side, of):
    """Does side's median lie within (or below) the spread of `of`'s blocks?"""
    return bool(side["median_ms"] <= of["max_ms"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("launch", "step", "parent"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its default step (the "
                                                        "`off_lazy` child of its tools/ema_bench.py) is timed in turn "
                                                        "with this tree's")
    ap.add_argument("--child", default=None, help="(internal) one train-step process of this kind")
    ap.add_argument("--root", default=None, help="(internal) the tree a child imports ick_amd from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "weight_decay_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.child is not None:
        print(json.dumps(train_step_child(a.child, a.blocks, a.steps)))
        return
    res = {"device": torch.cuda.get_device_name(0), "weight_decay": WD}
    if a.out and os.path.exists(a.out) and a.only:          # parts measured in separate runs join one file
        res.update(json.loads(open(a.out).read()))
    if a.only in (None, "launch"):
        res["adam_launch"] = {"%s_%s" % (name, form): adam_launch(name, form, a.blocks, a.launches)
                              for name in ("cfg2", "cfg4") for form in ("flat", "derive")}
    if a.only in (None, "step"):
        tr = run_children([(k, k, None) for k in KINDS], a.rounds, a.blocks, a.steps)
        tr["decay_over_off"] = round(tr["decay_lazy"]["median_ms"] / tr["off_lazy"]["median_ms"], 4)
        res["train_step"] = tr
    if a.only in (None, "parent"):
        if a.parent_root:
            vs = run_children([("parent", "off_lazy", a.parent_root), ("this_tree", "off_lazy", None)], a.rounds, a.blocks,
                              a.steps)
            vs["this_tree_over_parent"] = round(vs["this_tree"]["median_ms"] / vs["parent"]["median_ms"], 4)
            vs["this_tree_within_parents_spread"] = inside(vs["this_tree"], vs["parent"])
            res["default_step_vs_parent"] = vs
        elif "default_step_vs_parent" not in res:
            res["default_step_vs_parent"] = "not measured (no --parent-root)"
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
