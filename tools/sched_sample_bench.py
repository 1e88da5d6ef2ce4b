"""What scheduled sampling costs -- the sides of every comparison INTERLEAVED in one run, HIP-event times
of repeated blocks, the median over the blocks and their spread (min .. max) for each side.

  * the mix launch (ick_sched_sample_mix) over cfg2's and cfg4's packed score rows at prob 0.25 and 1.0, in both modes,
    beside ick_row_logprob_rank over the same rows -- the kernel that reads every packed row once, the yardstick for
    prob = 1;
  * the captured train step at cfg2 as bench.py builds it (feature-map input, Encoder.conv1 inside the step, lazy_update
    asked for) without the option, at prob 0.25 and at prob 1, at prob 0.25 with the first pass captured inside graph A
    (ICK_SS_ONE_GRAPH=1) instead of as a graph of its own, and the teacher-forced forward (decoder.forward with the
    attached encoder) in the same run: one object per child process, the kinds of process in turn;
  * the host route the fused path replaces, once: forward() under no_grad + torch.multinomial + where + a TrainStep call;
  * with --parent-root (a built checkout of the parent commit): the default step of that tree (the `off_lazy` child of its
    tools/weight_decay_bench.py) against the default step of this one, child processes of the two trees in turn:
        mkdir parent && git archive HEAD~1 | tar -x -C parent
        (cd parent && python -c "import __graft_entry__ as g; g.build()")

    python tools/sched_sample_bench.py [--blocks 15] [--launches 30] [--steps 20] [--rounds 3] [--parent-root DIR]
                                       [--only launch|step|host|parent] [--out profiles/sched_sample_bench.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import ick_amd  # noqa: E402
import ick_amd.ops as ops  # noqa: E402
import ick_amd.synth as synth  # noqa: E402
from ick_amd.training import TrainStep  # noqa: E402

KINDS = {"off_lazy": None, "ss_p025": dict(prob=0.25, mode="sample"), "ss_p100": dict(prob=1.0, mode="sample"),
         "ss_p025_one_graph": dict(prob=0.25, mode="sample"), "forward": None}
CHILD_ENV = {"ss_p025_one_graph": {"ICK_SS_ONE_GRAPH": "1"}}      # the first pass inside graph A (A/B)


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


def mix_launch(cfgname, blocks, n_launch):
    """The mix launch's sides and ick_row_logprob_rank over one config's packed rows (random scores, synth's lengths)."""
    c = synth.CONFIGS[cfgname]
    B, L, K, V, Fn = c["B"], c["L"], c["K"], c["V"], c["F"]
    Vx = V + K + Fn
    ld = (Vx + 3) // 4 * 4
    batch = synth.make_batch(c["variant"], B, L, K, V, Fn, 100)
    caps, masks = batch["captions"].cuda(), batch["caption_masks"].cuda()
    wm = synth.make_word_map(V)
    pack = ops.HeadRows(batch["caption_lengths"].cuda(), B, L)
    rows = int(pack.count.item())
    gen = torch.Generator(device="cuda").manual_seed(1)
    scores = torch.randn(B, L, ld, device="cuda", generator=gen)[:, :, :Vx]
    counter = torch.zeros(1, device="cuda", dtype=torch.int32)
    temp = torch.ones(1, device="cuda")
    seed = torch.tensor([12345], device="cuda")
    out = (torch.empty_like(caps), torch.empty_like(caps), torch.empty(B, L, device="cuda", dtype=torch.int32))
    rank_out = (torch.empty(B, L - 1, device="cuda"), torch.empty(B, L - 1, device="cuda", dtype=torch.int32),
                torch.empty(B, L - 1, device="cuda", dtype=torch.int32))
    sides, replaced = [], {}
    for prob in (0.25, 1.0):
        word = torch.full((1,), prob, device="cuda")
        for mode in ("sample", "argmax"):
            def fn(word=word, mode=mode):
                ops.sched_sample_mix(scores, pack, caps, masks, V, K, Fn, wm["<start>"], wm["<pad>"], word, temp, seed, counter,
                                     mode=mode, out=out)
            fn()
            replaced["%s_p%03d" % (mode, int(prob * 100))] = int(out[2].sum().item())
            sides.append(("%s_p%03d" % (mode, int(prob * 100)), fn))
    sides.append(("row_logprob_rank", lambda: ops.row_logprob_rank(scores, caps, pack, wm["<pad>"], out=rank_out)))
    for _, fn in sides:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k, _ in sides}
    for _ in range(blocks):
        for k, fn in sides:
            times[k].append(timed_block(fn, n_launch))
    res = {"config": cfgname, "positions": B * L, "packed_rows": rows, "row_bytes": 4 * Vx, "replaced": replaced,
           "launches_per_block": n_launch, "blocks": blocks}
    for k, v in times.items():
        res[k] = summary(v)
        res[k]["median_us"] = round(res[k]["median_ms"] * 1e3, 2)
    return res


def cfg2_objects():
    c = synth.CONFIGS["cfg2"]
    variant, B, L, K, V, Fn = c["variant"], c["B"], c["L"], c["K"], c["V"], c["F"]
    m = ick_amd.load_models(variant)
    batch = {k: v.cuda() for k, v in synth.make_batch(variant, B, L, K, V, Fn, 100).items()}
    feats = synth.make_feats(B, 100).cuda()
    dec = m.DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)
    dec.load_state_dict(synth.make_params(variant, V, 0), strict=False)
    enc = m.Encoder(emb_dim=300)
    cw, cb = synth.make_conv1(0)
    with torch.no_grad():
        enc.conv1.weight.copy_(cw)
        enc.conv1.bias.copy_(cb)
    return dec.cuda(), enc.cuda().eval(), batch, feats


def step_child(kind, blocks, n):
    """One object at cfg2, the only one of this process: a TrainStep as bench.py builds it (kind: without the option, prob
    0.25, prob 1, prob 0.25 with the first pass inside graph A) or the teacher-forced forward; the per-call times of
    `blocks` blocks of n calls (ms)."""
    dec, enc, batch, feats = cfg2_objects()
    args = (batch["captions"], feats, batch["caption_masks"], batch["caption_lengths"], batch["entities"])
    last = {}
    if kind == "forward":
        dec.eval().attach_encoder(enc)
        ts = None

        def step():
            with torch.no_grad():
                last["loss"] = dec(*args)[0][0, 0, 0]
    else:
        ts = TrainStep(dec.train(), lr=4e-4, grad_clip=5.0, encoder=enc, lazy_update=True, scheduled_sampling=KINDS[kind])

        def step():
            last["loss"] = ts(*args)

    for _ in range(5):
        step()
    times = []
    for _ in range(blocks):
        if ts is not None:
            ts.flush()
        torch.cuda.synchronize()
        times.append(timed_block(step, n))
    loss = float(last["loss"])
    out = {"kind": kind, "block_ms_per_step": [round(t, 5) for t in times], "last_loss": round(loss, 5),
           "captured": bool(ts.use_graph) if ts is not None else bool(dec.use_hip_graphs)}
    if ts is not None and ts.ss is not None:
        out["replaced_last_step"] = int(ts.sampled_inputs()[2].sum().item())
    return out


def host_route(n):
    """What a user does without the option: forward() under no_grad, a multinomial draw per position on the (B, L, Vx)
    scores, where() against a Bernoulli coin, masks by column range, and a plain TrainStep call on the result (its targets
    are then the mixed captions too -- the step cannot take separate targets)."""
    dec, enc, batch, feats = cfg2_objects()
    c = synth.CONFIGS["cfg2"]
    V, K = c["V"], c["K"]
    caps, masks, lens = batch["captions"], batch["caption_masks"], batch["caption_lengths"]
    ts = TrainStep(dec.train(), lr=4e-4, grad_clip=5.0, encoder=enc)
    dec.attach_encoder(enc)
    B, L = caps.shape
    pos = torch.arange(L, device="cuda").view(1, L)

    def step():
        ts.flush()
        with torch.no_grad():
            dec.eval()
            scores, caps_sorted, dl = dec(caps, feats, masks, lens, batch["entities"])
            dec.train()
            order = lens.view(-1).sort(descending=True).indices
            s = torch.empty_like(scores)
            s[order] = scores                                   # back into the batch's own order
            draw = torch.multinomial(torch.softmax(s.view(B * L, -1), dim=1), 1).view(B, L)
            pred = torch.cat([caps[:, :1], draw[:, :-1]], dim=1)
            ok = (pos >= 1) & (pos <= lens.view(-1, 1) - 2) & (torch.rand(B, L, device="cuda") < 0.25)
            caps_in = torch.where(ok, pred, caps)
            masks_in = torch.where(ok, (pred >= V).long() + (pred >= V + K).long(), masks)
        return ts(caps_in, feats, masks_in, lens, batch["entities"])

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    return {"config": "cfg2", "calls": n, "ms_per_step": round(timed_block(step, n), 4)}


def run_children(sides, rounds, blocks, n):
    """sides: [(name, kind, root)] in turn, each in a fresh child process, `rounds` times."""
    runs = {name: [] for name, _, _ in sides}
    for _ in range(rounds):
        for name, kind, root in sides:
            tool = os.path.join(root, "tools", "weight_decay_bench.py") if root else os.path.abspath(__file__)
            cmd = [sys.executable, tool, "--child", kind, "--blocks", str(blocks), "--steps", str(n)]
            if root:
                cmd += ["--root", root]
            env = dict(os.environ, **CHILD_ENV.get(kind, {})) if not root else None
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", default=None, choices=("launch", "step", "host", "parent"))
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its default step (the "
                                                        "`off_lazy` child of its tools/weight_decay_bench.py) is timed in "
                                                        "turn with this tree's")
    ap.add_argument("--child", default=None, help="(internal) one process of this kind")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sched_sample_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.child is not None:
        print(json.dumps(step_child(a.child, a.blocks, a.steps)))
        return
    res = {"device": torch.cuda.get_device_name(0)}
    if a.out and os.path.exists(a.out) and a.only:          # parts measured in separate runs join one file
        res.update(json.loads(open(a.out).read()))
    if a.only in (None, "launch"):
        res["mix_launch"] = {name: mix_launch(name, a.blocks, a.launches) for name in ("cfg2", "cfg4")}
    if a.only in (None, "step"):
        tr = run_children([(k, k, None) for k in KINDS], a.rounds, a.blocks, a.steps)
        for k in ("ss_p025", "ss_p100", "ss_p025_one_graph"):
            tr[k + "_minus_off_ms"] = round(tr[k]["median_ms"] - tr["off_lazy"]["median_ms"], 5)
        res["train_step"] = tr
    if a.only in (None, "host"):
        res["host_route"] = host_route(a.steps)
    if a.only in (None, "parent"):
        if a.parent_root:
            vs = run_children([("parent", "off_lazy", a.parent_root), ("this_tree", "off_lazy", None)], a.rounds, a.blocks,
                              a.steps)
            vs["this_tree_over_parent"] = round(vs["this_tree"]["median_ms"] / vs["parent"]["median_ms"], 4)
            vs["this_tree_within_parents_spread"] = bool(vs["this_tree"]["median_ms"] <= vs["parent"]["max_ms"])
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
