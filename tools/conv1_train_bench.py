"""What training Encoder.conv1 costs -- the sides of every comparison INTERLEAVED in one run, HIP-event
times of repeated blocks, the median over the blocks and their spread (min .. max) for each side.

  * the weight-gradient kernel alone (ick_conv1_wgrad: partial + finalise launch, scratch preallocated) at
    (B, C, P, d) = (64, 2048, 196, 300) and (32, ...), against the route Encoder's autograd function takes for the same
    result (decoder._Conv1Fn.backward: a token-major copy of the feature map, two zero fills, ick_gemm with float atomics
    over split-K slices and the column sums riding on it), and as a share of
    max(bytes of feats / HBM rate, 2 * d * C * B * P flop / fp32 matrix peak);
  * the captured train step at cfg2 as bench.py builds it (feature-map input, lazy_update) with conv1 frozen and with
    train_conv1=True -- the price of the feature -- and the per-step time of the loop a user had before: the reference's
    statement sequence through the autograd bridge with conv1 trainable (train.train's unfused branch with an encoder
    optimizer).  One step object per child process, the kinds of process in turn;
  * with --parent-root (a built checkout of the parent commit): the default step of that tree against the default step
    of this one, child processes of the two trees in turn.

    python tools/conv1_train_bench.py [--blocks 15] [--launches 20] [--steps 20] [--rounds 3] [--parent-root DIR]
                                      [--out profiles/conv1_train_bench.json]
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

HBM_PEAK = 8.0e12         # bytes/s, MI355X
FP32_MATRIX_PEAK = 157.3e12   # flop/s, MI355X (v_mfma_f32_*_f32)


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


def kernel_alone(B, blocks, n_launch, Cc=2048, P=196, d=300):
    feats = synth.make_feats(B, 3).cuda()
    g = torch.Generator(device="cuda").manual_seed(5)
    d_img = torch.rand(B, P, d, device="cuda", generator=g) * 2 - 1
    dw, db = torch.empty(d, Cc, device="cuda"), torch.empty(d, device="cuda")
    plan, floats = ops.conv1_wgrad_plan(B, Cc, P, d)
    scratch = torch.empty(floats, device="cuda")
    split = ops.wgrad_split(B * P, d, Cc)
    dy = d_img.view(B * P, d)

    def new():
        ops.conv1_wgrad(d_img, feats, dw, db, scratch)

    def old():                      # decoder._Conv1Fn.backward, the weight / bias part
        xt = feats.view(B, Cc, P).permute(0, 2, 1).contiguous().view(B * P, Cc)
        w = torch.zeros(d, Cc, device="cuda")
        b = torch.zeros(d, device="cuda")
        ops.gemm_raw(dy, xt, w, d, Cc, B * P, 1, d, 1, Cc, Cc, atomic=True, split_k=split, colsum_a=b)
        return w, b

    w_old, b_old = old()
    new()
    torch.cuda.synchronize()
    agree = max(((dw - w_old).abs().max() / w_old.abs().max()).item(), ((db - b_old).abs().max() / b_old.abs().max()).item())
    for fn in (new, old):
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    times = {"new": [], "old_route": []}
    for _ in range(blocks):
        for k, fn in (("new", new), ("old_route", old)):
            times[k].append(timed_block(fn, n_launch))
    flop = 2.0 * d * Cc * B * P
    floor_s = max(4.0 * feats.numel() / HBM_PEAK, flop / FP32_MATRIX_PEAK)
    res = {"shape_B_C_P_d": [B, Cc, P, d], "gflop": round(flop / 1e9, 2), "feats_mbytes": round(4e-6 * feats.numel(), 1),
           "plan_groups_kpergroup_coltiles_rows": list(plan), "scratch_mbytes": round(4e-6 * floats, 1),
           "old_route_split_k": split, "gemm_split_mode": ops.gemm_split_mode(), "floor_us": round(floor_s * 1e6, 1),
           "launches_per_block": n_launch, "blocks": blocks, "max_rel_difference_new_vs_old": agree}
    for k, v in times.items():
        res[k] = summary(v)
        res[k]["median_us"] = round(res[k]["median_ms"] * 1e3, 1)
        res[k]["floor_over_median"] = round(floor_s * 1e3 / res[k]["median_ms"], 4)
    res["new_over_old_route"] = round(res["new"]["median_ms"] / res["old_route"]["median_ms"], 4)
    res["new_at_least_as_fast_within_old_spread"] = res["new"]["median_ms"] <= res["old_route"]["max_ms"]
    return res


def cfg2_case():
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
    return dec.cuda().train(), enc.cuda(), args


def train_step_child(kind, blocks, n):
    """One step object at cfg2, the only one of this process: the per-step times of `blocks` blocks of n steps (ms)."""
    from ick_amd.training import TrainStep
    dec, enc, args = cfg2_case()
    last = {}
    if kind == "unfused":
        # train.train()'s unfused branch with an encoder optimizer over conv1: what fine_tune_encoder=True runs on a
        # feature-file dataset (the trunk gets no input there)
        from ick_amd import train as tr, utils as ut
        crit = torch.nn.CrossEntropyLoss(ignore_index=dec.word_map["<pad>"]).cuda()
        dopt = torch.optim.Adam([p for p in dec.parameters() if p.requires_grad], lr=4e-4)
        eopt = torch.optim.Adam([enc.conv1.weight, enc.conv1.bias], lr=1e-4)
        caps, feats, masks, lens, ent = args

        def step():
            scores, caps_sorted, dl = dec(caps, enc(feats), masks, lens, ent)
            loss = tr.packed_loss(crit, scores, caps_sorted, dl)
            dopt.zero_grad()
            eopt.zero_grad()
            loss.backward()
            ut.clip_gradient(dopt, 5.0)
            ut.clip_gradient(eopt, 5.0)
            dopt.step()
            eopt.step()
            last["loss"] = loss

        flush = torch.cuda.synchronize
        captured = False
    else:
        extra = dict(train_conv1=True, encoder_lr=1e-4) if kind == "train_conv1" else {}
        ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, encoder=enc.eval(), lazy_update=True, **extra)

        def step():
            last["loss"] = ts(*args)

        flush = ts.flush
    for _ in range(5):
        step()
    times = []
    for _ in range(blocks):
        flush()
        torch.cuda.synchronize()
        times.append(timed_block(step, n))
    loss = float(last["loss"])
    flush()
    if kind != "unfused":
        captured = bool(ts.use_graph)
    return {"kind": kind, "block_ms_per_step": [round(t, 5) for t in times], "last_loss": round(loss, 5),
            "captured": captured}


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
    res.update(config="cfg2", steps_per_block=n, blocks_per_process=blocks, processes_per_side=rounds)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=15)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--parent-root", default=None, help="a built checkout of the parent commit: its default step is timed "
                                                        "in turn with this tree's")
    ap.add_argument("--child", default=None, help="(internal) one train-step process of this kind")
    ap.add_argument("--root", default=None, help="(internal) the tree a child imports ick_amd from")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv1_train_bench.json"))
    a = ap.parse_args()
    torch.cuda.set_device(0)
    if a.child is not None:
        print(json.dumps(train_step_child(a.child, a.blocks, a.steps)))
        return
    res = {"kernel_alone": [kernel_alone(B, a.blocks, a.launches) for B in (64, 32)],
           "train_step": run_children([(k, k, None) for k in ("frozen", "train_conv1", "unfused")], a.rounds, a.blocks,
                                      a.steps),
           "device": torch.cuda.get_device_name(0)}
    if a.parent_root:
        res["default_step_vs_parent"] = run_children([("parent", "frozen", a.parent_root), ("this_tree", "frozen", ROOT)],
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
