"""bench.py's launcher logic, no GPU: `python bench.py --gpus N` (WORLD_SIZE unset) must start
`python -m torch.distributed.run --nproc-per-node N ... bench.py <same flags>` as a CHILD process -- never exec, never a
GPU call first -- and relay rank 0's JSON line with the child's exit code."""
import argparse
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_self_launch_builds_the_torchrun_child_and_relays_the_line(monkeypatch, capsys):
    sys.path.insert(0, ROOT)
    import bench
    seen = {}

    def fake_run(cmd, **kw):
        seen["cmd"], seen["env"] = cmd, kw["env"]
        return subprocess.CompletedProcess(cmd, 0, stdout="noise\n" + json.dumps({"n_gpus": 4, "ranks_seen": 4}) + "\n")

    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "7", "--warmup", "2"])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(SystemExit) as e:
        bench.self_launch(argparse.Namespace(gpus=4))
    assert e.value.code == 0
    cmd = seen["cmd"]
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"]
    assert "--nproc-per-node" in cmd and cmd[cmd.index("--nproc-per-node") + 1] == "4"
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and "--nnodes=1" in cmd
    assert cmd[-7:] == [os.path.join(ROOT, "bench.py"), "--gpus", "4", "--steps", "7", "--warmup", "2"]
    assert seen["env"]["HSA_ENABLE_IPC_MODE_LEGACY"] == "0"
    out = capsys.readouterr()
    assert json.loads(out.out.strip()) == {"n_gpus": 4, "ranks_seen": 4} and "noise" in out.err


def test_self_launch_propagates_a_failing_child(monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    monkeypatch.setattr(subprocess, "run", lambda cmd, **kw: subprocess.CompletedProcess(cmd, 3, stdout="boom\n"))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "2"])
    with pytest.raises(SystemExit) as e:
        bench.self_launch(argparse.Namespace(gpus=2))
    assert e.value.code == 3


def test_main_routes_to_the_launcher_only_without_world_size():
    src = open(os.path.join(ROOT, "bench.py")).read()
    body = src[src.index("def main():"):]
    assert body.index('"WORLD_SIZE" not in os.environ and args.gpus > 1') < body.index("torch.cuda.set_device")
    assert "os.exec" not in src


def test_dump_outputs_writes_float_arrays_within_the_budget(monkeypatch, tmp_path):
    """--dump-outputs: floating arrays as float32, integer ones as float64, whole while they fit the budget; above it a
    fixed sample of every large array (the same elements every run)."""
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import bench
    loss, seq = torch.tensor([2.5]), torch.arange(12).view(3, 4)
    big = torch.randn(5000, generator=torch.Generator().manual_seed(1))
    bench.dump_outputs(str(tmp_path / "a"), {"loss": loss, "sequences": seq, "params": big})
    a = {k: np.load(str(tmp_path / "a" / (k + ".npy"))) for k in ("loss", "sequences", "params")}
    assert a["loss"].dtype == np.float32 and a["loss"].tolist() == [2.5]
    assert a["sequences"].dtype == np.float64 and a["sequences"].shape == (3, 4)
    assert np.array_equal(a["sequences"], seq.numpy()) and np.array_equal(a["params"], big.numpy())
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096)
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"loss": loss, "params": big})
    assert sorted(os.listdir(str(tmp_path / "b"))) == ["loss.npy", "params_sample.npy"]
    b, c = (np.load(str(tmp_path / d / "params_sample.npy")) for d in ("b", "c"))
    assert b.shape == (100,) and np.array_equal(b, c) and np.isin(b, big.numpy()).all()


def _run_main(monkeypatch, capsys, argv):
    """bench.main() with the device work stubbed out: -> (JSON line, what the GPU / host legs were asked to do)."""
    sys.path.insert(0, ROOT)
    import torch
    import bench
    calls = {"children": [], "cpu_baseline": 0}

    class FakeWorkload:
        def __init__(self, mode, cfgname, rank):
            import ick_amd.synth as synth
            self.mode, self.cfgname, self.rank = mode, cfgname, rank
            self.cfg, self.seed, self.train_step = dict(synth.CONFIGS[cfgname]), 100 + rank, None

        def describe(self):
            return self.cfgname

    def fake_run_workload(wl, steps, warmup, min_seconds, world, profile_steps, max_repeats=400, dump_dir=None,
                          input_copy=False):
        calls["run_workload"] = {"steps": steps, "warmup": warmup, "profile_steps": profile_steps,
                                 "input_copy": input_copy, "dump_dir": dump_dir}
        return {"ms_per_step": 2.0, "value": 640000.0, "repeats": 1, "timed_region_s": 2e-3 * steps,
                "block_s_min_median_max": [2e-3 * steps] * 3, "graph": True, "by_kernel": [],
                "ms_per_step_with_input_copy": 2.5 if input_copy else None}

    def fake_subprocess_run(cmd, **kw):
        calls["children"].append(cmd)
        child = {"config": {"workload": "w", "graph": True}, "repeats": 1, "ms_per_step": 1.0, "value": 1.0,
                 "unit": "decode-steps/s", "roofline": {}}
        return subprocess.CompletedProcess(cmd, 0, stdout=json.dumps(child) + "\n", stderr="")

    def fake_cpu_baseline(*a, **kw):
        calls["cpu_baseline"] += 1
        return {"value": 1.0, "unit": "decode-steps/s", "cores": 1, "kind": "port", "sample": "", "threads": 1,
                "one_thread": {"value": 1.0, "cores": 1, "sample": ""}}

    monkeypatch.setattr(bench, "Workload", FakeWorkload)
    monkeypatch.setattr(bench, "run_workload", fake_run_workload)
    monkeypatch.setattr(bench, "cpu_baseline", fake_cpu_baseline)
    monkeypatch.setattr(bench, "_gemm_mode", lambda: 1)
    monkeypatch.setattr(subprocess, "run", fake_subprocess_run)
    monkeypatch.setattr(torch.cuda, "set_device", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a: None)
    monkeypatch.setattr(torch.cuda, "empty_cache", lambda *a: None)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    bench.main()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), calls


def test_plain_run_times_the_headline_and_nothing_else(monkeypatch, capsys):
    """`bench.py --gpus 1 --steps K --warmup W`: warm-up, the timed block, the line -- no per-kernel pass, no input-copy
    block, no child workloads, no host baseline."""
    d, calls = _run_main(monkeypatch, capsys, ["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert calls["run_workload"] == {"steps": 7, "warmup": 2, "profile_steps": 0, "input_copy": False, "dump_dir": None}
    assert calls["children"] == [] and calls["cpu_baseline"] == 0
    assert "modes" not in d and "cpu_baseline" not in d and "by_kernel" not in d["roofline"]
    assert d["metric"] == "decode_steps_per_sec" and d["unit"] == "decode-steps/s" and d["higher_is_better"] is True
    assert d["value"] == 640000.0 and d["ms_per_step"] == 2.0 and d["steps"] == 7 and d["warmup"] == 2
    assert d["dtype"] == "f32 (3xbf16 split products, fp32 accumulate)"
    assert d["roofline"]["pass_frac_executed"] > 0


def test_full_run_adds_the_other_legs(monkeypatch, capsys):
    """--full: the per-kernel pass, the input-copy block, the other workloads (each a child run with --full) and the host
    baseline, as a run without --full did before; --no-modes / --no-cpu-baseline / --no-profile drop single legs."""
    d, calls = _run_main(monkeypatch, capsys, ["--full", "--steps", "7", "--warmup", "2"])
    assert calls["run_workload"]["profile_steps"] == 3 and calls["run_workload"]["input_copy"] is True
    assert calls["cpu_baseline"] == 1 and "cpu_baseline" in d
    assert sorted(d["modes"]) == ["beam5_cfg5", "forward_cfg2", "forward_cfg2_exact_fp32", "greedy_cfg5",
                                  "train_cfg2_exact_fp32", "train_cfg4"]
    assert len(calls["children"]) == 6 and all("--full" in c and "--no-modes" in c for c in calls["children"])
    d, calls = _run_main(monkeypatch, capsys, ["--full", "--no-modes", "--no-cpu-baseline", "--no-profile"])
    assert calls["run_workload"]["profile_steps"] == 0 and calls["run_workload"]["input_copy"] is True
    assert calls["children"] == [] and calls["cpu_baseline"] == 0 and "modes" not in d and "cpu_baseline" not in d
