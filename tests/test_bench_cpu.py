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
