"""Worker of tests/test_conv1_train_gpu.py::test_two_ranks_train_conv1: one rank of a two-rank TrainStep(train_conv1=True)
under torchrun (collectives over gloo so that two ranks can share the one GPU of the test box).  Each rank takes its half
of one fixed batch, starts from a conv1 of its own (the constructor's broadcast must fix that) and runs two steps in
deterministic mode."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

if __name__ == "__main__":
    out_dir = sys.argv[1]
    import ick_amd.dp as dp
    from test_conv1_train_gpu import DP_CASE, build_step, small_case, step_args
    world = dp.init_from_env()
    rank = int(os.environ["RANK"])
    assert world == 2
    torch.cuda.set_device(0)
    variant, B = DP_CASE
    cfg, P, batch, feats, cw, cb = small_case(variant, B)
    half = B // world
    lo, hi = rank * half, (rank + 1) * half
    mine = {k: v[lo:hi] for k, v in batch.items()}
    ts, dec, enc = build_step(cfg, P, 31 + rank, deterministic=True)      # make_encoder(seed): another conv1 on rank 1
    args = step_args(mine, feats[lo:hi])
    ts(*args)
    g1 = ts.enc_g.detach().cpu().clone()
    ts(*args)
    torch.cuda.synchronize()
    torch.save({"enc_p": ts.enc_p.detach().cpu().clone(), "g1": g1, "flat_p": ts.flat_p.detach().cpu().clone(),
                "steps": int(ts.counter.item())}, os.path.join(out_dir, "conv1_rank%d.pt" % rank))
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()
