"""The one-launch pointer-score backward (ick_pointer_scores_bwd_fused[_packed]) against the pair of
launches it replaces, on the same inputs and the same pre-filled outputs.  dh and dctx are sums of one workgroup each:
the same bits in both modes.  dw and dbias meet in float atomics across the samples: the same bits in deterministic
mode and for a single sample, and within the atomics' own reordering error otherwise."""
import pytest
import torch

import ick_amd.ops as ops
from test_ops_gpu import rnd

pytestmark = pytest.mark.gpu

COL0 = 3


def make(B, L, K, d, packed, ind):
    ld = COL0 + K + 2
    lengths = torch.tensor([L + 1, max(1, L - 1)][:B], dtype=torch.int64).cuda()     # sample 1 has padded positions
    pack = ops.HeadRows(lengths, B, L) if packed else None
    ds = rnd(B * L, ld, seed=7 * K + d).cuda()
    ds = ds if packed else ds.view(B, L, ld)
    return dict(ds=ds, pack=pack, h=rnd(B, L, d, seed=1).cuda(), ctx=rnd(B, K, d, seed=2).cuda(), w=rnd(1, d, seed=3).cuda(),
                ind=(rnd(B, L, K, seed=4) > 0).float().cuda() if ind else None)


def run(c, B, L, K, d, fused):
    outs = [rnd(*sh, seed=10 + i).cuda() for i, sh in enumerate([(B, L, d), (B, K, d), (1, d), (1,)])]
    ops.pointer_scores_bwd(c["ds"], COL0, c["h"], c["ctx"], c["w"], c["ind"], *outs, pack=c["pack"], fused=fused)
    return outs


@pytest.mark.parametrize("det", [False, True])
@pytest.mark.parametrize("ind", [False, True])
@pytest.mark.parametrize("packed", [False, True])
@pytest.mark.parametrize("d", [64, 300])
@pytest.mark.parametrize("K", [1, 20])
@pytest.mark.parametrize("L", [1, 5])
@pytest.mark.parametrize("B", [1, 2])
def test_fused_equals_two_launches(B, L, K, d, packed, ind, det):
    c = make(B, L, K, d, packed, ind)
    was = ops.is_deterministic()
    ops.set_deterministic(det)
    try:
        ref = run(c, B, L, K, d, False)
        got = run(c, B, L, K, d, True)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was)
    what = (B, L, K, d, packed, ind, det)
    assert torch.equal(ref[0], got[0]), (what, "dh")
    assert torch.equal(ref[1], got[1]), (what, "dctx")
    for r, g, name, terms in ((ref[2], got[2], "dw", B * L * K), (ref[3], got[3], "dbias", B * L * K)):
        if det or B == 1:
            assert torch.equal(r, g), (what, name)
        else:
            # B atomic addends per address on a pre-filled value, each a sum of at most L * K products of |x| < 1: any two
            # orders differ by at most B roundings of a partial sum below 1 + terms
            tol = B * (1 + terms) * 2.0 ** -23
            assert (r - g).abs().max().item() <= tol, (what, name)
