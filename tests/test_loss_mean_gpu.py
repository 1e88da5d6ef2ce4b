"""The cross-entropy entries that also write the mean loss (ick_packed_ce_*_mean) against the entries
they stand in for, on the same inputs, bit for bit: loss sum, token count, every written gradient row -- and the mean
(sum / count, 0 for a batch without a token).  Row counts below one workgroup's worth, widths that are no multiple of 4
and more than one 256-column pass; a caption of length 1 (no row of that sample counts) and batches of nothing else
(M' = 0).  Every case launches twice, and a captured launch is replayed three times with new scores."""
import pytest
import torch

import ick_amd.ops as ops
from test_ops_gpu import rnd

pytestmark = pytest.mark.gpu

PAD = 0
FORMS = ("packed", "smooth", "weighted")


def lengths_for(B, L, empty):
    if empty:
        return [1] * B
    return [L, 1, 2][:B] if B > 1 else [L]


_CASES = {}


def case(B, L, Vx, empty=False, seed=0):
    key = (B, L, Vx, empty, seed)
    if key not in _CASES:
        ld = (Vx + 3) // 4 * 4
        g = torch.Generator().manual_seed(1000 * Vx + 10 * B + L + seed)
        scores = rnd(B, L, ld, seed=Vx + seed, scale=3.0).cuda()[:, :, :Vx]
        caps = torch.randint(1, Vx, (B, L), generator=g)
        if L > 2 and not empty:
            caps[0, 2] = PAD                       # a <pad> target inside caption 0: the row does not count
        lengths = torch.tensor(lengths_for(B, L, empty), dtype=torch.int64)
        _CASES[key] = dict(scores=scores, caps=caps.cuda(), lengths=lengths.cuda(),
                           dl=(lengths - 1).to(torch.int32).cuda(),
                           w=torch.tensor([1.5, -0.75, 2.0][:B], dtype=torch.float32).cuda(),
                           eps=torch.full((1,), 0.1, dtype=torch.float32, device="cuda"))
    return _CASES[key]


def inputs(form, c, scores=None):
    """-> (the score rows the form reads, its HeadRows or None, how many gradient rows it writes)"""
    scores = c["scores"] if scores is None else scores
    B, L, Vx = scores.shape
    if form == "weighted":
        return scores, None, B * L
    ld = scores.stride(1)
    pack = ops.HeadRows(c["lengths"], B, L)
    Mp = int(pack.count.item())
    base = torch.zeros(B * L, ld, device="cuda")
    base[:Mp, :Vx] = scores.reshape(B * L, Vx)[pack.rowmap[:Mp].long()]
    return base.view(B, L, ld)[:, :, :Vx], pack, Mp


def launch(form, c, rows, pack, mean=None):
    kw = dict(want_grad=True, mean=mean)
    if form == "weighted":
        return ops.packed_ce_weighted(rows, c["caps"], c["dl"], c["w"], PAD, **kw)
    if form == "packed":
        return ops.packed_ce_rows(rows, c["caps"], pack, PAD, **kw)
    return ops.packed_ce_smooth(rows, c["caps"], pack, PAD, c["eps"], weights=c["w"], **kw)


def written(out, Mp):
    s, n, d = out
    B, L, Vx = d.shape
    return s, n, d.reshape(B * L, Vx)[:Mp]          # packed forms: rows from M' on are not written


def run(form, c, scores=None, mean=None):
    """-> (loss_sum, count, the gradient rows the form writes)"""
    rows, pack, Mp = inputs(form, c, scores)
    return written(launch(form, c, rows, pack, mean), Mp)


def check(form, c, mean, what):
    ref = run(form, c)
    got = run(form, c, mean=mean)
    torch.cuda.synchronize()
    for r, g, name in zip(ref, got, ("loss_sum", "count", "dscores")):
        assert torch.equal(r, g), (what, name)
    want = ref[0] / ref[1] if float(ref[1]) > 0 else torch.zeros(1, device="cuda")
    assert torch.equal(mean, want), (what, "mean", mean.item(), want.item())
    return ref


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("Vx", [7, 260, 1031])
@pytest.mark.parametrize("L", [2, 5])
@pytest.mark.parametrize("B", [1, 3])
def test_mean_entries_equal_the_plain_ones(B, L, Vx, form):
    c = case(B, L, Vx)
    mean = torch.full((1,), -7.0, device="cuda")
    for i in range(2):
        ref = check(form, c, mean, (B, L, Vx, form, i))
        mean.fill_(-7.0)
    if B > 1 and L > 2:
        assert float(ref[1]) > 0


@pytest.mark.parametrize("form", FORMS)
def test_batch_without_a_token(form):
    c = case(3, 5, 260, empty=True)
    mean = torch.full((1,), -7.0, device="cuda")
    for i in range(2):
        ref = check(form, c, mean, (form, "empty", i))
        assert float(ref[0]) == 0.0 and float(ref[1]) == 0.0 and float(mean) == 0.0
        mean.fill_(-7.0)


def test_plain_unpacked_form():
    c = case(3, 5, 1031)
    mean = torch.zeros(1, device="cuda")
    ref = ops.packed_ce(c["scores"], c["caps"], c["dl"], PAD, want_grad=True)
    for _ in range(2):
        got = ops.packed_ce(c["scores"], c["caps"], c["dl"], PAD, want_grad=True, mean=mean)
        assert all(torch.equal(r, g) for r, g in zip(ref, got))
        assert torch.equal(mean, ref[0] / ref[1])


@pytest.mark.parametrize("form", FORMS)
def test_captured_launch_replays_with_new_inputs(form):
    B, L, Vx = 3, 5, 260
    c = case(B, L, Vx)
    mean = torch.zeros(1, device="cuda")
    rows, pack, Mp = inputs(form, c)
    static = rows.clone(memory_format=torch.preserve_format)
    launch(form, c, static, pack, mean=mean)           # warm-up off the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with ops.capture(g):
        out = launch(form, c, static, pack, mean=mean)
    for i in range(3):
        new = inputs(form, c, case(B, L, Vx, seed=i + 1)["scores"])[0]
        static.copy_(new)
        g.replay()
        ref = written(launch(form, c, new, pack), Mp)
        torch.cuda.synchronize()
        for r, o, name in zip(ref, written(out, Mp), ("loss_sum", "count", "dscores")):
            assert torch.equal(r, o), (form, i, name)
        assert torch.equal(mean, ref[0] / ref[1])
