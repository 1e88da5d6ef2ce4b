"""Weight gradients of the decoder layers over the valid caption rows only, on the GPU:
  * the k-line maps of csrc/gemm.hip (ick_gemm_args.a_kmap / b_kmap): a dW = dy^T x problem whose two k-major operands
    keep their logical rows and are read through an ascending row map, against the same launch on ops.gather_rows copies
    of both operands -- the arithmetic order is the same, only addresses differ, so one K slice is compared bit by bit;
    several K slices (some of them empty) with the split-K tolerance of tests/test_packed_head_gpu.py; the fused bias
    column sums; a grouped launch that mixes mapped and unmapped problems; the arguments the plan refuses;
  * the captured TrainStep with the valid-row reduction against ICK_NO_VALID_ROW_WGRAD=1 from the same state.
The reference's training step: geo-aware/train.py:275-292; the layers: geo-aware/models.py:241-244."""
import types

import pytest
import torch

import ick_amd.synth as synth
from test_forward_gpu import build_decoder
from test_packed_head_gpu import same_bits, within

pytestmark = pytest.mark.gpu

K_ROWS = 100                                   # logical rows of both operands (+ one NaN row no map entry may reach)
SHAPES = [(40, 72), (300, 52)]                 # (dy width, x width) = the output's shape: ragged on 32- and 64-wide tiles
BOUNDS = [0, 1, 31, 32, 33, 97, 100]


@pytest.fixture()
def ops(gemm_split):
    from ick_amd import ops as o
    return o


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def operands(n, kk, pad_a, pad_b, seed):
    """dy (K_ROWS + 1, n) and x (K_ROWS + 1, kk) as views with row strides n + pad_a / kk + pad_b; row K_ROWS is NaN."""
    dy = rnd(K_ROWS + 1, n + pad_a, seed=seed)[:, :n]
    x = rnd(K_ROWS + 1, kk + pad_b, seed=seed + 1)[:, :kk]
    dy[K_ROWS] = float("nan")
    x[K_ROWS] = float("nan")
    return dy, x


def row_list(Kp, seed):
    """An ascending map of Kp of the K_ROWS logical rows; the entries from Kp on point at the NaN row: a kernel that read
    a map entry at or past its bound would put NaNs into the result."""
    perm = torch.randperm(K_ROWS, generator=torch.Generator().manual_seed(seed))[:Kp].sort().values
    rowmap = torch.full((K_ROWS + 1,), K_ROWS, dtype=torch.int32)
    rowmap[:Kp] = perm.to(torch.int32)
    return types.SimpleNamespace(rowmap=rowmap.cuda(), count=torch.tensor([Kp], dtype=torch.int32).cuda())


def packed_copy(ops, t, pack):
    """ops.gather_rows copy of t's listed rows, with t's row stride (the two launches must pick the same staging)."""
    out = torch.empty(t.shape[0], t.stride(0), device=t.device)[:, :t.shape[1]]
    out.copy_(ops.gather_rows(t, pack))
    return out


def wgrad(ops, dy, x, dw, db, split_k, pack=None, mapped=False):
    n, kk = dy.shape[1], x.shape[1]
    kw = {} if pack is None else dict(k_bound=pack.count)
    if mapped:
        kw.update(a_kmap=pack.rowmap, b_kmap=pack.rowmap)
    return ops.gemm_args(dy, x, dw, n, kk, K_ROWS, 1, dy.stride(0), 1, x.stride(0), dw.stride(0), atomic=True,
                         split_k=split_k, colsum_a=db, **kw)


@pytest.mark.parametrize("pads", [(8, 4), (3, 5)], ids=["vector_staging", "elementwise_staging"])
@pytest.mark.parametrize("split_k", [1, 2, 3])
@pytest.mark.parametrize("n,kk", SHAPES)
def test_kmap_weight_gradient_vs_gathered_copies(ops, n, kk, split_k, pads):
    dy, x = operands(n, kk, pads[0], pads[1], seed=20)
    for Kp in BOUNDS:
        pack = row_list(Kp, seed=30 + Kp)
        dyg, xg = packed_copy(ops, dy, pack), packed_copy(ops, x, pack)
        idx = pack.rowmap[:Kp].long()
        ref = dy[idx].double().t() @ x[idx].double()
        for with_colsum in (False, True):
            dw0, db0 = rnd(n, kk, seed=40), rnd(n, seed=41)
            got_w, got_b = dw0.clone(), db0.clone()
            a = wgrad(ops, dy, x, got_w, got_b if with_colsum else None, split_k, pack, mapped=True)
            plan = ops.gemm_plan(a)
            assert plan["a_kmajor"] == 1 and plan["b_kmajor"] == 1 and plan["vec"] == (1 if pads == (8, 4) else 0)
            ops.gemm_grouped([a])
            one_w, one_b = dw0.clone(), db0.clone()     # the same problem on packed copies, one K slice
            b = wgrad(ops, dyg, xg, one_w, one_b if with_colsum else None, 1, pack)
            pb = ops.gemm_plan(b)
            assert all(pb[f] == plan[f] for f in ("tile_m", "tile_n", "vec", "split_bf16"))
            ops.gemm_grouped([b])
            torch.cuda.synchronize()
            assert torch.isfinite(got_w).all() and torch.isfinite(got_b).all(), Kp
            if Kp == 0:
                assert same_bits(got_w, dw0) and same_bits(got_b, db0)
            if not with_colsum:
                assert same_bits(got_b, db0)
            if split_k == 1:
                assert same_bits(got_w, one_w) and same_bits(got_b, one_b), (Kp, with_colsum)
            else:
                aa, ab = dy[idx].abs().t(), x[idx].abs()
                within(got_w, one_w.double(), aa, ab, Kp, base=dw0)
                within(got_w, dw0.double() + ref, aa, ab, Kp, base=dw0)
                if with_colsum:
                    ones = torch.ones(Kp, 1, device="cuda")
                    within(got_b.view(-1, 1), one_b.double().view(-1, 1), aa, ones, Kp, base=db0.view(-1, 1))


def test_kmap_on_one_operand_only(ops):
    """The packed head's form in the exact modes: dy is packed already, x keeps its logical rows (b_kmap alone)."""
    n, kk, Kp = 40, 72, 33
    dy, x = operands(n, kk, 8, 4, seed=50)
    pack = row_list(Kp, seed=51)
    xg = ops.gather_rows(x, pack)
    dw0, db0 = rnd(n, kk, seed=52), rnd(n, seed=53)
    got_w, got_b, one_w, one_b = dw0.clone(), db0.clone(), dw0.clone(), db0.clone()
    a = ops.gemm_args(dy, x, got_w, n, kk, K_ROWS, 1, dy.stride(0), 1, x.stride(0), kk, atomic=True, colsum_a=got_b,
                      k_bound=pack.count, b_kmap=pack.rowmap)
    b = ops.gemm_args(dy, xg, one_w, n, kk, K_ROWS, 1, dy.stride(0), 1, xg.stride(0), kk, atomic=True, colsum_a=one_b,
                      k_bound=pack.count)
    ops.gemm_grouped([a])
    ops.gemm_grouped([b])
    torch.cuda.synchronize()
    assert same_bits(got_w, one_w) and same_bits(got_b, one_b) and not same_bits(got_w, dw0)


def test_kmap_large_tiles(ops):
    """Enough 64 x 64 tiles (>= 512) for the large-tile instantiations -- split-bf16 planes in product mode 2."""
    n, kk, Kp = 1280, 1664, 97
    dy, x = operands(n, kk, 8, 4, seed=60)
    pack = row_list(Kp, seed=61)
    dyg, xg = ops.gather_rows(dy, pack), ops.gather_rows(x, pack)
    dw0, db0 = rnd(n, kk, seed=62), rnd(n, seed=63)
    got_w, got_b, one_w, one_b = dw0.clone(), db0.clone(), dw0.clone(), db0.clone()
    a = wgrad(ops, dy, x, got_w, got_b, 1, pack, mapped=True)
    plan = ops.gemm_plan(a)
    assert (plan["tile_m"], plan["tile_n"], plan["vec"]) == (64, 64, 1)
    assert plan["split_bf16"] == (1 if ops.gemm_split_mode() == 2 else 0)
    ops.gemm_grouped([a])
    ops.gemm_grouped([wgrad(ops, dyg, xg, one_w, one_b, 1, pack)])
    torch.cuda.synchronize()
    assert same_bits(got_w, one_w) and same_bits(got_b, one_b)
    idx = pack.rowmap[:Kp].long()
    within(got_w, dw0.double() + dy[idx].double().t() @ x[idx].double(), dy[idx].abs().t(), x[idx].abs(), Kp, base=dw0)


def test_kmap_grouped_launch_of_mapped_and_unmapped_problems(ops):
    """Three problems of one kernel configuration in one ick_gemm_grouped call: two with maps and bounds of their own, one
    without a map (it reduces over all K_ROWS rows)."""
    cases = [((40, 72), 33, 70), ((300, 52), 97, 71), ((40, 72), None, 72)]
    got, one, problems, copies, alive = [], [], [], [], []     # (the argument structs hold raw pointers)
    for (n, kk), Kp, seed in cases:
        dy, x = operands(n, kk, 8, 4, seed=seed)
        dw0, db0 = rnd(n, kk, seed=seed + 10), rnd(n, seed=seed + 20)
        got.append((dw0.clone(), db0.clone()))
        one.append((dw0.clone(), db0.clone()))
        if Kp is None:
            problems.append(wgrad(ops, dy, x, got[-1][0], got[-1][1], 1))
            copies.append(wgrad(ops, dy, x, one[-1][0], one[-1][1], 1))
        else:
            pack = row_list(Kp, seed=seed + 30)
            dyg, xg = ops.gather_rows(dy, pack), ops.gather_rows(x, pack)
            problems.append(wgrad(ops, dy, x, got[-1][0], got[-1][1], 1, pack, mapped=True))
            copies.append(wgrad(ops, dyg, xg, one[-1][0], one[-1][1], 1, pack))
            alive += [pack, dyg, xg]
        got[-1] += (dy, x, dw0)
    ops.gemm_grouped(problems)
    ops.gemm_grouped(copies)
    torch.cuda.synchronize()
    for (gw, gb, dy, x, dw0), (ow, ob) in zip(got, one):
        assert torch.isfinite(gw).all() and same_bits(gw, ow) and same_bits(gb, ob) and not same_bits(gw, dw0)
    gw, _, dy, x, dw0 = got[2]
    within(gw, dw0.double() + dy[:K_ROWS].double().t() @ x[:K_ROWS].double(), dy[:K_ROWS].abs().t(), x[:K_ROWS].abs(),
           K_ROWS, base=dw0)


def test_kmap_rejected_arguments(ops):
    import ick_amd.lib as L
    n, kk = 40, 72
    dy, x = operands(n, kk, 8, 4, seed=80)
    pack = row_list(33, seed=81)
    dw = rnd(n, kk, seed=82)
    ok = wgrad(ops, dy, x, dw, None, 1, pack, mapped=True)
    assert ops.gemm_plan(ok)["a_kmajor"] == 1
    # a k-contiguous operand has no k lines to gather: y = x @ w.T with a map on x, and with a map on w
    w, y = rnd(kk, n, seed=83), rnd(K_ROWS, kk, seed=84)
    for kw in (dict(a_kmap=pack.rowmap), dict(b_kmap=pack.rowmap)):
        bad = ops.gemm_args(dy, w, y, K_ROWS, kk, n, dy.stride(0), 1, n, 1, kk, **kw)
        with pytest.raises(L.IckError):
            ops.gemm_plan(bad)
        with pytest.raises(L.IckError):
            ops.gemm_grouped([bad])
    # the pre-split copy of B is gathered when it is made, not when it is read
    ps = ops.presplit_buffer(kk, K_ROWS, x.device)
    for kw in (dict(a_kmap=pack.rowmap), dict(b_kmap=pack.rowmap), dict(a_kmap=pack.rowmap, b_kmap=pack.rowmap)):
        bad = ops.gemm_args(dy, x, dw, n, kk, K_ROWS, 1, dy.stride(0), 1, x.stride(0), kk, atomic=True, b_ps=ps,
                            k_bound=pack.count, **kw)
        with pytest.raises(L.IckError):
            ops.gemm_plan(bad)
    torch.cuda.synchronize()


# ---- the captured step ---------------------------------------------------------------------------------------------

def _steps(monkeypatch, on, lengths, deterministic=None, steps=2, lr=0.0):
    """`steps` captured steps on the geo variant, B 4, L 6, from the same state -> (losses, parameters, bucket of the last
    step, the ick_gemm_args of every grouped problem).  lr 0 as in tests/test_packed_head_gpu.py's captured steps: the
    comparison is made on what the update consumes, the gradient bucket.  Parameters after an Adam update with lr > 0
    cannot be held to a tolerance tied to the accuracy of a gradient: Adam turns a gradient that is rounding noise -- the
    key bias of every attention, to which the softmax is invariant -- into a full +-lr step whose sign differs between any
    two summation orders (measured at lr 4e-4, two steps: layers.0.self_attn.in_proj_bias 1.06e-4 apart, 2.1e-3 of its
    largest element, every other tensor far inside 2e-3)."""
    from ick_amd import ops
    from ick_amd.training import TrainStep
    variant, B, L, K, Vc, seed = "geo", 4, 6, 5, 200, 37
    if on:
        monkeypatch.delenv("ICK_NO_VALID_ROW_WGRAD", raising=False)
    else:
        monkeypatch.setenv("ICK_NO_VALID_ROW_WGRAD", "1")
    monkeypatch.delenv("ICK_NO_PACKED_HEAD", raising=False)
    P = synth.make_params(variant, Vc, seed)
    batch = synth.make_batch(variant, B, L, K, Vc, 0, seed)
    enc_out = synth.make_enc_out(B, seed)
    dec = build_decoder(variant, Vc, P).train()
    ts = TrainStep(dec, lr=lr, grad_clip=5.0, seed=11, deterministic=deterministic)
    args = [batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(),
            torch.tensor(lengths, dtype=torch.int64).view(B, 1).cuda(), batch["entities"]]
    before = {k: p.detach().clone() for k, p in dec.named_parameters()}
    ops.GROUP_LOG = []
    try:
        losses = [ts(*args).item() for _ in range(steps)]
        torch.cuda.synchronize()
        log = ops.GROUP_LOG
    finally:
        ops.GROUP_LOG = None
    assert ts.use_graph and ts._graphs, "hipGraph capture failed: the captured step was not exercised"
    if hasattr(ts, "flush"):
        ts.flush()
    params = {k: p.detach().clone() for k, p in dec.named_parameters()}
    spans = {}
    for k, p in dec.named_parameters():
        if id(p) in ts.grads:
            off = (ts.grads[id(p)].data_ptr() - ts.flat_g.data_ptr()) // 4
            spans[k] = (off, off + p.numel())
    return losses, params, ts.flat_g[:ts.n].clone(), log, before, (B, L, dec.emb_dim), spans


def _mapped(log, rows):
    return [a for a in log if a.a_kmap and a.b_kmap and a.k_bound and a.K == rows]


def test_train_step_valid_row_wgrad_on_vs_off(gemm_split, monkeypatch):
    """Two steps (dropout on: both legs draw the same masks) with the valid-row reduction and with
    ICK_NO_VALID_ROW_WGRAD=1: the losses of both steps are equal, the parameters agree (bit for bit: lr 0, see _steps) and
    every parameter's gradient agrees within tests/test_packed_head_gpu.py's on/off tolerance, 2e-3 of the tensor's
    largest element, as does the whole bucket."""
    lengths = [1, 2, 4, 6]
    l_on, p_on, g_on, log_on, _, (B, L, d), spans = _steps(monkeypatch, True, lengths)
    l_off, p_off, g_off, log_off, _, _, _ = _steps(monkeypatch, False, lengths)
    print("losses on %s off %s; bucket max |diff| %.3e of max %.3e" %
          (l_on, l_off, (g_on - g_off).abs().max().item(), g_off.abs().max().item()))
    # the decoder layers' weight gradients really took the maps: 6 Linear problems in each of the 3 layers, per traced step
    on, off = _mapped(log_on, B * L), _mapped(log_off, B * L)
    assert len(on) >= 18 and len(on) % 18 == 0 and not off
    assert sorted({(a.M, a.N) for a in on}) == sorted({(d, 512), (512, d), (d, d), (3 * d, d)})
    from ick_amd import ops
    assert all(ops.gemm_plan(a)["a_kmajor"] == 1 and ops.gemm_plan(a)["b_kmajor"] == 1 for a in on)
    assert l_on == l_off
    layer_grads = 0
    for k in p_on:
        assert torch.equal(p_on[k], p_off[k]), k
        if k not in spans:
            continue
        a, b = g_on[spans[k][0]:spans[k][1]], g_off[spans[k][0]:spans[k][1]]
        s = max(1e-3, b.abs().max().item())
        assert (a - b).abs().max().item() / s < 2e-3, k
        layer_grads += int(k.startswith("transformer_decoder.layers.") and b.abs().max().item() > 0.0)
    assert layer_grads >= 18 * 2 - 6         # weights and biases of the 18 Linears (the key biases' gradient may be 0)
    s = max(1e-3, g_off.abs().max().item())
    assert (g_on - g_off).abs().max().item() / s < 2e-3


def test_train_step_valid_row_wgrad_deterministic_mode(monkeypatch):
    """ICK_DETERMINISTIC=1 (TrainStep(deterministic=True)): two runs of the `on` leg end bit-identical, and agree with the
    `off` leg like the default mode does.  (Deterministic mode keeps the full-row reduction, so `off` is bit-identical
    as well: tests/test_packed_head_gpu.py pins every gradient below the head bit-identical to the unpacked head's.)"""
    from ick_amd import ops
    lengths = [1, 2, 4, 6]
    try:
        a = _steps(monkeypatch, True, lengths, deterministic=True)
        b = _steps(monkeypatch, True, lengths, deterministic=True)
        c = _steps(monkeypatch, False, lengths, deterministic=True)
    finally:
        ops.set_deterministic(False)
    assert a[0] == b[0] and torch.equal(a[2], b[2]) and all(torch.equal(a[1][k], b[1][k]) for k in a[1])
    assert a[0] == c[0] and all(torch.equal(a[1][k], c[1][k]) for k in a[1])
    for k, (lo, hi) in a[6].items():
        s = max(1e-3, c[2][lo:hi].abs().max().item())
        assert (a[2][lo:hi] - c[2][lo:hi]).abs().max().item() / s < 2e-3, k


def test_train_step_valid_row_wgrad_without_a_single_valid_row(gemm_split, monkeypatch):
    """Every caption of length 1 (M' = 0): the mapped problems run with an empty reduction, no gradient is written and the
    update leaves every weight untouched."""
    losses, params, g, log, before, (B, L, d), _ = _steps(monkeypatch, True, [1, 1, 1, 1], steps=1, lr=4e-4)
    assert len(_mapped(log, B * L)) >= 18
    assert torch.equal(g, torch.zeros_like(g))
    for k in params:
        assert torch.equal(params[k], before[k]), k
