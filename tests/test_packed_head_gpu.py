"""The packed score head of the fused training step on the GPU, in the three product modes of the large
GEMM tiles:
  * ick_gemm with device-side row (m_bound) and reduction (k_bound) extents, with gather / scatter row maps, at the head's
    cfg2 shapes against fp64 torch products; what lies past the bound is byte-for-byte untouched, and NaN rows past the
    bound of an operand never reach a result;
  * the forward head over the packed rows: bit-identical to the unpacked head's rows at the valid positions;
  * the packed cross entropy: token count = sum(decode_len) exactly, gradients of the valid rows bit-identical;
  * TrainStep, new path against ICK_NO_PACKED_HEAD=1 from the same state: loss and the whole gradient bucket with dropout
    on, both paths against the oracle (dropout off: the oracle cannot draw the counter-based masks) with the tolerance of
    tests/test_round5_gpu.py, bit-reproducibility in deterministic mode, and a batch without a single valid row.
The reference's loss: geo-aware/train.py:275-281; its decoder forward: geo-aware/models.py:315-361."""
import math
import types

import pytest
import torch

import ick_amd.synth as synth
from oracle import restatement as R
from test_bench_sizes_gpu import reference_train_step
from test_forward_gpu import build_decoder
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu

M_ROWS, D, V = 1280, 300, 10000            # cfg2: B * L decoder rows, model width, vocabulary
BOUNDS = [1, 127, 128, 129, 744, 1280]


@pytest.fixture()
def ops(gemm_split):
    from ick_amd import ops as o
    return o


def rnd(*shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).cuda()


def rows_of(Mp, seed=5):
    """A synthetic packed row list of Mp rows over M_ROWS logical ones (an injective map: scatters do not collide)."""
    perm = torch.randperm(M_ROWS, generator=torch.Generator().manual_seed(seed)).to(torch.int32).cuda()
    return types.SimpleNamespace(rowmap=perm, count=torch.tensor([Mp], dtype=torch.int32).cuda(), rowstart=None)


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def within(got, ref, abs_a, abs_b, K, base=None):
    """|got - ref| against the probabilistic rounding bound of an fp32 inner product of length K accumulated in any order
    (Higham & Mary 2019: lambda sqrt(K) u sum |a_i b_i| with u = 2^-24; lambda = 4), element by element; base: a value the
    product was added to (one more rounding of the result).  A term left out, taken twice or read from a row past the
    bound is off by a whole product -- orders of magnitude above this."""
    tol = 4.0 * math.sqrt(max(K, 1)) * 2.0 ** -24 * (abs_a.double() @ abs_b.double())
    if base is not None:
        tol = tol + 2.0 ** -23 * (base.double().abs() + ref.abs())
    err = (got.double() - ref).abs()
    assert torch.isfinite(got).all()
    worst = (err / tol).max().item()
    assert worst <= 1.0, (worst, err.max().item())


@pytest.mark.parametrize("presplit", [False, True], ids=["b_direct", "b_presplit"])
@pytest.mark.parametrize("Mp", BOUNDS)
def test_gemm_row_bound_gather_forward(ops, Mp, presplit):
    """The vocabulary projection's form: A rows gathered through the row list, packed output rows, bias."""
    pack = rows_of(Mp)
    h, w, b = rnd(M_ROWS, D, seed=1), rnd(V, D, seed=2, scale=0.1), rnd(V, seed=3)
    ld = V + 24                                         # the pointer columns lie behind the vocabulary's
    out = rnd(M_ROWS, ld, seed=4)
    before = out.clone()
    w_ps = None
    if presplit and ops.gemm_split_mode() >= 1:
        w_ps = ops.presplit_buffer(V, D, w.device)
        ops.presplit_weights([(w, w_ps)])
    ops.gemm_raw(h, w, out, M_ROWS, V, D, D, 1, D, 1, ld, bias=b, b_ps=w_ps, a_grp=1, a_gs=D, a_gmap=pack.rowmap,
                 m_bound=pack.count)
    torch.cuda.synchronize()
    ref = h[pack.rowmap[:Mp].long()].double() @ w.double().t() + b.double()
    within(out[:Mp, :V], ref, h[pack.rowmap[:Mp].long()].abs(), w.abs().t(), D)
    assert same_bits(out[Mp:], before[Mp:]) and same_bits(out[:, V:], before[:, V:])


@pytest.mark.parametrize("split_k", [1, 12])
@pytest.mark.parametrize("presplit", [False, True], ids=["b_direct", "b_presplit"])
@pytest.mark.parametrize("Mp", BOUNDS)
def test_gemm_row_bound_scatter_data_gradient(ops, Mp, presplit, split_k):
    """The vocabulary data gradient's form: packed score-gradient rows (NaN past the bound, as uninitialised memory may
    be), k-major weight, rows scattered through the row list into a buffer that already holds values."""
    pack = rows_of(Mp)
    dy, w = rnd(M_ROWS, V, seed=6), rnd(V, D, seed=7, scale=0.1)
    dy[Mp:] = float("nan")
    dx = rnd(M_ROWS, D, seed=8)
    before = dx.clone()
    wt_ps = None
    if presplit and ops.gemm_split_mode() >= 1:
        wt_ps = ops.presplit_buffer(D, V, w.device)
        ops.presplit_weights([(w.t(), wt_ps)])
    ops.gemm_raw(dy, w, dx, M_ROWS, D, V, V, 1, 1, D, D, atomic=split_k > 1, accumulate=split_k == 1, split_k=split_k,
                 b_ps=wt_ps, m_bound=pack.count, c_grp=1, c_gs=D, c_gmap=pack.rowmap)
    torch.cuda.synchronize()
    idx = pack.rowmap[:Mp].long()
    ref = before[idx].double() + dy[:Mp].double() @ w.double()
    within(dx[idx], ref, dy[:Mp].abs(), w.abs(), V, base=before[idx])
    rest = torch.ones(M_ROWS, dtype=torch.bool, device="cuda")
    rest[idx] = False
    assert same_bits(dx[rest], before[rest])


@pytest.mark.parametrize("presplit", [False, True], ids=["b_packed_copy", "b_presplit_gathered"])
@pytest.mark.parametrize("Mp", BOUNDS)
def test_gemm_reduction_bound_weight_gradient(ops, Mp, presplit):
    """The vocabulary weight gradient's form: the reduction runs over the Mp packed rows; the activation operand is either
    the pre-split copy gathered through the row list or a packed copy; the bias gradient sums the same Mp rows."""
    pack = rows_of(Mp)
    dy, x = rnd(M_ROWS, V, seed=9), rnd(M_ROWS, D, seed=10, scale=0.1)
    dy[Mp:] = float("nan")
    dw, db = rnd(V, D, seed=11), rnd(V, seed=12)
    dw0, db0 = dw.clone(), db.clone()
    if presplit and ops.gemm_split_mode() >= 1:
        buf = ops.presplit_buffer(D, M_ROWS, x.device)
        buf.fill_(0xFF)                                  # bf16 NaNs wherever the gathered copy is not written
        ops.presplit_weights([(x.t(), buf)], k_map=pack.rowmap, k_bound=pack.count)
        wg = ops.gemm_args(dy, x, dw, V, D, M_ROWS, 1, V, 1, D, D, atomic=True, split_k=8, b_ps=buf, k_bound=pack.count)
        assert ops.gemm_plan(wg)["presplit"] == 1
        ops.gemm_grouped([wg, ops.colsum_problem(dy, db, split_k=5, k_bound=pack.count)])
    else:
        xk = ops.gather_rows(x, pack)
        wg = ops.gemm_args(dy, xk, dw, V, D, M_ROWS, 1, V, 1, D, D, atomic=True, split_k=5, colsum_a=db,
                           k_bound=pack.count)
        ops.gemm_grouped([wg])
    torch.cuda.synchronize()
    xg = x[pack.rowmap[:Mp].long()].double()
    within(dw, dw0.double() + dy[:Mp].double().t() @ xg, dy[:Mp].abs().t(), xg.abs(), Mp, base=dw0)
    ones = torch.ones(Mp, 1, device="cuda")
    within(db.view(-1, 1), (db0.double() + dy[:Mp].double().sum(0)).view(-1, 1), dy[:Mp].abs().t(), ones, Mp,
           base=db0.view(-1, 1))


def _lengths_cfg2(seed=100):
    c = synth.CONFIGS["cfg2"]
    return synth.make_batch(c["variant"], c["B"], c["L"], c["K"], c["V"], 0, seed)["caption_lengths"]


def test_head_forward_packed_rows_equal_unpacked_rows_bitwise(ops):
    """cfg2: the packed head's row m is the unpacked head's row rowmap[m], bit for bit (same K order per element)."""
    c = synth.CONFIGS["cfg2"]
    B, L, K, Vc = c["B"], c["L"], c["K"], c["V"]
    dec = build_decoder("geo", Vc, synth.make_params("geo", Vc, 7))
    lengths = _lengths_cfg2().cuda()
    pack = ops.HeadRows(lengths, B, L)
    torch.cuda.synchronize()
    Mp = int(pack.count.item())
    assert Mp == int((lengths - 1).sum().item()) == 744
    assert pack.decode_len.tolist() == (lengths.view(-1) - 1).tolist()
    expect = [b * L + t for b in range(B) for t in range(int(lengths[b]) - 1)]
    assert pack.rowmap[:Mp].tolist() == expect and pack.rowstart[B].item() == Mp
    h, ee = rnd(B, L, D, seed=20), rnd(B, K, D, seed=21)
    Vx = Vc + K
    full = torch.zeros(B, L, Vx, device="cuda")
    packed = rnd(B, L, Vx, seed=22)
    before = packed.clone()
    ps = dec._vocab_presplit(B * L) if ops.gemm_split_mode() >= 1 else None
    dec._score_head(h, ee, None, None, None, full, ps)
    dec._score_head(h, ee, None, None, None, packed, ps, pack=pack)
    torch.cuda.synchronize()
    got = packed.view(B * L, Vx)
    assert same_bits(got[:Mp], full.view(B * L, Vx)[pack.rowmap[:Mp].long()])
    assert same_bits(got[Mp:], before.view(B * L, Vx)[Mp:])


def test_head_forward_fact_variant_packed_rows(ops):
    """The knowledge head (predicate gate on the vocabulary rows, fact pointer scores under their indicator)."""
    variant, B, L, K, Vc, Fn = "knowledge", 6, 10, 6, 200, 9
    dec = build_decoder(variant, Vc, synth.make_params(variant, Vc, 8))
    batch = synth.make_batch(variant, B, L, K, Vc, Fn, 9)
    pack = ops.HeadRows(batch["caption_lengths"].cuda(), B, L)
    Mp = int(pack.count.item())
    assert 0 < Mp < B * L
    h, ee, fe = rnd(B, L, D, seed=23), rnd(B, K, D, seed=24), rnd(B, Fn, D, seed=25)
    eib = (torch.rand(B, L, Fn, generator=torch.Generator().manual_seed(1)) > 0.5).float().cuda()
    hv = ops.mul(h, rnd(B, L, D, seed=26))
    Vx = Vc + K + Fn
    full, packed = torch.zeros(B, L, Vx, device="cuda"), torch.zeros(B, L, Vx, device="cuda")
    dec._score_head(h, ee, fe, eib, hv, full)
    dec._score_head(h, ee, fe, eib, hv, packed, pack=pack)
    torch.cuda.synchronize()
    assert same_bits(packed.view(B * L, Vx)[:Mp], full.view(B * L, Vx)[pack.rowmap[:Mp].long()])
    assert packed.view(B * L, Vx)[Mp:].abs().max().item() == 0.0


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("Vx", [10020, 50071])
def test_packed_ce_rows_token_count_and_gradients(ops, Vx, weighted):
    B, L = 16, 12
    pad = 0
    g = torch.Generator().manual_seed(3)
    lengths = torch.randint(2, L + 1, (B, 1), generator=g)
    lengths[3] = 1                                      # a caption without a single row
    caps = torch.randint(1, Vx, (B, L), generator=g).cuda()
    ld = (Vx + 3) // 4 * 4                              # the training step's padded row stride
    scores = torch.zeros(B, L, ld, device="cuda")[:, :, :Vx]
    scores.copy_(rnd(B, L, Vx, seed=30))
    w = rnd(B, seed=31) if weighted else None
    pack = ops.HeadRows(lengths.cuda(), B, L)
    Mp = int(pack.count.item())
    assert Mp == int((lengths - 1).sum())
    idx = pack.rowmap[:Mp].long()
    sp_base = torch.zeros(B * L, ld, device="cuda")
    sp_base[:Mp, :Vx] = scores.reshape(B * L, Vx)[idx]
    sp = sp_base.view(B, L, ld)[:, :, :Vx]
    s1, c1, d1 = ops.packed_ce_rows(sp, caps, pack, pad, weights=w, want_grad=True)
    if weighted:
        s0, c0, d0 = ops.packed_ce_weighted(scores, caps, pack.decode_len, w, pad, want_grad=True)
    else:
        s0, c0, d0 = ops.packed_ce(scores, caps, pack.decode_len, pad, want_grad=True)
    torch.cuda.synchronize()
    assert c1.item() == float(Mp) == c0.item()          # the token count: sum(decode_len) exactly
    assert same_bits(d1.reshape(B * L, Vx)[:Mp], d0.reshape(B * L, Vx)[idx])
    # the row losses are the same numbers, summed in another order
    assert abs(s1.item() - s0.item()) <= 2.0 ** -20 * Mp * max(1.0, abs(s0.item()) / Mp)


_REF = {}


def _reference_step(variant, Vc, P, batch, enc_out, key):
    """The oracle's step is the same for every product mode: computed once per case."""
    if key not in _REF:
        _REF.clear()
        cfg = R.config_from_word_map(variant, synth.make_word_map(Vc))
        _REF[key] = reference_train_step(cfg, P, batch, enc_out)
    return _REF[key]


def _train_case(variant, B, L, K, Vc, Fn, seed):
    P = synth.make_params(variant, Vc, seed)
    batch = synth.make_batch(variant, B, L, K, Vc, Fn, seed)
    enc_out = synth.make_enc_out(B, seed)
    return P, batch, enc_out


def _one_step(variant, Vc, P, batch, enc_out, packed, monkeypatch, dropout, deterministic=None, lengths=None):
    """One captured step from the same state (lr 0 leaves the weights alone) -> (loss, bucket, TrainStep, decoder)."""
    from ick_amd.training import TrainStep
    if packed:
        monkeypatch.delenv("ICK_NO_PACKED_HEAD", raising=False)
    else:
        monkeypatch.setenv("ICK_NO_PACKED_HEAD", "1")
    dec = build_decoder(variant, Vc, P).train()
    if not dropout:
        zero_dropout(dec)
    ts = TrainStep(dec, lr=0.0, grad_clip=5.0, seed=11, deterministic=deterministic)
    assert ts.packed_head == packed
    args = [batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(),
            (batch["caption_lengths"] if lengths is None else lengths).cuda(), batch["entities"]]
    if variant != "geo":
        args.append(batch["facts"].cuda())
    loss = ts(*args)
    torch.cuda.synchronize()
    assert ts.use_graph and ts._graphs, "hipGraph capture failed: the captured step was not exercised"
    return loss.item(), ts.flat_g.clone(), ts, dec


def _oracle_errors(ts, dec, grads_ref):
    """Per gradient max |mine - oracle| / max(1e-3, |oracle|_max), with tests/test_round5_gpu.py's allowance for ReLU
    inputs within rounding of zero (at most two hidden units per linear1, at most two such tensors)."""
    named = dict(dec.named_parameters())
    errs, flipped = {}, 0
    for k, gr in grads_ref.items():
        mine = ts.grads[id(named[k])].detach().cpu()
        gr = gr.clamp(-5.0, 5.0)
        d = (mine - gr).abs()
        scale = max(1e-3, gr.abs().max().item())
        if d.max().item() / scale >= 2e-3 and k.endswith(("linear1.weight", "linear1.bias")):
            rows = d.view(d.shape[0], -1).max(dim=1).values
            bad = rows.topk(2).indices[rows.topk(2).values / scale >= 2e-3]
            d = d.clone()
            d[bad] = 0
            flipped += 1
        errs[k] = d.max().item() / scale
    return errs, flipped


TRAIN_CASES = [("geo", 64, 20, 20, 10000, 0, 31), ("knowledge", 16, 12, 6, 400, 9, 33)]


@pytest.mark.parametrize("variant,B,L,K,Vc,Fn,seed", TRAIN_CASES, ids=["geo_cfg2", "knowledge"])
def test_train_step_packed_head_vs_unpacked(gemm_split, monkeypatch, variant, B, L, K, Vc, Fn, seed):
    """Dropout on (the masks are keyed by the logical element index, so both paths draw the same ones): loss and the
    whole gradient bucket, new path against ICK_NO_PACKED_HEAD=1, with the tolerance tests/test_round5_gpu.py applies to
    a gradient (2e-3 of the tensor's largest element; here of the bucket's)."""
    P, batch, enc_out = _train_case(variant, B, L, K, Vc, Fn, seed)
    l_new, g_new, ts, _ = _one_step(variant, Vc, P, batch, enc_out, True, monkeypatch, dropout=True)
    l_old, g_old, _, _ = _one_step(variant, Vc, P, batch, enc_out, False, monkeypatch, dropout=True)
    n = ts.n
    print("loss new %.8f old %.8f; bucket max |diff| %.3e of max %.3e" %
          (l_new, l_old, (g_new[:n] - g_old[:n]).abs().max().item(), g_old[:n].abs().max().item()))
    assert abs(l_new - l_old) < 2e-5
    assert g_new[n + 1].item() == g_old[n + 1].item() == float((batch["caption_lengths"] - 1).sum())
    scale = max(1e-3, g_old[:n].abs().max().item())
    assert (g_new[:n] - g_old[:n]).abs().max().item() / scale < 2e-3
    # per parameter as well: the same bound against the parameter's own largest element
    named = dict(ts.dec.named_parameters())
    for k, p in named.items():
        if id(p) not in ts.grads:
            continue
        off = (ts.grads[id(p)].data_ptr() - ts.flat_g.data_ptr()) // 4
        a, b = g_new[off:off + p.numel()], g_old[off:off + p.numel()]
        s = max(1e-3, b.abs().max().item())
        assert (a - b).abs().max().item() / s < 2e-3, k


@pytest.mark.parametrize("variant,B,L,K,Vc,Fn,seed", TRAIN_CASES, ids=["geo_cfg2", "knowledge"])
def test_train_step_both_paths_vs_oracle(gemm_split, monkeypatch, variant, B, L, K, Vc, Fn, seed):
    """Dropout off (the oracle cannot draw the kernels' masks): both paths against the reference sequence on the oracle
    with the tolerance of tests/test_round5_gpu.py, the new path's worst error not above the old path's.  The comparison
    of the two errors runs in deterministic mode, where both figures are reproducible (in the default mode the float
    atomics of the split-K sums move either figure by a rounding from run to run): there the two paths differ in the
    vocabulary's weight and bias gradients alone, every other gradient is bit-identical."""
    import ick_amd.ops as ops
    P, batch, enc_out = _train_case(variant, B, L, K, Vc, Fn, seed)
    loss_ref, grads_ref, _ = _reference_step(variant, Vc, P, batch, enc_out, (variant, B, L, K, Vc, Fn, seed))
    worst = {}
    try:
        for det in (False, True):
            for packed in (True, False):
                loss, g, ts, dec = _one_step(variant, Vc, P, batch, enc_out, packed, monkeypatch, dropout=False,
                                             deterministic=det)
                errs, flipped = _oracle_errors(ts, dec, grads_ref)
                worst[(det, packed)] = (max(errs.values()), max(errs, key=errs.get), g)
                print("deterministic %s packed %s: loss %.8f (oracle %.8f), worst gradient error %.3e at %s" %
                      (det, packed, loss, loss_ref, worst[(det, packed)][0], worst[(det, packed)][1]))
                assert abs(loss - loss_ref) < 2e-5, (det, packed, loss, loss_ref)
                assert max(errs.values()) < 2e-3 and flipped <= 2, (det, packed, worst[(det, packed)][:2], flipped)
    finally:
        ops.set_deterministic(False)
    assert worst[(True, True)][0] <= worst[(True, False)][0], (worst[(True, True)][:2], worst[(True, False)][:2])
    # deterministic mode: only the vocabulary's parameter gradients may differ between the paths at all
    g_new, g_old = worst[(True, True)][2], worst[(True, False)][2]
    named = dict(dec.named_parameters())
    for k, p in named.items():
        if id(p) in ts.grads and not k.startswith("fc_vocab."):
            off = (ts.grads[id(p)].data_ptr() - ts.flat_g.data_ptr()) // 4
            assert torch.equal(g_new[off:off + p.numel()], g_old[off:off + p.numel()]), k


@pytest.mark.parametrize("variant,B,L,K,Vc,Fn,seed", TRAIN_CASES, ids=["geo_cfg2", "knowledge"])
def test_packed_head_deterministic_mode_is_bit_reproducible(monkeypatch, variant, B, L, K, Vc, Fn, seed):
    import ick_amd.ops as ops
    P, batch, enc_out = _train_case(variant, B, L, K, Vc, Fn, seed)
    try:
        runs = [_one_step(variant, Vc, P, batch, enc_out, True, monkeypatch, dropout=True, deterministic=True)[:2]
                for _ in range(2)]
    finally:
        ops.set_deterministic(False)
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("deterministic", [False, True])
def test_packed_head_without_a_single_valid_row(monkeypatch, deterministic):
    """Every caption of length 1: M' = 0.  The step completes, the token count is zero and no gradient was written."""
    import ick_amd.ops as ops
    variant, B, L, K, Vc, Fn, seed = "knowledge", 6, 10, 6, 200, 9, 35
    P, batch, enc_out = _train_case(variant, B, L, K, Vc, Fn, seed)
    try:
        _, g, ts, _ = _one_step(variant, Vc, P, batch, enc_out, True, monkeypatch, dropout=True,
                                deterministic=deterministic, lengths=torch.ones(B, 1, dtype=torch.int64))
    finally:
        ops.set_deterministic(False)
    n = ts.n
    assert g[n + 1].item() == 0.0 and g[n].item() == 0.0
    assert torch.equal(g[:n], torch.zeros_like(g[:n]))
