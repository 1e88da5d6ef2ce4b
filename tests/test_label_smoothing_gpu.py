"""Label smoothing of the fused training step's cross entropy on the GPU:
  * ick_packed_ce_smooth alone against the float64 restatement (tests/label_smoothing_ref.py, which the CPU tests pin to
    torch's criterion) at the row shapes where a path of the kernel begins or ends, in the plain, weighted and packed
    forms; with 0.0 in the device word it returns the plain entries' bits;
  * one TrainStep(label_smoothing=0.1) step against the CPU oracle with torch's smoothed criterion, torch autograd, clamp
    and Adam, on the packed head and ICK_NO_PACKED_HEAD=1, in every product mode, with and without caption_weights;
  * TrainStep's behaviour: the default step's bits, the effect of the value, bad values, replay after
    set_label_smoothing, a fresh step from the same state, reproducibility and eager launches in deterministic mode;
  * train.main(label_smoothing=0.1): the training loss falls and validation stays the plain loss."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ick_amd.ops as ops
import ick_amd.synth as synth
from ick_amd.lib import IckError
from ick_amd.training import TrainStep, forward_with_tape
from label_smoothing_ref import contributing, smoothed_ce
from oracle import restatement as R
from test_forward_gpu import build_decoder
from test_ops_gpu import rnd
from test_training_gpu import zero_dropout

pytestmark = pytest.mark.gpu

B, LC, PAD = 5, 6, 0
WEIGHTS = [1.5, -0.75, 0.0, 2.0, -3.0]
DECODE_LEN = [LC - 1, 4, 3, 0, 2]        # a full caption, one without a single row; the zero weight has rows
SENTINEL = 12345.0


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def word(eps):
    return torch.full((1,), eps, dtype=torch.float32, device="cuda")


_KERNEL_CASES = {}


def kernel_case(Vx, ld):
    """Scores (scaled by 3), captions with a <pad> target inside caption 1, the packed copy -- and the float64
    references per eps, computed once per shape."""
    key = (Vx, ld)
    if key not in _KERNEL_CASES:
        _KERNEL_CASES.clear()
        g = torch.Generator().manual_seed(Vx)
        sc = rnd(B, LC, ld, seed=Vx, scale=3.0).cuda()[:, :, :Vx]
        caps = torch.randint(1, Vx, (B, LC), generator=g)
        caps[1, 3] = PAD                                   # the target of row (1, 2), inside caption 1
        dl = torch.tensor(DECODE_LEN, dtype=torch.int32)
        pack = ops.HeadRows((dl.long() + 1).cuda(), B, LC)
        Mp = int(pack.count.item())
        assert Mp == sum(DECODE_LEN)
        idx = pack.rowmap[:Mp].long()
        sp_base = torch.full((B * LC, ld), SENTINEL, device="cuda")
        sp_base[:Mp, :Vx] = sc.reshape(B * LC, Vx)[idx]
        c = dict(sc=sc, caps=caps.cuda(), dl=dl.cuda(), pack=pack, Mp=Mp, idx=idx, sp=sp_base.view(B, LC, ld)[:, :, :Vx],
                 w=torch.tensor(WEIGHTS).cuda(), sc_np=sc.cpu().numpy(), caps_np=caps.numpy(), ref={})
        c["keep"] = contributing(c["caps_np"], DECODE_LEN, PAD, Vx)
        _KERNEL_CASES[key] = c
    return _KERNEL_CASES[key]


def reference(c, eps, weighted):
    k = (eps, weighted)
    if k not in c["ref"]:
        c["ref"][k] = smoothed_ce(c["sc_np"], c["caps_np"], DECODE_LEN, PAD, float(np.float32(eps)),
                                  np.array(WEIGHTS) if weighted else None)
    return c["ref"][k]


SHAPES = [(52, 52),             # register path, most lanes empty
          (10240, 10240),       # register path full
          (10244, 10244),       # first long vector row
          (1027, 1028),         # vector bulk plus 3-column tail
          (1027, 1027),         # scalar path
          (50071, 50072)]       # knowledge size


@pytest.mark.parametrize("eps", [0.1, 0.9])
@pytest.mark.parametrize("form", ["plain", "weighted", "packed", "packed_weighted"])
@pytest.mark.parametrize("Vx,ld", SHAPES)
def test_smoothed_ce_kernel_matches_restatement(Vx, ld, form, eps):
    """Bounds: those tests/test_scst_gpu.py holds the weighted kernel to (loss 1e-5 * max(1, |ref|) * count, gradient
    3e-6); every written gradient row sums to w * (1 - (1 - eps) - eps) = 0 within Vx * 1e-7 * |w|."""
    c = kernel_case(Vx, ld)
    weighted, packed = form.endswith("weighted"), form.startswith("packed")
    w = c["w"] if weighted else None
    loss_ref, n_ref, d_ref = reference(c, eps, weighted)
    if packed:
        ls, cnt, dsc = ops.packed_ce_smooth(c["sp"], c["caps"], c["pack"], PAD, word(eps), weights=w, want_grad=True)
        got = dsc.reshape(B * LC, Vx)[:c["Mp"]].cpu().double().numpy()
        d_ref = d_ref.reshape(B * LC, Vx)[c["idx"].cpu().numpy()]
        row_w = np.array(WEIGHTS)[c["idx"].cpu().numpy() // LC] if weighted else np.ones(c["Mp"])
    else:
        ls, cnt, dsc = ops.packed_ce_smooth(c["sc"], c["caps"], c["dl"], PAD, word(eps), weights=w, want_grad=True)
        got = dsc.cpu().double().numpy()
        assert not got[~c["keep"]].any()                   # rows that do not contribute are zero
        got, d_ref = got.reshape(B * LC, Vx), d_ref.reshape(B * LC, Vx)
        row_w = np.repeat(np.array(WEIGHTS) if weighted else np.ones(B), LC)
    loss_err, grad_err = abs(ls.item() - loss_ref), np.abs(got - d_ref).max()
    row_sum = np.abs(got.sum(-1))
    print("Vx %d ld %d %s eps %g: loss %.9g ref %.9g |err| %.3g, gradient max |err| %.3g, worst row sum / bound %.3g"
          % (Vx, ld, form, eps, ls.item(), loss_ref, loss_err, grad_err,
             (row_sum[row_w != 0] / (Vx * 1e-7 * np.abs(row_w[row_w != 0]))).max()))
    assert cnt.item() == n_ref == sum(DECODE_LEN) - 1      # exact; the <pad> target does not count
    assert loss_err < 1e-5 * max(1.0, abs(loss_ref)) * n_ref
    assert grad_err < 3e-6, grad_err
    assert (row_sum <= Vx * 1e-7 * np.abs(row_w)).all()
    if weighted:
        assert not got[row_w == 0].any() and (row_w == 0).sum() >= 3       # a zero weight: zero rows


@pytest.mark.parametrize("Vx,ld", SHAPES)
def test_smoothed_ce_with_zero_eps_has_the_plain_bits_and_packed_rows_equal_unpacked(Vx, ld):
    c = kernel_case(Vx, ld)
    sc, sp, caps, dl, pack, w, Mp, idx = (c[k] for k in ("sc", "sp", "caps", "dl", "pack", "w", "Mp", "idx"))
    zero = word(0.0)
    for got, ref, rows in [
            (ops.packed_ce_smooth(sc, caps, dl, PAD, zero, want_grad=True), ops.packed_ce(sc, caps, dl, PAD, want_grad=True),
             B * LC),
            (ops.packed_ce_smooth(sc, caps, dl, PAD, zero, weights=w, want_grad=True),
             ops.packed_ce_weighted(sc, caps, dl, w, PAD, want_grad=True), B * LC),
            (ops.packed_ce_smooth(sp, caps, pack, PAD, zero, want_grad=True),
             ops.packed_ce_rows(sp, caps, pack, PAD, want_grad=True), Mp),
            (ops.packed_ce_smooth(sp, caps, pack, PAD, zero, weights=w, want_grad=True),
             ops.packed_ce_rows(sp, caps, pack, PAD, weights=w, want_grad=True), Mp)]:
        assert same_bits(got[0], ref[0]) and same_bits(got[1], ref[1])
        assert same_bits(got[2].reshape(B * LC, Vx)[:rows], ref[2].reshape(B * LC, Vx)[:rows])
    # the packed and the unpacked smoothed forms: the same gradient bits row for row, the same token count
    for weights in (None, w):
        su, cu, du = ops.packed_ce_smooth(sc, caps, dl, PAD, word(0.1), weights=weights, want_grad=True)
        s1, c1, d1 = ops.packed_ce_smooth(sp, caps, pack, PAD, word(0.1), weights=weights, want_grad=True)
        assert c1.item() == cu.item() == Mp - 1
        assert same_bits(d1.reshape(B * LC, Vx)[:Mp], du.reshape(B * LC, Vx)[idx])
        # the row losses are the same numbers, summed in another order
        assert abs(s1.item() - su.item()) <= 2.0 ** -20 * Mp * max(1.0, abs(su.item()) / Mp)


def test_smoothed_ce_packed_rows_past_the_count_keep_their_sentinel():
    """The C entry with buffers of the test's own: nothing at or past the device row count is written."""
    import ick_amd.lib as L
    Vx, ld = 1027, 1028
    c = kernel_case(Vx, ld)
    dsc = torch.full((B * LC, ld), SENTINEL, device="cuda")
    row_loss = torch.full((B * LC,), SENTINEL, device="cuda")
    out = torch.zeros(2, device="cuda")
    eps, stream = word(0.1), torch.cuda.current_stream().cuda_stream
    L.check(L.load().ick_packed_ce_smooth(c["sp"].data_ptr(), ld, c["caps"].data_ptr(), c["pack"].rowmap.data_ptr(),
                                          c["pack"].count.data_ptr(), None, c["w"].data_ptr(), eps.data_ptr(), B, LC, Vx,
                                          PAD, row_loss.data_ptr(), out[0:1].data_ptr(), out[1:2].data_ptr(),
                                          dsc.data_ptr(), stream), "ick_packed_ce_smooth")
    torch.cuda.synchronize()
    Mp = c["Mp"]
    assert (dsc[Mp:] == SENTINEL).all() and (row_loss[Mp:] == SENTINEL).all()
    assert (dsc[:Mp, Vx:] == SENTINEL).all()                       # nor the padding columns of a written row
    assert not (dsc[:Mp, :Vx] == SENTINEL).any() and out[1].item() == Mp - 1
    _, _, ref = ops.packed_ce_smooth(c["sp"], c["caps"], c["pack"], PAD, eps, weights=c["w"], want_grad=True)
    assert same_bits(dsc[:Mp, :Vx], ref.reshape(B * LC, Vx)[:Mp])


def test_smoothed_ce_wrapper_refuses_a_host_eps():
    c = kernel_case(52, 52)
    for bad in (0.1, torch.tensor([0.1]), torch.zeros(2, device="cuda"), torch.zeros(1, device="cuda", dtype=torch.float64)):
        with pytest.raises(IckError):
            ops.packed_ce_smooth(c["sc"], c["caps"], c["dl"], PAD, bad)


# ------------------------------------------------------------------------------------------------ one step vs the oracle
STEP_CASES = {"geo": ("geo", 40, 0),              # V + K = 45: padded row stride, vector bulk plus a scalar tail
              "knowledge": ("knowledge", 40, 4),  # V + K + F = 49
              "geo_aligned": ("geo", 43, 0)}      # V + K = 48, a multiple of 4: the in-register path inside the step
STEP_WEIGHTS = [0.8, -1.3, 0.0, 2.1]
_ORACLE = {}


def step_case(name):
    variant, V, Fn = STEP_CASES[name]
    Bs, L, K, seed = 4, 8, 5, 17
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    batch = synth.make_batch(variant, Bs, L, K, V, Fn, seed)
    return variant, V, P, cfg, batch, synth.make_enc_out(Bs, seed)


def oracle_smoothed_step(name, eps, weights, lr=4e-4, clip=5.0):
    """reference_train_step of tests/test_bench_sizes_gpu.py with the smoothed loss: R.forward's scores, torch's
    cross_entropy(label_smoothing=eps) per row (weighted by its caption, over the unweighted token count), autograd,
    clamp, Adam.  -> (loss, gradients, parameters after the step)."""
    key = (name, eps, weights is not None)
    if key not in _ORACLE:
        _ORACLE.clear()
        variant, V, P, cfg, batch, enc_out = step_case(name)
        Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
        if cfg.has_facts:
            Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
        uniq = [v for k, v in Pr.items() if not k.startswith("fact_encoder.")]
        opt = torch.optim.Adam(uniq, lr=lr)
        st = {}
        scores, caps_s, dl = R.forward(cfg, Pr, batch["captions"], enc_out, batch["caption_masks"],
                                       batch["caption_lengths"], batch["entities"], batch.get("facts"), stages=st)
        Lc = caps_s.shape[1]
        tg = caps_s[:, 1:]
        keep = (torch.arange(Lc - 1).view(1, -1) < torch.tensor(dl).view(-1, 1)) & (tg != cfg.pad)
        if weights is None:
            loss = F.cross_entropy(scores[:, :Lc - 1][keep], tg[keep], label_smoothing=eps)
        else:
            ce = F.cross_entropy(scores[:, :Lc - 1].reshape(-1, scores.shape[2]), tg.reshape(-1), reduction="none",
                                 label_smoothing=eps)
            ws = torch.tensor(weights)[st["sort_ind"]]
            loss = (ce.view(tg.shape) * keep * ws.view(-1, 1)).sum() / keep.sum()
        loss.backward()
        grads = {k: v.grad.clone() for k, v in Pr.items() if not k.startswith("fact_encoder.")}
        for p in uniq:
            p.grad.clamp_(-clip, clip)
        opt.step()
        _ORACLE[key] = (loss.item(), grads, {k: v.detach() for k, v in Pr.items()})
    return _ORACLE[key]


def step_args(variant, batch, enc_out):
    return [batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
            batch["entities"]] + ([batch["facts"].cuda()] if variant != "geo" else [])


def compare_with_oracle(ts, dec, loss, loss_ref, grads_ref):
    """The loss and gradient tolerances of run_train_step_vs_oracle (tests/test_bench_sizes_gpu.py), its allowance for
    a ReLU input that rounds to the other side of zero included."""
    assert abs(loss - loss_ref) < 2e-5, (loss, loss_ref)
    named = dict(dec.named_parameters())
    flipped = {}
    for k, gr in grads_ref.items():
        mine = ts.grads[id(named[k])].detach().cpu()
        gr = gr.clamp(-5.0, 5.0)
        d = (mine - gr).abs()
        scale = max(1e-3, gr.abs().max().item())
        if d.max().item() / scale >= 2e-3 and k.endswith(("linear1.weight", "linear1.bias")):
            rows = d.view(d.shape[0], -1).max(dim=1).values
            bad = rows.topk(2).indices[rows.topk(2).values / scale >= 2e-3]
            flipped[k] = bad
            d = d.clone()
            d[bad] = 0
            assert (mine - gr).double().norm().item() <= 5e-3 * gr.double().norm().item(), ("gradient norm", k)
        err = d.max().item() / scale
        assert err < 2e-3, ("gradient", k, err)
    assert len(flipped) <= 2, flipped


STEP_PARAMS = [(n, False) for n in STEP_CASES] + [("knowledge", True)]


@pytest.mark.parametrize("head", ["packed_head", "no_packed_head"])
@pytest.mark.parametrize("name,weighted", STEP_PARAMS, ids=["%s%s" % (n, "_weighted" if w else "") for n, w in STEP_PARAMS])
def test_smoothed_train_step_matches_oracle(name, weighted, head, gemm_split, monkeypatch):
    if head == "no_packed_head":
        monkeypatch.setenv("ICK_NO_PACKED_HEAD", "1")
    eps = 0.1
    variant, V, P, cfg, batch, enc_out = step_case(name)
    loss_ref, grads_ref, _ = oracle_smoothed_step(name, eps, STEP_WEIGHTS if weighted else None)
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, label_smoothing=eps)
    assert ts.packed_head == (head == "packed_head")
    kw = dict(caption_weights=torch.tensor(STEP_WEIGHTS).cuda()) if weighted else {}
    loss = ts(*step_args(variant, batch, enc_out), **kw)
    assert ts.use_graph, "hipGraph capture failed: the captured step was not exercised"
    compare_with_oracle(ts, dec, loss.item(), loss_ref, grads_ref)


# ------------------------------------------------------------------------------------------------ TrainStep behaviour
@pytest.fixture()
def det_off_after():
    yield
    ops.set_deterministic(False)


def run_steps(name, nsteps, deterministic=True, use_graph=True, dropout=True, **kw):
    variant, V, P, cfg, batch, enc_out = step_case(name)
    dec = build_decoder(variant, V, P).train()
    if not dropout:
        zero_dropout(dec)
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0, seed=11, deterministic=deterministic, use_graph=use_graph, **kw)
    args = step_args(variant, batch, enc_out)
    losses = [ts(*args).clone() for _ in range(nsteps)]
    return ts, dec, args, losses


def test_zero_label_smoothing_is_todays_step(det_off_after):
    """TrainStep(dec) and TrainStep(dec, label_smoothing=0.0): the same launches, so (deterministic mode) the same bits."""
    ts0, _, _, l0 = run_steps("knowledge", 2)
    ts1, _, _, l1 = run_steps("knowledge", 2, label_smoothing=0.0)
    assert ts1._eps_word is None and list(ts0._graphs) == list(ts1._graphs)
    assert all(same_bits(a, b) for a, b in zip(l0, l1))
    assert same_bits(ts0.flat_p, ts1.flat_p) and same_bits(ts0.flat_g, ts1.flat_g)
    assert "label_smoothing" not in ts0.state_dict() and set(ts0.state_dict()) == set(ts1.state_dict())


def test_label_smoothing_changes_the_loss_as_the_restatement_predicts():
    name = "knowledge"
    variant, V, P, cfg, batch, enc_out = step_case(name)
    dec = zero_dropout(build_decoder(variant, V, P).train())
    caps, masks, lengths = batch["captions"].cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda()
    enc, ents, facts = dec._prepare_inputs(enc_out.cuda(), batch["entities"], batch["facts"].cuda())
    with torch.no_grad():
        scores, _ = forward_with_tape(dec, caps, masks, ents, facts, dec._token_major(enc).contiguous(), None)
    dl = (batch["caption_lengths"].view(-1) - 1).numpy()
    pred = {}
    for eps in (0.0, 0.1):
        s, n, _ = smoothed_ce(scores.cpu().numpy(), batch["captions"].numpy(), dl, cfg.pad, float(np.float32(eps)))
        pred[eps] = s / n
    del dec
    got = {eps: run_steps(name, 1, deterministic=None, dropout=False, label_smoothing=eps)[3][0].item()
           for eps in (0.0, 0.1)}
    print("loss at eps 0 / 0.1: step %.7f / %.7f, restatement %.7f / %.7f" % (got[0.0], got[0.1], pred[0.0], pred[0.1]))
    assert abs(pred[0.1] - pred[0.0]) > 10 * 2e-5                      # the value matters: ten times the tolerance below
    for eps in (0.0, 0.1):
        assert abs(got[eps] - pred[eps]) < 2e-5                        # (the loss tolerance of the oracle tests)
    assert abs((got[0.1] - got[0.0]) - (pred[0.1] - pred[0.0])) < 2e-5


def test_label_smoothing_bad_values():
    variant, V, P, cfg, batch, enc_out = step_case("geo")
    dec = build_decoder(variant, V, P).train()
    for bad in (-0.1, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(IckError):
            TrainStep(dec, label_smoothing=bad)
    ts = TrainStep(dec, label_smoothing=0.1)
    for bad in (-1e-9, 1.0, float("nan")):
        with pytest.raises(IckError):
            ts.set_label_smoothing(bad)
    assert ts.label_smoothing == 0.1 and ts._eps_word.item() == np.float32(0.1)


def _count_captures(ts):
    calls = []
    for name in ("_capture", "_capture_split"):
        fn = getattr(ts, name)
        setattr(ts, name, lambda *a, _fn=fn, **k: (calls.append(1), _fn(*a, **k))[1])
    return calls


def test_set_label_smoothing_replays_and_equals_a_fresh_step(det_off_after):
    """After a step at 0.1, set_label_smoothing(0.2) adds no graph and captures nothing, and (deterministic mode) the next
    step is, bit for bit, that of a fresh TrainStep(label_smoothing=0.2) started from the same parameters, moments and
    step count.  Moving to zero captures once for the plain kind, and moving back replays."""
    name = "geo"
    ts, dec, args, (l1,) = run_steps(name, 1, label_smoothing=0.1)
    graphs = dict(ts._graphs)
    assert len(graphs) == 1 and "label_smoothing" in next(iter(graphs))
    snap = {k: v.detach().clone() for k, v in dec.state_dict().items() if k != "pos_encoder.pe"}
    state = ts.state_dict()
    calls = _count_captures(ts)
    ts.set_label_smoothing(0.2)
    l2 = ts(*args).clone()
    assert ts._graphs == graphs and not calls
    assert ts._eps_word.item() == np.float32(0.2) and not same_bits(l1, l2)
    p2, g2 = ts.flat_p.clone(), ts.flat_g.clone()
    fresh_dec = build_decoder(STEP_CASES[name][0], STEP_CASES[name][1], snap).train()
    fresh = TrainStep(fresh_dec, lr=4e-4, grad_clip=5.0, seed=11, deterministic=True, label_smoothing=0.2)
    fresh.load_state_dict(state)
    lf = fresh(*args)
    assert same_bits(lf, l2) and same_bits(fresh.flat_g, g2) and same_bits(fresh.flat_p, p2)
    # zero <-> non-zero: one capture for the new kind, the graphs of the other kind are kept
    ts.set_label_smoothing(0.0)
    ts(*args)
    assert len(calls) == 2 and len(ts._graphs) == 2                    # (two captures: graph A and graph B of the plain step)
    ts.set_label_smoothing(0.3)
    ts(*args)
    assert len(calls) == 2 and len(ts._graphs) == 2 and ts._eps_word.item() == np.float32(0.3)


def test_smoothed_steps_are_bit_reproducible_and_eager_equals_captured(det_off_after):
    runs = [run_steps("knowledge", 3, label_smoothing=0.1) for _ in range(2)]
    (ts0, _, _, l0), (ts1, _, _, l1) = runs
    assert all(same_bits(a, b) for a, b in zip(l0, l1))
    assert same_bits(ts0.flat_g, ts1.flat_g) and same_bits(ts0.flat_p, ts1.flat_p)
    ts2, _, _, l2 = run_steps("knowledge", 3, use_graph=False, label_smoothing=0.1)
    assert not ts2._graphs
    assert all(same_bits(a, b) for a, b in zip(l0, l2))
    assert same_bits(ts0.flat_g, ts2.flat_g) and same_bits(ts0.flat_p, ts2.flat_p)


# ------------------------------------------------------------------------------------------------ the training script
def test_train_main_with_label_smoothing(tmp_path):
    """Fused run, two batches per epoch: the (smoothed) training loss is finite and falls; the reported validation loss
    is the PLAIN loss of the same validation batches, as score_captions computes it from the epoch's checkpoint."""
    from ick_amd import train as tr, utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    cfg = tr.Config(variant="geo", data_dir=data_dir, data_name="toy", epochs=3, batch_size=8, workers=0, print_freq=1000,
                    fused=True, out_dir=str(tmp_path), label_smoothing=0.1, max_batches=2)
    torch.manual_seed(0)
    hist = tr.main(cfg)
    assert len(hist) == 3 and all(math.isfinite(h[0]) and math.isfinite(h[1]) for h in hist)
    assert hist[-1][0] < hist[0][0]                                    # training loss goes down
    ck = ut.load_checkpoint(str(tmp_path / "checkpoint_2_toy.pth.tar"), map_location="cuda")
    dec, enc = ck["decoder"].cuda().eval(), ck["encoder"].cuda().eval()
    loaders, _, _ = tr.make_loaders(cfg, 0, 1, True)
    tot = torch.zeros(2, dtype=torch.float64, device="cuda")
    smooth_sum = 0.0
    with torch.no_grad():
        for i, batch in enumerate(loaders["VAL"]):
            imgs, caps, caplens, capmasks, ent, facts = tr._batch_to_device(batch, "cuda", False)
            s = dec.score_captions(caps, enc(imgs), capmasks, caplens, ent, facts, top_k=5)
            tot += torch.cat([s.loss_sum, s.count]).double()
            scores, caps_sorted, dl = dec(caps, enc(imgs), capmasks, caplens, ent)
            smooth_sum += tr.packed_loss(tr.make_criteria(0, 0.1)[0], scores, caps_sorted, dl).item() * sum(dl)
            if i + 1 >= cfg.max_batches:
                break
    plain = (tot[0] / tot[1]).item()
    print("validation loss reported %.7f, plain %.7f, smoothed %.7f" % (hist[-1][1], plain, smooth_sum / tot[1].item()))
    assert abs(hist[-1][1] - plain) < 2e-5 * max(1.0, plain)
    assert abs(smooth_sum / tot[1].item() - plain) > 1e-3              # ... and not the smoothed one
    assert ck["loss"] == hist[-1][1]
