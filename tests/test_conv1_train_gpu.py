"""Encoder.conv1's weight gradient straight from the NCHW feature map (ick_conv1_wgrad, csrc/conv1_bwd.hip; DESIGN.md
3.1i) against a float64 einsum on the host:
    dW[o, c] = sum_{b, p} d_img[b, p, o] * feats[b, c, p],     db[o] = sum_{b, p} d_img[b, p, o]."""
import contextlib

import pytest
import torch

import ick_amd.lib as L
import ick_amd.ops as ops
import ick_amd.synth as synth
from test_ops_gpu import close, rnd

pytestmark = pytest.mark.gpu

# (B, C, P, d): one element; P = 1; P = 9 (36-byte feats rows: no 16-byte loads) with two row blocks' worth of d on the
# scalar feats path; the workload's shape at three samples; a tail in the column tiles (260 = 4 * 64 + 4) with odd P;
# d = 512 (two row blocks); everything odd
INT_SHAPES = [(1, 1, 1, 1), (1, 8, 1, 4), (2, 100, 9, 300), (3, 2048, 196, 300), (5, 260, 49, 64), (2, 2048, 196, 512),
              (7, 33, 5, 17)]


@contextlib.contextmanager
def deterministic(on):
    before = L.load().ick_get_deterministic()
    ops.set_deterministic(on)
    try:
        yield
    finally:
        ops.set_deterministic(bool(before))


def reference(d_img, feats):
    """float64 on the host: (dW (d, C), db (d,))."""
    B, P, d = d_img.shape
    a = d_img.double().reshape(B * P, d)
    x = feats.double().reshape(B, feats.shape[1], P).permute(0, 2, 1).reshape(B * P, -1)
    return a.t() @ x, a.sum(0)


def int_operands(B, C, P, d, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-4, 5, (B, P, d), generator=g).float(), torch.randint(-4, 5, (B, C, P), generator=g).float())


def run(d_img, feats, fill=float("nan")):
    """The entry writes its whole output whatever it held before: the outputs start as NaN."""
    d, C = d_img.shape[2], feats.shape[1]
    dw = torch.full((d, C), fill, device="cuda")
    db = torch.full((d,), fill, device="cuda")
    ops.conv1_wgrad(d_img.cuda(), feats.cuda(), dw, db)
    return dw.cpu(), db.cpu()


@pytest.mark.parametrize("det", [False, True], ids=["atomics_allowed", "deterministic"])
@pytest.mark.parametrize("shape", INT_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_integer_operands_are_exact(shape, det, gemm_split):
    """Values in [-4, 4]: every product and every partial sum is an integer below 2^24, so any order of additions and any
    exact bf16 split gives the float64 result bit for bit."""
    d_img, feats = int_operands(*shape, seed=sum(shape))
    rw, rb = reference(d_img, feats)
    with deterministic(det):
        dw, db = run(d_img, feats)
    assert torch.equal(dw.double(), rw), (dw.double() - rw).abs().max().item()
    assert torch.equal(db.double(), rb), (db.double() - rb).abs().max().item()


@pytest.fixture(scope="module")
def normal_b64():
    """The workload's shape: operands and the float64 result, made once."""
    feats = synth.make_feats(64, 3).view(64, 2048, 196)
    d_img = rnd(64, 196, 300, seed=11)
    return d_img, feats, reference(d_img, feats)


def test_normal_data_b3(gemm_split):
    feats = synth.make_feats(3, 4).view(3, 2048, 196)
    d_img = rnd(3, 196, 300, seed=9)
    rw, rb = reference(d_img, feats)
    dw, db = run(d_img, feats)
    close(dw, rw, 2e-5, "conv1 dW")
    close(db, rb, 2e-5, "conv1 db")


def test_normal_data_b64(normal_b64, gemm_split):
    d_img, feats, (rw, rb) = normal_b64
    dw, db = run(d_img, feats)
    close(dw, rw, 2e-5, "conv1 dW")
    close(db, rb, 2e-5, "conv1 db")


def test_four_dimensional_map_and_conv_weight_views():
    """feats as the (B, C, H, W) map and dW as conv1's (d, C, 1, 1) weight: the same memory, the same result."""
    d_img, feats = int_operands(2, 40, 16, 24, seed=5)
    rw, rb = reference(d_img, feats)
    dw = torch.full((24, 40, 1, 1), float("nan"), device="cuda")
    db = torch.full((24,), float("nan"), device="cuda")
    ops.conv1_wgrad(d_img.cuda(), feats.view(2, 40, 4, 4).cuda(), dw, db)
    assert torch.equal(dw.cpu().view(24, 40).double(), rw) and torch.equal(db.cpu().double(), rb)


@pytest.mark.parametrize("which", ["first", "last"])
def test_samples_are_paired(which):
    """d_img zero except for one sample: dW is that sample's term alone (a kernel that paired d_img of sample b with feats
    of another sample, or lost the jump between samples, shows here)."""
    B, C, P, d = 5, 130, 49, 40
    d_img, feats = int_operands(B, C, P, d, seed=21)
    b = 0 if which == "first" else B - 1
    only = torch.zeros_like(d_img)
    only[b] = d_img[b]
    dw, db = run(only, feats)
    rw, rb = reference(d_img[b:b + 1], feats[b:b + 1])
    assert torch.equal(dw.double(), rw) and torch.equal(db.double(), rb)


def test_same_bits_twice_in_deterministic_mode():
    feats = synth.make_feats(6, 8).view(6, 2048, 196)
    d_img = rnd(6, 196, 300, seed=13)
    with deterministic(True):
        a = run(d_img, feats)
        b = run(d_img, feats, fill=0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_scratch_is_checked_and_reused():
    d_img, feats = int_operands(3, 70, 12, 20, seed=2)
    rw, rb = reference(d_img, feats)
    need = ops.conv1_wgrad_plan(3, 70, 12, 20)[1]
    dw, db = torch.empty(20, 70, device="cuda"), torch.empty(20, device="cuda")
    scratch = torch.full((need,), float("nan"), device="cuda")
    ops.conv1_wgrad(d_img.cuda(), feats.cuda(), dw, db, scratch=scratch)
    assert torch.equal(dw.cpu().double(), rw) and torch.equal(db.cpu().double(), rb)
    with pytest.raises(L.IckError):
        ops.conv1_wgrad(d_img.cuda(), feats.cuda(), dw, db, scratch=scratch[:need - 1])
    with pytest.raises(L.IckError):
        ops.conv1_wgrad(d_img.cuda(), feats[:, :, :11].contiguous().cuda(), dw, db)


def test_einval_leaves_the_outputs_untouched():
    B, C, P, d = 2, 16, 8, 12
    d_img, feats = (x.cuda() for x in int_operands(B, C, P, d, seed=1))
    dw = torch.full((d, C), 7.0, device="cuda")
    db = torch.full((d,), 7.0, device="cuda")
    scratch = torch.empty(ops.conv1_wgrad_plan(B, C, P, d)[1], device="cuda")
    lib = L.load()
    ptr = dict(d_img=d_img.data_ptr(), feats=feats.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr(),
               scratch=scratch.data_ptr())
    size = dict(B=B, C=C, P=P, d=d)

    def call(**over):
        a = {**ptr, **size, **over}
        return lib.ick_conv1_wgrad(a["d_img"], a["feats"], a["dw"], a["db"], a["B"], a["C"], a["P"], a["d"], a["scratch"],
                                   over.get("scratch_floats", scratch.numel()), None)

    for name in ptr:
        assert call(**{name: None}) == -1, name
    for name in size:
        for bad in (0, -3):
            assert call(**{name: bad}) == -1, (name, bad)
    assert call(scratch_floats=scratch.numel() - 1) == -1
    torch.cuda.synchronize()
    assert bool((dw == 7.0).all()) and bool((db == 7.0).all())
    assert call() == 0
    torch.cuda.synchronize()
    rw, rb = reference(d_img.cpu(), feats.cpu())
    assert torch.equal(dw.cpu().double(), rw) and torch.equal(db.cpu().double(), rb)


# ------------------------------------------------------------------------------------------------------------------
# TrainStep(..., encoder=enc, train_conv1=True): Encoder.conv1 trained inside the fused step against the
# reference sequence on the oracle with conv1's weight and bias requiring grad through R.feat_proj
# (geo-aware/train.py:269-294 with fine_tune_encoder=True on a feature-file encoder).
# ------------------------------------------------------------------------------------------------------------------
import copy  # noqa: E402

import ick_amd  # noqa: E402
from helpers import case_from_golden, load_golden  # noqa: E402
from oracle import restatement as R  # noqa: E402
from test_bench_sizes_gpu import make_encoder  # noqa: E402
from test_forward_gpu import build_decoder  # noqa: E402
from test_training_gpu import zero_dropout  # noqa: E402

LR, ENC_LR, CLIP = 4e-4, 1e-4, 5.0
_ORACLE = {}


def oracle_steps(key, cfg, P, batch, feats, cw, cb, steps, lr=LR, enc_lr=ENC_LR):
    """`steps` optimizer steps of the reference sequence on the CPU oracle, conv1 trainable with an Adam of its own.
    Returns the first step's loss and gradients (conv1's under "conv1.weight" / "conv1.bias") and, after the last step, the
    parameters and both torch optimizers.  Computed once per case."""
    if key in _ORACLE:
        return _ORACLE[key]
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
    if cfg.has_facts:
        Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
    names = [k for k in Pr if not k.startswith("fact_encoder.")]
    conv = {"conv1.weight": cw.clone().requires_grad_(True), "conv1.bias": cb.clone().requires_grad_(True)}
    opt = torch.optim.Adam([Pr[k] for k in names], lr=lr)
    eopt = torch.optim.Adam(list(conv.values()), lr=enc_lr)
    out = {}
    for s in range(steps):
        opt.zero_grad()
        eopt.zero_grad()
        enc_out = R.feat_proj(feats, conv["conv1.weight"], conv["conv1.bias"])
        scores, caps, dl = R.forward(cfg, Pr, batch["captions"], enc_out, batch["caption_masks"],
                                     batch["caption_lengths"], batch["entities"], batch.get("facts"))
        loss = R.packed_ce_loss(cfg, scores, caps, dl)
        loss.backward()
        if s == 0:
            out["loss"] = loss.item()
            out["grads"] = {k: Pr[k].grad.clone() for k in names}
            out["grads"].update({k: v.grad.clone() for k, v in conv.items()})
        for p in list(conv.values()) + [Pr[k] for k in names]:
            p.grad.clamp_(-CLIP, CLIP)
        opt.step()
        eopt.step()
    out.update(names=names, params=Pr, conv=conv, opt=opt, eopt=eopt)
    _ORACLE.clear()                     # one case at a time
    _ORACLE[key] = out
    return out


def small_case(variant, B, seed=31, L=9, K=6, V=200):
    Fn = 0 if variant == "geo" else 5
    P = synth.make_params(variant, V, seed)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    feats = synth.make_feats(B, seed)
    cw, cb = synth.make_conv1(seed)
    return cfg, P, batch, feats, cw, cb


def step_args(batch, feats):
    args = [batch["captions"].cuda(), feats.cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
            batch["entities"]]
    if "facts" in batch:
        args.append(batch["facts"].cuda())
    return args


def build_step(cfg, P, seed, **kw):
    from ick_amd.training import TrainStep
    enc, _, _ = make_encoder(seed)
    dec = zero_dropout(build_decoder(cfg.variant, cfg.vocab_size, P).train())
    kw.setdefault("lr", LR)
    kw.setdefault("encoder_lr", ENC_LR)
    return TrainStep(dec, grad_clip=CLIP, encoder=enc, train_conv1=True, **kw), dec, enc


def my_grads(ts, dec):
    named = dict(dec.named_parameters())
    g = {k: ts.grads[id(p)] for k, p in named.items() if id(p) in ts.grads}
    g["conv1.weight"], g["conv1.bias"] = ts._c1_gw, ts._c1_gb
    return g


def check_gradients(ts, dec, grads_ref, what=""):
    """The bucket after an applied update holds what Adam consumed: the token-mean gradient clamped to +-5.  The bound and
    the ReLU-flip allowance (at most two hidden units of a linear1, in at most two tensors) are those of
    test_bench_train_step_from_features_b64_vs_digest_and_oracle."""
    mine_all = my_grads(ts, dec)
    flipped, worst = 0, (0.0, None)
    for k, gr in grads_ref.items():
        mine = mine_all[k].detach().cpu().view(gr.shape)
        gr = gr.clamp(-CLIP, CLIP)
        d = (mine - gr).abs()
        scale = max(1e-3, gr.abs().max().item())
        if d.max().item() / scale >= 2e-3 and k.endswith(("linear1.weight", "linear1.bias")):
            rows = d.view(d.shape[0], -1).max(dim=1).values
            bad = rows.topk(2).indices[rows.topk(2).values / scale >= 2e-3]
            d = d.clone()
            d[bad] = 0
            flipped += 1
        worst = max(worst, (d.max().item() / scale, k))
        assert d.max().item() / scale < 2e-3, (what, "gradient", k, d.max().item() / scale)
    assert flipped <= 2
    print("%s worst gradient error / max: %.3e (%s)" % (what, worst[0], worst[1]))
    return flipped


@pytest.mark.parametrize("variant,B", [("geo", 5), ("geo", 8), ("knowledge", 5), ("knowledge", 8)])
def test_step_vs_oracle_three_steps(variant, B):
    """Loss and every gradient of step 1, then parameters and both sets of moments after three steps (decoder lr 4e-4,
    encoder lr 1e-4) against torch Adam on the oracle; no re-capture over five steps.

    Tolerances after three steps, from run_train_step_vs_oracle's for one step (P_after: any element within 8.5e-4 = about
    two decoder steps of lr, well-conditioned elements within 5e-5): an element moves by at most about lr per step, so
    three steps triple both bounds, and conv1's scale with its rate (1e-4 / 4e-4).  Well-conditioned = the oracle's first
    gradient is at least 1e-6 and ours is within 5 % of it, as there; at least 98 % of the elements that large must be.
    Moments: exp_avg within 2e-3 of its max (the gradients' bound; it is a mix of three gradients), exp_avg_sq within
    4e-3 of its max (squares double a relative error).  The ReLU-flip allowance of the gradient check (at most two hidden
    units of a linear1, in at most two tensors of the test) also covers a flip in step 2 or 3, which only the parameters
    and moments show: those units' rows are set aside in both."""
    cfg, P, batch, feats, cw, cb = small_case(variant, B)
    ref = oracle_steps((variant, B), cfg, P, batch, feats, cw, cb, steps=3)
    ts, dec, enc = build_step(cfg, P, 31)
    args = step_args(batch, feats)
    loss = ts(*args)
    assert ts.use_graph and len(ts._graphs) == 1
    assert abs(loss.item() - ref["loss"]) < 2e-5, (loss.item(), ref["loss"])
    flipped = check_gradients(ts, dec, ref["grads"], "%s B=%d" % (variant, B))
    g1 = {k: v.detach().cpu().clone() for k, v in my_grads(ts, dec).items()}
    graph = next(iter(ts._graphs.values()))[0]
    ts(*args)
    ts(*args)
    named = dict(dec.named_parameters())
    named.update({"conv1.weight": enc.conv1.weight, "conv1.bias": enc.conv1.bias})
    sd, esd = ts.state_dict(), ts.encoder_state_dict()
    order = {id(p): i for i, p in enumerate(ts._adam_order())}
    tsd = ts.as_torch_encoder_optimizer().state_dict()
    assert tsd["param_groups"][0]["lr"] == ENC_LR and tsd["param_groups"][0]["params"] == [0, 1]
    worst, units = {}, {}
    for k in ref["names"] + ["conv1.weight", "conv1.bias"]:
        is_conv = k.startswith("conv1.")
        pr = (ref["conv"] if is_conv else ref["params"])[k]
        st_ref = (ref["eopt"] if is_conv else ref["opt"]).state[pr]
        st = esd["state"][0 if k == "conv1.weight" else 1] if is_conv else sd["state"][order[id(named[k])]]
        if is_conv:
            tst = tsd["state"][0 if k == "conv1.weight" else 1]
            assert torch.equal(tst["exp_avg"], st["exp_avg"]) and torch.equal(tst["exp_avg_sq"], st["exp_avg_sq"])
        assert float(st["step"]) == float(st_ref["step"]) == 3.0
        rate = (ENC_LR if is_conv else LR) / LR
        diff = (named[k].detach().cpu() - pr.detach()).abs()
        gref = ref["grads"][k].clamp(-CLIP, CLIP)
        big = gref.abs() >= 1e-6
        well = big & ((g1[k].view(gref.shape) - gref).abs() <= 0.05 * gref.abs())
        keep = torch.ones(diff.shape[0], dtype=torch.bool)
        if k.endswith("linear1.bias") and k[:-4] in units:      # the units set aside in this Linear's weight: its bias too
            keep[units[k[:-4]]] = False
            flipped += 1
        if k.endswith(("linear1.weight", "linear1.bias")) and well.any() and \
                (diff * well).max().item() / rate >= 3 * 5e-5:
            # the ReLU-flip allowance, for a flip in step 2 or 3 (the gradients of those steps are not compared one by one):
            # the rows of at most two hidden units of this Linear are set aside, here and in its moments
            rows = (diff * well).view(diff.shape[0], -1).max(dim=1).values
            bad = rows.topk(2).indices[rows.topk(2).values / rate >= 3 * 5e-5]
            flipped += bool(keep.all())
            keep[bad] = False
            units[k.rsplit(".", 1)[0] + "."] = bad
            print("set aside as flipped ReLU units:", k, bad.tolist(), rows[bad].tolist())
        diff, well = diff[keep], well[keep]
        for mk, tol in (("exp_avg", 2e-3), ("exp_avg_sq", 4e-3)):
            mref = st_ref[mk]
            err = (st[mk].cpu() - mref)[keep].abs().max().item() / max(1e-12, mref.abs().max().item())
            worst[mk] = max(worst.get(mk, (0, None)), (err, k))
            assert err < tol, (mk, k, err)
        assert diff.max().item() <= 3 * 8.5e-4 * rate, ("parameter (any element)", k, diff.max().item())
        if big.any():
            assert well.sum().item() >= 0.98 * big[keep].sum().item(), ("too few well-conditioned elements", k)
        if well.any():
            err = diff[well].max().item() / rate
            worst["param"] = max(worst.get("param", (0, None)), (err, k))
            assert err < 3 * 5e-5, ("parameter", k, err)
    assert flipped <= 2, "more than two tensors with flipped ReLU units"
    print("%s B=%d after three steps, worst" % (variant, B), worst)
    ts(*args)
    ts(*args)
    assert len(ts._graphs) == 1 and next(iter(ts._graphs.values()))[0] is graph, "the step was captured again"
    assert int(ts.counter.item()) == 5


def test_step_b64_vs_digest_and_oracle(gemm_split):
    """The bench's own size, where a missing edge between the two streams shows: loss against the real reference's digest,
    every gradient (conv1's included) against the oracle, on the arguments and again on the step's own input buffers."""
    g = load_golden("digest_cfg2_b64")
    cfg, P, wm, batch, _ = case_from_golden(g)
    B, seed = int(g["B"]), int(g["seed"])
    assert B == 64
    cw, cb = synth.make_conv1(seed)
    feats = synth.make_feats(B, seed)
    ref = oracle_steps(("b64", seed), cfg, P, batch, feats, cw, cb, steps=1)
    assert abs(ref["loss"] - float(g["loss"][0])) < 1e-5
    ts, dec, enc = build_step(cfg, P, seed, lr=0.0, encoder_lr=0.0)     # rates 0: two steps see the same weights
    live = step_args(batch, feats)
    for what, args in (("arguments", live), ("in-place input buffers", None)):
        if args is None:
            args = ts.input_buffers()
            ts.flat_g.zero_()
        loss = ts(*args)
        assert ts.use_graph and ts._graphs
        assert abs(loss.item() - float(g["loss"][0])) < 2e-5, (what, loss.item())
        check_gradients(ts, dec, ref["grads"], "B=64 mode %d, %s" % (gemm_split, what))


def test_set_encoder_lr_applies_from_the_next_update():
    cfg, P, batch, feats, cw, cb = small_case("geo", 5)
    ts, dec, enc = build_step(cfg, P, 31, encoder_lr=0.0)
    args = step_args(batch, feats)
    w0 = enc.conv1.weight.detach().clone()
    ts(*args)
    assert torch.equal(enc.conv1.weight.detach(), w0)                   # rate 0: moments move, the weight does not
    ts.set_encoder_lr(1e-4)
    assert ts.encoder_lr == 1e-4
    ts(*args)
    st = ts.encoder_state_dict()["state"][0]
    assert float(st["step"]) == 2.0
    b1, b2 = ts.betas
    m, v = st["exp_avg"].double(), st["exp_avg_sq"].double()
    expect = w0.double() - 1e-4 * (m / (1 - b1 ** 2)) / ((v / (1 - b2 ** 2)).sqrt() + ts.eps)
    err = (enc.conv1.weight.detach().double() - expect).abs().max().item()
    assert err < 2e-7 + 1e-6 * w0.abs().max().item(), err               # run_train_step_vs_oracle's closed-form bound
    assert (enc.conv1.weight.detach() - w0).abs().max().item() > 5e-5


def test_lazy_update_and_flush_match_the_eager_order():
    """Same kernels, but the weight gradients' float atomics are not ordered: the same tolerance as against the oracle."""
    cfg, P, batch, feats, cw, cb = small_case("geo", 8)
    args = step_args(batch, feats)
    res = []
    for lazy in (False, True):
        ts, dec, enc = build_step(cfg, P, 31, lazy_update=lazy)
        for _ in range(3):
            ts(*args)
        if lazy:
            assert ts._pending and ts._lazy_active(args[1]) and int(ts.counter.item()) == 2
        ts.flush()
        assert int(ts.counter.item()) == 3
        res.append((ts.flat_p.clone(), ts.enc_p.clone(), ts.enc_m.clone(), ts.enc_v.clone()))
    (p0, e0, m0, v0), (p1, e1, m1, v1) = res
    assert (p0 - p1).abs().max().item() < 3 * 5e-5 and (e0 - e1).abs().max().item() < 3 * 5e-5 / 4
    assert (m0 - m1).abs().max().item() < 2e-3 * m0.abs().max().item()
    assert (v0 - v1).abs().max().item() < 4e-3 * v0.abs().max().item()
    assert (e0[:cw.numel()].cpu() - cw.reshape(-1)).abs().max().item() > 1e-4          # conv1 did train


def test_presplit_copy_is_fresh_after_steps(gemm_split, monkeypatch):
    """After three steps nothing reads stale planes: enc(feats) and decoder.forward with the encoder attached equal a
    float64 conv2d with the CURRENT weights, and conv1_presplit() finds its copy current (no launch)."""
    cfg, P, batch, feats, cw, cb = small_case("geo", 5)
    ts, dec, enc = build_step(cfg, P, 31, encoder_lr=1e-2)              # a rate at which stale planes would show
    args = step_args(batch, feats)
    w0 = enc.conv1.weight.detach().clone()
    for _ in range(3):
        ts(*args)
    assert (enc.conv1.weight.detach() - w0).abs().max().item() > 1e-3
    calls = []
    real = ops.presplit_weights
    monkeypatch.setattr(ops, "presplit_weights", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ps = enc.conv1_presplit()
    assert (ps is None) == (gemm_split == 0) and not calls
    monkeypatch.undo()
    ref = torch.nn.functional.conv2d(feats.double(), enc.conv1.weight.detach().double().cpu(),
                                     enc.conv1.bias.detach().double().cpu()).view(5, 300, -1)
    with torch.no_grad():
        close(enc(feats.cuda()), ref, 2e-5, "enc(feats) after three steps")
        dec.eval()
        dec.attach_encoder(enc)
        tail = args[2:]
        s_map, _, _ = dec(args[0], feats.cuda(), *tail)
        s_tok, _, _ = dec(args[0], ref.float().cuda(), *tail)
        close(s_map, s_tok.cpu(), 2e-5, "decoder.forward on the feature map after three steps")


def test_encoder_optimizer_save_and_load_continue_bit_for_bit():
    cfg, P, batch, feats, cw, cb = small_case("geo", 5)
    args = step_args(batch, feats)
    with deterministic(True):
        ts, dec, enc = build_step(cfg, P, 31, deterministic=True)
        ts(*args)
        ts(*args)
        saved = dict(dec=copy.deepcopy(dec.state_dict()), enc=copy.deepcopy(enc.state_dict()),
                     opt=ts.as_torch_optimizer().state_dict(), eopt=ts.as_torch_encoder_optimizer().state_dict())
        ts(*args)
        a = (ts.flat_p.clone(), ts.enc_p.clone(), ts.enc_m.clone(), ts.enc_v.clone())
        ts2, dec2, enc2 = build_step(cfg, P, 31, deterministic=True)
        dec2.load_state_dict(saved["dec"])
        enc2.load_state_dict(saved["enc"])
        ts2.load_state_dict(saved["opt"])
        ts2.load_encoder_state_dict(saved["eopt"])
        assert enc2.conv1.weight.data_ptr() == ts2.enc_p.data_ptr()
        ts2(*args)
        b = (ts2.flat_p, ts2.enc_p, ts2.enc_m, ts2.enc_v)
        for x, y, what in zip(a, b, ("decoder", "conv1", "conv1 exp_avg", "conv1 exp_avg_sq")):
            assert torch.equal(x, y), what


def test_refused_combinations():
    from ick_amd.scst import SelfCriticalStep
    from ick_amd.training import TrainStep
    cfg, P, batch, feats, cw, cb = small_case("geo", 5)
    dec = zero_dropout(build_decoder(cfg.variant, cfg.vocab_size, P).train())
    with pytest.raises(L.IckError, match="encoder="):
        TrainStep(dec, train_conv1=True)
    ts, dec, enc = build_step(cfg, P, 31)
    args = step_args(batch, feats)
    tok = enc(feats.cuda()).detach()
    with pytest.raises(L.IckError, match="conv1"):
        ts(args[0], tok, *args[2:])
    with pytest.raises(L.IckError):
        ts(*args, image_index=torch.arange(5))
    with pytest.raises(L.IckError, match="conv1"):
        ts(args[0], tok, *args[2:], image_index=torch.arange(5))
    with pytest.raises(L.IckError, match="train_conv1"):
        SelfCriticalStep(ts, lambda tokens, idx: [0.0] * len(idx))
    with pytest.raises(L.IckError, match="train_conv1"):
        TrainStep(zero_dropout(build_decoder(cfg.variant, cfg.vocab_size, P).train()), encoder=enc).set_encoder_lr(1e-4)


def test_without_the_flag_conv1_is_untouched():
    from ick_amd.training import TrainStep
    cfg, P, batch, feats, cw, cb = small_case("geo", 5)
    enc, _, _ = make_encoder(31)
    dec = zero_dropout(build_decoder(cfg.variant, cfg.vocab_size, P).train())
    ptr, w0, b0 = enc.conv1.weight.data_ptr(), enc.conv1.weight.detach().clone(), enc.conv1.bias.detach().clone()
    ts = TrainStep(dec, lr=LR, grad_clip=CLIP, encoder=enc)
    assert not ts.train_conv1 and ts.ne == 0 and not hasattr(ts, "enc_p") and ts.flat_g.numel() == ts.n + 2
    ts(*step_args(batch, feats))
    ts(*step_args(batch, feats))
    assert enc.conv1.weight.data_ptr() == ptr
    assert torch.equal(enc.conv1.weight.detach(), w0) and torch.equal(enc.conv1.bias.detach(), b0)
    with pytest.raises(L.IckError):
        ts.encoder_state_dict()


# ------------------------------------------------------------------------------------------------------------------
# data parallel: conv1's gradient travels in the one bucket
# ------------------------------------------------------------------------------------------------------------------
DP_CASE = ("geo", 6)


def test_two_ranks_train_conv1(tmp_path):
    """Two gloo ranks on the one GPU, three samples each, two steps in deterministic mode: conv1 (and the decoder) end
    bit-identical on both ranks, although rank 1 started from another conv1.  Against the single-process step on all six
    samples: the first step's conv1 gradient within 2e-6 of its largest element (the bound of
    test_two_shards_equal_full_batch_in_deterministic_mode: what remains is the association of the sample sums), conv1
    after two steps within the three-step test's bounds scaled to two steps."""
    import os
    import socket
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, ICK_DP_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.join(root, "tests", "dp_conv1_worker.py"), str(tmp_path)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-3000:]
    r0, r1 = torch.load(tmp_path / "conv1_rank0.pt"), torch.load(tmp_path / "conv1_rank1.pt")
    assert r0["steps"] == r1["steps"] == 2
    assert torch.equal(r0["enc_p"], r1["enc_p"]) and torch.equal(r0["flat_p"], r1["flat_p"])
    assert torch.equal(r0["g1"], r1["g1"])
    variant, B = DP_CASE
    cfg, P, batch, feats, cw, cb = small_case(variant, B)
    with deterministic(True):
        ts, dec, enc = build_step(cfg, P, 31, deterministic=True)
        args = step_args(batch, feats)
        ts(*args)
        g1 = ts.enc_g.detach().cpu().clone()
        ts(*args)
        full = ts.enc_p.detach().cpu().clone()
    err = (r0["g1"] - g1).abs().max().item()
    print("two ranks against one: conv1 gradient of step 1 differs by %.3e (max |g| %.3e)" % (err, g1.abs().max().item()))
    assert err < 2e-6 * max(1.0, g1.abs().max().item()), err
    diff = (r0["enc_p"] - full).abs() / (ENC_LR / LR)
    well = (g1.abs() >= 1e-6) & ((r0["g1"] - g1).abs() <= 0.05 * g1.abs())
    print("conv1 after two steps: any element %.3e, well-conditioned %.3e" % (diff.max().item(), diff[well].max().item()))
    assert diff.max().item() <= 2 * 8.5e-4 and diff[well].max().item() < 2 * 5e-5
    assert (full[:cw.numel()] - cw.reshape(-1)).abs().max().item() > 1e-4              # conv1 did train


# ------------------------------------------------------------------------------------------------------------------
# train.main(Config(train_conv1=True))
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("prefetch", [True, False], ids=["pipelined_loop", "plain_loop"])
def test_train_main_trains_conv1_checkpoints_and_resumes(tmp_path, prefetch):
    """Both training loops hand the feature map itself to the step."""
    from ick_amd import train as tr, utils as ut
    data_dir = str(tmp_path / "data")
    synth.write_dataset(data_dir, "toy", "geo", n_train=24, n_val=8, n_test=4, L=12, K=6, V=60, F=0)
    base = dict(variant="geo", data_dir=data_dir, data_name="toy", batch_size=8, workers=0, print_freq=1000, fused=True,
                seed=3, train_conv1=True, out_dir=str(tmp_path), prefetch=prefetch)
    torch.manual_seed(0)
    hist = tr.main(tr.Config(epochs=2, **base))
    assert len(hist) == 2 and hist[1][0] < hist[0][0]                                   # the training loss falls
    c0 = ut.load_checkpoint(str(tmp_path / "checkpoint_0_toy.pth.tar"), map_location="cuda")
    c1 = ut.load_checkpoint(str(tmp_path / "checkpoint_toy.pth.tar"), map_location="cuda")
    w0, w1 = c0["encoder"].conv1.weight.detach(), c1["encoder"].conv1.weight.detach()
    assert (w0 - w1).abs().max().item() > 1e-5                                         # conv1 moves between epochs
    eo = c1["encoder_optimizer"]
    assert isinstance(eo, torch.optim.Adam) and eo.param_groups[0]["lr"] == 1e-4
    assert [tuple(p.shape) for p in eo.param_groups[0]["params"]] == [(300, 2048, 1, 1), (300,)]
    assert {float(st["step"]) for st in eo.state.values()} == {6.0}                    # 2 epochs x 24 samples / batch 8
    assert {float(st["step"]) for st in c1["decoder_optimizer"].state.values()} == {6.0}
    # resume: epoch 2 continues both optimizers
    tr.main(tr.Config(epochs=3, checkpoint=str(tmp_path / "checkpoint_toy.pth.tar"), **base))
    c2 = ut.load_checkpoint(str(tmp_path / "checkpoint_2_toy.pth.tar"), map_location="cuda")
    assert c2["epoch"] == 2
    assert {float(st["step"]) for st in c2["encoder_optimizer"].state.values()} == {9.0}
    m1 = c1["encoder_optimizer"].state_dict()["state"][0]["exp_avg"]
    m2 = c2["encoder_optimizer"].state_dict()["state"][0]["exp_avg"]
    # three more steps of beta1 = 0.9 keep 0.729 of the restored first moment: a resume that lost it would start from zero
    assert ((m2 - 0.729 * m1).norm() < (m2 - 0.0 * m1).norm()).item()
    assert (c2["encoder"].conv1.weight.detach() - w1).abs().max().item() > 1e-5
