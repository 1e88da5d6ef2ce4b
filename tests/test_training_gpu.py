"""Training-step parity on the MI355X (row a14): backward kernels vs torch autograd in fp64, whole-model
gradients vs the reference's own gradients (golden fixtures), the fused TrainStep vs the reference
sequence (CE -> backward -> clamp -> Adam), and data-parallel equivalence."""
import math

import pytest
import torch
import torch.nn.functional as F
from torch.nn.utils.rnn import pack_padded_sequence

import ick_amd
import ick_amd.synth as synth
from helpers import case_from_golden, load_golden, t
from oracle import restatement as R
from test_forward_gpu import build_decoder
from test_ops_gpu import close, dev, ref_attention, rnd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ops():
    import ick_amd.ops as ops
    return ops


# ------------------------------------------------------------------------------- kernel level
def test_layernorm_bwd(ops):
    rows, d = 130, 300
    x, r, g, b, dy = rnd(rows, d, seed=1), rnd(rows, d, seed=2), 1 + rnd(d, seed=3, scale=0.1), rnd(d, seed=4), \
        rnd(rows, d, seed=5)
    xr, rr, gr, br = (v.double().requires_grad_(True) for v in (x, r, g, b))
    F.layer_norm(xr + rr, (d,), gr, br, 1e-5).backward(dy.double())
    y, mean, rstd = ops.add_layernorm(dev(x), dev(r), dev(g), dev(b), save_stats=True)
    dg, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    dz, dxd = ops.layernorm_bwd(dev(dy), dev(x), dev(r), dev(g), mean, rstd, dg, db)
    # without dropout the dropped operand's gradient is a separate copy of dz (the next dgrad GEMM accumulates
    # into dz in place while side-stream weight-gradient kernels still read the copy)
    assert dxd is not dz and torch.equal(dxd, dz)
    close(dz, xr.grad, 5e-6, "ln dz")
    close(dg, gr.grad, 2e-5, "ln dgamma")
    close(db, br.grad, 2e-5, "ln dbeta")


@pytest.mark.parametrize("B,T,S,causal", [(3, 20, 216, False), (3, 20, 20, True), (2, 7, 6, False), (2, 40, 300, False),
                                          (2, 64, 340, False), (2, 33, 257, True), (2, 80, 300, False),
                                          (2, 20, 600, False)])
def test_attention_bwd(ops, B, T, S, causal):
    """Matrix-core backward (T <= 64, S <= 512, LDS permitting) and the general kernel behind it (last two)."""
    H, d = 10, 300
    dh = d // H
    x, mem, do = rnd(B, T, d, seed=1), rnd(B, S, d, seed=2), rnd(B, T, d, seed=3)
    wq, wkv = rnd(d, d, seed=4, scale=0.1), rnd(2 * d, d, seed=5, scale=0.1)
    q = ops.project_heads(dev(x), dev(wq), None, 1, H, T)
    kv = ops.project_heads(dev(mem), dev(wkv), None, 2, H, S)
    out = torch.empty(B, T, d, device="cuda")
    lse = torch.empty(B * H * T, device="cuda")
    ops.attention_heads(q, kv, out, H, dh, T, S, 0, 0, 1, causal=causal, lse=lse)
    qr = (x.double() @ wq.double().t()).requires_grad_(True)
    kvr = (mem.double() @ wkv.double().t())
    kr, vr = kvr[..., :d].clone().requires_grad_(True), kvr[..., d:].clone().requires_grad_(True)
    ref = ref_attention_f64(qr, kr, vr, H, causal)
    ref.backward(do.double())
    # buffers as the training step allocates them; where the kernel claims to write everything, prove it with NaN
    dq = ops.attention_bwd_buffer((B, T, d), T, S, dh, "cuda")
    dkv = ops.attention_bwd_buffer((B, S, 2 * d), T, S, dh, "cuda")
    if ops.L.load().ick_attention_bwd_overwrites(T, S, dh):
        dq.fill_(float("nan"))
        dkv.fill_(float("nan"))
    ops.attention_heads_bwd(q, kv, out, dev(do), lse, dq, dkv[:, :, :d], dkv[:, :, d:], H, dh, T, S, 0, 0, 1,
                            causal=causal)
    close(out, ref.detach(), 5e-6, "fwd")
    close(dq, qr.grad, 1e-5, "dq")
    close(dkv[:, :, :d], kr.grad, 1e-5, "dk")
    close(dkv[:, :, d:], vr.grad, 1e-5, "dv")


def ref_attention_f64(q, k, v, H, causal):
    B, T, d = q.shape
    S = k.shape[1]
    dh = d // H
    qq = q.view(B, T, H, dh).transpose(1, 2)
    kk = k.view(B, S, H, dh).transpose(1, 2)
    vv = v.view(B, S, H, dh).transpose(1, 2)
    att = qq @ kk.transpose(-1, -2) / math.sqrt(dh)
    if causal:
        att = att + torch.full((T, S), float("-inf"), dtype=att.dtype).triu(1)
    return (att.softmax(-1) @ vv).transpose(1, 2).reshape(B, T, d)


def test_linear_bwd_relu_colsum(ops):
    M, N, K = 1280, 512, 300
    x, w, b, dy = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3), rnd(M, N, seed=4)
    xr, wr, br = (v.double().requires_grad_(True) for v in (x, w, b))
    yr = F.relu(F.linear(xr, wr, br))
    yr.backward(dy.double())
    y = ops.linear(dev(x), dev(w), dev(b), relu=True)
    dpre = ops.relu_bwd(dev(dy), y)
    dw, db = torch.zeros(N, K, device="cuda"), torch.zeros(N, device="cuda")
    dx = ops.linear_bwd(dpre, dev(x), dev(w), dw, db)
    close(dx, xr.grad, 2e-5, "dx")
    close(dw, wr.grad, 5e-5, "dw")
    close(db, br.grad, 5e-5, "db")


def test_pointer_and_embedding_bwd(ops):
    B, T, Kc, d, V = 4, 6, 7, 300, 50
    h, ctx, w, b = rnd(B, T, d, seed=1), rnd(B, Kc, d, seed=2), rnd(1, d, seed=3, scale=0.1), rnd(1, seed=4)
    ind = (rnd(B, T, Kc, seed=5) > 0).float()
    ds = rnd(B, T, V + Kc, seed=6)
    hr, cr, wr, br = (v.double().requires_grad_(True) for v in (h, ctx, w, b))
    s = ((hr.unsqueeze(2) * cr.unsqueeze(1) * ind.double().unsqueeze(3)) * wr.view(1, 1, 1, d)).sum(-1) + br
    s.backward(ds[:, :, V:].double())
    dh, dctx = torch.zeros(B, T, d, device="cuda"), torch.zeros(B, Kc, d, device="cuda")
    dw, db = torch.zeros(1, d, device="cuda"), torch.zeros(1, device="cuda")
    ops.pointer_scores_bwd(dev(ds), V, dev(h), dev(ctx), dev(w), dev(ind), dh, dctx, dw, db)
    close(dh, hr.grad, 1e-5, "dh")
    close(dctx, cr.grad, 1e-5, "dctx")
    close(dw, wr.grad, 2e-5, "dw")
    close(db, br.grad, 2e-5, "db")
    # caption embedding scatter
    variant, Lc, K, Fn = "knowledge", 9, 7, 6
    P = synth.make_params(variant, V, 3)
    cfg = R.config_from_word_map(variant, synth.make_word_map(V))
    batch = synth.make_batch(variant, B, Lc, K, V, Fn, 3)
    ee, fe = rnd(B, K, d, seed=7), rnd(B, Fn, d, seed=8)
    we = P["word_embedding.weight"]
    wer, eer, fer = (v.double().requires_grad_(True) for v in (we, ee, fe))
    emb = R.caption_embed(cfg, {"word_embedding.weight": wer}, batch["captions"], batch["caption_masks"], eer, fer)
    dx = rnd(B, Lc, d, seed=9)
    (emb * math.sqrt(d)).backward(dx.double())
    dword, dee, dfe = torch.zeros(V, d, device="cuda"), torch.zeros(B, K, d, device="cuda"), \
        torch.zeros(B, Fn, d, device="cuda")
    ops.caption_embed_bwd(dev(dx), dev(batch["captions"]), dev(batch["caption_masks"]), dword, dee, dfe, V, cfg.pad,
                          math.sqrt(d))
    close(dword, wer.grad, 1e-5, "dword")
    close(dee, eer.grad, 1e-5, "dee")
    close(dfe, fer.grad, 1e-5, "dfe")


def test_adam_clamp_matches_torch(ops):
    n = 10007
    p0, g0 = rnd(n, seed=1), rnd(n, seed=2, scale=20.0)
    pt = p0.clone().requires_grad_(True)
    opt = torch.optim.Adam([pt], lr=4e-4)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    for step in range(1, 4):
        g = g0 * step
        pt.grad = g.clone().clamp_(-5, 5)
        opt.step()
        ops.adam_update(p, dev(g), m, v, step, 4e-4, clip=5.0)
        close(p, pt.detach(), 2e-6, "adam step %d" % step)


# ------------------------------------------------------------------------------- dropout
def test_dropout_mask_statistics_and_determinism(ops):
    m1 = ops.dropout_mask(1280, 300, 0.5, 1234, 7)
    m2 = ops.dropout_mask(1280, 300, 0.5, 1234, 7)
    m3 = ops.dropout_mask(1280, 300, 0.5, 1234, 8)
    assert torch.equal(m1, m2) and not torch.equal(m1, m3)
    vals = set(m1.unique().tolist())
    assert vals == {0.0, 2.0}
    keep = (m1 > 0).float().mean().item()
    assert abs(keep - 0.5) < 0.01
    m4 = ops.dropout_mask(1280, 300, 0.1, 99, 1)
    assert abs((m4 > 0).float().mean().item() - 0.9) < 0.01
    assert abs(m4.max().item() - 1 / 0.9) < 1e-6
    # neighbouring elements are uncorrelated
    a = (m1[:, :-1] > 0).float() - 0.5
    b = (m1[:, 1:] > 0).float() - 0.5
    assert abs((a * b).mean().item()) < 0.01


def test_dropout_sites_match_their_mask(ops):
    """Every dropping kernel (GEMM epilogue, add_layernorm, attention fwd/bwd) against torch math that uses
    the mask reported by ick_dropout_mask for the same (p, seed, site)."""
    M, N, K, d = 130, 512, 300, 300
    drop = (0.5, 4242, 3)
    x, w, b = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=0.1), rnd(N, seed=3)
    mask = ops.dropout_mask(M, N, *drop).cpu().double()
    y = ops.linear(dev(x), dev(w), dev(b), relu=True, drop=drop)
    close(y, F.relu(F.linear(x.double(), w.double(), b.double())) * mask, 2e-5, "gemm relu dropout")
    # add_layernorm + backward
    rows = 130
    xx, r, g, be, dy = rnd(rows, d, seed=4), rnd(rows, d, seed=5), 1 + rnd(d, seed=6, scale=0.1), rnd(d, seed=7), \
        rnd(rows, d, seed=8)
    drop2 = (0.3, 77, 5)
    m2 = ops.dropout_mask(rows, d, *drop2).cpu().double()
    xr, rr, gr, br = (v.double().requires_grad_(True) for v in (xx, r, g, be))
    ref = F.layer_norm(xr * m2 + rr, (d,), gr, br, 1e-5)
    ref.backward(dy.double())
    yy, mean, rstd = ops.add_layernorm(dev(xx), dev(r), dev(g), dev(be), save_stats=True, drop=drop2)
    close(yy, ref.detach(), 5e-6, "ln dropout fwd")
    dg, db = torch.zeros(d, device="cuda"), torch.zeros(d, device="cuda")
    dz, dxd = ops.layernorm_bwd(dev(dy), dev(xx), dev(r), dev(g), mean, rstd, dg, db, drop=drop2)
    close(dz, rr.grad, 5e-6, "ln dropout dres")
    close(dxd, xr.grad, 5e-6, "ln dropout dx")
    close(dg, gr.grad, 2e-5, "ln dropout dgamma")
    # attention with weight dropout
    B, T, S, H = 2, 20, 216, 10
    dh = d // H
    drop3 = (0.5, 31337, 9)
    q0, mem, do = rnd(B, T, d, seed=9), rnd(B, S, d, seed=10), rnd(B, T, d, seed=11)
    wq, wkv = rnd(d, d, seed=12, scale=0.1), rnd(2 * d, d, seed=13, scale=0.1)
    qh = ops.project_heads(dev(q0), dev(wq), None, 1, H, T)
    kvh = ops.project_heads(dev(mem), dev(wkv), None, 2, H, S)
    out = torch.empty(B, T, d, device="cuda")
    lse = torch.empty(B * H * T, device="cuda")
    ops.attention_heads(qh, kvh, out, H, dh, T, S, 0, 0, 1, lse=lse, drop=drop3)
    m3 = ops.dropout_mask(B * H * T, S, *drop3).cpu().double().view(B, H, T, S)
    qr = (q0.double() @ wq.double().t()).requires_grad_(True)
    kvr = mem.double() @ wkv.double().t()
    kr, vr = kvr[..., :d].clone().requires_grad_(True), kvr[..., d:].clone().requires_grad_(True)
    att = (qr.view(B, T, H, dh).transpose(1, 2) @ kr.view(B, S, H, dh).transpose(1, 2).transpose(-1, -2)) / math.sqrt(dh)
    ref = ((att.softmax(-1) * m3) @ vr.view(B, S, H, dh).transpose(1, 2)).transpose(1, 2).reshape(B, T, d)
    ref.backward(do.double())
    close(out, ref.detach(), 1e-5, "attn dropout fwd")
    dq = torch.zeros(B, T, d, device="cuda")
    dkv = torch.zeros(B, S, 2 * d, device="cuda")
    ops.attention_heads_bwd(qh, kvh, out, dev(do), lse, dq, dkv[:, :, :d], dkv[:, :, d:], H, dh, T, S, 0, 0, 1,
                            drop=drop3)
    close(dq, qr.grad, 2e-5, "attn dropout dq")
    close(dkv[:, :, :d], kr.grad, 2e-5, "attn dropout dk")
    close(dkv[:, :, d:], vr.grad, 2e-5, "attn dropout dv")


def test_training_with_reference_dropout_reduces_loss():
    """The reference's training configuration (dropout 0.5/0.5/0.1, geo-aware/models.py:219): a few fused
    steps on a fixed batch must drive the loss down, and eval-mode scores stay finite."""
    from ick_amd.training import TrainStep
    variant, B, L, K, V, seed = "geo", 16, 12, 8, 200, 8
    m = ick_amd.load_models(variant)
    torch.manual_seed(0)
    dec = m.DecoderTransformer(synth.make_word_map(V), 300, 512, 512, 10, 3)   # default dropouts
    dec.load_state_dict(synth.make_params(variant, V, seed), strict=False)
    dec = dec.cuda().train()
    batch = synth.make_batch(variant, B, L, K, V, 0, seed)
    enc_out = synth.make_enc_out(B, seed).cuda()
    ts = TrainStep(dec, lr=4e-4, seed=3)
    losses = [ts(batch["captions"].cuda(), enc_out, batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
                 batch["entities"]).item() for _ in range(30)]
    assert all(math.isfinite(v) for v in losses)
    assert sum(losses[-5:]) / 5 < sum(losses[:5]) / 5 - 0.3, losses
    # the packed cross-K/V weights used by the next forward must follow the in-place Adam update
    d = dec.emb_dim
    wkv, _ = dec._packed_cross_kv()
    l0 = dec.transformer_decoder.layers[0].multihead_attn.in_proj_weight
    assert torch.equal(wkv[:2 * d], l0.detach()[d:])
    dec.eval()
    with torch.no_grad():
        sc, _, _ = dec(batch["captions"].cuda(), enc_out, batch["caption_masks"].cuda(),
                       batch["caption_lengths"].cuda(), batch["entities"])
    assert torch.isfinite(sc).all()


# ------------------------------------------------------------------------------- whole model
def zero_dropout(dec):
    for mod in dec.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return dec


def reference_loss(scores, caps_sorted, dl, pad):
    targets = caps_sorted[:, 1:]
    sp = pack_padded_sequence(scores, dl, batch_first=True).data
    tp = pack_padded_sequence(targets, dl, batch_first=True).data
    return F.cross_entropy(sp, tp, ignore_index=pad)


@pytest.mark.parametrize("name", ["fwd_tiny_geo", "fwd_tiny_knowledge", "fwd_tiny_news", "fwd_mid_geo",
                                  "fwd_mid_knowledge"])
def test_gradients_vs_reference_golden(name):
    """loss.backward() through the drop-in module == the reference's gradients (train.py's loss)."""
    g = load_golden(name)
    cfg, P, wm, batch, enc_out = case_from_golden(g)
    dec = build_decoder(cfg.variant, cfg.vocab_size, P)
    args = [batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
            batch["entities"]]
    if "facts" in batch:
        args.append(batch["facts"].cuda())
    scores, caps, dl = dec(*args)
    assert scores.requires_grad
    loss = reference_loss(scores, caps, dl, wm["<pad>"])
    assert abs(loss.item() - float(g["loss"][0])) < 2e-5
    loss.backward()
    named = dict(dec.named_parameters())
    norms = dict(zip(g["grad_norm_names"].tolist(), g["grad_norms"].tolist()))
    for k, n in norms.items():
        if k.startswith("fact_encoder."):
            continue
        assert named[k].grad is not None, k
        mine = float(named[k].grad.double().norm())
        assert abs(mine - n) <= 2e-4 * max(n, 1e-3), (k, mine, n)
    for k in g:
        if k.startswith("grad::"):
            ref = t(g[k])
            err = (named[k[6:]].grad.cpu() - ref).abs().max().item()
            assert err < 2e-5 * max(1.0, ref.abs().max().item()), (k, err)


def test_train_step_matches_reference_sequence_and_dp_split():
    """TrainStep (fused CE + backward + clamp + Adam) vs the reference sequence on the CPU oracle; then
    the same update from two half-batch 'ranks' whose buckets are summed (what the all-reduce does)."""
    from ick_amd.training import TrainStep, backward_from_tape, forward_with_tape
    import ick_amd.ops as ops
    variant, B, L, K, V, Fn, seed = "knowledge", 6, 9, 5, 120, 4, 5
    P = synth.make_params(variant, V, seed)
    wm = synth.make_word_map(V)
    cfg = R.config_from_word_map(variant, wm)
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    enc_out = synth.make_enc_out(B, seed)
    # reference sequence on the oracle (CPU autograd, torch Adam)
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items() if not k.startswith("fact_encoder.")}
    Pr["fact_encoder.predicate_embedding.weight"] = Pr["predicate_embedding.weight"]
    uniq = [v for k, v in Pr.items() if not k.startswith("fact_encoder.")]
    opt = torch.optim.Adam(uniq, lr=4e-4)
    scores, caps, dl = R.forward(cfg, Pr, batch["captions"], enc_out, batch["caption_masks"],
                                 batch["caption_lengths"], batch["entities"], batch["facts"])
    loss_ref = R.packed_ce_loss(cfg, scores, caps, dl)
    loss_ref.backward()
    for p in uniq:
        p.grad.clamp_(-5.0, 5.0)
    opt.step()
    # fused step
    dec = zero_dropout(build_decoder(variant, V, P).train())
    ts = TrainStep(dec, lr=4e-4, grad_clip=5.0)
    loss = ts(batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(),
              batch["caption_lengths"].cuda(), batch["entities"], batch["facts"].cuda())
    assert abs(loss.item() - loss_ref.item()) < 2e-5
    named = dict(dec.named_parameters())
    for k, pr in Pr.items():
        if k.startswith("fact_encoder."):
            continue
        err = (named[k].detach().cpu() - pr.detach()).abs().max().item()
        assert err < 5e-5, (k, err)   # Adam's first step moves every weight by ~lr=4e-4: a wrong gradient shows
    # ---- DP: two ranks, half the batch each; sum of the unnormalised buckets == full-batch bucket
    dec2 = zero_dropout(build_decoder(variant, V, P).train())
    full = TrainStep(dec2, lr=4e-4)
    buckets = []
    for lo in (0, 3):
        sub = {k: v[lo:lo + 3] for k, v in batch.items()}
        lengths, sort_ind = sub["caption_lengths"].squeeze(1).sort(descending=True)
        sd = sort_ind.cuda()
        caps_s = sub["captions"].cuda()[sd].contiguous()
        masks_s = sub["caption_masks"].cuda()[sd].contiguous()
        ents_s = sub["entities"].cuda()[sd].contiguous()
        facts_s = sub["facts"].cuda()[sd].contiguous()
        enc_tok = enc_out[lo:lo + 3].cuda().permute(0, 2, 1).contiguous()
        full.flat_g.zero_()
        sc, tape = forward_with_tape(dec2, caps_s, masks_s, ents_s, facts_s, enc_tok, sd.to(torch.int32))
        ls, cnt, dsc = ops.packed_ce(sc, caps_s, (lengths - 1).to(torch.int32).cuda(), wm["<pad>"], want_grad=True)
        backward_from_tape(dec2, tape, dsc, full.grads)
        full.flat_g[full.n:full.n + 1].copy_(ls)
        full.flat_g[full.n + 1:].copy_(cnt)
        buckets.append(full.flat_g.clone())
    summed = buckets[0] + buckets[1]           # == all_reduce(SUM)
    full.flat_g.zero_()
    sd = batch["caption_lengths"].squeeze(1).sort(descending=True)
    caps_s = batch["captions"].cuda()[sd.indices.cuda()].contiguous()
    sc, tape = forward_with_tape(dec2, caps_s, batch["caption_masks"].cuda()[sd.indices.cuda()].contiguous(),
                                 batch["entities"].cuda()[sd.indices.cuda()].contiguous(),
                                 batch["facts"].cuda()[sd.indices.cuda()].contiguous(),
                                 enc_out.cuda().permute(0, 2, 1).contiguous(), sd.indices.cuda().to(torch.int32))
    ls, cnt, dsc = ops.packed_ce(sc, caps_s, (sd.values - 1).to(torch.int32).cuda(), wm["<pad>"], want_grad=True)
    backward_from_tape(dec2, tape, dsc, full.grads)
    assert cnt.item() == summed[full.n + 1].item()
    err = (summed[:full.n] - full.flat_g[:full.n]).abs().max().item()
    assert err < 1e-4 * max(1.0, full.flat_g[:full.n].abs().max().item()), err


def test_train_step_split_allreduce_path_equals_single_graph(monkeypatch):
    """With several ranks TrainStep captures the step as two graphs (early / late gradients) around two all-reduces;
    forced on here with one rank: same loss, same gradients, same update as the single-graph step, for two steps."""
    from ick_amd.training import TrainStep, early_parameters
    variant, B, L, K, V, Fn, seed = "knowledge", 6, 9, 5, 120, 4, 7
    P = synth.make_params(variant, V, seed)
    batch = synth.make_batch(variant, B, L, K, V, Fn, seed)
    enc_out = synth.make_enc_out(B, seed)
    args = (batch["captions"].cuda(), enc_out.cuda(), batch["caption_masks"].cuda(), batch["caption_lengths"].cuda(),
            batch["entities"], batch["facts"].cuda())
    steps = []
    for split in ("0", "1"):
        monkeypatch.setenv("ICK_SPLIT_ALLREDUCE", split)
        dec = zero_dropout(build_decoder(variant, V, P).train())
        ts = TrainStep(dec, lr=4e-4, grad_clip=5.0)
        assert ts.split == (split == "1")
        n_early = sum((p.numel() + 63) // 64 * 64 for p in early_parameters(dec))   # 256-byte aligned slots
        assert ts.n_early == n_early and 0 < n_early < ts.n
        losses = [ts(*args).item() for _ in range(2)]
        steps.append((losses, ts.flat_g[:ts.n].clone(), ts.flat_p.clone()))
    (l0, g0, p0), (l1, g1, p1) = steps
    assert max(abs(a - b) for a, b in zip(l0, l1)) < 1e-5
    assert (g0 - g1).abs().max().item() < 1e-5 * max(1.0, g0.abs().max().item())
    # Adam divides by sqrt(v): where a gradient is rounding noise of the float atomics (1e-9), the two runs may step
    # in different directions by up to lr; anywhere else the updates agree
    assert ((p0 - p1).abs() > 5e-5).float().mean().item() < 1e-3


def test_bench_two_ranks_share_the_gpu_over_gloo():
    """`python bench.py --gpus 2` exactly as the driver types it, WITHOUT torchrun: bench.py starts torch.distributed.run
    itself as a child process (two ranks on the one GPU of this box, collectives over gloo instead of RCCL): rendezvous,
    per-rank shards, the bucket all-reduce inside the timed loop, the single JSON line relayed from rank 0 with the number
    of ranks the probe all-reduce saw and the host baseline (--full)."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    env.update(ICK_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "2",
           "--full", "--cpu-seconds", "2", "--min-seconds", "0.2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=root)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["ranks_seen"] == 2 and d["config"]["global_batch"] == 128 and d["value"] > 0
    assert d["scaling"] == "weak" and d["config"]["collective_backend"] == "gloo"
    assert d["config"]["graph"] is True and d["repeats"] >= 1 and d["steps"] == 3 and "modes" not in d
    assert "pass_frac" not in d["roofline"] and d["roofline"]["pass_frac_executed"] > 0
    assert d["cpu_baseline"]["value"] > 0 and d["cpu_baseline"]["kind"] == "port"
    assert d["config"]["allreduce_probe_ms"] > 0 and d["config"]["split_allreduce"] is False


def test_train_step_from_features_and_in_place_input_buffers():
    """TrainStep(encoder=...) takes the (B, 2048, 14, 14) feature map: Encoder.conv1 runs inside the captured step and
    writes the image rows into the memory buffer.  Same loss / gradients as encoder(feats) followed by the step; and a
    batch written in place into the step's own input buffers (no per-step input copy) gives the same result as passing
    it as arguments."""
    from ick_amd.training import TrainStep
    variant, B, L, K, V, seed = "geo", 5, 9, 6, 150, 3
    P = synth.make_params(variant, V, seed)
    m = ick_amd.load_models(variant)
    enc = m.Encoder(emb_dim=300)
    cw, cb = synth.make_conv1(seed)
    with torch.no_grad():
        enc.conv1.weight.copy_(cw)
        enc.conv1.bias.copy_(cb)
    enc = enc.cuda().eval()

    def batch_args(s2):
        b = synth.make_batch(variant, B, L, K, V, 0, s2)
        return b, synth.make_feats(B, s2).cuda()

    res = {}
    for mode in ("features", "encoder_out"):
        dec = zero_dropout(build_decoder(variant, V, P).train())
        ts = TrainStep(dec, lr=4e-4, encoder=enc if mode == "features" else None)
        out = []
        for s2 in (1, 2):
            b, feats = batch_args(s2)
            with torch.no_grad():
                x = feats if mode == "features" else enc(feats)
            loss = ts(b["captions"].cuda(), x, b["caption_masks"].cuda(), b["caption_lengths"].cuda(), b["entities"])
            out.append((loss.item(), ts.flat_g[:ts.n].clone()))
        res[mode] = (out, ts)
    for (la, ga), (lb, gb) in zip(res["features"][0], res["encoder_out"][0]):
        assert abs(la - lb) < 1e-5
        assert (ga - gb).abs().max().item() < 1e-5 * max(1.0, gb.abs().max().item())
    # in-place refill of the input buffers == passing the batch
    ts = res["features"][1]
    bufs = ts.input_buffers()
    b, feats = batch_args(7)
    dec2 = zero_dropout(build_decoder(variant, V, P).train())
    ref_ts = TrainStep(dec2, lr=4e-4, encoder=enc)
    with torch.no_grad():
        ts.flat_p.copy_(ref_ts.flat_p); ts.flat_m.zero_(); ts.flat_v.zero_(); ts.counter.zero_()
    ref_loss = ref_ts(b["captions"].cuda(), feats, b["caption_masks"].cuda(), b["caption_lengths"].cuda(), b["entities"])
    for dst, src in zip(bufs, (b["captions"], feats, b["caption_masks"], b["caption_lengths"], b["entities"])):
        dst.copy_(src)
    loss = ts(*bufs)
    assert abs(loss.item() - ref_loss.item()) < 1e-5
    assert (ts.flat_g[:ts.n] - ref_ts.flat_g[:ref_ts.n]).abs().max().item() < 1e-5 * max(1.0, ref_ts.flat_g[:ref_ts.n].abs().max().item())
