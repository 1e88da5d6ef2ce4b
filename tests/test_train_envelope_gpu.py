"""The training-step kernels across their supported envelope (tests/train_cases.py) against float64 torch autograd on
the CPU: attention forward / backward on both kernel families, the forward and backward row chains, the LayerNorm
backward.  Each attention case asserts its launch plan first.  Operand pad columns and padding rows hold NaN; outputs
the kernel overwrites start as NaN, and the memory around every output must come back unchanged.

Bars (relative to max(1, |ref|max)): attention output and lse 5e-6, gradients 1e-5 (with attention-weight dropout 1e-5
and 2e-5); row chains 2e-5 (norm outputs) to 5e-5 (GEMM outputs behind the norm); LayerNorm dz 5e-6, dgamma / dbeta 2e-5.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import ick_amd.ops as ops
from ick_amd import lib as L
from train_cases import ATTN, ATTN_REJECTED, CHAIN, CHAIN_BWD, LN, AttnCase
from test_train_plan_cpu import expected

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 1234.5          # value of the memory around an output


def close(got, ref, tol, what):
    got = got.detach().cpu().double()
    ref = ref.detach().double()
    assert torch.isfinite(got).all(), "%s: non-finite values" % what
    err = (got - ref).abs().max().item() if ref.numel() else 0.0
    lim = tol * max(1.0, ref.abs().max().item() if ref.numel() else 0.0)
    assert err <= lim, "%s max|err| %.3e > %.3e" % (what, err, lim)


def gen(seed):
    g = torch.Generator().manual_seed(seed)
    return lambda *s: torch.randn(*s, generator=g)


def seed_of(name):
    return sum((i + 1) * ord(ch) for i, ch in enumerate(name)) % 100003


# ------------------------------------------------------------------------------------------------------ attention
def attn_ref(c, q, k, v, mask):
    """float64 autograd: q (B, H, T, dh), k / v (B, H, S, dh) leaves; returns (out (B, T, d), lse (B, H, T))."""
    att = q @ k.transpose(-1, -2) / math.sqrt(c.dh)
    if c.causal:
        hidden = torch.arange(c.S).view(1, c.S) > c.pos0 + torch.arange(c.T).view(c.T, 1)
        att = att.masked_fill(hidden, float("-inf"))
    p = att.softmax(-1)
    if mask is not None:
        p = p * mask
    return (p @ v).transpose(1, 2).reshape(c.B, c.T, c.H * c.dh), att.logsumexp(-1)


@pytest.mark.parametrize("c", ATTN, ids=lambda c: c.name)
def test_attention(c: AttnCase):
    for direction, want in (("fwd", c.fwd), ("bwd", c.bwd)):
        got = ops.attention_plan(direction, c.T, c.S, c.dh)
        assert {k: got[k] for k in expected(want)} == expected(want), (direction, got)
    overwrites = ops.attention_plan("bwd", c.T, c.S, c.dh)["overwrites"]
    B, H, T, S, dh, hp = c.B, c.H, c.T, c.S, c.dh, c.hp
    d = H * dh
    r = gen(seed_of(c.name))
    q, k, v, dO = r(B, H, T, dh), r(B, H, S, dh), r(B, H, S, dh), r(B, T, d)
    # head-major padded operands with NaN pad columns and NaN rows past T / S
    qh = torch.full((B, 1, H, T + 3, hp), NAN, device="cuda")
    kvh = torch.full((B, 2, H, S + 5, hp), NAN, device="cuda")
    qh[:, 0, :, :T, :dh] = q.cuda()
    kvh[:, 0, :, :S, :dh] = k.cuda()
    kvh[:, 1, :, :S, :dh] = v.cuda()
    drop = (c.drop, 9001 + seed_of(c.name), 17) if c.drop > 0 else None
    mask = ops.dropout_mask(B * H * T, S, *drop).cpu().double().view(B, H, T, S) if drop else None
    obuf = torch.full((B, T + 1, d + 3), GUARD, device="cuda")
    O = obuf[:, :T, :d]
    O.fill_(NAN)
    gbuf = torch.full((B, T + 1, d + 3), NAN, device="cuda")      # dO: the backward reads it with O's strides
    gbuf[:, :T, :d] = dO.cuda()
    lbuf = torch.full((B * H * T + 4,), GUARD, device="cuda")
    lse = lbuf[:B * H * T]
    lse.fill_(NAN)
    ops.attention_heads(qh, kvh, O, H, dh, T, S, 0, 0, 1, causal=c.causal, q_pos0=c.pos0, lse=lse, drop=drop)

    qr, kr, vr = (x.double().requires_grad_(True) for x in (q, k, v))
    ref, lse_ref = attn_ref(c, qr, kr, vr, mask)
    ref.backward(dO.double())
    ftol, btol = (1e-5, 2e-5) if drop else (5e-6, 1e-5)
    close(O, ref, ftol, "out")
    close(lse.view(B, H, T), lse_ref, 5e-6, "lse")
    assert (obuf[:, T:] == GUARD).all() and (obuf[:, :T, d:] == GUARD).all() and (lbuf[B * H * T:] == GUARD).all()

    # backward: dQ rows (B, T, d), dK / dV the two column halves of one (B, S, 2d) buffer (as the training step's
    # packed K/V gradient); rows past T / S and columns past d are guards
    qbuf = torch.full((B, T + 1, d + 3), GUARD, device="cuda")
    kvbuf = torch.full((B, S + 1, 2 * d), GUARD, device="cuda")
    dQ, dK, dV = qbuf[:, :T, :d], kvbuf[:, :S, :d], kvbuf[:, :S, d:]
    for t in (dQ, dK, dV):
        t.fill_(NAN if overwrites else 0.0)
    ops.attention_heads_bwd(qh, kvh, O, gbuf[:, :T, :d], lse, dQ, dK, dV, H, dh, T, S, 0, 0, 1, causal=c.causal, drop=drop,
                            q_pos0=c.pos0)
    close(dQ, qr.grad.transpose(1, 2).reshape(B, T, d), btol, "dq")
    close(dK, kr.grad.transpose(1, 2).reshape(B, S, d), btol, "dk")
    close(dV, vr.grad.transpose(1, 2).reshape(B, S, d), btol, "dv")
    assert (qbuf[:, T:] == GUARD).all() and (qbuf[:, :T, d:] == GUARD).all() and (kvbuf[:, S:] == GUARD).all()


@pytest.mark.parametrize("direction,T,S,dh", ATTN_REJECTED)
def test_attention_entry_points_reject_what_the_plan_rejects(direction, T, S, dh):
    B, H = 1, 1
    hp = 64 if dh > 32 else 32
    qh = torch.zeros(B, 1, H, T, hp, device="cuda")
    kvh = torch.zeros(B, 2, H, S, hp, device="cuda")
    O = torch.zeros(B, T, H * dh, device="cuda")
    lse = torch.zeros(B * H * T, device="cuda")
    with pytest.raises(L.IckError, match="EINVAL"):
        if direction == "fwd":
            ops.attention_heads(qh, kvh, O, H, dh, T, S, 0, 0, 1, lse=lse)
        else:
            dq, dkv = torch.zeros(B, T, H * dh, device="cuda"), torch.zeros(B, S, 2 * H * dh, device="cuda")
            ops.attention_heads_bwd(qh, kvh, O, O, lse, dq, dkv[:, :, :H * dh], dkv[:, :, H * dh:], H, dh, T, S)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------- forward chain
def _chain_proj(c, a, w2p, b2, y2, heads, drop2):
    """ick_rowchain_fwd with ICK_CHAIN_PROJ: y2 = act(A W2^T + b2) (ops.rowchain_fwd has no such mode)."""
    g = L.RowChainArgs()
    g.A, g.a_rs, g.M, g.K1, g.d = a.data_ptr(), a.stride(0), c.M, c.K1, c.d
    g.w2p, g.b2, g.N2, g.flags = w2p.data_ptr(), b2.data_ptr(), c.N2, 512 | (1 if c.relu else 0) | (256 if c.slim else 0)
    if drop2:
        g.drop2_p, g.drop_seed, g.drop2_site = drop2[0], drop2[1], drop2[2]
    g.y2 = y2.data_ptr()
    if heads:
        nseg, H = heads
        g.y2_rs, g.y2_grp, g.y2_gs = 0, c.M // c.B, y2.stride(0)
        g.hs_dh, g.hs_dhp, g.hs_H, g.hs_S, g.hs_s0 = c.N2 // nseg // H, ops.DHP, H, c.M // c.B, 0
    else:
        g.y2_rs = y2.stride(0)
    L.check(L.load().ick_rowchain_fwd(C.byref(g), C.c_void_p(torch.cuda.current_stream().cuda_stream)),
            "ick_rowchain_fwd")


@pytest.mark.parametrize("c", CHAIN, ids=lambda c: c.name)
def test_rowchain_fwd(c):
    assert ops.rowchain_supported(c.K1, c.d, c.N2)
    M, K1, d, N2 = c.M, c.K1, c.d, c.N2
    r = gen(seed_of(c.name))
    a, w1, b1, res = r(M, K1), r(d, K1) / K1 ** 0.5, 0.1 * r(d), r(M, d)
    gamma, beta = 1 + 0.1 * r(d), 0.1 * r(d)
    w2, b2 = (r(N2, d) / d ** 0.5, 0.1 * r(N2)) if N2 else (None, None)
    s = seed_of(c.name) + 5
    drop1 = (c.drop1, s, 3) if c.drop1 > 0 else None
    drop2 = (c.drop2, s, 4) if c.drop2 > 0 else None
    m1 = ops.dropout_mask(M, d, *drop1).cpu().double() if drop1 else 1.0
    m2 = ops.dropout_mask(M, N2, *drop2).cpu().double() if drop2 else 1.0
    if c.heads:
        nseg, H = c.heads
        T, dh = M // c.B, N2 // nseg // H
        y2 = torch.full((c.B, nseg, H, T, ops.DHP), NAN, device="cuda")
    elif N2:
        y2buf = torch.full((M + 1, N2 + 3), GUARD, device="cuda")
        y2 = y2buf[:M, :N2]
        y2.fill_(NAN)

    if c.proj:
        _chain_proj(c, a.cuda(), ops.pack_weight(w2.cuda()), b2.cuda(), y2, c.heads, drop2)
        xin = a.double()
    else:
        xbuf = torch.full((M + 1, d + 3), GUARD, device="cuda")
        x = xbuf[:M, :d]
        x.fill_(NAN)
        o = torch.full((M, d), NAN, device="cuda")
        mean, rstd = ops.rowchain_fwd(a.cuda(), ops.pack_weight(w1.cuda()), b1.cuda(), res.cuda(), gamma.cuda(),
                                      beta.cuda(), 1e-5, x, drop1=drop1, o_out=o, save_stats=True,
                                      w2p=ops.pack_weight(w2.cuda()) if N2 else None, b2=b2.cuda() if N2 else None,
                                      y2=y2 if N2 else None, relu=c.relu, drop2=drop2,
                                      heads=(c.heads[0], c.heads[1], M // c.B, 0, M // c.B) if c.heads else None,
                                      slim=c.slim)
        ro = a.double() @ w1.double().t() + b1.double()
        z = ro * m1 + res.double()
        rx = F.layer_norm(z, (d,), gamma.double(), beta.double(), 1e-5)
        close(o, ro, 2e-5, "o")
        close(x, rx, 2e-5, "x")
        close(mean, z.mean(1), 2e-5, "mean")
        close(1 / rstd.double(), (z.var(1, unbiased=False) + 1e-5).sqrt(), 2e-5, "1/rstd")
        assert (xbuf[M:] == GUARD).all() and (xbuf[:M, d:] == GUARD).all()
        xin = rx
    if not N2:
        return
    ry = xin @ w2.double().t() + b2.double()
    if c.relu:
        ry = ry.relu()
    ry = ry * m2
    if c.heads:
        got = y2[..., :dh].permute(0, 3, 1, 2, 4).reshape(M, N2)
        assert torch.isnan(y2[..., dh:]).all()
    else:
        got = y2
        assert (y2buf[M:] == GUARD).all() and (y2buf[:M, N2:] == GUARD).all()
    close(got, ry, 5e-5, "y2")


# ------------------------------------------------------------------------------------------------ backward chain
def _ln_bwd_ref(dx, o, res, gamma, mask):
    """float64 add & norm backward: dz (gradient of the normalised sum), do = dz * mask, dgamma, dbeta."""
    z = (o.double() * mask + res.double()).requires_grad_(True)
    y = F.layer_norm(z, (z.shape[1],), gamma.double(), torch.zeros_like(gamma).double(), 1e-5)
    y.backward(dx)
    zh = ((z - z.mean(1, keepdim=True)) * (z.var(1, unbiased=False, keepdim=True) + 1e-5).rsqrt()).detach()
    return z.grad, z.grad * mask, (dx * zh).sum(0), dx.sum(0)


@pytest.mark.parametrize("c", CHAIN_BWD, ids=lambda c: c.name)
def test_rowchain_bwd(c):
    assert ops.rowchain_bwd_supported(c.K0, c.d, c.N1)
    M, d, K0, N1 = c.M, c.d, c.K0, c.N1
    r = gen(seed_of(c.name))
    seed = 300 + seed_of(c.name)
    p = c.drop
    masks = {}

    def mk(site):
        if site not in masks:
            masks[site] = ops.dropout_mask(M, d, p, seed, site).cpu().double() if p > 0 else torch.ones(M, d).double()
        return masks[site]

    def norm_inputs(site):
        o, res, gamma = r(M, d), r(M, d), 1 + 0.1 * r(d)
        z = o.double() * mk(site) + res.double()
        return dict(o=o.cuda(), res=res.cuda(), gamma=gamma.cuda(), mean=z.mean(1).float().cuda(),
                    rstd=(z.var(1, unbiased=False) + 1e-5).rsqrt().float().cuda(),
                    drop=(p, seed, site) if p > 0 else None, do=torch.full((M, d), NAN, device="cuda"),
                    part=ops.ln_partials(M, d, "cuda").fill_(NAN))

    n1 = norm_inputs(3)
    w3 = r(d, d) / d ** 0.5
    g0 = w0 = g0dev = None
    if K0:
        g0, w0 = r(M, K0), r(K0, d) / K0 ** 0.5
        if c.grouped:
            # the context rows of a (B, S, K0) gradient buffer: 7 other rows in front of each sample's group (NaN)
            Bn = M // c.grouped
            buf = torch.full((Bn, c.grouped + 7, K0), NAN, device="cuda")
            buf[:, 7:] = g0.view(Bn, c.grouped, K0).cuda()
            g0dev = buf[:, 7:]
        else:
            g0dev = g0.cuda()
    dzin = r(M, d) if c.dzin else None
    out3, dz_out = torch.full((M, d), NAN, device="cuda"), torch.full((M, d), NAN, device="cuda")
    kw = {}
    if N1:
        n2 = norm_inputs(4)
        w2l, w1l = r(d, N1) / N1 ** 0.5, r(N1, d) / d ** 0.5        # linear2.weight (d, N1), linear1.weight (N1, d)
        act = (r(M, N1).relu() * (torch.rand(M, N1, generator=torch.Generator().manual_seed(seed)) > 0.3)).contiguous()
        t_out = torch.full((M, N1), NAN, device="cuda")
        kw = dict(ffn=dict(w1p=ops.pack_weight(w2l.t().cuda()), w2p=ops.pack_weight(w1l.t().cuda()), act=act.cuda(),
                           gate_scale=1.25, t_out=t_out), norm2=n2)
    ops.rowchain_bwd(M, d, n1, ops.pack_weight(w3.t().cuda()), out3, dz_out, g0=g0dev,
                     w0p=ops.pack_weight(w0.t().cuda()) if K0 else None, dzin=dzin.cuda() if c.dzin else None, **kw)
    if c.grouped:
        assert torch.isnan(buf[:, :7]).all()
    dx = (dzin.double() if c.dzin else 0) + (g0.double() @ w0.double() if K0 else 0)
    dz1, do1, dg1, db1 = _ln_bwd_ref(dx, n1["o"].cpu(), n1["res"].cpu(), n1["gamma"].cpu(), mk(3))
    close(n1["do"], do1, 2e-5, "do1")
    part = n1["part"].cpu().double().sum(0)
    close(part[:d], dg1, 2e-5, "dgamma1")
    close(part[d:], db1, 2e-5, "dbeta1")
    last_do, last_dz = do1, dz1
    if N1:
        t = (do1 @ w2l.double()) * (act.double() > 0) * 1.25
        close(t_out, t, 5e-5, "t")
        dx2 = dz1 + t @ w1l.double()
        dz2, do2, dg2, db2 = _ln_bwd_ref(dx2, n2["o"].cpu(), n2["res"].cpu(), n2["gamma"].cpu(), mk(4))
        close(n2["do"], do2, 5e-5, "do2")
        part = n2["part"].cpu().double().sum(0)
        close(part[:d], dg2, 5e-5, "dgamma2")
        close(part[d:], db2, 5e-5, "dbeta2")
        last_do, last_dz = do2, dz2
    close(dz_out, last_dz, 5e-5, "dz_out")
    close(out3, last_do @ w3.double(), 5e-5, "out3")


# ----------------------------------------------------------------------------------------------- LayerNorm backward
@pytest.mark.parametrize("c", LN, ids=lambda c: c.name)
def test_layernorm_bwd(c):
    rows, d = c.rows, c.d
    r = gen(seed_of(c.name))
    x, res, gamma, dy = r(rows, d), r(rows, d), 1 + 0.1 * r(d), r(rows, d)
    drop = (c.drop, 4000 + seed_of(c.name), 6) if c.drop > 0 else None
    mask = ops.dropout_mask(rows, d, *drop).cpu().double() if drop else torch.ones(rows, d).double()
    z = (x.double() * mask + (res.double() if c.res else 0)).requires_grad_(True)
    gr, br = gamma.double().requires_grad_(True), torch.zeros(d).double().requires_grad_(True)
    F.layer_norm(z, (d,), gr, br, 1e-5).backward(dy.double())
    mean = z.detach().mean(1).float().cuda()
    rstd = (z.detach().var(1, unbiased=False) + 1e-5).rsqrt().float().cuda()
    buf = torch.full((2, rows * d + 5), GUARD, device="cuda")      # dense rows, guards behind them
    dz, dxd = buf[0, :rows * d].view(rows, d), buf[1, :rows * d].view(rows, d)
    dz.fill_(NAN)
    dxd.fill_(NAN)
    rpb = L.load().ick_layernorm_bwd_rows_per_block()
    part = None
    dg = db = None
    was_det = ops.is_deterministic()
    if c.atomics:
        gbuf = torch.full((2 * d + 4,), GUARD, device="cuda")
        dg, db = gbuf[:d], gbuf[d:2 * d]
        dg.fill_(0.0)
        db.fill_(0.0)
        ops.set_deterministic(False)       # the float-atomic form is refused in deterministic mode
    else:
        part = torch.full(((rows + rpb - 1) // rpb, 2 * d), NAN, device="cuda")
    pp = lambda t: None if t is None else t.data_ptr()
    dp, dseed, dsite = drop if drop else (0.0, 0, 0)
    dyd, xd, resd, gd = dy.cuda(), x.cuda(), res.cuda() if c.res else None, gamma.cuda()
    try:
        rc = L.load().ick_layernorm_bwd(pp(dyd), pp(xd), pp(resd), pp(gd), pp(mean), pp(rstd), pp(dz), pp(dg), pp(db),
                                        rows, d, pp(dxd), dp, dseed, dsite, None, pp(part),
                                        torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    finally:
        ops.set_deterministic(was_det)
    L.check(rc, "ick_layernorm_bwd")
    close(dz, z.grad, 5e-6, "dz")
    close(dxd, z.grad * mask, 5e-6, "dx_drop")
    assert (buf[:, rows * d:] == GUARD).all()
    if c.atomics:
        got_g, got_b = dg, db
        assert (gbuf[2 * d:] == GUARD).all()
    else:
        s = part.cpu().double().sum(0)
        got_g, got_b = s[:d], s[d:]
    close(got_g, gr.grad, 2e-5, "dgamma")
    close(got_b, br.grad, 2e-5, "dbeta")
