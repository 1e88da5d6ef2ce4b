"""Per-op Python wrappers over the C ABI.  Tensors are torch CUDA(ROCm) tensors used purely as
device memory + stream plumbing; all arithmetic happens in libick_amd.so."""
import contextlib
import ctypes as C
import gc
import math
import os

import torch

from . import lib as L


def _p(t):
    return None if t is None else t.data_ptr()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _f32c(t, name):
    if t.dtype != torch.float32 or not t.is_cuda:
        raise L.IckError("%s must be a float32 device tensor (got %s on %s)" % (name, t.dtype, t.device))
    return t


# bench.py hook: when set to {"shape": (M, N, K), "events": []}, every ick_gemm launch of that shape is
# bracketed by HIP events recorded on the launch stream (torch's current stream).
TIMED = None


def _extent(t):
    """Floats addressable from t.data_ptr() inside t's storage (bounds the kernel's buffer descriptor)."""
    return (t.untyped_storage().nbytes() - t.storage_offset() * t.element_size()) // 4


def _drop(a, drop):
    """drop = (p, seed, site[, epoch_tensor]) or None -> fields of an args struct."""
    if drop is not None and drop[0] > 0.0:
        a.drop_p, a.drop_seed, a.drop_site = float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2]) & 0xFFFFFFFF
        a.drop_epoch = _p(drop[3]) if len(drop) > 3 else None


def _dargs(drop):
    if drop is not None and drop[0] > 0.0:
        return (float(drop[0]), int(drop[1]) & 0xFFFFFFFF, int(drop[2]) & 0xFFFFFFFF,
                _p(drop[3]) if len(drop) > 3 else None)
    return 0.0, 0, 0, None


def gemm_args(A, B, Cout, M, N, K, a_rs, a_ks, b_rs, b_ks, c_rs, bias=None, a_grp=0, a_gs=0, a_gmap=None,
              c_grp=0, c_gs=0, c_gmap=None, relu=False, accumulate=False, atomic=False, split_k=1, alpha=1.0,
              drop=None, colsum_a=None, gate=None, gate_scale=1.0, b_ps=None, m_bound=None, k_bound=None,
              a_kmap=None, b_kmap=None):
    """ick_gemm_args for C[m,n] = act(alpha * sum_k A(m,k) B(n,k) + bias[n]) with explicit element strides; A/B/Cout
    are tensors (only their data pointers are used -- the caller guarantees the strides stay in bounds).
    split_k > 1 needs atomic=True and excludes relu and gate: the epilogue runs once per K slice, so either would be
    applied to the partial sums (the library answers ICK_EINVAL).
    colsum_a (k-major A only): colsum_a[m] += sum_k A(m,k).  b_ps: the pre-split copy of the (N, K) matrix B
    (presplit_weights): large problems then run on the LDS-DMA kernel of csrc/gemm_ps.hip.
    m_bound / k_bound: one-element int32 device tensors that bound the rows / the reduction length below M / K (the
    packed score head's row count; include/ick_amd.h).
    a_kmap / b_kmap: int32 device tensors, k-major operands only: reduction index k reads the operand's k line kmap[k]
    (the weight gradients over the valid caption rows of logical-row operands)."""
    for t in (A, B, Cout):
        if t.dtype != torch.float32:
            raise L.IckError("ick_gemm operands must be float32, got %s" % t.dtype)
    a = L.GemmArgs()
    a.A, a.B, a.C, a.bias = _p(A), _p(B), _p(Cout), _p(bias)
    a.M, a.N, a.K = M, N, K
    a.a_rs, a.a_ks, a.a_grp, a.a_gs, a.a_gmap = a_rs, a_ks, a_grp, a_gs, _p(a_gmap)
    a.b_rs, a.b_ks = b_rs, b_ks
    a.c_rs, a.c_grp, a.c_gs, a.c_gmap = c_rs, c_grp, c_gs, _p(c_gmap)
    a.flags = (L.GEMM_RELU if relu else 0) | (L.GEMM_ACCUM if accumulate else 0) | (L.GEMM_ATOMIC if atomic else 0)
    a.split_k = split_k
    a.alpha = alpha
    a.a_extent, a.b_extent = _extent(A), _extent(B)
    a.colsum_a = _p(colsum_a)
    if gate is not None:
        a.gate, a.gate_rs, a.gate_scale = _p(gate), gate.stride(0), gate_scale
    if b_ps is not None:
        assert b_ps.numel() * b_ps.element_size() == presplit_bytes(N, K), "b_ps is not the pre-split copy of an (N, K) matrix"
        a.b_ps = _p(b_ps)
    for name, t in (("m_bound", m_bound), ("k_bound", k_bound)):
        if t is not None:
            assert t.dtype == torch.int32 and t.numel() == 1 and t.is_cuda, "%s is a one-element int32 device tensor" % name
            setattr(a, name, _p(t))
    for name, t in (("a_kmap", a_kmap), ("b_kmap", b_kmap)):
        if t is not None:
            assert t.dtype == torch.int32 and t.is_cuda and t.is_contiguous(), "%s is an int32 device tensor" % name
            setattr(a, name, _p(t))
    _drop(a, drop)
    return a


DEFAULT_GEMM_SPLIT = 1      # the library's product mode when ICK_GEMM_SPLIT is not set (csrc/gemm.hip)


def presplit_bytes(N, K):
    n = L.i64()
    L.check(L.load_raw().ick_presplit_bytes(int(N), int(K), C.byref(n)), "ick_presplit_bytes")
    return int(n.value)


def presplit_weights(pairs, k_map=None, k_bound=None):
    """[(w (N, K) 2-D view with one unit stride -- a weight or its transposed view, dst uint8 buffer of
    presplit_bytes(N, K))]: the exact three-way bf16 split of every matrix in the image ick_gemm's b_ps wants
    (include/ick_amd.h, ick_presplit_weights); up to 16 matrices per launch.
    k_map / k_bound (int32 device tensors, transposed views only): column k of every matrix is read from source column
    k_map[k], and only the columns below k_bound[0] exist (the activation rows of the packed score head)."""
    items = (L.PresplitItem * len(pairs))()
    for it, (src, dst) in zip(items, pairs):
        assert src.dim() == 2 and src.dtype == torch.float32 and (src.stride(1) == 1 or src.stride(0) == 1)
        assert dst.numel() * dst.element_size() == presplit_bytes(src.shape[0], src.shape[1])
        it.src, it.dst, it.N, it.K = _p(src), _p(dst), src.shape[0], src.shape[1]
        it.src_rs, it.src_cs = src.stride(0), src.stride(1)
        if k_map is not None:
            assert k_map.dtype == torch.int32 and k_map.numel() >= src.shape[1] and src.stride(0) == 1
        it.k_map, it.k_bound = _p(k_map), _p(k_bound)
    L.check(L.load().ick_presplit_weights(items, len(pairs), _stream()), "ick_presplit_weights")


def presplit_buffer(N, K, device):
    return torch.empty(presplit_bytes(N, K), device=device, dtype=torch.uint8)


def presplit_cached(holder, name, w2d, key):
    """Persistent pre-split copy of the 2-D weight view `w2d`, kept in holder.__dict__ and refreshed IN PLACE (captured
    graphs keep reading the same buffer) when `key` (parameter versions / data pointers) changes.  None when the
    library's product mode is the exact fp32 MFMA: ick_gemm then never looks at it."""
    if gemm_split_mode() == 0:
        return None
    cache = holder.__dict__.setdefault("_ps_cache", {})
    ent = cache.get(name)
    nbytes = presplit_bytes(w2d.shape[0], w2d.shape[1])
    if ent is None or ent[1].numel() != nbytes or ent[1].device != w2d.device:
        ent = cache[name] = [None, torch.empty(nbytes, device=w2d.device, dtype=torch.uint8)]
    if ent[0] != key:
        presplit_weights([(w2d, ent[1])])
        ent[0] = key
    return ent[1]


def colsum_problem(a2d, out, split_k=1, k_bound=None):
    """ick_gemm_args of a pure column sum out[n] += sum_m a2d[m, n] (ICK_GEMM_COLSUM_ONLY): no kernel of its own,
    it rides in a grouped launch (gemm_grouped) with the weight-gradient GEMMs.  split_k: row slices (float atomics).
    k_bound: one-element int32 device tensor, only the rows below it are summed."""
    rows, cols = a2d.shape
    a = L.GemmArgs()
    a.A, a.colsum_a = _p(a2d), _p(out)
    a.M, a.N, a.K = cols, 1, rows
    a.a_rs, a.a_ks = 1, a2d.stride(0)
    a.flags, a.split_k, a.alpha = L.GEMM_COLSUM_ONLY | (L.GEMM_ATOMIC if split_k > 1 else 0), split_k, 1.0
    a.a_extent = _extent(a2d)
    a.k_bound = _p(k_bound)
    return a


def set_deterministic(on=True):
    """Deterministic mode of the library (ick_set_deterministic): scatter-adds and column sums of the backward pass in a
    fixed order instead of float atomics; every split below collapses to 1.  training.TrainStep(deterministic=True) and
    the autograd bridge also keep the step on one stream.  Slower, bit-reproducible run to run."""
    L.check(L.load().ick_set_deterministic(1 if on else 0), "ick_set_deterministic")


def set_gemm_split(mode):
    """Product mode of the large GEMM tiles (ick_set_gemm_split; ICK_GEMM_SPLIT in the environment; DEFAULT 1 since round
    4): 0 = every product on the exact fp32 MFMA; 1 = six bf16 x bf16 partial products of the exact three-way bf16 split
    of both fp32 operands, accumulated in fp32, where that is faster (B operand k-contiguous or pre-split); 2 = on every
    large-tile problem.  Non-finite operands (documented difference, tests/test_gemm_split_gpu.py): the residual planes
    of a +-inf element -- and of a finite one within 2^-8 of FLT_MAX, whose bf16 hi plane rounds to infinity -- are NaN
    (inf - inf), so its dot products are NaN in the split modes where the exact mode gives +-inf / a finite sum."""
    L.check(L.load().ick_set_gemm_split(int(mode)), "ick_set_gemm_split")


def gemm_split_mode():
    return int(L.load().ick_get_gemm_split())


def is_deterministic():
    return bool(L.load().ick_get_deterministic())


def wgrad_split(rows, n_out, k_in, grouped=False):
    """K split of a weight-gradient GEMM (reduction over `rows`): enough workgroups to fill the GPU (~1600), slices
    of at least 256 rows.  Measured (probe_ops): vocabulary 10000x300 over 1280 rows 121 us at 5 slices, 91 us at 2.
    grouped: the problem goes out in a layer's grouped launch (~1000 workgroups together): two slices are enough, more
    only add atomics and prologues (train step 2.01 -> 1.98 ms)."""
    if is_deterministic():
        return 1       # slices of one reduction meet in float atomics: their order would decide the rounding
    tiles = ((n_out + 63) // 64) * ((k_in + 63) // 64)
    cap = 2 if grouped else 16
    return max(1, min(cap, rows // 256, (1600 + tiles // 2) // tiles))


# K slices of a decoder-layer weight gradient that reduces over the valid caption rows only (linear_bwd's valid=): the
# split is sized from the host-side row count B * L, the reduction that runs is ~0.6 of it.  One against two slices inside
# the captured step: profiles/valid_row_wgrad_ab.txt (ICK_VALID_ROW_WGRAD_SLICES is that sweep's knob).
VALID_ROW_WGRAD_SLICES = max(1, int(os.environ.get("ICK_VALID_ROW_WGRAD_SLICES", "2") or 2))


CONV1_TILE = (128, 64)   # workgroup tile ick_gemm picks for Encoder.conv1 at bench size on the exact fp32 MFMA


def conv1_tile():
    """The workgroup tile Encoder.conv1 runs on at bench size in the library's current product mode (asserted by the
    parity tests): 128 x 80 of the pre-split kernel (csrc/gemm_ps.hip; two workgroups per CU, small enough to share the
    CU with the other stream's row chains) with split products, else CONV1_TILE."""
    return (128, 80) if gemm_split_mode() >= 1 else CONV1_TILE

# test hook: a list that receives (M, N, K, plan dict) of every single-problem ick_gemm launch while it is set
PLAN_LOG = None


def gemm_plan(a):
    """Kernel configuration ick_gemm would choose for the ick_gemm_args `a` (ick_gemm_plan)."""
    info = L.GemmPlanInfo()
    L.check(L.load().ick_gemm_plan(C.byref(a), C.byref(info)), "ick_gemm_plan")
    return {n: getattr(info, n) for n, _ in L.GemmPlanInfo._fields_}


def _log_plan(a):
    if PLAN_LOG is not None:
        PLAN_LOG.append((a.M, a.N, a.K, gemm_plan(a)))


def gemm_raw(A, B, Cout, M, N, K, *args, **kwargs):
    """Launch one GEMM (see gemm_args)."""
    a = gemm_args(A, B, Cout, M, N, K, *args, **kwargs)
    _log_plan(a)
    timed = TIMED is not None and TIMED["shape"] == (M, N, K)
    if timed:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
    L.check(L.load().ick_gemm(C.byref(a), _stream()), "ick_gemm")
    if timed:
        e1.record()
        TIMED["events"].append((e0, e1))
    return Cout


# test hook: a list that receives the ick_gemm_args of every problem handed to gemm_grouped while it is set
GROUP_LOG = None


def gemm_grouped(problems):
    """Launch a list of ick_gemm_args; problems of one kernel configuration share a launch."""
    if GROUP_LOG is not None:
        GROUP_LOG.extend(problems)
    for i in range(0, len(problems), 64):
        chunk = problems[i:i + 64]
        arr = (L.GemmArgs * len(chunk))(*chunk)
        L.check(L.load().ick_gemm_grouped(arr, len(chunk), _stream()), "ick_gemm_grouped")


def linear(x, w, bias=None, out=None, relu=False, drop=None, w_ps=None):
    """y = x @ w.T + bias for x (..., K) with contiguous last dim and uniform row stride, w (N, K)."""
    _f32c(x, "x"); _f32c(w, "w")
    K = x.shape[-1]
    N = w.shape[0]
    x2 = x.reshape(-1, K)
    if x2.stride(1) != 1:
        x2 = x2.contiguous()
    M = x2.shape[0]
    if out is None:
        out = torch.empty(x.shape[:-1] + (N,), device=x.device, dtype=torch.float32)
    o2 = out.view(-1, N) if out.is_contiguous() else out
    gemm_raw(x2, w, o2, M, N, K, x2.stride(0), 1, w.stride(0), 1, o2.stride(0), bias=bias, relu=relu, drop=drop,
             b_ps=w_ps)
    return out


def add_layernorm(x, res, gamma, beta, eps=1e-5, out=None, save_stats=False, drop=None):
    """LayerNorm(dropout(x) + res) * gamma + beta (dropout only in training: drop = (p, seed, site))."""
    d = x.shape[-1]
    x2 = x.reshape(-1, d)
    r2 = None if res is None else res.reshape(-1, d)
    rows = x2.shape[0]
    if out is None:
        out = torch.empty_like(x2)
    o2 = out.view(-1, d)
    mean = rstd = None
    if save_stats:
        mean = torch.empty(rows, device=x.device, dtype=torch.float32)
        rstd = torch.empty(rows, device=x.device, dtype=torch.float32)
    L.check(L.load().ick_add_layernorm(_p(x2), _p(r2), _p(gamma), _p(beta), _p(o2), rows, d, eps, x2.stride(0),
                                       0 if r2 is None else r2.stride(0), o2.stride(0), _p(mean), _p(rstd),
                                       *_dargs(drop), _stream()), "ick_add_layernorm")
    out = out.view(x.shape)
    return (out, mean, rstd) if save_stats else out


def rowchain_supported(K1, d, N2=0):
    """Can ick_rowchain_fwd run a chain with these widths (GEMM 1 input, LayerNorm width, GEMM 2 output)?"""
    return bool(L.load_raw().ick_rowchain_supported(int(K1), int(d), int(N2)))


def packed_weight_floats(N, K):
    n = L.i64()
    L.check(L.load_raw().ick_packed_weight_floats(int(N), int(K), C.byref(n)), "ick_packed_weight_floats")
    return int(n.value)


def pack_weights(pairs, copies=()):
    """[(m (N, K) 2-D view with positive strides, dst flat float buffer of packed_weight_floats(N, K))]: the packed
    copies the row-chain kernels read (include/ick_amd.h), up to 48 matrices per launch.  A transposed view (w.t())
    gives the operand of the data-gradient chains.  copies: [(src (N, K) view, dst (N, K) view with unit column
    stride)] plain copies that ride in the same launch."""
    todo = [(s_, d_, 0) for s_, d_ in pairs] + [(s_, d_, 1) for s_, d_ in copies]
    for i in range(0, len(todo), 48):
        chunk = todo[i:i + 48]
        items = (L.PackItem * len(chunk))()
        for it, (src, dst, plain) in zip(items, chunk):
            assert src.dim() == 2
            it.src, it.dst, it.N, it.K = _p(src), _p(dst), src.shape[0], src.shape[1]
            it.src_rs, it.src_cs = max(1, src.stride(0)), src.stride(1)
            if plain:
                assert dst.shape == src.shape and (dst.stride(1) == 1 or dst.shape[1] == 1)
                it.dst_rs = max(dst.stride(0), src.shape[1])
            else:
                assert dst.is_contiguous() and dst.numel() == packed_weight_floats(src.shape[0], src.shape[1])
                it.dst_rs = 0
        L.check(L.load().ick_pack_weights(items, len(chunk), _stream()), "ick_pack_weights")


def pack_weight(w):
    """Packed copy of one (N, K) weight (a new tensor)."""
    dst = torch.empty(packed_weight_floats(w.shape[0], w.shape[1]), device=w.device, dtype=torch.float32)
    pack_weights([(w, dst)])
    return dst


def rowchain_fwd(a, w1p, b1, res, gamma, beta, eps, x_out, drop1=None, o_out=None, save_stats=False,
                 w2p=None, b2=None, y2=None, relu=False, drop2=None, heads=None, slim=False):
    """One launch for  o = a @ W1.T + b1;  x = LayerNorm(res + dropout1(o)) * gamma + beta;  y2 = act(x @ W2.T + b2)
    (dropout2 on y2).  a (..., K1) rows with a uniform row stride; w1p / w2p are packed copies (pack_weights) of the
    (d, K1) and (N2, d) nn.Linear weights; b2 gives N2; x_out (..., d) may be a (B, T, d) view with a sample stride
    (rows inside the memory buffer); heads = (nseg, H, S, s0, grp): y2 is the head-major buffer (B, nseg, H, S, DHP)
    of project_heads.  slim: 8-wave workgroups (ICK_CHAIN_SLIM), for chains that run beside bulk GEMMs on another
    stream.  Returns (mean, rstd) -- (None, None) without save_stats."""
    K1, d = a.shape[-1], gamma.shape[0]
    a2 = a.reshape(-1, K1)
    if a2.stride(1) != 1:
        a2 = a2.contiguous()
    M = a2.shape[0]
    r2 = res.reshape(-1, d)
    g = L.RowChainArgs()
    g.A, g.a_rs, g.a_grp, g.a_gs = _p(a2), a2.stride(0), 0, 0
    g.M, g.K1, g.d = M, K1, d
    g.w1p, g.b1 = _p(w1p), _p(b1)
    g.res, g.res_rs = _p(r2), r2.stride(0)
    g.gamma, g.beta, g.eps = _p(gamma), _p(beta), eps
    g.drop1_p, g.drop_seed, g.drop1_site, g.drop_epoch = _dargs(drop1)
    if o_out is not None:
        g.o, g.o_rs = _p(o_out), o_out.reshape(-1, d).stride(0)
    if x_out.dim() == 3 and not x_out.is_contiguous():
        assert x_out.stride(2) == 1
        g.x, g.x_rs, g.x_grp, g.x_gs = _p(x_out), x_out.stride(1), x_out.shape[1], x_out.stride(0)
    else:
        g.x, g.x_rs, g.x_grp, g.x_gs = _p(x_out), x_out.reshape(-1, d).stride(0), 0, 0
    mean = rstd = None
    if save_stats:
        mean = torch.empty(M, device=a.device, dtype=torch.float32)
        rstd = torch.empty(M, device=a.device, dtype=torch.float32)
        g.mean, g.rstd = _p(mean), _p(rstd)
    if w2p is not None:
        N2 = b2.shape[0]
        g.w2p, g.b2, g.N2, g.flags = _p(w2p), _p(b2), N2, (1 if relu else 0)
        p2, seed2, site2, ep2 = _dargs(drop2)
        g.drop2_p, g.drop2_site = p2, site2
        if p2 > 0.0:
            if g.drop1_p > 0.0:
                assert seed2 == g.drop_seed
            else:
                g.drop_seed, g.drop_epoch = seed2, ep2
        g.y2 = _p(y2)
        if heads is not None:
            nseg, H, S, s0, grp = heads
            g.y2_rs, g.y2_grp, g.y2_gs = 0, grp, y2.stride(0)
            g.hs_dh, g.hs_dhp, g.hs_H, g.hs_S, g.hs_s0 = (N2 // nseg) // H, DHP, H, S, s0
        else:
            g.y2_rs, g.y2_grp, g.y2_gs = y2.reshape(-1, N2).stride(0), 0, 0
    if slim:
        g.flags |= 256
    L.check(L.load().ick_rowchain_fwd(C.byref(g), _stream()), "ick_rowchain_fwd")
    return mean, rstd


def rowchain_bwd_supported(K0, d, N1=0):
    return bool(L.load_raw().ick_rowchain_bwd_supported(int(K0), int(d), int(N1)))


def ln_partials(rows, d, device):
    """Buffer for the per-workgroup gamma / beta partial sums of a LayerNorm backward (8 rows per workgroup)."""
    rpb = L.load_raw().ick_layernorm_bwd_rows_per_block()
    return torch.empty((rows + rpb - 1) // rpb, 2 * d, device=device, dtype=torch.float32)


def rowchain_bwd(M, d, norm1, w3p, out3, dz_out, g0=None, w0p=None, dzin=None, ffn=None, norm2=None):
    """One launch for the data-gradient path between two attention-backward kernels (include/ick_amd.h,
    ick_rowchain_bwd).  norm1 / norm2 = dict(o, res, mean, rstd, gamma, drop, do, part): saved forward tensors of an
    add & norm, its dropout triple, and the outputs do (M, d) / part (ln_partials).  ffn = dict(w1p, w2p, act,
    gate_scale, t_out) with packed linear2.weight.T / linear1.weight.T.  g0 (M, K0) @ W0 (packed W0.T = w0p) and dzin
    (M, d) are the two addends of the incoming gradient.  (An 8-wave form of this kernel was built in round 4 -- the 16-wave
    one takes 480 of a SIMD's 512 registers, so its workgroups only start on CUs that hold nothing of the other stream --
    and measured slower inside the step all the same, 1.746 against 1.700 ms, profiles/r04_y_ab_slim_bwd.txt; removed.)"""
    a = L.RowChainBwdArgs()
    a.M, a.d = M, d
    a.flags = 0
    seeds = []

    def norm(prefix, n):
        setattr(a, "o" + prefix, _p(n["o"])); setattr(a, "res" + prefix, _p(n["res"]))
        setattr(a, "mean" + prefix, _p(n["mean"])); setattr(a, "rstd" + prefix, _p(n["rstd"]))
        setattr(a, "gamma" + prefix, _p(n["gamma"]))
        pp, seed, site, ep = _dargs(n.get("drop"))
        setattr(a, "drop%s_p" % prefix, pp); setattr(a, "drop%s_site" % prefix, site)
        if pp > 0.0:
            seeds.append((seed, ep))
        setattr(a, "do" + prefix, _p(n["do"])); setattr(a, "part" + prefix, _p(n["part"]))

    norm("1", norm1)
    if g0 is not None:
        if g0.dim() == 3 and not g0.is_contiguous():
            # rows of a (B, T, K0) view with a sample stride (the context rows of the cross K/V gradient buffer)
            assert g0.stride(2) == 1 and g0.shape[0] * g0.shape[1] == M
            a.g0, a.g0_rs, a.K0, a.w0p = _p(g0), g0.stride(1), g0.shape[2], _p(w0p)
            a.g0_grp, a.g0_gs = g0.shape[1], g0.stride(0)
        else:
            g2 = g0.reshape(M, -1)
            assert g2.stride(1) == 1
            a.g0, a.g0_rs, a.K0, a.w0p = _p(g2), g2.stride(0), g2.shape[1], _p(w0p)
    if dzin is not None:
        z2 = dzin.reshape(M, d)
        a.dzin, a.dzin_rs = _p(z2), z2.stride(0)
    if ffn is not None:
        a.w1p, a.N1, a.act, a.gate_scale = _p(ffn["w1p"]), ffn["act"].shape[-1], _p(ffn["act"]), float(ffn["gate_scale"])
        a.t_out, a.w2p = _p(ffn["t_out"]), _p(ffn["w2p"])
        norm("2", norm2)
    if seeds:
        assert all(s == seeds[0] for s in seeds)
        a.drop_seed, a.drop_epoch = seeds[0]
    a.w3p, a.out3, a.dz_out = _p(w3p), _p(out3), _p(dz_out)
    L.check(L.load().ick_rowchain_bwd(C.byref(a), _stream()), "ick_rowchain_bwd")


def attention_raw(Q, K, V, O, B, H, T, S, dh, q_bs, q_hs, q_ts, k_bs, k_hs, k_ss, v_bs, v_hs, v_ss, o_bs, o_ts,
                  causal=False, q_pos0=0, kv_len=None, lse=None, q_off=0, k_off=0, v_off=0, drop=None):
    """Strides in elements: batch / head / row for Q, K, V (see include/ick_amd.h); q_off/k_off/v_off are
    element offsets of the first (segment) inside a packed buffer."""
    a = L.AttnArgs()
    a.Q = Q.data_ptr() + 4 * q_off
    a.K = K.data_ptr() + 4 * k_off
    a.V = V.data_ptr() + 4 * v_off
    a.O, a.lse = _p(O), _p(lse)
    a.B, a.H, a.T, a.S, a.dh = B, H, T, S, dh
    a.q_bs, a.q_hs, a.q_ts = q_bs, q_hs, q_ts
    a.k_bs, a.k_hs, a.k_ss = k_bs, k_hs, k_ss
    a.v_bs, a.v_hs, a.v_ss = v_bs, v_hs, v_ss
    a.o_bs, a.o_ts = o_bs, o_ts
    a.scale = 1.0 / math.sqrt(dh)
    a.causal, a.q_pos0, a.kv_len = int(causal), q_pos0, _p(kv_len)
    _drop(a, drop)
    L.check(L.load().ick_attention(C.byref(a), _stream()), "ick_attention")
    return O


def attention(q, k, v, H, causal=False):
    """q (B,T,d), k/v (B,S,d) row-major -> (B,T,d)."""
    B, T, d = q.shape
    S = k.shape[1]
    dh = d // H
    out = torch.empty_like(q)
    attention_raw(q, k, v, out, B, H, T, S, dh, q.stride(0), dh, q.stride(1), k.stride(0), dh, k.stride(1),
                  v.stride(0), dh, v.stride(1), out.stride(0), out.stride(1), causal=causal)
    return out


DHP = 32  # padded head width of the head-major projection buffers


def project_heads(x, w, bias, nseg, H, S, out=None, s0=0, grp=None, a_gmap=None, a_gs=None, w_ps=None):
    """Packed projection x (B*grp rows, K) @ w.T (nseg*d, K) scattered into the head-major layout
    out (B, nseg, H, S, DHP) at positions s0 .. s0+grp-1 (ick_gemm head-split epilogue)."""
    d = w.shape[0] // nseg
    K = w.shape[1]
    strided = x.dim() == 3 and not x.is_contiguous() and x.stride(2) == 1 and a_gmap is None
    if strided:
        # rows of a (B, T, K) view with a sample stride (the image rows inside the (B, S, d) memory buffer): no copy,
        # the GEMM walks the groups itself
        x2 = x
        M = x.shape[0] * x.shape[1]
    else:
        x2 = x.reshape(-1, K)
        M = x2.shape[0]
    grp = grp if grp is not None else (x.shape[1] if x.dim() == 3 else M)
    Bn = M // grp
    if out is None:
        out = torch.empty(Bn, nseg, H, S, DHP, device=x.device, dtype=torch.float32)
    a = L.GemmArgs()
    a.A, a.B, a.C, a.bias = _p(x2), _p(w), _p(out), _p(bias)
    a.M, a.N, a.K = M, w.shape[0], K
    a.a_rs, a.a_ks = (x.stride(1) if strided else x2.stride(0)), 1
    if strided:
        a.a_grp, a.a_gs = x.shape[1], x.stride(0)
    if a_gmap is not None:
        a.a_grp, a.a_gs, a.a_gmap = grp, a_gs, _p(a_gmap)
    a.b_rs, a.b_ks = w.stride(0), 1
    a.c_rs, a.c_grp, a.c_gs = 0, grp, out.stride(0)
    a.split_k, a.alpha = 1, 1.0
    a.a_extent, a.b_extent = _extent(x2), _extent(w)
    a.hs_dh, a.hs_dhp, a.hs_H, a.hs_S, a.hs_s0 = d // H, DHP, H, S, s0
    if w_ps is not None:
        assert w_ps.numel() == presplit_bytes(w.shape[0], K)
        a.b_ps = _p(w_ps)
    _log_plan(a)
    L.check(L.load().ick_gemm(C.byref(a), _stream()), "ick_gemm(head-split)")
    return out


# test hook: a list that receives (direction, T, S, dh, causal) of every head-major attention launch while it is set
# (attention_plan(direction, T, S, dh) then names the kernels that launch took)
ATTN_LOG = None


def attention_heads(q, kv, O, H, dh, T, S, q_seg=0, k_seg=0, v_seg=1, causal=False, kv_len=None, q_pos0=0, q_t0=0,
                    lse=None, drop=None):
    """Attention over head-major buffers: q (B, nq, H, Tq_alloc, DHP), kv (B, nkv, H, S_alloc, DHP);
    the first T query rows starting at q_t0 attend to the first S key rows."""
    if ATTN_LOG is not None:
        ATTN_LOG.append(("fwd", T, S, dh, bool(causal)))
    B = q.shape[0]
    Tq, Sa, hp = q.shape[3], kv.shape[3], q.shape[4]
    assert kv.shape[4] == hp
    attention_raw(q, kv, kv, O, B, H, T, S, dh,
                  q.stride(0), Tq * hp, hp, kv.stride(0), Sa * hp, hp, kv.stride(0), Sa * hp, hp,
                  O.stride(0), O.stride(1), causal=causal, q_pos0=q_pos0, kv_len=kv_len, lse=lse, drop=drop,
                  q_off=q_seg * H * Tq * hp + q_t0 * hp, k_off=k_seg * H * Sa * hp, v_off=v_seg * H * Sa * hp)
    return O


def entity_encode(variant, entities, type_emb, d, facts=None, word_emb=None):
    B, K, cols = entities.shape
    out = torch.empty(B, K, d, device=entities.device, dtype=torch.float32)
    F = 0 if facts is None else facts.shape[1]
    L.check(L.load().ick_entity_encode(L.VARIANT_ID[variant], _p(entities), cols, _p(facts), _p(type_emb),
                                       type_emb.shape[0], _p(word_emb), 0 if word_emb is None else word_emb.shape[0],
                                       _p(out), B, K, F, d, _stream()), "ick_entity_encode")
    return out


def fact_encode(facts, entities_encoded, pred_emb):
    B, F, _ = facts.shape
    K, d = entities_encoded.shape[1], entities_encoded.shape[2]
    out = torch.empty(B, F, d, device=facts.device, dtype=torch.float32)
    L.check(L.load().ick_fact_encode(_p(facts), _p(entities_encoded), _p(pred_emb), pred_emb.shape[0], _p(out), B, K,
                                     F, d, _stream()), "ick_fact_encode")
    return out


def caption_embed(captions, masks, word_emb, entities_encoded, facts_encoded, pe, V, pad_token, scale, pos0=0,
                  want_emb=False, drop=None):
    B, Lc = captions.shape
    K, d = entities_encoded.shape[1], entities_encoded.shape[2]
    F = 0 if facts_encoded is None else facts_encoded.shape[1]
    out = torch.empty(B, Lc, d, device=captions.device, dtype=torch.float32)
    emb = torch.empty_like(out) if want_emb else None
    L.check(L.load().ick_caption_embed(_p(captions), _p(masks), _p(word_emb), _p(entities_encoded),
                                       _p(facts_encoded), _p(pe), _p(out), _p(emb), B, Lc, K, F, V, d, pad_token,
                                       scale, pos0, *_dargs(drop), _stream()), "ick_caption_embed")
    return (out, emb) if want_emb else out


def context_indicators(captions, facts, K, V, fc_pred_wt=None, fc_pred_b=None, mode=0, eib=None, gate=None,
                       dense_pred=0):
    """dense_pred = number of predicates: `gate` becomes the dense (B, T, num_pred) 0/1 predicate indicator instead of
    fc_predicate applied to it."""
    B, Lc = captions.shape
    F = facts.shape[1]
    T = Lc if mode == 0 else 1
    if eib is None:
        eib = torch.empty(B, T, F, device=captions.device, dtype=torch.float32)
    num_pred = d = 0
    if fc_pred_wt is not None:
        num_pred, d = fc_pred_wt.shape
        if gate is None:
            gate = torch.empty(B, T, d, device=captions.device, dtype=torch.float32)
    elif dense_pred:
        num_pred = d = dense_pred
        if gate is None:
            gate = torch.empty(B, T, d, device=captions.device, dtype=torch.float32)
    L.check(L.load().ick_context_indicators(_p(captions), _p(facts), _p(fc_pred_wt), _p(fc_pred_b), _p(eib),
                                            _p(gate), B, Lc, T, K, F, V, num_pred, d, mode, _stream()),
            "ick_context_indicators")
    return eib, gate


def pointer_scores(h, ctx, w, bias, out, col0, ind=None, out_gmap=None, pack=None):
    """pack (HeadRows): the scores of the valid rows only, into the packed rows of `out` (ick_pointer_scores_packed)."""
    B, T, d = h.shape
    Kc = ctx.shape[1]
    if pack is not None:
        assert out_gmap is None
        L.check(L.load().ick_pointer_scores_packed(_p(h), _p(ctx), _p(w), _p(bias), _p(ind), _p(out), B, T, Kc, d,
                                                   out.stride(-2), col0, _p(pack.rowmap), _p(pack.count), _stream()),
                "ick_pointer_scores_packed")
        return out
    L.check(L.load().ick_pointer_scores(_p(h), _p(ctx), _p(w), _p(bias), _p(ind), _p(out), B, T, Kc, d,
                                        out.stride(-2), col0, _p(out_gmap), _stream()), "ick_pointer_scores")
    return out


def mul(a, b, out=None):
    if out is None:
        out = torch.empty_like(a)
    L.check(L.load().ick_mul(_p(a), _p(b), _p(out), a.numel(), _stream()), "ick_mul")
    return out


def top2(scores):
    B, Vx = scores.shape
    best = torch.empty(B, device=scores.device, dtype=torch.int32)
    second = torch.empty_like(best)
    L.check(L.load().ick_top2(_p(scores), scores.stride(0), B, Vx, _p(best), _p(second), _stream()), "ick_top2")
    return best, second


def greedy_select(scores, output, hist, finished, next_token, next_mask, step, V, K, has_facts, end_token):
    """top2 + greedy_update of one decode step in one launch; scores (B, Vx) rows."""
    B, Vx = scores.shape
    L.check(L.load().ick_greedy_select(_p(scores), scores.stride(0), B, Vx, _p(output), _p(hist), _p(finished),
                                       _p(next_token), _p(next_mask), step, output.shape[1], V, K, int(has_facts),
                                       end_token, _stream()), "ick_greedy_select")


def greedy_update(best, second, output, hist, finished, next_token, next_mask, step, V, K, has_facts, end_token):
    B, max_len = output.shape
    L.check(L.load().ick_greedy_update(_p(best), _p(second), _p(output), _p(hist), _p(finished), _p(next_token),
                                       _p(next_mask), B, step, max_len, V, K, int(has_facts), end_token, _stream()),
            "ick_greedy_update")


def decode_supported(d, H, FF, S, max_len):
    return bool(L.load().ick_decode_supported(d, H, FF, S, max_len))


DECODE_PLAN_KEYS = ("g_self", "fsel", "g_cross", "cross_shared", "g_ffn", "head_merged", "gather_loop")


def decode_plan(R, rows_per_sample, d, H, FF):
    """The kernels ick_decode_layers launches for these sizes (ick_decode_plan; host only, no GPU needed)."""
    out = (C.c_int32 * len(DECODE_PLAN_KEYS))()
    L.check(L.load().ick_decode_plan(R, rows_per_sample, d, H, FF, out), "ick_decode_plan")
    return dict(zip(DECODE_PLAN_KEYS, (int(v) for v in out)))


def decode_beam_supported(Vx, beam):
    return bool(L.load().ick_decode_beam_supported(Vx, beam))


def decode_sample_supported(Vx, rows_per_sample):
    return bool(L.load().ick_decode_sample_supported(Vx, rows_per_sample))


def decode_layers(ctx, pos):
    """Decoder stack + score head of one KV-cached decode step (ick_decode_layers); ctx: lib.DecodeCtx."""
    L.check(L.load().ick_decode_layers(C.byref(ctx), pos, _stream()), "ick_decode_layers")


def decode_layers_part(ctx, pos, part):
    """part 1: the first self-attention block (with ctx.sel_state: the previous step's token selection inside it);
    part 2: the rest of the step."""
    L.check(L.load().ick_decode_layers_part(C.byref(ctx), pos, part, _stream()), "ick_decode_layers_part")


def decode_layers_attn(ctx, attn, pos, part=0):
    """decode_layers_part that also writes step `pos`'s cross-attention weights into attn: a float32 device tensor
    (max_len, R, layers, H, S) (ick_decode_layers_attn; attn=None: exactly decode_layers_part)."""
    if attn is not None:
        want = (ctx.max_len, ctx.R, ctx.layers, ctx.H, ctx.S)
        if not (attn.is_cuda and attn.dtype == torch.float32 and attn.is_contiguous() and tuple(attn.shape) == want):
            raise L.IckError("decode_layers_attn needs a contiguous float32 device tensor of shape %s (got %s %s on %s)"
                             % (want, tuple(attn.shape), attn.dtype, attn.device))
    if part not in (0, 1, 2):
        raise L.IckError("decode_layers_attn: part must be 0, 1 or 2")
    L.check(L.load().ick_decode_layers_attn(C.byref(ctx), None if attn is None else attn.data_ptr(), pos, part,
                                            _stream()), "ick_decode_layers_attn")


def decode_init(ctx, start_token, n_done_init=0):
    L.check(L.load().ick_decode_init(C.byref(ctx), start_token, n_done_init, _stream()), "ick_decode_init")


def decode_select_greedy(ctx, pos):
    L.check(L.load().ick_decode_select_greedy(C.byref(ctx), pos, _stream()), "ick_decode_select_greedy")


def _ref(s):
    return None if s is None else C.byref(s)


def decode_select_beam(ctx, beam_state, pos, rules=None, diversity=None, constraints=None, bias=None, prefix=None):
    """Beam selection of step `pos` (ick_decode_select_beam), under decoding rules (lib.DecodeRules: n-gram / min-length
    bans, length penalty) or none, as plain, diverse (lib.DecodeDiversity: groups, penalty: ick_..._diverse) or
    constrained beam search (lib.DecodeConstraints: force, met: ick_..._forced), or with a column bias (lib.DecodeBias:
    cols, vals, sum: ick_..._biased; not with groups or forced columns).  prefix: lib.DecodePrefix (cols: the forced column
    of every step, ick_..._prefix), with the rules, groups or a bias; not with forced columns."""
    if prefix is not None:
        if constraints is not None:
            raise L.IckError("decode_select_beam: a caption prefix does not compose with forced columns")
        if diversity is not None and bias is not None:
            raise L.IckError("decode_select_beam: a column bias does not compose with beam groups or forced columns")
        name, extra = "ick_decode_select_beam_prefix", (_ref(rules), _ref(diversity), _ref(bias), C.byref(prefix))
    elif bias is not None:
        if diversity is not None or constraints is not None:
            raise L.IckError("decode_select_beam: a column bias does not compose with beam groups or forced columns")
        name, extra = "ick_decode_select_beam_biased", (_ref(rules), C.byref(bias))
    elif constraints is not None:
        name, extra = "ick_decode_select_beam_forced", (_ref(rules), C.byref(constraints))
    elif diversity is not None:
        name, extra = "ick_decode_select_beam_diverse", (_ref(rules), C.byref(diversity))
    else:
        name, extra = ("ick_decode_select_beam", ()) if rules is None else ("ick_decode_select_beam_rules", (_ref(rules),))
    L.check(getattr(L.load(), name)(C.byref(ctx), C.byref(beam_state), *extra, pos, _stream()), name)


def decode_select_beam_forced(ctx, beam_state, rules, constraints, pos):
    decode_select_beam(ctx, beam_state, pos, rules, constraints=constraints)


def decode_select_sample(ctx, sample_state, pos, rules=None, bias=None, prefix=None):
    """Sampled token of step `pos` for every live row (ick_decode_select_sample); sample_state: lib.SampleState; rules:
    lib.DecodeRules (n-gram / min-length bans: ick_decode_select_sample_rules) or None; bias: lib.DecodeBias (cols, vals:
    ick_decode_select_sample_biased) or None; prefix: lib.DecodePrefix (cols: the forced column of every step,
    ick_decode_select_sample_prefix) or None."""
    if prefix is not None:
        name, extra = "ick_decode_select_sample_prefix", (_ref(rules), _ref(bias), C.byref(prefix))
    elif bias is not None:
        name, extra = "ick_decode_select_sample_biased", (_ref(rules), C.byref(bias))
    else:
        name, extra = ("ick_decode_select_sample", ()) if rules is None else \
            ("ick_decode_select_sample_rules", (_ref(rules),))
    L.check(getattr(L.load(), name)(C.byref(ctx), C.byref(sample_state), *extra, pos, _stream()), name)


class HeadRows:
    """The packed row list of a training step's score head (ick_head_rowmap), all int32 on the device:
    decode_len (B,), rowstart (B + 1,) with count = rowstart[B:] the number of valid rows M', rowmap (B * L,): packed row
    -> logical row b * L + t."""

    def __init__(self, lengths, B, Lc):
        dev = lengths.device
        lengths = lengths.reshape(-1)
        if lengths.dtype != torch.int64 or not lengths.is_contiguous():
            lengths = lengths.to(torch.int64).contiguous()
        assert lengths.numel() == B
        self.B, self.L = B, Lc
        self.decode_len = torch.empty(B, device=dev, dtype=torch.int32)
        self.rowstart = torch.empty(B + 1, device=dev, dtype=torch.int32)
        self.rowmap = torch.empty(B * Lc, device=dev, dtype=torch.int32)
        self.count = self.rowstart[B:]
        L.check(L.load().ick_head_rowmap(_p(lengths), B, Lc, _p(self.decode_len), _p(self.rowstart), _p(self.rowmap),
                                         _stream()), "ick_head_rowmap")


def gather_rows(x2, pack):
    """Packed copy of the valid rows of x2 (B * L, d): out[m] = x2[rowmap[m]] for m < M' (the rest is not written)."""
    rows, d = x2.shape
    assert x2.stride(1) == 1 and rows == pack.rowmap.numel()
    out = torch.empty(rows, d, device=x2.device, dtype=torch.float32)
    L.check(L.load().ick_gather_rows(_p(x2), x2.stride(0), _p(pack.rowmap), _p(pack.count), _p(out), d, rows, d,
                                     _stream()), "ick_gather_rows")
    return out


def packed_ce_rows(scores, captions, pack, pad_token, weights=None, want_grad=False, out_sum=None, out_count=None,
                   mean=None):
    """packed_ce / packed_ce_weighted over PACKED score rows (scores (B, L, Vx): the first M' rows of its B * L hold the
    valid positions in pack.rowmap's order): -> (loss_sum, count, dscores packed alike; rows from M' on are not written).
    mean: see _ce_mean."""
    B, Lc, Vx = scores.shape
    dev = scores.device
    if weights is not None and (weights.shape != (B,) or weights.dtype != torch.float32 or not weights.is_cuda or
                                not weights.is_contiguous()):
        raise L.IckError("packed_ce_rows needs contiguous (B,) float32 weights on the device")
    row_loss = torch.empty(B * Lc, device=dev, dtype=torch.float32)
    loss_sum = out_sum if out_sum is not None else torch.empty(1, device=dev, dtype=torch.float32)
    count = out_count if out_count is not None else torch.empty(1, device=dev, dtype=torch.float32)
    dscores = None
    assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1
    if want_grad:
        dscores = torch.empty(B, Lc, scores.stride(1), device=dev, dtype=torch.float32)[:, :, :Vx]
    name, tail = _ce_mean("ick_packed_ce_packed", mean)
    L.check(getattr(L.load(), name)(_p(scores), scores.stride(1), _p(captions), _p(pack.rowmap), _p(pack.count),
                                    _p(weights), B, Lc, Vx, pad_token, _p(row_loss), _p(loss_sum), _p(count), _p(dscores),
                                    *tail, _stream()), name)
    return loss_sum, count, dscores


def _ce_mean(name, mean):
    """The entry a loss wrapper calls and its extra argument.  mean: a one-element float32 device tensor; the reduction
    launch then also writes the token-mean loss into it (ick_*_mean; 0 for a batch without a token)."""
    if mean is None:
        return name, ()
    if mean.numel() != 1 or mean.dtype != torch.float32 or not mean.is_cuda:
        raise L.IckError("the loss's mean must be one float32 on the device")
    return name + "_mean", (_p(mean),)


def row_logprob_rank(scores, captions, pack, pad_token, out=None):
    """Per-token log-probability, rank and argmax of the PACKED score rows (scores (R, L, Vx) as _score_head(pack=) writes
    them; ick_row_logprob_rank) -> (token_log_probs f32, rank i32, best i32), each (R, L - 1) in LOGICAL order.  Only the
    elements of the pack's rows are written: caption_score_sums defines the rest.  out: the three tensors to write."""
    R, Lc, Vx = scores.shape
    dev = scores.device
    if captions.dtype != torch.int64 or not captions.is_contiguous() or tuple(captions.shape) != (R, Lc):
        raise L.IckError("row_logprob_rank needs contiguous int64 captions (%d, %d)" % (R, Lc))
    assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1 and pack.rowmap.numel() == R * Lc
    if out is None:
        out = (torch.empty(R, Lc - 1, device=dev, dtype=torch.float32),
               torch.empty(R, Lc - 1, device=dev, dtype=torch.int32),
               torch.empty(R, Lc - 1, device=dev, dtype=torch.int32))
    tlp, rank, best = out
    assert all(t.shape == (R, Lc - 1) and t.is_contiguous() for t in out)
    assert tlp.dtype == torch.float32 and rank.dtype == torch.int32 and best.dtype == torch.int32
    L.check(L.load().ick_row_logprob_rank(_p(scores), scores.stride(1), _p(captions), _p(pack.rowmap), _p(pack.count), R,
                                          Lc, Vx, pad_token, _p(tlp), _p(rank), _p(best), _stream()),
            "ick_row_logprob_rank")
    return tlp, rank, best


def caption_score_sums(pack, tlp, rank, best, top_k=5, out=None):
    """After row_logprob_rank: fills the positions past every caption, -> (log_prob (R,) f32, tokens (R,) i32, loss_sum,
    count, top1_hits, topk_hits (1,) f32 each) (ick_caption_score_sums).  out: (log_prob, tokens, totals (4,) f32)."""
    R, T = tlp.shape
    dev = tlp.device
    if out is None:
        out = (torch.empty(R, device=dev, dtype=torch.float32), torch.empty(R, device=dev, dtype=torch.int32),
               torch.empty(4, device=dev, dtype=torch.float32))
    log_prob, tokens, totals = out
    assert log_prob.shape == tokens.shape == (R,) and totals.shape == (4,) and totals.is_contiguous()
    assert log_prob.dtype == totals.dtype == torch.float32 and tokens.dtype == torch.int32
    assert pack.rowstart.numel() == R + 1 and tlp.is_contiguous() and rank.is_contiguous() and best.is_contiguous()
    L.check(L.load().ick_caption_score_sums(_p(pack.rowstart), R, T + 1, int(top_k), _p(tlp), _p(rank), _p(best),
                                            _p(log_prob), _p(tokens), _p(totals[0:1]), _p(totals[1:2]), _p(totals[2:3]),
                                            _p(totals[3:4]), _stream()), "ick_caption_score_sums")
    return log_prob, tokens, totals[0:1], totals[1:2], totals[2:3], totals[3:4]


def packed_ce(scores, captions_sorted, decode_len, pad_token, want_grad=False, out_sum=None, out_count=None, mean=None):
    """Returns (loss_sum (1,), count (1,), dscores or None): token-mean loss = loss_sum / count.  out_sum / out_count:
    one-element float tensors to receive the two scalars (the tail of TrainStep's gradient bucket).  mean: see _ce_mean
    (the weighted entry's form with no weights)."""
    B, Lc, Vx = scores.shape
    dev = scores.device
    row_loss = torch.empty(B * Lc, device=dev, dtype=torch.float32)
    loss_sum = out_sum if out_sum is not None else torch.empty(1, device=dev, dtype=torch.float32)
    count = out_count if out_count is not None else torch.empty(1, device=dev, dtype=torch.float32)
    dscores = None
    if want_grad:     # same (possibly padded) row stride as the scores: the kernel takes one leading dimension
        dscores = torch.empty(B, Lc, scores.stride(1), device=dev, dtype=torch.float32)[:, :, :Vx]
        assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1
    if mean is not None:
        name, tail = _ce_mean("ick_packed_ce_weighted", mean)
        L.check(getattr(L.load(), name)(_p(scores), scores.stride(1), _p(captions_sorted), _p(decode_len), None, B, Lc, Vx,
                                        pad_token, _p(row_loss), _p(loss_sum), _p(count), _p(dscores), *tail, _stream()),
                name)
        return loss_sum, count, dscores
    L.check(L.load().ick_packed_ce(_p(scores), scores.stride(1), _p(captions_sorted), _p(decode_len), B, Lc, Vx,
                                   pad_token, _p(row_loss), _p(loss_sum), _p(count), _p(dscores), _stream()),
            "ick_packed_ce")
    return loss_sum, count, dscores


def packed_ce_weighted(scores, captions_sorted, decode_len, weights, pad_token, want_grad=False, out_sum=None,
                       out_count=None, mean=None):
    """packed_ce with one fp32 weight per caption (weights (B,) on the device, any sign): loss_sum = sum over captions
    of weight * (sum of its token losses), count = the number of tokens (unweighted), dscores = weight * (softmax -
    onehot).  Weights of 1 give packed_ce's bits exactly (ick_packed_ce_weighted)."""
    B, Lc, Vx = scores.shape
    dev = scores.device
    if weights.shape != (B,) or weights.dtype != torch.float32 or not weights.is_cuda or not weights.is_contiguous():
        raise L.IckError("packed_ce_weighted needs contiguous (B,) float32 weights on the device")
    row_loss = torch.empty(B * Lc, device=dev, dtype=torch.float32)
    loss_sum = out_sum if out_sum is not None else torch.empty(1, device=dev, dtype=torch.float32)
    count = out_count if out_count is not None else torch.empty(1, device=dev, dtype=torch.float32)
    dscores = None
    if want_grad:
        dscores = torch.empty(B, Lc, scores.stride(1), device=dev, dtype=torch.float32)[:, :, :Vx]
        assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1
    name, tail = _ce_mean("ick_packed_ce_weighted", mean)
    L.check(getattr(L.load(), name)(_p(scores), scores.stride(1), _p(captions_sorted), _p(decode_len), _p(weights), B, Lc,
                                    Vx, pad_token, _p(row_loss), _p(loss_sum), _p(count), _p(dscores), *tail, _stream()),
            name)
    return loss_sum, count, dscores


def packed_ce_smooth(scores, captions, decode_len_or_pack, pad_token, eps, weights=None, want_grad=False, out_sum=None,
                     out_count=None, mean=None):
    """The packed cross entropy with label smoothing (ick_packed_ce_smooth; torch's CrossEntropyLoss(label_smoothing=)):
    row loss (1 - eps) * (lse - x[t]) + eps * (lse - mean(x)), gradient w * (softmax - (1 - eps) * onehot - eps / Vx).
    decode_len_or_pack: the int32 decode lengths (scores are the (B, L) rows, as packed_ce / packed_ce_weighted take them)
    or a HeadRows (scores hold its packed rows, as packed_ce_rows takes them).  eps: a ONE-element float32 device tensor,
    read by the kernel, so a captured launch follows the value written into it; 0.0 there gives the plain wrappers'
    bits."""
    B, Lc, Vx = scores.shape
    dev = scores.device
    if not isinstance(eps, torch.Tensor) or eps.numel() != 1 or eps.dtype != torch.float32 or not eps.is_cuda:
        raise L.IckError("packed_ce_smooth needs eps as a one-element float32 tensor on the device")
    if weights is not None and (weights.shape != (B,) or weights.dtype != torch.float32 or not weights.is_cuda or
                                not weights.is_contiguous()):
        raise L.IckError("packed_ce_smooth needs contiguous (B,) float32 weights on the device")
    pack = decode_len_or_pack if isinstance(decode_len_or_pack, HeadRows) else None
    row_loss = torch.empty(B * Lc, device=dev, dtype=torch.float32)
    loss_sum = out_sum if out_sum is not None else torch.empty(1, device=dev, dtype=torch.float32)
    count = out_count if out_count is not None else torch.empty(1, device=dev, dtype=torch.float32)
    dscores = None
    if pack is not None or want_grad:
        assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1
    if want_grad:
        dscores = torch.empty(B, Lc, scores.stride(1), device=dev, dtype=torch.float32)[:, :, :Vx]
    rowmap, rows, dl = (pack.rowmap, pack.count, None) if pack is not None else (None, None, decode_len_or_pack)
    name, tail = _ce_mean("ick_packed_ce_smooth", mean)
    L.check(getattr(L.load(), name)(_p(scores), scores.stride(1), _p(captions), _p(rowmap), _p(rows), _p(dl), _p(weights),
                                    _p(eps), B, Lc, Vx, pad_token, _p(row_loss), _p(loss_sum), _p(count), _p(dscores),
                                    *tail, _stream()), name)
    return loss_sum, count, dscores


def samples_to_captions(tokens, V, K, has_facts, start, end, pad, out=None):
    """Sampled rows tokens (R, T) int64 -> (captions (R, T+1), masks (R, T+1), lengths (R,)) int64 training rows
    (ick_samples_to_captions): [<start>, w_1 .. w_m, <end>, <pad> ..], length m + 2 (T + 1 without <end>); masks by
    predict()'s feedback rule.  out: the three tensors to write into."""
    R, T = tokens.shape
    if tokens.dtype != torch.int64 or not tokens.is_cuda or not tokens.is_contiguous():
        raise L.IckError("samples_to_captions needs a contiguous int64 (R, T) device tensor")
    if out is None:
        out = (torch.empty(R, T + 1, device=tokens.device, dtype=torch.int64),
               torch.empty(R, T + 1, device=tokens.device, dtype=torch.int64),
               torch.empty(R, device=tokens.device, dtype=torch.int64))
    caps, masks, lengths = out
    assert caps.shape == masks.shape == (R, T + 1) and lengths.shape == (R,)
    assert caps.is_contiguous() and masks.is_contiguous() and lengths.is_contiguous()
    L.check(L.load().ick_samples_to_captions(_p(tokens), R, T, V, K, int(bool(has_facts)), start, end, pad, _p(caps),
                                             _p(masks), _p(lengths), _stream()),
            "ick_samples_to_captions")
    return caps, masks, lengths


SCHED_SAMPLE_MODES = ("sample", "argmax")


def sched_sample_mix(scores, pack, captions, caption_masks, V, K, F, start_token, pad_token, prob, temperature, seed,
                     step, mode="sample", out=None):
    """Scheduled sampling's mixed inputs (ick_sched_sample_mix) from the PACKED score rows of a
    teacher-forced pass (scores (B, L, Vx) as _score_head(pack=) writes them, pack: the HeadRows) and the gold captions /
    caption_masks (B, L) int64 -> (captions_in, masks_in int64, replaced int32), each (B, L) and written whole.  prob,
    temperature (float32), seed (int64) and step (int32, read as uint32: TrainStep's counter) are ONE-element device
    tensors the kernel reads, so a captured launch follows new values; mode ("sample" | "argmax") is fixed at launch.
    out: the three tensors to write."""
    B, Lc, Vx = scores.shape
    dev = scores.device
    if mode not in SCHED_SAMPLE_MODES:
        raise L.IckError("sched_sample_mix: unknown mode %r (one of %s)" % (mode, ", ".join(SCHED_SAMPLE_MODES)))
    if Vx != V + K + F:
        raise L.IckError("sched_sample_mix: scores have %d columns, V + K + F is %d" % (Vx, V + K + F))
    for name, t in (("captions", captions), ("caption_masks", caption_masks)):
        if t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous() or tuple(t.shape) != (B, Lc):
            raise L.IckError("sched_sample_mix needs contiguous int64 %s (%d, %d) on the device" % (name, B, Lc))
    for name, t, dt in (("prob", prob, torch.float32), ("temperature", temperature, torch.float32),
                        ("seed", seed, torch.int64), ("step", step, torch.int32)):
        if not isinstance(t, torch.Tensor) or t.numel() != 1 or t.dtype != dt or not t.is_cuda:
            raise L.IckError("sched_sample_mix needs %s as a one-element %s tensor on the device" % (name, dt))
    # all B * L rows of the buffer exist (the valid ones packed at its top): the kernel's row bound relies on it
    assert scores.stride(0) == Lc * scores.stride(1) and scores.stride(2) == 1
    assert pack.B == B and pack.L == Lc
    if out is None:
        out = (torch.empty(B, Lc, device=dev, dtype=torch.int64), torch.empty(B, Lc, device=dev, dtype=torch.int64),
               torch.empty(B, Lc, device=dev, dtype=torch.int32))
    caps_in, masks_in, replaced = out
    assert all(tuple(t.shape) == (B, Lc) and t.is_contiguous() for t in out)
    assert caps_in.dtype == masks_in.dtype == torch.int64 and replaced.dtype == torch.int32
    L.check(L.load().ick_sched_sample_mix(_p(scores), scores.stride(1), _p(pack.rowstart), _p(pack.decode_len),
                                          _p(captions), _p(caption_masks), B, Lc, V, K, F, start_token, pad_token,
                                          _p(prob), _p(temperature), _p(seed), _p(step), int(mode == "argmax"),
                                          _p(caps_in), _p(masks_in), _p(replaced), _stream()), "ick_sched_sample_mix")
    return caps_in, masks_in, replaced


CIDER_MODES = {None: 0, "greedy": 1, "mean": 2}


def cider_d(tokens, refs, keys, counts, log_ref_len, sigma, start, end, pad, ignore=(), image_index=None,
            num_samples=0, baseline=None):
    """CIDEr-D of candidate rows tokens (N, T) against refs (B, M, Lr) (ick_cider_d; the metric: cider.py).  keys (U, 4)
    int32 (the uint32 df-table keys), counts (U,) int32, all int64 / int32 device tensors.  Returns (rewards (N,) f32,
    advantages (B * num_samples,) f32 or None).
    baseline=None: general mode, row i against image image_index[i] ((N,) int32 on the device).
    baseline="greedy" / "mean": the SCST layout (rows b * n + j, then with "greedy" the B greedy rows)."""
    if baseline not in CIDER_MODES:
        raise L.IckError('baseline must be None, "greedy" or "mean"')
    for t, name, dt in ((tokens, "tokens", torch.int64), (refs, "refs", torch.int64), (keys, "keys", torch.int32),
                        (counts, "counts", torch.int32)):
        if t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise L.IckError("cider_d: %s must be a contiguous %s device tensor" % (name, dt))
    if tokens.dim() != 2 or refs.dim() != 3 or keys.dim() != 2 or keys.shape[1] != 4 or counts.shape != keys.shape[:1]:
        raise L.IckError("cider_d needs tokens (N, T), refs (B, M, Lr), keys (U, 4) and counts (U,)")
    ignore = [int(i) for i in ignore]
    if len(ignore) > 16:
        raise L.IckError("cider_d takes at most 16 ignore ids")
    N, T = tokens.shape
    B, M, Lr = refs.shape
    dev = tokens.device
    mode = CIDER_MODES[baseline]
    idx = None
    if mode == 0:
        if image_index is None or image_index.shape != (N,):
            raise L.IckError("cider_d: general mode needs an (N,) image_index")
        idx = image_index.to(device=dev, dtype=torch.int32).contiguous()
    rewards = torch.empty(N, device=dev, dtype=torch.float32)
    adv = torch.empty(B * num_samples, device=dev, dtype=torch.float32) if mode else None
    ign = (C.c_int32 * 16)(*ignore)
    L.check(L.load().ick_cider_d(_p(tokens), N, T, _p(refs), B, M, Lr, _p(keys), _p(counts), keys.shape[0],
                                 float(log_ref_len), float(sigma), start, end, pad, ign, len(ignore), mode, _p(idx),
                                 int(num_samples), _p(rewards), _p(adv), _stream()),
            "ick_cider_d")
    return rewards, adv


def caption_metrics(tokens, refs, start, end, pad, ignore=(), pointer_base=-1, beta=1.2, image_index=None,
                    num_samples=0, baseline=None, base_rewards=None, weights=None):
    """BLEU components and sentence scores, ROUGE-L and pointer counts of candidate rows tokens (N, T) against refs
    (B, M, Lr) (ick_caption_metrics; the definitions: metrics.py), all int64 device tensors.  Returns (counts (N, 10)
    i32, bleu (N, 4) f32, rouge_l (N,) f32, pointers (N, 3) i32, rewards (N,) f32 or None, advantages (B * num_samples,)
    f32 or None).  baseline / image_index / num_samples: cider_d's modes.  weights: six floats w_base, w_b1..w_b4, w_rouge
    -> rewards (and, in the SCST layout, advantages); base_rewards (N,) f32: cider_d's rewards of the same rows."""
    if baseline not in CIDER_MODES:
        raise L.IckError('baseline must be None, "greedy" or "mean"')
    for t, name in ((tokens, "tokens"), (refs, "refs")):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.int64 or not t.is_cuda or not t.is_contiguous():
            raise L.IckError("caption_metrics: %s must be a contiguous int64 device tensor" % name)
    if tokens.dim() != 2 or refs.dim() != 3:
        raise L.IckError("caption_metrics needs tokens (N, T) and refs (B, M, Lr)")
    ignore = [int(i) for i in ignore]
    if len(ignore) > 16:
        raise L.IckError("caption_metrics takes at most 16 ignore ids")
    N, T = tokens.shape
    B, M, Lr = refs.shape
    dev = tokens.device
    mode = CIDER_MODES[baseline]
    idx = None
    if mode == 0:
        if image_index is None or image_index.shape != (N,):
            raise L.IckError("caption_metrics: general mode needs an (N,) image_index")
        idx = image_index.to(device=dev, dtype=torch.int32).contiguous()
    w = rewards = adv = None
    if weights is not None:
        weights = [float(x) for x in weights]
        if len(weights) != 6 or not all(math.isfinite(x) for x in weights):
            raise L.IckError("caption_metrics: weights are six finite floats (w_base, w_b1..w_b4, w_rouge)")
        w = (C.c_float * 6)(*weights)
        rewards = torch.empty(N, device=dev, dtype=torch.float32)
        adv = torch.empty(B * num_samples, device=dev, dtype=torch.float32) if mode else None
    if base_rewards is not None:
        if weights is None:
            raise L.IckError("caption_metrics: base_rewards need weights")
        if base_rewards.shape != (N,) or base_rewards.dtype != torch.float32 or not base_rewards.is_cuda or \
                not base_rewards.is_contiguous():
            raise L.IckError("caption_metrics: base_rewards must be a contiguous (N,) float32 device tensor")
    counts = torch.empty(N, 10, device=dev, dtype=torch.int32)
    bleu = torch.empty(N, 4, device=dev, dtype=torch.float32)
    rouge = torch.empty(N, device=dev, dtype=torch.float32)
    pointers = torch.empty(N, 3, device=dev, dtype=torch.int32)
    ign = (C.c_int32 * 16)(*ignore)
    L.check(L.load().ick_caption_metrics(_p(tokens), N, T, _p(refs), B, M, Lr, start, end, pad, ign, len(ignore),
                                         int(pointer_base), float(beta), mode, _p(idx), int(num_samples),
                                         _p(base_rewards), w, _p(counts), _p(bleu), _p(rouge), _p(pointers),
                                         _p(rewards), _p(adv), _stream()), "ick_caption_metrics")
    return counts, bleu, rouge, pointers, rewards, adv


def caption_metric_sums(counts, rouge_l, pointers, out=None):
    """Totals of caption_metrics' rows (ick_caption_metric_sums) -> (sums (14,) int64: the ten BLEU components, the three
    pointer counts and the number of rows counted; rouge_sum (1,) float64), on the device.  Rows with a NaN rouge_l are
    skipped.  out: the two tensors to write."""
    for t, dt, name in ((counts, torch.int32, "counts"), (rouge_l, torch.float32, "rouge_l"),
                        (pointers, torch.int32, "pointers")):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or not t.is_cuda or not t.is_contiguous():
            raise L.IckError("caption_metric_sums: %s must be a contiguous %s device tensor" % (name, dt))
    N = rouge_l.shape[0] if rouge_l.dim() == 1 else -1
    if N < 1 or tuple(counts.shape) != (N, 10) or tuple(pointers.shape) != (N, 3):
        raise L.IckError("caption_metric_sums needs counts (N, 10), rouge_l (N,) and pointers (N, 3), N >= 1")
    dev = counts.device
    if out is None:
        out = (torch.empty(14, device=dev, dtype=torch.int64), torch.empty(1, device=dev, dtype=torch.float64))
    sums, rouge_sum = out
    assert sums.shape == (14,) and sums.dtype == torch.int64 and sums.is_contiguous()
    assert rouge_sum.shape == (1,) and rouge_sum.dtype == torch.float64
    L.check(L.load().ick_caption_metric_sums(_p(counts), _p(rouge_l), _p(pointers), N, _p(sums), _p(rouge_sum),
                                             _p(sums[13:14]), _stream()), "ick_caption_metric_sums")
    return sums, rouge_sum


GEO_TERMS, GEO_NAME_CHARS, GEO_MAX_T, GEO_MAX_K, GEO_MAX_BINS, GEO_MAX_TYPES = 8, 50, 128, 4095, 64, 4096


def geo_reference_counts(tokens, image_index, entities, entity_names, V, trigger_ids, of_id, the_id, a_id,
                         bins_distance, bins_azimuth, n_types, seed=0, row_offset=0):
    """The geo-reference histograms of caption rows tokens (N, T) int64 (ick_geo_reference_counts; the definition:
    geo_metric.py).  image_index (N,) row -> image; entities (B, K, C) float32; entity_names (B, K, 52) int64;
    trigger_ids: the 8 terms' word ids (-1: absent); bins_distance / bins_azimuth: (n, 2) float64 device tables.
    Returns (generated, random, marks): two (8, 1 + 64 + 64 + n_types rounded up to 64) int32 histograms and the
    (N, T) int32 marks.  Everything is checked before the launch; nothing is read back."""
    for t, name, dt, nd in ((tokens, "tokens (N, T)", torch.int64, 2), (entities, "entities (B, K, C)", torch.float32, 3),
                            (entity_names, "entity_names (B, K, 52)", torch.int64, 3),
                            (bins_distance, "bins_distance (n, 2)", torch.float64, 2),
                            (bins_azimuth, "bins_azimuth (n, 2)", torch.float64, 2)):
        if not isinstance(t, torch.Tensor) or t.dtype != dt or t.dim() != nd or not t.is_cuda or not t.is_contiguous():
            raise L.IckError("geo_reference_counts: %s must be a contiguous %s device tensor" % (name, dt))
    N, T = tokens.shape
    B, K, Cf = entities.shape
    if N < 1 or not 1 <= T <= GEO_MAX_T:
        raise L.IckError("geo_reference_counts: N >= 1 and 1 <= T <= %d (got %d, %d)" % (GEO_MAX_T, N, T))
    if B < 1 or not 1 <= K <= GEO_MAX_K or Cf < 5:
        raise L.IckError("geo_reference_counts: entities need B >= 1, 1 <= K <= %d and C >= 5" % GEO_MAX_K)
    if tuple(entity_names.shape) != (B, K, 2 + GEO_NAME_CHARS):
        raise L.IckError("geo_reference_counts: entity_names must be (%d, %d, %d)" % (B, K, 2 + GEO_NAME_CHARS))
    for t, name in ((bins_distance, "bins_distance"), (bins_azimuth, "bins_azimuth")):
        if t.shape[1] != 2 or not 1 <= t.shape[0] <= GEO_MAX_BINS:
            raise L.IckError("geo_reference_counts: %s holds 1..%d [lo, hi] rows" % (name, GEO_MAX_BINS))
    if isinstance(n_types, bool) or not isinstance(n_types, int) or not 1 <= n_types <= GEO_MAX_TYPES:
        raise L.IckError("geo_reference_counts: 1 <= n_types <= %d" % GEO_MAX_TYPES)
    trigger_ids = [int(i) for i in trigger_ids]
    ids = trigger_ids + [int(of_id), int(the_id), int(a_id)]
    if len(trigger_ids) != GEO_TERMS or not isinstance(V, int) or V < 1 or not all(-1 <= i < V for i in ids):
        raise L.IckError("geo_reference_counts: 8 trigger ids and the ids of of / the / a, each -1 or in [0, V)")
    if not isinstance(image_index, torch.Tensor) or image_index.shape != (N,):
        raise L.IckError("geo_reference_counts needs an (N,) image_index")
    if not 0 <= int(row_offset) <= 2 ** 62 or not -2 ** 63 <= int(seed) < 2 ** 64:
        raise L.IckError("geo_reference_counts: row_offset >= 0 and a 64-bit seed")
    dev = tokens.device
    idx = image_index.to(device=dev, dtype=torch.int32).contiguous()
    seed = int(seed) & (2 ** 64 - 1)
    seed -= 2 ** 64 if seed >= 2 ** 63 else 0
    ld = 1 + 2 * GEO_MAX_BINS + (n_types + 63) // 64 * 64
    hist = torch.zeros(2, GEO_TERMS, ld, device=dev, dtype=torch.int32)
    marks = torch.empty(N, T, device=dev, dtype=torch.int32)
    trig = (C.c_int32 * GEO_TERMS)(*trigger_ids)
    L.check(L.load().ick_geo_reference_counts(_p(tokens), N, T, _p(idx), _p(entities), _p(entity_names), B, K, Cf, V, trig,
                                              int(of_id), int(the_id), int(a_id), _p(bins_distance),
                                              bins_distance.shape[0], _p(bins_azimuth), bins_azimuth.shape[0], n_types,
                                              ld, seed, int(row_offset), _p(marks), _p(hist[0]), _p(hist[1]), _stream()),
            "ick_geo_reference_counts")
    return hist[0], hist[1], marks


# ------------------------------------------------------------------------------------------------
# Backward / training-step wrappers
# ------------------------------------------------------------------------------------------------
def attention_bwd_buffer(shape, T, S, dh, device):
    """Gradient buffer for attention_heads_bwd: uninitialised when the kernel chosen for (T, S, dh) writes every
    element, zeroed when it accumulates query chunks with atomics."""
    if L.load().ick_attention_bwd_overwrites(T, S, dh):
        return torch.empty(shape, device=device, dtype=torch.float32)
    return torch.zeros(shape, device=device, dtype=torch.float32)


ATTN_PLAN_KEYS = ("mfma", "nqt", "maxt", "dhp", "tq", "chunks", "overwrites")


def attention_plan(direction, T, S, dh, head_major=True):
    """The kernels ick_attention (direction "fwd") / ick_attention_bwd ("bwd") launch for a (T, S, dh) problem
    (ick_attention_plan; host only, no GPU needed).  None when the entry point rejects the shape."""
    out = (C.c_int32 * len(ATTN_PLAN_KEYS))()
    rc = L.load_raw().ick_attention_plan({"fwd": 0, "bwd": 1}[direction], T, S, dh, int(head_major), out)
    if rc == -1:
        return None
    L.check(rc, "ick_attention_plan")
    return dict(zip(ATTN_PLAN_KEYS, (int(v) for v in out)))


def attention_heads_bwd(q, kv, O, dO, lse, dQ, dK, dV, H, dh, T, S, q_seg=0, k_seg=0, v_seg=1, causal=False,
                        drop=None, q_pos0=0):
    """Backward of attention_heads.  q (B,nq,H,Tq,DHP), kv (B,nkv,H,Sa,DHP); O/dO (B,T,d) row-major;
    dQ (B,T,*) / dK, dV (B,S,*) row-major views (last-dim stride 1; their column offset selects the
    segment), written as [h*dh + j].  The head-major buffers' row stride is DHP (dh <= 32) or 2 DHP."""
    if ATTN_LOG is not None:
        ATTN_LOG.append(("bwd", T, S, dh, bool(causal)))
    B = q.shape[0]
    Tq, Sa = q.shape[3], kv.shape[3]
    hp = q.shape[4]
    assert kv.shape[4] == hp
    a = L.AttnBwdArgs()
    a.Q = q.data_ptr() + 4 * (q_seg * H * Tq * hp)
    a.K = kv.data_ptr() + 4 * (k_seg * H * Sa * hp)
    a.V = kv.data_ptr() + 4 * (v_seg * H * Sa * hp)
    a.O, a.dO, a.lse = _p(O), _p(dO), _p(lse)
    a.dQ, a.dK, a.dV = _p(dQ), _p(dK), _p(dV)
    a.B, a.H, a.T, a.S, a.dh = B, H, T, S, dh
    a.q_bs, a.q_hs, a.q_ts = q.stride(0), Tq * hp, hp
    a.k_bs, a.k_hs, a.k_ss = kv.stride(0), Sa * hp, hp
    a.v_bs, a.v_hs, a.v_ss = kv.stride(0), Sa * hp, hp
    a.o_bs, a.o_ts = O.stride(0), O.stride(1)
    a.dq_bs, a.dq_ts = dQ.stride(0), dQ.stride(1)
    a.dk_bs, a.dk_ss = dK.stride(0), dK.stride(1)
    a.dv_bs, a.dv_ss = dV.stride(0), dV.stride(1)
    a.scale = 1.0 / math.sqrt(dh)
    a.causal, a.q_pos0 = int(causal), q_pos0
    _drop(a, drop)
    L.check(L.load().ick_attention_bwd(C.byref(a), _stream()), "ick_attention_bwd")


def layernorm_bwd(dy, x, res, gamma, mean, rstd, dgamma, dbeta, drop=None):
    """Returns (dz, dx): dz = gradient of the residual operand (and of z), dx = gradient of the operand the
    forward applied dropout to.  dx is always its own tensor (a copy of dz without dropout): dz is accumulated
    into in place by the next data-gradient GEMM while dx is still being read by weight-gradient kernels on the
    side stream.  The per-workgroup dgamma / dbeta partial sums are reduced by two column sums (side stream)."""
    d = x.shape[-1]
    rows = x.numel() // d
    dz = torch.empty_like(x)
    dxd = torch.empty_like(x)
    rpb = L.load().ick_layernorm_bwd_rows_per_block()
    part = torch.empty((rows + rpb - 1) // rpb, 2 * d, device=x.device, dtype=torch.float32)
    L.check(L.load().ick_layernorm_bwd(_p(dy), _p(x), _p(res), _p(gamma), _p(mean), _p(rstd), _p(dz), None, None,
                                       rows, d, _p(dxd), *_dargs(drop), _p(part), _stream()), "ick_layernorm_bwd")

    if SIDE is not None:
        SIDE.flush()     # side work marked earlier goes out now that the main chain has its next kernel
    ln_partials_reduce(part, dgamma, dbeta)
    return dz, dxd


def ln_partials_reduce(part, dgamma, dbeta):
    """dgamma / dbeta += column sums of the per-workgroup partials (rows x 2d) of a LayerNorm backward: inside the layer's
    grouped weight-gradient launch when a SideStream is installed (no kernel of their own), else two column sums."""
    d = part.shape[1] // 2
    adjacent = dbeta.data_ptr() == dgamma.data_ptr() + 4 * d      # adjacent in a flat gradient bucket: one problem
    if SIDE is not None:
        if adjacent:
            SIDE.add_problem(colsum_problem(part, dgamma), part)
        else:
            SIDE.add_problem(colsum_problem(part[:, :d], dgamma), part)
            SIDE.add_problem(colsum_problem(part[:, d:], dbeta), part)
    elif adjacent:
        colsum(part, dgamma, n_out=2 * d)
    else:
        colsum(part[:, :d], dgamma)
        colsum(part[:, d:], dbeta)


def relu_bwd(dy, act, out=None, scale=1.0):
    if out is None:
        out = torch.empty_like(dy)
    L.check(L.load().ick_relu_bwd(_p(dy), _p(act), _p(out), dy.numel(), scale, _stream()), "ick_relu_bwd")
    return out


def dropout_mask(rows, cols, p, seed, site, device="cuda"):
    out = torch.empty(rows, cols, device=device, dtype=torch.float32)
    L.check(L.load().ick_dropout_mask(_p(out), rows, cols, p, seed & 0xFFFFFFFF, site & 0xFFFFFFFF, _stream()),
            "ick_dropout_mask")
    return out


def colsum(a2d, out, n_out=None):
    """out[n] += sum_m a2d[m, n] for a row-major 2-D view (n_out: out really has that many elements from its
    data pointer on, e.g. two adjacent gradient buffers)."""
    M, N = a2d.shape
    assert (n_out or out.numel()) >= N
    L.check(L.load().ick_colsum(_p(a2d), M, N, a2d.stride(0), _p(out), _stream()), "ick_colsum")
    return out


# ------------------------------------------------------------------------------------------------
# Diagnostic time stamps (ICK_TIMESTAMPS=1): device wall-clock marks on whatever stream is current
# ------------------------------------------------------------------------------------------------
STAMPS = None   # {"buf": int64 tensor, "names": [...]} while enabled


def stamps_enable(n=512):
    global STAMPS
    STAMPS = {"buf": torch.zeros(n, device="cuda", dtype=torch.int64), "names": []}


def stamp(name):
    """Mark the current point of the current stream (no-op unless stamps_enable() was called)."""
    if STAMPS is None or len(STAMPS["names"]) >= STAMPS["buf"].numel():
        return
    i = len(STAMPS["names"])
    STAMPS["names"].append(name)
    L.check(L.load().ick_timestamp(STAMPS["buf"][i:].data_ptr(), _stream()), "ick_timestamp")


def stamps_report():
    """[(name, microseconds since the first stamp)] sorted by time."""
    t = STAMPS["buf"][:len(STAMPS["names"])].cpu().tolist()
    t0 = min(x for x in t if x > 0)
    return sorted(((n, (x - t0) / 100.0) for n, x in zip(STAMPS["names"], t)), key=lambda p: p[1])


def copy_batch(dst, src):
    """dst[i].copy_(src[i]) for up to 8 pairs of contiguous same-sized device tensors per launch (ick_copy_batch)."""
    for i in range(0, len(dst), 8):
        d, s_ = dst[i:i + 8], src[i:i + 8]
        n = len(d)
        sp = (C.c_void_p * n)(*[t.data_ptr() for t in s_])
        dp = (C.c_void_p * n)(*[t.data_ptr() for t in d])
        nb = (C.c_longlong * n)(*[t.numel() * t.element_size() for t in d])
        L.check(L.load().ick_copy_batch(sp, dp, nb, n, _stream()), "ick_copy_batch")


@contextlib.contextmanager
def capture(graph):
    """torch.cuda.graph(graph) for the package's hipGraph captures, with Python's cyclic garbage collector held off until
    the capture has ended.  A collection that starts inside the capture region may finalise objects of EARLIER work that
    sit in reference cycles -- a finished TrainStep's CUDAGraph, its streams -- and destroying those while the thread's
    stream is capturing aborts the process (seen once in the full GPU suite: `Fatal Python error: Aborted`,
    `Garbage-collecting`, inside a captured backward pass).  torch.cuda.graph itself collects right before it begins the
    capture, so nothing is left waiting; whatever the captured function leaves behind is collected after capture_end.
    thread_local: other threads (the RCCL watchdog) may touch the HIP runtime while this one captures."""
    was = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(graph, capture_error_mode="thread_local"):
            yield
    finally:
        if was:
            gc.enable()


class SideStream:
    """Second HIP stream for work that is off the critical path: in the backward pass the weight and bias
    gradients of a Linear only feed the optimizer, while the data gradient feeds the next layer's backward.

    fork(): the side stream waits for everything enqueued so far on the main stream (or for an earlier mark());
    join(): the main stream waits for the side stream (before the all-reduce / optimizer).
    submit()/flush(): deferred form -- the dependency point is marked now, the side work is enqueued at the next
    flush().  Callers flush right *after* enqueuing the next main-stream kernel, so that in a captured graph the
    main chain is the first child of every node: hipGraph keeps a node's first child on the parent's queue,
    and a hop to another queue costs ~15 us of idle time on the critical path."""

    def __init__(self, priority=0):
        # priority -1: the chain of small kernels on the side stream competes with a large GEMM on the main stream
        # for workgroup slots; a high-priority queue gets its workgroups dispatched first
        # ICK_GROUP_SAME_STREAM=1 (bench.py's per-kernel pass): same grouping and launch order as the captured step, but
        # everything on the caller's stream, so that HIP events around a launch time that launch alone
        self.stream = torch.cuda.current_stream() if os.environ.get("ICK_GROUP_SAME_STREAM") else \
            torch.cuda.Stream(priority=priority)
        self.pending = False
        self.keep = []   # tensors the side stream reads stay referenced until the pass ends, so the caching
                         # allocator cannot hand their memory to the main stream meanwhile (also under capture)
        self.deferred = []
        self.group = []  # weight-gradient problems (ick_gemm_args) waiting for the next flush_group()
        self.signals = {}

    def add_problem(self, args, *tensors):
        """Queue a GEMM whose operands are complete on the main stream by the next flush_group()."""
        self.group.append(args)
        self.keep.extend(t for t in tensors if t is not None)

    def flush_group(self):
        """One grouped launch (ick_gemm_grouped) of the queued problems on the side stream, ordered after
        everything enqueued so far on the main stream; like submit() it is enqueued at the next flush()."""
        if self.group:
            problems, self.group = self.group, []

            def launch():
                stamp("side: group of %d starts" % len(problems))
                gemm_grouped(problems)
                stamp("side: group of %d done" % len(problems))

            self.deferred.append((self.mark(), launch, ()))

    def flush_group_here(self):
        """The queued problems as one grouped launch on the CALLER's stream, right now: for the tail of a pass, where the
        main stream has run out of work and the side stream is what finishes last."""
        if self.group:
            problems, self.group = self.group, []
            gemm_grouped(problems)

    def mark(self):
        """Event at the current point of the main stream, for a later fork(..., after=event)."""
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream())
        return ev

    def fork(self, *tensors, after=None):
        ev = after if after is not None else self.mark()
        self.stream.wait_event(ev)
        self.keep.extend(t for t in tensors if t is not None)
        self.pending = True
        return torch.cuda.stream(self.stream)

    def signal(self, key):
        """Called from work running on the side stream: marks `key` as done at this point of it."""
        ev = torch.cuda.Event()
        ev.record(self.stream)
        self.signals[key] = ev

    def wait(self, key):
        """The main stream waits for the point signal(key) marked (no-op for keys never signalled)."""
        ev = self.signals.get(key)
        if ev is not None:
            torch.cuda.current_stream().wait_event(ev)

    def wait_or_join(self, key):
        """The main stream waits for signal(key) if deferred work signalled it (after enqueuing that work), else for
        the whole side stream."""
        self.flush_group()
        self.flush()
        if key in self.signals:
            self.wait(key)
        else:
            self.join()

    def submit(self, fn, *tensors):
        self.deferred.append((self.mark(), fn, tensors))

    def flush(self):
        work, self.deferred = self.deferred, []
        for ev, fn, tensors in work:
            with self.fork(*tensors, after=ev):
                fn()

    def join(self):
        self.flush_group()
        self.flush()
        if self.pending:
            torch.cuda.current_stream().wait_stream(self.stream)
            self.pending = False


SIDE = None   # set by training.TrainStep / backward_from_tape for the duration of a backward pass


def linear_bwd(dy, x, w, dw, db, need_dx=True, dx=None, accumulate_dx=False, group_now=False, gate=None,
               gate_scale=1.0, wt_ps=None, xt_ps=None, pack=None, valid=None):
    """Backward of y = x @ w.T + b for row-major 2-D views dy (M,N), x (M,K), w (N,K):
    dw += dy.T @ x (split-K over M, float atomics), db += colsum(dy), dx = dy @ w.
    With a SideStream installed the two parameter gradients run beside the data gradient.
    wt_ps: the pre-split copy of w.t() (presplit_weights) -- the data gradient's B operand.
    xt_ps: the pre-split copy of x.t() -- the weight gradient's B operand: dw then runs on csrc/gemm_ps.hip's kernel (the
    vocabulary: 10 000 x 300 outputs over 1 280 rows) and db becomes a column-sum problem of the same group.
    pack (HeadRows; the packed score head): dy holds the M' = pack.count valid rows packed at its top, x and dx keep their
    logical rows.  The reductions of dw / db run over M' rows (xt_ps must have been gathered through pack.rowmap; without
    it the rows of x are read in place through the k-line map of csrc/gemm.hip, b_kmap), dx is computed for M' rows and scattered through pack.rowmap into a dx that the
    caller zeroed (accumulate_dx): the rows of padded positions stay exactly zero.
    valid (HeadRows; the decoder layers below a packed head): dy and x both keep their logical rows, and the rows of dy
    that valid.rowmap does not list are exactly zero: dw / db reduce over the valid.count listed rows of
    both operands, read in place through the k-line maps of csrc/gemm.hip.  The data gradient is not touched."""
    M, N = dy.shape
    K = x.shape[1]
    assert pack is None or valid is None
    kb = pack.count if pack is not None else (valid.count if valid is not None else None)
    assert pack is None or (need_dx and dx is not None and accumulate_dx and gate is None)
    assert valid is None or (xt_ps is None and valid.rowmap.numel() == M)

    # dw += dy.T @ x with db += colsum(dy) riding on the first tile column of the same kernel
    wg = None
    extra = []
    if dw is not None and xt_ps is not None and gemm_split_mode() >= 1 and not is_deterministic():
        # 128 x 128 tiles, two workgroups per CU: K slices so that the ~512 slots of the chip are taken once
        tiles = ((N + 127) // 128) * ((K + 127) // 128)
        split = max(1, min(8, 480 // tiles, M // 512))
        wg = gemm_args(dy, x, dw, N, K, M, 1, dy.stride(0), 1, x.stride(0), dw.stride(0), atomic=True,
                       split_k=split, b_ps=xt_ps, k_bound=kb)
        if db is not None:
            extra.append(colsum_problem(dy, db, split_k=max(1, min(16, M // 256)), k_bound=kb))
    elif dw is not None:
        # pack: dy is packed, the k-major B operand gathers the logical rows of x through the row list; valid: both do
        rows = pack if pack is not None else valid
        split = wgrad_split(M, N, K, grouped=SIDE is not None)
        if valid is not None:
            split = min(split, VALID_ROW_WGRAD_SLICES)
        wg = gemm_args(dy, x, dw, N, K, M, 1, dy.stride(0), 1, x.stride(0), dw.stride(0), atomic=True,
                       split_k=split, colsum_a=db, k_bound=kb,
                       a_kmap=valid.rowmap if valid is not None else None,
                       b_kmap=rows.rowmap if rows is not None else None)

    def param_grads():
        if wg is not None and extra:
            gemm_grouped([wg] + extra)
        elif wg is not None:
            _log_plan(wg)
            L.check(L.load().ick_gemm(C.byref(wg), _stream()), "ick_gemm(wgrad)")
        elif db is not None:
            if pack is not None:
                gemm_grouped([colsum_problem(dy, db, k_bound=kb)])
            else:
                colsum(dy, db)

    # With a SideStream the weight gradients of a whole layer are queued and go out as one grouped launch at the
    # layer's end (SideStream.flush_group): each alone is a ~15 us latency-bound kernel, and every fork point of
    # the captured graph costs the main chain ~4 us.  The main stream never waits for the side stream until the
    # pass ends.
    overlap = SIDE is not None and (dw is not None or db is not None)
    if overlap:
        if wg is not None:
            SIDE.add_problem(wg, dy, x, xt_ps)
            for e in extra:
                SIDE.add_problem(e, dy)
            if group_now:      # a large problem of its own (the vocabulary): runs beside its data gradient
                SIDE.flush_group()
        else:
            SIDE.submit(param_grads, dy, x)
    if need_dx:
        # packed rows: M' of them, row m lands in row pack.rowmap[m] of dx
        scatter = {} if pack is None else dict(m_bound=kb, c_grp=1, c_gs=dx.stride(0), c_gmap=pack.rowmap)
        # a long reduction (the vocabulary: N = 10k..50k) over few output tiles is split over workgroups
        split = max(1, min(16, N // 1024)) if (M * K) <= 1280 * 512 else 1
        if is_deterministic():
            split = 1
        elif accumulate_dx and split == 1 and N >= 512 and (M * K) <= 1280 * 512:
            # the output already holds the residual-path gradient: K slices of ~300 can simply add to it
            # (1280 x 300 x 900: 22 -> ~10 us; the kernel is bound by the latency of its K loop)
            split = max(1, min(8, (N + 150) // 300))
        if wt_ps is not None and split > 1 and gemm_split_mode() >= 1 and K <= 320:
            # the pre-split kernel (the plan picks its 128 x 80 tile for split-K problems at most 320 columns wide): K slices
            # so that row tiles x 4 column tiles x slices take the chip's ~512 two-per-CU slots once (cfg2: 10 x 4 x 12)
            split = max(1, min(16, N // 512, 256 // ((M + 63) // 64)))
        if split > 1:
            if dx is None:
                dx = torch.zeros(M, K, device=dy.device, dtype=torch.float32)
            elif not accumulate_dx:
                dx.zero_()
            gemm_raw(dy, w, dx, M, K, N, dy.stride(0), 1, 1, w.stride(0), dx.stride(0), atomic=True, split_k=split,
                     b_ps=wt_ps, **scatter)
        else:
            if dx is None:
                dx = torch.empty(M, K, device=dy.device, dtype=torch.float32)
            # gate: the consumer wants ReLU'(act) * dx (FFN inner activation): applied in the epilogue
            gemm_raw(dy, w, dx, M, K, N, dy.stride(0), 1, 1, w.stride(0), dx.stride(0), accumulate=accumulate_dx,
                     gate=gate, gate_scale=gate_scale, **scatter)
            gate = None
    if not overlap:
        param_grads()
    if gate is not None:        # split-K path: the gate cannot ride on partial sums
        relu_bwd(dx, gate, out=dx, scale=gate_scale)
    return dx


def caption_embed_bwd(dx, captions, masks, dword, dee, dfe, V, pad_token, scale, drop=None):
    B, Lc = captions.shape
    K, d = dee.shape[1], dee.shape[2]
    F = 0 if dfe is None else dfe.shape[1]
    L.check(L.load().ick_caption_embed_bwd(_p(dx), _p(captions), _p(masks), _p(dword), _p(dee), _p(dfe), B, Lc, K, F,
                                           V, d, pad_token, scale, *_dargs(drop), _stream()), "ick_caption_embed_bwd")


def pointer_scores_bwd(dscores, col0, h, ctx, w, ind, dh, dctx, dw, dbias, pack=None, fused=False):
    """pack (HeadRows): dscores holds the packed rows of the valid positions (ick_pointer_scores_bwd_packed).  fused: both
    roles in one launch (ick_pointer_scores_bwd_fused[_packed]), the same bits."""
    B, T, d = h.shape
    Kc = ctx.shape[1]
    name = "ick_pointer_scores_bwd_fused" if fused else "ick_pointer_scores_bwd"
    tail = ()
    if pack is not None:
        name, tail = name + "_packed", (_p(pack.rowmap), _p(pack.rowstart))
    L.check(getattr(L.load(), name)(_p(dscores), dscores.stride(-2), col0, _p(h), _p(ctx), _p(w), _p(ind), _p(dh),
                                    _p(dctx), _p(dw), _p(dbias), B, T, Kc, d, *tail, _stream()), name)


def entity_encode_bwd(variant, dee, entities, ee, dtype_emb, word_emb=None, dword=None):
    B, K, cols = entities.shape
    d = dee.shape[2]
    L.check(L.load().ick_entity_encode_bwd(L.VARIANT_ID[variant], _p(dee), _p(entities), cols, _p(ee), _p(word_emb),
                                           0 if word_emb is None else word_emb.shape[0], _p(dtype_emb),
                                           dtype_emb.shape[0], _p(dword), B, K, d, _stream()),
            "ick_entity_encode_bwd")


def fact_encode_bwd(dfe, facts, dee, dpred):
    B, F, d = dfe.shape
    K = dee.shape[1]
    L.check(L.load().ick_fact_encode_bwd(_p(dfe), _p(facts), _p(dee), _p(dpred), dpred.shape[0], B, K, F, d,
                                         _stream()), "ick_fact_encode_bwd")


def context_gate_bwd(captions, facts, dgate, dw, dbias, K, V, mode=0):
    B, Lc = captions.shape
    F = facts.shape[1]
    T, d = dgate.shape[1], dgate.shape[2]
    L.check(L.load().ick_context_gate_bwd(_p(captions), _p(facts), _p(dgate), _p(dw), _p(dbias), B, Lc, T, K, F, V,
                                          dw.shape[1], d, mode, _stream()), "ick_context_gate_bwd")


def _opt_words(words, who):
    if not isinstance(words, torch.Tensor) or words.dtype != torch.float32 or not words.is_cuda or \
            words.numel() < L.OPT_WORDS or not words.is_contiguous() or words.data_ptr() % 16:
        raise L.IckError("%s needs the optimizer words as a contiguous, 16-byte aligned float32 device tensor of %d "
                         "elements (base lr, max_norm, norm, coef, lr used, sum of squares)" % (who, L.OPT_WORDS))
    return words


def lr_schedule_struct(schedule):
    """dict(kind=, warmup_steps=, total_steps=, min_lr_ratio=) or None (constant, no warmup) -> lib.LrSchedule."""
    if isinstance(schedule, L.LrSchedule):
        return schedule
    sch = schedule or {}
    kind = sch.get("kind", "constant")
    if kind not in L.LR_KINDS:
        raise L.IckError("unknown lr schedule kind %r (one of %s)" % (kind, ", ".join(sorted(L.LR_KINDS))))
    return L.LrSchedule(L.LR_KINDS[kind], int(sch.get("warmup_steps", 0)), int(sch.get("total_steps", 0)),
                        float(sch.get("min_lr_ratio", 0.0)))


def grad_sqnorm_plan(n):
    """(workgroups of the partial pass, floats per workgroup and trip, floats of scratch) of ick_grad_sqnorm for n."""
    plan = (L.i32 * 3)()
    L.check(L.load().ick_grad_sqnorm_plan(n, plan), "ick_grad_sqnorm_plan")
    return tuple(plan)


def grad_sqnorm(g, words, scratch=None, gscale=1.0, gscale_den=None):
    """The norm pass of the global-norm clip (ick_grad_sqnorm): words[5] = sum of squares of the flat fp32 bucket g,
    words[2] = its L2 norm times |gscale (/ the device scalar gscale_den)|, words[3] = min(1, words[1] / (norm + 1e-6))
    (1 while words[1] <= 0).  Fixed-order reduction; nothing is written while gscale_den is given and not > 0.  words: the
    optimizer words ON THE DEVICE (a host max_norm would be baked into a captured launch); scratch: float32 device
    tensor of grad_sqnorm_plan(n)[2] floats (allocated when None).  Returns words."""
    _opt_words(words, "grad_sqnorm")
    if g.dtype != torch.float32 or not g.is_cuda or not g.is_contiguous():
        raise L.IckError("grad_sqnorm needs a contiguous float32 device bucket")
    if scratch is None:
        scratch = torch.empty(grad_sqnorm_plan(g.numel())[2], device=g.device, dtype=torch.float32)
    L.check(L.load().ick_grad_sqnorm(_p(g), g.numel(), gscale, _p(gscale_den), _p(scratch), scratch.numel(), _p(words),
                                     _stream()), "ick_grad_sqnorm")
    return words


def conv1_wgrad_plan(B, Cc, P, d):
    """((groups, reduction indices per group, column tiles, rows per row block), floats of scratch) of ick_conv1_wgrad
    for d_img (B, P, d) and feats (B, Cc, P)."""
    plan, floats = (L.i32 * 4)(), L.i64()
    L.check(L.load().ick_conv1_wgrad_plan(B, Cc, P, d, plan, C.byref(floats)), "ick_conv1_wgrad_plan")
    return tuple(plan), floats.value


def conv1_wgrad(d_img, feats, dw, db, scratch=None):
    """Encoder.conv1's weight and bias gradient straight from the NCHW feature map (ick_conv1_wgrad):
    dw[o, c] = sum_{b, p} d_img[b, p, o] * feats[b, c, p], db[o] = sum_{b, p} d_img[b, p, o].  d_img (B, P, d), feats
    (B, C, P) or (B, C, H, W) with H * W = P, dw (d, C) or conv1's (d, C, 1, 1), db (d,): contiguous float32 device
    tensors.  dw and db are OVERWRITTEN.  Fixed-order reduction, the same bits on every run.  scratch: float32 device
    tensor of conv1_wgrad_plan(B, C, P, d)[1] floats (allocated when None).  Returns (dw, db)."""
    for name, t in (("d_img", d_img), ("feats", feats), ("dw", dw), ("db", db)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
            raise L.IckError("conv1_wgrad needs %s as a contiguous float32 device tensor" % name)
    if d_img.dim() != 3 or feats.dim() not in (3, 4):
        raise L.IckError("conv1_wgrad takes d_img (B, P, d) and feats (B, C, P) or (B, C, H, W)")
    B, P, d = d_img.shape
    Cc = feats.shape[1]
    if feats.shape[0] != B or feats.numel() != B * Cc * P or dw.numel() != d * Cc or db.numel() != d:
        raise L.IckError("conv1_wgrad: d_img %s, feats %s, dw %s, db %s do not fit together"
                         % (tuple(d_img.shape), tuple(feats.shape), tuple(dw.shape), tuple(db.shape)))
    need = conv1_wgrad_plan(B, Cc, P, d)[1]
    if scratch is None:
        scratch = torch.empty(need, device=d_img.device, dtype=torch.float32)
    elif scratch.dtype != torch.float32 or not scratch.is_cuda or not scratch.is_contiguous() or scratch.numel() < need:
        raise L.IckError("conv1_wgrad needs %d contiguous float32 device floats of scratch" % need)
    L.check(L.load().ick_conv1_wgrad(_p(d_img), _p(feats), _p(dw), _p(db), B, Cc, P, d, _p(scratch), scratch.numel(),
                                     _stream()), "ick_conv1_wgrad")
    return dw, db


DECAY_DECOUPLED, DECAY_COUPLED = 0, 1                                   # ICK_DECAY_*


def adam_update(p, g, m, v, step, lr=None, *, words=None, schedule=None, cover=None, clip=5.0, gscale=1.0, beta1=0.9,
                beta2=0.999, eps=1e-8, step_tensor=None, gscale_den=None, ema=None, ema_decay_word=None, ema_warmup=False,
                decay_word=None, decay_mask=None, decoupled=True, bump=None):
    """g = clamp(g * gscale (/ the device scalar gscale_den, if given), +-clip), then Adam's update of p, m, v; step (+ the
    uint32 device counter step_tensor, if given) is Adam's 1-based step count.  Nothing is written while gscale_den is
    given and not > 0.
    The rate is exactly one of
      lr     a host float (the entry's words == NULL);
      words  the optimizer words ON THE DEVICE -- a host scalar is refused (the kOpt instantiation): the base rate in
             words[0] shaped by `schedule` (lr_schedule_struct) on the step count, the gradient multiplied by words[3] (the
             global-norm clip's coefficient) between the scale and the clamp; words[4] receives the rate used.
    cover: None for the p.numel() floats of a flat bucket; otherwise the owner of a cover of the WHOLE bucket
    (weights.DerivedWeights: items_dev / blocks_dev, device arrays of ick_adam_item / ick_adam_block, n_blocks, and nbytes,
    the launch's algorithmic bytes for profiling.py), read at call time: the same pass then also writes the re-laid-out
    copies of the updated weights (ick_adam_step_derive instead of ick_adam_step).
    ema: None, or the exponential moving average of p, a float32 device tensor laid out like p, updated in the same pass
    (kEma, e != NULL): e += (1 - d) * (p_new - e) with the decay d read from ema_decay_word, a one-float tensor ON THE
    DEVICE (a host scalar is refused: it would be baked into a captured launch); ema_warmup: d = min(d, (1 + t) / (10 + t))
    on the step count t.  p, g, m, v get the bits they get without ema.
    decay_word + decay_mask (both or neither): weight decay in the same pass (kDecay, decay != NULL).  decay_word: wd, a
    one-float tensor ON THE DEVICE (a host scalar is refused for the reason the EMA word is); decay_mask: a uint8 device
    tensor of at least ceil(p.numel() / 64) granules (bucket.ParamBucket.decay_mask), one per 64 floats from p's start,
    non-zero where the elements decay.  decoupled: True, torch.optim.AdamW's p *= 1 - lr_t * wd ahead of the update;
    False, torch.optim.Adam(weight_decay=)'s wd * p added to the clamped gradient the moments see (g is written back
    without it).
    bump = (inc, ticket): the launch also advances step_tensor by inc once all of it has read the counter, iff the update
    ran (counter_add_if's rule on gscale_den) -- ticket != NULL, the same bits; ticket: a one-element int32 device
    tensor holding 0 (ops.adam_ticket), the launch's own between calls."""
    if (lr is None) == (words is None):
        raise L.IckError("adam_update needs exactly one of lr (a host float) and words (the optimizer words)")
    if words is None and schedule is not None:
        raise L.IckError("adam_update: a schedule shapes the rate in the optimizer words; give words, not lr")
    if ema is None and (ema_decay_word is not None or ema_warmup):
        raise L.IckError("adam_update: ema_decay_word / ema_warmup shape a moving average; give ema= as well")
    if (decay_word is None) != (decay_mask is None):
        raise L.IckError("adam_update: weight decay needs both decay_word (wd) and decay_mask (which granules decay)")
    checks = []                                                          # (name, tensor, dtype, least elements)
    if decay_word is not None:
        checks += [("decay_word", decay_word, torch.float32, 1),
                   ("decay_mask", decay_mask, torch.uint8, (p.numel() + 63) // 64)]
    if ema is not None:
        checks += [("ema", ema, torch.float32, p.numel()), ("ema_decay_word", ema_decay_word, torch.float32, 1)]
    if bump is not None and (step_tensor is None or bump[1].numel() != 1 or bump[1].dtype != torch.int32 or
                             not bump[1].is_cuda):
        raise L.IckError("adam_update: bump needs step_tensor and a one-element int32 device ticket")
    for what, t, dtype, least in checks:
        if not isinstance(t, torch.Tensor) or t.dtype != dtype or not t.is_cuda or not t.is_contiguous() or \
                t.numel() < least:
            raise L.IckError("adam_update needs %s as a contiguous %s device tensor of at least %d element(s)"
                             % (what, str(dtype).replace("torch.", ""), least))
    if ema is not None and ema.data_ptr() % (4 if cover is None else 16):
        raise L.IckError("adam_update: ema must lie on %d bytes" % (4 if cover is None else 16))
    if cover is None:
        name, over = "ick_adam_step", (p.numel(),)
    else:
        L.ADAM_DERIVE_BYTES, L.ADAM_DERIVE_FLOATS = cover.nbytes, p.numel()     # (profiling.py's byte model)
        name, over = "ick_adam_step_derive", (_p(cover.items_dev), _p(cover.blocks_dev), cover.n_blocks)
    rate = (0.0, _p(_opt_words(words, "adam_update")), lr_schedule_struct(schedule)) if words is not None else \
        (lr, None, L.LrSchedule())
    # every option by its pointer: None is the update without it
    avg = (_p(ema_decay_word), int(bool(ema_warmup)))
    decay = (None, None, 0, 0) if decay_word is None else \
        (_p(decay_word), _p(decay_mask), decay_mask.numel(), DECAY_DECOUPLED if decoupled else DECAY_COUPLED)
    inc, ticket = (0, None) if bump is None else bump
    L.check(getattr(L.load(), name)(_p(p), _p(g), _p(m), _p(v), _p(ema), *over, gscale, clip, *rate, beta1, beta2, eps, step,
                                    _p(step_tensor), _p(gscale_den), *avg, *decay, int(inc), _p(ticket), _stream()), name)


def adam_ticket(device):
    """The ticket word of adam_update(bump=): zero now, and zero again after every launch."""
    return torch.zeros(1, device=device, dtype=torch.int32)


def counter_add(counter, inc=1):
    L.check(L.load().ick_counter_add(_p(counter), inc, _stream()), "ick_counter_add")


def counter_add_if(counter, inc, flag):
    """counter += inc iff flag[0] > 0 (device scalar), see ick_counter_add_if."""
    L.check(L.load().ick_counter_add_if(_p(counter), inc, _p(flag), _stream()), "ick_counter_add_if")


def scale_by_ratio(x, num, den):
    L.check(L.load().ick_scale_by_ratio(_p(x), x.numel(), _p(num), _p(den), _stream()), "ick_scale_by_ratio")
