// clip_gradient + torch.optim.Adam.step (geo-aware/utils.py:75-85, geo-aware/train.py:287-292) over the flat parameter
// bucket, and -- in the same pass over the same registers -- every re-laid-out copy of the weights that the next step's
// kernels read: the packed row-chain images (forward and transposed, csrc/rowchain.hip), the gathered all-layer cross
// K/V weight / bias, the bf16 hi / mid / lo planes of the large GEMMs' weights (csrc/gemm_ps.hip), the transposed
// predicate weight.  The optimizer is the only writer of the parameters, so nothing else has to re-lay them out: round 4
// spent 3 ick_pack_weights + 3 ick_presplit_weights launches per step on it (126 us of kernel time at cfg2, 30 MB per
// launch at 0.18 of the HBM rate; skipping them took 105 us off the 1.73 ms step, profiles/r05_x_ceilings_train.txt).
//
//   g = clamp(g * gscale [/ *gscale_den], -clip, clip);  m = b1 m + (1-b1) g;  v = b2 v + (1-b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// (default betas / eps, no amsgrad.)  The update is written once: adam_hyper() is the prologue, adam1() the arithmetic of
// one element.  kDecay (decay != NULL): weight decay on the elements whose 64-float granule of
// the bucket has its byte of the caller's mask set -- decoupled (torch.optim.AdamW), p = p * (1 - lr_t * wd) ahead of
// the unchanged update, or coupled (torch.optim.Adam(weight_decay=), L2), wd * p added to the clamped gradient that the
// moments and the update see, while the gradient written back stays without the term; wd is read from a device word.
// kDecay = false is the code without it.  kEma (e != NULL): the lane that holds the new p
// also keeps an exponential moving average of it in a fourth array, e += (1 - d_t) (p - e) (ema1()), two more 16-byte
// streams in the same pass; kEma = false is the code without it.  Three kernels address the bucket differently around
// them:
//   adam_clamp_kernel       one float per lane and trip: tails, short and unaligned buckets;
//   adam_clamp_vec4_kernel  one float4 per lane and trip, seven 16-byte streams: the aligned bulk of a flat bucket;
//   adam_derive_kernel      one workgroup = one block of the caller's cover of the bucket (include/ick_amd.h,
//                           ick_adam_step_derive):
//     flat run   <= 1024 float4, the seven 16-byte streams of adam_clamp_vec4_kernel (+ an optional plain copy);
//     tile       64 rows x 64 columns of a 2-D parameter (row segments of 256 contiguous bytes): updated in registers,
//                written back, the new values staged in LDS and read out once per image in that image's own order, so
//                that every image is written in runs of >= 1 KiB (pack, pack_t: [64 rows][4 k] granules; ps, ps_t:
//                64-byte rows of one plane and K slice).
// tests/test_adam_derive_gpu.py and tests/test_grad_norm_gpu.py hold the three to the same bits, and the images to
// ick_pack_weights / ick_presplit_weights of the updated weights.
#include "gemm_common.h"
#include "opt_words.h"

namespace ick {
namespace {

struct AdamHyper {
    float gscale, clip, b1, b2, c1, c2, eps, step, bc2_sqrt, coef, w, wd, f;
    bool coupled;
};

// The moving average's operands (kEma): the array, the device word that holds the decay, the warmup flag.  Passed to
// every instantiation so that the kernels keep one signature; the ones without kEma never read it (nor AdamHyper::w):
// their instruction stream and register counts are those from before the flag, their kernarg segment is 24 bytes longer.
struct AdamEma {
    float* e;
    const float* decay;
    int warmup;
};

// The weight decay's operands (kDecay): the device word that holds wd, one byte (0 / 1) per 64-float granule of the bucket,
// how many there are, the offset in floats of the kernel's arrays from the bucket's start (the mask is indexed from the
// bucket's start, not from the address: the scalar tail of a flat launch starts behind the float4 part) and the form.
// Passed to every instantiation like AdamEma; the ones without kDecay never read it.
struct AdamDecay {
    const float* wd;
    const uint8_t* mask;
    int64_t granules;
    int64_t base;
    int coupled;
};

// The step counter's advance inside the optimizer launch (ick_adam_step[_derive]): ticket == nullptr is
// the code without it.  Every workgroup has read the counter in adam_hyper() before it draws its ticket; the workgroup
// that draws the last one adds inc to the counter -- nobody of this launch reads it any more -- and sets the ticket word
// back to 0 for the next launch.  A launch that returns from adam_hyper() (no token) draws no ticket and adds nothing.
struct AdamBump {
    uint32_t* counter;
    uint32_t inc;
    uint32_t* ticket;
};
__device__ __forceinline__ void adam_bump(const AdamBump& b) {
    if (b.ticket == nullptr) return;      // uniform
    __syncthreads();                      // every wave of the workgroup is past its read of the counter
    if (threadIdx.x == 0 &&
        __hip_atomic_fetch_add(b.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == gridDim.x - 1u) {
        *b.counter += b.inc;
        __hip_atomic_store(b.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

constexpr int kGranuleShift = 6;      // log2 of the granule: bucket.ALIGN = 64 floats, where every parameter starts

// Is the decay on for the element at float offset `at` from the bucket's start?  (A granule beyond the table: off.)
__device__ __forceinline__ bool decay_on(const AdamDecay& dec, int64_t at) {
    const int64_t gr = at >> kGranuleShift;
    return gr < dec.granules && dec.mask[gr] != 0;
}

// The prologue of every Adam kernel.  false: no token contributed to the (global) batch, which then has no mean loss --
// the kernel leaves parameters, moments, images and the rate word alone instead of spreading 0 * inf = NaN over every
// weight.  kOpt (words != NULL): the step's rate comes from the base rate word and the schedule
// instead of the literal, h.coef is the global-norm clip's coefficient, and workgroup 0 leaves the rate it used in
// words[4].  kEma: h.w = 1 - d_t, the weight of the new parameter in the moving average, with d_t = *decay or, with the
// warmup flag, min(*decay, (1 + t) / (10 + t)) on the step t of the bias correction.
template <bool kOpt, bool kEma, bool kDecay>
__device__ __forceinline__ bool adam_hyper(AdamHyper& h, float gscale, float clip, float lr, float b1, float b2, float eps,
                                           int step0, const uint32_t* step_ptr, const float* __restrict__ gscale_den,
                                           float* words, const ick_lr_schedule& sched, const AdamEma& ema,
                                           const AdamDecay& dec) {
    if (gscale_den) {
        if (!(gscale_den[0] > 0.f)) return false;
        gscale = gscale / gscale_den[0];
    }
    const float t = (float)(step0 + (step_ptr ? (int)*step_ptr : 0));
    const float bc1 = 1.f - powf(b1, t);
    h.bc2_sqrt = sqrtf(1.f - powf(b2, t));
    h.coef = 1.f;
    if (kOpt) {
        lr = lr_schedule(words[kWordBaseLr], sched, t);
        h.coef = words[kWordCoef];
        if (blockIdx.x == 0 && threadIdx.x == 0) words[kWordLrNow] = lr;
    }
    h.step = lr / bc1;
    h.w = 0.f;
    if (kEma) {
        float d = ema.decay[0];
        if (ema.warmup) d = fminf(d, (1.f + t) / (10.f + t));
        h.w = 1.f - d;
    }
    h.wd = 0.f; h.f = 1.f; h.coupled = false;
    if (kDecay) {
        h.wd = dec.wd[0];
        const float shrink = lr * h.wd;       // lr: the rate this update uses (the scheduled one with kOpt)
        h.f = 1.f - shrink;
        h.coupled = dec.coupled != 0;
    }
    h.gscale = gscale; h.clip = clip; h.b1 = b1; h.b2 = b2; h.c1 = 1.f - b1; h.c2 = 1.f - b2; h.eps = eps;
    return true;
}

// The update of one element, the only place its arithmetic is written (-ffp-contract=off keeps the operations apart).
// kOpt: the gradient times the clip coefficient between the scale and the clamp, as an operation of its own -- with
// coef == 1 and a constant schedule the bits are the plain instantiation's.  kDecay and `on` (the element's granule is
// selected): decoupled, the parameter shrinks first and the update is the unchanged one; coupled, the product wd * p and
// its sum with the clamped gradient feed the moments, behind the gradient's write-back.
template <bool kOpt, bool kDecay = false>
__device__ __forceinline__ void adam1(const AdamHyper& h, float& p, float& g, float& m, float& v, bool on = false) {
    float x = g * h.gscale;
    if (kOpt) x = x * h.coef;
    if (h.clip > 0.f) x = fminf(fmaxf(x, -h.clip), h.clip);
    g = x;
    if (kDecay && on) {
        if (h.coupled) {
            const float term = h.wd * p;
            x = x + term;
        } else {
            p = p * h.f;
        }
    }
    m = h.b1 * m + h.c1 * x;
    v = h.b2 * v + h.c2 * x * x;
    p -= h.step * m / (sqrtf(v) / h.bc2_sqrt + h.eps);
}

// The moving average of one element, written once like adam1: the difference, the product and the sum stay apart.
__device__ __forceinline__ void ema1(const AdamHyper& h, float& e, float p) {
    const float d = p - e;
    e = e + h.w * d;
}

__device__ __forceinline__ void ema4(const AdamHyper& h, float4& e, const float4& p) {
    ema1(h, e.x, p.x);
    ema1(h, e.y, p.y);
    ema1(h, e.z, p.z);
    ema1(h, e.w, p.w);
}

// (a float4 at a multiple of 4 floats from the bucket's start lies inside one granule: one `on` for the four)
template <bool kOpt, bool kDecay = false>
__device__ __forceinline__ void adam4(const AdamHyper& h, float4& p, float4& g, float4& m, float4& v, bool on = false) {
    adam1<kOpt, kDecay>(h, p.x, g.x, m.x, v.x, on);
    adam1<kOpt, kDecay>(h, p.y, g.y, m.y, v.y, on);
    adam1<kOpt, kDecay>(h, p.z, g.z, m.z, v.z, on);
    adam1<kOpt, kDecay>(h, p.w, g.w, m.w, v.w, on);
}

template <bool kOpt, bool kEma, bool kDecay>
__global__ __launch_bounds__(256) void adam_clamp_kernel(float* __restrict__ p, float* __restrict__ g,
                                                         float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                         float gscale, float clip, float lr, float b1, float b2,
                                                         float eps, int step0, const uint32_t* step_ptr,
                                                         const float* __restrict__ gscale_den, float* words,
                                                         ick_lr_schedule sched, AdamEma ema, AdamDecay dec, AdamBump bump) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    AdamHyper h;
    if (!adam_hyper<kOpt, kEma, kDecay>(h, gscale, clip, lr, b1, b2, eps, step0, step_ptr, gscale_den, words, sched, ema,
                                         dec))
        return;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float gi = g[i], mi = m[i], vi = v[i], pi = p[i], ei = 0.f;
        if (kEma) ei = ema.e[i];
        adam1<kOpt, kDecay>(h, pi, gi, mi, vi, kDecay && decay_on(dec, dec.base + i));
        g[i] = gi; m[i] = mi; v[i] = vi; p[i] = pi;
        if (kEma) { ema1(h, ei, pi); ema.e[i] = ei; }
    }
    adam_bump(bump);
}

// The same update on float4: seven 16-byte streams per lane (the scalar form reaches 0.66 of the HBM rate, 320 MB per
// cfg2 step).  n4 = n / 4 elements of float4; the launcher sends a tail of n % 4 to the scalar kernel.
template <bool kOpt, bool kEma, bool kDecay>
__global__ __launch_bounds__(256) void adam_clamp_vec4_kernel(float4* __restrict__ p, float4* __restrict__ g,
                                                              float4* __restrict__ m, float4* __restrict__ v, int64_t n4,
                                                              float gscale, float clip, float lr, float b1, float b2,
                                                              float eps, int step0, const uint32_t* step_ptr,
                                                              const float* __restrict__ gscale_den, float* words,
                                                              ick_lr_schedule sched, AdamEma ema, AdamDecay dec, AdamBump bump) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    AdamHyper h;
    if (!adam_hyper<kOpt, kEma, kDecay>(h, gscale, clip, lr, b1, b2, eps, step0, step_ptr, gscale_den, words, sched, ema,
                                         dec))
        return;
    float4* __restrict__ e = reinterpret_cast<float4*>(ema.e);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 gi = g[i], mi = m[i], vi = v[i], pi = p[i], ei;
        if (kEma) ei = e[i];
        adam4<kOpt, kDecay>(h, pi, gi, mi, vi, kDecay && decay_on(dec, dec.base + 4 * i));
        g[i] = gi; m[i] = mi; v[i] = vi; p[i] = pi;
        if (kEma) { ema4(h, ei, pi); e[i] = ei; }
    }
    adam_bump(bump);
}

constexpr int kT = 64;        // tile edge
constexpr int kLd = 68;       // LDS row stride of the tile (16-byte aligned rows, 4 banks of skew per row)

template <bool kOpt, bool kEma, bool kDecay>
__global__ __launch_bounds__(256) void adam_derive_kernel(float* __restrict__ p, float* __restrict__ g,
                                                          float* __restrict__ m, float* __restrict__ v,
                                                          const ick_adam_item* __restrict__ items,
                                                          const ick_adam_block* __restrict__ blocks, float gscale,
                                                          float clip, float lr, float b1, float b2, float eps, int step0,
                                                          const uint32_t* step_ptr, const float* __restrict__ gscale_den,
                                                          float* words, ick_lr_schedule sched, AdamEma ema, AdamDecay dec,
                                                          AdamBump bump) {
    __shared__ __attribute__((aligned(16))) float tile[kT * kLd];
    const ick_adam_block blk = blocks[blockIdx.x];
    AdamHyper h;
    if (!adam_hyper<kOpt, kEma, kDecay>(h, gscale, clip, lr, b1, b2, eps, step0, step_ptr, gscale_den, words, sched, ema,
                                         dec))
        return;
    const int tid = threadIdx.x;

    if (blk.item < 0) {
        // ---- flat run: up to four float4 per thread, every load issued before the first use
        float4* p4 = reinterpret_cast<float4*>(p) + blk.off4;
        float4* g4 = reinterpret_cast<float4*>(g) + blk.off4;
        float4* m4 = reinterpret_cast<float4*>(m) + blk.off4;
        float4* v4 = reinterpret_cast<float4*>(v) + blk.off4;
        float4* e4 = reinterpret_cast<float4*>(ema.e) + blk.off4;
        float4 pi[4], gi[4], mi[4], vi[4], ei[4];
        bool on[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = tid + 256 * i;
            on[i] = false;
            if (j < blk.cnt4) {
                gi[i] = g4[j]; mi[i] = m4[j]; vi[i] = v4[j]; pi[i] = p4[j];
                if (kEma) ei[i] = e4[j];
                if (kDecay) on[i] = decay_on(dec, 4 * ((int64_t)blk.off4 + j));
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int j = tid + 256 * i;
            if (j < blk.cnt4) {
                adam4<kOpt, kDecay>(h, pi[i], gi[i], mi[i], vi[i], on[i]);
                g4[j] = gi[i]; m4[j] = mi[i]; v4[j] = vi[i]; p4[j] = pi[i];
                if (kEma) { ema4(h, ei[i], pi[i]); e4[j] = ei[i]; }
                if (blk.copy) reinterpret_cast<float4*>(blk.copy)[j] = pi[i];
            }
        }
        adam_bump(bump);
        return;
    }

    // ---- tile (tn, tk) of an item
    const ick_adam_item it = items[blk.item];
    const int n0 = blk.tn * kT, k0 = blk.tk * kT;
    const int K = it.K;
    {
        float4 pi[4], gi[4], mi[4], vi[4], ei[4];
        int64_t at[4];
        bool on[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 4, c4 = idx & 15;
            const int r = n0 + row - it.drow0, k = k0 + 4 * c4;
            at[i] = (r >= 0 && r < it.rows && k < K) ? it.off + (int64_t)r * K + k : -1;
            if (at[i] >= 0) {
                gi[i] = *reinterpret_cast<const float4*>(g + at[i]);
                mi[i] = *reinterpret_cast<const float4*>(m + at[i]);
                vi[i] = *reinterpret_cast<const float4*>(v + at[i]);
                pi[i] = *reinterpret_cast<const float4*>(p + at[i]);
                if (kEma) ei[i] = *reinterpret_cast<const float4*>(ema.e + at[i]);
            }
            on[i] = kDecay && at[i] >= 0 && decay_on(dec, at[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int row = idx >> 4, c4 = idx & 15;
            float4 out = make_float4(0.f, 0.f, 0.f, 0.f);      // outside the item / the matrix: zeros (the images' padding)
            if (at[i] >= 0) {
                adam4<kOpt, kDecay>(h, pi[i], gi[i], mi[i], vi[i], on[i]);
                *reinterpret_cast<float4*>(g + at[i]) = gi[i];
                *reinterpret_cast<float4*>(m + at[i]) = mi[i];
                *reinterpret_cast<float4*>(v + at[i]) = vi[i];
                *reinterpret_cast<float4*>(p + at[i]) = pi[i];
                if (kEma) { ema4(h, ei[i], pi[i]); *reinterpret_cast<float4*>(ema.e + at[i]) = ei[i]; }
                out = pi[i];
                if (it.copy) *reinterpret_cast<float4*>(it.copy + (int64_t)(n0 + row) * it.copy_ld + k0 + 4 * c4) = pi[i];
            }
            *reinterpret_cast<float4*>(tile + row * kLd + 4 * c4) = out;
        }
    }
    __syncthreads();
    const int rlo = it.drow0 - n0, rhi = it.drow0 + it.rows - n0;      // tile rows [rlo, rhi) belong to the item

    if (it.pack) {
        // dst[slab = n / 64][k4][l = n % 64][4]: lanes <-> 64 rows, 1 KiB per k4
        const int K16 = (K + 15) & ~15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 256 * i;
            const int j = u >> 6, l = u & 63;
            const int k4 = blk.tk * 16 + j;
            if (l >= rlo && l < rhi && 4 * k4 < K)
                *reinterpret_cast<float4*>(it.pack + (((int64_t)blk.tn * (K16 / 4) + k4) * 64 + l) * 4) =
                    *reinterpret_cast<const float4*>(tile + l * kLd + 4 * j);
        }
    }
    if (it.pack_t) {
        // the image of W^T (K rows, Nd columns): dst[slab = k / 64][n / 4][l = k % 64][n % 4]; lanes <-> 64 k
        const int N16 = (it.Nd + 15) & ~15;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int u = tid + 256 * i;
            const int j = u >> 6, l = u & 63;          // rows 4j .. 4j+3 of the tile, column l
            if (4 * j >= rlo && 4 * j < rhi && k0 + l < K) {
                const float4 x = make_float4(tile[(4 * j) * kLd + l], tile[(4 * j + 1) * kLd + l],
                                             tile[(4 * j + 2) * kLd + l], tile[(4 * j + 3) * kLd + l]);
                *reinterpret_cast<float4*>(it.pack_t + (((int64_t)blk.tk * (N16 / 4) + (n0 >> 2) + j) * 64 + l) * 4) = x;
            }
        }
    }
    if (it.ps) {
        // plane[slice = k / 32][row n < Np][32 k] bf16: a thread splits 8 consecutive k of one row (16 bytes per plane)
        const int64_t np = (int64_t)((it.Nd + 63) / 64) * 64;
        const int K32 = (K + 31) & ~31;
        char* base = reinterpret_cast<char*>(it.ps);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i;
            const int row = u & 63, c = u >> 6;
            const int k = k0 + 8 * c;
            if (row >= rlo && row < rhi && k < K32) {
                const float4 a = *reinterpret_cast<const float4*>(tile + row * kLd + 8 * c);
                const float4 b = *reinterpret_cast<const float4*>(tile + row * kLd + 8 * c + 4);
                uint32_t hh[4], mm[4], ll[4];
                split3(a.x, a.y, hh[0], mm[0], ll[0]); split3(a.z, a.w, hh[1], mm[1], ll[1]);
                split3(b.x, b.y, hh[2], mm[2], ll[2]); split3(b.z, b.w, hh[3], mm[3], ll[3]);
                char* dst = base + (((int64_t)(k >> 5) * 3) * np + n0 + row) * 64 + (k & 31) * 2;
                *reinterpret_cast<uint4*>(dst) = uint4{hh[0], hh[1], hh[2], hh[3]};
                *reinterpret_cast<uint4*>(dst + np * 64) = uint4{mm[0], mm[1], mm[2], mm[3]};
                *reinterpret_cast<uint4*>(dst + 2 * np * 64) = uint4{ll[0], ll[1], ll[2], ll[3]};
            }
        }
    }
    if (it.ps_t) {
        // the image of W^T: plane[slice = n / 32][row k < Kp][32 n] bf16: a thread splits 8 consecutive n of one k
        const int64_t kp = (int64_t)((K + 63) / 64) * 64;
        char* base = reinterpret_cast<char*>(it.ps_t);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int u = tid + 256 * i;
            const int kk = u & 63, c = u >> 6;
            if (8 * c >= rlo && 8 * c < rhi && k0 + kk < K) {
                float x[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = tile[(8 * c + e) * kLd + kk];
                uint32_t hh[4], mm[4], ll[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) split3(x[2 * e], x[2 * e + 1], hh[e], mm[e], ll[e]);
                const int n = n0 + 8 * c;
                char* dst = base + (((int64_t)(n >> 5) * 3) * kp + k0 + kk) * 64 + (n & 31) * 2;
                *reinterpret_cast<uint4*>(dst) = uint4{hh[0], hh[1], hh[2], hh[3]};
                *reinterpret_cast<uint4*>(dst + kp * 64) = uint4{mm[0], mm[1], mm[2], mm[3]};
                *reinterpret_cast<uint4*>(dst + 2 * kp * 64) = uint4{ll[0], ll[1], ll[2], ll[3]};
            }
        }
    }
    if (it.tr) {
        // plain W^T: lanes <-> 64 consecutive n of one k (256 contiguous bytes)
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int u = tid + 256 * i;
            const int nl = u & 63, kl = u >> 6;
            if (nl >= rlo && nl < rhi && k0 + kl < K) it.tr[(int64_t)(k0 + kl) * it.tr_ld + n0 + nl] = tile[nl * kLd + kl];
        }
    }
    adam_bump(bump);
}

}  // namespace
}  // namespace ick

using namespace ick;

// What both entries ask of their arguments (count: the floats of a flat bucket, the blocks of a cover); al16: whether all
// the arrays lie on 16 bytes, which the float4 kernels need.  kEma: the moving average is one more array, and its decay
// word must be there.  kDecay: the decay word, the granule mask with at least one granule, a known form.
template <bool kEma, bool kDecay>
static int adam_args(const float* p, const float* g, const float* m, const float* v, int64_t count, int32_t step,
                     const uint32_t* step_ptr, const AdamEma& ema, const AdamDecay& dec, bool& al16) {
    ICK_CHECK_ARG(p && g && m && v && count > 0 && (step >= 1 || step_ptr != nullptr));
    if (kEma) ICK_CHECK_ARG(ema.e != nullptr && ema.decay != nullptr);
    if (kDecay)
        ICK_CHECK_ARG(dec.wd != nullptr && dec.mask != nullptr && dec.granules > 0 &&
                      (dec.coupled == ICK_DECAY_DECOUPLED || dec.coupled == ICK_DECAY_COUPLED));
    al16 = ((reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(m) |
             reinterpret_cast<uintptr_t>(v) | (kEma ? reinterpret_cast<uintptr_t>(ema.e) : 0)) & 15) == 0;
    return ICK_OK;
}

// ick_adam_step: the float4 kernel over the aligned bulk, the scalar kernel over the rest (which tells the mask where it
// starts: dec.base)
template <bool kOpt, bool kEma, bool kDecay>
static int launch_adam(float* p, float* g, float* m, float* v, int64_t n, float gscale, float clip, float lr, float* words,
                       ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step, const uint32_t* step_ptr,
                       const float* gscale_den, AdamEma ema, void* stream, AdamDecay dec, AdamBump bump) {
    bool al16;
    if (int rc = adam_args<kEma, kDecay>(p, g, m, v, n, step, step_ptr, ema, dec, al16)) return rc;
    if (kDecay) ICK_CHECK_ARG(dec.granules >= ceil_div(n, (int64_t)1 << kGranuleShift));
    if (kEma && (reinterpret_cast<uintptr_t>(ema.e) & 3)) return ICK_EALIGN;
    int64_t done = 0;
    if (n >= 4096 && al16) {
        const int64_t n4 = n / 4;
        const AdamBump here = n % 4 == 0 ? bump : AdamBump{};       // the counter moves in the bucket's LAST launch
        hipLaunchKernelGGL((adam_clamp_vec4_kernel<kOpt, kEma, kDecay>), dim3((int)std::min<int64_t>(ceil_div(n4, 256), 4096)),
                           dim3(256), 0, (hipStream_t)stream, reinterpret_cast<float4*>(p), reinterpret_cast<float4*>(g),
                           reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), n4, gscale, clip, lr, beta1, beta2,
                           eps, step, step_ptr, gscale_den, words, sched, ema, dec, here);
        done = 4 * n4;
        if (done == n) ICK_LAUNCH_RET();
    }
    if (kEma) ema.e += done;
    dec.base = done;
    hipLaunchKernelGGL((adam_clamp_kernel<kOpt, kEma, kDecay>), dim3((int)std::min<int64_t>(ceil_div(n - done, 256), 4096)),
                       dim3(256), 0, (hipStream_t)stream, p + done, g + done, m + done, v + done, n - done, gscale, clip, lr,
                       beta1, beta2, eps, step, step_ptr, gscale_den, words, sched, ema, dec, bump);
    ICK_LAUNCH_RET();
}

// ick_adam_step_derive (the cover lies on the device, so the granule count cannot be held against it here: the kernel
// treats a granule beyond the table as not selected)
template <bool kOpt, bool kEma, bool kDecay>
static int launch_adam_derive(float* p, float* g, float* m, float* v, const ick_adam_item* items,
                              const ick_adam_block* blocks, int32_t n_blocks, float gscale, float clip, float lr,
                              float* words, ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step,
                              const uint32_t* step_ptr, const float* gscale_den, AdamEma ema, void* stream, AdamDecay dec,
                              AdamBump bump) {
    bool al16;
    if (int rc = adam_args<kEma, kDecay>(p, g, m, v, blocks ? n_blocks : 0, step, step_ptr, ema, dec, al16)) return rc;
    if (!al16) return ICK_EALIGN;
    hipLaunchKernelGGL((adam_derive_kernel<kOpt, kEma, kDecay>), dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v,
                       items, blocks, gscale, clip, lr, beta1, beta2, eps, step, step_ptr, gscale_den, words, sched, ema,
                       dec, bump);
    ICK_LAUNCH_RET();
}

// The optimizer's two entries (include/ick_amd.h): every option by its pointer -- words == NULL takes the host rate lr
// (kOpt off), e == NULL keeps no average (kEma off), decay == NULL decays nothing (kDecay off) -- picks one of the eight
// <kOpt, kEma, kDecay> instantiations; ticket != NULL makes the launch advance the step counter as well (AdamBump).  An
// option's other arguments without the pointer that selects it are refused here, the rest of an option's arguments by
// adam_args and the launchers, all of it before any launch.
template <bool kDerive, typename... Over>
static int adam_step(float* p, float* g, float* m, float* v, float* e, float gscale, float clip, float lr, float* words,
                     ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step, uint32_t* step_ptr,
                     const float* gscale_den, const float* ema_decay, int32_t ema_warmup, const float* decay,
                     const uint8_t* decay_mask, int64_t n_granules, int32_t decay_form, uint32_t bump_inc,
                     uint32_t* ticket, void* stream, Over... over) {
    if (words) ICK_CHECK_ARG(lr_schedule_ok(sched));
    if (!e) ICK_CHECK_ARG(ema_decay == nullptr && ema_warmup == 0);
    ICK_CHECK_ARG((decay == nullptr) == (decay_mask == nullptr));
    if (ticket) ICK_CHECK_ARG(step_ptr != nullptr);
    if (!words) sched = ick_lr_schedule{};
    const AdamEma ema = e ? AdamEma{e, ema_decay, ema_warmup != 0} : AdamEma{};
    const AdamDecay dec = decay ? AdamDecay{decay, decay_mask, n_granules, 0, decay_form} : AdamDecay{};
    const AdamBump bump{step_ptr, bump_inc, ticket};
    auto go = [&](auto opt, auto avg, auto wd) {
        constexpr bool kOpt = decltype(opt)::value, kEma = decltype(avg)::value, kDecay = decltype(wd)::value;
        const float rate = kOpt ? 0.f : lr;
        if constexpr (kDerive)
            return launch_adam_derive<kOpt, kEma, kDecay>(p, g, m, v, over..., gscale, clip, rate, words, sched, beta1, beta2,
                                                          eps, step, step_ptr, gscale_den, ema, stream, dec, bump);
        else
            return launch_adam<kOpt, kEma, kDecay>(p, g, m, v, over..., gscale, clip, rate, words, sched, beta1, beta2, eps,
                                                   step, step_ptr, gscale_den, ema, stream, dec, bump);
    };
    using T = std::true_type;
    using F = std::false_type;
    switch ((words ? 1 : 0) | (e ? 2 : 0) | (decay ? 4 : 0)) {
        case 0: return go(F{}, F{}, F{});
        case 1: return go(T{}, F{}, F{});
        case 2: return go(F{}, T{}, F{});
        case 3: return go(T{}, T{}, F{});
        case 4: return go(F{}, F{}, T{});
        case 5: return go(T{}, F{}, T{});
        case 6: return go(F{}, T{}, T{});
        default: return go(T{}, T{}, T{});
    }
}

extern "C" int ick_adam_step(float* p, float* g, float* m, float* v, float* e, int64_t n, float gscale, float clip, float lr,
                             float* words, ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step,
                             uint32_t* step_ptr, const float* gscale_den, const float* ema_decay, int32_t ema_warmup,
                             const float* decay, const uint8_t* decay_mask, int64_t n_granules, int32_t decay_form,
                             uint32_t bump_inc, uint32_t* ticket, void* stream) {
    return adam_step<false>(p, g, m, v, e, gscale, clip, lr, words, sched, beta1, beta2, eps, step, step_ptr, gscale_den,
                            ema_decay, ema_warmup, decay, decay_mask, n_granules, decay_form, bump_inc, ticket, stream, n);
}

extern "C" int ick_adam_step_derive(float* p, float* g, float* m, float* v, float* e, const ick_adam_item* items,
                                    const ick_adam_block* blocks, int32_t n_blocks, float gscale, float clip, float lr,
                                    float* words, ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step,
                                    uint32_t* step_ptr, const float* gscale_den, const float* ema_decay,
                                    int32_t ema_warmup, const float* decay, const uint8_t* decay_mask, int64_t n_granules,
                                    int32_t decay_form, uint32_t bump_inc, uint32_t* ticket, void* stream) {
    return adam_step<true>(p, g, m, v, e, gscale, clip, lr, words, sched, beta1, beta2, eps, step, step_ptr, gscale_den,
                           ema_decay, ema_warmup, decay, decay_mask, n_granules, decay_form, bump_inc, ticket, stream,
                           items, blocks, n_blocks);
}
