// One KV-cached decode step of DecoderTransformer.predict() (geo-aware/models.py:389-443,
// knowledge-aware/models.py:545-608) for R independent rows (R = captions, or captions x beams) in
// 3 launches per decoder layer + 3 for the score head and the selection, instead of ~37 dependent launches:
//
//   dec_self_kernel   (row, head)   LN-on-load -> q|k|v rows of the head (GEMV) -> cache write -> causal
//                                   self-attention over the cached positions -> this head's slice of out_proj
//   dec_cross_kernel  (row, head)   LN-on-load -> q rows of the head -> attention over the S memory rows
//                                   [image ; entity ; fact] (K/V streamed once, coalesced 1 KiB per wave
//                                   instruction) -> this head's slice of out_proj
//   dec_ffn_kernel    (row, chunk)  LN-on-load -> 64 hidden units of linear1 + ReLU -> their slice of linear2
//   dec_head_kernel   (row)         final LayerNorm -> h (x predicate gate) -> pointer scores over entities / facts
//   dec_vocab_kernel  (16 words x 32 rows)  vocabulary logits on the fp32 MFMA, K split over the 4 waves,
//                                   per-tile top-2 candidates
// The kernels that choose tokens from a finished step's outputs (greedy, beam) are decode_select.hip, sampling is
// sample.hip; the greedy choice of step i - 1 can also run inside dec_self_kernel of step i (fused_select below).
//
// "LN-on-load": a block does not apply its closing residual + LayerNorm itself (that would need all heads /
// chunks of the row in one workgroup, i.e. too few workgroups to stream K/V at HBM rate).  It leaves its
// out-projection as per-head (per-chunk) partial rows; the NEXT kernel forms
//       x = LayerNorm(res + bias + sum_p partial_p) * gamma + beta
// while loading its input row (300 floats: a few hundred flops per workgroup), and the workgroup with
// head/chunk 0 stores x as the residual of the following block.  Sums run in a fixed order: results are
// deterministic (no float atomics anywhere on this path).
//
// Bounds: per token the path moves the cross K/V of every layer once (S x 32 floats x 2 per row, head, layer:
// 53 MB at B=32, S=216 -> HBM-bound) plus ~16 MB of weights that stay L2 / Infinity-Cache
// resident.  Every workgroup's weight loads are issued before the data they multiply is ready (they do not
// depend on it), so a kernel is ~3 memory round trips long.
#include "decode_select.h"

#include <cstdio>
#include <cstdlib>
#include <type_traits>

// Diagnostic build (-DICK_DECODE_STAMPS, tools/debug/decode_stamps.py): workgroup (0, 0) of every decode kernel
// records the shader clock at its phase boundaries.  Compiled out of the product library.
#ifdef ICK_DECODE_STAMPS
__device__ unsigned long long ick_stamps[8][16];
#define ICK_STAMP(kern, i)                                                                          \
    do {                                                                                            \
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) ick_stamps[kern][i] = __builtin_amdgcn_s_memtime(); \
    } while (0)
extern "C" int ick_debug_read_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ick_stamps), sizeof(ick_stamps));
}
#else
#define ICK_STAMP(kern, i)
#endif

namespace ick {
namespace {

constexpr int kDMax = 320;   // model width limit of this path: 5 float4 per lane of a 16-lane row group
constexpr int kD4Max = kDMax / 4;
constexpr int kSMax = 1024;  // memory rows (cross-attention keys)
constexpr int kMLMax = 128;  // caption positions (self-attention keys)
constexpr int kDhp = 32;     // padded head width of the head-major K/V layouts
constexpr int kPartsMax = 16;
constexpr int kNumCU = 256;

using f32x2 = __attribute__((ext_vector_type(2))) float;

struct RowSrc {
    const float* res;     // (R, d) residual rows; the input itself when nparts == 0
    const float* part;    // (R, nparts, d) partial out-projection rows of the previous block
    const float* bias;    // (d) bias of that out-projection
    const float* gamma;   // (d) LayerNorm affine
    const float* beta;
    float* out;           // (R, d) normalised rows (written by head/chunk 0), may be null
    int nparts;
    float eps;
};

// What bounds these kernels (in-kernel stamps + ISA counts, round 3): NOT the bytes -- a workgroup of four waves has one
// wave per SIMD, and a lone wave issues one instruction per ~4 cycles whatever its type; ~1500 instructions of address
// arithmetic, loads and reductions in front of the first barrier were 5-6 k cycles.  Hence: (1) 512-thread workgroups
// (two waves per SIMD share the issue slots, every wave holds half the weight registers: no accumulator-file spills,
// whose copies wait for the loads they copy); (2) the wave index is read with readfirstlane, so row and weight base
// addresses are scalar and the loads take the scalar-base + 32-bit-offset form; (3) no branch per source row: clamped
// loads weighted by 0 / 1; (4) the early-exit word is waited for after the loads have been issued.
constexpr int kNT = 512;           // threads of a block kernel
constexpr int kNW = kNT / 64;      // waves

// Workgroups are dealt round-robin over the 8 XCDs (linear id % 8), each with its own L2 that starts a kernel cold.
// The (weight slice, row group) units are therefore numbered so that the workgroups of one XCD are CONSECUTIVE units,
// slice-major: an XCD then pulls 2-3 heads' weights (or one FFN chunk) through its L2 instead of all of them -- the
// beyond-L2 traffic of a decode step drops from ~146 MB to ~82 MB.  Placement affects speed only, never results.
__device__ __forceinline__ void xcd_unit(int& slice, int& group, int ngroups) {
    const int nwg = gridDim.x * gridDim.y, lin = blockIdx.y * gridDim.x + blockIdx.x;
    const int xcd = lin & 7, slot = lin >> 3;
    const int u = xcd * (nwg >> 3) + min(xcd, nwg & 7) + slot;          // XCD x owns units [start_x, start_x + count_x)
    slice = u / ngroups;
    group = u - slice * ngroups;
}

__device__ __forceinline__ int wave_id() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
// uniform base + 32-bit byte offset: global_load_dwordx4 v, v_off, s[base:base+1]
__device__ __forceinline__ float4 ld4o(const float* base, uint32_t byteoff) {
    return *reinterpret_cast<const float4*>(reinterpret_cast<const char*>(base) + byteoff);
}
__device__ __forceinline__ float4 ld4o_stream(const float* base, uint32_t byteoff) {   // read once per step by one workgroup
#ifdef ICK_DECODE_NT_KV
    const f32x4 v = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(reinterpret_cast<const char*>(base) + byteoff));
    return make_float4(v[0], v[1], v[2], v[3]);
#else
    return ld4o(base, byteoff);
#endif
}
__device__ __forceinline__ float4 f4zero() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ void f4add(float4& a, const float4& b) { a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w; }

// lane exchanges inside a row of 16 lanes: DPP operands (decode_select.h)
__device__ __forceinline__ float sum8(float v) {      // over aligned groups of 8 lanes, result in every lane
    v += dpp_f32<kDppXor1>(v); v += dpp_f32<kDppXor2>(v); v += dpp_f32<kDppHalfMirror>(v);
    return v;
}
__device__ __forceinline__ float sum16(float v) { v = sum8(v); v += dpp_f32<kDppMirror>(v); return v; }

__device__ __forceinline__ float dot4(const float4& a, const float4& b) {
    return fmaf(a.x, b.x, fmaf(a.y, b.y, fmaf(a.z, b.z, a.w * b.w)));
}
// two-lane packed form (v_pk_fma_f32): the even and odd elements run as two independent chains
__device__ __forceinline__ f32x2 pkfma(const float4& a, const float4& b, f32x2 acc) {
    acc = __builtin_elementwise_fma(f32x2{a.x, a.y}, f32x2{b.x, b.y}, acc);
    return __builtin_elementwise_fma(f32x2{a.z, a.w}, f32x2{b.z, b.w}, acc);
}

// ---------------------------------------------------------------------------------------------------------
// "LN-on-load" of the G rows of a workgroup: x = LayerNorm(res + bias + sum_p partial_p) (or res itself when the source
// has no partial rows).  The NWAVES / G waves of a row each fetch and sum a slice of its source rows (residual, bias,
// partial 0, 1, ...: lane l holds float4 columns l and 64 + l), leave the slice sums in LDS, and after one barrier the
// row's first wave adds them in slice order and normalises: mean and variance are wave reductions (DPP + v_readlane).
// issue() only starts the loads -- the kernels issue them FIRST and their weight / K / V streams afterwards: vector-memory
// results return in issue order, so the rows are normalised while the streams are still arriving.  Every base address
// is wave-uniform (scalar); sums run in a fixed order: deterministic.
// ---------------------------------------------------------------------------------------------------------
template <int G, int NWAVES>
struct RowGather {
    static constexpr int WPR = NWAVES / G;                                  // waves per row (G = 3, 5: some waves idle)
    static constexpr int NS = (12 + WPR - 1) / WPR < 6 ? (12 + WPR - 1) / WPR : 6;   // source rows per wave and sweep
    static constexpr int PSUM = G * WPR * kD4Max;                           // float4 of the psum slices in LDS
    float4 a[NS], b[NS];
    float4 gm0, gm1, bt0, bt1;

    __device__ __forceinline__ static const float* src_row(const RowSrc& s, int64_t row, int d, int q) {
        return q == 0 ? s.res + row * d : (q == 1 ? s.bias : s.part + (row * s.nparts + (q - 2)) * d);
    }
    // source rows q0 .. q0 + NS - 1 of `row` (past the last: a copy of it, weighted 0 by the sum)
    __device__ __forceinline__ void sweep(const RowSrc& s, int64_t row, int d, int q0, int nrows) {
        const int lane = threadIdx.x & 63, d4 = d >> 2;
        const uint32_t o0 = 16u * (uint32_t)min(lane, d4 - 1), o1 = 16u * (uint32_t)min(64 + lane, d4 - 1);
#pragma unroll
        for (int j = 0; j < NS; ++j) {
            const float* src = src_row(s, row, d, min(q0 + j, nrows - 1));
            a[j] = ld4o(src, o0);
            if (d4 > 64) b[j] = ld4o(src, o1);
        }
    }
    __device__ __forceinline__ void issue(const RowSrc& s, int64_t r0, int R, int d) {
        const int lane = threadIdx.x & 63, wave = wave_id(), d4 = d >> 2;
        if (wave >= G * WPR) return;
        const int g = wave / WPR, wr = wave - g * WPR;
        const int64_t row = min(r0 + g, (int64_t)R - 1);
        const uint32_t o0 = 16u * (uint32_t)min(lane, d4 - 1), o1 = 16u * (uint32_t)min(64 + lane, d4 - 1);
        const int nrows = s.nparts > 0 ? s.nparts + 2 : 1;
        if (wr * NS < nrows) sweep(s, row, d, wr * NS, nrows);              // this slice holds source rows (uniform)
        gm0 = gm1 = bt0 = bt1 = f4zero();
        if (wr == 0 && s.nparts > 0) {
            gm0 = ld4o(s.gamma, o0); bt0 = ld4o(s.beta, o0);
            if (d4 > 64) { gm1 = ld4o(s.gamma, o1); bt1 = ld4o(s.beta, o1); }
        }
    }
    // psum: LDS float4 [G][WPR][kD4Max]; follow with a barrier
    __device__ __forceinline__ void slice_sums(const RowSrc& s, int64_t r0, int R, int d, float4* psum) {
        const int lane = threadIdx.x & 63, wave = wave_id(), d4 = d >> 2;
        if (wave >= G * WPR) return;
        const int g = wave / WPR, wr = wave - g * WPR;
        const bool wide = d4 > 64;
        const int nrows = s.nparts > 0 ? s.nparts + 2 : 1;
        f32x2 z0l = {0.f, 0.f}, z0h = {0.f, 0.f}, z1l = {0.f, 0.f}, z1h = {0.f, 0.f};
        auto add_sweep = [&](int q0) {
#pragma unroll
            for (int j = 0; j < NS; ++j) {
                const float f = q0 + j < nrows ? 1.f : 0.f;                 // scalar
                const f32x2 ff = {f, f};
                z0l = __builtin_elementwise_fma(f32x2{a[j].x, a[j].y}, ff, z0l);
                z0h = __builtin_elementwise_fma(f32x2{a[j].z, a[j].w}, ff, z0h);
                if (wide) {
                    z1l = __builtin_elementwise_fma(f32x2{b[j].x, b[j].y}, ff, z1l);
                    z1h = __builtin_elementwise_fma(f32x2{b[j].z, b[j].w}, ff, z1h);
                }
            }
        };
        // The sweep issue() requested is summed in straight-line code: its s_waitcnt then counts only the row loads, not
        // the weight / K / V streams requested after them (inside a loop the compiler waits for vmcnt(0), i.e. for the
        // whole stream).  Sources of more than 12 rows take the loop below.
        if (wr * NS < nrows) add_sweep(wr * NS);
        for (int q0 = (wr + WPR) * NS; q0 < nrows; q0 += WPR * NS) {
            sweep(s, min(r0 + g, (int64_t)R - 1), d, q0, nrows);
            add_sweep(q0);
        }
        float4* dst = psum + (g * WPR + wr) * kD4Max;
        dst[lane] = make_float4(z0l.x, z0l.y, z0h.x, z0h.y);
        if (lane < kD4Max - 64) dst[64 + lane] = make_float4(z1l.x, z1l.y, z1h.x, z1h.y);
    }
    // after the barrier: the first wave of every row normalises it into xs[g] (LDS, kDMax floats, zero beyond d) and,
    // when `writer`, into s.out; follow with a barrier
    __device__ __forceinline__ void finish(const RowSrc& s, int64_t r0, int R, int d, const float4* psum, float* xs,
                                           bool writer) {
        const int lane = threadIdx.x & 63, wave = wave_id(), d4 = d >> 2;
        if (wave >= G * WPR) return;
        const int g = wave / WPR, wr = wave - g * WPR;
        if (wr != 0) return;
        const int64_t row = min(r0 + g, (int64_t)R - 1);
        const bool ok0 = lane < d4, ok1 = 64 + lane < d4;
        const int l1 = min(64 + lane, kD4Max - 1);
        float4 z0 = psum[g * WPR * kD4Max + lane], z1 = psum[g * WPR * kD4Max + l1];
#pragma unroll
        for (int w = 1; w < WPR; ++w) {
            f4add(z0, psum[(g * WPR + w) * kD4Max + lane]);
            f4add(z1, psum[(g * WPR + w) * kD4Max + l1]);
        }
        if (!ok0) z0 = f4zero();
        if (!ok1) z1 = f4zero();
        if (s.nparts > 0) {
            const float mean = wave_sum(((z0.x + z0.y) + (z0.z + z0.w)) + ((z1.x + z1.y) + (z1.z + z1.w))) / (float)d;
            float v = 0.f;
            if (ok0) {
                v = fmaf(z0.x - mean, z0.x - mean, v); v = fmaf(z0.y - mean, z0.y - mean, v);
                v = fmaf(z0.z - mean, z0.z - mean, v); v = fmaf(z0.w - mean, z0.w - mean, v);
            }
            if (ok1) {
                v = fmaf(z1.x - mean, z1.x - mean, v); v = fmaf(z1.y - mean, z1.y - mean, v);
                v = fmaf(z1.z - mean, z1.z - mean, v); v = fmaf(z1.w - mean, z1.w - mean, v);
            }
            const float rstd = rsqrtf(wave_sum(v) / (float)d + s.eps);
            z0.x = (z0.x - mean) * rstd * gm0.x + bt0.x; z0.y = (z0.y - mean) * rstd * gm0.y + bt0.y;
            z0.z = (z0.z - mean) * rstd * gm0.z + bt0.z; z0.w = (z0.w - mean) * rstd * gm0.w + bt0.w;
            z1.x = (z1.x - mean) * rstd * gm1.x + bt1.x; z1.y = (z1.y - mean) * rstd * gm1.y + bt1.y;
            z1.z = (z1.z - mean) * rstd * gm1.z + bt1.z; z1.w = (z1.w - mean) * rstd * gm1.w + bt1.w;
            if (!ok0) z0 = f4zero();
            if (!ok1) z1 = f4zero();
        }
        float* x = xs + g * kDMax;
        reinterpret_cast<float4*>(x)[lane] = z0;
        if (lane < kD4Max - 64) reinterpret_cast<float4*>(x)[64 + lane] = z1;
        if (writer && r0 + g < R && s.out != nullptr) {
            if (ok0) reinterpret_cast<float4*>(s.out + row * d)[lane] = z0;
            if (ok1) reinterpret_cast<float4*>(s.out + row * d)[64 + lane] = z1;
        }
    }
};

// float4 of the LDS buffer a block kernel shares between RowGather's slice sums and ColDot's partial sums (with G = 1
// the eight slices of kD4Max float4 outgrow ColDot's G * kNT)
template <int G>
constexpr int part_f4() { return G * kNT > RowGather<G, kNW>::PSUM ? G * kNT : RowGather<G, kNW>::PSUM; }

// Dot products of up to 4 * kNW * NPASS weight rows (k contiguous) with the G LDS vectors xs[g]: 16 lanes per weight
// row, four weight rows per wave and pass; the weights stay in registers for all G rows.  load() only issues the weight
// loads (nothing depends on xs), run() consumes them.  rowoff(r): element offset of weight row r (and bias index
// bidx(r)); both are evaluated per lane on 32-bit integers.
template <int NPASS>
struct RowDot {
    float4 w[NPASS][5];
    float bv[NPASS];
    template <typename RowIdx>
    __device__ __forceinline__ void load(const float* __restrict__ W, const float* __restrict__ bias, int ld,
                                         RowIdx rowidx, int nrows, int d4) {
        const int lane = threadIdx.x & 63, wave = wave_id(), sub = lane >> 4, i = lane & 15;
        uint32_t col[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) col[it] = 16u * (uint32_t)min(i + 16 * it, d4 - 1);     // beyond d: xs is zero there
#pragma unroll
        for (int p = 0; p < NPASS; ++p) {
            const int r = min(4 * kNW * p + 4 * wave + sub, nrows - 1);
            const uint32_t ri = (uint32_t)rowidx(r);
            const uint32_t ro = ri * (uint32_t)ld * 4u;
#pragma unroll
            for (int it = 0; it < 5; ++it) w[p][it] = ld4o(W, ro + col[it]);
            bv[p] = bias ? bias[ri] : 0.f;     // fetched with the weights: a load inside run() would stall it
        }
    }
    // ys[g * ystride + r] = (dot(W[rowidx(r)], xs[g]) + bias[rowidx(r)]) * scale   (relu: max(., 0))
    template <int G>
    __device__ __forceinline__ void run(const float* xs, int nrows, float* ys, int ystride, float scale, bool relu) const {
        const int lane = threadIdx.x & 63, wave = wave_id(), sub = lane >> 4, i = lane & 15;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            float4 xr[5];
#pragma unroll
            for (int it = 0; it < 5; ++it) xr[it] = reinterpret_cast<const float4*>(xs + g * kDMax)[i + 16 * it];
#pragma unroll
            for (int p = 0; p < NPASS; ++p) {
                f32x2 acc = {0.f, 0.f};
#pragma unroll
                for (int it = 0; it < 5; ++it) acc = pkfma(w[p][it], xr[it], acc);
                const float t = sum16(acc.x + acc.y);
                const int r = 4 * kNW * p + 4 * wave + sub;
                if (i == 0 && r < nrows) {
                    const float y = (t + bv[p]) * scale;
                    ys[g * ystride + r] = relu ? fmaxf(y, 0.f) : y;
                }
            }
        }
    }
};

// out[g][n] = sum_{j < nj} o[g][j] * Wt[(j0 + j) * ld + n] for n < d (Wt = transposed weight: one k per row, n
// contiguous).  NG = min(8, kNT / (d/4)) thread groups take every NG-th j (nj <= NG * JMAX); their float4 partial
// sums meet in LDS.  o[g][.] must be zero for nj <= j < NG * JMAX.
template <int JMAX>
struct ColDot {
    float4 w[JMAX];
    __device__ __forceinline__ void load(const float* __restrict__ Wt, int ld, int j0, int nj, int d4) {
        const int NG = min(kNT / d4, 8);
        const int tid = threadIdx.x;
        const int grp = min(tid / d4, NG - 1), c = tid - grp * d4 < d4 ? tid - grp * d4 : 0;
        const uint32_t co = 16u * (uint32_t)c;
#pragma unroll
        for (int jj = 0; jj < JMAX; ++jj) {
            const int j = min(grp + NG * jj, nj - 1);
            w[jj] = ld4o(Wt, (uint32_t)(j0 + j) * (uint32_t)ld * 4u + co);
        }
    }
    // o: LDS [G][ostride]; part: LDS float4[NG * G * d4] (<= G * kNT); out row g at out + g * out_gs floats, rows g >= nvalid skipped
    template <int G>
    __device__ __forceinline__ void run(const float* o, int ostride, int d4, float4* part, float* __restrict__ out,
                                        int64_t out_gs, int nvalid) const {
        const int NG = min(kNT / d4, 8);
        const int tid = threadIdx.x;
        const int grp = tid / d4, c = tid - grp * d4;
        if (grp < NG) {
#pragma unroll
            for (int g = 0; g < G; ++g) {
                f32x2 lo = {0.f, 0.f}, hi = {0.f, 0.f};
#pragma unroll
                for (int jj = 0; jj < JMAX; ++jj) {
                    const float oj = o[g * ostride + grp + NG * jj];
                    lo = __builtin_elementwise_fma(f32x2{oj, oj}, f32x2{w[jj].x, w[jj].y}, lo);
                    hi = __builtin_elementwise_fma(f32x2{oj, oj}, f32x2{w[jj].z, w[jj].w}, hi);
                }
                part[(grp * G + g) * d4 + c] = make_float4(lo.x, lo.y, hi.x, hi.y);
            }
        }
        __syncthreads();
        for (int idx = tid; idx < G * d4; idx += kNT) {
            const int g = idx / d4, t = idx - g * d4;
            float4 s = part[g * d4 + t];
            for (int gg = 1; gg < NG; ++gg) f4add(s, part[(gg * G + g) * d4 + t]);
            if (g < nvalid) reinterpret_cast<float4*>(out + g * out_gs)[t] = s;
        }
    }
};

__device__ __forceinline__ float4 mask_cols(float4 v, int c, int dh) {   // zero the pad columns of a 32-float row
    const int j = 4 * c;
    if (j + 0 >= dh) v.x = 0.f;
    if (j + 1 >= dh) v.y = 0.f;
    if (j + 2 >= dh) v.z = 0.f;
    if (j + 3 >= dh) v.w = 0.f;
    return v;
}

// ---------------------------------------------------------------------------------------------------------
// Attention of one WAVE over a range of key / value rows: lane (p8 = lane >> 3, c = lane & 7) holds float4 c of the
// positions p0 + 8 q + p8 (q < NPC) of a chunk in registers.  Scores, softmax and P.V never touch LDS and need no
// barrier; a range longer than one chunk (8 * NPC positions) continues with a running maximum (the usual rescaling of
// the sums; with one chunk it is the plain two-pass softmax).  NQ query rows can share the same keys / values (beam
// search: the hypotheses of a caption).
// ---------------------------------------------------------------------------------------------------------
template <int NPC>
struct KVRegs {
    float4 k[NPC], v[NPC];
    // offk(p) / offv(p): byte offset (from kbase / vbase, both wave-uniform) of the 32-float row of position p < len
    template <bool STREAM, typename OffK, typename OffV>
    __device__ __forceinline__ void load(const float* kbase, const float* vbase, int p0, int len, OffK offk, OffV offv) {
        const int lane = threadIdx.x & 63, p8 = lane >> 3, c = lane & 7;
#pragma unroll
        for (int q = 0; q < NPC; ++q) {
            const uint32_t o = offk(min(p0 + 8 * q + p8, len - 1)) + 16u * (uint32_t)c;    // past the range: a copy of the last row
            k[q] = STREAM ? ld4o_stream(kbase, o) : ld4o(kbase, o);
        }
#pragma unroll
        for (int q = 0; q < NPC; ++q) {
            const uint32_t o = offv(min(p0 + 8 * q + p8, len - 1)) + 16u * (uint32_t)c;
            v[q] = STREAM ? ld4o_stream(vbase, o) : ld4o(vbase, o);
        }
    }
    // the same with this lane's NPC row offsets already known (off[q]: byte offset of the row of position p0 + 8 q + p8,
    // clamped by the caller; keys and values share the addressing)
    __device__ __forceinline__ void load_at(const float* kbase, const float* vbase, const uint32_t (&off)[NPC]) {
        const uint32_t c16 = 16u * (uint32_t)(threadIdx.x & 7);
#pragma unroll
        for (int q = 0; q < NPC; ++q) k[q] = ld4o(kbase, off[q] + c16);
#pragma unroll
        for (int q = 0; q < NPC; ++q) v[q] = ld4o(vbase, off[q] + c16);
    }
};

struct AttnState {      // running softmax state of one query row in one wave
    float m, l;         // wave-uniform maximum; this lane's share of the sum of weights
    float4 acc;         // this lane's share of sum of weight x value (columns 4c .. 4c+3)
    __device__ __forceinline__ void init() { m = -INFINITY; l = 0.f; acc = f4zero(); }
};

// pnew >= 0: position pnew is not in memory yet -- its key / value (kn, vn: this lane's float4 c) come from registers.
// The chunk's registers are masked in place (pad columns, rows past the range).
// STORE: the raw scores of query row n also go to sdst[n * sstride + p] (LDS); lane (p8, c < NPC) stores position
// p0 + 8 c + p8, so one instruction writes the chunk's 56 scores contiguously.
template <int NPC, int NQ, bool STORE = false>
__device__ __forceinline__ void attend_chunk(KVRegs<NPC>& kv, const float4 (&q4)[NQ], int p0, int len, int dh,
                                             int pnew, const float4& kn, const float4& vn, AttnState (&st)[NQ],
                                             float* sdst = nullptr, int sstride = 0) {
    const int lane = threadIdx.x & 63, p8 = lane >> 3, c = lane & 7;
    float4 (&kk)[NPC] = kv.k;
    float4 (&vv)[NPC] = kv.v;
#pragma unroll
    for (int q = 0; q < NPC; ++q) {
        const int p = p0 + 8 * q + p8;
        // rows past the range were fetched from a clamped address: their bits must not reach the sums
        kk[q] = p == pnew ? kn : (p < len ? mask_cols(kk[q], c, dh) : f4zero());
        vv[q] = p == pnew ? vn : (p < len ? mask_cols(vv[q], c, dh) : f4zero());
    }
#pragma unroll
    for (int n = 0; n < NQ; ++n) {
        float sc[NPC];
        float mc = -INFINITY;
#pragma unroll
        for (int q = 0; q < NPC; ++q) {
            const float s = sum8(dot4(q4[n], kk[q]));
            sc[q] = p0 + 8 * q + p8 < len ? s : -INFINITY;
            mc = fmaxf(mc, sc[q]);
        }
        if constexpr (STORE) {
            float v = sc[0];
#pragma unroll
            for (int q = 1; q < NPC; ++q) v = c == q ? sc[q] : v;
            const int p = p0 + 8 * c + p8;
            if (c < NPC && p < len) sdst[n * sstride + p] = v;
        }
        mc = wave_max(mc);
        const float mnew = fmaxf(st[n].m, mc);
        const float rescale = st[n].m == -INFINITY ? 0.f : __expf(st[n].m - mnew);
        st[n].l *= rescale;
        st[n].acc.x *= rescale; st[n].acc.y *= rescale; st[n].acc.z *= rescale; st[n].acc.w *= rescale;
#pragma unroll
        for (int q = 0; q < NPC; ++q) {
            const float e = sc[q] == -INFINITY ? 0.f : __expf(sc[q] - mnew);
            st[n].l += e;
            st[n].acc.x = fmaf(e, vv[q].x, st[n].acc.x); st[n].acc.y = fmaf(e, vv[q].y, st[n].acc.y);
            st[n].acc.z = fmaf(e, vv[q].z, st[n].acc.z); st[n].acc.w = fmaf(e, vv[q].w, st[n].acc.w);
        }
        st[n].m = mnew;
    }
}

// Sum a wave's shares: afterwards every lane holds the wave's sum of weights and (in acc) the weighted values of its
// columns 4c .. 4c+3.  A position's weight sits in its 8 column lanes, hence the exact factor 1/8.
__device__ __forceinline__ void attend_reduce(AttnState& st) {
    st.l = wave_sum(st.l) * 0.125f;
    st.acc.x += dpp_f32<kDppRor8>(st.acc.x); st.acc.y += dpp_f32<kDppRor8>(st.acc.y);
    st.acc.z += dpp_f32<kDppRor8>(st.acc.z); st.acc.w += dpp_f32<kDppRor8>(st.acc.w);
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        st.acc.x += __shfl_xor(st.acc.x, off, 64); st.acc.y += __shfl_xor(st.acc.y, off, 64);
        st.acc.z += __shfl_xor(st.acc.z, off, 64); st.acc.w += __shfl_xor(st.acc.w, off, 64);
    }
}

struct LayerW {
    const float *in_w, *in_b;      // self: (3d, d) packed in_proj; cross: its first d rows (q)
    const float *out_wt;           // (d, d) TRANSPOSED out_proj weight (row = input feature)
    RowSrc src;                    // how this block's input row is formed
    float* part;                   // (R, H, d) partial out-projection rows written here
};

// ---------------------------------------------------------------------------------------------------------
// Greedy selection folded into the first self-attention block of the NEXT step (ick_decode_ctx.sel_state != NULL):
// the workgroups of a row group pick the row's token of step `step` = pos - 1 from the vocabulary kernel's per-tile
// candidates and the pointer scores, apply predict()'s bookkeeping (geo-aware/models.py:410-441: <end>, repeated n-gram
// clean-up, pointer masks) and embed the token -- one launch per token less (the selection kernel alone was 6.5 us of a
// ~85 us step).  Every head's workgroup repeats the decision from the SAME inputs: candidates and pointer scores of the
// previous kernels, and a 12-int window {output[step-1 .. step-5], runner-ups of steps step-1 .. step-3, ended flag} kept
// in two alternating buffers, so that the one workgroup that records the decision (head 0: output / history / flags /
// counter / caption buffer / next window) never writes what the others read.
// ---------------------------------------------------------------------------------------------------------
struct SelFuse : GreedySel {
    const int32_t* st_in; int32_t* st_out;           // (R, 12)
};

__device__ __forceinline__ uint64_t top_key(float v, int idx) {      // larger value first, then smaller index
    uint32_t u = __float_as_uint(v);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)u << 32) | (uint32_t)(0x7fffffff - idx);
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t k) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)k, off, 64), hi = __shfl_xor((uint32_t)(k >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

// xs: LDS [G][kDMax] receives the embedded rows; keys: LDS uint64 [G][kNW][2]; follow with a barrier
template <int G>
__device__ __forceinline__ void fused_select(const SelFuse& f, int64_t r0, int R, int d, int pos, float* xs, uint64_t* keys,
                                             float* xa_out, bool recorder) {
    constexpr int WPR = kNW / G;                                   // waves per row
    const int lane = threadIdx.x & 63, wave = wave_id();
    const int g = min(wave / WPR, G - 1), wr = wave - g * WPR;
    const bool mine = wave < G * WPR;
    const int64_t row = min(r0 + g, (int64_t)R - 1);
    const TokenEmbed& e = f.emb;
    const int np = e.K + e.F, i = f.step;
    // this wave's share of the row's candidates: vocabulary tiles, then pointer scores
    float v1 = -INFINITY, v2 = -INFINITY;
    int i1 = 0x7fffffff, i2 = 0x7fffffff;
    for (int t = wr * 64 + lane; mine && t < f.ntiles + np; t += 64 * WPR) {
        float a1, a2; int j1, j2;
        if (t < f.ntiles) {
            const float4 c = f.cand[row * f.ntiles + t];
            a1 = c.x; j1 = __float_as_int(c.y); a2 = c.z; j2 = __float_as_int(c.w);
        } else {
            a1 = f.ptr[row * np + (t - f.ntiles)]; j1 = e.V + (t - f.ntiles); a2 = -INFINITY; j2 = 0x7fffffff;
        }
        // merge (a1, j1) >= (a2, j2) into the lane's running pair
        const bool b1 = top_key(a1, j1) > top_key(v1, i1);
        const float n2v = b1 ? v1 : a1; const int n2i = b1 ? i1 : j1;       // the loser of the two firsts
        v1 = b1 ? a1 : v1; i1 = b1 ? j1 : i1;
        float s2v = b1 ? a2 : v2; int s2i = b1 ? j2 : i2;                    // the winner's own second
        const bool b2 = top_key(n2v, n2i) > top_key(s2v, s2i);
        v2 = b2 ? n2v : s2v; i2 = b2 ? n2i : s2i;
    }
    const uint64_t kb = wave_max_u64(top_key(v1, i1));
    const int best_i = 0x7fffffff - (int)(uint32_t)kb;
    const uint64_t ks = wave_max_u64(i1 == best_i ? top_key(v2, i2) : top_key(v1, i1));
    if (mine && lane == 0) { keys[(g * kNW + wr) * 2] = kb; keys[(g * kNW + wr) * 2 + 1] = ks; }
    __syncthreads();
    if (!mine || wr != 0) return;
    // the row's first wave: merge the waves' pairs, decide, embed
    uint64_t B = keys[(g * kNW) * 2], S2 = keys[(g * kNW) * 2 + 1];
#pragma unroll
    for (int w = 1; w < WPR; ++w) {
        const uint64_t b = keys[(g * kNW + w) * 2], s2 = keys[(g * kNW + w) * 2 + 1];
        if (b > B) { S2 = B > s2 ? B : s2; B = b; } else { S2 = b > S2 ? b : S2; }
    }
    const int best = 0x7fffffff - (int)(uint32_t)B;
    int second = 0x7fffffff - (int)(uint32_t)S2;
    if (second == 0x7fffffff) second = best;                                    // no runner-up at all
    const int32_t* st = f.st_in + row * 12;
    int po[5], ph[3];
#pragma unroll
    for (int q = 0; q < 5; ++q) po[q] = st[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) ph[q] = st[5 + q];
    const int fin = st[8];
    const GreedyStep s = greedy_step(best, second, i, po, ph, fin, f.end_token, e.V, e.K, e.has_facts);
    if (recorder && r0 + g < R && lane == 0) {
        int64_t* o = f.output + row * f.max_len;
        if (!fin) {
            o[i] = s.cur;
            if (s.ended) { f.finished[row] = 1; atomicAdd(f.n_done, 1); }
            else {
                f.hist[row * f.max_len + i] = second;
                if (s.nrw >= 1) o[i - 1] = s.rw[0];
                if (s.nrw >= 3) { o[i - 2] = s.rw[1]; o[i - 3] = s.rw[2]; }
            }
        }
        e.next_token[row] = s.tok;
        e.next_mask[row] = s.msk;
        if (f.cap_buf != nullptr && i + 1 < f.max_len) f.cap_buf[row * f.max_len + i + 1] = s.tok;
        int32_t* so = f.st_out + row * 12;
        so[0] = fin ? po[0] : s.cur; so[1] = s.rw[0]; so[2] = s.rw[1]; so[3] = s.rw[2]; so[4] = po[3];
        so[5] = s.ended ? ph[0] : second; so[6] = ph[0]; so[7] = ph[1];
        so[8] = s.ended;
    }
    // CaptionEmbedder + sqrt(d) scale + PositionEncoder of the token (geo-aware/models.py:155-181,355-357)
    const float* src = e.row(s.tok, s.msk, row, d);
    const float* pe = e.pe + (int64_t)pos * d;
    const int d4 = d >> 2;
    const bool ok0 = lane < d4, ok1 = 64 + lane < d4;
    float4 z0 = f4zero(), z1 = f4zero();
    if (ok0) {
        const float4 e4 = ld4(src + 4 * lane), p4 = ld4(pe + 4 * lane);
        z0 = make_float4(fmaf(e4.x, e.emb_scale, p4.x), fmaf(e4.y, e.emb_scale, p4.y), fmaf(e4.z, e.emb_scale, p4.z),
                         fmaf(e4.w, e.emb_scale, p4.w));
    }
    if (ok1) {
        const float4 e4 = ld4(src + 4 * (64 + lane)), p4 = ld4(pe + 4 * (64 + lane));
        z1 = make_float4(fmaf(e4.x, e.emb_scale, p4.x), fmaf(e4.y, e.emb_scale, p4.y), fmaf(e4.z, e.emb_scale, p4.z),
                         fmaf(e4.w, e.emb_scale, p4.w));
    }
    float* x = xs + g * kDMax;
    reinterpret_cast<float4*>(x)[lane] = z0;
    if (lane < kD4Max - 64) reinterpret_cast<float4*>(x)[64 + lane] = z1;
    if (recorder && r0 + g < R && xa_out != nullptr) {
        if (ok0) reinterpret_cast<float4*>(xa_out + row * d)[lane] = z0;
        if (ok1) reinterpret_cast<float4*>(xa_out + row * d)[64 + lane] = z1;
    }
}

struct SelfArgs {
    LayerW w;
    SelFuse sel;                   // used by the FSEL instantiation (first layer, pos >= 1) only
    float* kc; float* vc;          // (R, H, ML, 32) key / value cache of this layer
    const int32_t* anc;            // optional (R, ML): cache row that holds position p of row r (beam search)
    int R, d, H, dh, ML, pos;
    float scale;
    const int32_t* n_done; int n_total;
};

// ---------------------------------------------------------------------------------------------------------
// self-attention block, one workgroup per (head, group of G <= 8 rows): the head's q|k|v and out_proj weights are
// streamed once for the G rows.  Wave w normalises row w and, later, attends for it.
// ---------------------------------------------------------------------------------------------------------
constexpr int kOPad = 48;          // attention output row in LDS: head width + the zero tail the out-projection reads
template <int G, bool FSEL>
__global__ __launch_bounds__(kNT) void dec_self_kernel(SelfArgs a) {
    static_assert(G <= kNW, "one wave per row");
    __shared__ __attribute__((aligned(16))) float xs[G][kDMax];
    __shared__ uint64_t selkeys[FSEL ? G * kNW * 2 : 2];
    __shared__ __attribute__((aligned(16))) float qkv[G][128];     // q | k | v of this head (3 x dh <= 96), zero tail
    __shared__ __attribute__((aligned(16))) float o[G][kOPad];
    __shared__ __attribute__((aligned(16))) float4 part[part_f4<G>()];
    int h, grp;
    xcd_unit(h, grp, gridDim.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int64_t r0 = (int64_t)grp * G;
    const int d = a.d, d4 = d >> 2, dh = a.dh, pos = a.pos, R = a.R;
    const int done = a.n_done != nullptr ? *a.n_done : 0;           // waited for only after the loads are out
    const int64_t myrow = min(r0 + wave, (int64_t)R - 1);
    const bool have_row = wave < G && r0 + wave < R;                // wave-uniform
    ICK_STAMP(0, 0);
    RowGather<G, kNW> in;
    if constexpr (!FSEL) in.issue(a.w.src, r0, R, d);
    RowDot<3> qd;
    qd.load(a.w.in_w, a.w.in_b, d,
            [&](int rr) { const int seg = (rr >= dh) + (rr >= 2 * dh); return seg * (d - dh) + h * dh + rr; }, 3 * dh, d4);
    if (done >= a.n_total) return;                                   // every caption has ended (uniform)
    ICK_STAMP(0, 1);
    for (int idx = tid; idx < G * 32; idx += kNT) qkv[idx >> 5][96 + (idx & 31)] = 0.f;
    for (int idx = tid; idx < G * kOPad; idx += kNT) (&o[0][0])[idx] = 0.f;
    if constexpr (FSEL) {
        // the token of the previous step is chosen and embedded here: the row source is that embedding
        fused_select<G>(a.sel, r0, R, d, pos, &xs[0][0], selkeys, a.w.src.out, h == 0);
    } else {
        in.slice_sums(a.w.src, r0, R, d, part);
        __syncthreads();
        in.finish(a.w.src, r0, R, d, part, &xs[0][0], h == 0);
    }
    __syncthreads();
    ICK_STAMP(0, 2);
    // the cached keys / values of this wave's row and the out-projection slice are requested before the products run
    constexpr int NPC = 4;
    KVRegs<NPC> kv;
    const int p8 = lane >> 3, c = lane & 7;
    const int plast = max(pos - 1, 0);                               // position `pos` itself is not in the cache yet
    // Row offsets of a chunk's positions.  With beam search the cache row of position p is the ancestor's
    // (anc[row][p]): those indices are fetched for the whole chunk in ONE basic block -- as a per-position lambda inside
    // the load loop every index load sat in a branch of its own and was waited for on the spot (load, vmcnt(0), key load,
    // and the same again for the value: eight memory round trips per chunk, ISA of round 5's build).
    uint32_t coff[NPC];
    auto cache_offs = [&](int p0) {
        int pp[NPC];
        int64_t cr[NPC];
#pragma unroll
        for (int q = 0; q < NPC; ++q) pp[q] = min(min(p0 + 8 * q + p8, pos), plast);
        if (a.anc != nullptr) {      // uniform
#pragma unroll
            for (int q = 0; q < NPC; ++q) cr[q] = (int64_t)a.anc[myrow * a.ML + pp[q]];
        } else {
#pragma unroll
            for (int q = 0; q < NPC; ++q) cr[q] = myrow;
        }
#pragma unroll
        for (int q = 0; q < NPC; ++q) coff[q] = (uint32_t)(((cr[q] * a.H + h) * a.ML + pp[q]) * kDhp) * 4u;
    };
    if (have_row) { cache_offs(0); kv.load_at(a.kc, a.vc, coff); }
    ColDot<6> od;
    od.load(a.w.out_wt, d, h * dh, dh, d4);
    qd.template run<G>(&xs[0][0], 3 * dh, &qkv[0][0], 128, 1.f, false);
    __syncthreads();
    ICK_STAMP(0, 3);
    if (have_row) {                                                   // wave-uniform
        const int g = wave;
        // the new key / value row joins the cache (pad columns stay unwritten and are masked by every reader)
        if (lane < dh) a.kc[((myrow * a.H + h) * a.ML + pos) * kDhp + lane] = qkv[g][dh + lane];
        else if (lane >= 32 && lane < 32 + dh) a.vc[((myrow * a.H + h) * a.ML + pos) * kDhp + lane - 32] = qkv[g][2 * dh + lane - 32];
        float4 q4[1], kn, vn;
        const float sc = a.scale;
        q4[0].x = 4 * c + 0 < dh ? qkv[g][4 * c + 0] * sc : 0.f; q4[0].y = 4 * c + 1 < dh ? qkv[g][4 * c + 1] * sc : 0.f;
        q4[0].z = 4 * c + 2 < dh ? qkv[g][4 * c + 2] * sc : 0.f; q4[0].w = 4 * c + 3 < dh ? qkv[g][4 * c + 3] * sc : 0.f;
        kn.x = 4 * c + 0 < dh ? qkv[g][dh + 4 * c + 0] : 0.f; kn.y = 4 * c + 1 < dh ? qkv[g][dh + 4 * c + 1] : 0.f;
        kn.z = 4 * c + 2 < dh ? qkv[g][dh + 4 * c + 2] : 0.f; kn.w = 4 * c + 3 < dh ? qkv[g][dh + 4 * c + 3] : 0.f;
        vn.x = 4 * c + 0 < dh ? qkv[g][2 * dh + 4 * c + 0] : 0.f; vn.y = 4 * c + 1 < dh ? qkv[g][2 * dh + 4 * c + 1] : 0.f;
        vn.z = 4 * c + 2 < dh ? qkv[g][2 * dh + 4 * c + 2] : 0.f; vn.w = 4 * c + 3 < dh ? qkv[g][2 * dh + 4 * c + 3] : 0.f;
        AttnState st[1];
        st[0].init();
        // positions 0 .. pos; loads cover the cached ones (< pos), the new row comes from the registers above
        for (int p0 = 0; p0 <= pos; p0 += 8 * NPC) {
            if (p0 > 0) { cache_offs(p0); kv.load_at(a.kc, a.vc, coff); }
            attend_chunk<NPC, 1>(kv, q4, p0, pos + 1, dh, pos, kn, vn, st);
        }
        attend_reduce(st[0]);
        if (p8 == 0) {
            const float inv = 1.f / st[0].l;
            reinterpret_cast<float4*>(&o[g][0])[c] = make_float4(st[0].acc.x * inv, st[0].acc.y * inv, st[0].acc.z * inv,
                                                                  st[0].acc.w * inv);
        }
    }
    __syncthreads();
    ICK_STAMP(0, 4);
    od.template run<G>(&o[0][0], kOPad, d4, part, a.w.part + (r0 * a.H + h) * d, (int64_t)a.H * d, (int)min((int64_t)G, R - r0));
    ICK_STAMP(0, 5);
}

struct CrossArgs {
    LayerW w;
    const float* Kmem; const float* Vmem;     // (B, ., H, S, 32) segments of the cross K/V buffer of this layer
    int64_t kv_bs;                            // sample stride of that buffer
    int R, rows_per_sample, d, H, dh, S;
    float scale;
    const int32_t* n_done; int n_total;
};
// the ATTN variants' arguments (a type of their own: the kernel arguments of the others stay as they were)
struct CrossAttnArgs : CrossArgs {
    float* attn; int64_t attn_rs;             // (R, ., H, S) weights of this step and layer, row stride
};

// ---------------------------------------------------------------------------------------------------------
// cross-attention block, one workgroup per (head, group of G rows).  SHARED: the G rows are hypotheses of one caption
// (beam search) -- its K and V are read once for all of them, each of the eight waves taking an eighth of the S memory
// rows; otherwise the waves are dealt out as (row, part of S).  Every wave keeps its part's keys and values in
// registers; the parts of a row meet in LDS as (maximum, sum, weighted values) records.
// ATTN: the attention weights are written too.  A wave keeps its part's raw scores in LDS while it attends (the final
// maximum M and sum L exist only after the parts have met); after the merge the workgroup writes exp(s - M) / L.
// ---------------------------------------------------------------------------------------------------------
// ATTN: the raw scores of the G rows of a workgroup, (G, kSMax) in LDS (only the ATTN variants reference it, so the
// others' LDS layout and code stay as they were)
template <int G>
__device__ __forceinline__ float* cross_scores() {
    __shared__ float ss[G][kSMax];
    return &ss[0][0];
}

template <int G, bool SHARED, bool ATTN>
__global__ __launch_bounds__(kNT) void dec_cross_kernel(std::conditional_t<ATTN, CrossAttnArgs, CrossArgs> a) {
    constexpr int PARTS = SHARED ? kNW : kNW / G;       // waves per row
    constexpr int NQ = SHARED ? G : 1;                  // query rows per wave
    constexpr int NPC = 7;                              // 56 memory rows per chunk and wave
    static_assert(SHARED || G == 1 || G == 2 || G == 4 || G == 8, "rows of different captions: 1, 2, 4 or 8 per workgroup");
    static_assert(G <= kNW, "one wave per row");
    __shared__ __attribute__((aligned(16))) float xs[G][kDMax];
    __shared__ __attribute__((aligned(16))) float qs[G][32];
    __shared__ __attribute__((aligned(16))) float o[G][kOPad];
    __shared__ __attribute__((aligned(16))) float4 part[part_f4<G>()];
    __shared__ __attribute__((aligned(16))) float4 pacc[G][kNW][8];
    __shared__ float pm[G][kNW], pl[G][kNW];
    int h, grp;
    xcd_unit(h, grp, gridDim.y);
    const int tid = threadIdx.x, lane = tid & 63, wave = wave_id();
    const int64_t r0 = (int64_t)grp * G;
    const int d = a.d, d4 = d >> 2, dh = a.dh, S = a.S, R = a.R;
    const int done = a.n_done != nullptr ? *a.n_done : 0;
    ICK_STAMP(1, 0);
    RowGather<G, kNW> in;
    in.issue(a.w.src, r0, R, d);
    ICK_STAMP(1, 1);
    RowDot<1> qd;
    qd.load(a.w.in_w, a.w.in_b, d, [&](int rr) { return h * dh + rr; }, dh, d4);
    ICK_STAMP(1, 2);
    // this wave's part of the memory
    const int g_mine = SHARED ? 0 : wave / PARTS, prt = SHARED ? wave : wave % PARTS;
    const int Sp = ((S + PARTS - 1) / PARTS + 7) & ~7;
    const int lo = prt * Sp, len = max(0, min(S - lo, Sp));
    const int64_t b = min(r0 + g_mine, (int64_t)R - 1) / a.rows_per_sample;
    const float* Kb = a.Kmem + b * a.kv_bs + ((int64_t)h * S + min(lo, S - 1)) * kDhp;
    const float* Vb = a.Vmem + b * a.kv_bs + ((int64_t)h * S + min(lo, S - 1)) * kDhp;
    auto kv_off = [&](int p) { return (uint32_t)p * (kDhp * 4u); };
    KVRegs<NPC> kv;
    kv.template load<true>(Kb, Vb, 0, max(len, 1), kv_off, kv_off);
    ICK_STAMP(1, 3);
    ColDot<6> od;
    od.load(a.w.out_wt, d, h * dh, dh, d4);
    ICK_STAMP(1, 4);
    if (done >= a.n_total) return;
    ICK_STAMP(1, 5);
    in.slice_sums(a.w.src, r0, R, d, part);
    ICK_STAMP(1, 6);
    for (int idx = tid; idx < G * 32; idx += kNT) (&qs[0][0])[idx] = 0.f;
    for (int idx = tid; idx < G * kOPad; idx += kNT) (&o[0][0])[idx] = 0.f;
    __syncthreads();
    ICK_STAMP(1, 7);
    in.finish(a.w.src, r0, R, d, part, &xs[0][0], h == 0);
    ICK_STAMP(1, 8);
    __syncthreads();
    ICK_STAMP(1, 9);
    qd.template run<G>(&xs[0][0], dh, &qs[0][0], 32, a.scale, false);     // q * 1/sqrt(dh), as nn.MultiheadAttention scales it
    ICK_STAMP(1, 10);
    __syncthreads();
    ICK_STAMP(1, 11);
    const int p8 = lane >> 3, c = lane & 7;
    {
        float4 q4[NQ];
        AttnState st[NQ];
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            q4[n] = reinterpret_cast<const float4*>(&qs[SHARED ? n : g_mine][0])[c];   // pad entries are zero
            st[n].init();
        }
        const float4 none = f4zero();
        for (int p0 = 0; p0 < len; p0 += 8 * NPC) {
            if (p0 > 0) kv.template load<true>(Kb, Vb, p0, len, kv_off, kv_off);
            if constexpr (ATTN)
                attend_chunk<NPC, NQ, true>(kv, q4, p0, len, dh, -1, none, none, st,
                                            cross_scores<G>() + (SHARED ? 0 : g_mine) * kSMax + lo, kSMax);
            else
                attend_chunk<NPC, NQ>(kv, q4, p0, len, dh, -1, none, none, st);
        }
#pragma unroll
        for (int n = 0; n < NQ; ++n) {
            attend_reduce(st[n]);
            const int g = SHARED ? n : g_mine;
            if (p8 == 0) pacc[g][prt][c] = st[n].acc;
            if (lane == 0) { pm[g][prt] = st[n].m; pl[g][prt] = st[n].l; }
        }
    }
    ICK_STAMP(1, 12);
    __syncthreads();
    ICK_STAMP(1, 13);
    if (tid < G * 8) {
        const int g = tid >> 3, cc = tid & 7;
        float M = pm[g][0];
#pragma unroll
        for (int w = 1; w < PARTS; ++w) M = fmaxf(M, pm[g][w]);
        float L = 0.f;
        float4 t = f4zero();
#pragma unroll
        for (int w = 0; w < PARTS; ++w) {
            const float f = pm[g][w] == -INFINITY ? 0.f : __expf(pm[g][w] - M);
            L = fmaf(pl[g][w], f, L);
            const float4 u = pacc[g][w][cc];
            t.x = fmaf(u.x, f, t.x); t.y = fmaf(u.y, f, t.y); t.z = fmaf(u.z, f, t.z); t.w = fmaf(u.w, f, t.w);
        }
        const float inv = 1.f / L;
        reinterpret_cast<float4*>(&o[g][0])[cc] = make_float4(t.x * inv, t.y * inv, t.z * inv, t.w * inv);
        if constexpr (ATTN) {
            if (cc == 0) { pm[g][0] = M; pl[g][0] = inv; }      // tid < G * 8 is one wave: its reads are issued above
        }
    }
    __syncthreads();
    ICK_STAMP(1, 14);
    od.template run<G>(&o[0][0], kOPad, d4, part, a.w.part + (r0 * a.H + h) * d, (int64_t)a.H * d, (int)min((int64_t)G, R - r0));
    ICK_STAMP(1, 15);
    if constexpr (ATTN) {
        // the rows' weights, exp(s - M) / L, in one coalesced pass of the whole workgroup (shared groups divide the rows
        // of a caption, so only unshared groups can run past the last row)
        const int gn = (int)min((int64_t)G, R - r0);
        const float* ss = cross_scores<G>();
        float* dst = a.attn + r0 * a.attn_rs + (int64_t)h * S;
        for (int g = 0; g < gn; ++g) {
            const float M = pm[g][0], inv = pl[g][0];
            for (int p = tid; p < S; p += kNT) dst[g * a.attn_rs + p] = __expf(ss[g * kSMax + p] - M) * inv;
        }
    }
}

struct FfnArgs {
    const float *w1, *b1;          // (FF, d), (FF)
    const float *w2t;              // (FF, d) TRANSPOSED linear2 weight
    RowSrc src;
    float* part;                   // (R, FF/64, d)
    int R, d, FF;
    const int32_t* n_done; int n_total;
};

// ---------------------------------------------------------------------------------------------------------
// feed-forward block, one workgroup per (64 hidden units, group of G rows)
// ---------------------------------------------------------------------------------------------------------
template <int G>
__global__ __launch_bounds__(kNT) void dec_ffn_kernel(FfnArgs a) {
    static_assert(G <= kNW, "one wave per row");
    __shared__ __attribute__((aligned(16))) float xs[G][kDMax];
    __shared__ __attribute__((aligned(16))) float f[G][96];
    __shared__ __attribute__((aligned(16))) float4 part[part_f4<G>()];
    int ch, grp;
    xcd_unit(ch, grp, gridDim.y);
    const int tid = threadIdx.x, nch = gridDim.x;
    const int64_t r0 = (int64_t)grp * G;
    const int d = a.d, d4 = d >> 2, R = a.R;
    const int j0 = ch * 64, nj = min(64, a.FF - j0);
    const int done = a.n_done != nullptr ? *a.n_done : 0;
    ICK_STAMP(2, 0);
    RowGather<G, kNW> in;
    in.issue(a.src, r0, R, d);
    RowDot<2> fd;
    fd.load(a.w1, a.b1, d, [&](int rr) { return j0 + rr; }, nj, d4);
    ColDot<11> od;
    od.load(a.w2t, d, j0, nj, d4);
    if (done >= a.n_total) return;
    ICK_STAMP(2, 1);
    in.slice_sums(a.src, r0, R, d, part);
    for (int idx = tid; idx < G * 96; idx += kNT) (&f[0][0])[idx] = 0.f;
    __syncthreads();
    in.finish(a.src, r0, R, d, part, &xs[0][0], ch == 0);
    __syncthreads();
    ICK_STAMP(2, 2);
    fd.template run<G>(&xs[0][0], nj, &f[0][0], 96, 1.f, true);
    __syncthreads();
    ICK_STAMP(2, 3);
    od.template run<G>(&f[0][0], 96, d4, part, a.part + (r0 * nch + ch) * d, (int64_t)nch * d, (int)min((int64_t)G, R - r0));
    ICK_STAMP(2, 4);
}

struct HeadArgs {
    RowSrc src;                    // final LayerNorm of the last layer; out = h (R, d)
    const float* gate;             // optional (R, d): fc_predicate(predicate indicator)
    float* hv;                     // (R, d) h * gate (== h when gate is null)
    const float *ee, *we, *be;     // entities_encoded (B, K, d), fc_entity
    const float *fe, *wf, *bf;     // facts_encoded (B, F, d), fc_fact (null for geo)
    const float* eib;              // (R, F) indicator
    float* ptr;                    // (R, K + F) pointer scores
    int R, rows_per_sample, d, K, F;
    const int32_t* n_done; int n_total;
};

// One row of the score head: final LayerNorm -> h (x gate) -> pointer scores.  Written for four waves; in a wider workgroup
// (the merged head + vocabulary launch) the waves beyond the fourth only keep the barriers company.
__device__ __forceinline__ void head_row(const HeadArgs& a, const int64_t r, float* xs, float4* psum) {
    const int tid = threadIdx.x;
    const int d = a.d, d4 = d >> 2;
    const int64_t b = r / a.rows_per_sample;
    const int lane = tid & 63, wave = wave_id(), sub = lane >> 4, i = lane & 15;
    const int done = a.n_done != nullptr ? *a.n_done : 0;
    RowGather<1, 4> in;
    in.issue(a.src, r, a.R, d);
    const float* wq[2] = {a.we, a.fe != nullptr && a.F > 0 ? a.wf : a.we};
    float4 wr2[2][5];
#pragma unroll
    for (int pp = 0; pp < 2; ++pp)
#pragma unroll
        for (int it = 0; it < 5; ++it) wr2[pp][it] = ld4(wq[pp] + 4 * min(i + 16 * it, d4 - 1));
    const float bias2[2] = {a.be[0], a.fe != nullptr && a.F > 0 ? a.bf[0] : 0.f};
    if (done >= a.n_total) return;
    in.slice_sums(a.src, r, a.R, d, psum);
    // the first context rows are requested while wave 0 normalises
    const float* ctx0 = a.ee;
    const int n0 = a.K;
    float4 cv0[5];
    {
        const float* cr = ctx0 + (b * n0 + min(4 * wave + sub, n0 - 1)) * d;
#pragma unroll
        for (int it = 0; it < 5; ++it) cv0[it] = ld4(cr + 4 * min(i + 16 * it, d4 - 1));
    }
    __syncthreads();
    in.finish(a.src, r, a.R, d, psum, xs, true);
    __syncthreads();
    if (tid < 256)
        for (int c = tid; c < d; c += 256) a.hv[r * d + c] = a.gate ? xs[c] * a.gate[r * d + c] : xs[c];
    if (wave >= 4) return;      // no barrier below
    float4 xr[5];
#pragma unroll
    for (int it = 0; it < 5; ++it) xr[it] = reinterpret_cast<const float4*>(xs)[i + 16 * it];      // zero beyond d
    for (int part = 0; part < 2; ++part) {
        const float* ctx = part == 0 ? a.ee : a.fe;
        const int n = part == 0 ? a.K : a.F;
        if (ctx == nullptr || n <= 0) continue;
        float4 wr[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) wr[it] = wr2[part][it];
        const float bias = bias2[part];
        for (int k0 = 0; k0 < n; k0 += 16) {
            const int k = k0 + 4 * wave + sub;
            float4 cv[5];
            if (part == 0 && k0 == 0) {
#pragma unroll
                for (int it = 0; it < 5; ++it) cv[it] = cv0[it];
            } else {
                const float* cr = ctx + (b * n + min(k, n - 1)) * d;
#pragma unroll
                for (int it = 0; it < 5; ++it) cv[it] = ld4(cr + 4 * min(i + 16 * it, d4 - 1));
            }
            float acc = 0.f;
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                // (h * ctx) * w summed over d, the order of the reference's broadcast product
                acc = fmaf(__fmul_rn(xr[it].x, cv[it].x), wr[it].x, acc);
                acc = fmaf(__fmul_rn(xr[it].y, cv[it].y), wr[it].y, acc);
                acc = fmaf(__fmul_rn(xr[it].z, cv[it].z), wr[it].z, acc);
                acc = fmaf(__fmul_rn(xr[it].w, cv[it].w), wr[it].w, acc);
            }
            acc = sum16(acc);
            if (i == 0 && k < n) {
                const float ind = (part == 1 && a.eib) ? a.eib[r * a.F + k] : 1.f;
                a.ptr[r * (a.K + a.F) + (part == 0 ? 0 : a.K) + k] = acc * ind + bias;
            }
        }
    }
}

__global__ __launch_bounds__(256) void dec_head_kernel(HeadArgs a) {
    __shared__ __attribute__((aligned(16))) float xs[kDMax];
    __shared__ __attribute__((aligned(16))) float4 psum[4 * kD4Max];
    head_row(a, blockIdx.x, xs, psum);
}

struct VocabArgs {
    const float* hv;               // (R, d)
    const float *wv, *bv;          // (V, d), (V)
    float* scores; int64_t ld;     // optional (R, ld) logits
    float4* cand;                  // (R, ntiles) {best value, best index, second value, second index}
    int R, d, V, ntiles;
    const int32_t* n_done; int n_total;
};

// ---------------------------------------------------------------------------------------------------------
// vocabulary logits: workgroup = kVocabTile words x all rows (blocks of 32), the eight waves split K; fp32 MFMA
// 16x16x4.  One workgroup per CU at V = 10 000 (209 of them): its 58 KB weight slice is fetched once and stays in
// registers for every block of 32 rows (beam search decodes captions x beams rows).
// ---------------------------------------------------------------------------------------------------------
constexpr int kVocabCT = kVocabTile / 16;     // 16-word column tiles per workgroup
constexpr int kVocabKC = 3;                   // 16-wide k chunks per wave: 8 x 3 x 16 = 384 >= kDMax
using VocabRed = float[kNW][2][kVocabCT][16][17];     // LDS: the waves' partial 32 x 48 products

// The tile of one workgroup, the part dec_vocab_kernel and dec_headvocab_kernel share: the wave's K slice of the 48
// weight rows in registers, the products of a block of 32 rows (the kernels differ in where the rows come from: global
// memory, or the LN-on-load rows in LDS), and the epilogue that reduces the eight slices.
struct VocabTile {
    float4 bw[kVocabCT][kVocabKC];
    uint32_t koff[kVocabKC];                     // byte offset of this lane's float4 of k chunk t in a row of d floats
    bool kok[kVocabKC];                          // d % 4 == 0: a float4 is entirely inside or outside
    float biasv[kVocabCT];
    // (The pieces take plain values, not the kernel's VocabArgs by reference: a kernel argument whose address is taken
    // is copied to private memory first, and the loads through its pointers stop being scalar loads.)
    // issues the loads only: the weights first (HBM, the longest wait of either kernel), then the bias
    __device__ __forceinline__ void load(const float* wv, const float* bv, int V, int d, int n0) {
        const int tid = threadIdx.x, lane = tid & 63, wave = wave_id(), fi = lane & 15, fq = lane >> 4, cp = tid & 15;
#pragma unroll
        for (int t = 0; t < kVocabKC; ++t) {
            const int k = 16 * (kVocabKC * wave + t) + 4 * fq;
            kok[t] = k < d;
            koff[t] = kok[t] ? 4u * (uint32_t)k : 0u;
        }
#pragma unroll
        for (int ct = 0; ct < kVocabCT; ++ct) {
            const uint32_t rb = (uint32_t)min(n0 + 16 * ct + fi, V - 1) * (uint32_t)d * 4u;
#pragma unroll
            for (int t = 0; t < kVocabKC; ++t) {
                bw[ct][t] = ld4o(wv, rb + koff[t]);
                if (!kok[t]) bw[ct][t] = f4zero();
            }
        }
#pragma unroll
        for (int e = 0; e < kVocabCT; ++e) biasv[e] = bv[min(n0 + kVocabCT * cp + e, V - 1)];
    }
    // av0 / av1: rows fi and 16 + fi of the block; follow with a barrier
    __device__ __forceinline__ void mma(const float4 (&av0)[kVocabKC], const float4 (&av1)[kVocabKC], VocabRed& red) const {
        const int lane = threadIdx.x & 63, wave = wave_id(), fi = lane & 15, fq = lane >> 4;
#pragma unroll
        for (int ct = 0; ct < kVocabCT; ++ct) {
            f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < kVocabKC; ++t) {
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[t].x, bw[ct][t].x, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[t].x, bw[ct][t].x, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[t].y, bw[ct][t].y, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[t].y, bw[ct][t].y, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[t].z, bw[ct][t].z, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[t].z, bw[ct][t].z, acc1, 0, 0, 0);
                acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av0[t].w, bw[ct][t].w, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av1[t].w, bw[ct][t].w, acc1, 0, 0, 0);
            }
            // C/D map: col = lane & 15, row = (lane >> 4) * 4 + reg
#pragma unroll
            for (int rg = 0; rg < 4; ++rg) {
                red[wave][0][ct][fq * 4 + rg][fi] = acc0[rg];
                red[wave][1][ct][fq * 4 + rg][fi] = acc1[rg];
            }
        }
    }
    // thread (row = tid >> 4 of the block, three columns): sum the eight K slices in a fixed order, add the bias, store
    // the logits (optional) and the tile's top-2 candidates of the row; gr: the row's global index
    __device__ __forceinline__ void epilogue(float* scores, int64_t ld, float4* cand, int ntiles, int R, int V, int n0,
                                             int gr, const VocabRed& red) const {
        const int row = threadIdx.x >> 4, cp = threadIdx.x & 15;
        Top2 t2{-INFINITY, -INFINITY, kNone, kNone};
#pragma unroll
        for (int e = 0; e < kVocabCT; ++e) {
            const int col = kVocabCT * cp + e, n = n0 + col, ct = col >> 4, cc = col & 15;
            float v = red[0][row >> 4][ct][row & 15][cc];
#pragma unroll
            for (int w = 1; w < kNW; ++w) v += red[w][row >> 4][ct][row & 15][cc];
            if (n < V) {
                v += biasv[e];
                if (scores != nullptr && gr < R) scores[(int64_t)gr * ld + n] = v;
                top2_push(t2, v, n);
            }
        }
        t2 = top2_merge_row(t2);                // empty slots carry (-inf, kNone): they never displace anything
        if (cp == 0 && gr < R)
            cand[(int64_t)gr * ntiles + blockIdx.x] =
                make_float4(t2.v1, __int_as_float(t2.i1), t2.v2, __int_as_float(t2.i2));
    }
};

__global__ __launch_bounds__(kNT) void dec_vocab_kernel(VocabArgs a) {
    __shared__ __attribute__((aligned(16))) VocabRed red;
    const int tid = threadIdx.x, fi = tid & 15;
    const int n0 = blockIdx.x * kVocabTile;
    const int d = a.d;
    const int done = a.n_done != nullptr ? *a.n_done : 0;
    ICK_STAMP(3, 0);
    VocabTile vt;
    vt.load(a.wv, a.bv, a.V, a.d, n0);
    if (done >= a.n_total) return;
    for (int m0 = 0; m0 < a.R; m0 += 32) {
        const uint32_t ra0 = (uint32_t)min(m0 + fi, a.R - 1) * (uint32_t)d * 4u,
                       ra1 = (uint32_t)min(m0 + 16 + fi, a.R - 1) * (uint32_t)d * 4u;
        float4 av0[kVocabKC], av1[kVocabKC];
#pragma unroll
        for (int t = 0; t < kVocabKC; ++t) {
            av0[t] = ld4o(a.hv, ra0 + vt.koff[t]);
            av1[t] = ld4o(a.hv, ra1 + vt.koff[t]);
            if (!vt.kok[t]) av0[t] = av1[t] = f4zero();
        }
        ICK_STAMP(3, 1);
        vt.mma(av0, av1, red);
        ICK_STAMP(3, 2);
        __syncthreads();
        ICK_STAMP(3, 3);
        vt.epilogue(a.scores, a.ld, a.cand, a.ntiles, a.R, a.V, n0, m0 + (tid >> 4), red);
        ICK_STAMP(3, 4);
        if (m0 + 32 < a.R) __syncthreads();       // the exchange buffer is reused by the next block of rows
    }
}

// ---------------------------------------------------------------------------------------------------------
// Score head + vocabulary logits in ONE launch for R <= 32 rows (greedy decoding): the vocabulary
// workgroups no longer wait for a launch that writes h -- each normalises the R rows itself (LN-on-load into LDS, 16
// lanes per row, four source rows' loads in flight at once: three L2 round trips, hidden behind the fetch of the
// workgroup's 58 KB weight slice from HBM), and R more workgroups of the same launch do what dec_head_kernel does
// (h, h x gate, pointer scores).  No workgroup depends on another.  One dependent launch less per token.
// The normalised rows are summed source by source in the order res, bias, partial 0, 1, ...: deterministic, the same in
// every vocabulary workgroup.
// ---------------------------------------------------------------------------------------------------------
constexpr int kHvSrc = 12;                    // residual + bias + up to 10 partial rows (heads / FFN chunks)
constexpr int kHvChunk = 4;                   // source rows in flight per lane (x 5 float4)
constexpr int kHvLd = kDMax + 4;              // LDS row stride of the normalised rows
__global__ __launch_bounds__(kNT) void dec_headvocab_kernel(HeadArgs ha, VocabArgs a) {
    __shared__ __attribute__((aligned(16))) VocabRed red;
    __shared__ __attribute__((aligned(16))) float xa[32 * kHvLd];
    __shared__ __attribute__((aligned(16))) float4 psum[4 * kD4Max];
    if ((int)blockIdx.x >= a.ntiles) {          // head role (uniform per workgroup)
        head_row(ha, (int64_t)blockIdx.x - a.ntiles, xa, psum);
        return;
    }
    const int tid = threadIdx.x, fi = tid & 15;
    const int n0 = blockIdx.x * kVocabTile;
    const int d = a.d, d4 = d >> 2;
    const int done = a.n_done != nullptr ? *a.n_done : 0;
    VocabTile vt;
    vt.load(a.wv, a.bv, a.V, a.d, n0);
    const int row = tid >> 4, cp = tid & 15;         // LN role: one row per 16 lanes
    if (done >= a.n_total) return;
    // ---- x[row] = LayerNorm(res + bias + sum of the partial rows) (x gate): lane cp holds float4 columns cp + 16 it
    {
        const RowSrc& s = ha.src;
        const int64_t r = min(row, a.R - 1);
        const int nrows = s.nparts > 0 ? s.nparts + 2 : 1;
        uint32_t col[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) col[it] = 16u * (uint32_t)min(cp + 16 * it, d4 - 1);
        float4 z[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) z[it] = f4zero();
#pragma unroll 1
        for (int half = 0; half < kHvSrc / kHvChunk; ++half) {
            float4 v[kHvChunk][5];
#pragma unroll
            for (int j = 0; j < kHvChunk; ++j) {
                const int q = min(half * kHvChunk + j, nrows - 1);
                const float* src = q == 0 ? s.res + r * d : (q == 1 ? s.bias : s.part + (r * s.nparts + (q - 2)) * d);
#pragma unroll
                for (int it = 0; it < 5; ++it) v[j][it] = ld4o(src, col[it]);
            }
#pragma unroll
            for (int j = 0; j < kHvChunk; ++j) {
                const float f = half * kHvChunk + j < nrows ? 1.f : 0.f;
#pragma unroll
                for (int it = 0; it < 5; ++it) {
                    z[it].x = fmaf(v[j][it].x, f, z[it].x); z[it].y = fmaf(v[j][it].y, f, z[it].y);
                    z[it].z = fmaf(v[j][it].z, f, z[it].z); z[it].w = fmaf(v[j][it].w, f, z[it].w);
                }
            }
            __builtin_amdgcn_sched_barrier(0);     // the next chunk's loads stay behind this chunk's sums (registers)
        }
        bool ok[5];
#pragma unroll
        for (int it = 0; it < 5; ++it) {
            ok[it] = cp + 16 * it < d4;
            if (!ok[it]) z[it] = f4zero();
        }
        if (s.nparts > 0) {
            float4 gm[5], bt[5];
#pragma unroll
            for (int it = 0; it < 5; ++it) { gm[it] = ld4o(s.gamma, col[it]); bt[it] = ld4o(s.beta, col[it]); }
            float sum = 0.f;
#pragma unroll
            for (int it = 0; it < 5; ++it) sum += (z[it].x + z[it].y) + (z[it].z + z[it].w);
            const float mean = sum16(sum) / (float)d;
            float var = 0.f;
#pragma unroll
            for (int it = 0; it < 5; ++it)
                if (ok[it]) {
                    var = fmaf(z[it].x - mean, z[it].x - mean, var); var = fmaf(z[it].y - mean, z[it].y - mean, var);
                    var = fmaf(z[it].z - mean, z[it].z - mean, var); var = fmaf(z[it].w - mean, z[it].w - mean, var);
                }
            const float rstd = rsqrtf(sum16(var) / (float)d + s.eps);
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                z[it].x = (z[it].x - mean) * rstd * gm[it].x + bt[it].x; z[it].y = (z[it].y - mean) * rstd * gm[it].y + bt[it].y;
                z[it].z = (z[it].z - mean) * rstd * gm[it].z + bt[it].z; z[it].w = (z[it].w - mean) * rstd * gm[it].w + bt[it].w;
            }
        }
        if (ha.gate != nullptr) {
#pragma unroll
            for (int it = 0; it < 5; ++it) {
                const float4 g = ld4o(ha.gate + r * d, col[it]);
                z[it].x *= g.x; z[it].y *= g.y; z[it].z *= g.z; z[it].w *= g.w;
            }
        }
#pragma unroll
        for (int it = 0; it < 5; ++it)
            reinterpret_cast<float4*>(xa + row * kHvLd)[cp + 16 * it] = ok[it] ? z[it] : f4zero();
    }
    __syncthreads();
    float4 av0[kVocabKC], av1[kVocabKC];
#pragma unroll
    for (int t = 0; t < kVocabKC; ++t) {
        av0[t] = vt.kok[t] ? *reinterpret_cast<const float4*>(xa + fi * kHvLd + (vt.koff[t] >> 2)) : f4zero();
        av1[t] = vt.kok[t] ? *reinterpret_cast<const float4*>(xa + (16 + fi) * kHvLd + (vt.koff[t] >> 2)) : f4zero();
    }
    vt.mma(av0, av1, red);
    __syncthreads();
    vt.epilogue(a.scores, a.ld, a.cand, a.ntiles, a.R, a.V, n0, row, red);
}

}  // namespace
}  // namespace ick

using namespace ick;

static RowSrc make_src(const ick_decode_ctx* c, const float* res, const float* part, int nparts, const float* bias,
                       const float* gamma, const float* beta, float* out) {
    RowSrc s;
    s.res = res; s.part = part; s.nparts = nparts; s.bias = bias; s.gamma = gamma; s.beta = beta; s.out = out;
    s.eps = c->ln_eps;
    return s;
}


// ---------------------------------------------------------------------------------------------------------
// How many rows a workgroup takes.  The decode step is bound by what every CU pulls through its L1 (a head's q|k|v +
// out_proj slices are 144 KB, a 64-unit FFN chunk 154 KB, a (row, head) of cross K/V 55 KB at S = 216): rows that share
// a workgroup share that stream, and the grid should not exceed one workgroup per CU.  ICK_DEC_G="self,cross,ffn"
// overrides the choice (tuning).
// ---------------------------------------------------------------------------------------------------------
struct GroupPlan {
    int g_self, g_cross, g_ffn;
    bool cross_shared;
    bool fsel;          // rows_per_sample == 1: a context with sel_state runs dec_self_kernel<g_self, true> at step >= 1
    bool head_merged;   // one dec_headvocab_kernel launch instead of dec_head_kernel + dec_vocab_kernel
    bool gather_loop;   // some LN-on-load source (RowGather) has more rows than one sweep of its kernel holds
};
static int pick_group(int units_per_row_group, int R, const int* cand, int ncand) {
    int g = cand[ncand - 1];
    for (int i = 0; i < ncand; ++i)
        if (units_per_row_group * ceil_div(R, cand[i]) <= kNumCU) { g = cand[i]; break; }
    return g;
}
// source rows one sweep of RowGather<G, kNW> holds (more take the loop in slice_sums)
template <int G> constexpr int sweep_rows() { return RowGather<G, kNW>::WPR * RowGather<G, kNW>::NS; }
static int sweep_rows_of(int g) {
    switch (g) {
    case 1: return sweep_rows<1>();
    case 2: return sweep_rows<2>();
    case 3: return sweep_rows<3>();
    case 4: return sweep_rows<4>();
    case 5: return sweep_rows<5>();
    default: return sweep_rows<8>();
    }
}
// the launches of a step are a function of these five sizes only: ick_decode_plan reports this to the tests
static GroupPlan plan_groups(int R, int rps, int H, int FF) {
    static const int pow2[] = {1, 2, 4, 8};
    GroupPlan p;
    const int nch = ceil_div(FF, 64);
    p.g_self = pick_group(H, R, pow2, 4);
    p.g_ffn = pick_group(nch, R, pow2, 4);
    p.cross_shared = false;
    p.g_cross = pick_group(H, R, pow2, 4);
    if (rps > 1) {
        // hypotheses of one caption read the same K / V: the largest group that divides the beam
        static const int shared[] = {8, 5, 4, 3, 2};
        p.g_cross = 1;
        for (int g : shared)
            if (rps % g == 0) { p.g_cross = g; p.cross_shared = true; break; }
    }
    p.fsel = rps == 1;
    // one launch for both when the rows fit one 32-row block and the final LayerNorm's sources fit the merged kernel's
    // registers (greedy decoding at cfg5)
    p.head_merged = R <= 32 && nch + 2 <= kHvSrc;
    // sources: self (layers >= 1) and the head sum the FFN chunks, cross and FFN the heads
    p.gather_loop = nch + 2 > sweep_rows_of(p.g_self) || H + 2 > sweep_rows_of(p.g_cross) ||
                    H + 2 > sweep_rows_of(p.g_ffn) || nch + 2 > RowGather<1, 4>::WPR * RowGather<1, 4>::NS;
    return p;
}
static void launch_self(int g, bool fsel, dim3 grid, hipStream_t s, const SelfArgs& a) {
    if (fsel) {
        switch (g) {
        case 1: hipLaunchKernelGGL((dec_self_kernel<1, true>), grid, dim3(kNT), 0, s, a); break;
        case 2: hipLaunchKernelGGL((dec_self_kernel<2, true>), grid, dim3(kNT), 0, s, a); break;
        case 4: hipLaunchKernelGGL((dec_self_kernel<4, true>), grid, dim3(kNT), 0, s, a); break;
        default: hipLaunchKernelGGL((dec_self_kernel<8, true>), grid, dim3(kNT), 0, s, a); break;
        }
        return;
    }
    switch (g) {
    case 1: hipLaunchKernelGGL((dec_self_kernel<1, false>), grid, dim3(kNT), 0, s, a); break;
    case 2: hipLaunchKernelGGL((dec_self_kernel<2, false>), grid, dim3(kNT), 0, s, a); break;
    case 4: hipLaunchKernelGGL((dec_self_kernel<4, false>), grid, dim3(kNT), 0, s, a); break;
    default: hipLaunchKernelGGL((dec_self_kernel<8, false>), grid, dim3(kNT), 0, s, a); break;
    }
}
static void launch_ffn(int g, dim3 grid, hipStream_t s, const FfnArgs& a) {
    switch (g) {
    case 1: hipLaunchKernelGGL(dec_ffn_kernel<1>, grid, dim3(kNT), 0, s, a); break;
    case 2: hipLaunchKernelGGL(dec_ffn_kernel<2>, grid, dim3(kNT), 0, s, a); break;
    case 4: hipLaunchKernelGGL(dec_ffn_kernel<4>, grid, dim3(kNT), 0, s, a); break;
    default: hipLaunchKernelGGL(dec_ffn_kernel<8>, grid, dim3(kNT), 0, s, a); break;
    }
}
template <bool ATTN, typename Args>
static void launch_cross_t(int g, bool shared, dim3 grid, hipStream_t s, const Args& a) {
    if (!shared) {
        switch (g) {
        case 1: hipLaunchKernelGGL((dec_cross_kernel<1, false, ATTN>), grid, dim3(kNT), 0, s, a); break;
        case 2: hipLaunchKernelGGL((dec_cross_kernel<2, false, ATTN>), grid, dim3(kNT), 0, s, a); break;
        case 4: hipLaunchKernelGGL((dec_cross_kernel<4, false, ATTN>), grid, dim3(kNT), 0, s, a); break;
        default: hipLaunchKernelGGL((dec_cross_kernel<8, false, ATTN>), grid, dim3(kNT), 0, s, a); break;
        }
        return;
    }
    switch (g) {
    case 2: hipLaunchKernelGGL((dec_cross_kernel<2, true, ATTN>), grid, dim3(kNT), 0, s, a); break;
    case 3: hipLaunchKernelGGL((dec_cross_kernel<3, true, ATTN>), grid, dim3(kNT), 0, s, a); break;
    case 4: hipLaunchKernelGGL((dec_cross_kernel<4, true, ATTN>), grid, dim3(kNT), 0, s, a); break;
    case 5: hipLaunchKernelGGL((dec_cross_kernel<5, true, ATTN>), grid, dim3(kNT), 0, s, a); break;
    default: hipLaunchKernelGGL((dec_cross_kernel<8, true, ATTN>), grid, dim3(kNT), 0, s, a); break;
    }
}
static void launch_cross(int g, bool shared, dim3 grid, hipStream_t s, const CrossAttnArgs& a) {
    if (a.attn == nullptr) launch_cross_t<false>(g, shared, grid, s, static_cast<const CrossArgs&>(a));
    else launch_cross_t<true>(g, shared, grid, s, a);
}

extern "C" int ick_decode_supported(int32_t d, int32_t H, int32_t FF, int32_t S, int32_t max_len) {
    return d > 0 && d % 4 == 0 && d <= kDMax && d >= 64 && H > 0 && H <= kPartsMax && d % H == 0 && d / H <= 32 && FF > 0 &&
           FF % 4 == 0 && FF <= 64 * kPartsMax &&
           S > 0 && S <= kSMax && max_len > 0 && max_len <= kMLMax;
}

extern "C" int ick_decode_plan(int32_t R, int32_t rows_per_sample, int32_t d, int32_t H, int32_t FF, int32_t* out) {
    ICK_CHECK_ARG(out && R > 0 && R <= 65535 && rows_per_sample > 0 && R % rows_per_sample == 0);
    ICK_CHECK_ARG(d > 0 && d % 4 == 0 && d <= kDMax && H > 0 && H <= kPartsMax && d % H == 0 && FF > 0 &&
                  FF % 4 == 0 && FF <= 64 * kPartsMax);
    const GroupPlan p = plan_groups(R, rows_per_sample, H, FF);
    out[0] = p.g_self; out[1] = p.fsel; out[2] = p.g_cross; out[3] = p.cross_shared; out[4] = p.g_ffn;
    out[5] = p.head_merged; out[6] = p.gather_loop;
    return 0;
}

// which: bit 0 self, 1 cross, 2 ffn, 3 head, 4 vocabulary (all set in the product path; the diagnostic build times subsets)
// attn: optional (max_len, R, layers, H, S) cross-attention weights (ick_decode_layers_attn)
static int decode_layers_impl(const ick_decode_ctx* c, int32_t pos, void* stream, unsigned which, int part = 0,
                              float* attn = nullptr) {
    ICK_CHECK_ARG(c && c->R > 0 && c->layers > 0 && c->layers <= ICK_MAX_LAYERS && pos >= 0 && pos < c->max_len);
    ICK_CHECK_ARG(ick_decode_supported(c->d, c->H, c->FF, c->S, c->max_len));
    ICK_CHECK_ARG(c->rows_per_sample > 0 && c->R % c->rows_per_sample == 0 && c->R <= 65535);
    ICK_CHECK_ARG(c->x0 && c->xa && c->xb && c->xc && c->p1 && c->p2 && c->p3 && c->hfin && c->hv && c->ptr && c->cand);
    ICK_CHECK_ARG(c->H <= kPartsMax && ceil_div(c->FF, 64) <= kPartsMax);
    hipStream_t s = (hipStream_t)stream;
    const int d = c->d, H = c->H, dh = d / H, R = c->R;
    const int nch = ceil_div(c->FF, 64);
    const float scale = 1.f / sqrtf((float)dh);
    const GroupPlan plan = plan_groups(R, c->rows_per_sample, H, c->FF);
    RowSrc src = make_src(c, c->x0, nullptr, 0, nullptr, nullptr, nullptr, c->xa);
    for (int l = 0; l < c->layers; ++l) {
        const ick_decode_layer& w = c->layer[l];
        ICK_CHECK_ARG(w.sa_in_w && w.sa_in_b && w.sa_out_wt && w.sa_out_b && w.ca_in_w && w.ca_in_b && w.ca_out_wt &&
                      w.ca_out_b && w.w1 && w.b1 && w.w2t && w.b2 && w.n1_g && w.n1_b && w.n2_g && w.n2_b && w.n3_g &&
                      w.n3_b && w.self_k && w.self_v && w.cross_k && w.cross_v);
        SelfArgs sa;
        sa.w.in_w = w.sa_in_w; sa.w.in_b = w.sa_in_b; sa.w.out_wt = w.sa_out_wt; sa.w.src = src; sa.w.part = c->p1;
        sa.kc = w.self_k; sa.vc = w.self_v; sa.anc = c->anc;
        sa.R = R; sa.d = d; sa.H = H; sa.dh = dh; sa.ML = c->max_len; sa.pos = pos; sa.scale = scale;
        sa.n_done = c->n_done; sa.n_total = R;
        const bool fsel = l == 0 && pos >= 1 && c->sel_state != nullptr;
        if (fsel) {
            // the token of step pos - 1 is chosen inside this launch (fused_select)
            ICK_CHECK_ARG(c->rows_per_sample == 1 && c->output && c->hist && c->finished && c->n_done && c->next_token &&
                          c->next_mask && c->word_emb && c->pe && c->cand && c->ptr && c->ee);
            const int i = pos - 1;
            fill_greedy_sel(sa.sel, c, i);
            sa.sel.st_in = c->sel_state + (size_t)(i & 1) * R * 12;
            sa.sel.st_out = c->sel_state + (size_t)((i + 1) & 1) * R * 12;
        }
        const bool first_self = l == 0;
        if ((which & 1u) && !(part == 2 && first_self))
            launch_self(plan.g_self, fsel, dim3(H, ceil_div(R, plan.g_self)), s, sa);
        if (part == 1) { ICK_LAUNCH_RET(); }
        CrossAttnArgs ca;
        ca.w.in_w = w.ca_in_w; ca.w.in_b = w.ca_in_b; ca.w.out_wt = w.ca_out_wt;
        ca.w.src = make_src(c, c->xa, c->p1, H, w.sa_out_b, w.n1_g, w.n1_b, c->xb);
        ca.w.part = c->p2;
        ca.Kmem = w.cross_k; ca.Vmem = w.cross_v; ca.kv_bs = c->kv_bs;
        ca.R = R; ca.rows_per_sample = c->rows_per_sample; ca.d = d; ca.H = H; ca.dh = dh; ca.S = c->S; ca.scale = scale;
        ca.n_done = c->n_done; ca.n_total = R;
        ca.attn = attn == nullptr ? nullptr : attn + ((int64_t)pos * R * c->layers + l) * H * c->S;
        ca.attn_rs = (int64_t)c->layers * H * c->S;
        if (which & 2u) launch_cross(plan.g_cross, plan.cross_shared, dim3(H, ceil_div(R, plan.g_cross)), s, ca);
        FfnArgs fa;
        fa.w1 = w.w1; fa.b1 = w.b1; fa.w2t = w.w2t;
        fa.src = make_src(c, c->xb, c->p2, H, w.ca_out_b, w.n2_g, w.n2_b, c->xc);
        fa.part = c->p3; fa.R = R; fa.d = d; fa.FF = c->FF; fa.n_done = c->n_done; fa.n_total = R;
        if (which & 4u) launch_ffn(plan.g_ffn, dim3(nch, ceil_div(R, plan.g_ffn)), s, fa);
        // the next consumer normalises: LayerNorm3(xc + b2 + sum of the chunk partials)
        src = make_src(c, c->xc, c->p3, nch, w.b2, w.n3_g, w.n3_b, l + 1 < c->layers ? c->xa : c->hfin);
    }
    ICK_CHECK_ARG(c->wv && c->bv && c->ee && c->we && c->be && c->V > 0 && c->K > 0);
    ICK_CHECK_ARG(c->F == 0 || (c->fe && c->wf && c->bf));
    HeadArgs ha;
    ha.src = src; ha.gate = c->gate; ha.hv = c->hv; ha.ee = c->ee; ha.we = c->we; ha.be = c->be;
    ha.fe = c->F > 0 ? c->fe : nullptr; ha.wf = c->wf; ha.bf = c->bf; ha.eib = c->eib; ha.ptr = c->ptr;
    ha.R = R; ha.rows_per_sample = c->rows_per_sample; ha.d = d; ha.K = c->K; ha.F = c->F;
    ha.n_done = c->n_done; ha.n_total = R;
    VocabArgs va;
    va.hv = c->hv; va.wv = c->wv; va.bv = c->bv; va.scores = c->scores; va.ld = c->scores_ld;
    va.cand = reinterpret_cast<float4*>(c->cand); va.R = R; va.d = d; va.V = c->V; va.ntiles = ceil_div(c->V, kVocabTile);
    va.n_done = c->n_done; va.n_total = R;
    if ((which & 24u) == 24u && plan.head_merged) {
        hipLaunchKernelGGL(dec_headvocab_kernel, dim3(va.ntiles + R), dim3(kNT), 0, s, ha, va);
        ICK_LAUNCH_RET();
    }
    if (which & 8u) hipLaunchKernelGGL(dec_head_kernel, dim3(R), dim3(256), 0, s, ha);
    if (which & 16u) hipLaunchKernelGGL(dec_vocab_kernel, dim3(va.ntiles), dim3(kNT), 0, s, va);
    ICK_LAUNCH_RET();
}

extern "C" int ick_decode_layers(const ick_decode_ctx* c, int32_t pos, void* stream) {
    return decode_layers_impl(c, pos, stream, 31u);
}

extern "C" int ick_decode_layers_part(const ick_decode_ctx* c, int32_t pos, int32_t part, void* stream) {
    ICK_CHECK_ARG(part >= 0 && part <= 2);
    return decode_layers_impl(c, pos, stream, 31u, part);
}

extern "C" int ick_decode_layers_attn(const ick_decode_ctx* c, float* attn, int32_t pos, int32_t part, void* stream) {
    ICK_CHECK_ARG(part >= 0 && part <= 2);
    return decode_layers_impl(c, pos, stream, 31u, part, attn);
}

// every per-call buffer of a greedy decode in one launch (they were eight fills, an embedding and a copy)
namespace ick { namespace {
__global__ __launch_bounds__(256) void dec_init_kernel(ick_decode_ctx c, int start_token, int n_done_init) {
    const int64_t r = blockIdx.x;
    const int tid = threadIdx.x;
    for (int p = tid; p < c.max_len; p += 256) {
        c.output[r * c.max_len + p] = c.pad_token;
        c.hist[r * c.max_len + p] = 0;
        if (c.cap_buf) c.cap_buf[r * c.max_len + p] = start_token;
    }
    if (tid == 0) {
        c.finished[r] = 0; c.next_token[r] = 0; c.next_mask[r] = 0;
        if (r == 0) *c.n_done = n_done_init;
    }
    if (c.sel_state && tid < 24) c.sel_state[(tid / 12) * (int64_t)c.R * 12 + r * 12 + tid % 12] = 0;
    // embedding of <start> at position 0 (CaptionEmbedder + sqrt(d) + PositionEncoder)
    const float* src = c.word_emb + (int64_t)start_token * c.d;
    for (int col = tid; col < c.d; col += 256) c.x0[r * c.d + col] = fmaf(src[col], c.emb_scale, c.pe[col]);
}
} }

extern "C" int ick_decode_init(const ick_decode_ctx* c, int32_t start_token, int32_t n_done_init, void* stream) {
    ICK_CHECK_ARG(c && c->R > 0 && c->max_len > 0 && c->d > 0 && c->output && c->hist && c->finished && c->n_done &&
                  c->next_token && c->next_mask && c->word_emb && c->pe && c->x0);
    ICK_CHECK_ARG(start_token >= 0 && start_token < c->V);
    hipLaunchKernelGGL(dec_init_kernel, dim3(c->R), dim3(256), 0, (hipStream_t)stream, *c, start_token, n_done_init);
    ICK_LAUNCH_RET();
}

#ifdef ICK_DECODE_STAMPS
// diagnostic build only: `reps` passes over a subset of the step's kernels (tools/debug/decode_repeat.py)
extern "C" int ick_debug_decode_subset(const ick_decode_ctx* c, int32_t pos, unsigned which, int32_t reps, void* stream) {
    for (int i = 0; i < reps; ++i) {
        const int rc = decode_layers_impl(c, pos, stream, which);
        if (rc != 0) return rc;
    }
    return 0;
}
#endif
