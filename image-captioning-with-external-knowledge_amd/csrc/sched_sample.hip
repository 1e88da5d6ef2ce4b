// Scheduled sampling of the fused training step (ick_sched_sample_mix): after a teacher-forced first
// pass, the token fed at position (b, q) is replaced with the model's own prediction for that position with
// probability p (Bengio et al. 2015; the two-pass form of Mihaylova & Martins 2019 / Duckworth et al. 2019).
//
// With n_b = clamp(decode_len[b], 0, L - 1), position (b, q) is ELIGIBLE when 1 <= q <= n_b - 1: its token is fed and
// packed score row rowstart[b] + q - 1 predicts it.  Every other position copies gold with replaced = 0.
//   coin:  x = element 0 of Philox-4x32-10 of counter (0xFFFFFFFF, step, q - 1, b) under key (seed lo, seed hi);
//          replaced iff (x >> 8) + 0.5 < prob * 2^24, compared in double (exact: prob = 1 replaces every eligible
//          position, prob = 0 none).  The quad 0xFFFFFFFF is never a column quad: Vx <= 2^24.
//   draw:  argmax mode: the lowest column that holds the row's maximum; else the first maximum of s[c] / T + g_c in
//          fp32, g_c = gumbel() (philox.h, the noise of sample.hip) of element c & 3 of Philox of counter
//          (c >> 2, step, q - 1, b).  Columns start_token and pad_token never win; <end> may.
//   token: column c < V gives (c, 0), V <= c < V + K gives (c, 1), c >= V + K gives (c, 2): token_kind(), the rule of
//          ick_samples_to_captions.
// A position that is not eligible or whose coin fails never reads its score row.  One workgroup of 1024 threads per
// position (as dec_sample_kernel: in sample mode a row costs a Philox block and eight logf per column quad, and the
// launch lasts as long as its slowest workgroup -- with 256 threads cfg4's 50 071 columns took 117 us against the 27 us
// in which ick_row_logprob_rank reads the same rows).  Every thread owns the same columns on every launch (thread t:
// quads t, t + 1024, ...), so its running best meets the columns in ascending order, the wave merge is a fixed
// butterfly and the sixteen waves merge in wave order: the same seed and counter give the same bits on every run (no
// atomics).  A row without a finite allowed score (never, for the head's scores) keeps gold.
#include "common.h"
#include "philox.h"

#include <climits>

namespace ick {
namespace {

constexpr int kMT = 1024;                  // threads per workgroup (one position)
constexpr int kMW = kMT / kWave;

struct MixArgs {
    const float* scores; int64_t ld;        // packed rows (M', ld)
    const int32_t *rowstart, *decode_len;   // ick_head_rowmap's
    const int64_t *caps, *masks;            // gold (B, L)
    const float *prob, *temperature;        // device words
    const int64_t* seed;
    const uint32_t* step;
    int64_t *caps_in, *masks_in;            // (B, L)
    int32_t* replaced;                      // (B, L)
    int B, L, V, K, F, start_token, pad_token;
};

struct Best {
    float v;
    int c;
};
__device__ __forceinline__ void best_push(Best& a, float v, int c) {      // columns arrive ascending: > keeps the lowest
    if (v > a.v) { a.v = v; a.c = c; }
}

template <bool ARGMAX>
__global__ __launch_bounds__(kMT) void sched_sample_mix_kernel(MixArgs a) {
    __shared__ float bv_sh[kMW];
    __shared__ int bc_sh[kMW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t pos = blockIdx.x;                     // b * L + q
    const int b = (int)(pos / a.L), q = (int)(pos - (int64_t)b * a.L);
    const int nb = min(max(a.decode_len[b], 0), a.L - 1);
    const int64_t seed = *a.seed;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)((uint64_t)seed >> 32), step = *a.step;
    const int Vx = a.V + a.K + a.F;
    const int64_t row = (int64_t)a.rowstart[b] + q - 1;
    // (the row bounds never bind for a row list of ick_head_rowmap: they keep any other list inside the packed rows)
    bool take = q >= 1 && q <= nb - 1 && row >= 0 && row < a.rowstart[b + 1] && row < (int64_t)a.B * a.L;
    if (take) {
        const uint32_t x = philox4x32_10(make_uint4(0xFFFFFFFFu, step, (uint32_t)(q - 1), (uint32_t)b), k0, k1).x;
        take = (double)(x >> 8) + 0.5 < (double)*a.prob * 16777216.0;
    }
    if (!take) {                                        // uniform: the whole workgroup leaves, the row is not read
        if (tid == 0) { a.caps_in[pos] = a.caps[pos]; a.masks_in[pos] = a.masks[pos]; a.replaced[pos] = 0; }
        return;
    }
    const float T = ARGMAX ? 1.f : *a.temperature;
    const float* r = a.scores + row * a.ld;
    const bool vec = (a.ld & 3) == 0 && (reinterpret_cast<uintptr_t>(a.scores) & 15) == 0;
    const float4* r4 = reinterpret_cast<const float4*>(r);
    const int nq = (Vx + 3) >> 2, nfull = Vx >> 2;      // quads of the row; the first nfull hold four columns
    Best best{-INFINITY, INT_MAX};
    for (int i0 = 0; i0 < nq; i0 += kMT * 4) {
        float4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + tid + kMT * j, c = 4 * i;
            if (i < nfull && vec) {
                x[j] = r4[i];                           // 16-byte loads of the aligned bulk
            } else {
                x[j].x = c < Vx ? r[c] : -INFINITY;     // the last, partial quad and rows that are not 16-byte aligned
                x[j].y = c + 1 < Vx ? r[c + 1] : -INFINITY;
                x[j].z = c + 2 < Vx ? r[c + 2] : -INFINITY;
                x[j].w = c + 3 < Vx ? r[c + 3] : -INFINITY;
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + tid + kMT * j, c = 4 * i;
            if (i >= nq) continue;
            const float s[4] = {x[j].x, x[j].y, x[j].z, x[j].w};
            uint32_t n[4] = {0u, 0u, 0u, 0u};
            if (!ARGMAX) {
                const uint4 p = philox4x32_10(make_uint4((uint32_t)i, step, (uint32_t)(q - 1), (uint32_t)b), k0, k1);
                n[0] = p.x; n[1] = p.y; n[2] = p.z; n[3] = p.w;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int col = c + e;
                if (col >= Vx || col == a.start_token || col == a.pad_token) continue;
                best_push(best, ARGMAX ? s[e] : s[e] / T + gumbel(n[e]), col);
            }
        }
    }
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = __shfl_xor(best.v, off, 64);
        const int oc = __shfl_xor(best.c, off, 64);
        if (ov > best.v || (ov == best.v && oc < best.c)) { best.v = ov; best.c = oc; }
    }
    if (lane == 0) { bv_sh[wave] = best.v; bc_sh[wave] = best.c; }
    __syncthreads();
    if (tid == 0) {
        best.v = bv_sh[0]; best.c = bc_sh[0];
#pragma unroll
        for (int w = 1; w < kMW; ++w)
            if (bv_sh[w] > best.v || (bv_sh[w] == best.v && bc_sh[w] < best.c)) { best.v = bv_sh[w]; best.c = bc_sh[w]; }
        const bool won = best.c != INT_MAX;
        a.caps_in[pos] = won ? (int64_t)best.c : a.caps[pos];
        a.masks_in[pos] = won ? (int64_t)token_kind(best.c, a.V, a.K, a.F > 0) : a.masks[pos];
        a.replaced[pos] = won ? 1 : 0;
    }
}

}  // namespace
}  // namespace ick

using namespace ick;

extern "C" int ick_sched_sample_mix(const float* scores, int64_t ld, const int32_t* rowstart, const int32_t* decode_len,
                                    const int64_t* captions, const int64_t* caption_masks, int32_t B, int32_t L,
                                    int32_t V, int32_t K, int32_t F, int32_t start_token, int32_t pad_token,
                                    const float* prob, const float* temperature, const int64_t* seed,
                                    const uint32_t* step, int32_t argmax, int64_t* captions_in, int64_t* masks_in,
                                    int32_t* replaced, void* stream) {
    ICK_CHECK_ARG(scores && rowstart && decode_len && captions && caption_masks && captions_in && masks_in && replaced);
    ICK_CHECK_ARG(prob && temperature && seed && step);
    ICK_CHECK_ARG(B > 0 && L >= 2 && V > 0 && K >= 0 && F >= 0 && (int64_t)B * L <= INT32_MAX);
    ICK_CHECK_ARG((int64_t)V + K + F <= (1 << 24) && ld >= (int64_t)V + K + F);
    MixArgs a;
    a.scores = scores; a.ld = ld; a.rowstart = rowstart; a.decode_len = decode_len; a.caps = captions;
    a.masks = caption_masks; a.prob = prob; a.temperature = temperature; a.seed = seed; a.step = step;
    a.caps_in = captions_in; a.masks_in = masks_in; a.replaced = replaced;
    a.B = B; a.L = L; a.V = V; a.K = K; a.F = F; a.start_token = start_token; a.pad_token = pad_token;
    void (*kern)(MixArgs) = argmax ? sched_sample_mix_kernel<true> : sched_sample_mix_kernel<false>;
    hipLaunchKernelGGL(kern, dim3((uint32_t)(B * L)), dim3(kMT), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}
