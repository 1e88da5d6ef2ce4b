// Score head pieces around the vocabulary GEMM: pointer scores over the entity / fact context,
// greedy selection and token bookkeeping of predict(), and the packed cross-entropy of train.py.
//   get_scores    geo-aware/models.py:291-313, knowledge-aware/models.py:420-455
//   predict loop  geo-aware/models.py:410-442, knowledge-aware/models.py:573-608
//   loss          geo-aware/train.py:275-281 (pack_padded_sequence + CrossEntropyLoss(ignore_index=<pad>))
// The vocabulary logits themselves are ick_gemm writing straight into the concatenated
// (B, L, V+K+F) rows; the pointer kernel fills columns [V, V+K) and [V+K, V+K+F) of the same
// rows, so the reference's (L,B,K,d) broadcast products and the torch.cat never exist.
#include "decode_select.h"

namespace ick {
namespace {

constexpr int kMaxPerLane = 16;

// one workgroup per (b, t) row of h; each wave walks context rows k = wave, wave+4, ... in batches of KB rows
// whose loads are all issued before the first reduction (one memory round trip per batch, not per row)
// rowmap / count (ick_pointer_scores_packed): workgroup m of the (T, B) grid takes the logical row rowmap[m] of h / ind and
// writes PACKED row m of out; workgroups m >= *count exit at once.
template <int NJ>
__global__ __launch_bounds__(256) void pointer_scores_kernel(const float* __restrict__ h, const float* __restrict__ ctx,
                                                             const float* __restrict__ w, const float* __restrict__ bias,
                                                             const float* __restrict__ ind, float* __restrict__ out,
                                                             int T, int Kc, int d, int64_t out_ld, int col0,
                                                             const int32_t* __restrict__ out_gmap,
                                                             const int32_t* __restrict__ rowmap,
                                                             const int32_t* __restrict__ count) {
    chain_priority();
    constexpr int KB = 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int b = blockIdx.y, t = blockIdx.x;
    int64_t orow_id = -1;
    if (rowmap != nullptr) {     // uniform
        const int m = b * T + t;
        if (m >= device_bound((int)gridDim.y * T, count)) return;
        const int lr = rowmap[m];
        b = lr / T;
        t = lr - b * T;
        orow_id = m;
    }
    const float* hr = h + ((int64_t)b * T + t) * d;
    float hv[NJ], wv[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        hv[j] = c < d ? hr[c] : 0.f;
        wv[j] = c < d ? w[c] : 0.f;
    }
    if (orow_id < 0) orow_id = (int64_t)(out_gmap ? out_gmap[b] : b) * T + t;
    float* orow = out + orow_id * out_ld + col0;
    const float bs = bias[0];
    for (int k0 = wave; k0 < Kc; k0 += 4 * KB) {
        float cv[KB][NJ];
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            const int k = k0 + 4 * q;
            const float* cr = ctx + ((int64_t)b * Kc + (k < Kc ? k : 0)) * d;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = lane + 64 * j;
                cv[q][j] = (k < Kc && c < d) ? cr[c] : 0.f;
            }
        }
#pragma unroll
        for (int q = 0; q < KB; ++q) {
            const int k = k0 + 4 * q;
            if (k >= Kc) break;      // wave-uniform
            float acc = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) acc = fmaf(__fmul_rn(hv[j], cv[q][j]), wv[j], acc);
            acc = wave_sum(acc);
            if (lane == 0) {
                const float f = ind ? ind[((int64_t)b * T + t) * Kc + k] : 1.f;
                orow[k] = acc * f + bs;
            }
        }
    }
}

// Top-2 of one score row by a 256-thread workgroup; the result is valid in thread 0 (sh[0]).  The row is read
// eight elements per thread at a time (loads first, comparisons after: one memory round trip per batch instead of
// one per element).
__device__ __forceinline__ Top2 row_top2(const float* __restrict__ r, int Vx, Top2* sh) {
    const int tid = threadIdx.x;
    Top2 s{-INFINITY, -INFINITY, 0x7fffffff, 0x7fffffff};
    for (int i0 = 0; i0 < Vx; i0 += 256 * 8) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + 256 * j;
            x[j] = i < Vx ? r[i] : -INFINITY;
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + 256 * j;
            if (i < Vx) top2_push(s, x[j], i);
        }
    }
    sh[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            Top2 a = sh[tid];
            const Top2 c = sh[tid + o];
            if (c.i1 != 0x7fffffff) top2_push(a, c.v1, c.i1);
            if (c.i2 != 0x7fffffff) top2_push(a, c.v2, c.i2);
            sh[tid] = a;
        }
        __syncthreads();
    }
    return sh[0];
}

__global__ __launch_bounds__(256) void top2_kernel(const float* __restrict__ scores, int64_t ld, int Vx,
                                                   int32_t* __restrict__ best, int32_t* __restrict__ second) {
    __shared__ Top2 sh[256];
    const int b = blockIdx.x;
    const Top2 t = row_top2(scores + (int64_t)b * ld, Vx, sh);
    if (threadIdx.x == 0) {
        best[b] = t.i1;
        second[b] = t.i2 == 0x7fffffff ? t.i1 : t.i2;
    }
}

// predict()'s per-step bookkeeping for caption b (geo-aware/models.py:410-441), given the step's two best tokens.
__device__ __forceinline__ void greedy_update_one(int b, int best_b, int second_b, int64_t* __restrict__ output,
                                                  int32_t* __restrict__ hist, int32_t* __restrict__ finished,
                                                  int64_t* __restrict__ next_token, int64_t* __restrict__ next_mask,
                                                  int step, int max_len, int V, int K, int has_facts, int end_token) {
    int64_t* o = output + (int64_t)b * max_len;
    int32_t* hs = hist + (int64_t)b * max_len;
    const int i = step, fin = finished[b];
    int po[5], ph[3];                       // output[i-1 .. i-5], runner-ups of steps i-1 .. i-3
#pragma unroll
    for (int q = 0; q < 5; ++q) po[q] = (int)o[max(i - 1 - q, 0)];
#pragma unroll
    for (int q = 0; q < 3; ++q) ph[q] = hs[max(i - 1 - q, 0)];
    const GreedyStep g = greedy_step(best_b, second_b, i, po, ph, fin, end_token, V, K, has_facts);
    if (!fin) {
        o[i] = g.cur;
        if (g.ended) {
            finished[b] = 1;
        } else {
            hs[i] = second_b;
            if (g.nrw >= 1) o[i - 1] = g.rw[0];
            if (g.nrw >= 3) { o[i - 2] = g.rw[1]; o[i - 3] = g.rw[2]; }
        }
    }
    if (g.ended || i < max_len - 1) {       // a live caption's last step has no next token: left as it is
        next_token[b] = g.tok;
        next_mask[b] = g.msk;
    }
}

// One lane per caption (separate selection and bookkeeping: ick_top2 + ick_greedy_update).
__global__ void greedy_update_kernel(const int32_t* __restrict__ best, const int32_t* __restrict__ second,
                                     int64_t* __restrict__ output, int32_t* __restrict__ hist,
                                     int32_t* __restrict__ finished, int64_t* __restrict__ next_token,
                                     int64_t* __restrict__ next_mask, int B, int step, int max_len, int V, int K,
                                     int has_facts, int end_token) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    greedy_update_one(b, best[b], second[b], output, hist, finished, next_token, next_mask, step, max_len, V, K,
                      has_facts, end_token);
}

// Selection and bookkeeping of a greedy step in one launch: workgroup b scans caption b's score row, its thread 0
// updates the caption's state (one launch less per token of the decode loop).
__global__ __launch_bounds__(256) void greedy_select_kernel(const float* __restrict__ scores, int64_t ld, int Vx,
                                                            int64_t* __restrict__ output, int32_t* __restrict__ hist,
                                                            int32_t* __restrict__ finished,
                                                            int64_t* __restrict__ next_token,
                                                            int64_t* __restrict__ next_mask, int step, int max_len,
                                                            int V, int K, int has_facts, int end_token) {
    __shared__ Top2 sh[256];
    const int b = blockIdx.x;
    const Top2 t = row_top2(scores + (int64_t)b * ld, Vx, sh);
    if (threadIdx.x == 0)
        greedy_update_one(b, t.i1, t.i2 == 0x7fffffff ? t.i1 : t.i2, output, hist, finished, next_token, next_mask, step,
                          max_len, V, K, has_facts, end_token);
}

// Packed cross entropy: one workgroup per (b, t) score row.  kWeighted (ick_packed_ce_weighted): the gradient of row
// (b, t) is scaled by weight[b]; row_loss keeps the UNWEIGHTED loss (>= 0, so the -1 marker still tells the rows apart)
// and the reduction applies the weight.  With kWeighted = false the weight is the constant 1 and folds away.
// kPacked (ick_packed_ce_packed): scores / row_loss / dscores hold the PACKED rows of the valid positions; workgroup m takes
// packed row m, which belongs to position rowmap[m] = b * L + t (valid by construction: t < min(length - 1, L - 1)); dl is
// the device row count, and workgroups at or past it exit without writing anything.
// kSmooth (ick_packed_ce_smooth): label smoothing with eps = eps_arg.word[0], a device word, uniform
// per launch -- row_loss = (1 - eps) * (lse - x[target]) + eps * (lse - mean(x)) and the gradient is
// w * (softmax - (1 - eps) * onehot - eps / Vx).  The row's sum is gathered in the pass that reads the row anyway.  The
// terms are written so that eps == 0 leaves the plain kernels' bits: the uniform term enters as + w * (0 - eps / Vx) (a
// zero of w's sign, which also keeps the sign of a gradient that underflowed to zero), the target's as - w * (1 - eps).
template <bool kSmooth>
struct CeEps { const float* word; };          // the device word holding eps
template <>
struct CeEps<false> {};                       // the plain kernels take no such argument
template <bool kWeighted, bool kPacked = false, bool kSmooth = false>
__global__ __launch_bounds__(256) void packed_ce_rows_kernel(const float* __restrict__ scores, int64_t ld,
                                                             const int64_t* __restrict__ caps,
                                                             const int32_t* __restrict__ dl, int L, int Vx, int pad,
                                                             float* __restrict__ row_loss, float* __restrict__ dscores,
                                                             const float* __restrict__ weight,
                                                             const int32_t* __restrict__ rowmap, CeEps<kSmooth> eps_arg) {
    __shared__ float red[4];
    int t = blockIdx.x, b = blockIdx.y;
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)b * L + t;
    if constexpr (kPacked) {
        if (row >= device_bound((int)gridDim.y * L, dl)) return;      // uniform
        const int lr = rowmap[row];
        b = lr / L;
        t = lr - b * L;
    }
    const float* r = scores + row * ld;
    float* dr = dscores ? dscores + row * ld : nullptr;
    int64_t target = -1;
    bool use = t < L - 1 && (kPacked || t < dl[b]);
    if (use) {
        target = caps[(int64_t)b * L + t + 1];
        use = target != pad && target >= 0 && target < Vx;
    }
    if (!use) {
        if (tid == 0) row_loss[row] = -1.f;  // marker: row does not contribute
        if (dr) {
            // (16-byte stores where the row allows: up to half of a batch's rows lie beyond their caption's length, and at
            // the knowledge vocabulary each is 200 KB of zeros)
            const int z4 = ((ld & 3) == 0 && (reinterpret_cast<uintptr_t>(dscores) & 15) == 0) ? (int)(Vx >> 2) : 0;
            float4* d4 = reinterpret_cast<float4*>(dr);
            for (int i = tid; i < z4; i += 256) d4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = 4 * z4 + tid; i < Vx; i += 256) dr[i] = 0.f;
        }
        return;
    }
    float eps = 0.f, keep = 1.f, nsub = 0.f, rs = 0.f;      // kSmooth: eps, 1 - eps, 0 - eps / Vx, the row's sum
    if constexpr (kSmooth) {
        eps = eps_arg.word[0];                              // uniform
        keep = 1.f - eps;
        nsub = 0.f - eps / (float)Vx;
    }
    // Rows of up to 256 * 4 * kCeVec floats (16-byte aligned) stay in registers between the passes: one read
    // of the logits and one write of the gradient instead of three reads; longer / unaligned rows re-read.
    constexpr int kCeVec = 10;
    const bool in_regs = (Vx & 3) == 0 && (ld & 3) == 0 && Vx <= 256 * 4 * kCeVec &&
                         (reinterpret_cast<uintptr_t>(scores) & 15) == 0 &&
                         (dr == nullptr || (reinterpret_cast<uintptr_t>(dscores) & 15) == 0);
    if (in_regs) {
        const float4* r4 = reinterpret_cast<const float4*>(r);
        const int n4 = Vx >> 2;
        float4 x[kCeVec];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kCeVec; ++j) {
            const int i = tid + 256 * j;
            x[j] = i < n4 ? r4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            m = fmaxf(m, fmaxf(fmaxf(x[j].x, x[j].y), fmaxf(x[j].z, x[j].w)));
            if constexpr (kSmooth) {
                if (i < n4) rs += (x[j].x + x[j].y) + (x[j].z + x[j].w);
            }
        }
        m = block_max<4>(m, red);
        if constexpr (kSmooth) rs = block_sum<4>(rs, red);
        float s = 0.f;
#pragma unroll
        for (int j = 0; j < kCeVec; ++j) {
            x[j].x = __expf(x[j].x - m); x[j].y = __expf(x[j].y - m);
            x[j].z = __expf(x[j].z - m); x[j].w = __expf(x[j].w - m);
            s += (x[j].x + x[j].y) + (x[j].z + x[j].w);
        }
        s = block_sum<4>(s, red);
        if (tid == 0) {
            if constexpr (kSmooth) {
                const float lse = m + __logf(s);
                row_loss[row] = keep * (lse - r[target]) + eps * (lse - rs / (float)Vx);
            } else {
                row_loss[row] = m + __logf(s) - r[target];
            }
        }
        if (dr) {
            const float wr = kWeighted ? weight[b] : 1.f;
            const float inv = wr / s;
            const float wt = kSmooth ? wr * keep : wr, wu = wr * nsub;
            float4* d4 = reinterpret_cast<float4*>(dr);
            const int tq = (int)(target >> 2), tr = (int)(target & 3);
#pragma unroll
            for (int j = 0; j < kCeVec; ++j) {
                const int i = tid + 256 * j;
                if (i < n4) {
                    float4 g = make_float4(x[j].x * inv, x[j].y * inv, x[j].z * inv, x[j].w * inv);
                    if constexpr (kSmooth) { g.x += wu; g.y += wu; g.z += wu; g.w += wu; }
                    if (i == tq) {
                        if (tr == 0) g.x -= wt; else if (tr == 1) g.y -= wt; else if (tr == 2) g.z -= wt; else g.w -= wt;
                    }
                    d4[i] = g;
                }
            }
        }
        return;
    }
    // Long rows (knowledge vocabulary: 50 071 columns): max and sum of exponentials in ONE pass with a running pair
    // (m, s) per thread, rescaled when the maximum moves; the pairs are merged through the block maximum.  Two reads of
    // the row instead of three.  Rows that start 16-byte aligned (the training step pads the row stride to a multiple
    // of 4 floats) are read and written as float4 with a scalar tail: a dword per lane moves 256 B per wave instruction,
    // a dwordx4 1 KiB (round 5: cfg4's loss 161 -> ~115 us for 2 x 256 MB read + 256 MB written).
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0 &&
                     (dr == nullptr || (reinterpret_cast<uintptr_t>(dscores) & 15) == 0);
    const int n4 = vec ? (int)(Vx >> 2) : 0;             // float4 elements of the aligned bulk; [4 n4, Vx) is the scalar tail
    const float4* r4 = reinterpret_cast<const float4*>(r);
    float m = -INFINITY, s = 0.f;
    for (int i0 = 0; i0 < n4; i0 += 256 * 4) {
        float4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + tid + 256 * j;
            x[j] = i < n4 ? r4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
            if constexpr (kSmooth) {
                if (i < n4) rs += (x[j].x + x[j].y) + (x[j].z + x[j].w);
            }
        }
        float bm = m;
#pragma unroll
        for (int j = 0; j < 4; ++j) bm = fmaxf(bm, fmaxf(fmaxf(x[j].x, x[j].y), fmaxf(x[j].z, x[j].w)));
        if (bm > -INFINITY) {
            s *= __expf(m - bm);            // m = -inf: s is 0 and stays 0
#pragma unroll
            for (int j = 0; j < 4; ++j)     // exp(-inf) = 0 for the tail
                s += (__expf(x[j].x - bm) + __expf(x[j].y - bm)) + (__expf(x[j].z - bm) + __expf(x[j].w - bm));
            m = bm;
        }
    }
    for (int i0 = 4 * n4; i0 < Vx; i0 += 256 * 8) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + 256 * j;
            x[j] = i < Vx ? r[i] : -INFINITY;
            if constexpr (kSmooth) {
                if (i < Vx) rs += x[j];
            }
        }
        float bm = m;
#pragma unroll
        for (int j = 0; j < 8; ++j) bm = fmaxf(bm, x[j]);
        if (bm > -INFINITY) {
            s *= __expf(m - bm);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += __expf(x[j] - bm);
            m = bm;
        }
    }
    const float mt = m;
    m = block_max<4>(m, red);
    s = block_sum<4>(mt > -INFINITY ? s * __expf(mt - m) : 0.f, red);
    const float lse = m + __logf(s);
    if constexpr (kSmooth) {
        rs = block_sum<4>(rs, red);
        if (tid == 0) row_loss[row] = keep * (lse - r[target]) + eps * (lse - rs / (float)Vx);
    } else {
        if (tid == 0) row_loss[row] = lse - r[target];
    }
    if (dr) {
        const float wr = kWeighted ? weight[b] : 1.f;
        const float inv = wr / s;
        const float wt = kSmooth ? wr * keep : wr, wu = wr * nsub;
        float4* d4 = reinterpret_cast<float4*>(dr);
        const int tq = (int)(target >> 2), tr = (int)(target & 3);
        for (int i0 = 0; i0 < n4; i0 += 256 * 4) {
            float4 x[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + tid + 256 * j;
                x[j] = i < n4 ? r4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int i = i0 + tid + 256 * j;
                if (i < n4) {
                    float4 gq = make_float4(__expf(x[j].x - m) * inv, __expf(x[j].y - m) * inv, __expf(x[j].z - m) * inv,
                                            __expf(x[j].w - m) * inv);
                    if constexpr (kSmooth) { gq.x += wu; gq.y += wu; gq.z += wu; gq.w += wu; }
                    if (i == tq) {
                        if (tr == 0) gq.x -= wt; else if (tr == 1) gq.y -= wt; else if (tr == 2) gq.z -= wt; else gq.w -= wt;
                    }
                    d4[i] = gq;
                }
            }
        }
        for (int i0 = 4 * n4; i0 < Vx; i0 += 256 * 8) {
            float x[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + tid + 256 * j;
                x[j] = i < Vx ? r[i] : 0.f;
            }
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int i = i0 + tid + 256 * j;
                if (i < Vx) {
                    if constexpr (kSmooth) dr[i] = (__expf(x[j] - m) * inv + wu) - (i == target ? wt : 0.f);
                    else dr[i] = __expf(x[j] - m) * inv - (i == target ? wr : 0.f);
                }
            }
        }
    }
}

// Fixed-order reduction of the per-row losses (deterministic, unlike float atomics); kWeighted: row i belongs to caption
// i / L and its loss enters the sum times that caption's weight (the count stays the number of rows).
// rowmap / nrows (the packed form): the first *nrows of the n rows exist, row i belongs to caption rowmap[i] / L.
// mean (ick_packed_ce_*_mean; else nullptr): also mean[0] = loss_sum / count, 0 when no row counts.
template <bool kWeighted>
__global__ __launch_bounds__(256) void packed_ce_reduce_kernel(const float* __restrict__ row_loss, int n, int L,
                                                               const float* __restrict__ weight,
                                                               float* __restrict__ loss_sum, float* __restrict__ count,
                                                               const int32_t* __restrict__ rowmap,
                                                               const int32_t* __restrict__ nrows,
                                                               float* __restrict__ mean) {
    __shared__ float red[4];
    float s = 0.f, c = 0.f;
    n = device_bound(n, nrows);
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = row_loss[i];
        if (v > -0.5f) { s += kWeighted ? weight[(rowmap ? rowmap[i] : i) / L] * v : v; c += 1.f; }
    }
    s = block_sum<4>(s, red);
    c = block_sum<4>(c, red);
    if (threadIdx.x == 0) {
        loss_sum[0] = s;
        count[0] = c;
        if (mean) mean[0] = c > 0.f ? s / c : 0.f;
    }
}

// Caption scoring (ick_row_logprob_rank): what a scorer needs of one packed score row -- the target's
// log-probability, its rank in a stable descending sort and the row's argmax -- from ONE read of the row.
struct RowScan {
    float m, s;      // running maximum and sum of exp(x - m); m is also the value of the running argmax
    float cnt;       // columns that beat the target (a count below 2^24: exact in fp32 in any order)
    int bi;          // lowest column that holds m
};
__device__ __forceinline__ void row_scan_push(RowScan& a, float x, int c, float st, int target) {
    a.s += __expf(x - a.m);       // a.m >= x: the caller has moved the maximum over the whole batch first
    a.cnt += (x > st || (x == st && c < target)) ? 1.f : 0.f;
}
// (a thread meets its columns in ascending order, so `>` alone keeps the lowest column of a tie)
__device__ __forceinline__ void row_scan_best(float& bv, int& bi, float x, int c) {
    if (x > bv) { bv = x; bi = c; }
}

// One workgroup per packed row m < *count of the (L, R) grid; the row belongs to position rowmap[m] = b * L + t and its
// results go to the LOGICAL element (b, t) of the (R, L - 1) outputs.  Same validity rule as packed_ce_rows_kernel: a
// target that is <pad> or outside [0, Vx) gives 0 / -1 / -1.  Scores are taken to be finite (the head's are): -inf is
// the padding of the lanes past the row, and a batch that holds nothing else is skipped.
__global__ __launch_bounds__(256) void row_logprob_rank_kernel(const float* __restrict__ scores, int64_t ld,
                                                               const int64_t* __restrict__ caps,
                                                               const int32_t* __restrict__ rowmap,
                                                               const int32_t* __restrict__ count, int L, int Vx, int pad,
                                                               float* __restrict__ tlp, int32_t* __restrict__ rank,
                                                               int32_t* __restrict__ best) {
    __shared__ float4 red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = (int64_t)blockIdx.y * L + blockIdx.x;
    if (row >= device_bound((int)gridDim.y * L, count)) return;      // uniform
    const int lr = rowmap[row];
    const int b = lr / L, t = lr - b * L;
    if (b >= (int)gridDim.y || t >= L - 1) return;                   // (never, for a row list of ick_head_rowmap)
    const int64_t o = (int64_t)b * (L - 1) + t;
    const int64_t target64 = caps[(int64_t)b * L + t + 1];
    if (target64 == pad || target64 < 0 || target64 >= Vx) {         // uniform
        if (tid == 0) { tlp[o] = 0.f; rank[o] = -1; best[o] = -1; }
        return;
    }
    const int target = (int)target64;
    const float* r = scores + row * ld;
    const float st = r[target];
    const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(scores) & 15) == 0;
    const int n4 = vec ? (Vx >> 2) : 0;             // float4 elements of the aligned bulk; [4 n4, Vx) is the scalar tail
    const float4* r4 = reinterpret_cast<const float4*>(r);
    RowScan a{-INFINITY, 0.f, 0.f, 0x7fffffff};
    for (int i0 = 0; i0 < n4; i0 += 256 * 4) {
        float4 x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = i0 + tid + 256 * j;
            x[j] = i < n4 ? r4[i] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
        float bm = a.m;
        int bi = a.bi;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = 4 * (i0 + tid + 256 * j);
            row_scan_best(bm, bi, x[j].x, c); row_scan_best(bm, bi, x[j].y, c + 1);
            row_scan_best(bm, bi, x[j].z, c + 2); row_scan_best(bm, bi, x[j].w, c + 3);
        }
        if (bm > -INFINITY) {
            a.s *= __expf(a.m - bm);                // a.m = -inf: s is 0 and stays 0
            a.m = bm; a.bi = bi;
#pragma unroll
            for (int j = 0; j < 4; ++j) {           // (columns past the row hold -inf: exp gives 0, no comparison holds)
                const int c = 4 * (i0 + tid + 256 * j);
                row_scan_push(a, x[j].x, c, st, target); row_scan_push(a, x[j].y, c + 1, st, target);
                row_scan_push(a, x[j].z, c + 2, st, target); row_scan_push(a, x[j].w, c + 3, st, target);
            }
        }
    }
    for (int i0 = 4 * n4; i0 < Vx; i0 += 256 * 8) {
        float x[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int i = i0 + tid + 256 * j;
            x[j] = i < Vx ? r[i] : -INFINITY;
        }
        float bm = a.m;
        int bi = a.bi;
#pragma unroll
        for (int j = 0; j < 8; ++j) row_scan_best(bm, bi, x[j], i0 + tid + 256 * j);
        if (bm > -INFINITY) {
            a.s *= __expf(a.m - bm);
            a.m = bm; a.bi = bi;
#pragma unroll
            for (int j = 0; j < 8; ++j) row_scan_push(a, x[j], i0 + tid + 256 * j, st, target);
        }
    }
    // merge: within the wave by the DPP reductions, then the four waves' results by thread 0 in wave order.  Column
    // numbers are below 2^24 (checked by the entry point), so the lowest column of the maximum is a float maximum of -c.
    const float wm = wave_max(a.m);
    const float ws = wave_sum(a.m > -INFINITY ? a.s * __expf(a.m - wm) : 0.f);
    const float wc = wave_sum(a.cnt);
    const float wi = wave_max(a.m == wm && a.bi != 0x7fffffff ? -(float)a.bi : -INFINITY);
    if (lane == 0) red[wave] = make_float4(wm, ws, wc, wi);
    __syncthreads();
    if (tid == 0) {
        float m = red[0].x;
#pragma unroll
        for (int w = 1; w < 4; ++w) m = fmaxf(m, red[w].x);
        float s = 0.f, c = 0.f, bi = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            if (red[w].x > -INFINITY) s += red[w].y * __expf(red[w].x - m);
            c += red[w].z;
            if (red[w].x == m) bi = fmaxf(bi, red[w].w);
        }
        tlp[o] = st - (m + __logf(s));
        rank[o] = (int32_t)c;
        best[o] = (int32_t)(-bi);
    }
}

// One wave per caption r (ick_caption_score_sums): the caption's valid rows are positions t < n = rowstart[r + 1] -
// rowstart[r]; the positions from n on get their fill values here (so no memset precedes the row kernel), the token
// log-probabilities are summed in position order by lane 0.
__global__ __launch_bounds__(256) void caption_sums_kernel(const int32_t* __restrict__ rowstart, int R, int L,
                                                           float* __restrict__ tlp, int32_t* __restrict__ rank,
                                                           int32_t* __restrict__ best, float* __restrict__ log_prob,
                                                           int32_t* __restrict__ tokens) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= R) return;
    const int n = min(max(rowstart[r + 1] - rowstart[r], 0), L - 1);
    const int64_t o = (int64_t)r * (L - 1);
    for (int t = n + lane; t < L - 1; t += 64) { tlp[o + t] = 0.f; rank[o + t] = -1; best[o + t] = -1; }
    if (lane == 0) {
        float s = 0.f;
        int c = 0;
        for (int t = 0; t < n; ++t) {
            if (rank[o + t] >= 0) { s += tlp[o + t]; ++c; }
        }
        log_prob[r] = s;
        tokens[r] = c;
    }
}

// The four totals over all R * (L - 1) positions in a fixed order (one workgroup, no float atomics).
__global__ __launch_bounds__(256) void caption_totals_kernel(const float* __restrict__ tlp, const int32_t* __restrict__ rank,
                                                             int64_t n, int top_k, float* __restrict__ loss_sum,
                                                             float* __restrict__ count, float* __restrict__ top1,
                                                             float* __restrict__ topk) {
    __shared__ float red[4];
    float s = 0.f, c = 0.f, h1 = 0.f, hk = 0.f;
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int rk = rank[i];
        if (rk >= 0) {
            s -= tlp[i];
            c += 1.f;
            h1 += rk == 0 ? 1.f : 0.f;
            hk += rk < top_k ? 1.f : 0.f;
        }
    }
    s = block_sum<4>(s, red);
    c = block_sum<4>(c, red);
    h1 = block_sum<4>(h1, red);
    hk = block_sum<4>(hk, red);
    if (threadIdx.x == 0) { loss_sum[0] = s; count[0] = c; top1[0] = h1; topk[0] = hk; }
}

// The packed row list of the training step's score head (ick_head_rowmap): one workgroup scans the B lengths.
__global__ __launch_bounds__(256) void head_rowmap_kernel(const int64_t* __restrict__ lengths, int B, int L,
                                                          int32_t* __restrict__ decode_len, int32_t* __restrict__ rowstart,
                                                          int32_t* __restrict__ rowmap) {
    __shared__ int part[256];
    __shared__ int total;
    const int tid = threadIdx.x;
    const int per = (B + 255) / 256;             // consecutive samples per thread
    const int b0 = min(B, tid * per), b1 = min(B, b0 + per);
    auto valid = [&](int64_t len) { return (int)min((int64_t)(L - 1), max((int64_t)0, len - 1)); };
    int sum = 0;
    for (int b = b0; b < b1; ++b) {
        const int64_t len = lengths[b];
        decode_len[b] = (int32_t)(len - 1);
        sum += valid(len);
    }
    part[tid] = sum;
    __syncthreads();
    if (tid == 0) {                              // exclusive scan of the 256 partial sums
        int run = 0;
        for (int i = 0; i < 256; ++i) { const int v = part[i]; part[i] = run; run += v; }
        total = run;
        rowstart[B] = run;
    }
    __syncthreads();
    int run = part[tid];
    for (int b = b0; b < b1; ++b) {
        const int n = valid(lengths[b]);
        rowstart[b] = run;
        for (int t = 0; t < n; ++t) rowmap[run + t] = b * L + t;
        run += n;
    }
    for (int m = total + tid; m < B * L; m += 256) rowmap[m] = 0;      // never used: a defined value all the same
}

// dst[m, :] = src[rowmap[m], :], one wave per packed row m < *count
__global__ __launch_bounds__(256) void gather_rows_kernel(const float* __restrict__ src, int64_t src_rs,
                                                          const int32_t* __restrict__ rowmap,
                                                          const int32_t* __restrict__ count, float* __restrict__ dst,
                                                          int64_t dst_rs, int max_rows, int d) {
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (m >= device_bound(max_rows, count)) return;
    const float* s = src + (int64_t)rowmap[m] * src_rs;
    float* o = dst + (int64_t)m * dst_rs;
    for (int c = lane; c < d; c += 64) o[c] = s[c];
}

}  // namespace
}  // namespace ick

namespace ick {
namespace {
int launch_pointer_scores(const float* h, const float* ctx, const float* w, const float* bias, const float* ind, float* out,
                          int B, int T, int Kc, int d, int64_t out_ld, int col0, const int32_t* out_gmap,
                          const int32_t* rowmap, const int32_t* count, hipStream_t s) {
    if (d <= 320)
        hipLaunchKernelGGL(pointer_scores_kernel<5>, dim3(T, B), dim3(256), 0, s, h, ctx, w, bias, ind, out, T, Kc, d,
                           out_ld, col0, out_gmap, rowmap, count);
    else if (d <= 512)
        hipLaunchKernelGGL(pointer_scores_kernel<8>, dim3(T, B), dim3(256), 0, s, h, ctx, w, bias, ind, out, T, Kc, d,
                           out_ld, col0, out_gmap, rowmap, count);
    else
        hipLaunchKernelGGL(pointer_scores_kernel<kMaxPerLane>, dim3(T, B), dim3(256), 0, s, h, ctx, w, bias, ind, out, T,
                           Kc, d, out_ld, col0, out_gmap, rowmap, count);
    ICK_LAUNCH_RET();
}
}  // namespace
}  // namespace ick

extern "C" int ick_pointer_scores(const float* h, const float* ctx, const float* w, const float* bias,
                                  const float* ind, float* out, int32_t B, int32_t T, int32_t Kc, int32_t d,
                                  int64_t out_ld, int32_t col0, const int32_t* out_gmap, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(h && ctx && w && bias && out && B > 0 && T > 0 && Kc > 0 && d > 0 && d <= 64 * kMaxPerLane);
    ICK_CHECK_ARG(B <= 65535 && col0 >= 0 && out_ld >= col0 + Kc);
    return ick::launch_pointer_scores(h, ctx, w, bias, ind, out, B, T, Kc, d, out_ld, col0, out_gmap, nullptr, nullptr,
                                      (hipStream_t)stream);
}

extern "C" int ick_pointer_scores_packed(const float* h, const float* ctx, const float* w, const float* bias,
                                         const float* ind, float* out, int32_t B, int32_t T, int32_t Kc, int32_t d,
                                         int64_t out_ld, int32_t col0, const int32_t* rowmap, const int32_t* count,
                                         void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(h && ctx && w && bias && out && B > 0 && T > 0 && Kc > 0 && d > 0 && d <= 64 * kMaxPerLane);
    ICK_CHECK_ARG(B <= 65535 && col0 >= 0 && out_ld >= col0 + Kc && rowmap && count && (int64_t)B * T <= INT32_MAX);
    return launch_pointer_scores(h, ctx, w, bias, ind, out, B, T, Kc, d, out_ld, col0, nullptr, rowmap, count,
                                 (hipStream_t)stream);
}

extern "C" int ick_head_rowmap(const int64_t* lengths, int32_t B, int32_t L, int32_t* decode_len, int32_t* rowstart,
                               int32_t* rowmap, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(lengths && decode_len && rowstart && rowmap && B > 0 && L > 0 && (int64_t)B * L <= INT32_MAX);
    hipLaunchKernelGGL(head_rowmap_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, lengths, B, L, decode_len, rowstart,
                       rowmap);
    ICK_LAUNCH_RET();
}

extern "C" int ick_gather_rows(const float* src, int64_t src_rs, const int32_t* rowmap, const int32_t* count, float* dst,
                               int64_t dst_rs, int32_t max_rows, int32_t d, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(src && rowmap && count && dst && max_rows > 0 && d > 0 && src_rs >= d && dst_rs >= d);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(ceil_div(max_rows, 4)), dim3(256), 0, (hipStream_t)stream, src, src_rs,
                       rowmap, count, dst, dst_rs, max_rows, d);
    ICK_LAUNCH_RET();
}

extern "C" int ick_top2(const float* scores, int64_t ld, int32_t B, int32_t Vx, int32_t* best, int32_t* second,
                        void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && best && second && B > 0 && Vx > 0 && ld >= Vx);
    hipLaunchKernelGGL(top2_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scores, ld, Vx, best, second);
    ICK_LAUNCH_RET();
}

extern "C" int ick_greedy_update(const int32_t* best, const int32_t* second, int64_t* output, int32_t* top2_hist,
                                 int32_t* finished, int64_t* next_token, int64_t* next_mask, int32_t B, int32_t step,
                                 int32_t max_len, int32_t V, int32_t K, int32_t has_facts, int32_t end_token,
                                 void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(best && second && output && top2_hist && finished && next_token && next_mask);
    ICK_CHECK_ARG(B > 0 && step >= 0 && step < max_len);
    hipLaunchKernelGGL(greedy_update_kernel, dim3(ceil_div(B, 64)), dim3(64), 0, (hipStream_t)stream, best, second,
                       output, top2_hist, finished, next_token, next_mask, B, step, max_len, V, K, has_facts,
                       end_token);
    ICK_LAUNCH_RET();
}

extern "C" int ick_greedy_select(const float* scores, int64_t ld, int32_t B, int32_t Vx, int64_t* output,
                                 int32_t* top2_hist, int32_t* finished, int64_t* next_token, int64_t* next_mask,
                                 int32_t step, int32_t max_len, int32_t V, int32_t K, int32_t has_facts,
                                 int32_t end_token, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && output && top2_hist && finished && next_token && next_mask);
    ICK_CHECK_ARG(B > 0 && Vx > 0 && ld >= Vx && step >= 0 && step < max_len);
    hipLaunchKernelGGL(greedy_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, scores, ld, Vx, output,
                       top2_hist, finished, next_token, next_mask, step, max_len, V, K, has_facts, end_token);
    ICK_LAUNCH_RET();
}

static int packed_ce_impl(const float* scores, int64_t ld, const int64_t* captions_sorted,
                             const int32_t* decode_len, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                             float* row_loss, float* loss_sum, float* count, float* dscores, float* mean, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && captions_sorted && decode_len && row_loss && loss_sum && count);
    ICK_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Vx > 0 && ld >= Vx);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(packed_ce_rows_kernel<false>, dim3(L, B), dim3(256), 0, s, scores, ld, captions_sorted, decode_len,
                       L, Vx, pad_token, row_loss, dscores, nullptr, nullptr, CeEps<false>{});
    hipLaunchKernelGGL(packed_ce_reduce_kernel<false>, dim3(1), dim3(256), 0, s, row_loss, B * L, L, nullptr, loss_sum,
                       count, nullptr, nullptr, mean);
    ICK_LAUNCH_RET();
}

static int packed_ce_packed_impl(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                    const int32_t* count, const float* weights, int32_t B, int32_t L, int32_t Vx,
                                    int32_t pad_token, float* row_loss, float* loss_sum, float* count_out, float* dscores,
                                    float* mean, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && captions && rowmap && count && row_loss && loss_sum && count_out);
    ICK_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Vx > 0 && ld >= Vx && (int64_t)B * L <= INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    if (weights != nullptr) {
        hipLaunchKernelGGL((packed_ce_rows_kernel<true, true>), dim3(L, B), dim3(256), 0, s, scores, ld, captions, count, L,
                           Vx, pad_token, row_loss, dscores, weights, rowmap, CeEps<false>{});
        hipLaunchKernelGGL(packed_ce_reduce_kernel<true>, dim3(1), dim3(256), 0, s, row_loss, B * L, L, weights, loss_sum,
                           count_out, rowmap, count, mean);
    } else {
        hipLaunchKernelGGL((packed_ce_rows_kernel<false, true>), dim3(L, B), dim3(256), 0, s, scores, ld, captions, count, L,
                           Vx, pad_token, row_loss, dscores, nullptr, rowmap, CeEps<false>{});
        hipLaunchKernelGGL(packed_ce_reduce_kernel<false>, dim3(1), dim3(256), 0, s, row_loss, B * L, L, nullptr, loss_sum,
                           count_out, rowmap, count, mean);
    }
    ICK_LAUNCH_RET();
}

static int packed_ce_smooth_impl(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                    const int32_t* count, const int32_t* decode_len, const float* weights,
                                    const float* eps, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                                    float* row_loss, float* loss_sum, float* count_out, float* dscores, float* mean,
                                    void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && captions && eps && row_loss && loss_sum && count_out);
    ICK_CHECK_ARG((rowmap != nullptr) == (count != nullptr) && (rowmap != nullptr || decode_len != nullptr));
    ICK_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Vx > 0 && ld >= Vx && (int64_t)B * L <= INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid(L, B), block(256);
    const int32_t* dl = rowmap ? count : decode_len;
#define ICK_CE_SMOOTH(W, P)                                                                                            \
    hipLaunchKernelGGL((packed_ce_rows_kernel<W, P, true>), grid, block, 0, s, scores, ld, captions, dl, L, Vx,         \
                       pad_token, row_loss, dscores, weights, rowmap, CeEps<true>{eps})
    if (weights != nullptr) {
        if (rowmap) { ICK_CE_SMOOTH(true, true); } else { ICK_CE_SMOOTH(true, false); }
        hipLaunchKernelGGL(packed_ce_reduce_kernel<true>, dim3(1), block, 0, s, row_loss, B * L, L, weights, loss_sum,
                           count_out, rowmap, count, mean);
    } else {
        if (rowmap) { ICK_CE_SMOOTH(false, true); } else { ICK_CE_SMOOTH(false, false); }
        hipLaunchKernelGGL(packed_ce_reduce_kernel<false>, dim3(1), block, 0, s, row_loss, B * L, L, nullptr, loss_sum,
                           count_out, rowmap, count, mean);
    }
#undef ICK_CE_SMOOTH
    ICK_LAUNCH_RET();
}

extern "C" int ick_row_logprob_rank(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                    const int32_t* count, int32_t R, int32_t L, int32_t Vx, int32_t pad_token,
                                    float* token_log_prob, int32_t* rank, int32_t* best, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && captions && rowmap && count && token_log_prob && rank && best);
    ICK_CHECK_ARG(R > 0 && R <= 65535 && L > 1 && Vx > 0 && Vx <= (1 << 24) && ld >= Vx && (int64_t)R * L <= INT32_MAX);
    hipLaunchKernelGGL(row_logprob_rank_kernel, dim3(L, R), dim3(256), 0, (hipStream_t)stream, scores, ld, captions,
                       rowmap, count, L, Vx, pad_token, token_log_prob, rank, best);
    ICK_LAUNCH_RET();
}

extern "C" int ick_caption_score_sums(const int32_t* rowstart, int32_t R, int32_t L, int32_t top_k, float* token_log_prob,
                                      int32_t* rank, int32_t* best, float* log_prob, int32_t* tokens, float* loss_sum,
                                      float* count, float* top1_hits, float* topk_hits, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(rowstart && token_log_prob && rank && best && log_prob && tokens && loss_sum && count && top1_hits &&
                  topk_hits);
    ICK_CHECK_ARG(R > 0 && L > 1 && top_k >= 1 && (int64_t)R * L <= INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(caption_sums_kernel, dim3(ceil_div(R, 4)), dim3(256), 0, s, rowstart, R, L, token_log_prob, rank,
                       best, log_prob, tokens);
    hipLaunchKernelGGL(caption_totals_kernel, dim3(1), dim3(256), 0, s, token_log_prob, rank, (int64_t)R * (L - 1), top_k,
                       loss_sum, count, top1_hits, topk_hits);
    ICK_LAUNCH_RET();
}

static int packed_ce_weighted_impl(const float* scores, int64_t ld, const int64_t* captions_sorted,
                                      const int32_t* decode_len, const float* weights, int32_t B, int32_t L, int32_t Vx,
                                      int32_t pad_token, float* row_loss, float* loss_sum, float* count, float* dscores,
                                      float* mean, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(scores && captions_sorted && decode_len && weights && row_loss && loss_sum && count);
    ICK_CHECK_ARG(B > 0 && B <= 65535 && L > 0 && Vx > 0 && ld >= Vx && (int64_t)B * L <= INT32_MAX);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(packed_ce_rows_kernel<true>, dim3(L, B), dim3(256), 0, s, scores, ld, captions_sorted, decode_len,
                       L, Vx, pad_token, row_loss, dscores, weights, nullptr, CeEps<false>{});
    hipLaunchKernelGGL(packed_ce_reduce_kernel<true>, dim3(1), dim3(256), 0, s, row_loss, B * L, L, weights, loss_sum,
                       count, nullptr, nullptr, mean);
    ICK_LAUNCH_RET();
}

// ---- the C entries of the packed cross entropy: the two-launch forms, and the same with the mean loss written by the
// reduction (ick_packed_ce_*_mean) -----------------------------------------------------------------
extern "C" int ick_packed_ce(const float* scores, int64_t ld, const int64_t* captions_sorted, const int32_t* decode_len,
                             int32_t B, int32_t L, int32_t Vx, int32_t pad_token, float* row_loss, float* loss_sum,
                             float* count, float* dscores, void* stream) {
    return packed_ce_impl(scores, ld, captions_sorted, decode_len, B, L, Vx, pad_token, row_loss, loss_sum, count, dscores,
                          nullptr, stream);
}

extern "C" int ick_packed_ce_weighted(const float* scores, int64_t ld, const int64_t* captions_sorted,
                                      const int32_t* decode_len, const float* weights, int32_t B, int32_t L, int32_t Vx,
                                      int32_t pad_token, float* row_loss, float* loss_sum, float* count, float* dscores,
                                      void* stream) {
    return packed_ce_weighted_impl(scores, ld, captions_sorted, decode_len, weights, B, L, Vx, pad_token, row_loss, loss_sum,
                                   count, dscores, nullptr, stream);
}

extern "C" int ick_packed_ce_packed(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                    const int32_t* count, const float* weights, int32_t B, int32_t L, int32_t Vx,
                                    int32_t pad_token, float* row_loss, float* loss_sum, float* count_out, float* dscores,
                                    void* stream) {
    return packed_ce_packed_impl(scores, ld, captions, rowmap, count, weights, B, L, Vx, pad_token, row_loss, loss_sum,
                                 count_out, dscores, nullptr, stream);
}

extern "C" int ick_packed_ce_smooth(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                    const int32_t* count, const int32_t* decode_len, const float* weights,
                                    const float* eps, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                                    float* row_loss, float* loss_sum, float* count_out, float* dscores, void* stream) {
    return packed_ce_smooth_impl(scores, ld, captions, rowmap, count, decode_len, weights, eps, B, L, Vx, pad_token, row_loss,
                                 loss_sum, count_out, dscores, nullptr, stream);
}

// (weights == NULL: the plain entry, ick_packed_ce)
extern "C" int ick_packed_ce_weighted_mean(const float* scores, int64_t ld, const int64_t* captions_sorted,
                                           const int32_t* decode_len, const float* weights, int32_t B, int32_t L,
                                           int32_t Vx, int32_t pad_token, float* row_loss, float* loss_sum, float* count,
                                           float* dscores, float* mean, void* stream) {
    ICK_CHECK_ARG(mean != nullptr);
    if (weights == nullptr)
        return packed_ce_impl(scores, ld, captions_sorted, decode_len, B, L, Vx, pad_token, row_loss, loss_sum, count,
                              dscores, mean, stream);
    return packed_ce_weighted_impl(scores, ld, captions_sorted, decode_len, weights, B, L, Vx, pad_token, row_loss, loss_sum,
                                   count, dscores, mean, stream);
}

extern "C" int ick_packed_ce_packed_mean(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                         const int32_t* count, const float* weights, int32_t B, int32_t L, int32_t Vx,
                                         int32_t pad_token, float* row_loss, float* loss_sum, float* count_out,
                                         float* dscores, float* mean, void* stream) {
    ICK_CHECK_ARG(mean != nullptr);
    return packed_ce_packed_impl(scores, ld, captions, rowmap, count, weights, B, L, Vx, pad_token, row_loss, loss_sum,
                                 count_out, dscores, mean, stream);
}

extern "C" int ick_packed_ce_smooth_mean(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                                         const int32_t* count, const int32_t* decode_len, const float* weights,
                                         const float* eps, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                                         float* row_loss, float* loss_sum, float* count_out, float* dscores, float* mean,
                                         void* stream) {
    ICK_CHECK_ARG(mean != nullptr);
    return packed_ce_smooth_impl(scores, ld, captions, rowmap, count, decode_len, weights, eps, B, L, Vx, pad_token, row_loss,
                                 loss_sum, count_out, dscores, mean, stream);
}
