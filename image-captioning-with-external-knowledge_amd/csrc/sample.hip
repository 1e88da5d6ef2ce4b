// Sampled caption decoding (DecoderTransformer.predict_sample): the selection step that replaces
// dec_select_kernel when a token is DRAWN instead of taken by argmax.  One workgroup of 1024 threads per row
// (R = captions x samples; the rows of a caption share its cross K/V in the layer kernels of csrc/decode.hip).
//
// For one row at one step, s = the V + K + F raw scores (ctx->scores for the words, ctx->ptr for the pointers):
//   z = s / T
//   top-k (k > 0):  keep s >= the k-th largest s (ties at the boundary are all kept)
//   top-p (p < 1):  over the kept set, w = exp(z - max z); keep t iff the mass of the kept tokens with z STRICTLY
//                   greater than z_t is < p * sum(w)
//   draw:           argmax over the kept set of z_t + g_t, ties to the smaller column; g_t = -log(-log(u_t)) in fp32
//                   (accurate logf), u_t = min(fl32((x[c & 3] >> 8) + 0.5) * 2^-24, 1 - 2^-24) where x = Philox-4x32-10
//                   of counter (c >> 2, step, sample j, caption b) under key (seed lo, seed hi).  The clamp keeps the
//                   one draw in 2^24 whose fp32 sum rounds up to 1.0 from becoming g = +inf.
// The noise of a column is a pure function of (seed, b, j, step, c): a caption's samples do not depend on the batch.
// log_prob receives the model's log_softmax(s)[token] (T = 1, no truncation).  No repeated n-gram clean-up.
// Decoding rules (ick_decode_select_sample_rules): columns banned by the no-repeat n-gram / min-length
// rules are absent before top-k and top-p (not counted in k, no mass; the top-p weights are taken relative to the
// allowed maximum) and from the draw; m, the sum of exp and log_prob still cover every column.
// Column bias (ick_decode_select_sample_biased): everything that selects -- the top-k threshold, z, the
// top-p weights and their maximum, the Gumbel arg-max -- runs on s' = s + b; a column with b = -inf is absent like a
// banned one.  m, the sum of exp and log_prob stay on the raw s, and a column's noise does not change.
//
// Determinism: every thread owns the same columns on every launch (lane t of group g: columns 4 (g*1024 + t) + 0..3),
// float reductions run per lane in column order, then over the wave (DPP / readlane, fixed pattern), then over the 16
// waves in wave order.  The thresholds are found by MSB-first radix select over the order-preserving uint32 key of s
// (top-k) and of z (top-p): four 8-bit digits, 256-bin LDS histograms filled with INTEGER atomics only -- counts for
// top-k, and for top-p fixed-point masses (u64, w rounded to 2^-32; an integer sum does not depend on the order the
// atomics land in).  At the top-p boundary the comparison is made on those fixed-point masses: G_fix(z_t) < p * W_fix
// (W_fix = the sum of the kept tokens' fixed-point weights, compared in double, exact below 2^53), so a token whose
// strictly-greater mass lies within ~Vx * 2^-33 of p * W can go either way relative to an exact-real restatement.
#include "common.h"
#include "philox.h"

#include <climits>
#include <type_traits>

namespace ick {
namespace {

constexpr int kSNT = 1024;                 // threads per workgroup (one row)
constexpr int kSNW = kSNT / kWave;
constexpr int kSGMax = 16;                 // groups of 4 columns per lane
constexpr int kSVxMax = kSGMax * 4 * kSNT; // 65 536 scores per row

struct SampleArgs {
    const float* scores; int64_t ld;       // (R, ld) word logits
    const float* ptr;                      // (R, K + F) pointer scores
    const int64_t* seed;                   // (1) device word
    const float* temp_top_p;               // (2) temperature, top_p
    const int32_t* top_k;                  // (1) 0 = off
    float* log_prob;                       // optional (R, max_len)
    int64_t* output;                       // (R, max_len)
    int32_t* finished;                     // (R)
    int32_t* n_done;                       // number of finished rows
    int64_t* next_token; int64_t* next_mask;
    int64_t* cap_buf;                      // optional (R, max_len)
    const float *word_emb, *ee, *fe, *pe;
    float* x0;                             // (R, d)
    int R, rows_per_sample, d, V, K, F, step, max_len, has_facts, end_token, pad_token;
    float emb_scale;
    int n_total;
    const int32_t* words;                  // optional rule words (no-repeat n-gram size, min length)
};

// The column-bias variant (BIASED) appends the bias lists (R / rows_per_sample, kBiasMax), for that variant alone: the
// hidden launch arguments the other instantiations read follow the explicit ones, and would move with them.
struct SampleBiasArgs : SampleArgs {
    const int32_t* bcols; const float* bvals;
};

// order-preserving key of a float (larger float -> larger key); -0 is folded onto +0 first (x + 0 = +0 for x = -0)
__device__ __forceinline__ uint32_t okey(float f) {
    const uint32_t b = __float_as_uint(f + 0.0f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// Wave 0 scans a 256-bin histogram from the top digit down and returns (in LDS) the first digit whose inclusive
// running total reaches `need` (counts) -- lane l owns digits 255 - 4l .. 252 - 4l.
template <typename T>
__device__ __forceinline__ void scan_desc(const T* hist, T need, T above, int* dig_out, T* above_out, int lane) {
    T c[4], loc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) { c[q] = hist[255 - 4 * lane - q]; loc += c[q]; }
    T incl = loc;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const T o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    T run = above + incl - loc;
    const bool hit = run < need && above + incl >= need;
    if (hit) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (run + c[q] >= need) { *dig_out = 255 - 4 * lane - q; *above_out = run; break; }
            run += c[q];
        }
    }
}

// The caption-prefix variant (PREFIX) appends the forced column of every step (R / rows_per_sample, max_len), -1 = a free
// step, to the plain and to the biased arguments, again for its own instantiations alone.
struct SamplePrefixArgs : SampleArgs {
    const int32_t* pcols;
};
struct SampleBiasPrefixArgs : SampleBiasArgs {
    const int32_t* pcols;
};
template <bool BIASED, bool PREFIX>
using SampleArgsOf = std::conditional_t<PREFIX, std::conditional_t<BIASED, SampleBiasPrefixArgs, SamplePrefixArgs>,
                                        std::conditional_t<BIASED, SampleBiasArgs, SampleArgs>>;

// Thread 0 records the token of step i of row r: column bc with raw score bs, under the row's raw maximum m and sum of
// exp(s - m).  tok_sh receives the next input token and its mask.
__device__ __forceinline__ void record_token(const SampleArgs& a, int64_t r, int i, int bc, float bs, float m, float sum,
                                             int64_t* tok_sh) {
    int64_t* o = a.output + r * a.max_len;
    if (a.log_prob != nullptr) a.log_prob[r * a.max_len + i] = (bs - m) - logf(sum);
    o[i] = bc;
    int64_t tok = 0, msk = 0;
    if (bc == a.end_token) {
        a.finished[r] = 1;
        atomicAdd(a.n_done, 1);
    } else {
        tok = bc;
        msk = token_kind(bc, a.V, a.K, a.has_facts);
    }
    tok_sh[0] = tok;
    tok_sh[1] = msk;
}

// After the step's token is in tok_sh (and a barrier): the row's next input token and mask, its caption buffer, and
// CaptionEmbedder + sqrt(d) scale + PositionEncoder of the next input token (as dec_select_kernel).
__device__ __forceinline__ void feed_next(const SampleArgs& a, int64_t r, int i, const int64_t* tok_sh) {
    const int tid = threadIdx.x;
    const int64_t tok = tok_sh[0], msk = tok_sh[1];
    if (tid == 0) {
        a.next_token[r] = tok;
        a.next_mask[r] = msk;
        if (a.cap_buf != nullptr && i + 1 < a.max_len) a.cap_buf[r * a.max_len + i + 1] = tok;
    }
    if (i + 1 >= a.max_len) return;
    const float* src = token_row(tok, (int)msk, r / a.rows_per_sample, a.word_emb, a.ee, a.fe, a.V, a.K, a.F, a.d,
                                 a.pad_token);
    const float* pe = a.pe + (int64_t)(i + 1) * a.d;
    for (int c = tid; c < a.d; c += kSNT) a.x0[r * a.d + c] = fmaf(src[c], a.emb_scale, pe[c]);
}

// NG = groups of 4 columns a lane holds in registers: 4 (Vx <= 16 384, cfg5) keeps them in VGPRs; 16 (cfg4's 50 071)
// exceeds the 128 registers a lane of a 1024-thread workgroup has and spills part of the row to scratch.
// RULES: the decoding-rules variant (ick_decode_select_sample_rules); the rule-free one compiles without the ban pass.
// BIASED: column bias (ick_decode_select_sample_biased), on the rules form.
// PREFIX: caption prefixes (ick_decode_select_sample_prefix), on the rules form, plain and biased.
template <int NG, bool RULES, bool BIASED = false, bool PREFIX = false>
__global__ __launch_bounds__(kSNT) void dec_sample_kernel(SampleArgsOf<BIASED, PREFIX> a) {
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t r = blockIdx.x;
    const int i = a.step;
    // the knobs, the early-exit count and this row's flag through the scalar cache, one wait for all of them (as
    // epoch_seed() in common.h: they were written by earlier launches, and a dispatch starts with a clean scalar cache)
    uint32_t nd, fin, kk;
    uint64_t sd, tp;
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile(
        "s_load_dword %0, %5, 0x0\n\t"
        "s_load_dword %1, %6, 0x0\n\t"
        "s_load_dwordx2 %2, %7, 0x0\n\t"
        "s_load_dwordx2 %3, %8, 0x0\n\t"
        "s_load_dword %4, %9, 0x0\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&s"(nd), "=&s"(fin), "=&s"(sd), "=&s"(tp), "=&s"(kk)
        : "s"(a.n_done), "s"(a.finished + r), "s"(a.seed), "s"(a.temp_top_p), "s"(a.top_k)
        : "memory");
#else
    nd = *a.n_done; fin = a.finished[r]; sd = *a.seed; tp = *(const uint64_t*)a.temp_top_p; kk = *a.top_k;
#endif
    if ((int)nd >= a.n_total) return;

    __shared__ float red[2][kSNW];
    __shared__ uint32_t hist_n[256];
    __shared__ unsigned long long hist_m[256];
    __shared__ int dig_sh;
    __shared__ uint32_t need_sh;
    __shared__ unsigned long long above_sh;
    __shared__ float bv_sh[kSNW], bs_sh[kSNW];
    __shared__ int bc_sh[kSNW];
    __shared__ int64_t tok_sh[2];
    __shared__ uint32_t ban[NG * kSNT * 4 / 32];
    __shared__ int hs[kRuleHistMax];
    __shared__ int all_sh;

    // A forced step of a caption prefix (uniform: one caption per workgroup, so the barriers below are met by every
    // thread): the token is the given column, whatever the rules ban -- no ban pass, bias, top-k, top-p or noise.  The
    // raw maximum and sum of exp are formed as below, over the same columns per lane and in the same order, but
    // streamed from the score row (it is read twice, from cache the second time) instead of held in registers; thread 0
    // then records the column with its raw score as it records a drawn one, and the step ends as every step does.
    if constexpr (PREFIX) {
        const int fcol = __builtin_amdgcn_readfirstlane(a.pcols[(r / a.rows_per_sample) * a.max_len + i]);
        const int np = a.K + a.F, Vx = a.V + np;
        if (!fin && fcol >= 0 && fcol < Vx) {
            const int ng = (Vx + 4 * kSNT - 1) / (4 * kSNT);
            const float* srow = a.scores + r * a.ld;
            const float* prow = a.ptr + r * np;
            float m = -INFINITY;
            for (int g = 0; g < ng; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = (g * kSNT + tid) * 4 + q;
                    if (c < Vx) m = fmaxf(m, c < a.V ? srow[c] : prow[c - a.V]);
                }
            m = wave_max(m);
            if (lane == 0) red[0][wid] = m;
            __syncthreads();
            m = red[0][0];
#pragma unroll
            for (int w = 1; w < kSNW; ++w) m = fmaxf(m, red[0][w]);
            float se = 0.f;
            for (int g = 0; g < ng; ++g)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int c = (g * kSNT + tid) * 4 + q;
                    if (c < Vx) se += expf((c < a.V ? srow[c] : prow[c - a.V]) - m);
                }
            se = wave_sum(se);
            if (lane == 0) red[1][wid] = se;
            __syncthreads();
            if (tid == 0) {
                float sum = red[1][0];
                for (int w = 1; w < kSNW; ++w) sum += red[1][w];
                record_token(a, r, i, fcol, fcol < a.V ? srow[fcol] : prow[fcol - a.V], m, sum, tok_sh);
            }
            __syncthreads();
            feed_next(a, r, i, tok_sh);
            return;
        }
    }
    const uint4 rw = RULES ? rule_words(a.words) : make_uint4(0u, 0u, 0u, 0u);
    const int nrep = (int)rw.x, mlen = (int)rw.y;
    // decoding rules (uniform): banned columns are absent from top-k, top-p and the draw -- not from the log-softmax
    const bool ban_any = RULES && !fin && (nrep > 0 || i < mlen);
    if (ban_any) mark_bans(a.output + r * a.max_len, i, nrep, mlen, a.end_token, ban, 0, NG * kSNT * 4 / 32, hs);

    if (!fin) {
        const float T = __uint_as_float((uint32_t)tp), top_p = __uint_as_float((uint32_t)(tp >> 32));
        const int top_k = (int)kk;
        const int np = a.K + a.F, Vx = a.V + np;
        const int ng = (Vx + 4 * kSNT - 1) / (4 * kSNT);          // uniform
        const float* srow = a.scores + r * a.ld;
        const float* prow = a.ptr + r * np;
        float s[NG * 4];
#pragma unroll
        for (int g = 0; g < NG; ++g) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int c = (g * kSNT + tid) * 4 + q;
                s[g * 4 + q] = g >= ng ? -INFINITY : (c < a.V ? srow[c] : (c < Vx ? prow[c - a.V] : -INFINITY));
            }
        }
        // banned[g * 4 + q]: column (g * 1024 + tid) * 4 + q is banned (the 4 columns of a group share a mask word)
        uint64_t banned = 0;
        if (ban_any) {
#pragma unroll
            for (int g = 0; g < NG; ++g) {
                const int c = (g * kSNT + tid) * 4;
                if (g < ng) banned |= (uint64_t)((ban[c >> 5] >> (c & 31)) & 15u) << (4 * g);
            }
        }
        // pass 1: maximum, then sum(exp(s - m)) for the log-probability (T = 1, untruncated)
        float m = -INFINITY;
#pragma unroll
        for (int e = 0; e < NG * 4; ++e) m = fmaxf(m, s[e]);
        m = wave_max(m);
        if (lane == 0) red[0][wid] = m;
        __syncthreads();
        m = red[0][0];
#pragma unroll
        for (int w = 1; w < kSNW; ++w) m = fmaxf(m, red[0][w]);
        float se = 0.f;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g >= ng) continue;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((g * kSNT + tid) * 4 + q < Vx) se += expf(s[g * 4 + q] - m);
        }
        se = wave_sum(se);
        if (lane == 0) red[1][wid] = se;
        // some column may be absent from the selection (uniform)
        const bool cut = ban_any || BIASED;
        if constexpr (BIASED) {
            // Column bias, after the raw reductions: s becomes s' = s + b in place, no second copy of the row.  The
            // non-empty slots are visited in order with their column as a uniform value; column c is element
            // (c >> 12) * 4 + (c & 3) of thread (c >> 2) & 1023, its only owner, and a column's lowest slot counts.
            // b = -inf: the column is absent like a banned one.
            const BiasLanes bl = bias_lanes(a.bcols, a.bvals, r / a.rows_per_sample);
            uint64_t done = 0;
            for (unsigned long long live = bl.live(0, Vx); live != 0;) {
                const int t = BiasLanes::next(live);
                const int c = bl.col_of(t);
                const float bias = bl.val_of(t);
                const int e = ((c >> 12) << 2) | (c & 3);
                if (((c >> 2) & (kSNT - 1)) == tid && !((done >> e) & 1u)) {
                    done |= 1ull << e;
                    if (bias == -INFINITY) banned |= 1ull << e;
#pragma unroll
                    for (int e2 = 0; e2 < NG * 4; ++e2)
                        if (e2 == e) s[e2] += bias;
                }
            }
        }
        // the maximum over the allowed columns: the top-p weights are exp(z - its z)
        float mk = m;
        if (cut) {
            mk = -INFINITY;
#pragma unroll
            for (int e = 0; e < NG * 4; ++e)
                if (!((banned >> e) & 1u)) mk = fmaxf(mk, s[e]);
            mk = wave_max(mk);
            __syncthreads();                           // every wave has read red[0]
            if (lane == 0) red[0][wid] = mk;
            __syncthreads();
            mk = red[0][0];
#pragma unroll
            for (int w = 1; w < kSNW; ++w) mk = fmaxf(mk, red[0][w]);
        }
        // top-k threshold: the key of the k-th largest s (radix select on counts); 0 keeps everything
        uint32_t thk = 0;
        if (top_k > 0 && top_k < Vx) {
            uint32_t prefix = 0, pmask = 0, need = (uint32_t)top_k;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                if (tid < 256) hist_n[tid] = 0;
                __syncthreads();
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (g >= ng) continue;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const uint32_t key = okey(s[g * 4 + q]);
                        if ((g * kSNT + tid) * 4 + q < Vx && !((banned >> (g * 4 + q)) & 1u) && (key & pmask) == prefix)
                            atomicAdd(&hist_n[(key >> shift) & 255u], 1u);
                    }
                }
                __syncthreads();
                if (wid == 0) {
                    if (pass == 0 && cut) {         // k >= the allowed columns: every allowed column is kept
                        uint32_t t4 = hist_n[4 * lane] + hist_n[4 * lane + 1] + hist_n[4 * lane + 2] + hist_n[4 * lane + 3];
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) t4 += __shfl_xor(t4, off, 64);
                        if (lane == 0) all_sh = t4 <= need;
                    }
                    uint32_t above_out = 0;
                    int dig = -1;
                    scan_desc<uint32_t>(hist_n, need, 0u, &dig, &above_out, lane);
                    if (dig >= 0) { dig_sh = dig; need_sh = need - above_out; }
                }
                __syncthreads();
                if (pass == 0 && cut && all_sh) { prefix = 0; break; }         // uniform
                prefix |= (uint32_t)dig_sh << shift;
                pmask |= 255u << shift;
                need = need_sh;
            }
            thk = prefix;
        }
        const float zmax = mk / T;
        // top-p threshold: the key of the first z (descending) where the running fixed-point mass of the top-k kept
        // set reaches p * W; 0 keeps everything
        uint32_t thp = 0;
        if (top_p < 1.f) {
            uint32_t prefix = 0, pmask = 0;
            unsigned long long above = 0;
            double target = 0.0;
            for (int pass = 0; pass < 4; ++pass) {
                const int shift = 24 - 8 * pass;
                if (tid < 256) hist_m[tid] = 0;
                __syncthreads();
#pragma unroll
                for (int g = 0; g < NG; ++g) {
                    if (g >= ng) continue;
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float sv = s[g * 4 + q];
                        const float z = sv / T;
                        const uint32_t key = okey(z);
                        if ((g * kSNT + tid) * 4 + q < Vx && !((banned >> (g * 4 + q)) & 1u) && okey(sv) >= thk &&
                            (key & pmask) == prefix) {
                            const unsigned long long wf = __float2ull_rn(expf(z - zmax) * 0x1p32f);
                            if (wf) atomicAdd(&hist_m[(key >> shift) & 255u], wf);
                        }
                    }
                }
                __syncthreads();
                if (wid == 0) {
                    if (pass == 0) {        // W = the whole kept mass = the sum of the first histogram
                        unsigned long long t4 = hist_m[4 * lane] + hist_m[4 * lane + 1] + hist_m[4 * lane + 2] +
                                                hist_m[4 * lane + 3];
#pragma unroll
                        for (int off = 32; off >= 1; off >>= 1) t4 += __shfl_xor(t4, off, 64);
                        target = (double)top_p * (double)t4;
                    }
                    // the integer `need` of scan_desc: the smallest integer mass >= p * W
                    const unsigned long long need = (unsigned long long)ceil(target);
                    unsigned long long above_out = 0;
                    int dig = -1;
                    scan_desc<unsigned long long>(hist_m, need, above, &dig, &above_out, lane);
                    if (dig >= 0) { dig_sh = dig; above_sh = above_out; }
                }
                __syncthreads();
                prefix |= (uint32_t)dig_sh << shift;
                pmask |= 255u << shift;
                above = above_sh;
            }
            thp = prefix;
        }
        // Gumbel-max over the kept set
        const uint32_t b = (uint32_t)(r / a.rows_per_sample), j = (uint32_t)(r % a.rows_per_sample);
        const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
        float bv = -INFINITY, bs = 0.f;
        int bc = INT_MAX;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g >= ng) continue;
            const uint32_t quad = (uint32_t)(g * kSNT + tid);
            bool kept[4], anyk = false;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float sv = s[g * 4 + q];
                kept[q] = (int)(quad * 4 + q) < Vx && !((banned >> (g * 4 + q)) & 1u) && okey(sv) >= thk &&
                          okey(sv / T) >= thp;
                anyk |= kept[q];
            }
            if (!anyk) continue;
            const uint4 x = philox4x32_10(make_uint4(quad, (uint32_t)i, j, b), k0, k1);
            const uint32_t xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                if (!kept[q]) continue;
                const float sv = s[g * 4 + q];
                const float v = sv / T + gumbel(xs[q]);
                if (v > bv) { bv = v; bc = (int)(quad * 4 + q); bs = sv; }   // columns ascend: ties keep the smaller
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const float ov = __shfl_xor(bv, off, 64), os = __shfl_xor(bs, off, 64);
            const int oc = __shfl_xor(bc, off, 64);
            if (ov > bv || (ov == bv && oc < bc)) { bv = ov; bc = oc; bs = os; }
        }
        if (lane == 0) { bv_sh[wid] = bv; bc_sh[wid] = bc; bs_sh[wid] = bs; }
        __syncthreads();
        if (tid == 0) {
            bv = bv_sh[0]; bc = bc_sh[0]; bs = bs_sh[0];
            for (int w = 1; w < kSNW; ++w)
                if (bv_sh[w] > bv || (bv_sh[w] == bv && bc_sh[w] < bc)) { bv = bv_sh[w]; bc = bc_sh[w]; bs = bs_sh[w]; }
            float sum = red[1][0];
            for (int w = 1; w < kSNW; ++w) sum += red[1][w];
            if constexpr (BIASED) {         // log_prob is the model's: the drawn column's raw score, from the score row
                if (bc < Vx) bs = bc < a.V ? srow[bc] : prow[bc - a.V];
            }
            record_token(a, r, i, bc, bs, m, sum, tok_sh);
        }
    } else if (tid == 0) {
        tok_sh[0] = 0;
        tok_sh[1] = 0;
    }
    __syncthreads();
    feed_next(a, r, i, tok_sh);
}

}  // namespace
}  // namespace ick

using namespace ick;

extern "C" int ick_decode_sample_supported(int32_t Vx, int32_t rows_per_sample) {
    return Vx >= 1 && Vx <= kSVxMax && rows_per_sample >= 1 && rows_per_sample <= 65535 ? 1 : 0;
}

static int select_sample_impl(const ick_decode_ctx* c, const ick_sample_state* s, const ick_decode_rules* rules,
                              const ick_decode_bias* bias, const ick_decode_prefix* px, int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && s && c->R > 0 && c->R <= 65535 && pos >= 0 && pos < c->max_len);
    ICK_CHECK_ARG(c->rows_per_sample >= 1 && c->R % c->rows_per_sample == 0);
    ICK_CHECK_ARG(c->V > 0 && c->K > 0 && c->F >= 0 && c->end_token >= 0 && c->end_token < c->V);
    ICK_CHECK_ARG(ick_decode_sample_supported(c->V + c->K + c->F, c->rows_per_sample));
    ICK_CHECK_ARG(c->scores && c->scores_ld >= c->V && c->ptr && c->output && c->finished && c->n_done &&
                  c->next_token && c->next_mask && c->word_emb && c->pe && c->x0 && c->ee && (c->F == 0 || c->fe));
    // the knobs are read with scalar loads: dword-aligned addresses
    ICK_CHECK_ARG(s->seed && s->temp_top_p && s->top_k && ((uintptr_t)s->seed & 3) == 0 &&
                  ((uintptr_t)s->temp_top_p & 3) == 0 && ((uintptr_t)s->top_k & 3) == 0);
    SampleArgs a;
    a.scores = c->scores; a.ld = c->scores_ld; a.ptr = c->ptr;
    a.seed = s->seed; a.temp_top_p = s->temp_top_p; a.top_k = s->top_k; a.log_prob = s->log_prob;
    a.output = c->output; a.finished = c->finished; a.n_done = c->n_done;
    a.next_token = c->next_token; a.next_mask = c->next_mask; a.cap_buf = c->cap_buf;
    a.word_emb = c->word_emb; a.ee = c->ee; a.fe = c->F > 0 ? c->fe : nullptr; a.pe = c->pe; a.x0 = c->x0;
    a.R = c->R; a.rows_per_sample = c->rows_per_sample; a.d = c->d; a.V = c->V; a.K = c->K; a.F = c->F; a.step = pos;
    a.max_len = c->max_len; a.has_facts = c->F > 0; a.end_token = c->end_token; a.pad_token = c->pad_token;
    a.emb_scale = c->emb_scale; a.n_total = c->R;
    a.words = rules ? rules->words : nullptr;
    const bool small = c->V + c->K + c->F <= 4 * 4 * kSNT;
    if (bias != nullptr) {
        // the column bias is instantiated on the rules form only: without rules the rule words read as zero
        if (px != nullptr) {            // caption prefixes: on the rules form only as well, plain (below) and biased
            SampleBiasPrefixArgs xa;
            static_cast<SampleArgs&>(xa) = a;
            xa.bcols = bias->cols; xa.bvals = bias->vals; xa.pcols = px->cols;
            void (*kern)(SampleBiasPrefixArgs) = small ? dec_sample_kernel<4, true, true, true>
                                                       : dec_sample_kernel<kSGMax, true, true, true>;
            hipLaunchKernelGGL(kern, dim3(c->R), dim3(kSNT), 0, (hipStream_t)stream, xa);
            ICK_LAUNCH_RET();
        }
        SampleBiasArgs ba;
        static_cast<SampleArgs&>(ba) = a;
        ba.bcols = bias->cols; ba.bvals = bias->vals;
        void (*kern)(SampleBiasArgs) = small ? dec_sample_kernel<4, true, true> : dec_sample_kernel<kSGMax, true, true>;
        hipLaunchKernelGGL(kern, dim3(c->R), dim3(kSNT), 0, (hipStream_t)stream, ba);
        ICK_LAUNCH_RET();
    }
    if (px != nullptr) {
        SamplePrefixArgs xa;
        static_cast<SampleArgs&>(xa) = a;
        xa.pcols = px->cols;
        void (*kern)(SamplePrefixArgs) = small ? dec_sample_kernel<4, true, false, true>
                                               : dec_sample_kernel<kSGMax, true, false, true>;
        hipLaunchKernelGGL(kern, dim3(c->R), dim3(kSNT), 0, (hipStream_t)stream, xa);
        ICK_LAUNCH_RET();
    }
    void (*kern)(SampleArgs) = rules == nullptr ? (small ? dec_sample_kernel<4, false> : dec_sample_kernel<kSGMax, false>)
                                                : (small ? dec_sample_kernel<4, true> : dec_sample_kernel<kSGMax, true>);
    hipLaunchKernelGGL(kern, dim3(c->R), dim3(kSNT), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}

extern "C" int ick_decode_select_sample(const ick_decode_ctx* c, const ick_sample_state* s, int32_t pos, void* stream) {
    return select_sample_impl(c, s, nullptr, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_sample_rules(const ick_decode_ctx* c, const ick_sample_state* s,
                                              const ick_decode_rules* rules, int32_t pos, void* stream) {
    ICK_CHECK_ARG(rules_ok(c, rules, false));
    return select_sample_impl(c, s, rules, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_sample_biased(const ick_decode_ctx* c, const ick_sample_state* s,
                                               const ick_decode_rules* rules, const ick_decode_bias* bias, int32_t pos,
                                               void* stream) {
    ICK_CHECK_ARG(c && bias && bias->cols && bias->vals);
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, false));
    return select_sample_impl(c, s, rules, bias, nullptr, pos, stream);
}

extern "C" int ick_decode_select_sample_prefix(const ick_decode_ctx* c, const ick_sample_state* s,
                                               const ick_decode_rules* rules, const ick_decode_bias* bias,
                                               const ick_decode_prefix* px, int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && px && px->cols);
    ICK_CHECK_ARG(bias == nullptr || (bias->cols && bias->vals));
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, false));
    return select_sample_impl(c, s, rules, bias, px, pos, stream);
}
