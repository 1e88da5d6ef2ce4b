// CIDEr-D on token ids (ick_cider_d; the metric is defined in include/ick_amd.h and cider.py).
//
// One workgroup per reference image (SCST layout) or per candidate row (general mode), 1..8 waves.
//   1. Each wave turns reference rows m = wave, wave + waves, .. of the image into LDS: the compacted words, the
//      tf-idf of the n-gram that starts at every word (n = 1..4), the four norms and the bigram count.
//   2. Each wave then takes candidate rows the same way (kept in registers), and compares them with every reference in
//      index order.  Lane i owns the four n-grams that start at the row's i-th word.  Equality of n-grams is the chain
//      e1 = (w_i == v_j), e2 = e1 && (w_i+1 == v_j+1), ..: a loop over the other row's words j with four broadcast
//      reads, no hashing and no sort.  tf is the number of j that match, and a lane is an n-gram's owner if no earlier
//      word starts the same n-gram; only owners count in the norms and in the similarity sum.
//   3. df comes from the host-built table by a branch-free binary search (same iteration count in every lane: the
//      length sequence depends on U only), the four searches of a lane interleaved.
//   4. SCST layout: after a barrier, the image's n sample rewards and its baseline give the advantages.
// Every float sum runs in a fixed order (wave_sum's DPP pattern, references in index order): bit-reproducible.
#include "caption_words.h"

namespace ick {
namespace {

struct CiderArgs {
    const int64_t* cand;
    const int64_t* refs;
    const uint4* keys;
    const int32_t* df;
    const int32_t* image_index;
    float* rewards;
    float* adv;
    int N, T, B, M, Lr, U, mode, n, rows_per_img;
    float log_ref_len, inv_two_sigma2;
    WordRule words;
};

struct RowVec {
    uint32_t w[4];      // words i .. i+3 of the row (lane i); kNone past the last word
    float x[4];         // tf-idf of the (s+1)-gram at word i (0 if the row has no such n-gram)
    bool own[4];        // the first occurrence of that n-gram in the row
    float norm[4];
    int W;              // words in the row (wave-uniform)
};

__device__ __forceinline__ bool key_greater(const uint4& k, const uint32_t* q) {     // k > q, lexicographic, unsigned
    if (k.x != q[0]) return k.x > q[0];
    if (k.y != q[1]) return k.y > q[1];
    if (k.z != q[2]) return k.z > q[2];
    return k.w > q[3];
}

// The n-gram vectors of one row of `len` tokens.  Wave-uniform call: every lane of the wave must be active.
__device__ RowVec row_vector(const CiderArgs& a, const int64_t* row, int len) {
    const int lane = threadIdx.x & 63;
    RowVec v;
    int W;
    v.w[0] = compact_words(a.words, row, len, W);       // caption_words.h: shared with ick_caption_metrics
    v.W = W;
    following_words(v.w, W);
    int tf[4];
    bool first[4];
    row_ngram_counts(v.w, W, tf, first);
    // document frequencies: branch-free binary search, the four n-grams of the lane interleaved
    uint32_t q[4][4];
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
        for (int k = 0; k < 4; ++k) q[s][k] = k <= s ? v.w[k] : kNone;
    int base[4] = {0, 0, 0, 0};
    for (int n = a.U; n > 1;) {
        const int half = n >> 1;
        uint4 k[4];
#pragma unroll
        for (int s = 0; s < 4; ++s) k[s] = a.keys[base[s] + half];
#pragma unroll
        for (int s = 0; s < 4; ++s) base[s] = key_greater(k[s], q[s]) ? base[s] : base[s] + half;
        n -= half;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const uint4 k = a.keys[base[s]];
        const bool found = k.x == q[s][0] && k.y == q[s][1] && k.z == q[s][2] && k.w == q[s][3];
        const float df = found ? (float)a.df[base[s]] : 0.f;
        const bool valid = lane + s < W;
        v.x[s] = valid ? (float)tf[s] * (a.log_ref_len - logf(fmaxf(1.f, df))) : 0.f;
        v.own[s] = valid && first[s];
        v.norm[s] = sqrtf(wave_sum(v.own[s] ? v.x[s] * v.x[s] : 0.f));
    }
    return v;
}

struct RefLds {
    uint32_t w[kMaxRefs][kMaxLen + 4];      // compacted words, kNone from W on
    float x[kMaxRefs][4][kMaxLen];          // tf-idf of the (s+1)-gram at word j, every occurrence
    float norm[kMaxRefs][4];
    int W[kMaxRefs];
    float reward[kMaxLen];                  // SCST layout: the image's rewards, for the advantages
};

__global__ __launch_bounds__(kMaxWaves * 64) void cider_kernel(CiderArgs a) {
    __shared__ RefLds L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const bool general = a.mode == 0;
    const int img = general ? a.image_index[blockIdx.x] : (int)blockIdx.x;
    const bool bad = img < 0 || img >= a.B;                 // general mode: an index outside the reference block
    const int rows = general ? 1 : a.rows_per_img;
    if (!bad) {
        for (int m = wave; m < a.M; m += waves) {
            const RowVec r = row_vector(a, a.refs + ((int64_t)img * a.M + m) * a.Lr, a.Lr);
            L.w[m][lane] = r.w[0];
            if (lane < 4) L.w[m][kMaxLen + lane] = kNone;
#pragma unroll
            for (int s = 0; s < 4; ++s) L.x[m][s][lane] = r.x[s];
            if (lane == 0) {
#pragma unroll
                for (int s = 0; s < 4; ++s) L.norm[m][s] = r.norm[s];
                L.W[m] = r.W;
            }
        }
    }
    __syncthreads();
    for (int r = wave; r < rows; r += waves) {
        const int64_t row = general ? (int64_t)blockIdx.x : (r < a.n ? (int64_t)img * a.n + r : (int64_t)a.B * a.n + img);
        float reward = __builtin_nanf("");
        if (!bad) {
            const RowVec c = row_vector(a, a.cand + row * a.T, a.T);
            const float len_c = (float)max(c.W - 1, 0);         // coco-caption's length: the bigram count
            float acc = 0.f;
            for (int m = 0; m < a.M; ++m) {
                const int Wr = L.W[m];
                float xr[4] = {0.f, 0.f, 0.f, 0.f};
                for (int j = 0; j < Wr; ++j) {
                    const bool e1 = c.w[0] == L.w[m][j];
                    const bool e2 = e1 && c.w[1] == L.w[m][j + 1];
                    const bool e3 = e2 && c.w[2] == L.w[m][j + 2];
                    const bool e4 = e3 && c.w[3] == L.w[m][j + 3];
                    const bool eq[4] = {e1, e2, e3, e4};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (eq[s]) xr[s] = L.x[m][s][j];
                }
                const float delta = len_c - (float)max(Wr - 1, 0);
                const float g = expf(-(delta * delta) * a.inv_two_sigma2);
                float score = 0.f;
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float val = wave_sum(c.own[s] ? fminf(c.x[s], xr[s]) * xr[s] : 0.f);
                    const float nn = c.norm[s] * L.norm[m][s];
                    score += (c.norm[s] != 0.f && L.norm[m][s] != 0.f ? val / nn : 0.f) * g;
                }
                acc += score * 0.25f;
            }
            reward = acc / (float)a.M * 10.f;
        }
        if (lane == 0) {
            a.rewards[row] = reward;
            if (!general) L.reward[r] = reward;
        }
    }
    if (general) return;
    __syncthreads();
    const int n = a.n;
    if ((int)threadIdx.x < n) {
        const float rj = L.reward[threadIdx.x];
        float b;
        if (a.mode == 1) {
            b = L.reward[n];                                        // the greedy caption's reward
        } else {
            float sum = 0.f;
            for (int k = 0; k < n; ++k) sum += L.reward[k];
            b = (sum - rj) / (float)(n - 1);                        // leave-one-out mean
        }
        a.adv[(int64_t)img * n + threadIdx.x] = rj - b;
    }
}

}  // namespace
}  // namespace ick

extern "C" int ick_cider_d(const int64_t* cand, int32_t N, int32_t T, const int64_t* refs, int32_t B, int32_t M,
                           int32_t Lr, const uint32_t* df_keys, const int32_t* df_count, int32_t U, float log_ref_len,
                           float sigma, int32_t start_token, int32_t end_token, int32_t pad_token,
                           const int32_t* ignore, int32_t n_ignore, int32_t mode, const int32_t* image_index,
                           int32_t num_samples, float* rewards, float* advantages, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(cand && refs && df_keys && df_count && rewards);
    ICK_CHECK_ARG(N > 0 && T > 0 && T <= kMaxLen && B > 0 && M > 0 && M <= kMaxRefs && Lr > 0 && Lr <= kMaxLen);
    ICK_CHECK_ARG(U > 0 && sigma > 0.f && sigma < 3.0e38f && log_ref_len >= 0.f && log_ref_len < 3.0e38f);
    ICK_CHECK_ARG(n_ignore >= 0 && n_ignore <= kMaxIgnore && (n_ignore == 0 || ignore));
    ICK_CHECK_ARG(mode >= 0 && mode <= 2);
    if (((uintptr_t)df_keys & 15) != 0) return ICK_EALIGN;
    CiderArgs a{};
    a.cand = cand; a.refs = refs; a.keys = (const uint4*)df_keys; a.df = df_count; a.image_index = image_index;
    a.rewards = rewards; a.adv = advantages;
    a.N = N; a.T = T; a.B = B; a.M = M; a.Lr = Lr; a.U = U; a.mode = mode; a.n = num_samples;
    a.log_ref_len = log_ref_len;
    a.inv_two_sigma2 = 1.f / (2.f * sigma * sigma);
    a.words.start = start_token; a.words.end = end_token; a.words.pad = pad_token; a.words.n_ignore = n_ignore;
    for (int k = 0; k < n_ignore; ++k) a.words.ignore[k] = ignore[k];
    int grid, rows;
    if (mode == 0) {
        ICK_CHECK_ARG(image_index);
        grid = N;
        rows = 1;
    } else {
        ICK_CHECK_ARG(advantages && num_samples >= 1 && (mode == 1 || num_samples >= 2));
        rows = num_samples + (mode == 1 ? 1 : 0);
        ICK_CHECK_ARG(rows <= kMaxLen && (int64_t)B * rows == (int64_t)N);
        grid = B;
    }
    a.rows_per_img = rows;
    const int waves = max(1, min(kMaxWaves, max(M, rows)));
    hipLaunchKernelGGL(cider_kernel, dim3(grid), dim3(waves * 64), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}
