// BLEU-1..4 components and sentence scores, ROUGE-L and pointer precision / recall counts on token ids
// (ick_caption_metrics, ick_caption_metric_sums; the definitions are in include/ick_amd.h and metrics.py).
//
// The launch shapes are ick_cider_d's: one workgroup per reference image (SCST layout) or per candidate row (general
// mode), 1..8 waves.
//   1. Each wave turns reference rows m = wave, wave + waves, .. of the image into LDS (the compacted words and their
//      count; caption_words.h, the code ick_cider_d runs).  With a pointer base, a second pass counts the distinct
//      pointer ids of the references taken together: the word at (m, j) counts unless an earlier (m', j') holds it.
//   2. Each wave then takes candidate rows.  Lane i owns the four n-grams that start at the row's i-th word: count_c is
//      the n-gram's matches in the row itself (taken by its first-occurrence lane), count_m its matches in reference m
//      (a loop over the reference's words with four broadcast LDS reads), clipped by the maximum over m in index
//      order.  The sums over lanes are of integers <= 64, carried as exact floats through wave_sum's fixed order.
//   3. LCS, bit-parallel (Allison-Dix / Hyyro): the reference's words sit one per lane, the match mask of candidate word
//      i is one __ballot, and V = (V + U) | (V - U) with U = V & M runs on wave-uniform 64-bit scalars; the LCS is the
//      number of zero bits of V among the reference's words.  min(c, 64) steps per pair, no table.
//   4. The sentence scores are evaluated in float64 on wave-uniform values (the formula multiplies up to four factors
//      of 1e-15: 1e-60 is below fp32's range) and rounded once to the float32 outputs, which lane 0 stores.
//   5. With reward weights: rewards, and in the SCST layout, after a barrier, the advantages by cider_kernel's formulas.
// Plain vector stores, no atomics; every result is a pure function of its row and references: bit-reproducible.
#include "caption_words.h"

namespace ick {
namespace {

struct MetricArgs {
    const int64_t* cand;
    const int64_t* refs;
    const int32_t* image_index;
    const float* base;              // rewards of a preceding ick_cider_d launch, or null
    int32_t* counts;
    float* bleu;
    float* rouge;
    int32_t* pointers;
    float* rewards;                 // null: no reward combination
    float* adv;
    int N, T, B, M, Lr, mode, n, rows_per_img, pointer_base;
    float w[6];                     // w_base, w_b1 .. w_b4, w_rouge
    double beta2;
    WordRule words;
};

struct RefWords {
    uint32_t w[kMaxRefs][kMaxLen + 4];      // compacted words, kNone from W on
    int W[kMaxRefs];
    int ptrs[kMaxRefs];                     // distinct pointer ids first seen in reference m
    float reward[kMaxLen];                  // SCST layout: the image's rewards, for the advantages
};

__device__ __forceinline__ int wave_count(int v) { return (int)wave_sum((float)v); }     // lane values sum to <= 64: exact

// Longest common subsequence of the candidate (words in the lanes of cw, c of them) and a reference whose words sit one
// per lane in rw (Wr of them).  Every operand of the recurrence is wave-uniform.
__device__ __forceinline__ int lcs_bits(uint32_t cw, int c, uint32_t rw, int Wr) {
    const int lane = threadIdx.x & 63;
    unsigned long long V = ~0ull;
    for (int i = 0; i < c; ++i) {
        const unsigned long long Mi = __ballot(lane < Wr && rw == lane_u32(cw, i));
        const unsigned long long U = V & Mi;
        V = (V + U) | (V - U);
    }
    const unsigned long long mask = Wr >= 64 ? ~0ull : ((1ull << Wr) - 1ull);
    return __popcll(~V & mask);
}

__global__ __launch_bounds__(kMaxWaves * 64) void metrics_kernel(MetricArgs a) {
    __shared__ RefWords L;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, waves = blockDim.x >> 6;
    const bool general = a.mode == 0;
    const int img = general ? a.image_index[blockIdx.x] : (int)blockIdx.x;
    const bool bad = img < 0 || img >= a.B;                 // general mode: an index outside the reference block
    const int rows = general ? 1 : a.rows_per_img;
    const bool ptr_on = a.pointer_base >= 0;
    const uint32_t pbase = (uint32_t)max(a.pointer_base, 0);
    if (!bad) {
        for (int m = wave; m < a.M; m += waves) {
            int W;
            const uint32_t w = compact_words(a.words, a.refs + ((int64_t)img * a.M + m) * a.Lr, a.Lr, W);
            L.w[m][lane] = w;
            if (lane < 4) L.w[m][kMaxLen + lane] = kNone;
            if (lane == 0) L.W[m] = W;
        }
    }
    __syncthreads();
    int ref_ptrs = 0;
    if (!bad && ptr_on) {
        for (int m = wave; m < a.M; m += waves) {
            const uint32_t w = L.w[m][lane];
            const bool is_ptr = lane < L.W[m] && w >= pbase;
            bool dup = false;
            for (int mm = 0; mm <= m; ++mm) {
                const int Wm = L.W[mm];
                for (int j = 0; j < Wm; ++j) dup = dup || (w == L.w[mm][j] && (mm < m || j < lane));
            }
            const int cnt = __popcll(__ballot(is_ptr && !dup));
            if (lane == 0) L.ptrs[m] = cnt;
        }
        __syncthreads();                                    // (uniform: bad and ptr_on are the same in every thread)
        for (int m = 0; m < a.M; ++m) ref_ptrs += L.ptrs[m];
    }
    for (int r = wave; r < rows; r += waves) {
        const int64_t row = general ? (int64_t)blockIdx.x : (r < a.n ? (int64_t)img * a.n + r : (int64_t)a.B * a.n + img);
        int cnt[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        int ptr[3] = {0, 0, 0};
        const float nan = __builtin_nanf("");
        float bleu[4] = {nan, nan, nan, nan};
        float rouge = nan, reward = nan;
        if (!bad) {
            uint32_t w[4];
            int c;
            w[0] = compact_words(a.words, a.cand + row * a.T, a.T, c);
            following_words(w, c);
            int tf[4];
            bool first[4];
            row_ngram_counts(w, c, tf, first);
            int best[4] = {0, 0, 0, 0};                     // max over m of count_m
            int lcs_max = 0, reflen = 0;
            double rec = 0.0;
            for (int m = 0; m < a.M; ++m) {
                const int Wr = L.W[m];
                int cm[4] = {0, 0, 0, 0};
                for (int j = 0; j < Wr; ++j) {
                    const bool e1 = w[0] == L.w[m][j];
                    const bool e2 = e1 && w[1] == L.w[m][j + 1];
                    const bool e3 = e2 && w[2] == L.w[m][j + 2];
                    const bool e4 = e3 && w[3] == L.w[m][j + 3];
                    cm[0] += e1; cm[1] += e2; cm[2] += e3; cm[3] += e4;
                }
#pragma unroll
                for (int s = 0; s < 4; ++s) best[s] = max(best[s], cm[s]);
                const int lcs = lcs_bits(w[0], c, L.w[m][lane], Wr);
                lcs_max = max(lcs_max, lcs);
                if (Wr > 0) rec = fmax(rec, (double)lcs / (double)Wr);
                // the closest reference length: minimise (|l_m - c|, l_m)
                const int d = abs(Wr - c), d0 = abs(reflen - c);
                if (m == 0 || d < d0 || (d == d0 && Wr < reflen)) reflen = Wr;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool own = lane + s < c && first[s];
                cnt[s] = max(0, c - s);
                cnt[4 + s] = wave_count(own ? min(tf[s], best[s]) : 0);
            }
            cnt[8] = c;
            cnt[9] = reflen;
            if (ptr_on) {
                const bool own_ptr = lane < c && first[0] && w[0] >= pbase;
                ptr[0] = __popcll(__ballot(own_ptr && best[0] > 0));
                ptr[1] = __popcll(__ballot(own_ptr));
                ptr[2] = ref_ptrs;
            }
            // sentence scores (uniform values; float64, rounded once)
            double p = 1.0, bp = 1.0;
            const double ratio = ((double)c + 1e-15) / ((double)reflen + 1e-9);
            if (ratio < 1.0) bp = exp(1.0 - 1.0 / ratio);
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                p *= ((double)cnt[4 + s] + 1e-15) / ((double)cnt[s] + 1e-9);
                bleu[s] = (float)(pow(p, 1.0 / (double)(s + 1)) * bp);
            }
            const double prec = c > 0 ? (double)lcs_max / (double)c : 0.0;
            rouge = prec > 0.0 && rec > 0.0 ? (float)((1.0 + a.beta2) * prec * rec / (rec + a.beta2 * prec)) : 0.f;
            if (a.rewards) {
                // w_base * base + w_b1 * bleu1 + .. + w_rouge * rouge, in this order; without base no first term
                reward = a.w[1] * bleu[0];
                if (a.base) reward = a.w[0] * a.base[row] + reward;
                reward = reward + a.w[2] * bleu[1];
                reward = reward + a.w[3] * bleu[2];
                reward = reward + a.w[4] * bleu[3];
                reward = reward + a.w[5] * rouge;
            }
        }
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 10; ++k) a.counts[row * 10 + k] = cnt[k];
#pragma unroll
            for (int k = 0; k < 4; ++k) a.bleu[row * 4 + k] = bleu[k];
            a.rouge[row] = rouge;
#pragma unroll
            for (int k = 0; k < 3; ++k) a.pointers[row * 3 + k] = ptr[k];
            if (a.rewards) {
                a.rewards[row] = reward;
                if (!general) L.reward[r] = reward;
            }
        }
    }
    if (general || a.rewards == nullptr) return;
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

// Totals of N rows, one workgroup: thread t adds rows t, t + 256, .. in that order; thread k < 14 then adds the 256
// partial sums of column k in thread order (13 sums and the row count) and thread 14 those of the ROUGE-L sum (float64).
// Rows whose ROUGE-L is NaN are skipped.
constexpr int kSumThreads = 256;

__global__ __launch_bounds__(kSumThreads) void metric_sums_kernel(const int32_t* counts, const float* rouge,
                                                                  const int32_t* pointers, int N, int64_t* sums,
                                                                  double* rouge_sum, int64_t* captions) {
    __shared__ int64_t part[14][kSumThreads];
    __shared__ double rpart[kSumThreads];
    const int t = threadIdx.x;
    int64_t s[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) s[k] = 0;
    double rs = 0.0;
    for (int i = t; i < N; i += kSumThreads) {
        const float r = rouge[i];
        if (r != r) continue;
#pragma unroll
        for (int k = 0; k < 10; ++k) s[k] += counts[(int64_t)i * 10 + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) s[10 + k] += pointers[(int64_t)i * 3 + k];
        s[13] += 1;
        rs += (double)r;
    }
#pragma unroll
    for (int k = 0; k < 14; ++k) part[k][t] = s[k];
    rpart[t] = rs;
    __syncthreads();
    if (t < 14) {
        int64_t tot = 0;
        for (int k = 0; k < kSumThreads; ++k) tot += part[t][k];
        if (t < 13) sums[t] = tot; else captions[0] = tot;
    } else if (t == 14) {
        double tot = 0.0;
        for (int k = 0; k < kSumThreads; ++k) tot += rpart[k];
        rouge_sum[0] = tot;
    }
}

}  // namespace
}  // namespace ick

extern "C" int ick_caption_metrics(const int64_t* cand, int32_t N, int32_t T, const int64_t* refs, int32_t B, int32_t M,
                                   int32_t Lr, int32_t start_token, int32_t end_token, int32_t pad_token,
                                   const int32_t* ignore, int32_t n_ignore, int32_t pointer_base, double beta, int32_t mode,
                                   const int32_t* image_index, int32_t num_samples, const float* base_rewards,
                                   const float* weights, int32_t* counts, float* bleu, float* rouge_l, int32_t* pointers,
                                   float* rewards, float* advantages, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(cand && refs && counts && bleu && rouge_l && pointers);
    ICK_CHECK_ARG(N > 0 && T > 0 && T <= kMaxLen && B > 0 && M > 0 && M <= kMaxRefs && Lr > 0 && Lr <= kMaxLen);
    ICK_CHECK_ARG(beta > 0.0 && beta < 1.0e18);
    ICK_CHECK_ARG(n_ignore >= 0 && n_ignore <= kMaxIgnore && (n_ignore == 0 || ignore));
    ICK_CHECK_ARG(mode >= 0 && mode <= 2);
    ICK_CHECK_ARG((rewards != nullptr) == (weights != nullptr) && (base_rewards == nullptr || rewards != nullptr));
    MetricArgs a{};
    a.cand = cand; a.refs = refs; a.image_index = image_index; a.base = base_rewards;
    a.counts = counts; a.bleu = bleu; a.rouge = rouge_l; a.pointers = pointers; a.rewards = rewards; a.adv = advantages;
    a.N = N; a.T = T; a.B = B; a.M = M; a.Lr = Lr; a.mode = mode; a.n = num_samples;
    a.pointer_base = pointer_base < 0 ? -1 : pointer_base;
    a.beta2 = beta * beta;
    if (weights)
        for (int k = 0; k < 6; ++k) {
            ICK_CHECK_ARG(weights[k] > -3.0e38f && weights[k] < 3.0e38f);
            a.w[k] = weights[k];
        }
    a.words.start = start_token; a.words.end = end_token; a.words.pad = pad_token; a.words.n_ignore = n_ignore;
    for (int k = 0; k < n_ignore; ++k) a.words.ignore[k] = ignore[k];
    int grid, rows;
    if (mode == 0) {
        ICK_CHECK_ARG(image_index);
        grid = N;
        rows = 1;
    } else {
        ICK_CHECK_ARG(num_samples >= 1 && (mode == 1 || num_samples >= 2) && (rewards == nullptr) == (advantages == nullptr));
        rows = num_samples + (mode == 1 ? 1 : 0);
        ICK_CHECK_ARG(rows <= kMaxLen && (int64_t)B * rows == (int64_t)N);
        grid = B;
    }
    a.rows_per_img = rows;
    const int waves = max(1, min(kMaxWaves, max(M, rows)));
    hipLaunchKernelGGL(metrics_kernel, dim3(grid), dim3(waves * 64), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}

extern "C" int ick_caption_metric_sums(const int32_t* counts, const float* rouge_l, const int32_t* pointers, int32_t N,
                                       int64_t* sums, double* rouge_sum, int64_t* captions, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(counts && rouge_l && pointers && sums && rouge_sum && captions && N > 0);
    hipLaunchKernelGGL(metric_sums_kernel, dim3(1), dim3(kSumThreads), 0, (hipStream_t)stream, counts, rouge_l, pointers,
                       N, sums, rouge_sum, captions);
    ICK_LAUNCH_RET();
}
