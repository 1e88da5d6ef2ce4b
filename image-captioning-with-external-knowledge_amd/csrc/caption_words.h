// The words of a caption row, shared by the caption metrics on token ids (cider.hip: ick_cider_d; metrics.hip:
// ick_caption_metrics).  The rule is the one include/ick_amd.h states for ick_cider_d: the tokens before the first
// <end>, without <start>, <pad> and the ignored ids; removal closes the gap.
#pragma once
#include "common.h"

namespace ick {

constexpr uint32_t kNone = 0xFFFFFFFFu;     // an unused key slot / a position past a row's last word
constexpr int kMaxRefs = 16, kMaxLen = 64, kMaxIgnore = 16, kMaxWaves = 8;

struct WordRule {
    int start, end, pad, n_ignore;
    int ignore[kMaxIgnore];
};

__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// One row of `len` <= 64 tokens -> its words, compacted: lane i holds the row's i-th word (its low 32 bits), kNone from
// W (the word count, wave-uniform) on.  Wave-uniform call: every lane of the wave must be active.
__device__ __forceinline__ uint32_t compact_words(const WordRule& a, const int64_t* row, int len, int& W) {
    const int lane = threadIdx.x & 63;
    const int64_t t = lane < len ? row[lane] : (int64_t)a.end;
    const unsigned long long ends = __ballot(lane < len && t == a.end);
    const int e = ends ? __builtin_ctzll(ends) : len;
    bool keep = lane < e && t != a.start && t != a.pad;
    for (int k = 0; k < a.n_ignore; ++k) keep = keep && t != a.ignore[k];
    const unsigned long long km = __ballot(keep);
    W = __popcll(km);
    const int pos = __builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0));
    // compaction: kept lane -> its rank among kept lanes; the others after them in lane order (a permutation)
    const int target = keep ? pos : W + (lane - pos);
    uint32_t cw = (uint32_t)__builtin_amdgcn_ds_permute(target * 4, (int)(uint32_t)t);
    if (lane >= W) cw = kNone;
    return cw;
}

// Words i+1 .. i+3 beside word i (w[0] = compact_words' result): lane i then holds the four n-grams that start at the
// row's i-th word; kNone past the last word.
__device__ __forceinline__ void following_words(uint32_t (&w)[4], int W) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        const uint32_t o = (uint32_t)__builtin_amdgcn_ds_bpermute(((lane + k) & 63) * 4, (int)w[0]);
        w[k] = lane + k < W ? o : kNone;
    }
}

// Term frequencies and first occurrences inside the row: tf[s] = how many words of the row start the (s+1)-gram that
// starts at word `lane`, first[s] = no earlier word does (the lane is that n-gram's owner).  Equality of n-grams is the
// chain e1 = (w_i == w_j), e2 = e1 && (w_i+1 == w_j+1), ..  Lanes whose n-gram runs past the row compare kNone slots:
// the caller masks them with lane + s < W.
__device__ __forceinline__ void row_ngram_counts(const uint32_t (&w)[4], int W, int (&tf)[4], bool (&first)[4]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int s = 0; s < 4; ++s) { tf[s] = 0; first[s] = true; }
    for (int j = 0; j < W; ++j) {
        const bool e1 = w[0] == lane_u32(w[0], j);
        const bool e2 = e1 && w[1] == lane_u32(w[1], j);
        const bool e3 = e2 && w[2] == lane_u32(w[2], j);
        const bool e4 = e3 && w[3] == lane_u32(w[3], j);
        const bool eq[4] = {e1, e2, e3, e4};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            tf[s] += eq[s];
            if (j < lane && eq[s]) first[s] = false;
        }
    }
}

}  // namespace ick
