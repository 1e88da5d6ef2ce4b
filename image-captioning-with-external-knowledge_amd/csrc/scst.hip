// Self-critical sequence training (SelfCriticalStep, scst.py): sampled captions back into teacher-forced training rows.
//
// ick_samples_to_captions turns the sampler's token rows (R, T) into the captions / caption_masks / caption_lengths of a
// training batch: [<start>, w_1 .. w_m, <end>, <pad> ..] of length m + 2, or [<start>, w_1 .. w_T] (length T + 1) for a
// row that never drew <end>.  The mask of a position is predict()'s feedback rule (knowledge-aware/models.py:600-606):
// 2 for a fact token (w >= V + K, variants with facts), 1 for an entity token (w >= V), 0 for a word.
// One thread per row: R is a few hundred rows of ~20 tokens, the launch is a single short wave per 64 rows.
#include "common.h"

namespace ick {
namespace {

__global__ __launch_bounds__(64) void samples_to_captions_kernel(const int64_t* __restrict__ tokens, int R, int T, int V,
                                                                 int K, int has_facts, int start, int end, int pad,
                                                                 int64_t* __restrict__ captions,
                                                                 int64_t* __restrict__ masks,
                                                                 int64_t* __restrict__ lengths) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= R) return;
    const int64_t* tok = tokens + (int64_t)r * T;
    int64_t* cap = captions + (int64_t)r * (T + 1);
    int64_t* msk = masks + (int64_t)r * (T + 1);
    cap[0] = start;
    msk[0] = 0;
    int64_t len = T + 1;
    bool ended = false;
    for (int t = 0; t < T; ++t) {
        int64_t w = tok[t];
        if (ended) {
            w = pad;
        } else if (w == end) {
            ended = true;
            len = t + 2;
        }
        cap[t + 1] = w;
        msk[t + 1] = ended ? 0 : token_kind(w, V, K, has_facts);
    }
    lengths[r] = len;
}

}  // namespace
}  // namespace ick

extern "C" int ick_samples_to_captions(const int64_t* tokens, int32_t R, int32_t T, int32_t V, int32_t K,
                                       int32_t has_facts, int32_t start_token, int32_t end_token, int32_t pad_token,
                                       int64_t* captions, int64_t* masks, int64_t* lengths, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(tokens && captions && masks && lengths);
    ICK_CHECK_ARG(R > 0 && T > 0 && T < INT32_MAX && V > 0 && K >= 0);
    hipLaunchKernelGGL(samples_to_captions_kernel, dim3(ceil_div(R, 64)), dim3(64), 0, (hipStream_t)stream, tokens, R, T,
                       V, K, has_facts, start_token, end_token, pad_token, captions, masks, lengths);
    ICK_LAUNCH_RET();
}
