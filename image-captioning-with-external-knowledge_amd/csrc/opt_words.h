// The optimizer words and the learning-rate schedule of ick_adam_step / ick_adam_step_derive (include/ick_amd.h, DESIGN.md
// 3.1h): what the three Adam kernels share when they are instantiated with kOpt, which words != NULL selects.
#pragma once
#include "common.h"

namespace ick {

constexpr int kWordBaseLr = 0, kWordMaxNorm = 1, kWordNorm = 2, kWordCoef = 3, kWordLrNow = 4, kWordSqSum = 5;

inline bool lr_schedule_ok(const ick_lr_schedule& s) {
    if (s.warmup < 0 || !(s.min_ratio >= 0.f && s.min_ratio <= 1.f)) return false;
    switch (s.kind) {
        case ICK_LR_CONSTANT: return true;
        case ICK_LR_INVERSE_SQRT: return s.warmup >= 1;
        case ICK_LR_COSINE:
        case ICK_LR_LINEAR: return s.total > s.warmup;
        default: return false;
    }
}

// The rate of the 1-based step t (an integer held in a float, as the Adam kernels' bias correction has it).  A constant
// schedule without warmup returns `base` itself, so the step size is then the float words == NULL gets from lr.
__device__ __forceinline__ float lr_schedule(float base, const ick_lr_schedule s, float t) {
    const float W = (float)s.warmup;
    if (s.kind == ICK_LR_INVERSE_SQRT) return base * fminf(t / W, sqrtf(W / t));
    if (t < W) return base * (t / W);                   // the linear warmup of the three other kinds
    if (s.kind == ICK_LR_CONSTANT) return base;
    const float N = (float)s.total, r = s.min_ratio;
    const float tt = fminf(t, N);
    if (s.kind == ICK_LR_COSINE) return base * (r + (1.f - r) * (0.5f * (1.f + cospif((tt - W) / (N - W)))));
    return base * (r + (1.f - r) * ((N - tt) / (N - W)));
}

}  // namespace ick
