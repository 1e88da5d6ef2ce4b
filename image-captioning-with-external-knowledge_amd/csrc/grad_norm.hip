// The global L2 norm of the gradient bucket and the coefficient of torch.nn.utils.clip_grad_norm_ (norm_type 2) from it
// (ick_grad_sqnorm, include/ick_amd.h).  One read of the bucket, the only memory pass the clip adds to a
// training step: the Adam kernels multiply by the coefficient in the pass they make anyway.
//
// Two launches, no atomics, one order of additions whatever the mode:
//   partial   <= kMaxWg workgroups, each a grid-stride loop over trips of 1024 float4 (four per thread, every load issued
//             before its first use, as the flat-run branch of adam_derive_kernel); a thread adds its squares in the order
//             it loaded them, the workgroup's 256 sums fold in an LDS tree, scratch[workgroup] gets the result.  Thread 0
//             of workgroup 0 also takes the n % 4 floats behind the last float4.
//   finalise  one workgroup: thread i adds scratch[i], scratch[i + 256], ... in that order, the same LDS tree, and thread
//             0 writes the sum of squares, the norm and the coefficient into the optimizer words.
// Both return at once while the token count word is not > 0 (no pending gradients: the Adam kernels' rule).
#include <algorithm>

#include "opt_words.h"

namespace ick {
namespace {

constexpr int kMaxWg = 1024;          // 4 workgroups on each of the 256 CUs
constexpr int kTrip4 = 1024;          // float4 one workgroup takes per trip

// s[256] -> s[0], pairs (i, i + o) for o = 128, 64, .. 1: the order is a function of the thread index alone
__device__ __forceinline__ float tree_sum_256(float v, float* s) {
    const int tid = threadIdx.x;
    s[tid] = v;
    __syncthreads();
#pragma unroll
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    return s[0];
}

__global__ __launch_bounds__(256) void grad_sqnorm_partial_kernel(const float* __restrict__ g, int64_t n,
                                                                  const float* __restrict__ gscale_den,
                                                                  float* __restrict__ scratch) {
    __shared__ float s[256];
    if (gscale_den && !(gscale_den[0] > 0.f)) return;
    const float4* g4 = reinterpret_cast<const float4*>(g);
    const int64_t n4 = n / 4;
    const int tid = threadIdx.x;
    float acc = 0.f;
    for (int64_t base = (int64_t)blockIdx.x * kTrip4; base < n4; base += (int64_t)gridDim.x * kTrip4) {
        float4 x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int64_t j = base + tid + 256 * i;
            x[i] = j < n4 ? g4[j] : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) acc += (x[i].x * x[i].x + x[i].y * x[i].y) + (x[i].z * x[i].z + x[i].w * x[i].w);
    }
    if (blockIdx.x == 0 && tid == 0)
        for (int64_t i = 4 * n4; i < n; ++i) acc += g[i] * g[i];
    const float total = tree_sum_256(acc, s);
    if (tid == 0) scratch[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void grad_sqnorm_finalise_kernel(const float* __restrict__ scratch, int n_partials,
                                                                   float gscale, const float* __restrict__ gscale_den,
                                                                   float* __restrict__ words) {
    __shared__ float s[256];
    if (gscale_den) {
        if (!(gscale_den[0] > 0.f)) return;
        gscale = gscale / gscale_den[0];            // the Adam kernels' scale, the same float
    }
    float acc = 0.f;
    for (int i = threadIdx.x; i < n_partials; i += 256) acc += scratch[i];
    const float sq = tree_sum_256(acc, s);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(sq) * fabsf(gscale);
        const float max_norm = words[kWordMaxNorm];
        float coef = 1.f;
        if (max_norm > 0.f) {
            const float c = max_norm / (norm + 1e-6f);
            coef = c >= 1.f ? 1.f : c;              // clamp(c, max = 1) that lets a NaN through, as torch's does
        }
        words[kWordNorm] = norm;
        words[kWordCoef] = coef;
        words[kWordSqSum] = sq;
    }
}

int plan_workgroups(int64_t n) { return (int)std::min<int64_t>(std::max<int64_t>(ceil_div(n / 4, kTrip4), 1), kMaxWg); }

}  // namespace
}  // namespace ick

extern "C" int ick_grad_sqnorm_plan(int64_t n, int32_t* plan) {
    using namespace ick;
    ICK_CHECK_ARG(n > 0 && plan != nullptr);
    plan[0] = plan_workgroups(n);
    plan[1] = 4 * kTrip4;
    plan[2] = kMaxWg;
    return ICK_OK;
}

extern "C" int ick_grad_sqnorm(const float* g, int64_t n, float gscale, const float* gscale_den, float* scratch,
                               int64_t scratch_floats, float* words, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(g && scratch && words && n > 0 && scratch_floats >= kMaxWg);
    if ((reinterpret_cast<uintptr_t>(g) & 15) != 0) return ICK_EALIGN;
    const int wg = plan_workgroups(n);
    hipLaunchKernelGGL(grad_sqnorm_partial_kernel, dim3(wg), dim3(256), 0, (hipStream_t)stream, g, n, gscale_den, scratch);
    hipLaunchKernelGGL(grad_sqnorm_finalise_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scratch, wg, gscale,
                       gscale_den, words);
    ICK_LAUNCH_RET();
}
