// Philox-4x32-10 (Salmon et al. 2011), the counter-based generator of the sampled selection (sample.hip) and of the
// random-entity baseline of the geo-reference counts (geo_metric.hip): a pure function of (counter, key).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ick {

__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// The Gumbel noise of a 32-bit draw x (Gumbel-max sampling: sample.hip, sched_sample.hip): -log(-log(u)) in fp32 with the
// accurate logf, u = min(fl32((x >> 8) + 0.5) * 2^-24, 1 - 2^-24).
__device__ __forceinline__ float gumbel(uint32_t x) {
    float u = ((float)(x >> 8) + 0.5f) * 0x1p-24f;
    u = fminf(u, 0x1.fffffep-1f);
    return -logf(-logf(u));
}

}  // namespace ick
