// The weight and bias gradient of Encoder.conv1 (1x1 convolution) straight from the NCHW feature map
// (ick_conv1_wgrad, include/ick_amd.h):
//     dW[o, c] = sum over b, p of d_img[b, p, o] * feats[b, c, p],     db[o] = sum over b, p of d_img[b, p, o].
//
// As a GEMM this is M = d, N = C, K = B * P.  Over the flat reduction index kk = b * P + p the A operand (d_img) is ONE
// row-major (K, d) matrix; only feats jumps between samples (address (b * C + c) * P + p), which ick_gemm cannot express
// for an operand whose k runs along the row.  So the kernel walks kk in chunks of kKC and splits (b, p) per load.
//
//   partial   grid (column tiles of kBN = 64, groups of chunks, row blocks of 16 * MT).  A workgroup of four waves holds the
//             whole row block for its 64 columns: wave w owns columns [16 w, 16 w + 16) and MT accumulator tiles of the
//             exact fp32 v_mfma_f32_16x16x4_f32.  Per chunk the (kKC, 16 MT) slice of d_img and the (64, kKC) slice of
//             feats go global -> registers -> LDS, the loads of chunk i + 1 issued before the products of chunk i.
//             feats is read by one workgroup only (once from HBM when d fits one row block); d_img is re-read by the
//             column tiles, out of L2.  The group's result goes to scratch[group]; the workgroups of column tile 0
//             also add the column sums of their d_img slices (the bias gradient) from the tile in LDS.
//   finalise  dW[i] = scratch[0][i] + scratch[1][i] + ... in that order, db likewise.
// No atomics: one order of additions whatever the mode, so the result has the same bits on every run.  dW and db are
// OVERWRITTEN.
//
// Fast loads need 16-byte alignment: d % 4 == 0 and an aligned d_img for the A slices, P % 4 == 0 and an aligned feats
// for the B slices (a float4 of four consecutive kk then lies inside one sample).  Every other case takes the scalar
// form of the same loads (template switches), so any B, C, P, d >= 1 is served by the one entry point.
#include <algorithm>

#include "common.h"

namespace ick {
namespace {

constexpr int kKC = 32;               // reduction indices per chunk
constexpr int kBN = 64;               // columns (input channels) per workgroup: 16 per wave
constexpr int kLDB = kKC + 4;         // LDS row stride of the feats tile (floats; 16-byte multiple)
constexpr int kTargetWg = 512;        // two workgroups on each of the 256 CUs
constexpr int kMaxGroups = 64;

template <int MT>
struct Tile {
    static constexpr int MP = 16 * MT;            // rows (output channels) of one row block
    static constexpr int LDA = MP + 4;            // == 4 mod 16: the four k rows a wave reads at once hit 64 distinct banks
    static constexpr int AR = kKC / 4;            // d_img rows one wave loads per chunk
    static constexpr int ACV = (MP / 4 + 63) / 64;   // float4 per lane and row
    static constexpr int ACS = (MP + 63) / 64;       // floats per lane and row (scalar form)
    static constexpr int DBN = (MP + 255) / 256;     // bias-gradient columns per thread
};

template <int MT, bool VA, bool VB>
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ dimg, const float* __restrict__ feats,
                                                          float* __restrict__ part_w, float* __restrict__ part_b, int C,
                                                          int P, int d, int K, int cpg) {
    using T = Tile<MT>;
    __shared__ __attribute__((aligned(16))) float As[kKC * T::LDA];
    __shared__ __attribute__((aligned(16))) float Bs[kBN * kLDB];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int fi = lane & 15, kq = lane >> 4;
    const int c0 = blockIdx.x * kBN, g = blockIdx.y, m0 = blockIdx.z * T::MP;
    const int md = min(d - m0, T::MP);                       // valid rows of this block
    const int k_begin = g * cpg * kKC, k_end = min(K, k_begin + cpg * kKC);
    const bool want_db = blockIdx.x == 0;

    float4 ra4[VA ? T::AR : 1][VA ? T::ACV : 1];
    float ra1[VA ? 1 : T::AR][VA ? 1 : T::ACS];
    float4 rb4[2];
    float rb1[8];

    auto load = [&](int kk0) {
#pragma unroll
        for (int r = 0; r < T::AR; ++r) {
            const int kk = kk0 + 4 * r + wave;
            const float* row = dimg + (int64_t)kk * d + m0;
            if constexpr (VA) {
#pragma unroll
                for (int i = 0; i < T::ACV; ++i) {
                    const int c = 4 * (lane + 64 * i);
                    ra4[r][i] = (kk < k_end && c < md) ? *reinterpret_cast<const float4*>(row + c)
                                                       : make_float4(0.f, 0.f, 0.f, 0.f);
                }
            } else {
#pragma unroll
                for (int i = 0; i < T::ACS; ++i) {
                    const int c = lane + 64 * i;
                    ra1[r][i] = (kk < k_end && c < md) ? row[c] : 0.f;
                }
            }
        }
        if constexpr (VB) {
            const int kk = kk0 + 4 * (tid & 7);
            const int b = kk / P, p = kk - b * P;
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = c0 + (tid >> 3) + 32 * i;
                rb4[i] = (kk < k_end && c < C) ? *reinterpret_cast<const float4*>(feats + ((int64_t)b * C + c) * P + p)
                                               : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        } else {
            const int kk = kk0 + (tid & 31);
            const int b = kk / P, p = kk - b * P;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int c = c0 + (tid >> 5) + 8 * i;
                rb1[i] = (kk < k_end && c < C) ? feats[((int64_t)b * C + c) * P + p] : 0.f;
            }
        }
    };
    auto store = [&]() {
#pragma unroll
        for (int r = 0; r < T::AR; ++r) {
            float* row = As + (4 * r + wave) * T::LDA;
            if constexpr (VA) {
#pragma unroll
                for (int i = 0; i < T::ACV; ++i) {
                    const int c = 4 * (lane + 64 * i);
                    if (c < T::MP) *reinterpret_cast<float4*>(row + c) = ra4[r][i];
                }
            } else {
#pragma unroll
                for (int i = 0; i < T::ACS; ++i) {
                    const int c = lane + 64 * i;
                    if (c < T::MP) row[c] = ra1[r][i];
                }
            }
        }
        if constexpr (VB) {
#pragma unroll
            for (int i = 0; i < 2; ++i)
                *reinterpret_cast<float4*>(Bs + ((tid >> 3) + 32 * i) * kLDB + 4 * (tid & 7)) = rb4[i];
        } else {
#pragma unroll
            for (int i = 0; i < 8; ++i) Bs[((tid >> 5) + 8 * i) * kLDB + (tid & 31)] = rb1[i];
        }
    };

    f32x4 acc[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[mt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float dbacc[T::DBN];
#pragma unroll
    for (int i = 0; i < T::DBN; ++i) dbacc[i] = 0.f;

    load(k_begin);
    for (int kk0 = k_begin; kk0 < k_end; kk0 += kKC) {
        store();
        __syncthreads();
        if (kk0 + kKC < k_end) load(kk0 + kKC);
        // within a block of 16 reduction indices lane group kq and step u stand for index 4 kq + u, in both operands
#pragma unroll
        for (int ks = 0; ks < kKC / 16; ++ks) {
            const float4 bq = *reinterpret_cast<const float4*>(Bs + (wave * 16 + fi) * kLDB + ks * 16 + 4 * kq);
            const float* ap = As + (ks * 16 + 4 * kq) * T::LDA + fi;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[mt * 16], bq.x, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[mt * 16 + T::LDA], bq.y, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[mt * 16 + 2 * T::LDA], bq.z, acc[mt], 0, 0, 0);
                acc[mt] = __builtin_amdgcn_mfma_f32_16x16x4f32(ap[mt * 16 + 3 * T::LDA], bq.w, acc[mt], 0, 0, 0);
            }
        }
        if (want_db) {                                        // uniform over the workgroup
#pragma unroll
            for (int i = 0; i < T::DBN; ++i) {
                const int o = tid + 256 * i;
                if (o < md)
                    for (int k = 0; k < kKC; ++k) dbacc[i] += As[k * T::LDA + o];
            }
        }
        __syncthreads();
    }

    // C/D map of the 16x16 MFMA: column = lane & 15, row = (lane >> 4) * 4 + register
    float* out = part_w + (int64_t)g * d * C;
    const int c = c0 + wave * 16 + fi;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int o = mt * 16 + 4 * kq + r;
            if (o < md && c < C) out[(int64_t)(m0 + o) * C + c] = acc[mt][r];
        }
    if (want_db) {
#pragma unroll
        for (int i = 0; i < T::DBN; ++i) {
            const int o = tid + 256 * i;
            if (o < md) part_b[(int64_t)g * d + m0 + o] = dbacc[i];
        }
    }
}

__global__ __launch_bounds__(256) void conv1_wgrad_finalise_kernel(const float* __restrict__ part_w,
                                                                   const float* __restrict__ part_b, int groups,
                                                                   int64_t nw, int d, float* __restrict__ dw,
                                                                   float* __restrict__ db) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nw) {
        float s = part_w[i];
        for (int g = 1; g < groups; ++g) s += part_w[g * nw + i];
        dw[i] = s;
    } else if (i < nw + d) {
        const int64_t o = i - nw;
        float s = part_b[o];
        for (int g = 1; g < groups; ++g) s += part_b[(int64_t)g * d + o];
        db[o] = s;
    }
}

struct Plan {
    int mt, row_blocks, col_tiles, groups, cpg;
    int64_t scratch;
};

Plan make_plan(int64_t K, int C, int d) {
    Plan p;
    p.mt = d <= 64 ? 4 : (d <= 160 ? 10 : 19);
    p.row_blocks = ceil_div(d, 16 * p.mt);
    p.col_tiles = ceil_div(C, kBN);
    const int chunks = ceil_div(K, kKC);
    const int tiles = p.row_blocks * p.col_tiles;
    const int want = std::min(std::min(std::max(ceil_div(kTargetWg, tiles), 1), kMaxGroups), chunks);
    p.cpg = ceil_div(chunks, want);
    p.groups = ceil_div(chunks, p.cpg);       // no empty group
    p.scratch = (int64_t)p.groups * ((int64_t)d * C + d);
    return p;
}

template <int MT>
void launch(const Plan& p, bool va, bool vb, hipStream_t s, const float* dimg, const float* feats, float* pw, float* pb,
            int C, int P, int d, int K) {
    const dim3 grid(p.col_tiles, p.groups, p.row_blocks), block(256);
    if (va && vb) hipLaunchKernelGGL((conv1_wgrad_kernel<MT, true, true>), grid, block, 0, s, dimg, feats, pw, pb, C, P, d, K, p.cpg);
    else if (va) hipLaunchKernelGGL((conv1_wgrad_kernel<MT, true, false>), grid, block, 0, s, dimg, feats, pw, pb, C, P, d, K, p.cpg);
    else if (vb) hipLaunchKernelGGL((conv1_wgrad_kernel<MT, false, true>), grid, block, 0, s, dimg, feats, pw, pb, C, P, d, K, p.cpg);
    else hipLaunchKernelGGL((conv1_wgrad_kernel<MT, false, false>), grid, block, 0, s, dimg, feats, pw, pb, C, P, d, K, p.cpg);
}

bool sizes_ok(int B, int C, int P, int d) {
    // the chunk walk keeps kk + kKC and the grid's y / z extents inside their integer types
    return B > 0 && C > 0 && P > 0 && d > 0 && (int64_t)B * P <= (int64_t)0x7fffffff - 2 * kKC &&
           ceil_div(d, 16 * 19) <= 65535;
}

}  // namespace
}  // namespace ick

extern "C" int ick_conv1_wgrad_plan(int32_t B, int32_t C, int32_t P, int32_t d, int32_t* plan, int64_t* scratch_floats) {
    using namespace ick;
    ICK_CHECK_ARG(plan != nullptr && scratch_floats != nullptr && sizes_ok(B, C, P, d));
    const Plan p = make_plan((int64_t)B * P, C, d);
    plan[0] = p.groups;
    plan[1] = p.cpg * kKC;
    plan[2] = p.col_tiles;
    plan[3] = 16 * p.mt;
    *scratch_floats = p.scratch;
    return ICK_OK;
}

extern "C" int ick_conv1_wgrad(const float* d_img, const float* feats, float* dw, float* db, int32_t B, int32_t C,
                               int32_t P, int32_t d, float* scratch, int64_t scratch_floats, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(d_img && feats && dw && db && scratch && sizes_ok(B, C, P, d));
    const int K = B * P;
    const Plan p = make_plan(K, C, d);
    ICK_CHECK_ARG(scratch_floats >= p.scratch);
    const bool va = d % 4 == 0 && (reinterpret_cast<uintptr_t>(d_img) & 15) == 0;
    const bool vb = P % 4 == 0 && (reinterpret_cast<uintptr_t>(feats) & 15) == 0;
    float* pw = scratch;
    float* pb = scratch + (int64_t)p.groups * d * C;
    hipStream_t s = (hipStream_t)stream;
    if (p.mt == 4) launch<4>(p, va, vb, s, d_img, feats, pw, pb, C, P, d, K);
    else if (p.mt == 10) launch<10>(p, va, vb, s, d_img, feats, pw, pb, C, P, d, K);
    else launch<19>(p, va, vb, s, d_img, feats, pw, pb, C, P, d, K);
    const int64_t nw = (int64_t)d * C;
    hipLaunchKernelGGL(conv1_wgrad_finalise_kernel, dim3(ceil_div(nw + d, 256)), dim3(256), 0, s, pw, pb, p.groups, nw, d,
                       dw, db);
    ICK_LAUNCH_RET();
}
