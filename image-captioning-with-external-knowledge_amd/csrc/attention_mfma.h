// Matrix-core attention kernels (attention_mfma.hip); ick_attention / ick_attention_bwd try them first and
// fall back to the general kernels of attention.hip for shapes / layouts they do not cover.
#pragma once
#include "common.h"

namespace ick {

constexpr int kAttnMfmaUnsupported = -1000;   // not an error: "use the general kernel"

bool attn_mfma_shape_ok(int T, int S, int dh);
// the (NQT, MAXT) instantiation both launchers pick for a shape attn_mfma_shape_ok accepts: query tiles of 16, key
// tiles per wave
int attn_mfma_nqt(int T);
int attn_mfma_maxt(int S);
// Q / K / V in the head-major padded layout of ick_gemm's head-split epilogue: rows of DHP floats, every row 16-byte
// aligned (what the matrix-core kernels, the general backward and the general forward's float4 form read)
template <class Args>
inline bool attn_head_major(const Args& a, int DHP) {
    auto al16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
    return a.q_ts == DHP && a.k_ss == DHP && a.v_ss == DHP && al16(a.Q) && al16(a.K) && al16(a.V) && a.q_bs % 4 == 0 &&
           a.q_hs % 4 == 0 && a.k_bs % 4 == 0 && a.k_hs % 4 == 0 && a.v_bs % 4 == 0 && a.v_hs % 4 == 0;
}
int launch_attn_mfma(const ick_attn_args& a, hipStream_t s);
int launch_attn_bwd_mfma(const ick_attn_bwd_args& a, hipStream_t s);

}  // namespace ick
