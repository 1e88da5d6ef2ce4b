// fp32 GEMM with split-bf16 products whose B operand (an nn.Linear / 1x1 conv weight) arrives PRE-SPLIT.
//
//   C[m, n] = epilogue( sum_k A(m,k) * B(n,k) ),   A fp32 activations,  B = hi + mid + lo bf16 planes (ick_presplit_weights)
//
// Call sites (include/ick_amd.h, ick_gemm with b_ps set): Encoder.conv1 (geo-aware/models.py:32,45), the cross K/V
// projection of the image rows and fc_vocab (geo-aware/models.py:241-242,303), and fc_vocab's data gradient.
//
// Why a kernel of its own (csrc/gemm.hip splits BOTH operands between the global load and the LDS store): there the
// split costs 5.5 VALU instructions per staged element and the vector issue port, not the matrix pipe, bounds the
// kernel.  A weight is the same for the whole step, so it is split once per step by the packing launch; what is left to
// split is the activation operand, and that is done on the 16 x 32 MFMA fragment a wave is about to use (8 elements per
// lane and slice).  Nothing is staged through registers any more:
//   * every tile slice travels global -> LDS by LDS-DMA (buffer_load_dwordx4 ... lds, 1 KiB per wave instruction): the
//     pre-split B planes in the MFMA operand's image (64-byte rows, XOR-swizzled chunks -- the swizzle is applied to
//     the SOURCE address, the LDS side of a DMA is lane-linear), the A tile as raw fp32;
//   * both operands run through two LDS buffers, one slice in flight ahead of the one being read; the only waits are
//     one s_waitcnt vmcnt(0) + one raw s_barrier per slice;
//   * a wave owns TM x 16 rows x (TN x 16) columns: it requests its B fragments (PF blocks ahead, or the whole slice),
//     reads its raw A fragment (k-major: eight ds_read_b32 from a line image rotated by 16 floats per 8 k lines;
//     k-contiguous: two ds_read_b128 from 128-byte rows with XOR-swizzled chunks -- both conflict free: PMC
//     SQ_LDS_BANK_CONFLICT = 0), splits it (44 VALU) and issues 6 x TM x TN v_mfma_f32_16x16x32_bf16;
//   * tile shapes: the three of the table above launch_gemm_ps below, all two workgroups per CU.  Measured
//     (profiles/r04_*_gemm_ps_tiles.txt, PMC profiles/r04_c_pmc_gemm_ps.txt): 128 x 128 is the fastest wherever the
//     output is wider than 320 columns (cross K/V 128 -> 100 us, vocabulary 76 -> 65 us against the stager-split
//     kernel).  Ring depth, fragment prefetch depth, tile size and non-temporal A loads all left the rate at 120-135
//     TFLOP/s fp32-equivalent with the matrix pipe ~50 % busy on the CUs in use -- about 60 % of what bf16 MFMA loops
//     hold on random data at the clock the chip keeps under that load (MI355X_MICROARCH.md, DVFS give-back: 1.25
//     PFLOP/s at 1.9 GHz, i.e. ~208 TFLOP/s fp32-equivalent).  The variants of those sweeps (eight more tile shapes,
//     ring depths 2 and 3) are no longer in the source: DESIGN.md section 3.1c.
#include <algorithm>

#include "gemm_common.h"

// Diagnostic build (-DICK_PS_STAMPS, tools/debug/gemm_ps_stamps.py): wave 0 of one workgroup in the middle of the grid sums
// the shader-clock ticks it spends in each phase of a slice.  Compiled out of the product library.
#ifdef ICK_PS_STAMPS
__device__ unsigned long long ick_ps_stamps[10];
#define ICK_PSTAMP(var)                                   \
    do {                                                  \
        __builtin_amdgcn_sched_barrier(0);                \
        var = __builtin_amdgcn_s_memtime();               \
        __builtin_amdgcn_sched_barrier(0);                \
    } while (0)
extern "C" int ick_debug_read_ps_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(ick_ps_stamps), sizeof(ick_ps_stamps));
}
#else
#define ICK_PSTAMP(var)
#endif

namespace ick {
namespace {

typedef __attribute__((address_space(3))) void* lds_void_ptr;

inline int64_t ps_rows(int N) { return (int64_t)ceil_div(N, 64) * 64; }
inline int64_t ps_bytes(int N, int K) { return (int64_t)ceil_div(K, 32) * 3 * ps_rows(N) * 64; }

// ---------------------------------------------------------------------------------------------------------------------
// Pre-split copies: dst[slice s][plane p][row n < Np][32 k] bf16, zero beyond N / K.
constexpr int kPsMaxItems = 16;
struct PsBatch {
    int count;
    int first[kPsMaxItems + 1];     // first workgroup of every item
    ick_presplit_item it[kPsMaxItems];
};

__global__ __launch_bounds__(256) void presplit_kernel(PsBatch b) {
    __shared__ float tile[64][33];
    int gi = 0;
    while (gi + 1 < b.count && (int)blockIdx.x >= b.first[gi + 1]) ++gi;
    const ick_presplit_item it = b.it[gi];
    const int local = blockIdx.x - b.first[gi];
    const int blocks_n = (it.N + 63) / 64;
    const int nb = local % blocks_n, s = local / blocks_n;
    const int t = threadIdx.x;
    const float* src = it.src;
    // columns that exist (device-side bound; uniform): slices past them are left alone, the last one is zero-padded
    const int Kr = device_bound(it.K, it.k_bound);
    if (32 * s >= Kr) return;
    // 32 contiguous source bytes per thread: two 16-byte loads where the view allows (the activation planes of the backward
    // pass -- memory^T, h^T -- are made inside the step: a dword per lane moves a quarter of what a dwordx4 does)
    const bool al16 = (reinterpret_cast<uintptr_t>(src) & 15) == 0;
    if (it.src_cs == 1) {                 // k contiguous: 8 consecutive k of one row per thread
        const int r = t >> 2, kk = (t & 3) * 8;
        const int n = nb * 64 + r;
        const int k0 = 32 * s + kk;
        if (al16 && (it.src_rs & 3) == 0 && n < it.N && k0 + 7 < Kr) {
            const float4* q = reinterpret_cast<const float4*>(src + (int64_t)n * it.src_rs + k0);
            const float4 a = q[0], b = q[1];
            tile[r][kk + 0] = a.x; tile[r][kk + 1] = a.y; tile[r][kk + 2] = a.z; tile[r][kk + 3] = a.w;
            tile[r][kk + 4] = b.x; tile[r][kk + 5] = b.y; tile[r][kk + 6] = b.z; tile[r][kk + 7] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int k = k0 + j;
                tile[r][kk + j] = (n < it.N && k < Kr) ? src[(int64_t)n * it.src_rs + k] : 0.f;
            }
        }
    } else {                              // rows contiguous (a transposed view): 8 consecutive rows at one k per thread
        const int kk = t >> 3, r0 = (t & 7) * 8;
        const int k = 32 * s + kk;
        const int n0 = nb * 64 + r0;
        // k_map: column k of the matrix is source column k_map[k] (activation rows gathered through a row list)
        const int ks = (it.k_map != nullptr && k < Kr) ? it.k_map[k] : k;
        if (al16 && it.src_rs == 1 && (it.src_cs & 3) == 0 && n0 + 7 < it.N && k < Kr) {
            const float4* q = reinterpret_cast<const float4*>(src + n0 + (int64_t)ks * it.src_cs);
            const float4 a = q[0], b = q[1];
            tile[r0 + 0][kk] = a.x; tile[r0 + 1][kk] = a.y; tile[r0 + 2][kk] = a.z; tile[r0 + 3][kk] = a.w;
            tile[r0 + 4][kk] = b.x; tile[r0 + 5][kk] = b.y; tile[r0 + 6][kk] = b.z; tile[r0 + 7][kk] = b.w;
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const int n = n0 + j;
                tile[n - nb * 64][kk] = (n < it.N && k < Kr) ? src[(int64_t)n * it.src_rs + (int64_t)ks * it.src_cs] : 0.f;
            }
        }
    }
    __syncthreads();
    const int r = t >> 2, c = t & 3;
    uint32_t h[4], m[4], l[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) split3(tile[r][8 * c + 2 * j], tile[r][8 * c + 2 * j + 1], h[j], m[j], l[j]);
    const int64_t np = (int64_t)blocks_n * 64;
    char* dst = reinterpret_cast<char*>(it.dst) + ((int64_t)s * 3 * np + nb * 64 + r) * 64 + c * 16;
    *reinterpret_cast<uint4*>(dst) = uint4{h[0], h[1], h[2], h[3]};
    *reinterpret_cast<uint4*>(dst + np * 64) = uint4{m[0], m[1], m[2], m[3]};
    *reinterpret_cast<uint4*>(dst + 2 * np * 64) = uint4{l[0], l[1], l[2], l[3]};
}

}  // namespace

// ---------------------------------------------------------------------------------------------------------------------
template <int WM_, int WN_, int TM_, int TN_, bool AKM_, int PF_>
struct PsCfg {
    static constexpr int WM = WM_, WN = WN_, TM = TM_, TN = TN_;
    static constexpr int PF = PF_ < TN_ ? PF_ : TN_;   // B fragment blocks requested from LDS ahead of the MFMAs that use them
    static constexpr int ST = 2;                        // LDS buffers per operand: the slice being read and the next one
    static constexpr bool AKM = AKM_;
    static constexpr int BM = WM * TM * 16, BN = WN * TN * 16, NW = WM * WN, NT = NW * 64;
    static constexpr int A_STAGE = BM * 32 * 4;          // bytes: raw fp32 slice of the A tile
    static constexpr int B_PLANE = BN * 64;              // bytes: one bf16 plane of the B tile slice
    static constexpr int B_STAGE = 3 * B_PLANE;
    static constexpr int NPA = BM / 8;                   // 1 KiB DMA pieces of an A slice
    static constexpr int NPB = 3 * BN / 16;              // ... of a B slice (16 rows of one plane each)
    static constexpr int PA_W = NPA / NW;                // pieces per wave
    static constexpr int PB_W = (NPB + NW - 1) / NW;
    static constexpr int LDS = ST * (A_STAGE + B_STAGE);
    static constexpr int WGS_PER_CU = 160 * 1024 / LDS;  // what the LDS footprint leaves room for
    // waves per SIMD the register allocator may plan for: those of the workgroups that share a CU, on its 4 SIMDs (4 for
    // the eight-wave tiles, 2 for the four-wave tile: 256 VGPRs each, enough to hold a whole slice's B fragments)
    static constexpr int WAVES_PER_EU = WGS_PER_CU * NW / 4;
    static_assert(NPA % NW == 0 && PA_W >= 1, "every wave issues the same number of A pieces");
    static_assert(LDS <= 160 * 1024, "tile exceeds the LDS of a CU");
};

#define ICK_WAIT_VMCNT0() asm volatile("s_waitcnt vmcnt(0)" ::: "memory")
// every wave is done reading the slice (its LDS reads have been consumed by MFMAs; the explicit wait covers reads the
// compiler may have left in flight) and its DMA pieces have landed: one barrier publishes both
#define ICK_LDS_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")

// One slice of the B tile / of the A tile by LDS-DMA: this wave's 1 KiB pieces (see the kernel below).
template <class C>
__device__ __forceinline__ void ps_dma_b(const __amdgpu_buffer_rsrc_t& rsrc, char* Bs, int buf, int wave,
                                         uint32_t bvoff, int slice, bool valid, int n0, int np_rows) {
#pragma unroll
    for (int j = 0; j < C::PB_W; ++j) {
        const int g = wave + C::NW * j;
        if (g < C::NPB) {               // wave-uniform
            const int plane = g / (C::BN / 16), rblk = g % (C::BN / 16);
            const bool in = valid && (n0 + rblk * 16 < np_rows);
            const uint32_t soff = (uint32_t)((((int64_t)slice * 3 + plane) * np_rows + rblk * 16) * 64);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lds_void_ptr)(Bs + buf * C::B_STAGE + plane * C::B_PLANE + rblk * 1024),
                                                     16, in ? bvoff : kOobOffset, in ? soff : 0u, 0, 0);
        }
    }
}
// nt: non-temporal loads.  Measured without gain and always false: launch_ps_cfg passes 0.  The
// kernel argument and this arm stay because the compiler schedules the K loop differently without them.
template <class C>
__device__ __forceinline__ void ps_dma_a(const __amdgpu_buffer_rsrc_t& rsrc, char* As, int buf, int wave,
                                         const uint32_t* avoff, const int* akl, int k0, int kend,
                                         uint32_t soff, bool nt) {
#pragma unroll
    for (int j = 0; j < C::PA_W; ++j) {
        const int g = wave + C::NW * j;
        const bool in = k0 + akl[j] < kend;      // also false for every lane of a slice beyond the K range
        lds_void_ptr dst = (lds_void_ptr)(As + buf * C::A_STAGE + g * 1024);
        if (nt) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, in ? avoff[j] : kOobOffset, soff, 0, 2);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, 16, in ? avoff[j] : kOobOffset, soff, 0, 0);
    }
}

// Piece `idx` of this wave's share of a slice (B pieces first, then A pieces): the kernel issues them one at a time BETWEEN
// its MFMAs.  (All eight waves issuing their pieces together right behind the barrier stalled every wave for ~700 cycles
// per slice: a CU's address unit takes one 1 KiB wave request per 16 cycles -- tools/debug/gemm_ps_stamps.py.)
template <class C>
__device__ __forceinline__ void ps_dma_piece(int idx, const __amdgpu_buffer_rsrc_t& rsrc_a, const __amdgpu_buffer_rsrc_t& rsrc_b,
                                             char* As, char* Bs, int buf, int wave, uint32_t bvoff,
                                             const uint32_t* avoff, const int* akl, int slice, bool valid,
                                             int n0, int np_rows, int k0, int kend, uint32_t soff_a) {
    if (idx < C::PB_W) {
        const int g = wave + C::NW * idx;
        if (g < C::NPB) {               // wave-uniform
            const int plane = g / (C::BN / 16), rblk = g % (C::BN / 16);
            const bool in = valid && (n0 + rblk * 16 < np_rows);
            const uint32_t soff = (uint32_t)((((int64_t)slice * 3 + plane) * np_rows + rblk * 16) * 64);
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_b, (lds_void_ptr)(Bs + buf * C::B_STAGE + plane * C::B_PLANE + rblk * 1024),
                                                     16, in ? bvoff : kOobOffset, in ? soff : 0u, 0, 0);
        }
    } else {
        const int j = idx - C::PB_W;
        const int g = wave + C::NW * j;
        const bool in = k0 + akl[j] < kend;
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc_a, (lds_void_ptr)(As + buf * C::A_STAGE + g * 1024), 16,
                                                 in ? avoff[j] : kOobOffset, soff_a, 0, 0);
    }
}

template <int WM_, int WN_, int TM_, int TN_, bool AKM_, int PF_>
__global__ __launch_bounds__(WM_ * WN_ * 64)
__attribute__((amdgpu_waves_per_eu(1, (PsCfg<WM_, WN_, TM_, TN_, AKM_, PF_>::WAVES_PER_EU)))) void gemm_ps_kernel(
    ick_gemm_args p, int np_rows, int64_t bps_bytes, int tiles_m, int tiles_n, int kchunk, int a_nt) {
    using C = PsCfg<WM_, WN_, TM_, TN_, AKM_, PF_>;
    constexpr int BM = C::BM, BN = C::BN, TM = C::TM, TN = C::TN, NW = C::NW, ST = C::ST;
    constexpr bool AKM = C::AKM;
    extern __shared__ __attribute__((aligned(1024))) char smem_ps[];
#ifdef ICK_PS_STAMPS
    unsigned long long t_start = 0, t_loop = 0, t_end = 0;
    ICK_PSTAMP(t_start);
    const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();      // 100 MHz: the shader clock this workgroup saw
#endif
    char* const As = smem_ps;
    char* const Bs = smem_ps + ST * C::A_STAGE;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    constexpr int WN = C::WN;
    const int wm = wave / WN, wn = wave % WN;
    const int fi = lane & 15, fq = lane >> 4;

    // tile of this workgroup: XCD-aware order (workgroups are dealt to the 8 XCDs round robin in linear order: b, b + 8, ...
    // share an XCD).  Without a K split each XCD walks a contiguous run of tiles.  With one, the (K slice, tile) pairs are
    // numbered slice-major and each XCD takes a contiguous run of THAT order: an XCD then streams only its own K range of
    // both operands (one to two slices) and the re-reads by the tiles of the grid hit its L2 -- with the tile-major order
    // every XCD read the whole K range of both operands (PMC: the vocabulary's data gradient moved 262 MB for ~70 MB of
    // operands, a cross K/V weight gradient ~400 MB for 59 MB).
    int bid = blockIdx.x;
    int zid = blockIdx.z;
    {
        const int nwg = tiles_m * tiles_n;
        if (gridDim.z > 1) {
            const int total = nwg * (int)gridDim.z, lin = bid + nwg * zid;
            const int xcd = lin & 7, qq = total >> 3, rr = total & 7;
            const int v = xcd * qq + min(xcd, rr) + (lin >> 3);
            zid = v / nwg;
            bid = v - zid * nwg;
        } else {
            const int xcd = bid & 7, qq = nwg >> 3, rr = nwg & 7;
            bid = (xcd < rr ? xcd * (qq + 1) : rr * (qq + 1) + (xcd - rr) * qq) + (bid >> 3);
        }
    }
    int tm, tn;
    if (tiles_m <= tiles_n) { tm = bid % tiles_m; tn = bid / tiles_m; }
    else { tn = bid % tiles_n; tm = bid / tiles_n; }
    const int m0 = tm * BM, n0 = tn * BN;
    // Device-side extents (m_bound / k_bound; uniform), as in csrc/gemm.hip: the K slices partition [0, K'), a tile at or
    // past a bound exits before any load.  (The pre-split copy of B is zero from K' to the end of its last slice.)
    const int Mr = device_bound(p.M, p.m_bound), Kr = device_bound(p.K, p.k_bound);
    if (p.k_bound != nullptr) kchunk = ((Kr + (int)gridDim.z - 1) / (int)gridDim.z + 31) / 32 * 32;
    const int kbeg = zid * kchunk;
    if (m0 >= Mr || kbeg >= Kr) return;
    const int kend = min(Kr, kbeg + kchunk);
    const int nk = (kend - kbeg + 31) >> 5;
    const int s0 = kbeg >> 5;

    // ---- A: per-lane source offsets of this wave's pieces (fixed for the whole K loop; the K position is the scalar offset)
    const __amdgpu_buffer_rsrc_t rsrc_a =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.A), (short)0, (int)(p.a_extent * 4), 0x00020000);
    const RowMap amap{p.a_grp, p.a_gs, p.a_gmap, p.a_rs};
    uint32_t avoff[C::PA_W];
    int akl[C::PA_W];                       // k (relative to the slice) of the lane's 16 bytes
#pragma unroll
    for (int j = 0; j < C::PA_W; ++j) {
        const int g = wave + NW * j;
        int row, extra;
        if constexpr (AKM) {
            constexpr int LPK = BM / 4, KPP = 64 / LPK;        // lanes per k line, k lines per piece
            const int kl = g * KPP + lane / LPK, cpos = lane % LPK;
            const int c = (cpos - 4 * ((kl >> 3) & 3)) & (LPK - 1);   // the line image is rotated by 16 floats per 8 k lines
            row = m0 + 4 * c;
            akl[j] = kl;
            extra = 0;
            const int one[1] = {min(row, Mr - 1)};
            int64_t mo[1];
            map_rows<1>(amap, one, mo);
            avoff[j] = row < Mr ? (uint32_t)(mo[0] * 4) + (uint32_t)((int64_t)kl * p.a_ks * 4) : kOobOffset;
        } else {
            const int rt = g * 8 + (lane >> 3), cpos = lane & 7;
            const int c = cpos ^ ((rt >> 1) & 7);
            row = m0 + rt;
            akl[j] = 4 * c;
            extra = 4 * c;
            const int one[1] = {min(row, Mr - 1)};
            int64_t mo[1];
            map_rows<1>(amap, one, mo);
            avoff[j] = row < Mr ? (uint32_t)((mo[0] + extra) * 4) : kOobOffset;
        }
    }
    // ---- B: one per-lane offset; plane / 16-row block / slice are scalar
    const __amdgpu_buffer_rsrc_t rsrc_b =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p.b_ps), (short)0, (int)bps_bytes, 0x00020000);
    const uint32_t bvoff = (uint32_t)((n0 + (lane >> 2)) * 64 + (((lane & 3) ^ ((-(lane >> 4)) & 3)) * 16));

    auto dma_b = [&](int it, int buf) { ps_dma_b<C>(rsrc_b, Bs, buf, wave, bvoff, s0 + it, it < nk, n0, np_rows); };
    auto dma_a = [&](int it, int buf) {
        const int k0 = kbeg + 32 * it;
        const uint32_t soff = it < nk ? (uint32_t)(AKM ? (int64_t)k0 * p.a_ks * 4 : (int64_t)k0 * 4) : 0u;
        ps_dma_a<C>(rsrc_a, As, buf, wave, avoff, akl, k0, kend, soff, a_nt != 0);
    };

    f32x4 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

    // prologue: the slices ahead of the K loop, one per buffer but the last (B then A); they must have landed.  (A loop of
    // one trip: with the two calls written out the compiler schedules the K loop differently, 40 instructions longer on
    // the 64 x 160 tile.)
#pragma unroll
    for (int i = 0; i < ST - 1; ++i) { dma_b(i, i); dma_a(i, i); }
    ICK_WAIT_VMCNT0();
    ICK_LDS_BARRIER();

#ifdef ICK_PS_STAMPS
    unsigned long long ph[6] = {0, 0, 0, 0, 0, 0}, ta = 0, tb = 0, tc = 0, td = 0, te = 0, tf = 0;
    ICK_PSTAMP(t_loop);
#endif
    int buf = 0;                             // LDS buffer holding slice `it`
    for (int it = 0; it < nk; ++it) {
        ICK_PSTAMP(ta);
        // slice it + 1 goes into the buffer that was read in iteration it - 1 (a slice beyond the range is a zero fill that
        // touches no memory); its pieces are issued one by one between the MFMAs below
        int nb = buf + 1;
        if (nb >= ST) nb -= ST;
        const int k0_nx = kbeg + 32 * (it + 1);
        const uint32_t soff_nx = it + 1 < nk ? (uint32_t)(AKM ? (int64_t)k0_nx * p.a_ks * 4 : (int64_t)k0_nx * 4) : 0u;
        auto piece = [&](int idx) {
            ps_dma_piece<C>(idx, rsrc_a, rsrc_b, As, Bs, nb, wave, bvoff, avoff, akl, s0 + it + 1, it + 1 < nk, n0, np_rows,
                            k0_nx, kend, soff_nx);
        };
        const int abuf = buf, bbuf = buf;
        ICK_PSTAMP(tb);
        // B fragments PF blocks ahead of their MFMAs (PF = TN: the whole slice is requested first, so the LDS latency is
        // paid once per slice and the 6 x TM x TN MFMAs then issue back to back; the ds_reads return in order)
        const char* bt = Bs + bbuf * C::B_STAGE;
        auto read_b = [&](int b, bf16x8_t (&f)[3]) {
            const int row = (wn * TN + b) * 16 + fi;
            const char* ptr = bt + row * 64 + 16 * (fq ^ kc_swz(row));
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
                f[pl] = __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(ptr + pl * C::B_PLANE));
        };
        // The TN column blocks are processed in groups of GB = PF blocks: the next group's fragments are requested while
        // this group's MFMAs issue, and inside a group the six partial products are the OUTER loop -- consecutive MFMAs
        // then go to different accumulators.  (Six MFMAs in a row into one accumulator ran at half rate: every tile shape
        // settled at 32 cycles per v_mfma_f32_16x16x32_bf16, profiles/r04_*_gemm_ps_tiles.txt.)  The order of the six
        // products per accumulator is unchanged (smallest first), so the sums are bit-identical.
        constexpr int GB = C::PF, NG = (TN + GB - 1) / GB;
        bf16x8_t bf[2][GB][3];
#pragma unroll
        for (int j = 0; j < GB; ++j) read_b(j, bf[0][j]);
        // the wave's A fragments (TM x 16 rows x 32 k): raw fp32 -> three bf16 planes each (the split's ~44 VALU
        // instructions per fragment run while the B fragments are on their way)
        bf16x8_t af[TM][3];
        const char* at = As + abuf * C::A_STAGE;
#pragma unroll
        for (int a = 0; a < TM; ++a) {
            float x[8];
            const int r0 = (wm * TM + a) * 16;
            if constexpr (AKM) {
                const int pos = (r0 + fi + 16 * fq) & (BM - 1);
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = *reinterpret_cast<const float*>(at + ((8 * fq + j) * BM + pos) * 4);
            } else {
                const int row = r0 + fi, sw = (row >> 1) & 7;
                const float4 u = *reinterpret_cast<const float4*>(at + row * 128 + 16 * ((2 * fq) ^ sw));
                const float4 v = *reinterpret_cast<const float4*>(at + row * 128 + 16 * ((2 * fq + 1) ^ sw));
                x[0] = u.x; x[1] = u.y; x[2] = u.z; x[3] = u.w; x[4] = v.x; x[5] = v.y; x[6] = v.z; x[7] = v.w;
            }
            uint32_t h[4], m[4], l[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) split3(x[2 * j], x[2 * j + 1], h[j], m[j], l[j]);
            af[a][0] = __builtin_bit_cast(bf16x8_t, u32x4_t{h[0], h[1], h[2], h[3]});
            af[a][1] = __builtin_bit_cast(bf16x8_t, u32x4_t{m[0], m[1], m[2], m[3]});
            af[a][2] = __builtin_bit_cast(bf16x8_t, u32x4_t{l[0], l[1], l[2], l[3]});
        }
        // the scheduler must not sink the fragment requests back to their uses (it would, to save registers)
        __builtin_amdgcn_sched_barrier(0);
        ICK_PSTAMP(tc);
        constexpr int pa[6] = {0, 2, 1, 0, 1, 0}, pb[6] = {2, 0, 1, 1, 0, 0};     // (A plane, B plane), smallest products first
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) {
#pragma unroll
                for (int j = 0; j < GB; ++j)
                    if ((g + 1) * GB + j < TN) read_b((g + 1) * GB + j, bf[(g + 1) & 1][j]);
            }
#pragma unroll
            for (int q = 0; q < 6; ++q) {
#pragma unroll
                for (int j = 0; j < GB; ++j)
#pragma unroll
                    for (int a = 0; a < TM; ++a) {
                        const int b = g * GB + j;
                        if (b < TN)
                            acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[a][pa[q]], bf[g & 1][j][pb[q]], acc[a][b], 0, 0, 0);
                    }
                // one DMA piece of slice it + 1 per slot, in the first half of the slots (they must have landed by the end of
                // this iteration)
                constexpr int NS = NG * 6, NP = C::PB_W + C::PA_W;
                constexpr int SPAN = (NS + 1) / 2;
                constexpr int STRIDE = SPAN / NP > 0 ? SPAN / NP : 1;
                const int slot = g * 6 + q;
                if (slot % STRIDE == 0 && slot / STRIDE < NP) piece(slot / STRIDE);
                if (slot == NS - 1) {            // whatever did not fit the slots
#pragma unroll
                    for (int r = (NS - 1) / STRIDE + 1; r < NP; ++r) piece(r);
                }
            }
        }
        ICK_PSTAMP(td);
        // slice it + 1 has landed
        ICK_WAIT_VMCNT0();
        ICK_PSTAMP(te);
        ICK_LDS_BARRIER();
        ICK_PSTAMP(tf);
#ifdef ICK_PS_STAMPS
        ph[0] += tb - ta; ph[1] += tc - tb; ph[2] += td - tc; ph[3] += te - td; ph[4] += tf - te; ph[5] += 1;
#endif
        if (++buf == ST) buf = 0;
    }
#ifdef ICK_PS_STAMPS
    ICK_PSTAMP(t_end);
    const unsigned long long t_loop_end = t_end;
#endif
    ICK_WAIT_VMCNT0();       // the zero fill of the last iteration writes LDS too: it may not outlive the workgroup
    gemm_epilogue<TM, TN>(p, Mr, acc, m0, n0, wm, wn, fi, fq, zid);
#ifdef ICK_PS_STAMPS
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the stores of the epilogue have been acknowledged
    ICK_PSTAMP(t_end);
    if (threadIdx.x == 0 && blockIdx.x == (gridDim.x >> 1) && blockIdx.z == 0) {
        for (int i = 0; i < 6; ++i) ick_ps_stamps[i] = ph[i];
        ick_ps_stamps[6] = t_loop - t_start;          // set-up + first slices requested and landed
        ick_ps_stamps[7] = t_end - t_loop_end;        // epilogue incl. its stores
        ick_ps_stamps[8] = t_end - t_start;
        ick_ps_stamps[9] = __builtin_amdgcn_s_memrealtime() - rt_start;
    }
#endif
}


namespace {

template <class C>
int launch_ps_cfg(const ick_gemm_args& a, int np_rows, int64_t bytes, int tiles_m, int tiles_n, int kchunk, int split,
                  hipStream_t s) {
    static LdsAttrOnce attr;
    if (int e = attr.ensure(reinterpret_cast<const void*>(gemm_ps_kernel<C::WM, C::WN, C::TM, C::TN, C::AKM, C::PF>), 160 * 1024))
        return e;
    hipLaunchKernelGGL((gemm_ps_kernel<C::WM, C::WN, C::TM, C::TN, C::AKM, C::PF>), dim3(tiles_m * tiles_n, 1, split),
                       dim3(C::NT), C::LDS, s, a, np_rows, bytes, tiles_m, tiles_n, kchunk, /*a_nt=*/0);
    ICK_LAUNCH_RET();
}

// The tiles of the pre-split kernel: waves as WM x WN, wave tile TM x TN blocks of 16 x 16, PF = B fragment blocks requested
// ahead of their MFMAs.  Two workgroups per CU each: they are not barrier-coupled, so their fragment and MFMA phases overlap.
//   128 x 128  8 x 1 waves of 16 x 128, PF 2, 80 KB of LDS   <- outputs wider than 320 columns
//   64 x 160   2 x 2 waves of 32 x 80, PF 5, 76 KB           <- one column tile pair, too few rows to fill the chip by 128
//   128 x 80   8 x 1 waves of 16 x 80, PF 2, 62 KB           <- outputs at most 320 wide: Encoder.conv1, split-K gradients
template <bool AKM> using Ps128x128 = PsCfg<8, 1, 1, 8, AKM, 2>;
template <bool AKM> using Ps64x160 = PsCfg<2, 2, 2, 5, AKM, 5>;
template <bool AKM> using Ps128x80 = PsCfg<8, 1, 1, 5, AKM, 2>;

// f(the PsCfg of `tile` for this A layout)
template <class F>
auto with_ps_tile(PsTile tile, bool akm, F f) {
    switch (tile) {
        case kPs128x128: return akm ? f(Ps128x128<true>{}) : f(Ps128x128<false>{});
        case kPs64x160: return akm ? f(Ps64x160<true>{}) : f(Ps64x160<false>{});
        case kPs128x80: return akm ? f(Ps128x80<true>{}) : f(Ps128x80<false>{});
    }
    __builtin_unreachable();
}

}  // namespace

PsTileInfo gemm_ps_tile(PsTile tile) {
    return with_ps_tile(tile, false, [](auto c) { return PsTileInfo{c.BM, c.BN, c.NW, c.WGS_PER_CU}; });
}

int launch_gemm_ps(const ick_gemm_args& a, bool akm, PsTile tile, int tiles_m, int tiles_n, int kchunk, int split, hipStream_t s) {
    const int np = (int)ps_rows(a.N);
    const int64_t bytes = ps_bytes(a.N, a.K);
    if (bytes >= ((int64_t)1 << 31)) return ICK_EINVAL;
    return with_ps_tile(tile, akm, [&](auto c) {
        return launch_ps_cfg<decltype(c)>(a, np, bytes, tiles_m, tiles_n, kchunk, split, s);
    });
}

}  // namespace ick

extern "C" int ick_presplit_bytes(int32_t N, int32_t K, int64_t* bytes) {
    if (N <= 0 || K <= 0 || !bytes) return ICK_EINVAL;
    *bytes = ick::ps_bytes(N, K);
    return ICK_OK;
}

extern "C" int ick_presplit_weights(const ick_presplit_item* items, int32_t count, void* stream) {
    using namespace ick;
    if (!items || count <= 0) return ICK_EINVAL;
    for (int i0 = 0; i0 < count; i0 += kPsMaxItems) {
        PsBatch b;
        b.count = std::min(kPsMaxItems, count - i0);
        int total = 0;
        for (int i = 0; i < b.count; ++i) {
            const ick_presplit_item& it = items[i0 + i];
            ICK_CHECK_ARG(it.src && it.dst && it.N > 0 && it.K > 0);
            ICK_CHECK_ARG(it.src_cs == 1 || it.src_rs == 1);
            ICK_CHECK_ARG(it.k_map == nullptr || (it.src_rs == 1 && it.src_cs != 1));
            ICK_CHECK_ARG((reinterpret_cast<uintptr_t>(it.dst) & 15) == 0);
            b.it[i] = it;
            b.first[i] = total;
            total += ceil_div(it.N, 64) * ceil_div(it.K, 32);
        }
        b.first[b.count] = total;
        hipLaunchKernelGGL(presplit_kernel, dim3(total), dim3(256), 0, (hipStream_t)stream, b);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    return ICK_OK;
}
