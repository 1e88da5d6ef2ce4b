// Geo-reference counts (ick_geo_reference_counts): the histograms behind the geo variant's Jensen-Shannon metric
// (geo-aware/jensen_shannon_metric.py of the reference: JSGeoMetric.run / store_data_for_idx), on token ids.  The
// definition is stated in include/ick_amd.h and geo_metric.py; DESIGN.md 3.2j has the reasoning.
//
// One workgroup of ONE wave per caption row:
//   1. the row (T <= 128 tokens) and the two bin-edge tables go to LDS;
//   2. every position is tested against the three preposition windows on the LDS copy of the row -- this needs no
//      entity data, and a row without a candidate (or with an image_index out of range) writes its marks and leaves;
//   3. the lanes build the image's entity records in LDS, 64 entities per pass: a lane runs the "unk_ent" search over
//      ONE name (a single pass: 'u' occurs only at the head of the pattern, so a mismatch falls back to state 1 on a 'u'
//      and to 0 otherwise) and finds the entity's distance bin, azimuth bin and type; a ballot compacts the slots of the
//      non-unk entities, in slot order, into the list the random baseline draws from;
//   4. the candidates look their entity up, draw the random one (Philox-4x32-10, philox.h) and add to the histograms.
// The histograms are added up with global INTEGER atomics: a caption holds a handful of geo references at most, so a
// workgroup issues a few dozen adds; an LDS partial histogram (8 x (129 + n_types) words, twice) would cost more to
// clear than that.  Integer sums do not depend on the order the adds land in, so the totals are the same bits on every
// run and ICK_DETERMINISTIC needs no second path.
#include "common.h"
#include "philox.h"

namespace ick {
namespace {

constexpr int kGeoMaxT = ICK_GEO_MAX_T;
constexpr int kGeoMaxK = ICK_GEO_MAX_K;
constexpr int kGeoMaxBins = ICK_GEO_MAX_BINS;
constexpr int kGeoMaxTypes = ICK_GEO_MAX_TYPES;
constexpr int kGeoTerms = ICK_GEO_TERMS;
constexpr int kGeoChars = ICK_GEO_NAME_CHARS;
constexpr int kGeoNameLd = 2 + kGeoChars;
constexpr int kGeoPasses = kGeoMaxT / kWave;

struct GeoArgs {
    const int64_t* tokens;        // (N, T)
    const int32_t* image_index;   // (N)
    const float* ent;             // (B, K, C)
    const int64_t* names;         // (B, K, 2 + 50)
    const double* bins_d;         // (n_dist, 2) lo, hi
    const double* bins_a;         // (n_az, 2)
    int32_t *marks, *gen, *rnd;
    int64_t hist_ld;
    uint64_t row0;
    uint32_t k0, k1;
    int N, T, B, K, C, V, n_dist, n_az, n_types;
    int trig[kGeoTerms];          // -1: the word map lacks the word
    int of_id, the_id, a_id;
};

// an entity record: bits 0-12 type + 1, 13-19 distance bin + 1, 20-26 azimuth bin + 1 (0 = none), bit 31 unk_ent
constexpr uint32_t kGeoUnk = 0x80000000u;

__device__ __forceinline__ bool geo_is(int64_t t, int id) { return id >= 0 && t == (int64_t)id; }

__device__ __forceinline__ int geo_term(const GeoArgs& a, int64_t t) {
    int term = -1;
#pragma unroll
    for (int q = kGeoTerms - 1; q >= 0; --q)
        if (geo_is(t, a.trig[q])) term = q;
    return term;
}

// term << 12 | entity slot of position i when it is a pointer behind one of the three windows, else -1
__device__ __forceinline__ int geo_candidate(const GeoArgs& a, const int64_t* tok, int i) {
    if (i < 1) return -1;
    const int64_t t = tok[i], p0 = tok[i - 1];
    if (t < a.V || t - a.V >= a.K || p0 >= a.V) return -1;
    int term = geo_term(a, p0);
    if (term < 0 && i >= 2) {
        const bool of0 = geo_is(p0, a.of_id), art0 = geo_is(p0, a.the_id) || geo_is(p0, a.a_id);
        if (of0 || art0) {
            const int64_t p1 = tok[i - 2];
            term = geo_term(a, p1);
            if (term < 0 && i >= 3 && art0 && geo_is(p1, a.of_id)) term = geo_term(a, tok[i - 3]);
        }
    }
    return term < 0 ? -1 : (term << 12) | (int)(t - a.V);
}

__device__ __forceinline__ bool geo_name_unk(const int64_t* nm) {
    static constexpr int64_t pat[7] = {'u', 'n', 'k', '_', 'e', 'n', 't'};
    const int64_t len = nm[1];
    const int n = (len < 0 || len > kGeoChars) ? kGeoChars : (int)len;
    int s = 0;
    for (int j = 0; j < n; ++j) {
        const int64_t c = nm[2 + j];
        s = c == pat[s] ? s + 1 : (c == pat[0] ? 1 : 0);
        if (s == 7) return true;
    }
    return false;
}

// 1 + the first bin with lo <= x < hi, 0 when there is none (NaN included)
__device__ __forceinline__ uint32_t geo_bin(const double (*bins)[2], int nb, float x) {
    const double v = (double)x;
    for (int b = 0; b < nb; ++b)
        if (v >= bins[b][0] && v < bins[b][1]) return (uint32_t)b + 1u;
    return 0u;
}

__device__ __forceinline__ void geo_count(int32_t* hist, int64_t ld, int term, uint32_t rec) {
    int32_t* h = hist + (int64_t)term * ld;
    atomicAdd(h, 1);
    const uint32_t ty = rec & 0x1FFFu, d = (rec >> 13) & 0x7Fu, az = (rec >> 20) & 0x7Fu;
    if (term < 4) {
        if (d) atomicAdd(h + d, 1);                                   // column 1 + (d - 1)
    } else if (az) {
        atomicAdd(h + kGeoMaxBins + az, 1);                           // column 1 + 64 + (az - 1)
    }
    if (term >= 1 && term <= 3 && ty) atomicAdd(h + 2 * kGeoMaxBins + ty, 1);
}

__global__ __launch_bounds__(kWave) void geo_counts_kernel(GeoArgs a) {
    __shared__ int64_t s_tok[kGeoMaxT];
    __shared__ double s_bins[2][kGeoMaxBins][2];
    __shared__ uint32_t s_rec[kGeoMaxK + 1];
    __shared__ uint16_t s_list[kGeoMaxK + 1];
    const int n = blockIdx.x, lane = threadIdx.x;
    const int64_t* row = a.tokens + (int64_t)n * a.T;
    for (int i = lane; i < a.T; i += kWave) s_tok[i] = row[i];
    if (lane < a.n_dist) { s_bins[0][lane][0] = a.bins_d[2 * lane]; s_bins[0][lane][1] = a.bins_d[2 * lane + 1]; }
    if (lane < a.n_az) { s_bins[1][lane][0] = a.bins_a[2 * lane]; s_bins[1][lane][1] = a.bins_a[2 * lane + 1]; }
    __syncthreads();

    int cand[kGeoPasses];
    bool any = false;
#pragma unroll
    for (int c = 0; c < kGeoPasses; ++c) {
        const int i = c * kWave + lane;
        cand[c] = i < a.T ? geo_candidate(a, s_tok, i) : -1;
        any = any || cand[c] >= 0;
    }
    const int img = a.image_index[n];
    int32_t* marks = a.marks + (int64_t)n * a.T;
    if (!__syncthreads_or(any) || img < 0 || img >= a.B) {           // block-uniform
        for (int i = lane; i < a.T; i += kWave) marks[i] = -1;
        return;
    }

    const float* ent = a.ent + (int64_t)img * a.K * a.C;
    const int64_t* names = a.names + (int64_t)img * a.K * kGeoNameLd;
    int known = 0;                                                    // non-unk entities so far (wave-uniform)
    for (int kb = 0; kb < a.K; kb += kWave) {
        const int k = kb + lane;
        bool ok = false;
        if (k < a.K) {
            const float* f = ent + (int64_t)k * a.C;
            const float ty = f[4];
            uint32_t rec = geo_name_unk(names + (int64_t)k * kGeoNameLd) ? kGeoUnk : 0u;
            rec |= geo_bin(s_bins[0], a.n_dist, f[1]) << 13;
            rec |= geo_bin(s_bins[1], a.n_az, f[2]) << 20;
            if (ty >= 0.f && ty < (float)a.n_types && ty == floorf(ty)) rec |= (uint32_t)(int)ty + 1u;
            s_rec[k] = rec;
            ok = !(rec & kGeoUnk);
        }
        const uint64_t m = __ballot(ok);
        if (ok) s_list[known + __popcll(m & ((1ull << lane) - 1ull))] = (uint16_t)k;
        known += __popcll(m);
    }
    __syncthreads();

#pragma unroll
    for (int c = 0; c < kGeoPasses; ++c) {
        const int i = c * kWave + lane;
        if (i >= a.T) continue;
        int mark = -1;
        if (cand[c] >= 0) {
            const int term = cand[c] >> 12, k = cand[c] & 0xFFF;
            const uint32_t rec = s_rec[k];
            if (!(rec & kGeoUnk)) {                                   // so known >= 1
                const uint64_t r = a.row0 + (uint64_t)n;
                const uint32_t x = philox4x32_10(make_uint4((uint32_t)i, (uint32_t)r, (uint32_t)(r >> 32), 0u),
                                                 a.k0, a.k1).x;
                const int rk = s_list[x % (uint32_t)known];
                geo_count(a.gen, a.hist_ld, term, rec);
                geo_count(a.rnd, a.hist_ld, term, s_rec[rk]);
                mark = (term << 24) | (rk << 12) | k;
            }
        }
        marks[i] = mark;
    }
}

}  // namespace
}  // namespace ick

extern "C" int ick_geo_reference_counts(const int64_t* tokens, int32_t N, int32_t T, const int32_t* image_index,
                                        const float* entities, const int64_t* entity_names, int32_t B, int32_t K,
                                        int32_t C, int32_t V, const int32_t* trigger_ids, int32_t of_id, int32_t the_id,
                                        int32_t a_id, const double* bins_distance, int32_t n_distance,
                                        const double* bins_azimuth, int32_t n_azimuth, int32_t n_types, int64_t hist_ld,
                                        int64_t seed, int64_t row_offset, int32_t* marks, int32_t* generated,
                                        int32_t* random, void* stream) {
    using namespace ick;
    ICK_CHECK_ARG(tokens && image_index && entities && entity_names && trigger_ids && bins_distance && bins_azimuth);
    ICK_CHECK_ARG(marks && generated && random && generated != random);
    ICK_CHECK_ARG(N > 0 && T > 0 && T <= kGeoMaxT && B > 0 && K > 0 && K <= kGeoMaxK && C >= 5 && V > 0);
    ICK_CHECK_ARG(n_distance > 0 && n_distance <= kGeoMaxBins && n_azimuth > 0 && n_azimuth <= kGeoMaxBins);
    ICK_CHECK_ARG(n_types > 0 && n_types <= kGeoMaxTypes && hist_ld >= 1 + 2 * kGeoMaxBins + (int64_t)n_types);
    ICK_CHECK_ARG(row_offset >= 0 && of_id < V && the_id < V && a_id < V);
    GeoArgs a{};
    for (int q = 0; q < kGeoTerms; ++q) {
        ICK_CHECK_ARG(trigger_ids[q] < V);
        a.trig[q] = trigger_ids[q] < 0 ? -1 : trigger_ids[q];
    }
    a.tokens = tokens; a.image_index = image_index; a.ent = entities; a.names = entity_names;
    a.bins_d = bins_distance; a.bins_a = bins_azimuth; a.marks = marks; a.gen = generated; a.rnd = random;
    a.hist_ld = hist_ld; a.row0 = (uint64_t)row_offset;
    a.k0 = (uint32_t)((uint64_t)seed & 0xFFFFFFFFull); a.k1 = (uint32_t)((uint64_t)seed >> 32);
    a.N = N; a.T = T; a.B = B; a.K = K; a.C = C; a.V = V; a.n_dist = n_distance; a.n_az = n_azimuth; a.n_types = n_types;
    a.of_id = of_id < 0 ? -1 : of_id; a.the_id = the_id < 0 ? -1 : the_id; a.a_id = a_id < 0 ? -1 : a_id;
    hipLaunchKernelGGL(geo_counts_kernel, dim3(N), dim3(kWave), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}
