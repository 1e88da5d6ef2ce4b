// Token selection of a KV-cached decode step: what follows the layer and score-head kernels of decode.hip.
//
//   dec_select_kernel        (row)           greedy: top-2 over the vocabulary kernel's per-tile candidates + pointer
//                                            scores, predict()'s bookkeeping (n-gram clean-up, <end>), embedding +
//                                            position code of the next token
//   dec_beam_partial_kernel  (chunk, row)    beam search, stage 1: a chunk's maximum, sum of exponentials and k best
//   dec_select_beam_kernel   (caption)       beam search, stage 2: the k winners of a caption's candidates (plain, rules,
//                                            diverse, constrained), their histories and embeddings
//
// Sampling is sample.hip.  The greedy selection also exists folded into the next step's first launch (decode.hip:
// fused_select); both forms take predict()'s decision from greedy_step() (decode_select.h).
#include "decode_select.h"

#include <type_traits>

namespace ick {
namespace {

struct SelectArgs : GreedySel {
    float* x0;                     // (R, d) embedding of the next token
    int d, n_total;
};

__device__ __forceinline__ Top2 top2_merge_wave(Top2 t) {
    t = top2_merge_row(t);
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        Top2 o;
        o.v1 = __shfl_xor(t.v1, off, 64); o.i1 = __shfl_xor(t.i1, off, 64);
        o.v2 = __shfl_xor(t.v2, off, 64); o.i2 = __shfl_xor(t.i2, off, 64);
        top2_push(t, o.v1, o.i1);
        top2_push(t, o.v2, o.i2);
    }
    return t;
}

// Selection + predict()'s per-step bookkeeping for one caption (geo-aware/models.py:410-441) + embedding of the
// next input token.  Thread 0 fetches the caption's recent history while the workgroup scans the candidates, so the
// n-gram clean-up runs on registers: the kernel is two memory round trips long (candidates, embedding row).
__global__ __launch_bounds__(256) void dec_select_kernel(SelectArgs a) {
    if (*a.n_done >= a.n_total) return;
    __shared__ Top2 sh[4];
    __shared__ int64_t tok_sh[2];
    const int tid = threadIdx.x, i = a.step;
    const int64_t r = blockIdx.x;
    int64_t* o = a.output + r * a.max_len;
    int32_t* hs = a.hist + r * a.max_len;
    int po[5] = {-1, -1, -1, -1, -1};         // output[i-1 .. i-5]
    int ph[3] = {0, 0, 0};                    // runner-ups of steps i-1 .. i-3
    int fin = 0;
    if (tid == 0) {
        fin = a.finished[r];
#pragma unroll
        for (int q = 0; q < 5; ++q) po[q] = (int)o[max(i - 1 - q, 0)];
#pragma unroll
        for (int q = 0; q < 3; ++q) ph[q] = hs[max(i - 1 - q, 0)];
    }
    Top2 s{-INFINITY, -INFINITY, kNone, kNone};
    constexpr int NC = 4;                      // 1024 candidate tiles (49 152 words) per sweep
    for (int t0 = 0; t0 < a.ntiles; t0 += 256 * NC) {
        float4 cd[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) cd[q] = a.cand[r * a.ntiles + min(t0 + tid + 256 * q, a.ntiles - 1)];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            if (t0 + tid + 256 * q >= a.ntiles) continue;
            const int i1 = __float_as_int(cd[q].y), i2 = __float_as_int(cd[q].w);
            top2_push(s, cd[q].x, i1);
            top2_push(s, cd[q].z, i2);
        }
    }
    const TokenEmbed& e = a.emb;
    const int np = e.K + e.F;
    for (int k = tid; k < np; k += 256) top2_push(s, a.ptr[r * np + k], e.V + k);
    s = top2_merge_wave(s);
    if ((tid & 63) == 0) sh[tid >> 6] = s;
    __syncthreads();
    if (tid == 0) {
        Top2 t = sh[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            top2_push(t, sh[w].v1, sh[w].i1);
            top2_push(t, sh[w].v2, sh[w].i2);
        }
        const int second = t.i2 == kNone ? t.i1 : t.i2;
        const GreedyStep g = greedy_step(t.i1, second, i, po, ph, fin, a.end_token, e.V, e.K, e.has_facts);
        if (!fin) {
            o[i] = g.cur;
            if (g.ended) {
                a.finished[r] = 1;
                atomicAdd(a.n_done, 1);
            } else {
                hs[i] = second;
                if (g.nrw >= 1) o[i - 1] = g.rw[0];
                if (g.nrw >= 3) { o[i - 2] = g.rw[1]; o[i - 3] = g.rw[2]; }
            }
        }
        e.next_token[r] = g.tok;
        e.next_mask[r] = g.msk;
        tok_sh[0] = g.tok;
        tok_sh[1] = g.msk;
        if (a.cap_buf != nullptr && i + 1 < a.max_len) a.cap_buf[r * a.max_len + i + 1] = g.tok;
    }
    __syncthreads();
    if (i + 1 >= a.max_len) return;
    // CaptionEmbedder + sqrt(d) scale + PositionEncoder of the next input token (geo-aware/models.py:155-181,355-357)
    const float* src = e.row(tok_sh[0], (int)tok_sh[1], r, a.d);
    const float* pe = e.pe + (int64_t)(i + 1) * a.d;
    for (int c = tid; c < a.d; c += 256) a.x0[r * a.d + c] = fmaf(src[c], e.emb_scale, pe[c]);
}

// ---------------------------------------------------------------------------------------------------------
// beam selection: one workgroup per caption; its k hypotheses are rows b*k .. b*k+k-1
// ---------------------------------------------------------------------------------------------------------
constexpr int kBeamMax = 8;
struct BeamArgs {
    const float* rec;                   // (R, nchunk, kBeamRec) chunk records of dec_beam_partial_kernel
    float* cum;                         // (R) cumulative log-probability of every hypothesis
    int32_t* fin;                       // (R) hypothesis has produced <end>
    const int64_t* seq_in; int64_t* seq_out;     // (R, max_len) tokens so far
    const int32_t* anc_in; int32_t* anc_out;     // (R, max_len) cache row of every position
    const int64_t* cap_in; int64_t* cap_out;     // optional (R, max_len) caption buffers (<start> + tokens)
    int32_t* n_done;
    TokenEmbed emb;                     // (rows_per_sample: the beam width k)
    float* x0;
    int R, d, step, max_len, end_token, start_token;
    int n_total;
    // decoding rules (the RULES variant): rule words (length penalty: words[2] != 0), lp[0..max_len], and the tokens
    // of every hypothesis, <end> included
    const int32_t* words; const float* lp; int32_t* len;
    // diverse beam search (the DIVERSE variant): `groups` groups of k / groups hypotheses, and the penalty lambda (one
    // fp32 in device memory)
    int groups; const float* penalty;
    // constrained beam search (the FORCED variant): the forced columns (B, kForceMax), -1 = empty slot, the met-slot
    // mask of every hypothesis (R), and the step's score rows (the unmet forced columns are read from them)
    const int32_t* force; int32_t* met;
    const float* scores; int64_t ld; const float* ptr;
};
constexpr int kForceMax = 8;            // forced-column slots per caption (ick_decode_constraints)

// The diversity penalty lambda of ick_decode_diversity, read through the scalar cache like rule_words(): a device input
// the host writes before a (replayed) decode.
__device__ __forceinline__ float diversity_penalty(const float* p) {
#if defined(__HIP_DEVICE_COMPILE__)
    uint32_t v;
    asm volatile("s_load_dword %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(v) : "s"(p) : "memory");
    return __uint_as_float(v);
#else
    return *p;                              // (the host pass only parses device code)
#endif
}

// Block-wide arg-best of (value, code) pairs: larger value wins, ties go to the smaller code.  Result in every thread.
__device__ __forceinline__ void block_best(float& v, int& c, float* shv, int* shc) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const float ov = __shfl_xor(v, off, 64);
        const int oc = __shfl_xor(c, off, 64);
        const bool take = ov > v || (ov == v && oc < c);
        v = take ? ov : v;
        c = take ? oc : c;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shv[threadIdx.x >> 6] = v; shc[threadIdx.x >> 6] = c; }
    __syncthreads();
    v = shv[0]; c = shc[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const bool take = shv[w] > v || (shv[w] == v && shc[w] < c);
        v = take ? shv[w] : v;
        c = take ? shc[w] : c;
    }
}

// block_best() with a leading integer rank: the larger rank wins, then the larger value, then the smaller code.
__device__ __forceinline__ bool ranked_before(int p, float v, int c, int op, float ov, int oc) {
    return op > p || (op == p && (ov > v || (ov == v && oc < c)));
}
__device__ __forceinline__ void block_best_ranked(int& p, float& v, int& c, int* shp, float* shv, int* shc) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int op = __shfl_xor(p, off, 64);
        const float ov = __shfl_xor(v, off, 64);
        const int oc = __shfl_xor(c, off, 64);
        const bool take = ranked_before(p, v, c, op, ov, oc);
        p = take ? op : p;
        v = take ? ov : v;
        c = take ? oc : c;
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { shp[threadIdx.x >> 6] = p; shv[threadIdx.x >> 6] = v; shc[threadIdx.x >> 6] = c; }
    __syncthreads();
    p = shp[0]; v = shv[0]; c = shc[0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
        const bool take = ranked_before(p, v, c, shp[w], shv[w], shc[w]);
        p = take ? shp[w] : p;
        v = take ? shv[w] : v;
        c = take ? shc[w] : c;
    }
}

constexpr int kBeamChunk = 1024;      // scores per stage-1 workgroup
constexpr int kBeamCandPerThread = 16; // stage 2 holds beam^2 x chunks candidates in the registers of 256 threads
constexpr int kBeamRec = 2 + 2 * kBeamMax;   // floats per (row, chunk) record: max, sum of exp, kBeamMax x (value, index)

// Stage 1 of the beam selection, one workgroup per (chunk of 1024 scores, row): the chunk's maximum, its sum of
// exp(score - maximum), and its k best (value, index) pairs -- 5 x 10 k scores per caption are reduced by 50
// workgroups instead of one.
struct BeamPartArgs {
    const float* scores; int64_t ld; const float* ptr;
    const float* cum; const int32_t* fin;
    float* rec;                         // (R, nchunk, kBeamRec)
    int R, k, V, np, nchunk;
    const int32_t* n_done; int n_total;
    // decoding rules (nullptr: off): the row's tokens so far seq (R, max_len), the rule words
    const int64_t* seq; const int32_t* words;
    int step, max_len, end_token;
};
// Constrained beam search (the FORCED variant) appends the forced columns (R / k, kForceMax) and the met-slot masks (R).
// They extend the struct for that variant alone: the hidden launch arguments the other instantiations read follow the
// explicit ones, and would move with them.
struct BeamPartForcedArgs : BeamPartArgs {
    const int32_t* force; const int32_t* met;
};
// The column-bias variant (BIASED) appends the bias lists (R / k, kBiasMax) in the same way.
struct BeamPartBiasArgs : BeamPartArgs {
    const int32_t* bcols; const float* bvals;
};
// The caption-prefix variant (PREFIX) appends the forced column of every step (R / k, max_len), -1 = a free step, to the
// plain and to the biased arguments, again for its own instantiations alone.
struct BeamPartPrefixArgs : BeamPartArgs {
    const int32_t* pcols;
};
struct BeamPartBiasPrefixArgs : BeamPartBiasArgs {
    const int32_t* pcols;
};
template <bool FORCED, bool BIASED, bool PREFIX>
using BeamPartArgsOf = std::conditional_t<
    PREFIX, std::conditional_t<BIASED, BeamPartBiasPrefixArgs, BeamPartPrefixArgs>,
    std::conditional_t<FORCED, BeamPartForcedArgs, std::conditional_t<BIASED, BeamPartBiasArgs, BeamPartArgs>>>;
// RULES: the decoding-rules variant (ick_decode_select_beam_rules); FORCED: constrained beam search
// (ick_decode_select_beam_forced); BIASED: column bias (ick_decode_select_beam_biased, §3.2k); PREFIX:
// caption prefixes (ick_decode_select_beam_prefix, §3.2l)
template <bool RULES, bool FORCED = false, bool BIASED = false, bool PREFIX = false>
__global__ __launch_bounds__(256)
void dec_beam_partial_kernel(BeamPartArgsOf<FORCED, BIASED, PREFIX> a) {
    static_assert(!(FORCED && BIASED), "the column bias does not compose with forced columns");
    static_assert(!(FORCED && PREFIX), "a caption prefix does not compose with forced columns");
    if (*a.n_done >= a.n_total) return;
    __shared__ float shv[4];
    __shared__ int shc[4];
    __shared__ float red[8];
    __shared__ uint32_t ban[kBeamChunk / 32];
    __shared__ int hs[kRuleHistMax];
    const int tid = threadIdx.x, ch = blockIdx.x;
    const int64_t r = blockIdx.y;
    if (a.fin[r] || a.cum[r] == -INFINITY) return;         // ended / unused hypothesis: nothing to expand (uniform)
    const uint4 rw = RULES ? rule_words(a.words) : make_uint4(0u, 0u, 0u, 0u);
    const int nrep = (int)rw.x, mlen = (int)rw.y;
    const int Vx = a.V + a.np;
    const float* row = a.scores + r * a.ld;
    const float* pr = a.ptr + r * a.np;
    float x[4];
    int idx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        idx[q] = ch * kBeamChunk + tid + 256 * q;
        const int v = min(idx[q], Vx - 1);
        x[q] = v < a.V ? row[v] : pr[v - a.V];
        if (idx[q] >= Vx) { x[q] = -INFINITY; idx[q] = kNone; }
    }
    float m = fmaxf(fmaxf(x[0], x[1]), fmaxf(x[2], x[3]));
    m = block_max<4>(m, red);
    float e = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) e += x[q] == -INFINITY ? 0.f : __expf(x[q] - m);
    e = block_sum<4>(e, red);
    float* rec = a.rec + (r * a.nchunk + ch) * kBeamRec;
    if (tid == 0) { rec[0] = m; rec[1] = e; }
    if constexpr (PREFIX) {
        // A forced step (uniform: one column per caption and step): the row's pool is that column alone, whatever the
        // rules ban, so neither the ban pass nor the k arg-best rounds run.  The chunk that holds the column records
        // it in slot 0 -- its raw score, plus its bias in the biased form -- and every other slot of every chunk is
        // written as empty: stage 2 reads all k of them.  The maximum and the sum of exp above cover every raw column.
        const int fc = __builtin_amdgcn_readfirstlane(a.pcols[(r / a.k) * a.max_len + a.step]);
        if (fc >= 0) {
            float fb = 0.f;
            if constexpr (BIASED) {                         // the bias of the column's lowest slot, as in the pool
                const BiasLanes bl = bias_lanes(a.bcols, a.bvals, r / a.k);
                const unsigned long long hit = __ballot(bl.col == fc);
                if (hit) fb = bl.val_of(__ffsll((long long)hit) - 1);
            }
            if (tid < a.k) {
                float v = -INFINITY; int c = kNone;
                if (tid == 0 && fc < Vx && fc / kBeamChunk == ch) {
                    v = (fc < a.V ? row[fc] : pr[fc - a.V]) + fb;
                    c = v == -INFINITY ? kNone : fc;
                }
                rec[2 + 2 * tid] = v; rec[3 + 2 * tid] = __int_as_float(c);
            }
            return;
        }
    }
    if (RULES && (nrep > 0 || a.step < mlen)) {             // uniform: the banned columns leave the pool (not the sums)
        mark_bans(a.seq + r * a.max_len, a.step, nrep, mlen, a.end_token, ban, ch * kBeamChunk, kBeamChunk / 32, hs);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int c = tid + 256 * q;
            if ((ban[c >> 5] >> (c & 31)) & 1u) { x[q] = -INFINITY; idx[q] = kNone; }
        }
    }
    if constexpr (FORCED) {
        // The row's unmet forced columns, and <end> while one is unmet, leave the pool as bans do (not the sums):
        // stage 2 ranks the former as candidates of their own, in a higher bank.  Every column left has the row's bank.
        const int32_t* fr = a.force + (r / a.k) * kForceMax;
        const int met = a.met[r];
        bool unmet_any = false;
#pragma unroll
        for (int s = 0; s < kForceMax; ++s) {
            const int w = fr[s];
            const bool unmet = w >= 0 && !((met >> s) & 1);
            unmet_any = unmet_any || unmet;
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (unmet && idx[q] == w) { x[q] = -INFINITY; idx[q] = kNone; }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (unmet_any && idx[q] == a.end_token) { x[q] = -INFINITY; idx[q] = kNone; }
    }
    if constexpr (BIASED) {
        // Column bias: the pool holds s + b (the maximum and the sum of exp above stay raw).  The slots that fall in
        // this chunk -- most chunks have none -- are visited in order with their column as a uniform value and added by
        // the lane that owns the column (column c of the chunk is x[c >> 8] of thread c & 255), a column's lowest slot
        // only.  A banned column stays out whatever its bias, and a -inf bias takes its column out as a ban does.
        const BiasLanes bl = bias_lanes(a.bcols, a.bvals, r / a.k);
        int done = 0;
        for (unsigned long long live = bl.live(ch * kBeamChunk, min((ch + 1) * kBeamChunk, Vx)); live != 0;) {
            const int t = BiasLanes::next(live);
            const int c = bl.col_of(t) - ch * kBeamChunk;
            const float b = bl.val_of(t);
            const int q = c >> 8;
            if ((c & 255) == tid && !((done >> q) & 1)) {
                done |= 1 << q;
#pragma unroll
                for (int q2 = 0; q2 < 4; ++q2)
                    if (q2 == q) x[q2] += b;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (x[q] == -INFINITY) idx[q] = kNone;
    }
    for (int round = 0; round < a.k; ++round) {
        float bv = -INFINITY; int bc = kNone;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bool take = x[q] > bv || (x[q] == bv && idx[q] < bc);
            bv = take ? x[q] : bv;
            bc = take ? idx[q] : bc;
        }
        block_best(bv, bc, shv, shc);
        if (tid == 0) { rec[2 + 2 * round] = bv; rec[3 + 2 * round] = __int_as_float(bc); }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (idx[q] == bc) { x[q] = -INFINITY; idx[q] = kNone; }      // the winner leaves the pool
    }
}

// The LDS tables of one caption's selection step, by hypothesis (force: by forced slot).  met, force, nmet belong to the
// FORCED variant and xtok to the DIVERSE one.
struct BeamRows {
    float *cum, *lse;
    int *fin, *len, *parent, *tok, *nfin, *met, *force, *nmet, *xtok;
    float* bsum;
};
// The column-bias variant (BIASED) appends the bias lists (R / k, kBiasMax) and every hypothesis' bias sum (R), for
// that variant alone (as BeamPartBiasArgs).
struct BeamBiasArgs : BeamArgs {
    const int32_t* bcols; const float* bvals; float* bsum;
};

// One selection round: the block-wide arg-best (bv, bc) of every thread's candidates; the winner leaves the pool.
template <int N>
__device__ __forceinline__ void beam_round(float (&v)[N], int (&c)[N], float& bv, int& bc, float* shv, int* shc) {
    bv = -INFINITY; bc = kNone;
#pragma unroll
    for (int q = 0; q < N; ++q) {
        const bool take = v[q] > bv || (v[q] == bv && c[q] < bc);
        bv = take ? v[q] : bv;
        bc = take ? c[q] : bc;
    }
    block_best(bv, bc, shv, shc);
#pragma unroll
    for (int q = 0; q < N; ++q)
        if (c[q] == bc) { v[q] = -INFINITY; c[q] = kNone; }
}

// The winner of a round (code c, key `key`) becomes hypothesis h: thread 0 decides parent, token and ended-or-not and
// stores the step's bookkeeping.  cum is the raw summed log-probability: where the key is not that (length penalty,
// diversity penalty, banks, column bias) it is derived again from the step's score row, by the expression that made the
// key.  BIASED: bsum_out is the caption's bias sums in global memory and bw the bias of the winner's column; the new
// hypothesis carries its parent's sum plus bw, a carried one its own.
template <bool DIVERSE, bool FORCED, bool BIASED = false>
__device__ __forceinline__ void beam_winner(const BeamArgs& a, const BeamRows& s, int64_t r0, bool lp_on, int h,
                                            float key, int c, float* bsum_out = nullptr, float bw = 0.f) {
    const int np = a.emb.K + a.emb.F, Vx = a.emb.V + np;
    const bool rederive = DIVERSE || FORCED || BIASED || lp_on;
    float v = rederive || c == kNone ? -INFINITY : key;         // fewer candidates than beams: a dead slot
    int parent = 0, tok = a.emb.pad_token, nf = 1, len = 0, met = 0;
    float bsum = 0.f;
    if (c != kNone) {
        parent = c / Vx;
        if constexpr (FORCED) met = s.met[parent];
        if constexpr (BIASED) bsum = s.bsum[parent];
        if (s.fin[parent]) {                                    // an ended hypothesis is carried as it is
            if (rederive) v = s.cum[parent];
            if (lp_on) len = s.len[parent];
        } else {
            if constexpr (BIASED) bsum += bw;
            tok = c - parent * Vx; nf = tok == a.end_token;
            if (rederive) {
                const float x = tok < a.emb.V ? a.scores[(r0 + parent) * a.ld + tok]
                                          : a.ptr[(r0 + parent) * np + (tok - a.emb.V)];
                v = s.cum[parent] - s.lse[parent] + x;
            }
            len = a.step + 1;
            if constexpr (FORCED)
                for (int f = 0; f < kForceMax; ++f) met |= s.force[f] == tok ? 1 << f : 0;
        }
    }
    s.parent[h] = parent; s.tok[h] = tok; s.nfin[h] = nf;
    if constexpr (FORCED) s.nmet[h] = met;
    if constexpr (DIVERSE) s.xtok[h] = c != kNone && !s.fin[parent] ? tok : -1;
    if (lp_on) a.len[r0 + h] = len;
    if constexpr (BIASED) bsum_out[h] = bsum;
    a.cum[r0 + h] = v;
    a.fin[r0 + h] = nf;
    const bool live = c != kNone && !nf;
    a.emb.next_token[r0 + h] = live ? tok : 0;
    a.emb.next_mask[r0 + h] = live ? token_kind(tok, a.emb.V, a.emb.K, a.emb.has_facts) : 0;
}

// DIVERSE: diverse beam search (ick_decode_select_beam_diverse); FORCED: constrained beam search
// (ick_decode_select_beam_forced); BIASED: column bias (ick_decode_select_beam_biased, §3.2k)
template <bool RULES, bool DIVERSE = false, bool FORCED = false, bool BIASED = false>
__global__ __launch_bounds__(256) void dec_select_beam_kernel(std::conditional_t<BIASED, BeamBiasArgs, BeamArgs> a) {
    static_assert(!(BIASED && (DIVERSE || FORCED)), "the column bias composes with the rules only");
    // No exit on *n_done here: other workgroups of this very launch add to it, and the hypothesis tables are
    // ping-pong buffers -- a step that skipped its carry-copy would leave the previous step's rows (in another
    // order) in the buffer the caller reads.  The decision below only looks at this caption's own state, which no
    // other workgroup writes.
    __shared__ float shv[4];
    __shared__ int shc[4];
    __shared__ float cum_s[kBeamMax], lse_s[kBeamMax];
    __shared__ int fin_s[kBeamMax], parent_s[kBeamMax], tok_s[kBeamMax], nfin_s[kBeamMax];
    __shared__ int len_s[kBeamMax];
    __shared__ float lpf_s[kBeamMax];
    __shared__ int met_s[FORCED ? kBeamMax : 1], force_s[FORCED ? kForceMax : 1], nmet_s[FORCED ? kBeamMax : 1];
    __shared__ int shp[FORCED ? 4 : 1];
    __shared__ int xtok_s[DIVERSE ? kBeamMax : 1];          // column expanded into slot j at this step, or -1
    __shared__ float bsum_s[BIASED ? kBeamMax : 1];         // bias sum of hypothesis j going into this step
    __shared__ int bcol_s[BIASED ? kBiasMax : 1];           // the caption's bias list
    __shared__ float bval_s[BIASED ? kBiasMax : 1];
    const BeamRows rows{cum_s, lse_s, fin_s, len_s, parent_s, tok_s, nfin_s, met_s, force_s, nmet_s, xtok_s, bsum_s};
    const int tid = threadIdx.x, k = a.emb.rows_per_sample;
    const int64_t r0 = (int64_t)blockIdx.x * k;
    const int np = a.emb.K + a.emb.F, Vx = a.emb.V + np;
    const int nchunk = (Vx + kBeamChunk - 1) / kBeamChunk;
    // length penalty (uniform): candidates are ranked by cum / lp[L], L = step + 1 for a live expansion and the length
    // it ended at for an ended hypothesis; cum itself stays the raw summed log-probability
    const bool lp_on = RULES && rule_words(a.words).z != 0u;
    if (tid < k) {
        cum_s[tid] = a.cum[r0 + tid]; fin_s[tid] = a.fin[r0 + tid];
        if (lp_on) { len_s[tid] = a.len[r0 + tid]; lpf_s[tid] = a.lp[len_s[tid]]; }
    }
    if constexpr (FORCED) {
        if (tid < k) met_s[tid] = a.met[r0 + tid];
        if (tid >= 64 && tid < 64 + kForceMax) force_s[tid - 64] = a.force[blockIdx.x * kForceMax + tid - 64];
    }
    if constexpr (BIASED) {
        if (tid < k) bsum_s[tid] = a.bsum[r0 + tid];
        if (tid >= 64 && tid < 64 + kBiasMax) {
            bcol_s[tid - 64] = a.bcols[blockIdx.x * kBiasMax + tid - 64];
            bval_s[tid - 64] = a.bvals[blockIdx.x * kBiasMax + tid - 64];
        }
    }
    __syncthreads();
    bool live_any = false;
    for (int j = 0; j < k; ++j) live_any = live_any || !(fin_s[j] || cum_s[j] == -INFINITY);
    if (!live_any) {
        // every hypothesis of this caption has ended: the tables move to the other buffer as they are
        for (int idx = tid; idx < k * a.max_len; idx += 256) {
            const int64_t e = r0 * a.max_len + idx;
            a.seq_out[e] = a.seq_in[e];
            a.anc_out[e] = a.anc_in[e];
            if (a.cap_out != nullptr) a.cap_out[e] = a.cap_in[e];
        }
        if (tid < k) { a.emb.next_token[r0 + tid] = 0; a.emb.next_mask[r0 + tid] = 0; }
        return;
    }
    // log-sum-exp of every live row from its chunk records (wave j handles row j, j + 4)
    for (int j = tid >> 6; j < k; j += 4) {
        if (fin_s[j] || cum_s[j] == -INFINITY) continue;
        const int lane = tid & 63;
        float m = -INFINITY;
        for (int c = lane; c < nchunk; c += 64) m = fmaxf(m, a.rec[((r0 + j) * nchunk + c) * kBeamRec]);
        m = wave_max(m);
        float e = 0.f;
        for (int c = lane; c < nchunk; c += 64) {
            const float* rc = a.rec + ((r0 + j) * nchunk + c) * kBeamRec;
            e += rc[1] * __expf(rc[0] - m);
        }
        e = wave_sum(e);
        if (lane == 0) lse_s[j] = m + __logf(e);
    }
    __syncthreads();
    // candidates: k per (live row, chunk), one per ended row; every thread keeps up to NC of them
    constexpr int NC = kBeamCandPerThread;
    const float lp_live = lp_on ? a.lp[a.step + 1] : 1.f;
    float cv[NC]; int cc[NC];
    const int per_row = nchunk * k, total = k * per_row;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        cv[q] = -INFINITY; cc[q] = kNone;
        const int id = tid + 256 * q;
        if (id < total) {
            const int j = id / per_row, rem = id - j * per_row, c = rem / k, slot = rem - c * k;
            if (cum_s[j] != -INFINITY) {
                if (fin_s[j]) {
                    if (rem == 0) {                                      // an ended hypothesis competes as it is
                        const float v = BIASED ? cum_s[j] + bsum_s[j] : cum_s[j];
                        cv[q] = lp_on ? v / lpf_s[j] : v; cc[q] = j * Vx;
                    }
                } else {
                    const float* rc = a.rec + ((r0 + j) * nchunk + c) * kBeamRec;
                    const int idx = __float_as_int(rc[3 + 2 * slot]);
                    if (idx != kNone) {
                        float v = cum_s[j] - lse_s[j] + rc[2 + 2 * slot];       // (BIASED: the record holds s + b)
                        if constexpr (BIASED) v += bsum_s[j];
                        cv[q] = lp_on ? v / lp_live : v; cc[q] = j * Vx + idx;
                    }
                }
            }
        }
    }
    if constexpr (FORCED) {
        // Constrained beam search (dynamic beam allocation): every candidate carries its bank, the number of met slots
        // of the hypothesis it would make.  A pool candidate has its row's bank (stage 1 took the unmet forced columns
        // and a closed <end> out of the pool); thread j * kForceMax + s adds row j's unmet forced column of slot s,
        // scored from the row like the pool's.  The k rounds visit the banks from the highest down and round again,
        // skipping empty ones: the rank below puts the non-empty bank whose turn it is first, so one ranked arg-best
        // per round takes that bank's best candidate.
        constexpr int NF = NC + 1;
        float fv[NF]; int fc[NF], fb[NF];
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            fv[q] = cv[q]; fc[q] = cc[q];
            fb[q] = cc[q] == kNone ? -32 : __popc(met_s[cc[q] / Vx]);
        }
        fv[NC] = -INFINITY; fc[NC] = kNone; fb[NC] = -32;
        if (tid < k * kForceMax) {
            const int j = tid / kForceMax, s = tid - j * kForceMax, w = force_s[s];
            bool cand = w >= 0 && !((met_s[j] >> s) & 1) && !fin_s[j] && cum_s[j] != -INFINITY;
            int add = 0;
#pragma unroll
            for (int s2 = 0; s2 < kForceMax; ++s2) {
                const bool same = force_s[s2] == w;
                cand = cand && !(same && s2 < s);               // slots holding one id: one candidate, the first slot's
                add |= same ? 1 << s2 : 0;
            }
            if (cand) {
                const float x = w < a.emb.V ? a.scores[(r0 + j) * a.ld + w] : a.ptr[(r0 + j) * np + (w - a.emb.V)];
                const float v = cum_s[j] - lse_s[j] + x;
                fv[NC] = lp_on ? v / lp_live : v; fc[NC] = j * Vx + w;
                fb[NC] = __popc(met_s[j] | add);
            }
        }
        int turn = kForceMax + 1;                               // the bank visited last
        for (int round = 0; round < k; ++round) {
            int bp = -64; float bv = -INFINITY; int bc = kNone;
#pragma unroll
            for (int q = 0; q < NF; ++q) {
                const int p = fb[q] < turn ? fb[q] + 16 : fb[q];
                const bool take = ranked_before(bp, bv, bc, p, fv[q], fc[q]);
                bp = take ? p : bp;
                bv = take ? fv[q] : bv;
                bc = take ? fc[q] : bc;
            }
            block_best_ranked(bp, bv, bc, shp, shv, shc);
#pragma unroll
            for (int q = 0; q < NF; ++q)
                if (fc[q] == bc) { fv[q] = -INFINITY; fc[q] = kNone; fb[q] = -32; }
            if (bc != kNone) turn = bp >= 16 ? bp - 16 : bp;
            if (tid == 0) beam_winner<false, true>(a, rows, r0, lp_on, round, bv, bc);
        }
        __syncthreads();
        if (tid < k) a.met[r0 + tid] = nmet_s[tid];
    } else if constexpr (BIASED) {
        // Column bias: the key holds the hypothesis' bias sum and the column's bias, cum does not (beam_winner derives
        // it again from the raw score).  Wave 0 finds the winner's bias in the caption's list, the lowest slot first.
        for (int round = 0; round < k; ++round) {
            float bv; int bc;
            beam_round(cv, cc, bv, bc, shv, shc);
            if (tid < kBiasMax) {
                const int tok = bc == kNone ? -2 : bc % Vx;
                const unsigned long long hit = __ballot(bcol_s[tid] == tok);
                const float bw = hit ? bval_s[__ffsll(hit) - 1] : 0.f;
                if (tid == 0) beam_winner<false, false, true>(a, rows, r0, lp_on, round, bv, bc, a.bsum + r0, bw);
            }
        }
    } else if constexpr (!DIVERSE) {
        for (int round = 0; round < k; ++round) {
            float bv; int bc;
            beam_round(cv, cc, bv, bc, shv, shc);
            if (tid == 0) beam_winner<false, false>(a, rows, r0, lp_on, round, bv, bc);
        }
    } else {
        // Diverse beam search: the groups choose in order.  Group g ranks the candidates of its own rows g*kg ..
        // (g+1)*kg - 1 by key - lambda * n, n = the number of hypotheses of groups 0 .. g-1 expanded with the
        // candidate's column at this step (an ended hypothesis competes with its key as it is), and its kg rounds fill
        // slots g*kg + round: k rounds in all, as without groups.
        const int kg = k / a.groups;
        const float lam = diversity_penalty(a.penalty);
        for (int g = 0; g < a.groups; ++g) {
            const int lo = g * kg * Vx, hi = lo + kg * Vx;
            float gv[NC]; int gc[NC];
#pragma unroll
            for (int q = 0; q < NC; ++q) {
                gv[q] = -INFINITY; gc[q] = kNone;
                if (cc[q] >= lo && cc[q] < hi) {            // (kNone is above every code)
                    const int j = cc[q] / Vx, col = cc[q] - j * Vx;
                    int n = 0;
                    if (!fin_s[j])
                        for (int i = 0; i < g * kg; ++i) n += xtok_s[i] == col;
                    gv[q] = cv[q] - lam * (float)n; gc[q] = cc[q];
                }
            }
            for (int round = 0; round < kg; ++round) {
                float bv; int bc;
                beam_round(gv, gc, bv, bc, shv, shc);
                if (tid == 0) beam_winner<true, false>(a, rows, r0, lp_on, g * kg + round, bv, bc);
            }
            __syncthreads();                                // xtok_s of this group before the next group reads it
        }
    }
    __syncthreads();
    if (tid == 0) {
        int before = 0, after = 0;
        for (int j = 0; j < k; ++j) { before += fin_s[j] || cum_s[j] == -INFINITY; after += nfin_s[j]; }
        if (after != before) atomicAdd(a.n_done, after - before);
    }
    // histories of the chosen parents move to their new rows
    for (int idx = tid; idx < k * a.max_len; idx += 256) {
        const int j = idx / a.max_len, p = idx - j * a.max_len;
        const int64_t src = (r0 + parent_s[j]) * a.max_len + p, dst = (r0 + j) * a.max_len + p;
        const bool carried = fin_s[parent_s[j]] != 0;
        a.seq_out[dst] = p < a.step ? a.seq_in[src] : (p == a.step && !carried ? (int64_t)tok_s[j]
                                                       : (carried ? a.seq_in[src] : (int64_t)a.emb.pad_token));
        a.anc_out[dst] = p < a.step ? a.anc_in[src] : (p == a.step ? (int32_t)(r0 + parent_s[j]) : 0);
        if (a.cap_out != nullptr)
            a.cap_out[dst] = p <= a.step ? a.cap_in[src]
                                         : (p == a.step + 1 && !nfin_s[j] ? (int64_t)tok_s[j] : (int64_t)a.start_token);
    }
    if (a.step + 1 >= a.max_len) return;
    const float* pe = a.emb.pe + (int64_t)(a.step + 1) * a.d;
    for (int idx = tid; idx < k * a.d; idx += 256) {
        const int j = idx / a.d, c = idx - j * a.d;
        const int tok = nfin_s[j] ? 0 : tok_s[j];
        // (tok is in [0, Vx), has_facts is F > 0 and fe is non-null exactly then: no clamp of token_row() acts here)
        const float* src = token_row(tok, token_kind(tok, a.emb.V, a.emb.K, a.emb.has_facts), (int64_t)blockIdx.x, a.emb.word_emb, a.emb.ee,
                                     a.emb.fe, a.emb.V, a.emb.K, a.emb.F, a.d, a.emb.pad_token);
        a.x0[(r0 + j) * a.d + c] = fmaf(src[c], a.emb.emb_scale, pe[c]);
    }
}

}  // namespace
}  // namespace ick

using namespace ick;

extern "C" int ick_decode_beam_supported(int32_t Vx, int32_t beam) {
    if (Vx <= 0 || beam < 1 || beam > kBeamMax) return 0;
    return (int64_t)beam * beam * ceil_div(Vx, kBeamChunk) <= 256 * kBeamCandPerThread;   // candidates the selection holds
}

extern "C" int ick_decode_select_greedy(const ick_decode_ctx* c, int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && c->R > 0 && pos >= 0 && pos < c->max_len);
    ICK_CHECK_ARG(c->output && c->hist && c->finished && c->n_done && c->next_token && c->next_mask && c->word_emb &&
                  c->pe && c->x0 && c->cand && c->ptr && c->ee);
    SelectArgs a;
    fill_greedy_sel(a, c, pos);
    a.x0 = c->x0; a.d = c->d; a.n_total = c->R;
    hipLaunchKernelGGL(dec_select_kernel, dim3(c->R), dim3(256), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}

static int select_beam_impl(const ick_decode_ctx* c, const ick_beam_state* bs, const ick_decode_rules* rules,
                            const ick_decode_diversity* div, const ick_decode_constraints* fc,
                            const ick_decode_bias* bias, const ick_decode_prefix* px, int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && bs && c->R > 0 && pos >= 0 && pos < c->max_len);
    ICK_CHECK_ARG(c->rows_per_sample >= 1 && c->rows_per_sample <= kBeamMax && c->R % c->rows_per_sample == 0);
    ICK_CHECK_ARG(c->scores && c->scores_ld >= c->V && c->ptr && c->n_done && c->next_token && c->next_mask &&
                  c->word_emb && c->pe && c->x0 && c->ee);
    ICK_CHECK_ARG(bs->cum && bs->fin && bs->seq_in && bs->seq_out && bs->anc_in && bs->anc_out);
    ICK_CHECK_ARG((bs->cap_in == nullptr) == (bs->cap_out == nullptr));
    ICK_CHECK_ARG(bs->rec != nullptr);
    const int Vx = c->V + c->K + c->F, nchunk = ceil_div(Vx, kBeamChunk);
    ICK_CHECK_ARG(ick_decode_beam_supported(Vx, c->rows_per_sample));
    BeamPartForcedArgs pa;
    pa.scores = c->scores; pa.ld = c->scores_ld; pa.ptr = c->ptr; pa.cum = bs->cum; pa.fin = bs->fin; pa.rec = bs->rec;
    pa.R = c->R; pa.k = c->rows_per_sample; pa.V = c->V; pa.np = c->K + c->F; pa.nchunk = nchunk;
    pa.n_done = c->n_done; pa.n_total = c->R;
    pa.seq = bs->seq_in; pa.words = rules ? rules->words : nullptr;
    pa.step = pos; pa.max_len = c->max_len; pa.end_token = c->end_token;
    if (px != nullptr) {
        // caption prefixes are instantiated on the rules form only, plain and biased (as the column bias is); beam
        // groups differ in stage 2 alone
        if (bias != nullptr) {
            BeamPartBiasPrefixArgs xa;
            static_cast<BeamPartArgs&>(xa) = pa;
            xa.bcols = bias->cols; xa.bvals = bias->vals; xa.pcols = px->cols;
            hipLaunchKernelGGL((dec_beam_partial_kernel<true, false, true, true>), dim3(nchunk, c->R), dim3(256), 0,
                               (hipStream_t)stream, xa);
        } else {
            BeamPartPrefixArgs xa;
            static_cast<BeamPartArgs&>(xa) = pa;
            xa.pcols = px->cols;
            hipLaunchKernelGGL((dec_beam_partial_kernel<true, false, false, true>), dim3(nchunk, c->R), dim3(256), 0,
                               (hipStream_t)stream, xa);
        }
    } else if (fc != nullptr) {
        pa.force = fc->force; pa.met = fc->met;
        void (*part)(BeamPartForcedArgs) = rules ? dec_beam_partial_kernel<true, true> : dec_beam_partial_kernel<false, true>;
        hipLaunchKernelGGL(part, dim3(nchunk, c->R), dim3(256), 0, (hipStream_t)stream, pa);
    } else if (bias != nullptr) {
        // the column bias is instantiated on the rules form only: without rules the rule words read as zero
        BeamPartBiasArgs ba;
        static_cast<BeamPartArgs&>(ba) = pa;
        ba.bcols = bias->cols; ba.bvals = bias->vals;
        hipLaunchKernelGGL((dec_beam_partial_kernel<true, false, true>), dim3(nchunk, c->R), dim3(256), 0,
                           (hipStream_t)stream, ba);
    } else {
        void (*part)(BeamPartArgs) = rules ? dec_beam_partial_kernel<true> : dec_beam_partial_kernel<false>;
        hipLaunchKernelGGL(part, dim3(nchunk, c->R), dim3(256), 0, (hipStream_t)stream, (const BeamPartArgs&)pa);
    }
    BeamArgs a;
    a.rec = bs->rec; a.cum = bs->cum; a.fin = bs->fin;
    a.seq_in = bs->seq_in; a.seq_out = bs->seq_out; a.anc_in = bs->anc_in; a.anc_out = bs->anc_out;
    a.cap_in = bs->cap_in; a.cap_out = bs->cap_out; a.n_done = c->n_done;
    a.emb = token_embed_of(c); a.x0 = c->x0;
    a.R = c->R; a.d = c->d; a.step = pos; a.max_len = c->max_len; a.end_token = c->end_token;
    a.start_token = bs->start_token; a.n_total = c->R;
    a.words = rules ? rules->words : nullptr; a.lp = rules ? rules->lp : nullptr; a.len = rules ? rules->len : nullptr;
    a.groups = div ? div->groups : 1; a.penalty = div ? div->penalty : nullptr;
    a.force = fc ? fc->force : nullptr; a.met = fc ? fc->met : nullptr;
    a.scores = c->scores; a.ld = c->scores_ld; a.ptr = c->ptr;
    if (bias != nullptr) {
        BeamBiasArgs ba;
        static_cast<BeamArgs&>(ba) = a;
        ba.bcols = bias->cols; ba.bvals = bias->vals; ba.bsum = bias->sum;
        hipLaunchKernelGGL((dec_select_beam_kernel<true, false, false, true>), dim3(c->R / c->rows_per_sample),
                           dim3(256), 0, (hipStream_t)stream, ba);
        ICK_LAUNCH_RET();
    }
    void (*sel)(BeamArgs) = fc ? (rules ? dec_select_beam_kernel<true, false, true>
                                        : dec_select_beam_kernel<false, false, true>) :
                            div ? (rules ? dec_select_beam_kernel<true, true> : dec_select_beam_kernel<false, true>)
                                : (rules ? dec_select_beam_kernel<true, false> : dec_select_beam_kernel<false, false>);
    hipLaunchKernelGGL(sel, dim3(c->R / c->rows_per_sample), dim3(256), 0, (hipStream_t)stream, a);
    ICK_LAUNCH_RET();
}

extern "C" int ick_decode_select_beam(const ick_decode_ctx* c, const ick_beam_state* bs, int32_t pos, void* stream) {
    return select_beam_impl(c, bs, nullptr, nullptr, nullptr, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_beam_rules(const ick_decode_ctx* c, const ick_beam_state* bs,
                                            const ick_decode_rules* rules, int32_t pos, void* stream) {
    ICK_CHECK_ARG(rules_ok(c, rules, true));
    return select_beam_impl(c, bs, rules, nullptr, nullptr, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_beam_diverse(const ick_decode_ctx* c, const ick_beam_state* bs,
                                              const ick_decode_rules* rules, const ick_decode_diversity* div,
                                              int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && div && div->penalty && div->groups >= 1 && c->rows_per_sample >= 1 &&
                  c->rows_per_sample % div->groups == 0);
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, true));
    return select_beam_impl(c, bs, rules, div, nullptr, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_beam_forced(const ick_decode_ctx* c, const ick_beam_state* bs,
                                             const ick_decode_rules* rules, const ick_decode_constraints* fc,
                                             int32_t pos, void* stream) {
    ICK_CHECK_ARG(c && fc && fc->force && fc->met && c->rows_per_sample >= 1 && c->rows_per_sample <= kBeamMax);
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, true));
    return select_beam_impl(c, bs, rules, nullptr, fc, nullptr, nullptr, pos, stream);
}

extern "C" int ick_decode_select_beam_biased(const ick_decode_ctx* c, const ick_beam_state* bs,
                                             const ick_decode_rules* rules, const ick_decode_bias* bias, int32_t pos,
                                             void* stream) {
    ICK_CHECK_ARG(c && bias && bias->cols && bias->vals && bias->sum);
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, true));
    return select_beam_impl(c, bs, rules, nullptr, nullptr, bias, nullptr, pos, stream);
}

extern "C" int ick_decode_select_beam_prefix(const ick_decode_ctx* c, const ick_beam_state* bs,
                                             const ick_decode_rules* rules, const ick_decode_diversity* div,
                                             const ick_decode_bias* bias, const ick_decode_prefix* px, int32_t pos,
                                             void* stream) {
    ICK_CHECK_ARG(c && px && px->cols && !(div && bias));
    ICK_CHECK_ARG(div == nullptr || (div->penalty && div->groups >= 1 && c->rows_per_sample >= 1 &&
                                     c->rows_per_sample % div->groups == 0));
    ICK_CHECK_ARG(bias == nullptr || (bias->cols && bias->vals && bias->sum));
    ICK_CHECK_ARG(rules == nullptr || rules_ok(c, rules, true));
    return select_beam_impl(c, bs, rules, div, nullptr, bias, px, pos, stream);
}
