// The index rules of the context inputs, each written once: which table row a caption token stands for, the indices
// of an entity row, the (subject, predicate) pair of a fact, and the per-sample tables of the predicate gate.  The
// forward kernels (prefill.hip), their backward kernels in both forms (backward.hip) and the decode, sampling and SCST
// kernels (through token_row / token_kind) all decode through these, so the clamping contract of DESIGN.md §4
// (deviation 2) has one home.  Plain stateless device functions and small structs.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ick_amd.h"

namespace ick {

// An int64 row index clamped to [0, n - 1].  The clamp runs in int64 and only then narrows: an index such as 2^32 + 1
// is out of range, not row 1.
__device__ __forceinline__ int clamp_row(int64_t v, int n) {
    return (int)(v < 0 ? 0 : (v >= (int64_t)n ? (int64_t)n - 1 : v));
}

// ---- caption token -> table row (geo-aware/models.py:155-181) ------------------------------------------------------
// kind is the caption mask CaptionEmbedder reads: 1 an entity slot, 2 a fact slot when the fact table is given,
// anything else a word.  A slot outside its table is <unk_ent> / <unk_fact>, the last row; a word id outside [0, V) is
// <pad>.  The token is clamped in its own integer width, before anything narrows it.  Caption b owns rows
// [b K, (b + 1) K) of the entity table and [b F, (b + 1) F) of the fact table; the row is formed inside each branch
// (not from a block-local index afterwards) so that a uniform token's address stays one scalar chain per branch.
enum CaptionTable : int { kWordTable = 0, kEntityTable = 1, kFactTable = 2 };
struct CaptionSlot {
    int table;      // CaptionTable
    int64_t row;    // in that table
    // that row of d floats (P: float or const float)
    template <typename P>
    __device__ __forceinline__ P* row_of(P* word, P* ent, P* fact, int d) const {
        return (table == kEntityTable ? ent : (table == kFactTable ? fact : word)) + row * d;
    }
};
template <typename T>
__device__ __forceinline__ CaptionSlot caption_slot(T tok, int64_t kind, int64_t b, int V, int K, int F, int pad_token,
                                                    bool has_fact_table) {
    if (kind == 1) {
        T e = tok - V;
        if (e < 0 || e >= K) e = K - 1;
        return {kEntityTable, b * K + e};
    }
    if (kind == 2 && has_fact_table) {
        T e = tok - V - K;
        if (e < 0 || e >= F) e = F - 1;
        return {kFactTable, b * F + e};
    }
    return {kWordTable, (int64_t)(tok >= 0 && tok < V ? tok : (T)pad_token)};
}
// The next input token of a decode step: its kind, and the embedding row of caption b it stands for.
template <typename T>
__device__ __forceinline__ int token_kind(T tok, int V, int K, bool has_facts) {
    return (has_facts && tok >= V + K) ? 2 : (tok >= V ? 1 : 0);
}
template <typename T>
__device__ __forceinline__ const float* token_row(T tok, int kind, int64_t b, const float* word_emb, const float* ee,
                                                  const float* fe, int V, int K, int F, int d, int pad_token) {
    return caption_slot(tok, kind, b, V, K, F, pad_token, fe != nullptr).row_of(word_emb, ee, fe, d);
}

// ---- entity row -> indices -----------------------------------------------------------------------------------------
// Columns [0, type_off) of an encoded entity are feature slots, the rest the type embedding row `type`; the news
// variant scales by the mean of five name-word rows.  Type and name ids arrive as floats and truncate towards zero.
struct EntityIndex {
    int type_off;   // 4 / 6 / 5 for geo / knowledge / news
    int type;       // in [0, ntypes)
    int name[5];    // in [0, vocab); news only, zeros otherwise
};
__device__ __forceinline__ EntityIndex entity_index(int variant, const float* e, int ntypes, int vocab) {
    EntityIndex ix = {variant == ICK_GEO ? 4 : (variant == ICK_KNOWLEDGE ? 6 : 5), 0, {0, 0, 0, 0, 0}};
    const int ty = (int)e[4];
    ix.type = ty < 0 ? 0 : (ty >= ntypes ? ntypes - 1 : ty);
    if (variant == ICK_NEWS) {
#pragma unroll
        for (int w = 0; w < 5; ++w) {
            const int n = (int)e[5 + w];
            ix.name[w] = n < 0 ? 0 : (n >= vocab ? vocab - 1 : n);
        }
    }
    return ix;
}

// ---- fact triple -> (subject, predicate) ---------------------------------------------------------------------------
struct FactPair {
    int subj, pred;     // in [0, K) and [0, num_pred)
};
__device__ __forceinline__ FactPair fact_pair(const int64_t* facts, int64_t row, int K, int num_pred) {
    return {clamp_row(facts[row * 3 + 1], K), clamp_row(facts[row * 3 + 2], num_pred)};
}

// ---- gate tables (get_context_indicators) --------------------------------------------------------------------------
//   first[k] = first caption position that names entity k, kInf if none does
//   act[j]   = first position at which fact j's subject counts as "already mentioned" (mode 1: 0 once mentioned)
//   pred[j]  = fact j's predicate, -1 when out of range: such a fact opens no gate
//   rep[j]   = fact j is the first (by act, then index) fact carrying its predicate
constexpr int kInf = 0x3fffffff;
inline size_t gate_table_ints(int K, int F) { return (size_t)K + 3 * (size_t)F; }
struct GateTables {
    int *first, *act, *pred, *rep;  // K, F, F, F ints
    int* end;                       // the caller's own LDS starts here
};
// Builds the tables of sample b in lds (gate_table_ints(K, F) ints).  Every thread of the 256-thread workgroup calls
// it; on return the tables are complete and visible to all of them.
__device__ __forceinline__ GateTables build_gate_tables(int* lds, const int64_t* __restrict__ captions,
                                                        const int64_t* __restrict__ facts, int b, int L, int K, int F,
                                                        int V, int num_pred, int mode) {
    const GateTables g = {lds, lds + K, lds + K + F, lds + K + 2 * F, lds + K + 3 * F};
    int *first = g.first, *act = g.act, *pred = g.pred, *rep = g.rep;
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += 256) first[k] = kInf;
    __syncthreads();
    for (int t = tid; t < L; t += 256) {
        const int64_t n = captions[(int64_t)b * L + t] - V;
        if (n >= 0 && n < K) atomicMin(&first[(int)n], t);
    }
    __syncthreads();
    for (int j = tid; j < F; j += 256) {
        const int64_t subj = facts[((int64_t)b * F + j) * 3 + 1];
        const int64_t q = facts[((int64_t)b * F + j) * 3 + 2];
        int a = kInf;
        if (subj >= 0 && subj < K && first[(int)subj] < kInf) a = mode == 0 ? first[(int)subj] + 1 : 0;
        act[j] = a;
        pred[j] = (q >= 0 && q < num_pred) ? (int)q : -1;
    }
    __syncthreads();
    for (int j = tid; j < F; j += 256) {
        int r = act[j] < kInf && pred[j] >= 0;
        if (r) {
            for (int i = 0; i < F; ++i) {
                if (i != j && pred[i] == pred[j] && (act[i] < act[j] || (act[i] == act[j] && i < j))) { r = 0; break; }
            }
        }
        rep[j] = r;
    }
    __syncthreads();
    return g;
}

}  // namespace ick
