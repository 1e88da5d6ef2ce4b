// What the decode step (decode.hip), the selection kernels that follow it (decode_select.hip) and the unfused greedy
// kernels (score_head.hip) share: the top-2 pair and its merges, predict()'s per-step decision, and the kernel arguments
// that say how the chosen token is recorded and embedded.
#pragma once
#include "common.h"

namespace ick {

// Lane exchanges inside a row of 16 lanes as DPP operands (one VALU instruction each) instead of ds_bpermute round
// trips through the LDS crossbar (~100 cycles each, four in a row per dot product): quad_perm [1,0,3,2] / [2,3,0,1]
// pair lanes inside a quad, row_half_mirror / row_mirror then pair quads and halves (every lane of a quad / half
// already holds the same partial result), row_ror:8 swaps the halves of a row.  Full waves only (common.h: dpp_f32).
constexpr int kDppXor1 = 0xB1, kDppXor2 = 0x4E, kDppHalfMirror = 0x141, kDppMirror = 0x140, kDppRor8 = 0x128;
template <int CTRL>
__device__ __forceinline__ int dppi(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }

// The two best (value, index) pairs seen: larger value first, then smaller index.  Empty slots are (-inf, kNone) and
// never displace anything.
constexpr int kNone = 0x7fffffff;
struct Top2 {
    float v1, v2;
    int i1, i2;
};
// branch-free: the merges run in every lane of a wave (nested ifs compile to exec-mask branches, ~20 per merge)
__device__ __forceinline__ void top2_push(Top2& s, float v, int i) {
    const bool b1 = v > s.v1 || (v == s.v1 && i < s.i1);
    const bool b2 = v > s.v2 || (v == s.v2 && i < s.i2);
    const float nv2 = b1 ? s.v1 : (b2 ? v : s.v2);
    const int ni2 = b1 ? s.i1 : (b2 ? i : s.i2);
    s.v1 = b1 ? v : s.v1;
    s.i1 = b1 ? i : s.i1;
    s.v2 = nv2;
    s.i2 = ni2;
}
template <int CTRL>
__device__ __forceinline__ Top2 top2_merge_dpp(Top2 t) {
    const float v1 = dpp_f32<CTRL>(t.v1), v2 = dpp_f32<CTRL>(t.v2);
    const int i1 = dppi<CTRL>(t.i1), i2 = dppi<CTRL>(t.i2);
    top2_push(t, v1, i1);
    top2_push(t, v2, i2);
    return t;
}
// over the aligned groups of 16 lanes, result in every lane
__device__ __forceinline__ Top2 top2_merge_row(Top2 t) {
    t = top2_merge_dpp<kDppXor1>(t);
    t = top2_merge_dpp<kDppXor2>(t);
    t = top2_merge_dpp<kDppHalfMirror>(t);
    return top2_merge_dpp<kDppMirror>(t);
}

constexpr int kVocabTile = 48;      // words per candidate tile: ick_decode_ctx.cand holds ceil(V / kVocabTile) per row

// ---------------------------------------------------------------------------------------------------------
// predict()'s decision of step i for one caption (geo-aware/models.py:410-441), on registers: <end>, the repeated
// n-gram clean-up (:421-435), the next input token and its caption mask.  best / second: the step's two best columns;
// po: output[i-1 .. i-5]; ph: the runner-ups of steps i-1 .. i-3 (entries before step 0 are never looked at); ended: the
// caption had produced <end> before this step.  The callers load that window and store the result, each in its own way.
// ---------------------------------------------------------------------------------------------------------
struct GreedyStep {
    int cur;            // output[i] (a caption that had ended keeps its own)
    int tok, msk;       // next input token and its mask; 0, 0 once the caption has ended
    int ended;          // the ended flag after this step
    int nrw, rw[3];     // rw = output[i-1 .. i-3] after the clean-up; the first nrw (0, 1 or 3) of them changed
};
__device__ __forceinline__ GreedyStep greedy_step(int best, int second, int i, const int (&po)[5], const int (&ph)[3],
                                                  int ended, int end_token, int V, int K, int has_facts) {
    GreedyStep s{0, 0, 0, ended, 0, {po[0], po[1], po[2]}};
    if (ended) return s;
    s.cur = best;
    if (best == end_token) { s.ended = 1; return s; }
    if (i > 0 && best == po[0]) {
        s.cur = second;
    } else if (i > 2 && best == po[1] && po[0] == po[2]) {
        s.cur = second; s.rw[0] = ph[0]; s.nrw = 1;
    } else if (i > 4 && best == po[2] && po[0] == po[3] && po[1] == po[4]) {
        s.cur = second; s.rw[0] = ph[0]; s.rw[1] = ph[1]; s.rw[2] = ph[2]; s.nrw = 3;
    }
    s.tok = s.cur;
    s.msk = token_kind(s.cur, V, K, has_facts);
    return s;
}

// How a chosen token becomes the next step's input: where it and its mask go, and the tables its embedding row comes
// from (CaptionEmbedder + sqrt(d) scale + PositionEncoder, geo-aware/models.py:155-181,355-357).
struct TokenEmbed {
    const float *word_emb, *ee, *fe, *pe;       // fe: null without facts
    int64_t* next_token; int64_t* next_mask;    // (R)
    int rows_per_sample, V, K, F, has_facts, pad_token;
    float emb_scale;
    // the embedding row of token tok (kind: token_kind()) of row r, out-of-range indices clamped
    template <typename T>
    __device__ __forceinline__ const float* row(T tok, int kind, int64_t r, int d) const {
        return token_row(tok, kind, r / rows_per_sample, word_emb, ee, fe, V, K, F, d, pad_token);
    }
};
inline TokenEmbed token_embed_of(const ick_decode_ctx* c) {
    TokenEmbed e;
    e.word_emb = c->word_emb; e.ee = c->ee; e.fe = c->F > 0 ? c->fe : nullptr; e.pe = c->pe;
    e.next_token = c->next_token; e.next_mask = c->next_mask;
    e.rows_per_sample = c->rows_per_sample; e.V = c->V; e.K = c->K; e.F = c->F; e.has_facts = c->F > 0;
    e.pad_token = c->pad_token; e.emb_scale = c->emb_scale;
    return e;
}

// Greedy selection of step `step`: what dec_select_kernel (decode_select.hip) and the selection folded into the next
// step's first launch (decode.hip: fused_select) both read and record.
struct GreedySel {
    const float4* cand;            // (R, ntiles) {best value, best index, second value, second index} of every tile
    const float* ptr;              // (R, K + F) pointer scores
    int64_t* output;               // (R, max_len)
    int32_t* hist;                 // (R, max_len) runner-up of every step
    int32_t* finished;             // (R)
    int32_t* n_done;               // number of finished rows (early exit of the following steps)
    int64_t* cap_buf;              // optional (R, max_len): the caption buffer get_context_indicators reads
    TokenEmbed emb;
    int ntiles, step, max_len, end_token;
};
template <typename Args>           // Args: GreedySel or a struct that extends it
inline void fill_greedy_sel(Args& a, const ick_decode_ctx* c, int step) {
    a.cand = reinterpret_cast<const float4*>(c->cand); a.ptr = c->ptr;
    a.output = c->output; a.hist = c->hist; a.finished = c->finished; a.n_done = c->n_done; a.cap_buf = c->cap_buf;
    a.emb = token_embed_of(c);
    a.ntiles = ceil_div(c->V, kVocabTile); a.step = step; a.max_len = c->max_len; a.end_token = c->end_token;
}

}  // namespace ick
