// Backward kernels of the training step (loss.backward() through the
// decoder of geo-aware/train.py:282-292; clip_gradient + Adam.step are csrc/adam.hip).  The GEMM-shaped
// gradients (data / weight gradients of every Linear) reuse ick_gemm with k-major operands; this
// file holds the rest: LayerNorm, ReLU mask, bias column sums, the gather/scatter backward of the
// embedding and encoder stages, the pointer-score head, the predicate gate, and the step counter
// and token-mean scale of the training graphs.
#include "common.h"

namespace ick {
namespace {

// ---------------------------------------------------------------------------------------------
// LayerNorm backward for y = LN(z) * gamma + beta with z = x + res (recomputed here):
//   zh = (z - mean) * rstd;  g = dy * gamma
//   dz = rstd * (g - mean_d(g) - zh * mean_d(g * zh));   dgamma += sum_rows dy * zh;  dbeta += sum_rows dy
// One wave per row; per-workgroup partial dgamma/dbeta are combined in LDS and then either written to
// row blockIdx.x of `partials` (nblocks x 2d; the caller column-sums it off the critical path -- 160
// workgroups hammering the same 600 addresses with float atomics cost more than the rest of the kernel)
// or, without a workspace, added to dgamma/dbeta with one float atomic per column per workgroup.
// ---------------------------------------------------------------------------------------------
template <int NJ>
__global__ __launch_bounds__(256) void layernorm_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ x,
                                                            const float* __restrict__ res,
                                                            const float* __restrict__ gamma,
                                                            const float* __restrict__ mean,
                                                            const float* __restrict__ rstd, float* __restrict__ dz,
                                                            float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                            int64_t rows, int d, int rows_per_block,
                                                            float* __restrict__ dx_drop, DropArg darg,
                                                            float* __restrict__ partials) {
    chain_priority();
    extern __shared__ float sm[];  // 4 waves x 2 * d partial sums, added in wave order (no LDS atomics: deterministic)
    const Dropout drop = darg.get();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float ag[NJ], ab[NJ], gm[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        ag[j] = 0.f; ab[j] = 0.f;
        gm[j] = c < d ? gamma[c] : 0.f;
    }
    const int64_t row0 = (int64_t)blockIdx.x * rows_per_block;
    // two rows per wave and iteration: all loads of both rows are in flight before either is reduced (the
    // kernel is bound by memory latency: 160 workgroups x 4 waves, ~15 small loads per row)
    for (int r = wave; r < rows_per_block; r += 8) {
        int64_t rows2[2] = {row0 + r, row0 + r + 4};
        bool live[2] = {rows2[0] < rows, r + 4 < rows_per_block && rows2[1] < rows};
        float zv[2][NJ], dyv[2][NJ], mu[2], rs[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int64_t row = live[q] ? rows2[q] : row0;   // row0 < rows: a valid address for dead slots
            mu[q] = mean[row]; rs[q] = rstd[row];
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = lane + 64 * j;
                float z = 0.f, dv = 0.f, rv = 0.f;
                if (c < d) {
                    z = x[row * d + c];
                    if (res) rv = res[row * d + c];
                    dv = dy[row * d + c];
                }
                if (drop.on()) z *= drop.mask((uint32_t)row * (uint32_t)d + (uint32_t)c);
                zv[q][j] = z + rv;
                dyv[q][j] = dv;
            }
        }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (!live[q]) continue;     // wave-uniform
            const int64_t row = rows2[q];
            float zh[NJ], g[NJ];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = lane + 64 * j;
                zh[j] = c < d ? (zv[q][j] - mu[q]) * rs[q] : 0.f;
                g[j] = dyv[q][j] * gm[j];
                s1 += g[j];
                s2 += g[j] * zh[j];
                ag[j] += dyv[q][j] * zh[j];
                ab[j] += dyv[q][j];
            }
            s1 = wave_sum(s1) / (float)d;
            s2 = wave_sum(s2) / (float)d;
#pragma unroll
            for (int j = 0; j < NJ; ++j) {
                const int c = lane + 64 * j;
                if (c < d) {
                    const float v = rs[q] * (g[j] - s1 - zh[j] * s2);
                    dz[row * d + c] = v;
                    if (dx_drop) dx_drop[row * d + c] = drop.on() ? v * drop.mask((uint32_t)row * (uint32_t)d + (uint32_t)c) : v;
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int c = lane + 64 * j;
        if (c < d) {
            sm[wave * 2 * d + c] = ag[j];
            sm[wave * 2 * d + d + c] = ab[j];
        }
    }
    __syncthreads();
    if (partials) {
        float* pr = partials + (int64_t)blockIdx.x * 2 * d;
        for (int i = threadIdx.x; i < 2 * d; i += 256) pr[i] = (sm[i] + sm[2 * d + i]) + (sm[4 * d + i] + sm[6 * d + i]);
        return;
    }
    for (int i = threadIdx.x; i < d; i += 256) {
        atomicAdd(dgamma + i, (sm[i] + sm[2 * d + i]) + (sm[4 * d + i] + sm[6 * d + i]));
        atomicAdd(dbeta + i, (sm[d + i] + sm[3 * d + i]) + (sm[5 * d + i] + sm[7 * d + i]));
    }
}

// dpre = dpost where the forward activation was positive (ReLU), in place or out of place
__global__ __launch_bounds__(256) void relu_bwd_kernel(const float* __restrict__ dy, const float* __restrict__ act,
                                                       float* __restrict__ dx, int64_t n, float scale) {
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        dx[i] = act[i] > 0.f ? dy[i] * scale : 0.f;
}

// out[n] += sum_m a[m, n]   (bias gradients).  grid (column blocks of 64, row slabs); each wave owns
// 64 columns x a run of rows, waves of a workgroup are combined in LDS, slabs by float atomics.
__global__ __launch_bounds__(256) void colsum_kernel(const float* __restrict__ a, int64_t M, int N, int64_t ld,
                                                     float* __restrict__ out, int rows_per_block) {
    __shared__ float sm[4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    const int64_t r1 = min(M, r0 + rows_per_block);
    float s = 0.f;
    if (c < N)
        for (int64_t r = r0 + wave; r < r1; r += 4) s += a[r * ld + c];
    sm[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < N) atomicAdd(out + c, sm[0][lane] + sm[1][lane] + sm[2][lane] + sm[3][lane]);
}

// ---------------------------------------------------------------------------------------------
// Scatter-adds of the gather stages' backward: one kernel body per stage, the walk chosen by SEQ.  The indices come
// from the rules the forward kernels use (context_index.h).
//   atomic (SEQ = false): one wave per source row, lanes stride the columns, terms added with float atomics -- the
//     hardware picks the order in which a destination row receives its terms.
//   ordered (SEQ = true; ick_set_deterministic / ICK_DETERMINISTIC=1): a (kDetParts, column blocks of 256) grid.  Every
//     workgroup walks ALL source rows in index order and workgroup p applies only the terms whose destination key has
//     key % kDetParts == p: one thread owns one column of a destination row for the whole launch, so its terms arrive
//     in source order.
// ---------------------------------------------------------------------------------------------
constexpr int kDetParts = 32;

template <bool SEQ>
struct ScatterWalk {
    int row, row_end;       // source rows [row, row_end)
    int col, col_step;      // columns col, col + col_step, .. below d
    int part;
    __device__ __forceinline__ explicit ScatterWalk(int rows) {
        if (SEQ) {
            row = 0; row_end = rows;
            col = blockIdx.y * 256 + threadIdx.x; col_step = 256 * gridDim.y;       // one column per thread
            part = blockIdx.x;
        } else {
            row = blockIdx.x * 4 + (threadIdx.x >> 6); row_end = min(row + 1, rows);
            col = threadIdx.x & 63; col_step = 64;
            part = 0;
        }
    }
    // whether this workgroup applies the terms of destination key `key` (uniform over the workgroup)
    __device__ __forceinline__ bool owns(int64_t key) const { return !SEQ || (int)(key % kDetParts) == part; }
    // *dst += v: a float atomic, or the plain read-modify-write of the one thread that owns dst
    __device__ __forceinline__ void add(float* dst, int64_t key, float v) const {
        if (!SEQ) atomicAdd(dst, v);
        else if (owns(key)) *dst += v;
    }
};

// CaptionEmbedder backward: dx (B,L,d) * scale is added to the row each token was read from (word embedding /
// encoded entity / encoded fact: caption_slot()).
template <bool SEQ>
__global__ __launch_bounds__(256) void caption_embed_bwd_kernel(const float* __restrict__ dx,
                                                                const int64_t* __restrict__ captions,
                                                                const int64_t* __restrict__ masks,
                                                                float* __restrict__ dword, float* __restrict__ dee,
                                                                float* __restrict__ dfe, int B, int L, int K, int F,
                                                                int V, int d, int pad_token, float scale,
                                                                DropArg darg) {
    if (!SEQ) chain_priority();
    const Dropout drop = darg.get();
    const ScatterWalk<SEQ> w(B * L);
    for (int row = w.row; row < w.row_end; ++row) {
        const CaptionSlot s = caption_slot(captions[row], masks[row], row / L, V, K, F, pad_token, dfe != nullptr);
        if (s.table == kWordTable && dword == nullptr) continue;
        // the three tables share the parts; the offsets keep their first rows out of one workgroup
        const int64_t key = s.row + (s.table == kFactTable ? 11 : (s.table == kWordTable ? 23 : 0));
        if (!w.owns(key)) continue;
        float* dst = s.row_of(dword, dee, dfe, d);
        for (int c = w.col; c < d; c += w.col_step) {
            float v = dx[(int64_t)row * d + c] * scale;
            if (drop.on()) v *= drop.mask((uint32_t)row * (uint32_t)d + (uint32_t)c);   // PositionEncoder dropout
            // positions past the caption's end carry exactly zero gradient (nothing after them is in the loss) and all
            // point at the <pad> row: skipping zero addends removes a ~400-way atomic pile-up on that row
            if (v != 0.f) w.add(dst + c, key, v);
        }
    }
}

// EntityEncoder backward: only the type embedding is trainable (feature slots are inputs).  News:
// e = enc * avg(name words)  =>  d enc = de * avg ; d word_emb[name_w] += de * enc / 5.
template <bool SEQ>
__global__ __launch_bounds__(256) void entity_encode_bwd_kernel(int variant, const float* __restrict__ dee,
                                                                const float* __restrict__ ent, int cols,
                                                                const float* __restrict__ ee,
                                                                const float* __restrict__ word_emb, int vocab,
                                                                float* __restrict__ dtype_emb, int ntypes,
                                                                float* __restrict__ dword, int B, int K, int d) {
    if (!SEQ) chain_priority();
    const ScatterWalk<SEQ> w(B * K);
    for (int row = w.row; row < w.row_end; ++row) {
        const EntityIndex ix = entity_index(variant, ent + (int64_t)row * cols, ntypes, vocab);
        // ordered form: a row none of whose destinations this workgroup owns costs no further loads
        bool mine = w.owns(ix.type);
        if (variant == ICK_NEWS && dword != nullptr) {
#pragma unroll
            for (int q = 0; q < 5; ++q) mine = mine || w.owns(ix.name[q]);
        }
        if (!mine) continue;
        for (int c = w.col; c < d; c += w.col_step) {
            float g = dee[(int64_t)row * d + c];
            if (variant == ICK_NEWS) {
                float s = 0.f;
#pragma unroll
                for (int q = 0; q < 5; ++q) s += word_emb[(int64_t)ix.name[q] * d + c];
                const float avg = s / 5.0f;
                // enc = ee / avg is not recoverable when avg == 0; recompute enc's trainable part instead
                const float enc_g = g * avg;                       // gradient wrt the un-scaled encoding
                if (dword) {
                    // d avg = g * enc ; enc = ee / avg when avg != 0, and the product ee is what we stored
                    const float enc = avg != 0.f ? ee[(int64_t)row * d + c] / avg : 0.f;
                    const float gw = g * enc / 5.0f;
#pragma unroll
                    for (int q = 0; q < 5; ++q) w.add(dword + (int64_t)ix.name[q] * d + c, ix.name[q], gw);
                }
                g = enc_g;
            }
            if (c >= ix.type_off)
                w.add(dtype_emb + (int64_t)ix.type * (d - ix.type_off) + (c - ix.type_off), ix.type, g);
        }
    }
}

// FactEncoder backward: f = ee[subject] + pred_emb[predicate]
template <bool SEQ>
__global__ __launch_bounds__(256) void fact_encode_bwd_kernel(const float* __restrict__ dfe,
                                                              const int64_t* __restrict__ facts, float* __restrict__ dee,
                                                              float* __restrict__ dpred, int num_pred, int B, int K,
                                                              int F, int d) {
    if (!SEQ) chain_priority();
    const ScatterWalk<SEQ> w(B * F);
    for (int row = w.row; row < w.row_end; ++row) {
        const FactPair f = fact_pair(facts, row, K, num_pred);
        const int64_t erow = (int64_t)(row / F) * K + f.subj;
        if (!w.owns(erow) && !w.owns(f.pred)) continue;
        for (int c = w.col; c < d; c += w.col_step) {
            const float g = dfe[(int64_t)row * d + c];
            w.add(dee + erow * d + c, erow, g);
            w.add(dpred + (int64_t)f.pred * d + c, f.pred, g);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// Pointer-score backward.  s[b,t,k] = ind * sum_d h*ctx*w + bias
//   dh[b,t,:]   += sum_k ds*ind * ctx[b,k,:] * w        (one workgroup per (b,t))
//   dctx[b,k,:] += sum_t ds*ind * h[b,t,:] * w          (one workgroup per (b,k))
//   dw          += sum ds*ind * h * ctx ;  dbias += sum ds
// Packed form (ick_pointer_scores_bwd_packed; rowmap / rowstart of ick_head_rowmap): ds holds the packed rows of the
// valid positions only -- sample b's are rows rowstart[b] .. rowstart[b + 1] - 1 in position order -- while h, ind, dh keep
// their logical rows.  The dh kernel's workgroup m takes packed row m (logical row rowmap[m]) and exits past the row count
// rowstart[B]; the dctx kernel reads a zero gradient for the positions beyond a sample's rows.
// ---------------------------------------------------------------------------------------------
// (the roles are written once, as functions of the workgroup's place in its role's own grid: the two-launch entry points
// run each as a kernel of its own, the fused ones as workgroup ranges of one launch)
__device__ __forceinline__ void pointer_bwd_dh_role(int bx, int by, int B, const float* __restrict__ ds, int64_t ds_ld,
                                                    int col0, const float* __restrict__ ctx, const float* __restrict__ w,
                                                    const float* __restrict__ ind, float* __restrict__ dh, int T, int Kc,
                                                    int d, const int32_t* __restrict__ rowmap,
                                                    const int32_t* __restrict__ count) {
    int b = by, t = bx;
    int64_t dsrow = (int64_t)b * T + t;
    if (rowmap != nullptr) {     // uniform
        if (dsrow >= device_bound(B * T, count)) return;
        const int lr = rowmap[dsrow];
        b = lr / T;
        t = lr - b * T;
    }
    const float* dsr = ds + dsrow * ds_ld + col0;
    for (int c = threadIdx.x; c < d; c += 256) {
        float acc = 0.f;
        const float* cc = ctx + (int64_t)b * Kc * d + c;
        int k = 0;
        for (; k + 8 <= Kc; k += 8) {        // eight context rows in flight
            float v[8], g[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                v[q] = cc[(int64_t)(k + q) * d];
                g[q] = dsr[k + q];
                if (ind) g[q] *= ind[((int64_t)b * T + t) * Kc + k + q];
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) acc = fmaf(g[q], v[q], acc);
        }
        for (; k < Kc; ++k) {
            float g = dsr[k];
            if (ind) g *= ind[((int64_t)b * T + t) * Kc + k];
            acc = fmaf(g, cc[(int64_t)k * d], acc);
        }
        dh[((int64_t)b * T + t) * d + c] += acc * w[c];
    }
}

__global__ __launch_bounds__(256) void pointer_bwd_dh_kernel(const float* __restrict__ ds, int64_t ds_ld, int col0,
                                                             const float* __restrict__ ctx, const float* __restrict__ w,
                                                             const float* __restrict__ ind, float* __restrict__ dh,
                                                             int T, int Kc, int d, const int32_t* __restrict__ rowmap,
                                                             const int32_t* __restrict__ count) {
    chain_priority();
    pointer_bwd_dh_role(blockIdx.x, blockIdx.y, gridDim.y, ds, ds_ld, col0, ctx, w, ind, dh, T, Kc, d, rowmap, count);
}

// One workgroup per (sample, 64 columns): the (T x Kc) score gradients of the sample sit in LDS, lane <-> column,
// the four waves share the Kc context rows.  d w and d bias leave the workgroup as one float atomic per column /
// one per sample (a workgroup per (sample, row) made 1280 workgroups fight over the same 300 addresses: 59 us).
// SEQ (deterministic mode): one workgroup per column block walks the samples in order and adds its d w / d bias terms
// with plain read-modify-writes instead of one float atomic per sample.
// kBatch (the fused launch): a lane's T hidden values are loaded eight at a time into registers before the first of
// them is used; the products enter acc in the same order, t = 0 .. T - 1.
template <bool SEQ, bool kBatch>
__device__ __forceinline__ void pointer_bwd_dctx_role(int bx, int by, float* gs, const float* __restrict__ ds,
                                                      int64_t ds_ld, int col0, const float* __restrict__ h,
                                                      const float* __restrict__ ctx, const float* __restrict__ w,
                                                      const float* __restrict__ ind, float* __restrict__ dctx,
                                                      float* __restrict__ dw, float* __restrict__ dbias, int B, int T,
                                                      int Kc, int d, const int32_t* __restrict__ rowstart) {
    // gs: T * Kc gradients (indicator applied), 4 floats of scratch, 4 x 64 partial d w
    float* red = gs + T * Kc;
    float* dwp = red + 4;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int b = SEQ ? 0 : bx; b < (SEQ ? B : bx + 1); ++b) {
    float bsum = 0.f;
    // packed score gradients: the sample's nrow rows start at row0; the positions beyond them contribute exact zeros
    const int64_t row0 = rowstart ? rowstart[b] : (int64_t)b * T;
    const int nrow = rowstart ? min(T, rowstart[b + 1] - rowstart[b]) : T;
    for (int idx = threadIdx.x; idx < T * Kc; idx += 256) {
        const int t = idx / Kc, k = idx - t * Kc;
        float g = t < nrow ? ds[(row0 + t) * ds_ld + col0 + k] : 0.f;
        bsum += g;
        if (ind) g *= ind[((int64_t)b * T + t) * Kc + k];
        gs[idx] = g;
    }
    bsum = block_sum<4>(bsum, red);   // contains the barriers that publish gs
    if (threadIdx.x == 0 && by == 0) { if (SEQ) dbias[0] += bsum; else atomicAdd(dbias, bsum); }
    const int c = by * 64 + lane;
    const bool ok = c < d;
    const float* hb = h + (int64_t)b * T * d + (ok ? c : 0);
    const float wc = ok ? w[c] : 0.f;
    float dwl = 0.f;
    for (int k = wave; k < Kc; k += 4) {
        float acc = 0.f;
        if (kBatch) {
            int t = 0;
            for (; t + 8 <= T; t += 8) {
                float hv[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) hv[q] = hb[(int64_t)(t + q) * d];
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = fmaf(gs[(t + q) * Kc + k], hv[q], acc);
            }
            for (; t < T; ++t) acc = fmaf(gs[t * Kc + k], hb[(int64_t)t * d], acc);
        } else {
            for (int t = 0; t < T; ++t) acc = fmaf(gs[t * Kc + k], hb[(int64_t)t * d], acc);
        }
        if (ok) {
            const int64_t o = ((int64_t)b * Kc + k) * d + c;
            dctx[o] += acc * wc;
            dwl = fmaf(acc, ctx[o], dwl);
        }
    }
    dwp[wave * 64 + lane] = dwl;
    __syncthreads();
    if (wave == 0 && ok) {
        const float t = (dwp[lane] + dwp[64 + lane]) + (dwp[128 + lane] + dwp[192 + lane]);
        if (SEQ) dw[c] += t; else atomicAdd(dw + c, t);
    }
    if (SEQ) __syncthreads();          // the LDS buffers are rewritten for the next sample
  }
}

template <bool SEQ>
__global__ __launch_bounds__(256) void pointer_bwd_dctx_kernel(const float* __restrict__ ds, int64_t ds_ld, int col0,
                                                               const float* __restrict__ h, const float* __restrict__ ctx,
                                                               const float* __restrict__ w, const float* __restrict__ ind,
                                                               float* __restrict__ dctx, float* __restrict__ dw,
                                                               float* __restrict__ dbias, int B, int T, int Kc, int d,
                                                               const int32_t* __restrict__ rowstart) {
    chain_priority();
    extern __shared__ float gs[];
    pointer_bwd_dctx_role<SEQ, false>(blockIdx.x, blockIdx.y, gs, ds, ds_ld, col0, h, ctx, w, ind, dctx, dw, dbias, B, T, Kc,
                                      d, rowstart);
}

// Both roles in one launch (ick_pointer_scores_bwd_fused[_packed]): the two write disjoint outputs and read only what
// earlier launches wrote, so their workgroups run beside each other.  Workgroups [0, n_ctx) take the dctx role -- the
// longer one, dispatched first -- as (x = id % ctx_x, y = id / ctx_x) of its own grid; the rest take the dh role as
// (t = id % T, b = id / T).
template <bool SEQ>
__global__ __launch_bounds__(256) void pointer_bwd_fused_kernel(const float* __restrict__ ds, int64_t ds_ld, int col0,
                                                                const float* __restrict__ h, const float* __restrict__ ctx,
                                                                const float* __restrict__ w, const float* __restrict__ ind,
                                                                float* __restrict__ dh, float* __restrict__ dctx,
                                                                float* __restrict__ dw, float* __restrict__ dbias, int B,
                                                                int T, int Kc, int d, const int32_t* __restrict__ rowmap,
                                                                const int32_t* __restrict__ rowstart, int ctx_x,
                                                                int n_ctx) {
    chain_priority();
    extern __shared__ float gs[];
    const int id = blockIdx.x;      // uniform
    if (id < n_ctx) {
        pointer_bwd_dctx_role<SEQ, true>(id % ctx_x, id / ctx_x, gs, ds, ds_ld, col0, h, ctx, w, ind, dctx, dw, dbias, B, T,
                                         Kc, d, rowstart);
    } else {
        const int r = id - n_ctx;
        pointer_bwd_dh_role(r % T, r / T, B, ds, ds_ld, col0, ctx, w, ind, dh, T, Kc, d, rowmap,
                            rowstart ? rowstart + B : nullptr);
    }
}

// Predicate-gate backward (knowledge variants): gate[b,p,:] = bias + sum_{distinct active preds} W[:, pred]
// => dW[:, pred] += sum over positions where pred is active of dgate[b,p,:];  dbias += sum dgate.
// Activation and representatives are the gate tables context_indicators_kernel builds (context_index.h).
template <bool SEQ>
__global__ __launch_bounds__(256) void context_gate_bwd_kernel(const int64_t* __restrict__ captions,
                                                               const int64_t* __restrict__ facts,
                                                               const float* __restrict__ dgate, float* __restrict__ dw,
                                                               float* __restrict__ dbias, int B, int L, int T, int K, int F,
                                                               int V, int num_pred, int d, int mode) {
    extern __shared__ int smi[];
    const int tid = threadIdx.x;
  for (int b = SEQ ? 0 : blockIdx.x; b < (SEQ ? B : (int)blockIdx.x + 1); ++b) {
    const GateTables g = build_gate_tables(smi, captions, facts, b, L, K, F, V, num_pred, mode);
    const int *act = g.act, *pred = g.pred, *rep = g.rep;
    // suffix sums of dgate over positions, once per column (registers walk p = T-1 .. 0, LDS keeps suf[p]): a predicate
    // active from position a gets suf[a] = sum_{p >= a} dgate[b,p,c]  (was: T loads per (fact, column) pair)
    float* suf = reinterpret_cast<float*>(g.end);       // T * 256 floats
    const int c = blockIdx.y * 256 + tid;
    if (c < d) {
        float run = 0.f;
        for (int p = T - 1; p >= 0; --p) {
            run += dgate[((int64_t)b * T + p) * d + c];
            suf[p * 256 + tid] = run;
        }
        if (SEQ) dbias[c] += run; else atomicAdd(dbias + c, run);
        for (int j = 0; j < F; ++j) {
            if (!rep[j] || act[j] >= T) continue;
            float* dst = dw + (int64_t)c * num_pred + pred[j];             // fc_predicate.weight is (d, num_pred)
            if (SEQ) *dst += suf[act[j] * 256 + tid]; else atomicAdd(dst, suf[act[j] * 256 + tid]);
        }
    }
    if (SEQ) __syncthreads();          // the LDS tables are rebuilt for the next sample
  }
}

__global__ void counter_add_kernel(uint32_t* c, uint32_t inc, const float* flag) {
    if (flag == nullptr || flag[0] > 0.f) *c += inc;
}

__global__ __launch_bounds__(256) void scale_kernel(float* __restrict__ x, int64_t n, const float* __restrict__ num,
                                                    const float* __restrict__ den) {
    const float s = num[0] / den[0];
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) x[i] *= s;
}

}  // namespace
}  // namespace ick

using namespace ick;

extern "C" int ick_layernorm_bwd_rows_per_block(void) { return 8; }

extern "C" int ick_layernorm_bwd(const float* dy, const float* x, const float* res, const float* gamma,
                                 const float* mean, const float* rstd, float* dz, float* dgamma, float* dbeta,
                                 int64_t rows, int32_t d, float* dx_drop, float drop_p, uint32_t drop_seed,
                                 uint32_t drop_site, const uint32_t* drop_epoch, float* partials, void* stream) {
    ICK_CHECK_ARG(dy && x && gamma && mean && rstd && dz && rows > 0 && d > 0 && d <= 1024);
    ICK_CHECK_ARG(partials || (dgamma && dbeta));
    ICK_CHECK_ARG(partials || !deterministic());       // without a workspace the workgroups meet in float atomics
    ICK_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f && (drop_p == 0.f || dx_drop != nullptr));
    const int rpb = ick_layernorm_bwd_rows_per_block();   // two rows per wave: 160 workgroups for the 1280 rows of a layer (one row per wave measured slower: 10.0 vs 8.4 us)
    const DropArg dr{drop_p, drop_seed, drop_site, drop_epoch};
    float* dxd = dx_drop;   // written whenever given: dz * mask, or a plain copy of dz without dropout
    const dim3 grid(ceil_div(rows, rpb));
    const size_t sm = 8 * d * sizeof(float);
    hipStream_t s = (hipStream_t)stream;
    if (d <= 320)
        hipLaunchKernelGGL(layernorm_bwd_kernel<5>, grid, dim3(256), sm, s, dy, x, res, gamma, mean, rstd, dz, dgamma,
                           dbeta, rows, d, rpb, dxd, dr, partials);
    else if (d <= 512)
        hipLaunchKernelGGL(layernorm_bwd_kernel<8>, grid, dim3(256), sm, s, dy, x, res, gamma, mean, rstd, dz, dgamma,
                           dbeta, rows, d, rpb, dxd, dr, partials);
    else
        hipLaunchKernelGGL(layernorm_bwd_kernel<16>, grid, dim3(256), sm, s, dy, x, res, gamma, mean, rstd, dz, dgamma,
                           dbeta, rows, d, rpb, dxd, dr, partials);
    ICK_LAUNCH_RET();
}

extern "C" int ick_relu_bwd(const float* dy, const float* act, float* dx, int64_t n, float scale, void* stream) {
    ICK_CHECK_ARG(dy && act && dx && n > 0);
    hipLaunchKernelGGL(relu_bwd_kernel, dim3((int)std::min<int64_t>(ceil_div(n, 256), 2048)), dim3(256), 0,
                       (hipStream_t)stream, dy, act, dx, n, scale);
    ICK_LAUNCH_RET();
}

extern "C" int ick_colsum(const float* a, int64_t M, int32_t N, int64_t ld, float* out, void* stream) {
    ICK_CHECK_ARG(a && out && M > 0 && N > 0 && ld >= N);
    const int rpb = deterministic() ? (int)std::min<int64_t>(M, 1 << 30) : 64;     // one slab: no atomics between slabs
    ICK_CHECK_ARG(ceil_div(M, rpb) <= 65535);
    hipLaunchKernelGGL(colsum_kernel, dim3(ceil_div(N, 64), ceil_div(M, rpb)), dim3(256), 0, (hipStream_t)stream, a, M,
                       N, ld, out, rpb);
    ICK_LAUNCH_RET();
}

extern "C" int ick_caption_embed_bwd(const float* dx, const int64_t* captions, const int64_t* masks, float* dword,
                                     float* dee, float* dfe, int32_t B, int32_t L, int32_t K, int32_t F, int32_t V,
                                     int32_t d, int32_t pad_token, float scale, float drop_p, uint32_t drop_seed,
                                     uint32_t drop_site, const uint32_t* drop_epoch, void* stream) {
    ICK_CHECK_ARG(dx && captions && masks && dee && B > 0 && L > 0 && K > 0 && d > 0);
    if (deterministic())
        hipLaunchKernelGGL(caption_embed_bwd_kernel<true>, dim3(kDetParts, ceil_div(d, 256)), dim3(256), 0,
                           (hipStream_t)stream, dx, captions, masks, dword, dee, dfe, B, L, K, F, V, d, pad_token, scale,
                           DropArg{drop_p, drop_seed, drop_site, drop_epoch});
    else
        hipLaunchKernelGGL(caption_embed_bwd_kernel<false>, dim3(ceil_div((int64_t)B * L, 4)), dim3(256), 0, (hipStream_t)stream,
                           dx, captions, masks, dword, dee, dfe, B, L, K, F, V, d, pad_token, scale,
                           DropArg{drop_p, drop_seed, drop_site, drop_epoch});
    ICK_LAUNCH_RET();
}

extern "C" int ick_pointer_scores_bwd(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                      const float* w, const float* ind, float* dh, float* dctx, float* dw,
                                      float* dbias, int32_t B, int32_t T, int32_t Kc, int32_t d, void* stream) {
    return ick_pointer_scores_bwd_packed(ds, ds_ld, col0, h, ctx, w, ind, dh, dctx, dw, dbias, B, T, Kc, d, nullptr, nullptr,
                                         stream);
}

extern "C" int ick_pointer_scores_bwd_packed(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                             const float* w, const float* ind, float* dh, float* dctx, float* dw,
                                             float* dbias, int32_t B, int32_t T, int32_t Kc, int32_t d,
                                             const int32_t* rowmap, const int32_t* rowstart, void* stream) {
    ICK_CHECK_ARG(ds && h && ctx && w && dh && dctx && dw && dbias && B > 0 && B <= 65535 && T > 0 && Kc > 0 && d > 0);
    ICK_CHECK_ARG((rowmap == nullptr) == (rowstart == nullptr) && (int64_t)B * T <= INT32_MAX);
    // every argument check comes before the first launch: a rejected call leaves dh untouched as well
    const size_t smem = ((size_t)T * Kc + 4 + 256) * sizeof(float);
    ICK_CHECK_ARG(smem <= 64 * 1024);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pointer_bwd_dh_kernel, dim3(T, B), dim3(256), 0, s, ds, ds_ld, col0, ctx, w, ind, dh, T, Kc, d, rowmap,
                       rowstart ? rowstart + B : nullptr);
    if (deterministic())
        hipLaunchKernelGGL(pointer_bwd_dctx_kernel<true>, dim3(1, ceil_div(d, 64)), dim3(256), smem, s, ds, ds_ld, col0, h,
                           ctx, w, ind, dctx, dw, dbias, B, T, Kc, d, rowstart);
    else
        hipLaunchKernelGGL(pointer_bwd_dctx_kernel<false>, dim3(B, ceil_div(d, 64)), dim3(256), smem, s, ds, ds_ld, col0, h,
                           ctx, w, ind, dctx, dw, dbias, B, T, Kc, d, rowstart);
    ICK_LAUNCH_RET();
}

// The pair of launches above as ONE: the same sums in the same order, bit for bit.
extern "C" int ick_pointer_scores_bwd_fused_packed(const float* ds, int64_t ds_ld, int32_t col0, const float* h,
                                                   const float* ctx, const float* w, const float* ind, float* dh,
                                                   float* dctx, float* dw, float* dbias, int32_t B, int32_t T, int32_t Kc,
                                                   int32_t d, const int32_t* rowmap, const int32_t* rowstart,
                                                   void* stream) {
    ICK_CHECK_ARG(ds && h && ctx && w && dh && dctx && dw && dbias && B > 0 && B <= 65535 && T > 0 && Kc > 0 && d > 0);
    ICK_CHECK_ARG((rowmap == nullptr) == (rowstart == nullptr) && (int64_t)B * T <= INT32_MAX);
    const size_t smem = ((size_t)T * Kc + 4 + 256) * sizeof(float);
    ICK_CHECK_ARG(smem <= 64 * 1024);
    const int ctx_x = deterministic() ? 1 : B;
    const int64_t n_ctx = (int64_t)ctx_x * ceil_div(d, 64);
    ICK_CHECK_ARG(n_ctx + (int64_t)B * T <= INT32_MAX);
    const dim3 grid((unsigned)(n_ctx + (int64_t)B * T));
    hipStream_t s = (hipStream_t)stream;
    if (deterministic())
        hipLaunchKernelGGL(pointer_bwd_fused_kernel<true>, grid, dim3(256), smem, s, ds, ds_ld, col0, h, ctx, w, ind, dh,
                           dctx, dw, dbias, B, T, Kc, d, rowmap, rowstart, ctx_x, (int)n_ctx);
    else
        hipLaunchKernelGGL(pointer_bwd_fused_kernel<false>, grid, dim3(256), smem, s, ds, ds_ld, col0, h, ctx, w, ind, dh,
                           dctx, dw, dbias, B, T, Kc, d, rowmap, rowstart, ctx_x, (int)n_ctx);
    ICK_LAUNCH_RET();
}

extern "C" int ick_pointer_scores_bwd_fused(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                            const float* w, const float* ind, float* dh, float* dctx, float* dw,
                                            float* dbias, int32_t B, int32_t T, int32_t Kc, int32_t d, void* stream) {
    return ick_pointer_scores_bwd_fused_packed(ds, ds_ld, col0, h, ctx, w, ind, dh, dctx, dw, dbias, B, T, Kc, d, nullptr,
                                               nullptr, stream);
}

extern "C" int ick_entity_encode_bwd(int32_t variant, const float* dee, const float* entities, int32_t ent_cols,
                                     const float* ee, const float* word_emb, int32_t vocab, float* dtype_emb,
                                     int32_t ntypes, float* dword, int32_t B, int32_t K, int32_t d, void* stream) {
    ICK_CHECK_ARG(dee && entities && dtype_emb && B > 0 && K > 0 && d > 6);
    if (variant == ICK_NEWS) ICK_CHECK_ARG(ee && word_emb && vocab > 0);
    if (deterministic())
        hipLaunchKernelGGL(entity_encode_bwd_kernel<true>, dim3(kDetParts, ceil_div(d, 256)), dim3(256), 0,
                           (hipStream_t)stream, variant, dee, entities, ent_cols, ee, word_emb, vocab, dtype_emb, ntypes,
                           dword, B, K, d);
    else
        hipLaunchKernelGGL(entity_encode_bwd_kernel<false>, dim3(ceil_div((int64_t)B * K, 4)), dim3(256), 0, (hipStream_t)stream,
                           variant, dee, entities, ent_cols, ee, word_emb, vocab, dtype_emb, ntypes, dword, B, K, d);
    ICK_LAUNCH_RET();
}

extern "C" int ick_fact_encode_bwd(const float* dfe, const int64_t* facts, float* dee, float* dpred, int32_t num_pred,
                                   int32_t B, int32_t K, int32_t F, int32_t d, void* stream) {
    ICK_CHECK_ARG(dfe && facts && dee && dpred && B > 0 && K > 0 && F > 0 && d > 0);
    if (deterministic())
        hipLaunchKernelGGL(fact_encode_bwd_kernel<true>, dim3(kDetParts, ceil_div(d, 256)), dim3(256), 0, (hipStream_t)stream,
                           dfe, facts, dee, dpred, num_pred, B, K, F, d);
    else
        hipLaunchKernelGGL(fact_encode_bwd_kernel<false>, dim3(ceil_div((int64_t)B * F, 4)), dim3(256), 0, (hipStream_t)stream,
                           dfe, facts, dee, dpred, num_pred, B, K, F, d);
    ICK_LAUNCH_RET();
}

extern "C" int ick_context_gate_bwd(const int64_t* captions, const int64_t* facts, const float* dgate, float* dw,
                                    float* dbias, int32_t B, int32_t L, int32_t T, int32_t K, int32_t F, int32_t V,
                                    int32_t num_pred, int32_t d, int32_t mode, void* stream) {
    ICK_CHECK_ARG(captions && facts && dgate && dw && dbias && B > 0 && L > 0 && K > 0 && F > 0);
    ICK_CHECK_ARG((mode == 0 && T == L) || (mode == 1 && T == 1));
    const size_t smem = gate_table_ints(K, F) * sizeof(int) + (size_t)T * 256 * sizeof(float);    // + the suffix sums
    ICK_CHECK_ARG(smem <= 64 * 1024);
    if (deterministic())
        hipLaunchKernelGGL(context_gate_bwd_kernel<true>, dim3(1, ceil_div(d, 256)), dim3(256), smem, (hipStream_t)stream,
                           captions, facts, dgate, dw, dbias, B, L, T, K, F, V, num_pred, d, mode);
    else
        hipLaunchKernelGGL(context_gate_bwd_kernel<false>, dim3(B, ceil_div(d, 256)), dim3(256), smem, (hipStream_t)stream,
                           captions, facts, dgate, dw, dbias, B, L, T, K, F, V, num_pred, d, mode);
    ICK_LAUNCH_RET();
}

extern "C" int ick_scale_by_ratio(float* x, int64_t n, const float* num, const float* den, void* stream) {
    ICK_CHECK_ARG(x && num && den && n > 0);
    hipLaunchKernelGGL(scale_kernel, dim3((int)std::min<int64_t>(ceil_div(n, 256), 4096)), dim3(256), 0,
                       (hipStream_t)stream, x, n, num, den);
    ICK_LAUNCH_RET();
}

extern "C" int ick_counter_add(uint32_t* counter, uint32_t inc, void* stream) {
    ICK_CHECK_ARG(counter != nullptr);
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, inc, (const float*)nullptr);
    ICK_LAUNCH_RET();
}

extern "C" int ick_counter_add_if(uint32_t* counter, uint32_t inc, const float* flag, void* stream) {
    ICK_CHECK_ARG(counter != nullptr && flag != nullptr);
    hipLaunchKernelGGL(counter_add_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, counter, inc, flag);
    ICK_LAUNCH_RET();
}
