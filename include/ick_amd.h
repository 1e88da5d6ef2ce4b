/*
 * ick_amd.h -- C ABI of libick_amd.so: the MI355X (gfx950) caption-decoder hot path of
 * sonniki/image-captioning-with-external-knowledge.
 *
 * The reference has no FFI layer: its boundary for this path is the Python API of
 * <variant>/models.py.  The entry points below are the op boundaries of
 * SURVEY.md §8(a) rows a1-a14 that the package's Python `models` shim binds through ctypes;
 * each comment names the reference call site it replaces (paths relative to the reference
 * root).  Conventions:
 *   - every pointer is a DEVICE pointer to fp32 / int32 / int64 data owned by the caller
 *     (PyTorch's caching allocator in the shipped binding); nothing is allocated or freed here;
 *   - every entry takes the hipStream_t (as void*) to launch on and returns 0 on success,
 *     a negative ICK_E* code for argument errors, or a positive hipError_t;
 *   - all activations are batch-major, row-major fp32: (B, T, d) with d contiguous;
 *   - no entry synchronises the stream or the device.
 */
#ifndef ICK_AMD_H
#define ICK_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ICK_OK 0
#define ICK_EINVAL (-1)   /* bad shape / null pointer / unsupported size */
#define ICK_EALIGN (-2)   /* pointer or stride violates an alignment requirement */
#define ICK_EWORKSPACE (-3) /* workspace too small */

#define ICK_MAX_LAYERS 8

/* Library / device probe (no reference counterpart). */
int ick_version(void);
/* Deterministic mode: gradient reductions that otherwise use float atomics (scatter-adds of the embedding / entity /
 * fact / predicate-gate backward, bias and LayerNorm column sums) run in a fixed order -- slower, bit-reproducible.
 * Default: the environment variable ICK_DETERMINISTIC (1 = on).  Callers must also keep every GEMM unsplit
 * (split_k = 1) and the step on one stream; training.TrainStep(deterministic=True) does. */
int ick_set_deterministic(int on);
int ick_get_deterministic(void);
int ick_device_info(int* num_cu, int* wave_size, char* arch_name, int arch_name_len);

/* ------------------------------------------------------------------------------------------
 * Generic fp32 GEMM on the matrix cores:  C[m, n] = act( sum_k A(m,k) * B(n,k) + bias[n] )
 * Replaces every nn.Linear / 1x1 nn.Conv2d call site on the path:
 *   Encoder.conv1                         geo-aware/models.py:32,45
 *   MultiheadAttention in/out projections geo-aware/models.py:241-244 (torch.nn internals)
 *   linear1 / linear2 of the layers       geo-aware/models.py:241-244
 *   fc_vocab, fc_predicate                geo-aware/models.py:303; knowledge-aware/models.py:436-438
 * A element (m,k) lives at A[a_goff(m) + (m % a_grp) * a_rs + k * a_ks] with
 *   a_goff(m) = (a_gmap ? a_gmap[m / a_grp] : m / a_grp) * a_gs      (a_grp == 0: one group)
 * B element (n,k) at B[n * b_rs + k * b_ks];  C row m starts at
 *   C + (c_gmap ? c_gmap[m / c_grp] : m / c_grp) * c_gs + (m % c_grp) * c_rs.
 * Exactly one of (a_rs, a_ks) and one of (b_rs, b_ks) must be 1.
 * flags: bit0 = ReLU, bit1 = accumulate into C (C += ...), bit2 = atomic accumulate (split-K).
 * ReLU is rejected (ICK_EINVAL) with split_k > 1: the epilogue runs once per K slice, so it would
 * compute sum_z relu(partial_z) instead of relu(sum) -- like the gate, which is rejected there too.
 * Head-split epilogue (hs_dh > 0): the N columns are [segment][head][hs_dh] (packed q|k|v or
 * k|v-per-layer projections) and are scattered into the attention kernel's head-major layout
 *   C[ goff(m) + seg*(hs_H*hs_S*hs_dhp) + head*(hs_S*hs_dhp) + (hs_s0 + m % c_grp)*hs_dhp + j ]
 * i.e. per sample [segment][head][position][hs_dhp] with rows padded to hs_dhp floats (pad columns
 * are not written).  c_rs is ignored in this mode.
 */
typedef struct {
    const float* A; const float* B; float* C; const float* bias;
    int32_t M, N, K;
    int64_t a_rs, a_ks; int32_t a_grp; int64_t a_gs; const int32_t* a_gmap;
    int64_t b_rs, b_ks;
    int64_t c_rs; int32_t c_grp; int64_t c_gs; const int32_t* c_gmap;
    int32_t flags;
    int32_t split_k;       /* >1: K is split over blockIdx.z, partial sums added atomically */
    float   alpha;         /* scales the product before bias (1.0f normally) */
    int32_t hs_dh, hs_dhp, hs_H, hs_S, hs_s0;   /* head-split epilogue, see above (hs_dh == 0: off) */
    float drop_p; uint32_t drop_seed, drop_site; /* training dropout on the output (after bias/ReLU), see ick_dropout_mask */
    const uint32_t* drop_epoch;                  /* optional device counter added to drop_seed (graph replays) */
    int64_t a_extent, b_extent;   /* floats addressable from A / B (bounds of the buffer descriptors); 0 = derive from
                                     the strides -- required when a_gmap is given, otherwise the slow path is taken */
    float* colsum_a;              /* optional, k-major A only: colsum_a[m] += sum_k A(m,k) (float atomics) -- the bias
                                     gradient of a Linear rides on its weight-gradient GEMM (A = dY^T) */
    const float* gate;            /* optional (plain row-major C only): C[m,n] = gate[m*gate_rs + n] > 0 ? v * gate_scale : 0,
                                     applied last -- the ReLU (+ dropout) backward of the FFN rides on the data-gradient
                                     GEMM of linear2 (gate = the saved activation, gate_scale = 1/(1-p)) */
    int64_t gate_rs; float gate_scale;
    const void* b_ps;             /* optional: the pre-split copy of B (ick_presplit_weights of the same (N, K) matrix).  With
                                     it, and the split-bf16 product mode on, large problems run on the kernel that stages both
                                     operands by LDS-DMA and splits only the A fragments (csrc/gemm_ps.hip); B itself must
                                     still be valid (the other kernels read it).  The caller refreshes the copy whenever B
                                     changes (training: once per step, in the packing launches) */
    const int32_t* m_bound;       /* optional DEVICE scalar: only rows m < min(M, *m_bound) of the problem exist.  The grid
                                     stays sized for M; tiles at or past the bound exit before any load, the partial tile
                                     masks its rows, nothing beyond the bound is written.  Not with dropout / gate (both are
                                     keyed by the row number) or colsum_a. */
    const int32_t* k_bound;       /* optional DEVICE scalar: the reduction runs over k < K' = min(K, *k_bound); the K slices
                                     of a split-K problem partition [0, K') (slices past it exit), colsum_a sums K' rows.
                                     K' = 0: C and colsum_a stay untouched.  Both bounds are read once per workgroup through
                                     the scalar cache (training: the number of valid caption rows of a captured step, whose
                                     lengths are a device input -- the packed score head) */
    const int32_t* a_kmap;
    const int32_t* b_kmap;        /* optional DEVICE arrays of at least min(K, *k_bound) int32, k-major operands only (a_rs == 1 /
                                     b_rs == 1): reduction index k reads the operand's k line a_kmap[k] / b_kmap[k] instead of k
                                     (element (m, k) at A[... + a_kmap[k] * a_ks]).  k_bound keeps its meaning: the K slices
                                     partition [0, K'), colsum_a sums the K' gathered lines.  The entries must name lines inside
                                     a_extent / b_extent.  Not with b_ps (the pre-split copy is gathered when it is made:
                                     ick_presplit_item.k_map).  Training: the weight gradients of the decoder layers reduce over
                                     the valid caption rows of the logical (B * L)-row operands, DESIGN.md 3.1f */
} ick_gemm_args;

#define ICK_GEMM_RELU 1
#define ICK_GEMM_ACCUM 2
#define ICK_GEMM_ATOMIC 4
#define ICK_GEMM_COLSUM_ONLY 16   /* no product: colsum_a[m] += sum_k A(m,k) for a k-major A (B, C, N ignored) -- lets plain
                                    column sums (LayerNorm gamma/beta partials) ride in an ick_gemm_grouped launch */

int ick_gemm(const ick_gemm_args* args, void* stream);
/* The kernel configuration ick_gemm would launch for `args` (nothing is launched): workgroup tile, waves per
 * workgroup, tile grid, K split, operand layouts, 16-byte vector staging.  The parity tests assert through it that
 * the instantiation a benchmark quotes is the one they compared with the oracle. */
typedef struct {
    int32_t tile_m, tile_n, waves, tiles_m, tiles_n, split_k, a_kmajor, b_kmajor, vec;
    int32_t split_bf16;   /* 1: products formed as six bf16 x bf16 partial products of the exact three-way bf16 split of
                           * both fp32 operands, accumulated in fp32 (64x64 / 128x64 tiles); 0: v_mfma_f32_16x16x4_f32 */
    int32_t presplit;     /* 1: the B operand is read from its pre-split copy (b_ps): 64 x 320 or 128 x 128 tiles of
                           * csrc/gemm_ps.hip, both operands staged by LDS-DMA */
} ick_gemm_plan_info;
int ick_gemm_plan(const ick_gemm_args* args, ick_gemm_plan_info* out);
/* Process-wide mode of the split-bf16 product path of the large GEMM tiles.  0: every product on the exact fp32 MFMA
 * (v_mfma_f32_16x16x4_f32).  1 (DEFAULT; environment ICK_GEMM_SPLIT overrides): split products where they are faster (B
 * operand k-contiguous or pre-split: forward GEMMs, Encoder.conv1, the vocabulary data gradient).  2: for every large-tile
 * problem.  The split is exact (x = hi + mid + lo in bf16), six of the
 * nine partial products are formed; error against fp64 no larger than the exact path's (tests/test_gemm_split_gpu.py). */
int ick_set_gemm_split(int mode);
int ick_get_gemm_split(void);
/* Pre-split copies of weight matrices for ick_gemm's b_ps: the exact three-way bf16 split (hi + mid + lo) of the (N, K)
 * matrix whose element (n, k) is src[n * src_rs + k * src_cs] (one of the two strides must be 1: a weight or its
 * transposed view), stored as dst[K slice of 32][plane hi | mid | lo][row n, padded to a multiple of 64][32 k] bf16 with
 * zeros beyond N and K -- the image the matrix cores' B operand is read in.  ick_presplit_bytes gives the size of dst
 * (16-byte aligned).  One launch for up to 16 matrices.  Call sites: the weights of Encoder.conv1, of the all-layer cross
 * K/V projection and of fc_vocab (and fc_vocab's transposed view for its data gradient), geo-aware/models.py:32,241-242,303. */
typedef struct {
    const float* src; void* dst;
    int32_t N, K;
    int64_t src_rs, src_cs;
    const int32_t* k_map;     /* optional (src_rs == 1 only), device array: column k of the matrix is read from source column
                                 k_map[k] -- the transposed view of activation rows gathered through a row list */
    const int32_t* k_bound;   /* optional device scalar: columns k >= K' = min(K, *k_bound) do not exist: the 32-column slices
                                 below K' are written (zeros from K' up to the slice's end), the slices past it are left alone */
} ick_presplit_item;
int ick_presplit_bytes(int32_t N, int32_t K, int64_t* bytes);
int ick_presplit_weights(const ick_presplit_item* items, int32_t count, void* stream);
/* `count` (<= 64) independent problems; those that select the same kernel configuration share one launch (up to 8
 * per launch).  Used for the weight-gradient GEMMs of a layer (geo-aware/train.py:284 `loss.backward()`), each of
 * which alone is a latency-bound launch of a few hundred workgroups. */
int ick_gemm_grouped(const ick_gemm_args* problems, int32_t count, void* stream);

/* y[r,:] = LayerNorm(x[r,:] + res[r,:]) * gamma + beta   (res may be NULL), d <= 1024.
 * Replaces norm1/norm2/norm3 + the residual adds of Transformer{En,De}coderLayer
 * (torch/nn/modules/transformer.py post-LN path; built at geo-aware/models.py:241-244).
 * Optional outputs mean/rstd (rows) are kept for the backward pass. */
int ick_add_layernorm(const float* x, const float* res, const float* gamma, const float* beta,
                      float* y, int64_t rows, int32_t d, float eps,
                      int64_t x_ld, int64_t res_ld, int64_t y_ld,
                      float* save_mean, float* save_rstd,
                      float drop_p, uint32_t drop_seed, uint32_t drop_site, /* dropout applied to x (dropout1/2/3) */
                      const uint32_t* drop_epoch, void* stream);

/* Row-resident chain of a post-LN Transformer block, one launch instead of three (GEMM, add & norm, GEMM):
 *     o  = A W1^T + b1                                        (M x d;   A is M x K1)
 *     x  = LayerNorm(res + dropout1(o)) * gamma + beta         (M x d)
 *     y2 = act(x W2^T + b2), dropout2                          (M x N2;  optional: w2p == NULL stops after x)
 * i.e. what torch's TransformerDecoderLayer / TransformerEncoderLayer forward (post-LN) does between two attention
 * cores for the layers built at geo-aware/models.py:241-244, knowledge-aware/models.py:319-330:
 *   self_attn.out_proj -> dropout1 -> norm1 -> multihead_attn q-projection        (K1 = d,   N2 = d, head-split)
 *   multihead_attn.out_proj -> dropout2 -> norm2 -> linear1 + ReLU + dropout      (K1 = d,   N2 = FF)
 *   linear2 -> dropout3 -> norm3 -> the next layer's self_attn in_proj            (K1 = FF,  N2 = 3 d, head-split)
 * Weights are passed as PACKED copies of the nn.Linear weights (w1p of the (d, K1) weight, w2p of the (N2, d) one),
 * laid out for the kernel's operand loads and refreshed by ick_pack_weights after every optimizer step.
 * Row r of A at A + (r / a_grp) * a_gs + (r % a_grp) * a_rs (a_grp <= 0: r * a_rs); x and y2 likewise; with
 * hs_dh > 0 y2 is scattered head-major exactly like ick_gemm's head-split epilogue (y2_grp / y2_gs = c_grp / c_gs).
 * o, mean, rstd are optional outputs for the backward pass.  Dropout masks are those of ick_add_layernorm (drop1,
 * element index r * d + c) and of ick_gemm (drop2, r * N2 + c).  Limits: K1 <= 512, d <= 320, N2 <= 1024. */
typedef struct {
    const float* A; int64_t a_rs; int32_t a_grp; int64_t a_gs;
    int32_t M, K1, d;
    const float* w1p; const float* b1;
    const float* res; int64_t res_rs;
    const float* gamma; const float* beta; float eps;
    float drop1_p; uint32_t drop_seed, drop1_site; const uint32_t* drop_epoch;
    float* o; int64_t o_rs;
    float* x; int64_t x_rs; int32_t x_grp; int64_t x_gs;
    float* mean; float* rstd;
    const float* w2p; const float* b2; int32_t N2; int32_t flags;   /* flags: ICK_GEMM_RELU, ICK_CHAIN_SLIM, ICK_CHAIN_PROJ */
    float drop2_p; uint32_t drop2_site;
    float* y2; int64_t y2_rs; int32_t y2_grp; int64_t y2_gs;
    int32_t hs_dh, hs_dhp, hs_H, hs_S, hs_s0;
} ick_rowchain_args;
#define ICK_CHAIN_SLIM 256   /* ick_rowchain_fwd: 8-wave workgroups, for chains that run beside bulk GEMMs on another stream
                                (they find room on a busy CU where the 16-wave form waits for the bulk kernel to drain) */
#define ICK_CHAIN_PROJ 512   /* ick_rowchain_fwd: projection only, y2 = act(A W2^T + b2) with A (M, d); w1p / norm arguments unused */
int ick_rowchain_supported(int32_t K1, int32_t d, int32_t N2);
int ick_rowchain_fwd(const ick_rowchain_args* args, void* stream);

/* Backward of the row-resident chains, one launch for the data-gradient path between two attention-backward
 * kernels (what `loss.backward()`, geo-aware/train.py:284, runs for a post-LN Transformer block):
 *     dx        = dzin + g0 W0                  (g0: M x K0 gradient of the Linear that consumed the block's output,
 *                                                W0 its (K0, d) weight; either addend may be absent)
 *     dz1, do1  = LayerNorm'(dx)                 (ick_layernorm_bwd semantics: dz1 = gradient of the normalised sum and of
 *                                                the residual operand, do1 = dz1 * dropout mask = gradient of o1)
 *     t         = do1 W2, zeroed / scaled by the ReLU + dropout gate (ick_gemm's gate)     } FFN blocks only
 *     dx2       = dz1 + t W1                                                                } (w1p != NULL):
 *     dz2, do2  = LayerNorm'(dx2)                                                           } linear2, linear1, norm
 *     out3      = do W3                          (do = do2 for FFN blocks, do1 otherwise; W3 = the out-projection)
 *     dz_out    = dz2 (FFN blocks) or dz1
 * Weights are packed copies (ick_pack_weights) of the TRANSPOSED nn.Linear weights: w0p of W0^T (d x K0), w1p of
 * linear2.weight^T (N1 x d), w2p of linear1.weight^T (d x N1), w3p of out_proj.weight^T (d x d).
 * o / res / mean / rstd / gamma are the saved forward tensors of the norms (as for ick_layernorm_bwd); part1 / part2
 * receive the per-workgroup gamma / beta partial sums, ceil(M / 8) x 2d floats each (ick_layernorm_bwd's layout, 8 rows
 * per workgroup).  All row-major with dense rows (d, N1) except g0 / dzin (g0_rs, dzin_rs).
 * Limits: K0 <= 1920, d <= 320, N1 <= 512. */
typedef struct {
    int32_t M, d;
    uint32_t drop_seed; const uint32_t* drop_epoch;
    const float* g0; int64_t g0_rs; int32_t K0; const float* w0p;
    int32_t g0_grp; int64_t g0_gs;     /* g0_grp > 0: row r of g0 at g0 + (r / g0_grp) * g0_gs + (r % g0_grp) * g0_rs */
    const float* dzin; int64_t dzin_rs;
    const float* o1; const float* res1; const float* mean1; const float* rstd1; const float* gamma1;
    float drop1_p; uint32_t drop1_site;
    float* do1; float* part1;
    const float* w1p; int32_t N1; const float* act; float gate_scale; float* t_out;
    const float* w2p;
    const float* o2; const float* res2; const float* mean2; const float* rstd2; const float* gamma2;
    float drop2_p; uint32_t drop2_site;
    float* do2; float* part2;
    const float* w3p; float* out3;
    float* dz_out;
    int32_t flags;                     /* unused (0): the backward chain has one form, ICK_CHAIN_SLIM is ignored */
} ick_rowchain_bwd_args;
int ick_rowchain_bwd_supported(int32_t K0, int32_t d, int32_t N1);
int ick_rowchain_bwd(const ick_rowchain_bwd_args* args, void* stream);

/* Packed copy of an (N, K) matrix whose element (n, k) is src[n * src_rs + k * src_cs] (a weight: src_cs = 1; its
 * transpose, for the data-gradient chains: src_rs = 1, src_cs = the weight's row stride):
 *   dst[((slab * (K16 / 4) + k4) * 64 + l) * 4 + kk] = M[64 * slab + l][4 * k4 + kk]   (0 for rows >= N, k >= K),
 * K16 = K rounded up to 16, slabs = ceil(N / 64); dst holds *floats of ick_packed_weight_floats(N, K, &floats)
 * floats, 16-byte aligned.  count <= 48 matrices per launch. */
typedef struct {
    const float* src; float* dst; int32_t N, K; int64_t src_rs, src_cs;
    int64_t dst_rs;   /* 0: the packed layout above.  > 0: a plain copy dst[n * dst_rs + k] = src(n, k) riding in the same
                       * launch (the all-layer cross K/V weight / bias the step gathers from the layers' in_proj) */
} ick_pack_item;
int ick_packed_weight_floats(int32_t N, int32_t K, int64_t* floats);
int ick_pack_weights(const ick_pack_item* items, int32_t count, void* stream);

/* Multi-head attention core: O = softmax(Q K^T * scale [+ causal mask]) V per (batch, head).
 * Q element (b,t,h,j) at Q[b*q_bs + h*q_hs + t*q_ts + j]; K/V element (b,s,h,j) at
 * K[b*k_bs + h*k_hs + s*k_ss + j]; O element at O[b*o_bs + t*o_ts + h*dh + j] (row-major rows for the
 * output projection).  The head-major padded layout written by ick_gemm's head-split epilogue
 * (q_ts == k_ss == v_ss == 32, 16-byte aligned) takes the vectorised path.  kv_len (optional, int32[B]) limits
 * the keys of sample b to s < kv_len[b] (KV-cached greedy decode); q_pos0 is the absolute
 * position of query row 0 for the causal mask (key s visible iff s <= q_pos0 + t).
 * Replaces the scaled-dot-product core of nn.MultiheadAttention for
 *   decoder self-attention (causal), decoder cross-attention over [image ; entity ; fact] memory,
 *   context-encoder self-attention            geo-aware/models.py:348,358; knowledge-aware:495-496,508
 * lse (optional, B*H*T) receives log-sum-exp per query row for the backward pass. */
typedef struct {
    const float* Q; const float* K; const float* V; float* O; float* lse;
    int32_t B, H, T, S, dh;
    int64_t q_bs, q_hs, q_ts, k_bs, k_hs, k_ss, v_bs, v_hs, v_ss, o_bs, o_ts;
    float scale; int32_t causal; int32_t q_pos0; const int32_t* kv_len;
    float drop_p; uint32_t drop_seed, drop_site;   /* attention-weight dropout (training), element index ((b*H+h)*T+t)*S+s */
    const uint32_t* drop_epoch;
} ick_attn_args;
int ick_attention(const ick_attn_args* args, void* stream);

/* ------------------------------------------------------------------------------------------
 * Prefill gathers (rows a2-a5, a11).
 * variant: 0 geo, 1 knowledge, 2 news. */
#define ICK_GEO 0
#define ICK_KNOWLEDGE 1
#define ICK_NEWS 2

/* EntityEncoder.forward: geo-aware/models.py:82-104; knowledge-aware/models.py:82-133;
 * news-knowledge-aware/models.py:79-134.  entities (B,K,cols) fp32, facts (B,F,3) int64 (may be
 * NULL for geo), type_emb (ntypes, d-type_off), word_emb (V,d) (news only) -> out (B,K,d). */
int ick_entity_encode(int32_t variant, const float* entities, int32_t ent_cols, const int64_t* facts,
                      const float* type_emb, int32_t ntypes, const float* word_emb, int32_t vocab,
                      float* out, int32_t B, int32_t K, int32_t F, int32_t d, void* stream);

/* FactEncoder.forward: knowledge-aware/models.py:170-188. */
int ick_fact_encode(const int64_t* facts, const float* entities_encoded, const float* pred_emb,
                    int32_t num_pred, float* out, int32_t B, int32_t K, int32_t F, int32_t d, void* stream);

/* CaptionEmbedder.forward + `* sqrt(emb_dim)` + PositionEncoder (eval):
 * geo-aware/models.py:143-181,355-357,199-209; knowledge-aware/models.py:209-259.
 * captions/masks (B,L) int64; pos0 = absolute position of column 0 (greedy decode steps);
 * pe (max_len, d) sinusoid table.  out (B,L,d) = emb*scale + pe[pos0+l].  emb_out (optional)
 * receives the unscaled embedding rows (fixture stage "embeddings"). */
int ick_caption_embed(const int64_t* captions, const int64_t* masks, const float* word_emb,
                      const float* entities_encoded, const float* facts_encoded, const float* pe,
                      float* out, float* emb_out, int32_t B, int32_t L, int32_t K, int32_t F, int32_t V,
                      int32_t d, int32_t pad_token, float scale, int32_t pos0,
                      float drop_p, uint32_t drop_seed, uint32_t drop_site, /* PositionEncoder dropout (training) */
                      const uint32_t* drop_epoch, void* stream);

/* get_context_indicators: knowledge-aware/models.py:380-418.  Produces, per (b, position p):
 *   eib (B,T,F) 0/1: subject of fact j was mentioned before p (T==L) / anywhere so far (T==1)
 *   gate (B,T,d) = fc_predicate(predicate_indicator) = bias + sum over DISTINCT active predicates
 *   of fc_predicate.weight[:, pred]  (the dense (B,L,3000) indicator and its GEMM,
 *   knowledge-aware/models.py:436, are never materialised).  fc_pred_wt is the TRANSPOSED weight,
 *   (num_pred, d) row-major, so one predicate is one contiguous row.  gate may be NULL.
 * With fc_pred_wt == NULL and d == num_pred, `gate` receives the dense 0/1 predicate indicator (B,T,num_pred)
 *   itself (the public get_context_indicators method returns it).
 * mode 0: teacher-forced (strictly-before semantics), mode 1: predict (whole buffer). */
int ick_context_indicators(const int64_t* captions, const int64_t* facts, const float* fc_pred_wt,
                           const float* fc_pred_b, float* eib, float* gate, int32_t B, int32_t L,
                           int32_t T, int32_t K, int32_t F, int32_t V, int32_t num_pred, int32_t d,
                           int32_t mode, void* stream);

/* Pointer scores of get_scores (geo-aware/models.py:305-310; knowledge-aware/models.py:439-452):
 *   out[b,t,col0+k] = sum_d h[b,t,d]*ctx[b,k,d]*w[d] * (ind ? ind[b,t,k] : 1) + bias[0]
 * written in place into the concatenated score rows (row stride out_ld).  out_gmap (optional,
 * int32[B]) redirects sample b's rows to batch slot out_gmap[b]. */
int ick_pointer_scores(const float* h, const float* ctx, const float* w, const float* bias,
                       const float* ind, float* out, int32_t B, int32_t T, int32_t Kc, int32_t d,
                       int64_t out_ld, int32_t col0, const int32_t* out_gmap, void* stream);

/* Training dropout (nn.Dropout / MultiheadAttention(dropout=p) sites of the reference's layers): every
 * kernel that drops takes (p, seed, site); element `idx` of a site is kept iff
 * murmur3_fmix(idx * 0x9E3779B1 ^ (seed + site * 0x85EBCA6B)) >= p * 2^32 and scaled by 1/(1-p), so the
 * backward kernels regenerate the mask.  This entry writes that mask (rows x cols, idx = r*cols + c). */
int ick_dropout_mask(float* out, int64_t rows, int32_t cols, float p, uint32_t seed, uint32_t site, void* stream);

/* elementwise y = a * b  (vocab_input = h * gate, knowledge-aware/models.py:437) */
int ick_mul(const float* a, const float* b, float* y, int64_t n, void* stream);

/* Greedy selection of predict(): softmax -> argmax and runner-up per row
 * (geo-aware/models.py:410-419).  scores (B, Vx) row stride ld -> best/second int32[B]. */
int ick_top2(const float* scores, int64_t ld, int32_t B, int32_t Vx, int32_t* best, int32_t* second,
             void* stream);

/* One step of predict()'s token bookkeeping for B independent captions, entirely on device
 * (geo-aware/models.py:412-442; knowledge-aware/models.py:575-608): writes output[step],
 * applies the repeated-n-gram clean-up, marks finished captions, and emits the next input
 * token + mask.  output (B, max_len) int64 pre-filled with <pad>; top2_hist (B, max_len) int32;
 * finished (B) int32. */
int ick_greedy_update(const int32_t* best, const int32_t* second, int64_t* output, int32_t* top2_hist,
                      int32_t* finished, int64_t* next_token, int64_t* next_mask, int32_t B,
                      int32_t step, int32_t max_len, int32_t V, int32_t K, int32_t has_facts,
                      int32_t end_token, void* stream);
/* ick_top2 + ick_greedy_update in one launch (one workgroup per caption): the per-token selection of predict(). */
int ick_greedy_select(const float* scores, int64_t ld, int32_t B, int32_t Vx, int64_t* output, int32_t* top2_hist,
                      int32_t* finished, int64_t* next_token, int64_t* next_mask, int32_t step, int32_t max_len,
                      int32_t V, int32_t K, int32_t has_facts, int32_t end_token, void* stream);

/* ------------------------------------------------------------------------------------------
 * Fused decode step of predict() (geo-aware/models.py:389-443; knowledge-aware/models.py:545-608): one token
 * for R independent rows (R = captions x rows_per_sample; rows_per_sample > 1 = beams sharing their caption's
 * memory) in 3 launches per decoder layer + 2 (ick_decode_layers) + 1 (ick_decode_select_*), KV-cached.
 * A block's closing residual + LayerNorm is applied by the NEXT kernel while it loads its input row (see
 * csrc/decode.hip; the selection kernels are csrc/decode_select.hip); partial out-projection rows travel through
 * p1 / p2 / p3.  out_wt / w2t are the TRANSPOSED out_proj / linear2 weights ((in_features, d) row-major).  All buffers
 * are caller-owned device memory. */
typedef struct {
    const float *sa_in_w, *sa_in_b, *sa_out_wt, *sa_out_b, *n1_g, *n1_b;   /* self_attn, norm1 */
    const float *ca_in_w, *ca_in_b, *ca_out_wt, *ca_out_b, *n2_g, *n2_b;   /* multihead_attn (q rows used), norm2 */
    const float *w1, *b1, *w2t, *b2, *n3_g, *n3_b;                         /* linear1, linear2, norm3 */
    float *self_k, *self_v;           /* (R, H, max_len, 32) key / value cache of the caption positions */
    const float *cross_k, *cross_v;   /* this layer's key / value segment of the (B, 2*layers, H, S, 32) memory projection */
} ick_decode_layer;

typedef struct {
    int32_t R, rows_per_sample, d, H, FF, layers, S, max_len, V, K, F;
    int32_t end_token, pad_token;
    float ln_eps, emb_scale;          /* LayerNorm eps; sqrt(emb_dim) */
    int64_t kv_bs, scores_ld;         /* sample stride of the memory projection; row stride of `scores` */
    ick_decode_layer layer[ICK_MAX_LAYERS];
    const int32_t* anc;               /* optional (R, max_len): cache row holding position p of row r (beam search) */
    const float *wv, *bv, *we, *be, *wf, *bf;   /* fc_vocab, fc_entity, fc_fact (wf / bf NULL without facts) */
    const float *ee, *fe;             /* entities_encoded (B, K, d), facts_encoded (B, F, d) */
    const float *gate, *eib;          /* knowledge variants: (R, d) predicate gate and (R, F) indicator of this step */
    const float *word_emb, *pe;       /* word embedding (V, d), sinusoid table (>= max_len, d) */
    float *x0;                        /* (R, d) embedded input token of this step; select writes the next one */
    float *xa, *xb, *xc;              /* (R, d) residual rows between the blocks */
    float *p1, *p2, *p3;              /* (R, H, d), (R, H, d), (R, ceil(FF/64), d) partial out-projections */
    float *hfin, *hv;                 /* (R, d) decoder output h and h * gate */
    float *ptr;                       /* (R, K+F) pointer scores */
    float *cand;                      /* (R, ceil(V/16), 4) per-tile top-2 candidates {v1, idx1, v2, idx2} */
    float *scores;                    /* optional (R, scores_ld) vocabulary logits */
    int64_t *output;                  /* (R, max_len) generated tokens, pre-filled with <pad> */
    int32_t *hist, *finished, *n_done;/* (R, max_len) runner-ups; (R) ended flags; (1) number of ended rows */
    int64_t *next_token, *next_mask;  /* (R) */
    int64_t *cap_buf;                 /* optional (R, max_len) caption buffer read by ick_context_indicators */
    int32_t *sel_state;               /* optional (2, R, 12) workspace: with it (greedy, rows_per_sample == 1) ick_decode_layers
                                       * of position pos >= 1 chooses the token of step pos - 1 inside its first launch, and
                                       * ick_decode_select_greedy is only called for the last step */
} ick_decode_ctx;

/* 1 when the fused path handles these sizes (d % 4 == 0, 64 <= d <= 320, head width <= 32, S <= 1024,
 * max_len <= 128); callers fall back to the per-op launches otherwise. */
int ick_decode_supported(int32_t d, int32_t H, int32_t FF, int32_t S, int32_t max_len);
/* The launch plan of ick_decode_layers for R rows (rows_per_sample per caption) of a d / H / FF model, host only:
 * out[0] rows per workgroup of dec_self_kernel, out[1] 1 when a context with sel_state fuses the greedy selection
 * into it (rows_per_sample == 1), out[2] rows per workgroup of dec_cross_kernel, out[3] 1 when those rows share a
 * caption's K / V, out[4] rows per workgroup of dec_ffn_kernel, out[5] 1 for the merged score head + vocabulary
 * launch, out[6] 1 when some LayerNorm-on-load source has more rows than one sweep of its kernel.  ick_decode_layers
 * launches by the same function. */
int ick_decode_plan(int32_t R, int32_t rows_per_sample, int32_t d, int32_t H, int32_t FF, int32_t* out);
/* Decoder stack + score head for position `pos`: reads x0, leaves ptr / cand (/ scores / hfin). */
int ick_decode_layers(const ick_decode_ctx* ctx, int32_t pos, void* stream);
/* The same in two parts (part 1: the first self-attention block -- with sel_state the selection of the previous step --,
 * part 2: everything behind it; part 0 = ick_decode_layers): the knowledge variants run ick_context_indicators on the
 * caption buffer between the two. */
int ick_decode_layers_part(const ick_decode_ctx* ctx, int32_t pos, int32_t part, void* stream);
/* ick_decode_layers_part that also writes the cross-attention weights of step `pos`: softmax(q . k / sqrt(dh)) over
 * the S memory rows [P image ; K entity ; F fact] (the order of the cross K/V buffer), for every row, layer and head,
 * with the query of position pos (the one that produces output token pos).  attn: caller-owned fp32
 * (max_len, R, layers, H, S); this call fills attn[pos] (parts 0 and 2; part 1 launches no cross-attention).  Nothing
 * is written when every row has ended before the step (*n_done >= R), and rows that ended earlier are still written:
 * the caller zeroes the buffer before the decode and masks the steps after each row's <end> afterwards.
 * attn == NULL: exactly ick_decode_layers_part. */
int ick_decode_layers_attn(const ick_decode_ctx* ctx, float* attn, int32_t pos, int32_t part, void* stream);
/* One launch that initialises every per-call buffer of a decode: output = <pad>, history / flags / windows = 0,
 * caption buffer = <start>, *n_done = n_done_init, x0 = embedding of <start> at position 0. */
int ick_decode_init(const ick_decode_ctx* ctx, int32_t start_token, int32_t n_done_init, void* stream);
/* Greedy selection + predict()'s bookkeeping + embedding of the next input token into x0 (models.py:410-442). */
int ick_decode_select_greedy(const ick_decode_ctx* ctx, int32_t pos, void* stream);

/* Beam selection of one step (beam = ctx->rows_per_sample <= 8 hypotheses per caption, rows b*beam..): every live
 * hypothesis offers log_softmax(scores) + its cumulative log-probability for each of the V+K+F tokens, an ended one
 * offers itself unchanged; the best `beam` candidates of a caption (ties: lower hypothesis, lower token) become its
 * new rows.  Token histories, caption buffers and the cache-ancestry table (which cache row holds position p of row
 * r: ick_decode_ctx.anc of the NEXT step) are copied from the chosen parents (double buffered).  Needs ctx->scores.
 * The reference has no beam search (geo-aware/eval.py:61,83 decodes greedily): parity-unpinned; beam 1 is routed
 * to the pinned greedy path by the Python caller. */
typedef struct {
    float* cum; int32_t* fin;                       /* (R) cumulative log-probability (-inf: unused slot), ended flag */
    const int64_t* seq_in; int64_t* seq_out;        /* (R, max_len) */
    const int32_t* anc_in; int32_t* anc_out;        /* (R, max_len) */
    const int64_t* cap_in; int64_t* cap_out;        /* optional (R, max_len) */
    float* rec;                                     /* workspace (R, ceil((V+K+F)/1024), 18): per-chunk max / sum / best-k records */
    int32_t start_token;
} ick_beam_state;
int ick_decode_select_beam(const ick_decode_ctx* ctx, const ick_beam_state* beam, int32_t pos, void* stream);
/* 1 when ick_decode_select_beam handles `beam` hypotheses over Vx = V+K+F scores (beam <= 8 and
 * beam^2 * ceil(Vx / 1024) <= 4096 candidates); callers check this BEFORE capturing a decode graph. */
int ick_decode_beam_supported(int32_t Vx, int32_t beam);

/* Sampled selection of one step (csrc/sample.hip; DecoderTransformer.predict_sample): every live row draws its token
 * from the V+K+F scores (ctx->scores + ctx->ptr) -- temperature, top-k (ties at the boundary kept), top-p (smallest
 * prefix by strictly-greater mass), Gumbel-max with Philox-4x32-10 noise keyed by the seed, counter (c >> 2, step,
 * sample j = r % rows_per_sample, caption b = r / rows_per_sample) -- then does predict()'s bookkeeping (<end>,
 * finished / n_done, next token / mask, caption buffer, embedding of the next token into x0) WITHOUT the repeated
 * n-gram clean-up.  The knobs live in device memory (read with scalar loads), so a captured decode graph replays with
 * a new seed / temperature / top-k / top-p.  Rows of a caption share its cross K/V (rows_per_sample = samples,
 * anc = NULL: every row keeps its own self-attention cache).  Needs ctx->scores. */
typedef struct {
    const int64_t* seed;          /* (1) */
    const float* temp_top_p;      /* (2) temperature > 0, top_p in (0, 1] */
    const int32_t* top_k;         /* (1) 0 = off */
    float* log_prob;              /* optional (R, max_len): log_softmax(scores)[token] at T = 1; the caller zeroes it */
} ick_sample_state;
int ick_decode_select_sample(const ick_decode_ctx* ctx, const ick_sample_state* s, int32_t pos, void* stream);
/* 1 when ick_decode_select_sample handles Vx = V+K+F scores per row (Vx <= 65536) and rows_per_sample samples per
 * caption (<= 65535); host-only, callers check it BEFORE capturing a decode graph. */
int ick_decode_sample_supported(int32_t Vx, int32_t rows_per_sample);

/* Decoding rules of beam search and sampling.  At step t a row has generated y_0 .. y_{t-1}:
 *   no-repeat n-gram (n = words[0], 0..8, 0 = off): every y_p, n-1 <= p <= t-1, with y_{p-n+1..p-1} == y_{t-n+1..t-1}
 *     is banned (n = 1: every earlier token);
 *   min length (m = words[1], 0 = off): <end> is banned while t < m;
 *   length penalty (beam only, on when words[2] != 0): candidates are ranked by the fp32 key cum / lp[L], L = t + 1 for
 *     a live expansion, the length it ended at (<end> counted) for an ended hypothesis; len carries L with the parents.
 * A ban only removes candidates: the log-softmax normaliser still runs over all V+K+F scores, so cum and log_prob stay
 * the model's untruncated log-probabilities; in sampling banned columns are absent before top-k / top-p.  words, lp and
 * len are device memory read by the kernels at run time, so a captured decode graph replays with new rules; with every
 * word 0 the results are the bits of the entry points without rules.  Needs max_len <= 128; the caller keeps
 * V+K+F > max_len so that some column is always allowed. */
typedef struct {
    const int32_t* words;         /* (4) {no_repeat_ngram_size, min_len, length penalty on, 0}, 16-byte aligned */
    const float* lp;              /* (max_len + 1) lp[L] = ((5 + L) / 6)^alpha, fp32 (beam only) */
    int32_t* len;                 /* (R) beam only: hypothesis lengths, zeroed by the caller before step 0 */
} ick_decode_rules;
int ick_decode_select_beam_rules(const ick_decode_ctx* ctx, const ick_beam_state* beam, const ick_decode_rules* rules,
                                 int32_t pos, void* stream);
int ick_decode_select_sample_rules(const ick_decode_ctx* ctx, const ick_sample_state* s, const ick_decode_rules* rules,
                                   int32_t pos, void* stream);

/* Diverse beam search (Vijayakumar et al., AAAI 2018): the beam of a caption is split into `groups`
 * groups of k_g = beam / groups hypotheses, rows g*k_g .. (g+1)*k_g - 1 of the caption forming group g.  At each step
 * the groups choose in order g = 0 .. groups-1; group g ranks the candidates of its own rows by
 *   key - lambda * c(w),  c(w) = number of hypotheses of groups 0 .. g-1 that were expanded with column w at this step
 * (key: the ranking key of ick_decode_select_beam, or of ick_decode_select_beam_rules with rules; an ended hypothesis
 * competes with its key as it is, and carried or dead slots count for no column), and its k_g best (ties: lower
 * hypothesis, lower token) fill slots g*k_g + round.  The penalty only ranks: cum stays the raw summed log-probability.
 * The caller starts every group from the <start> hypothesis (cum = 0 at rows g*k_g, -inf elsewhere).  penalty is one
 * fp32 in device memory, read at run time, so a captured decode graph replays with a new lambda.  groups must divide
 * ctx->rows_per_sample; rules == NULL: no decoding rules. */
typedef struct {
    int32_t groups;               /* G >= 1, divides the beam */
    const float* penalty;         /* (1) lambda >= 0, fp32, device memory */
} ick_decode_diversity;
int ick_decode_select_beam_diverse(const ick_decode_ctx* ctx, const ick_beam_state* beam,
                                   const ick_decode_rules* rules /* NULL: no rules */,
                                   const ick_decode_diversity* div, int32_t pos, void* stream);

/* Constrained beam search (dynamic beam allocation, Post & Vilar, NAACL 2018, for single-column constraints; DESIGN.md
 * §3.2g): up to 8 forced columns per caption, ids in [0, V+K+F) (entity k: V + k, fact j: V + K + j), -1 = empty slot.
 * Every hypothesis carries the mask `met` of the slots whose column it has emitted (slots holding one id are met
 * together); its bank is the number of met slots.  <end> is closed to a hypothesis with an unmet slot.  At each step
 * every candidate (an ended hypothesis as it is, or a live hypothesis and a column the rules do not ban) has the bank
 * of the hypothesis it would make and the ranking key of ick_decode_select_beam(_rules); the k new hypotheses are taken
 * by visiting the banks n_req, n_req - 1, .., 0 (n_req = the caption's non-empty slots) and round again, each visit
 * taking that bank's best remaining candidate (ties: lower hypothesis, lower column) and skipping empty banks; slot i
 * receives the i-th candidate taken.  cum stays the raw summed log-probability.  With every slot empty this is
 * ick_decode_select_beam(_rules) bit for bit.  force is read at run time, so a captured decode graph replays with new
 * ids; the caller zeroes met before step 0 and picks the final best by (bank, key).  rules == NULL: no rules. */
typedef struct {
    const int32_t* force;         /* (R / rows_per_sample, 8) forced columns, -1 = empty, device memory */
    int32_t* met;                 /* (R) bit s: slot s met; zeroed by the caller before step 0 */
} ick_decode_constraints;
int ick_decode_select_beam_forced(const ick_decode_ctx* ctx, const ick_beam_state* beam,
                                  const ick_decode_rules* rules /* NULL: no rules */,
                                  const ick_decode_constraints* constraints, int32_t pos, void* stream);

/* Column bias: up to 64 (column, value) slots per caption, ids as ick_decode_constraints numbers
 * them, -1 = an empty slot (its value is not used); a value is a finite float or -inf.  If one id sits in two slots of a
 * row, the lowest slot counts.  cols and vals are read at run time, so a captured decode graph replays with new ids and
 * values.  The supported sizes are those of ick_decode_beam_supported / ick_decode_sample_supported.
 *   Beam: every hypothesis carries sum[r], the bias sum of the columns it has emitted.  Hypothesis j expanded with
 *     column w is ranked by (cum_j - lse_j + s_w + b_w) + sum_j, an ended hypothesis by cum_j + sum_j (each over its
 *     own lp[L] under a length penalty); lse runs over the raw scores of every column and cum stays the model's raw
 *     summed log-probability.  A column with b = -inf leaves the candidate pool as a banned column does, and a rule ban
 *     wins over any bias.  The caller zeroes sum before step 0 and picks the final best by the same key.
 *   Sampling: top-k, z = s' / T, the top-p weights (relative to the allowed maximum of s') and the Gumbel arg-max run on
 *     s' = s + b; a -inf column is absent like a rule-banned one (not counted in k, no mass).  The noise of a column and
 *     log_prob (log_softmax of the raw scores) do not change.
 * With every slot empty, or every value 0, the results are the bits of ick_decode_select_beam_rules /
 * ick_decode_select_sample_rules (rules == NULL: of the entries without rules).  Argument errors (a NULL pointer, sum
 * missing for the beam entry) return ICK_EINVAL without a launch. */
#define ICK_BIAS_MAX 64
typedef struct {
    const int32_t* cols;          /* (R / rows_per_sample, 64) column ids, -1 = empty slot; device memory */
    const float*   vals;          /* same shape; finite or -inf */
    float*         sum;           /* beam: (R) bias sum of every hypothesis, zeroed by the caller before step 0;
                                   * sampling: NULL */
} ick_decode_bias;
int ick_decode_select_beam_biased(const ick_decode_ctx* ctx, const ick_beam_state* beam,
                                  const ick_decode_rules* rules /* NULL: no rules */, const ick_decode_bias* bias,
                                  int32_t pos, void* stream);
int ick_decode_select_sample_biased(const ick_decode_ctx* ctx, const ick_sample_state* s,
                                    const ick_decode_rules* rules /* NULL: no rules */, const ick_decode_bias* bias,
                                    int32_t pos, void* stream);

/* Caption prefixes: cols[b][t] >= 0 is the column that every live row of caption b takes at step t (a
 * forced step), numbered as ick_decode_constraints numbers columns; -1 leaves step t free.  The table has max_len
 * columns whatever the prefixes' lengths and is read at run time, so a captured decode graph replays with new ids and
 * lengths.  The caller keeps <start>, <end> and <pad> out of it and fills a row's forced steps from step 0 on.
 *   A forced step: the only candidate of a live row is the forced column.  It wins over the rule bans (no n-gram or
 *     min-length ban is applied at that step) and over finite biases; the log-softmax normaliser still runs over every
 *     raw column, so cum (beam) and log_prob (sampling) hold the model's log-probability of the forced token.  The
 *     token counts as a generated one everywhere: n-gram history, length, the hypothesis' bias sum, the caption buffer,
 *     the embedding of the next step.  A -inf bias on a forced column is a contradiction the caller refuses: the row
 *     then has no candidate.
 *   Beam: a row offers one candidate, so a caption that starts from one live hypothesis (one per group with
 *     ick_decode_diversity) keeps one through its forced steps; the other slots stay unused (cum = -inf, counted in
 *     n_done), and the first free step fans out from that one parent as step 0 of a plain search does.  An ended
 *     hypothesis competes as it is.  The ban pass and the k arg-best rounds of stage 1 do not run at a forced step.
 *   Sampling: a forced step draws nothing (no top-k, top-p or noise).  The noise is keyed by (seed, caption, sample,
 *     step, column), so later steps draw what they would have drawn.
 * At a free step, and with a table that is all -1, the results are the bits of ick_decode_select_beam_rules / _diverse /
 * _biased and of ick_decode_select_sample_rules / _biased with the same arguments (rules == NULL: of the entries without
 * rules).  diversity and bias together, a NULL table and unsupported sizes return ICK_EINVAL without a launch. */
typedef struct {
    const int32_t* cols;   /* (R / rows_per_sample, max_len) forced column of step t, -1 = free; device memory */
} ick_decode_prefix;
int ick_decode_select_beam_prefix(const ick_decode_ctx* ctx, const ick_beam_state* beam,
                                  const ick_decode_rules* rules /* NULL: no rules */,
                                  const ick_decode_diversity* diversity /* NULL: one group */,
                                  const ick_decode_bias* bias /* NULL: no bias */, const ick_decode_prefix* prefix,
                                  int32_t pos, void* stream);
int ick_decode_select_sample_prefix(const ick_decode_ctx* ctx, const ick_sample_state* s,
                                    const ick_decode_rules* rules /* NULL: no rules */,
                                    const ick_decode_bias* bias /* NULL: no bias */, const ick_decode_prefix* prefix,
                                    int32_t pos, void* stream);

/* fused token-mean cross entropy over the packed rows of train.py
 * (pack_padded_sequence + CrossEntropyLoss(ignore_index=<pad>), geo-aware/train.py:275-281):
 * rows (b,t) with t < decode_len[b] and target != pad contribute.  Writes loss_sum[0] (sum of
 * token losses), count[0] (number of tokens) and, if dscores != NULL, the UNNORMALISED gradient
 * (softmax - onehot) for contributing rows and zeros elsewhere. */
int ick_packed_ce(const float* scores, int64_t ld, const int64_t* captions_sorted, const int32_t* decode_len,
                  int32_t B, int32_t L, int32_t Vx, int32_t pad_token, float* row_loss /* B*L workspace */,
                  float* loss_sum, float* count, float* dscores, void* stream);
/* ick_packed_ce with a per-caption weight (self-critical sequence training, Rennie et al. 2017: the policy gradient
 * -(r - b) * sum_t log p(w_t) is the cross entropy of the sampled caption weighted by its advantage).  Same rows as
 * ick_packed_ce; loss_sum[0] = sum_b weights[b] * sum_t loss(b, t), count[0] = the number of contributing tokens
 * (unweighted, as in ick_packed_ce), dscores = weights[b] * (softmax - onehot) on contributing rows and zeros elsewhere.
 * weights: (B,) fp32 on the device, any sign.  With weights == 1 every output is bit-identical to ick_packed_ce. */
int ick_packed_ce_weighted(const float* scores, int64_t ld, const int64_t* captions_sorted, const int32_t* decode_len,
                           const float* weights, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                           float* row_loss /* B*L workspace */, float* loss_sum, float* count, float* dscores,
                           void* stream);
/* Sampled token rows -> teacher-forced training rows (csrc/scst.hip).  tokens (R, T): the sampler's output (one row per
 * sample, <pad> after <end>).  Writes captions (R, T+1) = [<start>, w_1 .. w_m, <end>, <pad> ..] with lengths[r] = m + 2,
 * or [<start>, w_1 .. w_T] with length T + 1 when the row has no <end>; masks (R, T+1) = 2 for w >= V + K (has_facts),
 * 1 for w >= V, else 0 -- the rule predict() feeds tokens back with (knowledge-aware/models.py:600-606). */
int ick_samples_to_captions(const int64_t* tokens, int32_t R, int32_t T, int32_t V, int32_t K, int32_t has_facts,
                            int32_t start_token, int32_t end_token, int32_t pad_token, int64_t* captions, int64_t* masks,
                            int64_t* lengths, void* stream);

/* CIDEr-D on token ids, the reward of self-critical training (cider.py: CiderD; csrc/cider.hip).  The metric is
 * coco-caption's CIDEr-D applied to token ids:
 *   words of a row (candidate, reference, corpus alike): the tokens before the first end_token, without start_token,
 *     pad_token and the `ignore` ids (removal closes the gap: "a <pad> b" has the bigram "a b"); pointer ids (>= V)
 *     stay ids; a row without end_token uses all its tokens;
 *   n-grams n = 1..4 with their counts tf(g);
 *   df(g): the number of corpus images whose references, together, contain g; log_ref_len = log(corpus images);
 *   x_n(g) = tf(g) * (log_ref_len - log(max(1, df(g)))), norm ||x_n||_2;
 *   length: the row's BIGRAM count (coco-caption accumulates its length at n-index 1 -- kept as is);
 *   with one reference: s_n = sum over g in the candidate of min(x_n^c(g), x_n^r(g)) * x_n^r(g) / (|x_n^c| |x_n^r|),
 *     0 if either norm is 0, times exp(-(len_c - len_r)^2 / (2 sigma^2));
 *   score: the mean of s_n over n = 1..4, averaged over the image's M references, x 10 (range [0, 10]).
 * It equals coco-caption's CIDEr-D on the space-joined id strings, not on detokenised text.
 *
 * cand (N, T) int64 candidate rows; refs (B, M, Lr) int64, every one of the M rows of an image counts as a reference.
 * df table: df_keys (U, 4) uint32 n-grams (unused slots 0xFFFFFFFF), sorted lexicographically as unsigned, unique,
 * 16-byte aligned; df_count (U,) int32.  ignore: a HOST array of n_ignore <= 16 ids (copied into the launch).
 * Ids must lie in [0, 2^31 - 1) (others are read as their low 32 bits).
 * mode 0 (general): row i is scored against image image_index[i] (int32, (N,)); an index outside [0, B) gives NaN.
 * mode 1 / 2 (SCST layout): rows b * n + j (j < n = num_samples) are the samples of image b; mode 1 ("greedy") adds the
 *   greedy rows B * n + b (N = B * (n + 1)), mode 2 ("mean", n >= 2) has none (N = B * n).  Writes also
 *   advantages (B * n,) f32: mode 1 r_bj - r_greedy_b, mode 2 the leave-one-out mean r_bj - (sum_k r_bk - r_bj)/(n-1).
 * rewards (N,) f32.  Limits: T, Lr <= 64, M <= 16, rows per image (n or n + 1) <= 64, U >= 1.  fp32 with fixed-order
 * sums, no atomics: bit-reproducible. */
int ick_cider_d(const int64_t* cand, int32_t N, int32_t T, const int64_t* refs, int32_t B, int32_t M, int32_t Lr,
                const uint32_t* df_keys, const int32_t* df_count, int32_t U, float log_ref_len, float sigma,
                int32_t start_token, int32_t end_token, int32_t pad_token, const int32_t* ignore, int32_t n_ignore,
                int32_t mode, const int32_t* image_index, int32_t num_samples, float* rewards, float* advantages,
                void* stream);

/* BLEU-1..4, ROUGE-L and pointer precision / recall on token ids (metrics.py: CaptionMetrics; csrc/metrics.hip).  The
 * definitions are coco-caption's, applied to token ids:
 *   words of a row: ick_cider_d's words exactly (the same device code); c = the candidate's word count, l_m the word
 *     count of its reference m.
 *   BLEU components per candidate, n = 1..4 (bleu_scorer with option="closest"):
 *     guess_n = max(0, c - n + 1);
 *     correct_n = sum over the distinct candidate n-grams g of min(count_c(g), max_m count_m(g));
 *     testlen = c;  reflen = the l_m that minimises (|l_m - c|, l_m).
 *   sentence BLEU-n = (prod_{k<=n} (correct_k + 1e-15) / (guess_k + 1e-9)) ** (1/n), times exp(1 - 1/ratio) if
 *     ratio = (testlen + 1e-15) / (reflen + 1e-9) < 1.  Corpus BLEU-n: the same formula on the components' sums.
 *   ROUGE-L (Rouge, beta = 1.2): P = max_m LCS(c, r_m) / c, R = max_m LCS(c, r_m) / l_m (an empty reference gives 0),
 *     score (1 + beta^2) P R / (R + beta^2 P), 0 when P or R is 0 or c = 0.  Corpus: the mean over captions.
 *   pointers (pointer_base = V): generated = the distinct ids >= V among the candidate's words, reference = the
 *     distinct ids >= V in the union of its references' words, hits = the size of the intersection.  Corpus precision
 *     = sum hits / sum generated, recall = sum hits / sum reference, each 0 when its denominator is 0.  This is the
 *     id-level counterpart of the news variant's named-entity precision / recall in its "exact" mode.
 * Like ick_cider_d the scores equal coco-caption's on the space-joined id strings, not on detokenised text.
 *
 * cand (N, T) int64, refs (B, M, Lr) int64, ignore: a HOST array of n_ignore <= 16 ids; modes, image_index and
 * num_samples as for ick_cider_d (mode 0 general, 1 / 2 the SCST layout with / without the B greedy rows).
 * Outputs per row: counts (N, 10) int32 = guess1..4, correct1..4, testlen, reflen; bleu (N, 4) f32 sentence scores;
 * rouge_l (N,) f32; pointers (N, 3) int32 = hits, generated, reference (all zero when pointer_base < 0).  A row whose
 * image_index lies outside [0, B) gets NaN floats and zero counts.
 * Rewards (optional): weights, a HOST array of six floats w_base, w_b1..w_b4, w_rouge, and rewards (N,) f32 go together;
 * rewards = w_base * base_rewards + w_b1 * bleu1 + .. + w_b4 * bleu4 + w_rouge * rouge_l, evaluated in fp32 in this
 * order; base_rewards (N,) f32 (the rewards of a preceding ick_cider_d launch) may be null, then the first term is
 * absent.  In modes 1 / 2 rewards and advantages (B * n,) f32 go together, the advantages by ick_cider_d's formulas.
 * The sentence scores are evaluated in float64 and rounded once.  Limits: T, Lr <= 64, M <= 16, rows per image <= 64.
 * No atomics, fixed order: bit-reproducible. */
int ick_caption_metrics(const int64_t* cand, int32_t N, int32_t T, const int64_t* refs, int32_t B, int32_t M, int32_t Lr,
                        int32_t start_token, int32_t end_token, int32_t pad_token, const int32_t* ignore,
                        int32_t n_ignore, int32_t pointer_base, double beta, int32_t mode, const int32_t* image_index,
                        int32_t num_samples, const float* base_rewards, const float* weights, int32_t* counts,
                        float* bleu, float* rouge_l, int32_t* pointers, float* rewards, float* advantages, void* stream);

/* Totals of ick_caption_metrics' per-row outputs over N rows, written to the device: sums (13,) int64 = the ten BLEU
 * components and the three pointer counts, rouge_sum (1,) float64, captions (1,) int64 = the rows counted.  Rows whose
 * rouge_l is NaN (an image_index out of range) are skipped.  One workgroup, fixed order: bit-reproducible.  A validation
 * loop adds the totals of its batches on the device and reads them once. */
int ick_caption_metric_sums(const int32_t* counts, const float* rouge_l, const int32_t* pointers, int32_t N,
                            int64_t* sums, double* rouge_sum, int64_t* captions, void* stream);


/* ------------------------------------------------------------------------------------------
 * Training step (row a14): backward kernels behind loss.backward() of geo-aware/train.py:282-292,
 * and clip_gradient + Adam.step (geo-aware/utils.py:75-85, train.py:287-292).  Weight and data
 * gradients of the Linear layers are ick_gemm calls with k-major operands.
 */
/* Backward of ick_attention.  Q/K/V: the forward's head-major padded buffers (row stride 32 or 64
 * floats); O, dO row-major with (o_bs, o_ts); lse from the forward.  Outputs are row-major:
 * dQ element (b,t,h,j) at dQ[b*dq_bs + t*dq_ts + h*dh + j], dK/dV element (b,s,h,j) at
 * dK[b*dk_bs + s*dk_ss + h*dh + j].  When the queries do not fit one workgroup's LDS the key/value
 * gradients are accumulated with float atomics and dK/dV must be zero on entry. */
typedef struct {
    const float* Q; const float* K; const float* V; const float* O; const float* dO; const float* lse;
    float* dQ; float* dK; float* dV;
    int32_t B, H, T, S, dh;
    int64_t q_bs, q_hs, q_ts, k_bs, k_hs, k_ss, v_bs, v_hs, v_ss, o_bs, o_ts;
    int64_t dq_bs, dq_ts, dk_bs, dk_ss, dv_bs, dv_ss;
    float scale; int32_t causal; int32_t q_pos0;
    float drop_p; uint32_t drop_seed, drop_site;   /* must equal the forward's */
    const uint32_t* drop_epoch;
} ick_attn_bwd_args;
int ick_attention_bwd(const ick_attn_bwd_args* args, void* stream);
/* 1 when ick_attention_bwd writes every element of dQ / dK / dV for this shape (no pre-zeroing needed), 0 when it
 * accumulates query chunks with float atomics into buffers the caller must have zeroed. */
int ick_attention_bwd_overwrites(int32_t T, int32_t S, int32_t dh);
/* The launch plan of ick_attention (dir 0) / ick_attention_bwd (dir 1) for a (T, S, dh) problem, host only (nothing is
 * launched; both entry points choose their kernels by the same function, ICK_ATTN_NO_MFMA included).  head_major: Q / K /
 * V in the head-major padded layout (row stride 32 floats for dh <= 32, else 64; rows 16-byte aligned), which the
 * backward requires.  out[0] 1 for the matrix-core kernels (attention_mfma.hip), 0 for the general ones (attention.hip);
 * out[1] NQT (query tiles of 16) and out[2] MAXT (key tiles per wave) of the matrix-core instantiation, else 0; out[3] DHP
 * of the general instantiation (32 or 64), else 0; out[4] queries per workgroup; out[5] query chunks (workgroups per
 * (sample, head)); out[6] 1 when every element of the outputs is overwritten, 0 when the backward's chunks accumulate
 * dK / dV with float atomics (ick_attention_bwd_overwrites).  Returns ICK_EINVAL for what the entry point rejects. */
int ick_attention_plan(int32_t dir, int32_t T, int32_t S, int32_t dh, int32_t head_major, int32_t* out);

/* dz = dLN/d(x+res).  Parameter gradients: with `partials` == NULL, dgamma += ..., dbeta += ... (float atomics);
 * otherwise workgroup i writes its partial [dgamma | dbeta] sums to partials[i*2d .. i*2d+2d) for
 * i < ceil(rows / ick_layernorm_bwd_rows_per_block()) and the caller reduces them (ick_colsum), off the critical path. */
int ick_layernorm_bwd_rows_per_block(void);
int ick_layernorm_bwd(const float* dy, const float* x, const float* res, const float* gamma, const float* mean,
                      const float* rstd, float* dz, float* dgamma, float* dbeta, int64_t rows, int32_t d,
                      float* dx_drop /* optional: dz * mask = gradient of the dropped operand x (required when drop_p > 0; a copy of dz when drop_p == 0) */,
                      float drop_p, uint32_t drop_seed, uint32_t drop_site, const uint32_t* drop_epoch, float* partials,
                      void* stream);
/* dx = dy where the forward ReLU output `act` was positive, else 0. */
int ick_relu_bwd(const float* dy, const float* act, float* dx, int64_t n, float scale /* 1/(1-p) of the FFN dropout */,
                 void* stream);
/* out[n] += sum_m a[m*ld + n]  (bias gradients). */
int ick_colsum(const float* a, int64_t M, int32_t N, int64_t ld, float* out, void* stream);
/* Backward of ick_caption_embed: dx*scale is scatter-added to word_emb / entity / fact gradient rows. */
int ick_caption_embed_bwd(const float* dx, const int64_t* captions, const int64_t* masks, float* dword,
                          float* dee, float* dfe, int32_t B, int32_t L, int32_t K, int32_t F, int32_t V,
                          int32_t d, int32_t pad_token, float scale, float drop_p, uint32_t drop_seed,
                          uint32_t drop_site, const uint32_t* drop_epoch, void* stream);
/* Backward of ick_pointer_scores: ds = dscores[..., col0:col0+Kc] (row stride ds_ld);
 * dh += ..., dctx += ..., dw += ..., dbias += ... */
int ick_pointer_scores_bwd(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                           const float* w, const float* ind, float* dh, float* dctx, float* dw, float* dbias,
                           int32_t B, int32_t T, int32_t Kc, int32_t d, void* stream);
/* Backward of ick_entity_encode (type embedding; news: also the name-word embeddings). */
int ick_entity_encode_bwd(int32_t variant, const float* dee, const float* entities, int32_t ent_cols,
                          const float* ee, const float* word_emb, int32_t vocab, float* dtype_emb,
                          int32_t ntypes, float* dword, int32_t B, int32_t K, int32_t d, void* stream);
/* Backward of ick_fact_encode: dee[b, subject] += dfe, dpred_emb[predicate] += dfe. */
int ick_fact_encode_bwd(const float* dfe, const int64_t* facts, float* dee, float* dpred, int32_t num_pred,
                        int32_t B, int32_t K, int32_t F, int32_t d, void* stream);
/* Backward of the predicate gate of ick_context_indicators: dgate (B,T,d) ->
 * fc_predicate.weight.grad (d, num_pred) and bias.grad (d), accumulated. */
int ick_context_gate_bwd(const int64_t* captions, const int64_t* facts, const float* dgate, float* dw,
                         float* dbias, int32_t B, int32_t L, int32_t T, int32_t K, int32_t F, int32_t V,
                         int32_t num_pred, int32_t d, int32_t mode, void* stream);
/* ------------------------------------------------------------------------------------------
 * Global-norm gradient clipping and a learning-rate schedule on the device.
 *
 * The optimizer words: ICK_OPT_WORDS floats of device memory, 16-byte aligned, that the kernels below read and write
 * so that a captured optimizer graph follows new values without being captured again:
 *   [0] base learning rate                               (written by the host)
 *   [1] max_norm of the global-norm clip, <= 0: off      (written by the host)
 *   [2] norm: the L2 norm of the token-mean gradient g * gscale / *gscale_den over the whole bucket, before any clip
 *   [3] coef = min(1, max_norm / (norm + 1e-6)), 1 while max_norm <= 0 (torch.nn.utils.clip_grad_norm_, norm_type 2,
 *       error_if_nonfinite=False: a NaN norm gives a NaN coef)           ([2], [3], [5]: written by ick_grad_sqnorm)
 *   [4] the learning rate the last applied update used   (written by ick_adam_step[_derive] with words)
 *   [5] the sum of squares of the raw bucket g[0, n) that [2] was made from
 *   [6], [7] unused.
 * The schedule's shape is an argument (baked into a captured graph), defined on the 1-based step count t that the
 * Adam entries already take (step + *step_ptr), with W = warmup, N = total, r = min_ratio, base = words[0]:
 *   ICK_LR_CONSTANT      base * min(1, t / W)                                   (W = 0: base)
 *   ICK_LR_INVERSE_SQRT  base * min(t / W, sqrt(W / t))                         (W >= 1)
 *   ICK_LR_COSINE        t < W: base * t / W, else base * (r + (1 - r) * 0.5 * (1 + cos(pi * (min(t, N) - W) / (N - W))))
 *   ICK_LR_LINEAR        t < W: base * t / W, else base * (r + (1 - r) * (N - min(t, N)) / (N - W))       (both: N > W) */
#define ICK_OPT_WORDS 8
enum { ICK_LR_CONSTANT = 0, ICK_LR_INVERSE_SQRT = 1, ICK_LR_COSINE = 2, ICK_LR_LINEAR = 3 };
typedef struct ick_lr_schedule {
    int32_t kind, warmup, total;
    float min_ratio;
} ick_lr_schedule;
/* The launch plan of ick_grad_sqnorm for n floats: plan[0] = workgroups of the partial pass, plan[1] = floats one
 * workgroup takes per trip of its grid-stride loop, plan[2] = the most workgroups any n gets = the floats of scratch the
 * entry needs. */
int ick_grad_sqnorm_plan(int64_t n, int32_t* plan);
/* words[5] = sum of g[i]^2 over [0, n), words[2] and words[3] from it as above.  Two launches: plan[0] workgroups each
 * leave the partial sum of their float4 stream (plus, in workgroup 0, the n % 4 tail) in scratch, one workgroup then adds
 * the partials in a fixed order.  No atomics: the same input gives the same bits on every run, in and out of
 * deterministic mode.  With gscale_den (may be NULL) both launches do nothing while *gscale_den is not > 0, as the Adam
 * entries.  g 16-byte aligned; scratch_floats >= plan[2]. */
int ick_grad_sqnorm(const float* g, int64_t n, float gscale, const float* gscale_den, float* scratch,
                    int64_t scratch_floats, float* words, void* stream);
/* The optimizer: two entries, ick_adam_step over a flat fp32 bucket of n floats and ick_adam_step_derive over a cover
 * of the whole bucket (below).  The base update, with every option pointer NULL:
 *     g = clamp(g * gscale [/ *gscale_den], +-clip)   (clip <= 0: no clamp),  then torch.optim.Adam's update of p, m, v
 * with the host rate lr (default betas / eps semantics, no amsgrad).  The 1-based step count is t = step + *step_ptr
 * (step_ptr may be NULL; a device-resident counter lets a captured graph advance the bias correction on every replay).
 * With gscale_den (device scalar, may be NULL) the gradient scale is gscale / *gscale_den: the token-mean normalisation
 * by the all-reduced token count without a host round trip or a separate pass over the bucket.  While *gscale_den is not
 * > 0 nothing at all is written, whatever the options.  The gradient written back is the clamped one.
 *
 * The cover (ick_adam_step_derive): the same update, one function in csrc/adam.hip and the same bits in p, g, m, v,
 * which ALSO keeps the re-laid-out copies of the weights current that the next step's kernels read (geo-aware/train.py:292
 * optimizer.step() is the only writer of the parameters, so the packed / transposed / bf16-plane images need no launches
 * of their own: round 4 spent 126 us of kernel time per cfg2 step on ick_pack_weights + ick_presplit_weights).  The
 * bucket is cut into workgroup-sized `blocks`:
 *   - a flat run of <= 1024 float4 (item < 0), optionally mirrored into a plain copy (the gathered cross K/V bias);
 *   - a 64 x 64 tile of an `item`: `rows` x K floats, row-major with row stride K, starting `off` floats into the
 *     bucket, which are rows drow0 .. drow0 + rows - 1 of a logical (Nd, K) matrix W.  The tile (tn, tk) covers rows
 *     64 tn .. 64 tn + 63 of W and columns 64 tk .. 64 tk + 63; after the update its new values are written to every
 *     non-NULL image of W: `pack` = ick_pack_weights(W), `pack_t` = ick_pack_weights(W^T), `copy` = W with row stride
 *     copy_ld, `ps` = ick_presplit_weights(W), `ps_t` = ick_presplit_weights(W^T), `tr` = W^T with row stride tr_ld.
 *     The images must have been filled once by those entry points (their zero padding is never rewritten).
 *     Constraints: K % 4 == 0, off % 4 == 0; pack_t needs drow0 % 4 == 0 and rows % 4 == 0; ps_t needs drow0 % 8 == 0
 *     and rows % 8 == 0; copy_ld % 4 == 0.
 * Every float of the bucket must lie in exactly one block (the caller builds the cover).  items / blocks are DEVICE
 * arrays.  The images stay images of p under every option.
 *
 * The options, each selected by one pointer and independent of the others; an option that is off leaves the bits of
 * the update without it:
 *   words != NULL  the optimizer words above: the rate is schedule(words[0], t) instead of lr (which is
 *       not read), and the gradient is multiplied by coef = words[3] between the scale and the clamp, as an operation of
 *       its own:  x = g * gscale [/ *gscale_den];  x = x * coef;  clamp.  words[4] receives the rate used.  With coef == 1
 *       and ICK_LR_CONSTANT, warmup 0, p, g, m, v are those of words == NULL with lr = words[0], bit for bit.  words ==
 *       NULL: sched is not read.
 *   e != NULL  an exponential moving average of the parameters in a fourth array laid out like p.  The
 *       lane that has made the new p updates e at the same offset, in this order of float32 operations:
 *           w = 1 - d_t;   e = e + w * (p_new - e)
 *       with d_t = *ema_decay (a DEVICE float: a captured graph follows a new value), or, with ema_warmup != 0,
 *       d_t = min(*ema_decay, (1 + t) / (10 + t)).  p, g, m, v keep the bits they have with e == NULL.
 *   decay != NULL, with decay_mask  weight decay on a per-parameter selection.  decay: a DEVICE float
 *       wd.  decay_mask: n_granules bytes on the device, one per 64 floats of the bucket counted from the bucket's start
 *       (p itself, whatever its address); the elements of a granule whose byte is non-zero decay, the others keep the
 *       bits they have with decay == NULL.  Every parameter of a bucket starts at a multiple of 64 floats, so a granule
 *       belongs to one parameter.  decay_form, in float32 operations kept apart:
 *         ICK_DECAY_DECOUPLED (torch.optim.AdamW)   once: f = 1 - lr_t * wd, lr_t the rate this update uses (lr, or with
 *                                                   words the scheduled rate);  per element: p = p * f, then the
 *                                                   unchanged update;
 *         ICK_DECAY_COUPLED (Adam(weight_decay=))   per element, x the gradient after scale, clip coefficient and clamp:
 *                                                   x2 = x + wd * p feeds the moments and the update; g is written back
 *                                                   as x.
 *   ticket != NULL  the launch also advances the step counter.  ticket: ONE uint32 in device memory, 0
 *       before the first launch; the launch leaves it 0 again.  Once every workgroup has read step_ptr[0], the last one
 *       to finish does step_ptr[0] += bump_inc -- iff the update ran, that is gscale_den == NULL or gscale_den[0] > 0,
 *       ick_counter_add_if's rule.  Everything else keeps the bits it has with ticket == NULL, where the counter is only
 *       read and bump_inc is not.
 * ICK_EINVAL without a launch: p, g, m or v NULL; n < 1, or blocks NULL or n_blocks < 1; step < 1 with step_ptr NULL;
 * words with an unknown schedule kind; e without ema_decay; ema_decay or a non-zero ema_warmup without e; decay and
 * decay_mask one without the other; with decay, an unknown decay_form, n_granules < ceil(n / 64) (flat form) or < 1
 * (derive form, whose cover lies on the device: there the kernel takes a granule beyond the table as not selected);
 * ticket without step_ptr.  ICK_EALIGN without a launch: e not on 4 bytes (flat form; like p, g, m, v it need not lie on
 * 16: the scalar kernel then runs); p, g, m, v or e not on 16 bytes (derive form). */
typedef struct ick_adam_item {
    int64_t off;
    int32_t rows, K, drow0, Nd;
    float* pack;
    float* pack_t;
    float* copy;
    void* ps;
    void* ps_t;
    float* tr;
    int64_t copy_ld, tr_ld;
} ick_adam_item;
typedef struct ick_adam_block {
    int32_t item, tn, tk, cnt4;
    int64_t off4;
    float* copy;
} ick_adam_block;
#define ICK_DECAY_DECOUPLED 0
#define ICK_DECAY_COUPLED 1
int ick_adam_step(float* p, float* g, float* m, float* v, float* e, int64_t n, float gscale, float clip, float lr,
                  float* words, ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step,
                  uint32_t* step_ptr, const float* gscale_den, const float* ema_decay, int32_t ema_warmup,
                  const float* decay, const uint8_t* decay_mask, int64_t n_granules, int32_t decay_form,
                  uint32_t bump_inc, uint32_t* ticket, void* stream);
int ick_adam_step_derive(float* p, float* g, float* m, float* v, float* e, const ick_adam_item* items,
                         const ick_adam_block* blocks, int32_t n_blocks, float gscale, float clip, float lr, float* words,
                         ick_lr_schedule sched, float beta1, float beta2, float eps, int32_t step, uint32_t* step_ptr,
                         const float* gscale_den, const float* ema_decay, int32_t ema_warmup, const float* decay,
                         const uint8_t* decay_mask, int64_t n_granules, int32_t decay_form, uint32_t bump_inc,
                         uint32_t* ticket, void* stream);
/* The weight and bias gradient of Encoder.conv1 (1x1 convolution) straight from the NCHW feature map:
 *     dw[o, c] = sum over b, p of d_img[b, p, o] * feats[b, c, p],     db[o] = sum over b, p of d_img[b, p, o].
 * d_img (B, P, d): the gradient of the image memory rows; feats (B, C, P): the feature map as it lies; dw (d, C): conv1's
 * weight layout; db (d); all float32, contiguous.  Any B, C, P, d >= 1 with B * P < 2^31 - 64; 16-byte loads where
 * d % 4 == 0 / P % 4 == 0 and the pointers allow, scalar loads otherwise.  Exact fp32 matrix products in every product mode.
 * Two launches: workgroups per (64 columns, group of reduction chunks, block of up to 304 rows) leave their partial
 * result in scratch, a second pass adds the groups in a fixed order.  No atomics: the same input gives the same bits on
 * every run, in and out of deterministic mode.  dw and db are OVERWRITTEN (they need not be zeroed; nothing is
 * accumulated into them).  ICK_EINVAL without a launch: a null pointer, a size < 1, scratch_floats too small.
 * ick_conv1_wgrad_plan: plan[0] = groups the reduction is split into, plan[1] = reduction indices per group, plan[2] =
 * column tiles, plan[3] = rows per row block; *scratch_floats = plan[0] * (d * C + d), the scratch the entry needs. */
int ick_conv1_wgrad_plan(int32_t B, int32_t C, int32_t P, int32_t d, int32_t* plan, int64_t* scratch_floats);
int ick_conv1_wgrad(const float* d_img, const float* feats, float* dw, float* db, int32_t B, int32_t C, int32_t P,
                    int32_t d, float* scratch, int64_t scratch_floats, void* stream);
/* *counter += inc on the stream (step / dropout-epoch counter of captured training graphs). */
int ick_counter_add(uint32_t* counter, uint32_t inc, void* stream);
/* ... only if *flag > 0 (device scalar): the step counter of a training step whose optimizer update is deferred into the
 * next step's graph advances exactly when that update is applied -- ick_adam_step[_derive] with gscale_den = flag is a
 * no-op under the same condition (no pending gradients: first call, or the update was flushed). */
int ick_counter_add_if(uint32_t* counter, uint32_t inc, const float* flag, void* stream);
/* n <= 8 device-to-device copies (src[i] -> dst[i], bytes[i]) in one launch; host arrays of device pointers. */
int ick_copy_batch(const void* const* src, void* const* dst, const long long* bytes, int n, void* stream);
/* Diagnostic: *out = device wall clock (100 MHz ticks) when the stream reaches this point. */
int ick_timestamp(unsigned long long* out, void* stream);
/* x *= num[0] / den[0] with device-resident scalars (token-mean normalisation without a host sync). */
int ick_scale_by_ratio(float* x, int64_t n, const float* num, const float* den, void* stream);

/* ------------------------------------------------------------------------------------------
 * Packed score head of the fused training step: the loss of geo-aware/train.py:275-281 only reads the
 * positions t < caption_length[b] - 1, and the decoder's causal self-attention (geo-aware/models.py:315-361, no
 * key-padding mask) lets no valid position read a padded one -- so the head (vocabulary projection, pointer scores, cross
 * entropy and their backward) runs over the packed list of valid rows only.  The list's length is known on the device
 * alone; every launch keeps a grid sized for B * L rows and its surplus workgroups exit at once.
 *
 * ick_head_rowmap (one workgroup): n_b = clamp(lengths[b] - 1, 0, L - 1);
 *   decode_len[b] = lengths[b] - 1 (int32, as the unpacked loss takes it), rowstart[b] = sum_{b' < b} n_b' (B + 1 entries:
 *   rowstart[B] = M', the number of valid rows -- the `count` of the entry points below), rowmap[m] = b * L + t for packed
 *   row m = rowstart[b] + t, t < n_b (sample-major, t ascending); entries m >= M' are set to 0 and never used. */
int ick_head_rowmap(const int64_t* lengths, int32_t B, int32_t L, int32_t* decode_len, int32_t* rowstart,
                    int32_t* rowmap, void* stream);
/* ick_pointer_scores over the packed rows: h / ind are indexed by the logical row rowmap[m], the scores go to columns
 * [col0, col0 + Kc) of PACKED row m of out (row stride out_ld), m < *count. */
int ick_pointer_scores_packed(const float* h, const float* ctx, const float* w, const float* bias, const float* ind,
                              float* out, int32_t B, int32_t T, int32_t Kc, int32_t d, int64_t out_ld, int32_t col0,
                              const int32_t* rowmap, const int32_t* count, void* stream);
/* ick_packed_ce[_weighted] (weights may be NULL) over packed score rows: row m < *count belongs to position
 * (b, t) = (rowmap[m] / L, rowmap[m] % L), its target is captions[b, t + 1] and its weight weights[b]; row_loss and
 * dscores are packed like the scores; rows >= *count are neither read nor written (nothing is zero-filled).
 * *count == 0: loss_sum = count_out = 0. */
int ick_packed_ce_packed(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                         const int32_t* count, const float* weights, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                         float* row_loss, float* loss_sum, float* count_out, float* dscores, void* stream);
/* The packed cross entropy with label smoothing (Szegedy et al. 2016; torch's CrossEntropyLoss(label_smoothing=eps);
 * DESIGN.md 3.1g).  For a contributing row with scores x[0 .. Vx), target t and lse = logsumexp(x):
 *     loss = (1 - eps) * (lse - x[t]) + eps * (lse - mean(x)),
 *     d loss / d x[c] = softmax(x)[c] - (1 - eps) * [c == t] - eps / Vx,
 * every column of the row counting, pointer columns included.  Which rows contribute, loss_sum, count_out, weights (may
 * be NULL) and the layout are those of the plain entries: with rowmap and count the scores are PACKED rows as in
 * ick_packed_ce_packed (decode_len is not read); with both NULL they are the (B, L) rows of ick_packed_ce[_weighted] and
 * decode_len is required.  eps: ONE float in device memory, 0 <= eps < 1, read by the kernel at run time -- a captured
 * launch follows a new value written to the word.  NULL eps: ICK_EINVAL.  With 0.0 in the word every output has the bits
 * of the plain entry of the same layout and weights. */
int ick_packed_ce_smooth(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                         const int32_t* count, const int32_t* decode_len, const float* weights, const float* eps,
                         int32_t B, int32_t L, int32_t Vx, int32_t pad_token, float* row_loss, float* loss_sum,
                         float* count_out, float* dscores, void* stream);
/* ick_pointer_scores_bwd reading PACKED score-gradient rows (sample b's rows are rowstart[b] .. rowstart[b + 1] - 1, in
 * position order); h, ind and dh keep their logical (B, T) rows; dh rows of padded positions are not touched. */
int ick_pointer_scores_bwd_packed(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                  const float* w, const float* ind, float* dh, float* dctx, float* dw, float* dbias,
                                  int32_t B, int32_t T, int32_t Kc, int32_t d, const int32_t* rowmap,
                                  const int32_t* rowstart, void* stream);
/* dst[m, :] = src[rowmap[m], :] for m < *count (d floats per row; grid sized for max_rows): the packed copy of the
 * activation rows for the weight-gradient kernels that cannot gather their k-major B operand (exact / deterministic
 * product modes; the pre-split kernel gathers in ick_presplit_weights instead). */
int ick_gather_rows(const float* src, int64_t src_rs, const int32_t* rowmap, const int32_t* count, float* dst,
                    int64_t dst_rs, int32_t max_rows, int32_t d, void* stream);

/* ------------------------------------------------------------------------------------------
 * The lean step's entries.  Every output has the bits of the entry it stands in for.
 *
 * ick_packed_ce_weighted_mean (weights may be NULL: ick_packed_ce), ick_packed_ce_packed_mean,
 * ick_packed_ce_smooth_mean: the reduction launch also writes mean[0] = loss_sum / count_out (0 when count_out is 0),
 *   so that a training step needs no launch of its own for the division.  NULL mean: ICK_EINVAL.
 * ick_pointer_scores_bwd_fused[_packed]: the dh and the dctx / dw / dbias workgroups of ick_pointer_scores_bwd[_packed]
 *   as ranges of ONE grid instead of two launches in series. */
int ick_packed_ce_weighted_mean(const float* scores, int64_t ld, const int64_t* captions, const int32_t* decode_len,
                                const float* weights, int32_t B, int32_t L, int32_t Vx, int32_t pad_token,
                                float* row_loss, float* loss_sum, float* count_out, float* dscores, float* mean,
                                void* stream);
int ick_packed_ce_packed_mean(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                              const int32_t* count, const float* weights, int32_t B, int32_t L, int32_t Vx,
                              int32_t pad_token, float* row_loss, float* loss_sum, float* count_out, float* dscores,
                              float* mean, void* stream);
int ick_packed_ce_smooth_mean(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                              const int32_t* count, const int32_t* decode_len, const float* weights, const float* eps,
                              int32_t B, int32_t L, int32_t Vx, int32_t pad_token, float* row_loss, float* loss_sum,
                              float* count_out, float* dscores, float* mean, void* stream);
int ick_pointer_scores_bwd_fused(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                 const float* w, const float* ind, float* dh, float* dctx, float* dw, float* dbias,
                                 int32_t B, int32_t T, int32_t Kc, int32_t d, void* stream);
int ick_pointer_scores_bwd_fused_packed(const float* ds, int64_t ds_ld, int32_t col0, const float* h, const float* ctx,
                                        const float* w, const float* ind, float* dh, float* dctx, float* dw,
                                        float* dbias, int32_t B, int32_t T, int32_t Kc, int32_t d, const int32_t* rowmap,
                                        const int32_t* rowstart, void* stream);

/* ------------------------------------------------------------------------------------------
 * Caption scoring: how likely a GIVEN caption is, from the packed score rows of the head above.
 *
 * ick_row_logprob_rank: one read of packed score row m < *count (position (b, t) = (rowmap[m] / L, rowmap[m] % L), target
 *   c* = captions[b, t + 1]) gives, at the LOGICAL element (b, t) of the (R, L - 1) outputs,
 *     token_log_prob = s[c*] - logsumexp(s),
 *     rank = #{c : s[c] > s[c*], or s[c] == s[c*] and c < c*}  (the target's place in a stable descending sort: 0 = argmax),
 *     best = the lowest column that holds the row's maximum.
 *   A target that is <pad> or outside [0, Vx) gives 0 / -1 / -1.  Elements of positions that are no packed row are not
 *   written here.  Vx <= 2^24, L >= 2, R <= 65535.
 * ick_caption_score_sums, after it: fills every element past a caption's valid rows (t >= rowstart[r + 1] - rowstart[r])
 *   with 0 / -1 / -1, log_prob[r] = the caption's token log-probabilities summed in position order, tokens[r] = how many
 *   were scored, and the totals over all captions in a fixed order (bit-identical from run to run): loss_sum = -sum of
 *   log-probabilities, count, top1_hits (rank == 0), topk_hits (rank < top_k), one float each. */
int ick_row_logprob_rank(const float* scores, int64_t ld, const int64_t* captions, const int32_t* rowmap,
                         const int32_t* count, int32_t R, int32_t L, int32_t Vx, int32_t pad_token, float* token_log_prob,
                         int32_t* rank, int32_t* best, void* stream);
int ick_caption_score_sums(const int32_t* rowstart, int32_t R, int32_t L, int32_t top_k, float* token_log_prob,
                           int32_t* rank, int32_t* best, float* log_prob, int32_t* tokens, float* loss_sum, float* count,
                           float* top1_hits, float* topk_hits, void* stream);

/* ------------------------------------------------------------------------------------------
 * Scheduled sampling (csrc/sched_sample.hip): the inputs of a training step's second pass, from the packed
 * score rows of a teacher-forced first pass (scores (M', ld), rowstart, decode_len: the packed head's and
 * ick_head_rowmap's).  captions / caption_masks (B, L) int64 are the gold rows; captions_in / masks_in (B, L) int64 and
 * replaced (B, L) int32 are written whole.  With n_b = clamp(decode_len[b], 0, L - 1), position (b, q) is eligible when
 * 1 <= q <= n_b - 1; packed row rowstart[b] + q - 1 predicts its token.  Every other position copies gold, replaced = 0.
 *   coin: x = element 0 of Philox-4x32-10 of counter (0xFFFFFFFF, *step, q - 1, b) under key (lo32(*seed), hi32(*seed));
 *     the position is replaced iff (x >> 8) + 0.5 < *prob * 2^24 (exact: 0 replaces nothing, 1 every eligible position).
 *   draw: argmax != 0: the lowest column that holds the row's maximum; else the first maximum of s[c] / *temperature +
 *     g_c in fp32, g_c the Gumbel noise of ick_decode_select_sample applied to element c & 3 of Philox of counter
 *     (c >> 2, *step, q - 1, b).  Columns start_token and pad_token never win.
 *   token: column c < V gives (c, 0), V <= c < V + K gives (c, 1), c >= V + K gives (c, 2) in (captions_in, masks_in):
 *     the rule of ick_samples_to_captions.
 * A position that is not replaced does not read its score row.  prob, temperature (float), seed (int64) and step
 * (uint32) are ONE word each in device memory, read at run time: a captured launch follows new values.  No atomics: the
 * same words give the same bits on every run.  F = 0 without facts.
 * ICK_EINVAL, without a launch: a NULL pointer or word, B < 1, L < 2, B * L > 2^31 - 1, V + K + F > 2^24, ld < V + K + F. */
int ick_sched_sample_mix(const float* scores, int64_t ld, const int32_t* rowstart, const int32_t* decode_len,
                         const int64_t* captions, const int64_t* caption_masks, int32_t B, int32_t L, int32_t V,
                         int32_t K, int32_t F, int32_t start_token, int32_t pad_token, const float* prob,
                         const float* temperature, const int64_t* seed, const uint32_t* step, int32_t argmax,
                         int64_t* captions_in, int64_t* masks_in, int32_t* replaced, void* stream);

/* ------------------------------------------------------------------------------------------
 * Geo-reference counts: the histograms of the geo variant's Jensen-Shannon metric (the reference's
 * JSGeoMetric.run / store_data_for_idx), on token ids.  One launch, one wave per caption row.
 *
 * Inputs: tokens (N, T) int64 caption rows, scanned whole (tokens after <end> are <pad> and never match); image_index
 *   (N) int32, row -> image; entities (B, K, C) float32, C >= 5, column 1 = distance, 2 = azimuth, 4 = type;
 *   entity_names (B, K, 2 + ICK_GEO_NAME_CHARS) int64 = [idx, length, chars...].
 * Terms: 0 near, 1 along, 2 across, 3 in, 4 north, 5 south, 6 east, 7 west.  trigger_ids: 8 HOST ints, the word id of
 *   each term's trigger (the azimuth words are north_of.. where the word map has north_of, else north..), -1 where the
 *   word map lacks it; of_id, the_id, a_id: the ids of "of", "the", "a", -1 when absent.  V = the word map's size.
 * Position i >= 1 with token t >= V counts when the previous token p0 < V and one of the windows holds:
 *     p0 is a trigger;  i >= 2, p1 is a trigger and p0 in {of, the, a};  i >= 3, p2 is a trigger, p1 == of and p0 in
 *     {the, a}  (the term is the trigger that matched),
 *   and k = t - V < K, and the effective name of entity k of the row's image does not contain the seven character codes
 *   of "unk_ent".  The effective name is the first min(length, 50) chars; a negative length gives all 50, 0 none.
 * A counted reference adds, in row `term` of `generated` (8, hist_ld) int32: +1 to column 0 (n_occurrences); terms 0-3:
 *   +1 to column 1 + b for the first distance bin b with lo_b <= (double)x < hi_b (nothing when no bin matches);
 *   terms 4-7: +1 to column 1 + 64 + b for the azimuth bin found the same way; terms 1-3: +1 to column 1 + 64 + 64 + x
 *   when the type x is an exact integer in [0, n_types).  bins_distance (n_distance, 2) / bins_azimuth (n_azimuth, 2):
 *   float64 [lo, hi] tables in DEVICE memory, at most ICK_GEO_MAX_BINS rows each.
 * `random` receives the same three increments for the random-entity baseline: entity s[j] where s = the slots of the
 *   image's non-unk_ent entities in slot order and j = x mod |s|, x = the .x word of Philox-4x32-10 of counter
 *   (i, lo32(r), hi32(r), 0), r = row_offset + n (n = the row's index in this launch), under key (lo32(seed), hi32(seed)).
 * marks (N, T) int32 is written whole by every launch: -1 where no reference is counted, else
 *   term << 24 | random entity << 12 | entity.  The histograms are ADDED to (integer atomics: the caller clears them; the
 *   totals do not depend on the order of the adds, so they are the same bits on every run and in deterministic mode).
 * A row whose image_index is outside [0, B) gets marks of -1 and no counts.
 * ICK_EINVAL: a null pointer, N, B, K, V, n_* < 1, T > ICK_GEO_MAX_T, K > ICK_GEO_MAX_K, C < 5, more than ICK_GEO_MAX_BINS
 *   bins, n_types > ICK_GEO_MAX_TYPES, hist_ld < 1 + 64 + 64 + n_types, an id >= V, row_offset < 0, generated == random. */
#define ICK_GEO_TERMS 8
#define ICK_GEO_NAME_CHARS 50
#define ICK_GEO_MAX_T 128
#define ICK_GEO_MAX_K 4095
#define ICK_GEO_MAX_BINS 64
#define ICK_GEO_MAX_TYPES 4096
int ick_geo_reference_counts(const int64_t* tokens, int32_t N, int32_t T, const int32_t* image_index,
                             const float* entities, const int64_t* entity_names, int32_t B, int32_t K, int32_t C,
                             int32_t V, const int32_t* trigger_ids, int32_t of_id, int32_t the_id, int32_t a_id,
                             const double* bins_distance, int32_t n_distance, const double* bins_azimuth,
                             int32_t n_azimuth, int32_t n_types, int64_t hist_ld, int64_t seed, int64_t row_offset,
                             int32_t* marks, int32_t* generated, int32_t* random, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ICK_AMD_H */
