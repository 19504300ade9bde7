/*
 * scream_hip.h -- C ABI of libscream_hip.so: the MI355X (gfx950) kernels behind the
 * SCREAM registration hot path.
 *
 * The reference (xujiabo/SCREAM) has no FFI/operator layer: its hot path is stock ATen
 * calls made from Python.  Each entry point below therefore cites the reference
 * *call site* (file:line under the reference checkout) whose arithmetic it replaces;
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add at that site.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is DEVICE memory owned by the caller
 *     unless the name ends in _host; kernels never allocate and keep no global state;
 *   - asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - returns 0 on success, a negative SCREAM_E* code on a rejected argument (checked on
 *     the host before any launch), or the positive hipError_t of a failed launch;
 *   - every input, output and accumulation is IEEE fp32 (fp64 only inside the 3x3 Kabsch solve; the split GEMMs hold their
 *     operands as exact sums of 16-bit planes inside the kernels, see scream_gemm_split_f32);
 *   - "rows" are points/tokens.  A *packed batch* holds several clouds back to back, each
 *     cloud starting on a 128-row boundary (SCREAM_ROW_TILE) and zero-padded to one, so a
 *     128-row tile never spans two clouds.
 */
#ifndef SCREAM_HIP_H
#define SCREAM_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCREAM_ROW_TILE 128
#define SCREAM_D_MODEL 256
#define SCREAM_NHEAD 8
#define SCREAM_HEAD_DIM 32
#define SCREAM_KV_CHUNK 256 /* tokens per partial K^T V reduction */

#define SCREAM_EINVAL (-1) /* bad size / alignment / NULL pointer */
#define SCREAM_EUNSUPPORTED (-2) /* shape outside what the gfx950 kernels are built for */

/* GEMM epilogues (models/transformer.py:79-88, models/pointnet.py:27-33) */
enum {
    SCREAM_EPI_NONE = 0,      /* C = A W^T */
    SCREAM_EPI_ELU1 = 1,      /* columns < n_act: elu(x)+1 (transformer.py:7-8,28-29); rest plain */
    SCREAM_EPI_RELU = 2,      /* relu (transformer.py:66) */
    SCREAM_EPI_BIAS_RELU = 3, /* + bias, relu (pointnet.py:28-31) */
    SCREAM_EPI_RES_LN = 4,    /* LayerNorm(C + residual) * gamma + beta, N == 256 (transformer.py:84,88) */
    SCREAM_EPI_QKV = 5        /* internal to scream_gemm_qkv_f32 */
};

/* ---- Activation layouts of a [M, 256] fp32 matrix (M % 32 == 0).
 * Row-major is the default everywhere.  FRAGMENT-major (SCREAM_ACT_FRAG) is the layout the operand-split kernels pass
 * between each other inside scream_forward: element (row 32 t + r, feature 32 blk + 8 a + 4 h + b) -- t the 32-row group,
 * blk the 32-feature segment, a in 0..3, h in 0..1, b in 0..3 -- lives at float offset
 *     ((((t * 8 + blk) * 4 + a) * 64 + r + 32 h) * 4 + b.
 * A 32-row group occupies the same 32 KiB as in row-major, so slices of whole groups are the same pointers in both
 * layouts.  Why: lane r + 32 h of a wave owns exactly the 16-byte pieces 2a + h of every 128-byte segment of row r as an
 * MFMA operand; stored this way, each of its four loads per segment is one fully contiguous 1 KiB wave access instead of
 * 32 half-used cache lines (scream_amd/csrc/tail_split.hip).  scream_act_layout converts a matrix between the two. */
#define SCREAM_LAYOUT_A_FRAG 1 /* the GEMM's A operand is fragment-major */
#define SCREAM_LAYOUT_C_FRAG 2 /* the activated (elu + 1) query tile of the GEMM's output is fragment-major */
int scream_act_layout(const float* src, float* dst, int64_t M, int32_t to_fragment, void* stream);

/* Library / build identification: "scream_hip gfx950 <abi>"; abi bumps on any signature change. */
const char* scream_version(void);
int scream_abi_version(void);

/* ---- A2/A4/A6: C[M,N] = epilogue(A[M,K] . W[N,K]^T), fp32-input MFMA (v_mfma_f32_32x32x2_f32).
 * Replaces torch.nn.Linear / Conv1d(k=1) at models/transformer.py:79-81,83,87 and
 * models/pointnet.py:60.  M % 128 == 0, N % 256 == 0, K % 64 == 0; lda/ldc/ldr in floats, multiples of 4;
 * A, W, C and residual 16-byte aligned. */
int scream_gemm_f32(const float* A, int64_t lda, const float* W, float* C, int64_t ldc,
                    int64_t M, int32_t N, int32_t K, int32_t epilogue, int32_t n_act,
                    const float* bias, const float* residual, int64_t ldr,
                    const float* gamma, const float* beta, void* stream);

/* ---- A2 + A3 (reduce) fused: q/k/v projections whose key/value tiles never leave the chip.
 * Replaces models/transformer.py:79-81 together with :28-29 (elu+1) and :38-40 (values / v_length, K^T V, K.sum).
 * W [N,K] is laid out [ q (n_q = 256 rows, or 0 rows for the cross layers' key/value-only call) |
 * k heads 0-3 | v heads 0-3 | k heads 4-7 | v heads 4-7 ] (128 rows each), so one 256-wide tile holds K and V of
 * four heads for the same 128 tokens.  Query tiles are stored as elu(q)+1 into Q [M, ldq]; key/value tiles are
 * reduced in the epilogue straight from the MFMA accumulators into kv_partial [M/128][8][33*32] (per 128-row
 * tile and head: K'^T (V/S) as [d][v], then Ksum[d]); rows past the cloud's length are masked.  A's row 0 is
 * packed row `row_base`; tile_cloud / cloud_row0 / cloud_len describe the packed batch (absolute rows).
 * scream_kv_finalize then adds the tiles of every cloud in order. */
int scream_gemm_qkv_f32(const float* A, int64_t lda, const float* W, float* Q, int64_t ldq, int64_t M,
                        int32_t N, int32_t K, int32_t n_q, const int32_t* tile_cloud,
                        const int32_t* cloud_row0, const int32_t* cloud_len, int64_t row_base,
                        float* kv_partial, void* stream);
int scream_kv_finalize(const float* kv_partial, const int32_t* cloud_row0, const int32_t* cloud_len,
                       int64_t row_base, int32_t cloud_begin, int32_t n_kv, float* kv_out, void* stream);

/* ---- The same two GEMM entry points on the 16-bit matrix cores by OPERAND SPLITTING, fp32-level accuracy
 * (scream_amd/csrc/gemm_split.hip, split.h).  `split` selects the arithmetic:
 *   SCREAM_SPLIT_H2  (2): x 2^e = x0 + x1 in fp16, three fp16 MFMAs per 16-deep step (a1b0 + a0b1 + a0b0), fp32 accumulate --
 *                    the default of the forward since round 3.  fp16 has a 5-bit exponent, so each operand carries an exact
 *                    power-of-two scale: w_exp is baked into the packed weights, a_exp is applied to A as it is split, the
 *                    accumulators are multiplied by 2^-(a_exp + w_exp).  CONTRACT: |A| 2^a_exp <= 2^15 and |W| 2^w_exp <= 2^15 for
 *                    every element (fp16 overflows at 65 504; values below 2^-3 / 2^exp lose relative precision, so choose the
 *                    largest exponent the bound allows).  scream_amd/scales.py derives a_exp for every GEMM of the forward from
 *                    the weights alone (LayerNorm outputs are bounded by gamma / beta).
 *   SCREAM_SPLIT_BF3 (3): x = x0 + x1 + x2 in bf16 (exact), six bf16 MFMAs per step; bf16 keeps fp32's exponent range, so
 *                    a_exp / w_exp are ignored and the result is scale invariant bit for bit.  Rounds 1-2's arithmetic.
 * The weight matrix is pre-split and re-tiled ONCE by scream_pack_w_split (device to device): W [N,K] fp32 ->
 * W_packed, 2*split*N*K bytes: [split planes][K/32 k-tiles][N][32] 16-bit values, stored k-tile by k-tile in the order the
 * kernel stages it in LDS.  A, C, residual and bias stay fp32.  M % 128 == 0, N % 256 == 0, K = 64 + 192 j (64, 256, 448, ...,
 * 1024: the k-loop rotates three operand register sets over two LDS stages, so the k-tile count K/32 is even and 2 mod 3;
 * anything else is SCREAM_EUNSUPPORTED).  A row-block [n0, n0 + n) of W must be packed on its own to be used as a GEMM
 * operand on its own.  scream_gemm_qkv_split_f32 also takes N = 512 L with n_q == 0: the key/value projections of L layers
 * applied to the SAME rows as one GEMM (the cross stage's target side: the target features are frozen after the stem,
 * models/pointnet.py:53-57); W is then the L matrices [k heads 0-3 | v 0-3 | k 4-7 | v 4-7] stacked, and layer l's partials
 * are written at kv_partial + l * (M/128) * 8 * 1056 floats.  k_exp / v_exp (fp16 splits; ignored on SCREAM_SPLIT_BF3): the K^T V
 * reduction in the epilogue runs on fp16 x 2 planes of K' = elu(k) + 1 and V as well -- CONTRACT |K'| 2^k_exp, |V| 2^v_exp <= 2^15
 * (|k| and |v| are bounded like any projection of a LayerNorm output; K' <= 1 + max(k, 0)).  layout (SCREAM_LAYOUT_* bits): A fragment-major needs lda == K == 256; C fragment-major applies to the
 * activated tile of an ELU1 / QKV epilogue with n_act == ldc == 256 (the queries). */
#define SCREAM_SPLIT_H1 1 /* ONE fp16 plane, one product: NOT fp32-accurate (2^-11 per operand) -- the mirror of the reference's
                            * `with autocast()` around the KITTI forward (evaluate_kitti.py:37); exponents as for SCREAM_SPLIT_H2;
                            * explicit opt-in only (evaluate_kitti.evaluate(autocast=True)) */
#define SCREAM_SPLIT_H2 2
#define SCREAM_SPLIT_BF3 3
int scream_pack_w_split(const float* W, int32_t N, int32_t K, int32_t split, int32_t w_exp, void* W_packed,
                        void* stream);
int scream_gemm_split_f32(const float* A, int64_t lda, const void* W_packed, float* C, int64_t ldc, int64_t M,
                          int32_t N, int32_t K, int32_t epilogue, int32_t n_act, const float* bias,
                          const float* residual, int64_t ldr, const float* gamma, const float* beta,
                          int32_t layout, int32_t split, int32_t a_exp, int32_t w_exp, void* stream);
int scream_gemm_qkv_split_f32(const float* A, int64_t lda, const void* W_packed, float* Q, int64_t ldq,
                              int64_t M, int32_t N, int32_t K, int32_t n_q, const int32_t* tile_cloud,
                              const int32_t* cloud_row0, const int32_t* cloud_len, int64_t row_base,
                              float* kv_partial, int32_t layout, int32_t split, int32_t a_exp, int32_t w_exp,
                              int32_t k_exp, int32_t v_exp, void* stream);

/* ---- The same fused q/k/v projection (A2 + the A3 reduce) as a RING kernel (scream_amd/csrc/proj_ring.hip, round 4; fp16 splits,
 * fragment-major x in and Q' out): one wave per SIMD owns 64 rows and keeps their operand planes in registers for all of
 * q | k | v, the weights stream chunk by chunk (32 output columns over K = 256 = one 32 KiB stage) through a ring of LDS stages,
 * and every chunk's epilogue -- elu + 1 and the stores of a query chunk, or K' = elu(k) + 1, the operand split and K'^T V of a
 * head -- runs in the shadow of the NEXT chunk's matrix instructions.  Same arithmetic per product and the same outputs as
 * scream_gemm_qkv_split_f32 with SCREAM_LAYOUT_A_FRAG | SCREAM_LAYOUT_C_FRAG (Q' and the kv_partial array scream_kv_finalize_image
 * sums; the partial of a 128-row tile is added up from two 64-row halves instead of four 32-row quarters, so the two kernels
 * agree to fp32 rounding, not bit for bit).  The weight matrix W [N, 256] (row order of scream_gemm_qkv_f32 above: q | per
 * layer k 0-3 | v 0-3 | k 4-7 | v 4-7; n_q = 256 with N = 768, or n_q = 0 with N = 512 L) is packed once by scream_pack_proj
 * into scream_proj_image_bytes(N, split) bytes: [N / 32 stages][split planes][16 fragments][64 lanes][8] fp16, in the order the
 * kernel consumes them (query chunks 0 .. 7, then per layer and head K_h, V_h).  M % 128 == 0; exponents as for
 * scream_gemm_qkv_split_f32 (a_exp, w_exp of the product; k_exp, v_exp of K' and V in the reduction), and SCREAM_EINVAL unless
 * a_exp + w_exp, v_exp - a_exp - w_exp and k_exp + v_exp lie in [-126, 126]. */
int64_t scream_proj_image_bytes(int32_t N, int32_t split);
int scream_pack_proj(const float* W, int32_t N, int32_t n_q, int32_t split, int32_t w_exp, void* proj_image, void* stream);
int scream_proj_qkv_f32(const float* x, const void* proj_image, float* Q, int64_t M, int32_t N, int32_t n_q,
                        const int32_t* tile_cloud, const int32_t* cloud_row0, const int32_t* cloud_len,
                        int64_t row_base, float* kv_partial, int32_t split, int32_t a_exp, int32_t w_exp, int32_t k_exp,
                        int32_t v_exp, void* stream);

/* ---- A3 (apply) + A4 as ONE launch: everything of an MHAttention block that is local to a row,
 *     att = ((Q' . KV) * Z) * S;  m1 = LayerNorm1(att . Wm^T + x);  y = LayerNorm2(x + W2 . relu(W1 . m1))
 * Replaces models/transformer.py:41-42,83-88, i.e. scream_attn_apply + scream_gemm_split_f32(merge, EPI_RES_LN) +
 * scream_gemm_split_f32(mlp.0, EPI_RELU) + scream_gemm_split_f32(mlp.2, EPI_RES_LN), with the same split arithmetic; att, m1
 * and the 1024-wide hidden activations never reach memory (scream_amd/csrc/tail_split.hip).  Operands:
 * Q, x and y are FRAGMENT-major [M, 256] matrices (SCREAM_ACT_FRAG above; scream_act_layout converts):
 *   Q             the elu+1 mapped queries written by scream_gemm_qkv_split_f32 / scream_gemm_split_f32(EPI_ELU1) with
 *                 SCREAM_LAYOUT_C_FRAG;
 *   kv_image      scream_kv_image_bytes() per cloud, written by scream_kv_finalize_image from the K^T V partials of
 *                 scream_gemm_qkv_split_f32 (same arguments as scream_kv_finalize): KV^T / S as MFMA operand fragments + Ksum in fp32, for the SAME `split` as the tail that reads it: three bf16 planes
 *                 (SCREAM_SPLIT_BF3) or -- fp16 splits, round 4 -- two fp16 planes of KV_h^T / S * 2^e_h, e_h chosen on the device from the
 *                 head's largest |element| (a maximum: exact, order independent) with 2^-e_h stored beside them;  the key cloud of 128-row
 *                 tile t is tile_cloud[t] + kv_cloud_offset (tile_cloud points at the entry of the first row), cloud_len gives S;
 *   x             the block input (residual of BOTH norms), must not alias y;
 *   tail_image    scream_tail_image_bytes(split), built once by scream_pack_tail from merge [256,256], mlp.0 [1024,256]
 *                 and mlp.2 [256,1024] (fp32, device to device) for the same `split` and exponents;
 *   exps          SCREAM_SPLIT_H2 only (NULL otherwise): the power-of-two exponents of the operands.  CONTRACT, for every value
 *                 the operand can take: |att| 2^e_att, |m1| 2^e_m1, |relu(W1 m1)| 2^e_h <= 2^15 and |Wm| 2^e_wm, |W1| 2^e_w1,
 *                 |W2| 2^e_w2 <= 2^15.  |att| <= max |v| (a convex combination of value rows), |m1| <= 16 |gamma1| + |beta1|,
 *                 |W1 m1| <= 16 |W1_row * gamma1|_2 + |W1_row . beta1|: scream_amd/scales.py computes them from the weights.
 *                 Exponents in [-40, 40], e_wm + e_att and e_w2 + e_h in [-44, 44] (SCREAM_EINVAL otherwise).
 * M % 128 == 0, every pointer 16-byte aligned. */
typedef struct {
    int32_t e_att, e_wm, e_m1, e_w1, e_h, e_w2;
    int32_t e_y, e_wq; /* only with a next-layer query projection in the image (below): of the block output y and of that Wq */
    int32_t e_q;       /* of Q' = elu(q) + 1 as an operand of the attention apply (fp16 x 2 since round 4): |Q'| 2^e_q <= 2^15, Q' <= 1 + the
                        * bound of the query projection (scream_amd/scales.py: 16 |w * gamma|_2 + |w . beta| over the rows of Wq) */
} scream_tail_exps_t;
int64_t scream_tail_image_bytes(int32_t split, int32_t with_next_q);
int64_t scream_kv_image_bytes(void);
/* Wq_next (may be NULL; fp16 splits): q_proj.weight [256,256] of the NEXT layer when that layer takes its queries from this
 * block's output rows (a cross layer behind a self layer, models/transformer.py:130): eight more stages in the image, and
 * scream_layer_tail_f32 called with q_next != NULL ends every tile with Q'_next = elu(y . Wq_next^T) + 1 (fragment-major) --
 * the separate scream_gemm_split_f32(..., SCREAM_EPI_ELU1) launch of that layer is then not needed. */
int scream_pack_tail(const float* Wm, const float* W1, const float* W2, const float* Wq_next, int32_t split,
                     const scream_tail_exps_t* exps, void* tail_image, void* stream);
/* n_layers > 1: the partials of a batched key/value projection (scream_gemm_qkv_split_f32 with N = 512 n_layers): layer l
 * reads kv_partial + l * partial_layer_stride floats ((M/128) * 8 * 1056 of that GEMM) and writes its n_kv cloud images at
 * kv_image + l * image_layer_stride bytes.  n_layers == 1: strides ignored. */
int scream_kv_finalize_image(const float* kv_partial, const int32_t* cloud_row0, const int32_t* cloud_len,
                          int64_t row_base, int32_t cloud_begin, int32_t n_kv, void* kv_image, int32_t n_layers,
                          int64_t partial_layer_stride, int64_t image_layer_stride, int32_t split, void* stream);
int scream_layer_tail_f32(const float* Q, const void* kv_image, const int32_t* tile_cloud,
                          int32_t kv_cloud_offset, const int32_t* cloud_len, const float* x,
                          const void* tail_image, const float* g1, const float* b1, const float* g2,
                          const float* b2, float* y, float* q_next, int64_t M, int32_t split,
                          const scream_tail_exps_t* exps, void* stream);

/* ---- A1: feats = LayerNorm(PE_sine(xyz) + W_e (xyz - center[cloud]) + b_e)
 * Replaces models/pointnet.py:45-48 (+ models/transformer.py:157-179).  xyz [rows,3] packed;
 * tile_cloud[rows/128] gives the cloud of each 128-row tile; center [n_clouds,3] (zeros for
 * target clouds); dim_t [84] is the host-computed frequency table of transformer.py:168-170. */
int scream_pe_embed_ln(const float* xyz, const int32_t* tile_cloud, const float* center,
                       const float* dim_t, const float* emb_w, const float* emb_b,
                       const float* gamma, const float* beta, float* feats, int64_t rows,
                       void* stream);
/* the same values written FRAGMENT-major (SCREAM_ACT_FRAG below): what the fused forward feeds its first projection */
int scream_pe_embed_ln_frag(const float* xyz, const int32_t* tile_cloud, const float* center,
                            const float* dim_t, const float* emb_w, const float* emb_b,
                            const float* gamma, const float* beta, float* feats, int64_t rows,
                            void* stream);

/* ---- A3 (reduce): per key cloud and head, KV = sum_s K[s]^T (V[s]/S), Ksum = sum_s K[s]
 * Replaces models/transformer.py:38-41 (values / v_length, the "nshd,nshv->nhdv" einsum, K.sum).
 * Kf/Vf point at column 0 of the (elu+1)-mapped keys / raw values, row stride ld floats, row 0 =
 * packed row `row_base`.  cloud_row0/cloud_len [n_clouds] (int32, absolute packed rows / true lengths).
 * Processes clouds [cloud_begin, cloud_begin + n_kv).  partial is scratch of
 * n_kv * max_chunks * 8 * 33 * 32 floats; kv_out [n_clouds][8][33][32]: rows 0-31 of a head hold KV^T
 * ([v][d], d contiguous -- the layout scream_attn_apply stages into LDS), row 32 holds Ksum[d]. */
int scream_kv_reduce(const float* Kf, const float* Vf, int64_t ld, int64_t row_base,
                     const int32_t* cloud_row0, const int32_t* cloud_len, int32_t cloud_begin,
                     int32_t n_kv, int32_t max_chunks, float* partial, float* kv_out, void* stream);

/* ---- A3 (apply): out[l,h,:] = (Q[l,h,:] . KV[h]) * 1/(Q[l,h,:].Ksum[h] + 1e-6) * S
 * Replaces models/transformer.py:41-42.  Qf [rows, ldq] (elu+1 mapped), kv as written by
 * scream_kv_reduce; the key cloud of query tile t is tile_cloud[t] + kv_cloud_offset. */
int scream_attn_apply(const float* Qf, int64_t ldq, const float* kv, const int32_t* tile_cloud,
                      int32_t kv_cloud_offset, const int32_t* cloud_len, float* out, int64_t ldo,
                      int64_t rows, void* stream);

/* ---- A6 (head): out[rows,3] = X[rows,256] . W[3,256]^T + b.  models/pointnet.py:32,60 */
int scream_coor_head(const float* X, const float* W, const float* b, float* out, int64_t rows,
                     void* stream);

/* ---- Whole forward pass of PointTransformer over a packed batch (A1-A6).
 * Replaces models/pointnet.py:38-60 for B pairs at once (the reference asserts B == 1, :39-40). */
/* scream_model_t.gemm_split alone selects the forward's schedule.  Each value reads exactly the fields of its row; a model that
 * does not match its row is refused with SCREAM_EINVAL before the first launch (the pointers never select a schedule):
 *
 *   gemm_split            | self layers (stem, stem_tgt, cross.2j)    | cross layers (cross.2j+1.layer) | scream_model_t (n_cross > 0)
 *   ----------------------+-------------------------------------------+---------------------------------+-----------------------------
 *   0 (fp32)              | wqkv, wm, w1, w2; tail NULL               | wq, wkv, wm, w1, w2; tail NULL  | --
 *   SCREAM_SPLIT_BF3      | wqkv, tail                                | wq, tail                        | wkv_cross
 *   SCREAM_SPLIT_H2 / H1  | proj, tail (cross.2j: with Wq_next,       | tail                            | proj_cross
 *                         |             tail_next_q = 1)              |                                 |
 *
 * tail_next_q is 1 on the cross-stage self layers of the fp16 splits and 0 everywhere else.  Fields outside a row are not read.
 *   fp32:  row-major features; scream_gemm_qkv_f32, scream_kv_finalize, scream_attn_apply and three scream_gemm_f32 per layer;
 *          the cross layers project their queries (wq, ELU1) and the target side (wkv) per layer.
 *   BF3:   fragment-major features (SCREAM_ACT_FRAG); scream_gemm_qkv_split_f32, scream_kv_finalize_image and
 *          scream_layer_tail_f32 per layer; the target side of ALL cross layers in one launch after the stem (wkv_cross); the cross
 *          layers' queries on scream_gemm_split_f32 (wq, ELU1).
 *   fp16:  as BF3 with the projections on scream_proj_qkv_f32 (proj, proj_cross) and the cross layers' queries written by the
 *          tail of the self layer in front (tail_next_q). */
typedef struct {
    /* fp32 [N,K] when gemm_split == 0, scream_pack_w_split images (the pointers are then really const void*) on SCREAM_SPLIT_BF3 */
    const float* wqkv; /* [768,256]: q_proj | k_proj[0:128] | v_proj[0:128] | k_proj[128:256] | v_proj[128:256] */
    const float* wq;   /* rows [0,256) of wqkv as their own matrix (cross layers project q and k/v from different clouds) */
    const float* wkv;  /* fp32 only: rows [256,768) of wqkv as their own matrix */
    const float* wm;   /* fp32 only: merge [256,256] */
    const float* w1;   /* fp32 only: mlp.0 [1024,256] */
    const float* w2;   /* fp32 only: mlp.2 [256,1024] */
    const float* g1; const float* b1; /* norm1 */
    const float* g2; const float* b2; /* norm2 */
    /* gemm_split != 0: scream_pack_tail image of (wm, w1, w2) for the same split -- attention apply, merge + norm1 and the
     * FFN + norm2 as ONE launch per block (scream_layer_tail_f32).  NULL on fp32. */
    const void* tail;
    /* fp16 splits only: power-of-two exponents (scream_amd/scales.py).  e_xq / e_xkv: the block input on the query side and on
     * the key/value side (different clouds in a cross layer), bounded by the LayerNorm that produced it; e_wqkv, e_wq: of the
     * matrices above as packed; tail_exps: of the layer tail and its image. */
    int32_t e_xq, e_xkv, e_wqkv, e_wq;
    int32_t e_k, e_v; /* of K' = elu(k) + 1 and of V in the projection's K^T V epilogue */
    scream_tail_exps_t tail_exps;
    int32_t tail_next_q; /* the tail image carries the NEXT layer's query projection (scream_pack_tail, Wq_next) */
    const void* proj;    /* fp16 splits, self layers: scream_pack_proj image of wqkv (n_q = 256, exponent e_wqkv) */
} scream_layer_t;

typedef struct {
    int32_t n_self;  /* stem layers (models/pointnet.py:18-20) */
    int32_t n_cross; /* (self, cross) layer pairs (:22-25) */
    const float* dim_t; /* [84] */
    const float* emb_w; const float* emb_b; /* [256,3], [256] */
    const float* pre_g; const float* pre_b; /* pre_norm */
    const scream_layer_t* layers_host; /* HOST array: n_self stem layers, then cross.0, cross.1.layer, ... */
    const float* c0_w; const float* c0_b; /* coor_mlp.0 [256,256],[256] */
    const float* c2_w; const float* c2_b; /* coor_mlp.2 */
    const float* c4_w; const float* c4_b; /* coor_mlp.4 [3,256],[3] */
    /* NULL for PointTransformer (one stem for both clouds, models/pointnet.py:50-52).  DEMTransformer
     * (models/pointnet.py:113-118,143-145): HOST array of n_self layers applied to the SECOND clouds (stem_dem) while
     * layers_host[0..n_self) (stem_dsm) are applied to the first clouds only. */
    const scream_layer_t* stem_tgt_layers_host;
    /* 0, SCREAM_SPLIT_BF3, SCREAM_SPLIT_H2 or SCREAM_SPLIT_H1: the arithmetic AND the schedule (the table above scream_layer_t).
     * gemm_split != 0: c0_w and c2_w are scream_pack_w_split images and the coordinate MLP runs on scream_gemm_split_f32 -- same
     * fp32 results to rounding (tests/test_gpu_parity.py holds fp32, BF3 and H2 to the same tolerances). */
    int32_t gemm_split;
    /* fp16 splits only: exponents of the coordinate MLP's two GEMMs (input: the last LayerNorm2 / relu(c0 . + b0)) */
    int32_t e_c0x, e_c0w, e_c2x, e_c2w;
    /* SCREAM_SPLIT_BF3 with n_cross > 0: scream_pack_w_split image of the n_cross cross layers' key/value matrices (rows
     * [256,768) of their wqkv) stacked, [512 n_cross, 256].  The target features are frozen after the stem, so they are
     * projected for ALL cross layers in one launch (and their K^T V images finalised in one). */
    const float* wkv_cross;
    int32_t e_wkv_cross, e_k_cross, e_v_cross; /* fp16 splits: of proj_cross; e_k / e_v the smallest over the cross layers */
    /* fp16 splits with n_cross > 0: scream_pack_proj image of the same stacked matrix (n_q = 0, exponent e_wkv_cross) */
    const void* proj_cross;
} scream_model_t;

typedef struct {
    int32_t n_pairs;     /* B; clouds 0..B-1 are the sources, B..2B-1 the targets */
    int64_t rows_src;    /* packed rows of all source clouds (multiple of 128) */
    int64_t rows_total;  /* sources then targets (multiple of 128) */
    int32_t max_chunks;  /* max over clouds of ceil(len / SCREAM_KV_CHUNK) */
    const float* xyz;          /* [rows_total,3], zero in padding rows */
    const float* center;       /* [2B,3]: src_center per source cloud, zeros for targets */
    const int32_t* tile_cloud; /* [rows_total/128] */
    const int32_t* cloud_row0; /* [2B] */
    const int32_t* cloud_len;  /* [2B] */
} scream_batch_t;

/* Bytes of scratch scream_forward needs for this batch geometry and this model (its gemm_split and n_cross).  gemm_split != 0:
 * 3 KB per row (two feature buffers and Q') plus the partials and images of every cross layer's target-side K^T V side by side;
 * fp32: the attention output, LayerNorm1 output and FFN hidden buffers of its launch-per-step chain as well (9 KB per row). */
int64_t scream_forward_workspace_bytes(int64_t rows_src, int64_t rows_total, int32_t n_pairs,
                                       int32_t max_chunks, int32_t gemm_split, int32_t n_cross);

/* src_pred [rows_src,3] (padding rows hold don't-care values).  If feats_out != NULL the final
 * source features [rows_src,256] are copied there (test hook).  trace: NULL, or a handle from
 * scream_trace_create -- then every kernel group of the forward is bracketed by HIP events on `stream`. */
int scream_forward(const scream_model_t* model, const scream_batch_t* batch, void* workspace,
                   int64_t workspace_bytes, float* src_pred, float* feats_out, void* trace,
                   void* stream);

/* Per-launch timing for bench.py's roofline leg.  A trace owns 2*capacity HIP events; records beyond
 * capacity are dropped.  scream_trace_read (after the stream has been synchronised) fills, per record,
 * the elapsed ms, the kind (a SCREAM_EPI_* value for a GEMM with its M, N, K; 100 = embed, 101 = K^T V
 * reduce, 102 = attention apply, 103 = 256->3 head, with M = rows) and returns the record count. */
void* scream_trace_create(int32_t capacity);
void scream_trace_destroy(void* trace);
int scream_trace_reset(void* trace);
int scream_trace_read(void* trace, int32_t max_records, float* ms, int32_t* kind, int64_t* m,
                      int32_t* n, int32_t* k);
/* Start of every record in ms after the start of record 0.  One trace may be handed to forwards running on
 * several streams at once (pairs are independent, so a step can run as concurrent lanes); their records then
 * overlap in time and the busy time of a kernel class is the union of its intervals, not the sum. */
int scream_trace_read_starts(void* trace, int32_t max_records, float* start_ms);

/* ---- A7: thresholded 1-NN of every query point in its pair's target cloud.
 * Replaces square_distance(src_pred / s, tgt / s)[0].min(dim=1) and the threshold compare at
 * evaluate_3d_match.py:94-95 (also models/pointnet.py:71-72, evaluate_kitti.py:53-54) without
 * materialising the N x M matrix.  Bit-exact fp32 arithmetic of utils.py:72-78 as torch-CPU
 * executes it: a = x / fp32(s) (IEEE divide); dot = fma(a2,b2,fma(a1,b1,a0*b0));
 * |a|^2 = (a0^2 + a1^2) + a2^2; d = ((-2 dot) + |a|^2) + |b|^2; ties -> lowest target index.
 * One launch set covers n_pairs pairs.  query/ref are packed [rows,3]; q_row0/q_len, r_row0/r_len
 * [n_pairs] int32 (device); s [n_pairs] fp32 (device).  Outputs are indexed by packed query row:
 * idx (int32, index inside the pair's target cloud; -1 in rows outside any cloud), dmin (fp32),
 * valid (uint8: dmin < thresh).  Scratch: ref_prep 4 floats per ref row, keys one uint64 per query row. */
int scream_nn_search(const float* query, const float* ref, const int32_t* q_row0,
                     const int32_t* q_len, const int32_t* r_row0, const int32_t* r_len,
                     const float* s, int32_t n_pairs, int32_t max_q_len, int32_t max_r_len,
                     int64_t q_rows_total, int64_t r_rows_total, float thresh, float* ref_prep,
                     uint64_t* keys, int32_t* idx, float* dmin, uint8_t* valid, void* stream);

/* Dense utils.square_distance (utils.py:72-78): out[B,N,M] = -2 src.dst^T + |src|^2 + |dst|^2 with the
 * rounding sequence above.  API compatibility only -- the hot path uses scream_nn_search. */
int scream_square_distance(const float* src, const float* dst, float* out, int32_t B, int32_t N,
                           int32_t M, void* stream);

/* ---- A8 + A9 (+ A10): correspondence gather fused into the weighted Kabsch solve.
 * Replaces evaluate_3d_match.py:96-101 and utils.py:138-178 for n_pairs pairs in one launch:
 *   A_n = src[n] / s + c, B_n = ref[idx[n]] / s + c for every n with valid[n] (idx == NULL: B row = n,
 *   the corr="src_pred" branch of evaluate_3d_match.py:99-101); centroids sum/(K + 1e-6);
 *   H = sum (A-cA)(B-cB)^T; 3x3 SVD by one-sided Jacobi in registers (fp64), R = V diag(1,1,det(V U^T)) U^T,
 *   t = cB - R cA.  K == 0 gives the identity, as torch.svd of a zero matrix does.
 * Domain of the solve (both entry points): H is held in fp32, as the reference holds it, and the SVD is scale-free, so the
 *   pose has the accuracy of an O(1) problem while the largest entry of H is a normal fp32 number with its 24 bits, i.e.
 *   2^-102 <= max |H_ij| < 2^127: centred coordinates between about 2^-50 / sqrt(K) and 2^62 / sqrt(K) in both clouds
 *   (tests hold 2^-40 .. 2^20).  Below that H loses bits to gradual underflow and the rotation degrades with it (still a
 *   proper rotation; H == 0 exactly gives the identity); above it H overflows.  Neither is detected.
 * T_out [n_pairs,16] row-major 4x4; n_corr [n_pairs] (int32) = K.  c is [n_pairs,3]. */
int scream_kabsch_corr(const float* src, const float* ref, const int32_t* src_row0,
                       const int32_t* src_len, const int32_t* ref_row0, const int32_t* idx,
                       const uint8_t* valid, const float* s, const float* c, int32_t n_pairs,
                       float* T_out, int32_t* n_corr, void* stream);

/* Drop-in for utils.rigid_transform_3d (utils.py:138): A, B [bs,K,3] dense, w [bs,K] or NULL.
 * Weights below weight_threshold count as 0 (utils.py:151).  T_out [bs,16]. */
int scream_rigid_transform_3d(const float* A, const float* B, const float* w,
                              float weight_threshold, int32_t bs, int32_t K, float* T_out,
                              void* stream);

/* ---- A10: RE [deg] = acos(clamp((tr(Rp^T Rg) - 1)/2)) * 180/pi, TE = |tp - tg| (utils.py:181-189).
 * T_pred, T_gt [n,16]; re, te [n]. */
int scream_transformation_error(const float* T_pred, const float* T_gt, int32_t n, float* re,
                                float* te, void* stream);

/* ---- A11 (the per-pair L1 point loss the evaluators report): loss[p] = mean_n sum_xyz |src_pred_n - (R_p src_n + t_p)|
 * Replaces PointTransformer.loss (models/pointnet.py:93-99) called once per pair (evaluate_3d_match.py:86): src_pred / src packed
 * [rows,3] in the normalised frame, rot [n_pairs,9] / trans [n_pairs,3] the ground-truth pose of the same frame. */
int scream_point_loss(const float* src_pred, const float* src, const int32_t* src_row0, const int32_t* src_len,
                      const float* rot, const float* trans, int32_t n_pairs, float* loss, void* stream);

/* ---- next row: batched point-to-point ICP refinement on the GPU.
 * Replaces o3d.registration_icp(src_pc, tgt_pc, max_correspondence_distance, init) at
 * evaluate_3d_match.py:106-113 / evaluate_kitti.py:61-70 (open3d is absent here: parity with open3d is
 * unpinned; the loop is open3d's published RegistrationICP and is checked against oracle/icp_ref.py).
 * src/ref packed, normalised frame; metric points are x / s + c.  T [n_pairs,16] holds the initial
 * transforms on entry and the refined ones on return.  Per iteration (one launch): transform the source (a = T x, fp32),
 * thresholded 1-NN: the nearest target b is a correspondence iff d^2 < max_corr_dist * max_corr_dist (strict; the fp32 product,
 * compared with the search's fp32 value d^2 = (-2 a.b + |a|^2) + |b|^2, which SELECTS and is used for nothing else);
 * fitness = #corr / N and inlier_rmse = sqrt(mean |a - b|^2) with the DIFFERENCE a - b taken in fp64 (what open3d measures;
 * exactly 0 for coincident clouds in any frame); stop a pair when both change by less than rel_fitness / rel_rmse or after
 * max_iter updates; otherwise compose the Kabsch update of the correspondences, T <- dT . T.  iters = the number of updates
 * applied.  A pair that finds no correspondence (an empty source included) has fitness 0 and inlier_rmse 0, takes the identity
 * as its update and goes on, as open3d's loop does: its T stays the initial T bit for bit, and iters is 1 when both thresholds
 * are positive (its second evaluation repeats the first, so it stops there), max_iter when a threshold is 0 (|change| < 0 never
 * holds), and 0 when max_iter is 0.  fitness_rmse [n_pairs,2] and iters [n_pairs] may be NULL.  The clouds of a batch may be
 * packed in any order (the per-chunk partial sums are indexed by a prefix sum of the source lengths).
 * ASYNCHRONOUS, like every entry point: scream_icp_p2p enqueues the whole schedule (max_iter + 2 launches at most) and never
 * waits for the device; a pair that has stopped freezes there (its blocks return at their first instruction).  A caller with a
 * LONG schedule (KITTI: 1000) that wants to stop launching once every pair has stopped asks for the schedule in pieces:
 * scream_icp_p2p_range enqueues launches [it_begin, it_end) of the same run (launch `it` = evaluate search it - 1, stop or
 * update, search it; launch max_iter + 1 = the evaluation of the last search; it_begin == 0 also does the set-up, so a run
 * starts there; every call of a run gets the same arguments and workspace) and then copies the per-pair stopped flags to
 * done_flags [n_pairs] (device int32, may be NULL) -- the caller copies them to pinned memory behind an event and decides on the
 * host, between pieces, without ever blocking the stream (scream_amd/ops.py: IcpRun).  T is complete for pair p once its flag
 * is set.  Results do not depend on how the schedule was cut.
 * scream_icp_p2p_brute_range is the YARDSTICK of the tests and of tools/icp_bench.py, not a product path: the arguments and the
 * schedule of scream_icp_p2p_range, with every search done by scream_nn_search over all targets instead of the target grid
 * (three or four launches per iteration instead of one).  Its results are bit for bit those of scream_icp_p2p_range.  A run
 * uses ONE of the two entry points from it_begin == 0 to its end (they lay the workspace out differently);
 * scream_icp_workspace_bytes covers both.  Nothing here reads the process environment. */
int64_t scream_icp_workspace_bytes(int64_t src_rows_total, int64_t ref_rows_total, int32_t n_pairs);
int scream_icp_p2p_range(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                         const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                         int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                         int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                         float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, int32_t it_begin, int32_t it_end,
                         int32_t* done_flags, void* workspace, int64_t workspace_bytes, void* stream);
int scream_icp_p2p_brute_range(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                               const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                               int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                               int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                               float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, int32_t it_begin, int32_t it_end,
                               int32_t* done_flags, void* workspace, int64_t workspace_bytes, void* stream);
int scream_icp_p2p(const float* src, const float* ref, const int32_t* src_row0, const int32_t* src_len,
                   const int32_t* ref_row0, const int32_t* ref_len, const float* s, const float* c,
                   int32_t n_pairs, int32_t max_src_len, int32_t max_ref_len, int64_t src_rows_total,
                   int64_t ref_rows_total, float max_corr_dist, int32_t max_iter, float rel_fitness,
                   float rel_rmse, float* T, float* fitness_rmse, int32_t* iters, void* workspace,
                   int64_t workspace_bytes, void* stream);

/* ---- Training (backward pass of PointTransformer, fp32; csrc/backward.hip, composed by scream_amd/train.py).
 * Every reduction is deterministic: fixed-order partial slabs in the caller's workspace, then a reduce launch; no float
 * atomics.  Rows are packed rows; padded rows must carry zero gradient (dY = 0) and finite activations. */
/* dW[N,K] (+)= sum_r dY[r,:]^T X[r,:] over `rows` rows (row-major dY [rows, ldy], X [rows, ldx]); N % 128 == 0, K % 128 == 0.
 * accumulate != 0 adds into dW (and colsum).  colsum [N] (may be NULL) receives sum_r dY[r,:] (bias gradients).
 * workspace: scream_wgrad_workspace_bytes(rows, N, K) bytes, 16-byte aligned. */
int64_t scream_wgrad_workspace_bytes(int64_t rows, int32_t N, int32_t K);
int scream_gemm_wgrad_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N,
                          int32_t K, float* dW, int32_t accumulate, float* colsum, void* workspace,
                          int64_t workspace_bytes, void* stream);
/* The same weight gradient, same contract, on the 16-bit matrix cores with fp32 accumulation (train_backend "split"): both
 * operands are split into exact sums of 16-bit planes on the way into LDS (csrc/split.h) and every 16-row step runs the split's
 * products.  split: SCREAM_SPLIT_BF3 (three bf16 planes, six v_mfma_f32_32x32x16_bf16 per step; scale free: dY times a power of
 * two gives dW times that power bit for bit, as long as nothing leaves fp32's normal range -- what a loss scale needs);
 * any other value is SCREAM_EINVAL.  colsum is an fp32 sum of the unsplit dY.  Fixed-order slabs and the index-order reduce
 * launch of scream_gemm_wgrad_f32, no atomics: two identical calls are bitwise identical.
 * workspace: scream_wgrad_split_workspace_bytes(rows, N, K) bytes, 16-byte aligned. */
int64_t scream_wgrad_split_workspace_bytes(int64_t rows, int32_t N, int32_t K);
int scream_gemm_wgrad_split_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N,
                                int32_t K, float* dW, int32_t accumulate, float* colsum, int32_t split, void* workspace,
                                int64_t workspace_bytes, void* stream);
/* ---- train_backend "bf16": ONE bf16 product per training GEMM, fp32 accumulation (csrc/gemm_bf16.hip).
 * The arithmetic of all three entry points: sum_k bf16(a_k) * bf16(b_k).  Both operands are fp32 in memory and are rounded to
 * bf16 by round-to-nearest-even on their way into the kernel (v_cvt_pk_bf16_f32, in registers); the products of two bf16
 * values are exact; the sum is accumulated in fp32 on v_mfma_f32_32x32x16_bf16 and stored as fp32.  bf16, not fp16: it keeps
 * fp32's exponent range, so no operand carries an exponent that would have to follow the weights after every optimizer step,
 * gradients of any magnitude pass (a GradScaler's 2^16 included), and a power of two on one operand comes out of the result
 * bit for bit as long as nothing leaves fp32's normal range.  No float atomics, every output element is one fixed-order sum:
 * two identical calls are bitwise identical.  Nothing is packed or transposed beforehand: W is torch's [N,K] fp32 matrix.
 *
 * Forward: C[M,N] = epilogue(A[M,K] . W[N,K]^T).  M % 128 == 0, N % 256 == 0, K % 64 == 0 (SCREAM_EUNSUPPORTED otherwise);
 * lda >= K, ldc >= N, both multiples of 4, pointers 16-byte aligned (SCREAM_EINVAL otherwise).  epilogue: SCREAM_EPI_NONE,
 * SCREAM_EPI_ELU1 (n_act % 256 == 0), SCREAM_EPI_RELU or SCREAM_EPI_BIAS_RELU (bias [N]), applied in fp32 to the fp32 sum;
 * SCREAM_EPI_RES_LN is SCREAM_EUNSUPPORTED. */
int scream_gemm_bf16_f32(const float* A, int64_t lda, const float* W, float* C, int64_t ldc, int64_t M, int32_t N, int32_t K,
                         int32_t epilogue, int32_t n_act, const float* bias, void* stream);
/* Data gradient: dX[M,K] = dY[M,N] . W[N,K], summed over all of N in one launch (W is transposed inside the kernel, on its way
 * into LDS).  M % 128 == 0, K % 256 == 0, N % 64 == 0; ldy >= N, ldx >= K, multiples of 4.  Zero rows of dY (padded rows) give
 * zero rows of dX. */
int scream_gemm_dgrad_bf16_f32(const float* dY, int64_t ldy, const float* W, float* dX, int64_t ldx, int64_t M, int32_t N,
                               int32_t K, void* stream);
/* Weight gradient: the contract of scream_gemm_wgrad_f32 (rows >= 0, N % 128 == 0, K % 128 == 0, accumulate, colsum, ldy, ldx,
 * fixed-order row-slice partials in the workspace and the index-order reduce launch) in the arithmetic above.  colsum is an fp32
 * sum of the UNROUNDED dY.  workspace: scream_wgrad_bf16_workspace_bytes(rows, N, K) bytes, 16-byte aligned. */
int64_t scream_wgrad_bf16_workspace_bytes(int64_t rows, int32_t N, int32_t K);
int scream_gemm_wgrad_bf16_f32(const float* dY, int64_t ldy, const float* X, int64_t ldx, int64_t rows, int32_t N, int32_t K,
                               float* dW, int32_t accumulate, float* colsum, void* workspace, int64_t workspace_bytes,
                               void* stream);
/* y = LayerNorm(a + b) * gamma + beta over rows of 256 (b may be NULL), with the per-row mean and rstd = 1/sqrt(var + 1e-5). */
int scream_ln_fwd(const float* a, const float* b, const float* gamma, const float* beta, float* y, float* mean,
                  float* rstd, int64_t rows, void* stream);
/* LayerNorm backward from the forward's inputs and statistics (xhat recomputed as (a + b - mean) rstd):
 * dz = rstd (g - mean(g) - xhat mean(g xhat)), g = gamma dy; dsum (may be NULL) += dz; dgamma / dbeta (+)= sum dy xhat / sum dy.
 * workspace: scream_ln_bwd_workspace_bytes(rows). */
int64_t scream_ln_bwd_workspace_bytes(int64_t rows);
int scream_ln_bwd(const float* dy, const float* a, const float* b, const float* mean, const float* rstd,
                  const float* gamma, float* dz, float* dsum, float* dgamma, float* dbeta, int32_t accumulate,
                  int64_t rows, void* workspace, int64_t workspace_bytes, void* stream);
/* Linear-attention backward (self and cross) for the query clouds [q_cloud_begin, + n_q_clouds), whose key cloud is
 * query cloud + kv_cloud_offset.  Query side: Q' (elu + 1, [., ldq]), O (the attention output) and dO ([., 256]), q_rows rows
 * from packed row q_row_base; key side: K' and V ([., ldkv]), kv_rows rows from kv_row_base.  kv as written by
 * scream_kv_reduce (Ksum is read from it).  Writes dq = dQ' min(Q', 1) on the query rows and dk = dK' min(K', 1), dv on the
 * key rows (zero on padded rows).  workspace: scream_attn_bwd_workspace_bytes(n_q_clouds, max_chunks). */
int64_t scream_attn_bwd_workspace_bytes(int32_t n_q_clouds, int32_t max_chunks);
int scream_attn_bwd(const float* Qf, int64_t ldq, int64_t q_rows, int64_t q_row_base, const float* O,
                    const float* dO, const float* Kf, const float* Vf, int64_t ldkv, int64_t kv_rows,
                    int64_t kv_row_base, const float* kv, const int32_t* tile_cloud, const int32_t* cloud_row0,
                    const int32_t* cloud_len, int32_t q_cloud_begin, int32_t n_q_clouds, int32_t kv_cloud_offset,
                    int32_t max_chunks, float* dq, int64_t lddq, float* dk, float* dv, int64_t lddkv,
                    void* workspace, int64_t workspace_bytes, void* stream);
/* dy[i] = y[i] > 0 ? dy[i] : 0 (n % 4 == 0). */
int scream_relu_bwd(float* dy, const float* y, int64_t n, void* stream);
/* y += x (n % 4 == 0). */
int scream_add_f32(float* y, const float* x, int64_t n, void* stream);
/* out[C][R] = in[R][C]. */
int scream_transpose_f32(const float* in, int32_t R, int32_t C, float* out, void* stream);
/* coor_mlp head backward (data): dH[r,k] = (H[r,k] > 0) sum_j dout[r,j] W[j,k]; W [3,256], H the relu output in front. */
int scream_coor_head_bwd(const float* dout, const float* W, const float* H, float* dH, int64_t rows, void* stream);
/* P[j][k] (+)= sum_r s[r][j] w[r][k] for w [rows,256] and s [rows,3] (s - center[cloud of the row] when center is given:
 * the embedding's input), written to dW as [3][256] or, transpose_w != 0, [256][3]; col_w [256] / col_s [3] (may be NULL)
 * receive the column sums of w / s.  workspace: scream_grad3_workspace_bytes(rows). */
int64_t scream_grad3_workspace_bytes(int64_t rows);
int scream_grad3(const float* w, const float* s, const float* center, const int32_t* tile_cloud, int64_t rows,
                 float* dW, int32_t transpose_w, float* col_w, float* col_s, int32_t accumulate, void* workspace,
                 int64_t workspace_bytes, void* stream);
/* The sum in front of pre_norm, PE_sine(xyz) + W_e (xyz - center[cloud]) + b_e, as scream_pe_embed_ln computes it, without
 * the LayerNorm (the training forward normalises with scream_ln_fwd and keeps the statistics). */
int scream_pe_embed(const float* xyz, const int32_t* tile_cloud, const float* center, const float* dim_t,
                    const float* emb_w, const float* emb_b, float* z, int64_t rows, void* stream);

/* ---- Depth renderer of the training-time GAN loss (models/render.py:8-73, RegistrationRender; csrc/render.hip).
 * For pair p and view v (rot [n_views, 9], row-major fp32 3x3 matrices R_v), every point of the pair's source cloud (packed
 * rows s_row0[p] .. + s_len[p] of src) and target cloud (t_row0 / t_len of tgt) is rotated, X = R_v x; then
 *   dmin, dmax = min / max of X_z over BOTH clouds (on the device; no host synchronisation),
 *   pv_k = 1 - (X_k,z - dmin) / (dmax - dmin),
 *   c_p = ((j - w/2 + 0.5) / (w/2), (i - w/2 + 0.5) / (w/2)) for pixel p = i w + j (row i, column j),
 *   g_kp = exp(-rho^2 / 2 |X_k,xy - c_p|^2)  (rho^2 multiplies: exp(-288 d^2) at rho = 24; evaluated as one exp2),
 *   img[p] = max_k pv_k g_kp over the side's own points (channel 0: source, channel 1: target),
 * and writes imgs [n_pairs, n_views, 2, w, w] = (img - 0.5) / 0.5 with argmax [n_pairs, n_views, 2, w, w] (int32, the index of the
 * selected point inside its cloud).  Rules the reference leaves open:
 *   ties: the lowest point index within the side wins (torch on the CPU; torch on the GPU promises nothing);
 *   zero pixels: where the maximum is exactly 0 the argmax is -1 and the pixel passes no gradient (its points' g underflowed);
 *   flat views: dmax == dmin is 0 / 0 in the reference -- every pixel of both images of that view is NaN, argmax -1, no fault;
 *   empty clouds: rejected by the Python layer (scream_amd/render.py), as PackedBatch does.
 * Results are bitwise the same however many pairs share the call (the point ranges are split over blocks and merged with an
 * integer atomicMax of (value, ~index) keys, which does not depend on the order).  w % 64 == 0 (the reference renders 64 x 64
 * chunks), n_views >= 1, rho finite, n_pairs * n_views * 2 <= 65535.  max_s_len / max_t_len (host) bound the cloud lengths and
 * size the grid; src_rows_total is the row count of src (it sizes the backward's part of the workspace).
 * workspace: scream_render_workspace_bytes(n_pairs, n_views, w, src_rows_total) bytes, 16-byte aligned; it begins with the depth
 * ranges, which scream_render_depth_bwd reads: hand the backward the forward's workspace, untouched. */
int64_t scream_render_workspace_bytes(int32_t n_pairs, int32_t n_views, int32_t w, int64_t src_rows_total);
int scream_render_depth(const float* src, const int32_t* s_row0, const int32_t* s_len, const float* tgt,
                        const int32_t* t_row0, const int32_t* t_len, int32_t n_pairs, int32_t max_s_len, int32_t max_t_len,
                        int64_t src_rows_total, const float* rot, int32_t n_views, int32_t w, float rho, float* imgs,
                        int32_t* argmax, void* workspace, int64_t workspace_bytes, void* stream);
/* Backward of the source images: dsrc[row] = sum over views (ascending) of R_v^T sum over the pixels p of the view's source image
 * whose argmax is that point (raster order) of dimgs[p] do_p/dX, with do/dX_x = -2 rho^2 pv g (X_x - c_x) (same for y) and
 * do/dX_z = -2 g / (dmax - dmin) (dmin, dmax constants, as the reference's .item() makes them).  The target channel of dimgs is
 * not read (no caller differentiates the target).  Fixed-order sums, no float atomics: two identical calls give identical bits.
 * Rows of src outside every source cloud are not written.  argmax and workspace: those of the scream_render_depth call. */
int scream_render_depth_bwd(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t n_pairs, int32_t max_s_len,
                            int64_t src_rows_total, const float* rot, int32_t n_views, int32_t w, float rho,
                            const float* dimgs, const int32_t* argmax, void* workspace, int64_t workspace_bytes, float* dsrc,
                            void* stream);

/* ---- voxel_down_sample of a batch of clouds (open3d's legacy voxel_down_sample as the reference calls it on every cloud it
 * feeds the models: process_3d_match.py:30-32, process_kitti.py:55-56, datasets/kitti.py:137-138, datasets/open_gf.py:22,42,62;
 * csrc/voxel.hip).  Cloud c is rows row0[c] .. + len[c] of xyz [rows,3]; the clouds need no 128-row alignment here and must not
 * overlap.  Per cloud, with v = voxel[c] (DEVICE doubles, one per cloud):
 *   origin = min_bound - v / 2                 (min_bound the exact per-axis fp32 minimum, the rest in float64),
 *   (i, j, k) = floor((p - origin) / v)        (float64 from the fp32 coordinate, a real division),
 *   one output row per occupied voxel = the float64 sum of its points in ascending row index, divided in float64 by their
 *   number and rounded once to fp32; rows in ascending (i, j, k), i most significant (the order of np.unique(axis=0)),
 * written to out_xyz rows row0[c] .. + out_len[c] (out_xyz [rows,3]: compact from the cloud's own first row; the rows behind are
 * not written), their point counts to out_count [rows] at the same rows unless out_count is NULL, and the number of voxels to
 * out_len[c].  Fixed-order sums, no float atomics: the result is a pure function of the cloud -- bitwise repeatable, independent of
 * the other clouds of the call and equal bit for bit to the float64 numpy restatement of tests/voxel_ref.py.  Parity with open3d
 * itself is not pinned (its output order is that of a hash map).
 * Refused clouds are reported, not faulted: out_len[c] = -1 and no rows for a cloud whose grid needs more than 2^21 cells on an
 * axis, that holds a non-finite coordinate, whose voxel is not a positive finite number, or whose rows break the bounds below;
 * the other clouds are unaffected.  len[c] = 0 gives out_len[c] = 0.
 * max_len (host) bounds every len[c] and sizes the grids.  workspace: scream_voxel_workspace_bytes(rows_total, n_clouds) bytes,
 * 16-byte aligned, rows_total (<= 2^31 - 1) the row count of xyz: the rows the workspace was sized for are recovered from
 * workspace_bytes, every cloud must end inside them, and less than scream_voxel_workspace_bytes(max_len, n_clouds) is
 * SCREAM_EINVAL.  n_clouds <= 65535 (SCREAM_EUNSUPPORTED beyond); n_clouds = 0 does nothing.  The passes of the radix sort a cloud
 * does not need are skipped on the device; the call never synchronises with the host. */
int64_t scream_voxel_workspace_bytes(int64_t rows_total, int32_t n_clouds);
int scream_voxel_down_sample(const float* xyz, const int32_t* row0, const int32_t* len, int32_t n_clouds, int32_t max_len,
                             const double* voxel, float* out_xyz, int32_t* out_len, int32_t* out_count, void* workspace,
                             int64_t workspace_bytes, void* stream);

/* ---- Point-to-point ICP of RAW scans in float64 (csrc/icp_raw.hip): the pose refinement datasets/kitti.py:105-126 runs with
 * open3d.registration_icp on the unvoxelised scans (~120 k points each, +-80 m, radius 0.2 m, start pose from the odometry).
 * Parity with open3d itself is unpinned (it is not installed); the loop is open3d's published RegistrationICP with
 * TransformationEstimationPointToPoint, and tests/rawicp_ref.py restates every step below in numpy.
 * src / tgt: packed fp32 [rows,3] exactly as the .bin files hold them (metric: there is no s / c); pair p is rows
 * src_row0[p] .. + src_len[p] and tgt_row0[p] .. + tgt_len[p]; the clouds of a batch may be packed in any order.  T float64
 * [n_pairs,16] (row-major 4x4) holds the start poses on entry and the results on return.  Every step is ONE IEEE float64
 * operation, in this order, without fma contraction:
 *   transform    a_k = ((t_k0 x + t_k1 y) + t_k2 z) + t_k3 from the fp32 row
 *   distance     d2 = (dx^2 + dy^2) + dz^2 with d = a - b (direct differences; b the fp32 target row)
 *   selection    the nearest target row wins; equal d2 goes to the LOWEST original target row
 *   rule         a correspondence iff d2 < r2, STRICTLY, r2 = the double product max_corr_dist * max_corr_dist (the FLANN rule)
 *   grid         origin = min_bound - h / 2 over the target, cell edge h = max_corr_dist, cell(v) = floor((v - origin) / h) per
 *                axis for source and target alike, a query scans cell(a - R) .. cell(a + R) per axis.  The grid only filters:
 *                the result equals the brute-force search bit for bit
 *   sums         count, sum d2, sum a, sum b, sum a b^T (with b widened) per evaluation.  A chunk = 256 consecutive source rows,
 *                a row without a correspondence contributing 0.0; inside a chunk each wave of 64 rows by the butterfly
 *                v += v[lane ^ 1], ^ 2, ^ 4, ^ 8, ^ 16, ^ 32, then the four waves as (w0 + w1) + (w2 + w3); the chunk sums of a
 *                pair sequentially in ascending chunk order from 0.0.  No float atomics: a pair's result depends neither on its
 *                batch nor on how the schedule was cut
 *   evaluation   fitness = cnt / N (0 for N = 0), inlier_rmse = sqrt(sum d2 / cnt) (0 for cnt = 0)
 *   update       cA = sum a / cnt, cB = sum b / cnt (no + 1e-6); H = sum a b^T - cA (sum b)^T; R = V diag(1, 1, det) U^T from
 *                the float64 Jacobi SVD of csrc/svd3.h, entries (V_i0 U_j0 + V_i1 U_j1) + delta V_i2 U_j2;
 *                t = cB - R cA with (R_i0 cA_0 + R_i1 cA_1) + R_i2 cA_2; T <- dT . T accumulated in k order
 *   stop         after the evaluation where |d fitness| < rel_fitness and |d rmse| < rel_rmse (float64, against the previous
 *                evaluation), or after max_iter updates.  iters = the number of updates applied
 * An evaluation without correspondences (an empty source included) takes the identity as its update and goes on: T stays the
 * start pose bit for bit, and iters follows the rule documented for scream_icp_p2p (1 with positive thresholds, max_iter with a
 * zero threshold, 0 for max_iter = 0).
 * Pair status: a pair whose target needs more than 2^21 cells on an axis, that holds a non-finite coordinate, whose rows do not
 * fit (row0 < 0, len < 0 or > max_*_len, row0 + len > *_rows_total), or any pair of a call whose radius is not positive and
 * finite, gets iters = -1, its T is untouched and its flag is set; the other pairs are unaffected.
 * scream_icp_raw_range follows scream_icp_p2p_range: it enqueues iterations [it_begin, it_end) of the run (iteration `it` =
 * search under T_it, then evaluation it: stop or update; max_iter + 1 iterations at most), it_begin == 0 also does the set-up
 * (grid, records, status), every call of a run gets the same arguments and workspace, the per-pair stopped flags are copied to
 * done_flags [n_pairs] (device int32, may be NULL), and nothing ever waits for the device.  fitness_rmse [n_pairs,2] float64 and
 * iters may be NULL.  workspace: scream_icp_raw_workspace_bytes bytes, 256-byte aligned.  n_pairs <= 65535.
 * scream_icp_raw_nn is the loop's search alone under the given T: idx int32 [src_rows_total] (-1: no target row with d2 < r2) and
 * d2 float64 (+inf for none) at every row of every accepted pair (other rows are not written), status int32 [n_pairs] (0 / -1,
 * may be NULL). */
int64_t scream_icp_raw_workspace_bytes(int64_t src_rows_total, int64_t tgt_rows_total, int32_t n_pairs);
int scream_icp_raw_range(const float* src, const float* tgt, const int32_t* src_row0, const int32_t* src_len,
                         const int32_t* tgt_row0, const int32_t* tgt_len, int32_t n_pairs, int32_t max_src_len,
                         int32_t max_tgt_len, int64_t src_rows_total, int64_t tgt_rows_total, double max_corr_dist,
                         int32_t max_iter, double rel_fitness, double rel_rmse, double* T, double* fitness_rmse, int32_t* iters,
                         int32_t it_begin, int32_t it_end, int32_t* done_flags, void* workspace, int64_t workspace_bytes,
                         void* stream);
int scream_icp_raw_nn(const float* src, const float* tgt, const int32_t* src_row0, const int32_t* src_len,
                      const int32_t* tgt_row0, const int32_t* tgt_len, int32_t n_pairs, int32_t max_src_len, int32_t max_tgt_len,
                      int64_t src_rows_total, int64_t tgt_rows_total, double radius, const double* T, int32_t* idx, double* d2,
                      int32_t* status, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- DSM extraction for a batch of OpenGF windows (the reference's process_open_gf.py:219-228: for every ground point, the
 * highest window point within the radius in the xy plane; csrc/dsm.hip).  Cloud c's window points ("patch") are rows
 * p_row0[c] .. + p_len[c] of patch [patch_rows_total,3], its ground points ("dem") rows d_row0[c] .. + d_len[c] of dem
 * [dem_rows_total,3] (DEVICE int32 arrays; no 128-row alignment; the clouds must not overlap).  With q a dem row and p a patch
 * row of the same cloud, every step one IEEE operation:
 *   R   = float64(float32(radius));  R2 = R * R                      (one float64 rounding; exact, R being an fp32 value)
 *   dx  = float32(p.x - q.x),  dy = float32(p.y - q.y)               (one fp32 rounding each, as the reference subtracts fp32 tensors)
 *   d2  = float64(dx)*float64(dx) + float64(dy)*float64(dy)          (both products exact in float64, so a contracted fma gives the same bits)
 *   p is a candidate of q  iff  d2 <= R2
 *   winner = the candidate with the largest z; equal z -> the LOWEST patch row index   (torch.max's first-maximum rule on patch[dis <= r])
 *   out_xyz = the winner's three fp32 coordinates unchanged, out_idx = its row;   no candidate: out_xyz = q unchanged, out_idx = -1
 * written at the dem's own rows: out_xyz [dem_rows_total,3], out_idx [dem_rows_total] (int32, the patch row relative to
 * p_row0[c]).  The reference compares the fp32 sqrt of the fp32 sum with 0.8; that differs from the above only for points within
 * about one fp32 ulp of the radius (tests/test_dsm_host.py pins it).  The result is a pure function of the cloud: bitwise
 * repeatable, independent of the other clouds of the call and of the launch geometry, equal bit for bit to the brute-force
 * float64 restatement of tests/dsm_ref.py.  The kernels use a per-cloud uniform 2-D grid with a bounded number of cells as a
 * conservative candidate filter (its cells grow with the extent: no cloud is refused for its size); the predicate above alone
 * decides membership.  No float atomics, no host synchronisation.
 * p_len[c] = 0: every dem row of the cloud returns itself with -1.  d_len[c] = 0 writes nothing.  n_clouds = 0 does nothing.
 * Non-finite coordinates are outside the contract (voxel_down_sample refuses such clouds upstream): no fault, no hang, the
 * values returned for them are unspecified.
 * SCREAM_EINVAL: a radius that is not a positive finite number; row totals outside 0 .. 2^31 - 1, max_p_len / max_d_len (host
 * bounds of every p_len[c] / d_len[c]) negative or beyond their totals; a workspace smaller than
 * scream_dsm_workspace_bytes(patch_rows_total, n_clouds, max_p_len) or not 16-byte aligned.  SCREAM_EUNSUPPORTED: n_clouds > 65535.
 * All of these are decided before any launch.  The per-cloud arrays live on the device and the call does not synchronise, so a
 * cloud whose own rows fall outside the arrays or exceed max_p_len / max_d_len is found on the device: it reads and writes
 * nothing, the other clouds are unaffected. */
int64_t scream_dsm_workspace_bytes(int64_t patch_rows_total, int32_t n_clouds, int32_t max_p_len);
int scream_dsm_extract(const float* patch, const int32_t* p_row0, const int32_t* p_len, int32_t max_p_len,
                       int64_t patch_rows_total, const float* dem, const int32_t* d_row0, const int32_t* d_len, int32_t max_d_len,
                       int64_t dem_rows_total, int32_t n_clouds, float radius, float* out_xyz, int32_t* out_idx, void* workspace,
                       int64_t workspace_bytes, void* stream);
/* The [n,6] sample rows of process_open_gf.py:234-242.  Cloud c is rows row0[c] .. + len[c] of dsm and dem (both [rows_total,3],
 * the dsm at the dem's rows as scream_dsm_extract writes it).  Per cloud and axis, in fp32 as numpy does on fp32 arrays:
 *   centre = float32(min + max) / 2   over the cloud's dsm and dem rows together (min and max are exact in any order),
 *   out[row] = float32(dsm - centre) | float32(dem - centre)          (out [rows_total,6]),
 * centre written to centre [n_clouds,3] (zeros for len[c] = 0).  Same refusals as above; a cloud whose rows fall outside the
 * arrays writes no rows and a zero centre. */
int scream_dsm_dem_assemble(const float* dsm, const float* dem, const int32_t* row0, const int32_t* len, int32_t n_clouds,
                            int32_t max_len, int64_t rows_total, float* out, float* centre, void* stream);

/* ---- Fixed-radius search for a batch of cloud pairs: every target point within the radius of every transformed source point
 * (the reference's utils.get_correspondences, utils.py:94-108, as datasets/three_d_match.py:106-113 calls it at 0.03 m to find
 * the overlap of a 3DMatch pair; csrc/radius.hip).  Pair p's source points are rows s_row0[p] .. + s_len[p] of src
 * [src_rows_total,3], its target points rows t_row0[p] .. + t_len[p] of tgt [tgt_rows_total,3] (fp32; DEVICE int32 arrays; no
 * 128-row alignment; the clouds must not overlap), M = T[p] its transform (DEVICE doubles, [n_pairs,16], row-major 4x4; the
 * last row is not read).  With x a source row i and b a target row j of the same pair, every step ONE IEEE float64 operation:
 *   a_k = ((M[k][0]*x0 + M[k][1]*x1) + M[k][2]*x2) + M[k][3]          (x converted exactly from fp32)
 *   d_k = a_k - float64(b_k)
 *   d2  = (d0*d0 + d1*d1) + d2*d2
 *   R2  = radius * radius
 *   j is a neighbour of i  iff  d2 < R2                                 (STRICT: a point exactly at the radius is not one)
 * This is FLANN's radius rule as open3d's search_radius_vector_3d uses it, up to how each evaluates the distance: the two can
 * differ only for points exactly at the radius (to within the rounding of d2).  Parity with open3d itself is not pinned (it
 * is not installed here).
 *   count[row of i] = the number of neighbours of i, before any K                                      (scream_radius_count)
 *   pair_j[offset[row] .. offset[row] + min(count, K)) = the neighbours of i in ascending (d2, j)      (scream_radius_pairs)
 * -- nearest first, as FLANN's sorted search returns them; equal d2 goes to the LOWEST target row (that tie rule is this
 * library's: FLANN's order among equal distances is unspecified).  Target rows are relative to t_row0[p].  K <= 0: no limit.
 * offset [src_rows_total + 1] (DEVICE int64) is the caller's exclusive prefix sum of min(count, K) over all source rows, with
 * the total in its last element; pair_j holds offset[last] int32 values.  A row writes at most offset[row + 1] - offset[row]
 * values and nothing outside 0 .. offset[last], whatever offset holds.
 * scream_radius_count fills the workspace (the target's cell lists); scream_radius_pairs reads it: hand it the SAME inputs and
 * the SAME workspace, untouched, as the count call.  The result is a pure function of the pair: bitwise repeatable, independent
 * of the other pairs of the call and of the launch geometry, equal to the brute-force float64 restatement of
 * tests/radius_ref.py.  The kernels use a per-pair uniform 3-D grid over the target (cell edge >= radius, at most 64^3 cells;
 * the cells grow with the extent: no cloud is refused for its size) as a conservative candidate filter; the predicate above
 * alone decides membership.  No float atomics, no host synchronisation in either call.
 * Cost: a source row evaluates (candidates in its 27 cells) distances to count and (candidates) x (neighbours + 1) to fill --
 * the rank of a neighbour is found by counting the smaller ones.  At 0.03 m on 0.025 m voxel clouds that is about ten
 * neighbours; a radius under which every point neighbours every point is correct but costs t_len^2 evaluations per source row.
 * s_len[p] = 0 writes nothing.  t_len[p] = 0 gives zero counts.  n_pairs = 0 does nothing.  Rows of count outside every pair
 * are not written.  Non-finite coordinates or matrices are outside the contract: no fault, no hang, values unspecified.
 * SCREAM_EINVAL: a radius that is not a positive finite number; row totals outside 0 .. 2^31 - 1, max_s_len / max_t_len (host
 * bounds of every s_len[p] / t_len[p]) negative or beyond their totals; a workspace smaller than
 * scream_radius_workspace_bytes(tgt_rows_total, n_pairs, max_t_len) or not 16-byte aligned.  SCREAM_EUNSUPPORTED: n_pairs > 65535.
 * All of these are decided before any launch.  A pair whose own rows fall outside the arrays or exceed max_s_len / max_t_len is
 * found on the device: it reads and writes nothing, the other pairs are unaffected. */
int64_t scream_radius_workspace_bytes(int64_t tgt_rows_total, int32_t n_pairs, int32_t max_t_len);
int scream_radius_count(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t max_s_len, int64_t src_rows_total,
                        const float* tgt, const int32_t* t_row0, const int32_t* t_len, int32_t max_t_len, int64_t tgt_rows_total,
                        const double* T, int32_t n_pairs, double radius, int32_t* count, void* workspace, int64_t workspace_bytes,
                        void* stream);
int scream_radius_pairs(const float* src, const int32_t* s_row0, const int32_t* s_len, int32_t max_s_len, int64_t src_rows_total,
                        const float* tgt, const int32_t* t_row0, const int32_t* t_len, int32_t max_t_len, int64_t tgt_rows_total,
                        const double* T, int32_t n_pairs, double radius, void* workspace, int64_t workspace_bytes, int32_t K,
                        const int64_t* offset, int32_t* pair_j, void* stream);

/* ---- Training-batch preparation: augment, normalise and pack B raw pairs in one call (the reference's augment() and unit-ball /
 * bounding-box normalisation, datasets/three_d_match.py:129-153,175-192 and datasets/kitti.py:233-273, per item on the host
 * there; csrc/prep.hip).  raw [raw_rows,3] holds every cloud back to back, fp32 or (raw_is_f64 != 0) float64; cloud q's rows
 * are raw_row0[q] .. + raw_len[q] (DEVICE int32 [2 n_pairs]: the sources of pairs 0 .. n_pairs - 1, then the targets); T and
 * perturb are DEVICE doubles [n_pairs,16], row-major 4x4 whose last rows are not read (perturb = identity: no perturbation);
 * side [n_pairs] DEVICE int32 (0: the source is perturbed, otherwise the target); sample_id [n_pairs] DEVICE int64; cloud_row0
 * [2 n_pairs] the packed first rows of PackedBatch.layout (every cloud padded to 128 rows).  mode 0: unit ball, 1: bounding box.
 *
 * Every step below is ONE IEEE float64 operation on the stated operands; fp32 input is widened first (exactly).
 *   chunk sum: the rows of a cloud in 256-row chunks, inside a chunk s = v[0]; s += v[1]; ... in ascending row order
 *   cloud sum: acc = chunk[0]; acc += chunk[1]; ... in ascending chunk order; a union: source chunks first, then target chunks
 *   3x3 products: every element (x*y + x*y) + x*y in ascending inner index;
 *   apply(R, t, x)_k = ((R[k][0]*x0 + R[k][1]*x1) + R[k][2]*x2) + t_k
 * 1. m = (cloud sum of the perturbed side's raw cloud) / n
 * 2. P'.R = P.R;  P'.t_k = (P.t_k + m_k) - ((P.R[k][0]*m0 + P.R[k][1]*m1) + P.R[k][2]*m2)          (the reference's C^-1 P C)
 * 3. side 0: q_k = -((P.R[0][k]*P'.t0 + P.R[1][k]*P'.t1) + P.R[2][k]*P'.t2);  T'.R = T.R P.R^T, T'.t = apply(T.R, T.t, q)   (T P'^-1)
 *            a = apply(P.R, P'.t, x) on source rows; a = x on target rows
 *    side 1: T'.R = P.R T.R, T'.t = apply(P.R, P'.t, T.t)   (P' T);  a = apply(P.R, P'.t, x) on target rows; a = x on source rows
 * 4. noise_std > 0:  a_k = a_k + noise_std * z_k on both clouds, z from Philox4x32-10 with counter (row inside the cloud,
 *    cloud: 0 source / 1 target, sample_id low word, high word) and key (seed low word, high word); with its output w0 .. w3,
 *    u_i = (w_i + 0.5) * 2^-32:  z_x = sqrt(-2 ln u0) * cos(2 pi u1), z_y = sqrt(-2 ln u0) * sin(2 pi u1),
 *    z_z = sqrt(-2 ln u2) * cos(2 pi u3), 2 pi the double 6.283185307179586.  The noise of a sample depends on (seed, sample_id,
 *    cloud, row) alone.  The device's log / sin / cos are not another library's to the last bit: with noise, outputs agree with
 *    a host restatement to within one fp32 neighbour, and are bitwise repeatable on the device.
 * 5. reg = apply(T'.R, T'.t, a) on source rows, a on target rows.
 *    mode 0 (three_d_match.py:183-186): c = (union sum of reg) / (N + M);  d = reg - c;  s = 1 / sqrt(max (d0*d0 + d1*d1) + d2*d2)
 *    mode 1 (kitti.py:268-273):         c = (lo + hi) / 2;  s = 1 / ((max_k (hi_k - lo_k)) / 2),  lo / hi the bounds of reg
 * 6. xyz = fp32(s * (a - c)) at the cloud's packed rows, every padding row exactly zero;  rot = fp32(T'.R);
 *    trans_k = fp32(s * ((T'.t_k - c_k) + ((T'.R[k][0]*c0 + T'.R[k][1]*c1) + T'.R[k][2]*c2)));  s, c, T_aug = T' in float64
 * 7. center [2 n_pairs,3]: target rows zero; source row p by center_rule
 *      0  fp32((cloud sum of the fp32 xyz rows of the source, widened) / N)      (what PackedBatch.from_pairs(None) means)
 *      1  trans                                                                   (train_3d_match.py:172)
 *      2  fp32(-R^T tr), k-th element -((T'.R[0][k]*tr0 + T'.R[1][k]*tr1) + T'.R[2][k]*tr2), tr the float64 trans before its
 *         rounding                                                                (train_kitti.py:156)
 * The result of a pair is a pure function of that pair: bitwise repeatable, independent of the other pairs of the call.  No
 * float atomics, no host synchronisation.  Non-finite coordinates and a union of zero extent (s is not finite) are OUTSIDE the
 * contract: values unspecified, no fault; nothing looks for them.
 * SCREAM_EINVAL: row totals outside 0 .. 2^31 - 1, max_len (host bound of every raw_len) outside 0 .. raw_rows, a mode /
 * center_rule outside the above, a negative or non-finite noise_std, a null pointer, a workspace smaller than
 * scream_prep_pairs_workspace_bytes(raw_rows, n_pairs, max_len) or not 16-byte aligned.  SCREAM_EUNSUPPORTED: n_pairs > 32767.
 * A pair whose rows leave raw / xyz or exceed max_len is found on the device: it reads and writes no row. */
int64_t scream_prep_pairs_workspace_bytes(int64_t raw_rows, int32_t n_pairs, int32_t max_len);
int scream_prep_pairs(const void* raw, int32_t raw_is_f64, int64_t raw_rows, const int32_t* raw_row0, const int32_t* raw_len,
                      int32_t max_len, const double* T, const double* perturb, const int32_t* side, double noise_std, uint64_t seed,
                      const int64_t* sample_id, int32_t mode, int32_t center_rule, const int32_t* cloud_row0, int32_t n_pairs,
                      int64_t rows_total, float* xyz, float* center, float* rot, float* trans, double* s, double* c, double* T_aug,
                      void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The L1 point loss of a packed batch (models/pointnet.py:93-99 and 163-167) and its gradient (csrc/prep.hip).
 *   loss_pair[p] = (cloud sum over the source rows of pair p of (|d0| + |d1|) + |d2|) / N_p,   d_k = float64(pred_k) - g_k
 *   loss         = fp32((loss_pair[0] + loss_pair[1] + ...) / n_pairs)
 * with the chunk and cloud sums above, in float64.  g = target row (fp32, widened) when target [rows_src,3] is given
 * (DEMTransformer); otherwise g_k = ((R[k][0]*x0 + R[k][1]*x1) + R[k][2]*x2) + t_k from the fp32 xyz row, rot [n_pairs,9] and
 * trans [n_pairs,3], all widened.  cloud_row0 / cloud_len are the batch's (the first n_pairs entries are read).
 *   dpred_k = fp32((float64(dout) * sign(d_k)) / (float64(N_p) * float64(n_pairs))),  sign(0) = 0;  padding rows zero
 * dout: one fp32 on the DEVICE.  SCREAM_EINVAL: null pointers, n_pairs / max_len / rows_src not positive, max_len > rows_src, a
 * workspace smaller than scream_l1_pairs_workspace_bytes(n_pairs, max_len).  A pair whose rows leave [0, rows_src) is skipped. */
int64_t scream_l1_pairs_workspace_bytes(int32_t n_pairs, int32_t max_len);
int scream_l1_pairs_fwd(const float* pred, const float* xyz, const float* rot, const float* trans, const float* target,
                        const int32_t* cloud_row0, const int32_t* cloud_len, int32_t n_pairs, int32_t max_len, int64_t rows_src,
                        double* loss_pair, float* loss, void* workspace, int64_t workspace_bytes, void* stream);
int scream_l1_pairs_bwd(const float* dout, const float* pred, const float* xyz, const float* rot, const float* trans,
                        const float* target, const int32_t* cloud_row0, const int32_t* cloud_len, int32_t n_pairs, int32_t max_len,
                        int64_t rows_src, float* dpred, void* stream);

/* ---- The Chamfer distance of packed cloud pairs (the ChamferDistance module of evaluate_open_gf.py:25-41: square_distance, two
 * min, two means) and its gradient (csrc/chamfer.hip; scream_amd/chamfer.py is the host layer, tests/chamfer_ref.py the numpy
 * restatement).  a [a_rows,3] and b [b_rows,3] fp32 packed; a_row0 / a_len / b_row0 / b_len [n_pairs] int32 on the DEVICE;
 * max_a_len / max_b_len host bounds of every a_len / b_len.  For pair p, N = a_len[p], M = b_len[p]:
 *
 * Forward, every step ONE rounded fp32 operation, no fma:
 *   d(n,m)     = ((dx*dx + dy*dy) + dz*dz),  dx = a_n.x - b_m.x, dy, dz likewise -- the DIFFERENCE form (the expansion
 *                -2ab + |a|^2 + |b|^2 of scream_nn_search cancels: coordinates of size 5 leave 3e-6 of error on a 4e-4 distance);
 *                d(n,m) has the same bits seen from a or from b
 *   d_ab[n]    = min over m of d(n,m);  idx_ab[n] = the LOWEST m that attains it (strict < scanning m upwards, the tie rule of
 *                scream_nn_search); d_ba[m], idx_ba[m] the same from the other side; indices count inside the pair's other cloud
 *   rows outside every cloud (the padding of a PackedBatch), and the rows of a pair with an empty side: idx = -1, d = 0
 *   S_ab       = float64 sum of the widened d_ab of the pair: 256-row chunks, inside a chunk s = v[0]; s += v[1]; ... in
 *                ascending row order, then acc = chunk[0]; acc += chunk[1]; ... (the chunk and cloud sums of scream_l1_pairs_fwd);
 *                S_ba likewise over d_ba
 *   loss_pair[p] = S_ab / N + S_ba / M  in float64 (two divisions, one addition);  0 when N == 0 or M == 0
 *   loss       = fp32((loss_pair[0] + loss_pair[1] + ...) / n_pairs)
 * Backward, the gradient of loss for the upstream dout (one fp32 on the DEVICE); every step ONE float64 operation, no fma, on
 * the fp32 coordinates widened (A, B); idx_ab / idx_ba are the forward's:
 *   g = float64(dout) / n_pairs;  w_ab = (2 g) / N;  w_ba = (2 g) / M
 *   da[n][k] = fp32((A_nk - B_jk) w_ab + acc w_ba),  j = idx_ab[n],
 *              acc = 0.0; acc = acc + (A_nk - B_mk) for every m with idx_ba[m] == n, IN ASCENDING m, one after the other
 *   db[m][k] = fp32((B_mk - A_ik) w_ba + acc w_ab),  i = idx_ba[m],  acc over the n with idx_ab[n] == m in ascending n
 *   every other row of da / db (padding, the rows of a pair with an empty side) is exactly zero.  da or db NULL: that side is
 *   skipped.
 * Scratch, as typed arrays (there is no workspace sizer): keys_a uint64 [a_rows], keys_b uint64 [b_rows], part double
 * [n_pairs * (ceil(max_a_len / 256) + ceil(max_b_len / 256))].  Outputs: idx_ab int32 / d_ab fp32 [a_rows], idx_ba / d_ba
 * [b_rows], loss_pair double [n_pairs], loss one fp32.  The backward needs no scratch: the scatter term is a re-scan of the
 * other side's indices in ascending order.  No float atomics (the blocks that share a long target cloud merge 64-bit
 * (distance, index) keys with an integer minimum), no host synchronisation; the result of a pair is a pure function of that
 * pair: bitwise repeatable, independent of the rest of the batch.  Non-finite coordinates are OUTSIDE the contract: values
 * unspecified, no fault (every index is clamped into its cloud before it addresses anything).
 * SCREAM_EINVAL: a null pointer (da / db excepted), n_pairs not positive, row totals outside 0 .. 2^31 - 1, max_a_len outside
 * 0 .. a_rows or max_b_len outside 0 .. b_rows, keys / part / loss_pair not 8-byte aligned.  SCREAM_EUNSUPPORTED: n_pairs >
 * 65535.  A pair whose rows leave a or b, or exceed the declared maxima, is found on the device and counts as empty. */
int scream_chamfer_fwd(const float* a, const int32_t* a_row0, const int32_t* a_len, int64_t a_rows, int32_t max_a_len,
                       const float* b, const int32_t* b_row0, const int32_t* b_len, int64_t b_rows, int32_t max_b_len,
                       int32_t n_pairs, uint64_t* keys_a, uint64_t* keys_b, double* part, int32_t* idx_ab, float* d_ab,
                       int32_t* idx_ba, float* d_ba, double* loss_pair, float* loss, void* stream);
int scream_chamfer_bwd(const float* dout, const float* a, const int32_t* a_row0, const int32_t* a_len, int64_t a_rows,
                       int32_t max_a_len, const float* b, const int32_t* b_row0, const int32_t* b_len, int64_t b_rows,
                       int32_t max_b_len, int32_t n_pairs, const int32_t* idx_ab, const int32_t* idx_ba, float* da, float* db,
                       void* stream);

/* ---- The optimiser step: torch.optim.Adam (weight_decay = 0, amsgrad = False, maximize = False) over every parameter of a
 * model in one launch (csrc/optim.hip; scream_amd/optim.py is its host layer, tests/adam_ref.py its numpy restatement).
 * tensors: DEVICE work list of n_tensors rows of SCREAM_ADAM_TENSOR_BYTES bytes, { float* p; const float* grad; float* m;
 * float* v; int64_t numel; }, every array contiguous fp32.  chunks: DEVICE int32 [n_chunks,2], (row of the work list, chunk
 * inside that tensor); chunk k of a tensor is its elements k * SCREAM_ADAM_CHUNK .. min((k + 1) * SCREAM_ADAM_CHUNK, numel),
 * one block each, so the caller lists ceil(numel / SCREAM_ADAM_CHUNK) chunks per tensor (none for an empty one).  A tensor
 * whose four bases are all 16-byte aligned moves in 16-byte accesses with its numel % 4 tail element by element; any other
 * tensor is handled element by element.  Nothing is read or written past numel.
 * state: DEVICE, 8-byte aligned, { double q1; double q2; float step; float unused; }: the running powers beta1^step and
 * beta2^step (both 1.0 before the first step) and the step count.  grad_scale / found_inf: optional fp32 DEVICE scalars
 * (a GradScaler's); lr, beta1, beta2, eps by value.
 *
 * Every step below is ONE IEEE float64 operation on the stated operands, from the fp32 values widened first:
 *   g   = double(grad) * inv,  inv = 1.0 / double(*grad_scale)  (1.0 without a grad_scale)
 *   m'  = m + (g - m) * (1 - beta1)
 *   v'  = (beta2 * v) + ((1 - beta2) * (g * g))
 *   q1' = q1 * beta1,  q2' = q2 * beta2
 *   step_size = lr / (1 - q1'),  denom = sqrt(v') / sqrt(1 - q2') + eps
 *   p'  = p - step_size * (m' / denom)
 * p', m' and v' are each rounded to fp32 once and stored; p' is computed from the unrounded m' and v'.
 * If found_inf is given and *found_inf != 0 the call changes nothing, bit for bit: not p, m, v, nor q1, q2, step.
 * Two launches on `stream`: the element kernel reads q1, q2 and computes q1', q2' for itself; a one-thread kernel BEHIND it
 * stores q1', q2' and step + 1 (no block of the first launch can still be reading what the second writes; there is no
 * double-buffering and the host keeps no step parity).  No atomics, no host synchronisation; bitwise repeatable.
 * step is fp32 as in torch: exact up to 2^24 steps.
 * SCREAM_EINVAL: negative counts, n_chunks > 2^31 - 1, a null or misaligned state, null tables with n_chunks > 0, tables not
 * 8-byte aligned, lr or eps negative or not finite, a beta outside [0, 1).  A chunk row that names no tensor of the list or
 * begins past its numel is skipped on the device. */
#define SCREAM_ADAM_CHUNK 4096
#define SCREAM_ADAM_TENSOR_BYTES 40
int scream_adam_step(const void* tensors, int32_t n_tensors, const int32_t* chunks, int64_t n_chunks, double* state,
                     const float* grad_scale, const float* found_inf, double lr, double beta1, double beta2, double eps,
                     void* stream);

/* ---- The adversarial loss: the PatchGAN discriminator NLayerDiscriminator(input_nc, ndf, n_layers = 3) of models/gan.py:15-65,
 * its backward, and the hinge losses of loss.py:31-35,53-66 (csrc/gan.hip; scream_amd/gan.py is the host layer, tests/gan_ref.py
 * the float64 restatement).  Every tensor is contiguous NCHW fp32, weights are torch's [Cout,Cin,4,4]; no image of either is kept.
 *
 * Convolution (kernel 4, padding 1, stride s in {1, 2}):
 *   y[n,co,oh,ow] = b[co] + sum over (ci, kh, kw) of w[co,ci,kh,kw] x[n,ci,oh s - 1 + kh,ow s - 1 + kw],  zero outside the image,
 *   Ho = floor((H - 2) / s) + 1, Wo likewise from W; H and W independent, odd allowed, both >= 2.
 * Forward, data gradient and weight gradient are implicit GEMMs on v_mfma_f32_32x32x2_f32: fp32 products, fp32 fma chains.  The
 * contraction -- (ci,kh,kw) forward, (co,kh,kw) for dx, the pixels (n,oh,ow) for dw -- is cut into z equal ranges of whole
 * 8-element steps, z a function of the shape alone; each range is summed in ascending index from 0, and a second launch adds
 * the z partial results of an element in ascending range order, then the bias.  dbias[co] is the float64 block sum (below) of dy
 * over n and the pixels.  No float atomics anywhere: two identical calls give identical bits.
 *   scream_gan_conv_fwd    y = conv(x) (+ bias unless NULL), then x > 0 ? x : 0.2 x when leaky != 0
 *   scream_gan_conv_dgrad  dx = the gradient of x for dy; with mask [n,cin,h,w] != NULL, dx *= (mask > 0 ? 1 : 0.2)
 *   scream_gan_conv_wgrad  dw [cout,cin,4,4] and, unless NULL, dbias [cout]
 * workspace: scream_gan_conv_workspace_bytes(mode, ...) bytes (mode 0 forward, 1 dgrad, 2 wgrad), 16-byte aligned, as must be w.
 * SCREAM_EINVAL: null pointers, sizes not positive, a stride other than 1 or 2, a tensor of 2^30 elements or more, a short
 * workspace.
 *
 * Float64 block sum of a channel (or of a whole tensor): the elements in the order n-major, pixel-minor; thread t of 256 adds
 * elements t, t + 256, ... from 0.0; then v[t] += v[t + 128], v[t] += v[t + 64], ... v[0] += v[1].
 *
 * BatchNorm2d in training mode, fused with LeakyReLU(0.2) (scream_gan_bn_fwd), per channel over cnt = n hw values:
 *   m = (sum x) / cnt, var = max((sum x^2) / cnt - m^2, 0) in float64 from the block sums; mean = fp32(m),
 *   invstd = fp32(1 / sqrt(var + 1e-5));  z = ((x - mean) invstd) gamma + beta, each operation rounded to fp32;  y = z > 0 ? z : 0.2 z
 *   running_mean = fp32(0.9 running_mean + 0.1 m), running_var = fp32(0.9 running_var + 0.1 var cnt / (cnt - 1)),
 *   *num_batches_tracked += 1 (int64 on the device; may be NULL).  cnt == 1 is SCREAM_EINVAL, as torch refuses it.
 * training == 0: mean = running_mean, invstd = fp32(1 / sqrt(running_var + 1e-5)), nothing is updated.
 * scream_gan_bn_bwd, for dy the gradient of y: dz = dy (y > 0 ? 1 : 0.2) -- the mask is the saved output's sign --
 *   dbeta = sum dz, dgamma = sum dz xhat (float64 block sums, xhat = fp32((x - mean) invstd) as the forward rounds it),
 *   dx = fp32(gamma invstd ((dz - dbeta / cnt) - xhat (dgamma / cnt))) in float64.  sums: 2 c doubles of scratch, 8-byte aligned;
 *   dgamma / dbeta may be NULL; dx may be dy.
 *
 * Losses, float64 block sums over all elements, one fp32 result on the device:
 *   scream_gan_loss_g   loss = fp32(-(sum logits) / cnt);                 bwd: dlogits = fp32(-dout / cnt)
 *   scream_gan_loss_d   loss = fp32(0.5 ((sum max(1 - real, 0)) / cnt_r + (sum max(1 + fake, 0)) / cnt_f)), 1 -+ x in fp32;
 *                       bwd: dreal = 1 - real > 0 ? fp32(-(0.5 dout) / cnt_r) : 0,  dfake = 1 + fake > 0 ? fp32((0.5 dout) / cnt_f) : 0
 *   (relu'(0) = 0).  dout: one fp32 on the DEVICE.
 *
 * The whole network on [n,cin,h,w] images: conv(s2, bias) leaky | conv(s2) bn leaky | conv(s2) bn leaky | conv(s1) bn leaky |
 * conv(s1, bias) -> logits [n,1,.,.]; channels cin -> ndf -> 2 ndf -> 4 ndf -> 8 ndf -> 1.  Supported: 1 <= cin <= 4,
 * ndf % 32 == 0, h and w >= 24 (SCREAM_EUNSUPPORTED otherwise).  workspace: scream_gan_workspace_bytes(n, cin, ndf, h, w) bytes,
 * 16-byte aligned, one carve: the activations a pass keeps (each layer's convolution output and activated output, mean and
 * invstd), two gradient buffers and the partial tiles of the convolution in flight.  scream_gan_backward takes the workspace
 * of the forward pass it differentiates, untouched in its activation part, with the same x and parameters; several passes may be
 * alive at once, each in its own workspace.  dx (may be NULL) and grads (may be NULL: then no weight gradient is computed) are
 * written, not accumulated.  scream_gan_backward differentiates a training-mode forward only. */
typedef struct {
    const float* w[5];                /* main.0, main.2, main.5, main.8, main.11 .weight */
    const float* b0;                  /* main.0.bias [ndf] */
    const float* b4;                  /* main.11.bias [1] */
    const float* gamma[3];            /* main.3, main.6, main.9 .weight */
    const float* beta[3];             /*                        .bias */
    float* running_mean[3];
    float* running_var[3];
    int64_t* num_batches_tracked[3];  /* each may be NULL */
} scream_gan_params_t;
typedef struct {
    float* w[5];
    float* b0;
    float* b4;
    float* gamma[3];
    float* beta[3];
} scream_gan_grads_t;
int64_t scream_gan_conv_workspace_bytes(int32_t mode, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w, int32_t stride);
int scream_gan_conv_fwd(const float* x, const float* wt, const float* bias, int32_t n, int32_t cin, int32_t cout, int32_t h,
                        int32_t w, int32_t stride, int32_t leaky, float* y, void* workspace, int64_t workspace_bytes, void* stream);
int scream_gan_conv_dgrad(const float* dy, const float* wt, const float* mask, int32_t n, int32_t cin, int32_t cout, int32_t h,
                          int32_t w, int32_t stride, float* dx, void* workspace, int64_t workspace_bytes, void* stream);
int scream_gan_conv_wgrad(const float* x, const float* dy, int32_t n, int32_t cin, int32_t cout, int32_t h, int32_t w,
                          int32_t stride, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);
int scream_gan_bn_fwd(const float* x, const float* gamma, const float* beta, float* running_mean, float* running_var,
                      int64_t* num_batches_tracked, int32_t n, int32_t c, int32_t hw, int32_t training, float* y, float* mean,
                      float* invstd, void* stream);
int scream_gan_bn_bwd(const float* dy, const float* y, const float* x, const float* gamma, const float* mean, const float* invstd,
                      int32_t n, int32_t c, int32_t hw, double* sums, float* dx, float* dgamma, float* dbeta, void* stream);
int scream_gan_loss_g(const float* logits, int64_t cnt, float* loss, void* stream);
int scream_gan_loss_g_bwd(const float* dout, int64_t cnt, float* dlogits, void* stream);
int scream_gan_loss_d(const float* real, int64_t cnt_r, const float* fake, int64_t cnt_f, float* loss, void* stream);
int scream_gan_loss_d_bwd(const float* dout, const float* real, int64_t cnt_r, const float* fake, int64_t cnt_f, float* dreal,
                          float* dfake, void* stream);
/* The ground-truth source rows that the `real` images are rendered from (train_3d_match.py:198), for every pair of a packed
 * batch in one launch: out[row] = ((R[k][0] x + R[k][1] y) + R[k][2] z) + t[k] in fp32, R = rot [n_pairs,9] and t = trans
 * [n_pairs,3] of pair tile_cloud[row / 128], over the rows_src packed source rows (a multiple of 128) of xyz. */
int scream_pairs_transform(const float* xyz, const float* rot, const float* trans, const int32_t* tile_cloud, int32_t n_pairs,
                           int64_t rows_src, float* out, void* stream);
int64_t scream_gan_workspace_bytes(int32_t n, int32_t cin, int32_t ndf, int32_t h, int32_t w);
int scream_gan_forward(const float* x, const scream_gan_params_t* params, int32_t n, int32_t cin, int32_t ndf, int32_t h, int32_t w,
                       int32_t training, float* logits, void* workspace, int64_t workspace_bytes, void* stream);
int scream_gan_backward(const float* dlogits, const float* x, const scream_gan_params_t* params, int32_t n, int32_t cin,
                        int32_t ndf, int32_t h, int32_t w, void* workspace, int64_t workspace_bytes, float* dx,
                        const scream_gan_grads_t* grads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SCREAM_HIP_H */
