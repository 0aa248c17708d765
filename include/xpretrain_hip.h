/*
 * xpretrain_hip.h -- C ABI of libxpretrain_hip.so: hand-written HIP (gfx950 / CDNA4) kernels for the
 * CLIP-ViP video-text contrastive hot path of microsoft/XPretrain.
 *
 * The reference has NO native/FFI layer (pure Python on torch/cuDNN/cuBLAS/apex/Horovod),
 * so every entry point below cites the reference *Python* call site whose arithmetic it replaces
 * (paths relative to /root/reference/CLIP-ViP/src).  The Python host side
 * (xpretrain_amd/modeling/) binds these through ctypes -- see INTEGRATION.md.
 *
 * Conventions (SURVEY.md §8b "C-ABI the new extension must export"):
 *   - plain pointers + sizes; no torch types.  Every pointer is a DEVICE pointer unless named host_*.
 *   - never allocates, never synchronises, never owns memory; launches only on `stream`
 *     (a hipStream_t passed as void*); re-entrant (forward thread + autograd thread).
 *     The three deviations an integrator must know, all documented at the entry point concerned: (1) xp_encoder_layer_bwd (and
 *     xp_encoder_layer_pooled_bwd) runs a layer's weight-gradient GEMMs on ONE library-owned stream per device (xp_side_stream(), created on first use, ordered against
 *     `stream` by library-owned events, joined before the call returns); (2) xp_set_cu_budget() is process-global planning state;
 *     (3) xp_attn_bwd / xp_attn_bwd2 enqueue one 4-byte hipMemsetAsync on `stream` (the fused backward's problem counter, inside the
 *     caller's workspace).
 *   - returns 0 on success, a negative XP_ERR_* otherwise; xp_last_error() gives the thread-local message.
 *   - `dtype`: element type of activations / GEMM operands (XP_BF16 or XP_F32).  Parameters that are read
 *     directly from the fp32 master copy (biases, LayerNorm affine, embedding tables) are always float.
 *     Every bf16 store of an fp32 value is one round-to-nearest-even, subnormals included (see xp_cast).
 *   - sizes are int64_t elements; `ld*` are row strides in elements.
 *   - Pointer alignment.  Every device pointer -- parameters and the pointer fields of the argument structs alike -- has one of two
 *     classes per (entry, operand), stated in the `align[entry]` comment in front of each prototype:
 *       need N   (N = 4, 8 or 16; `need 8/16`: 8 with bf16 storage, 16 with fp32 -- four elements per access)  the widest access a
 *                kernel of the entry makes through that pointer, LDS-DMA loads included.  A base that is not N-byte aligned is
 *                refused with XP_ERR_ARG on the host before anything is launched or written; xp_last_error() reads
 *                "<entry>: <operand>=<address> is not N-byte aligned".  A NULL pointer is aligned; whether an operand may be
 *                absent is the entry's own rule.
 *       any      every element-aligned base is served: the kernels behind that operand touch it one element at a time, or choose a
 *                wider path per call (per chunk, in the optimizer) only where every address involved allows it.  These are the
 *                operands the host side itself hands over at arbitrary element offsets: the optimizer's tensors and gradients
 *                (views of flat buffers), a launch table's slice of the norm partials, the rows xp_reduce_rows_batch sums,
 *                xp_sim_matrix and the streamed retrieval's features (and the statistics slice a gallery shard is searched with),
 *                the frame transforms' source bytes and output.
 *     `all need 16` stands for every operand the comment does not name.  No kernel issues a vector access at an address that is not
 *     a multiple of its width: what the hardware does with one is not something this library depends on.  Row pitches keep their
 *     own rules (`ld % 4`, `% 8`): base and pitch together decide the alignment of every row.  tests/alignment_cases.py is this
 *     table as data; tests/test_alignment_cpu.py holds the two together.
 */
#ifndef XPRETRAIN_HIP_H
#define XPRETRAIN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define XP_ABI_VERSION 1

enum { XP_BF16 = 0, XP_F32 = 1 };
enum { XP_OK = 0, XP_ERR_ARG = -1, XP_ERR_LAUNCH = -2, XP_ERR_UNSUPPORTED = -3 };

int xp_abi_version(void);
const char* xp_last_error(void);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C[M,N] = epilogue( sum_k A(m,k) * B(n,k) ).  One MFMA kernel family for every dense contraction on
 * the path: q/k/v/out projections (modeling/CLIP_ViP.py:341-343,379), MLP fc1/fc2 (:393-395), the
 * patch-embedding conv as a GEMM (:157-159,178), visual/text projections (:1142,1145), and their
 * autograd backward products (dX = dY.W, dW = dY^T.X).
 *
 * Operand storage: a_kstrided/b_kstrided == 0: row index major, k contiguous (A[m*lda + k]);
 *                  == 1: k major (A[k*lda + m]) -- read through LDS transpose loads, no copy.
 */
enum {
  XP_EPI_NONE = 0,       /* C = acc                                                              */
  XP_EPI_BIAS = 1,       /* C = acc + bias[n]                                                    */
  XP_EPI_BIAS_QSCALE = 2,/* C = (acc + bias[n]) * (n < scale_cols ? scale : 1)   q*dh^-0.5 (:341)  */
  XP_EPI_BIAS_GELU = 3,  /* aux = acc + bias[n];  C = aux * sigmoid(1.702 aux)   quick_gelu (:394); aux == NULL: the
                          * pre-activation is not stored (forward-only passes: retrieval / inference)        */
  XP_EPI_BIAS_RESID = 4, /* C = acc + bias[n] + resid[m,n]                       (:455,:460)       */
  XP_EPI_GELU_BWD = 5,   /* C = acc * d/dx quick_gelu(resid[m,n])                                 */
  XP_EPI_PATCH = 6,      /* C = acc + tab1[t,n] + tab2[l,n], t=(m%c_grp)/tab_L, l=m%tab_L (:182-185) */
  XP_EPI_SCALE = 7,      /* C = acc * scale                                                      */
  /* hidden_act "gelu" (transformers' GELUActivation, the erf form; LAION / OpenCLIP conversions): kinds 3 and 5 with the other
   * activation -- same operands, same planning (family, epilogue implementation, tile height, split, column sums, workspace), a
   * kernel instantiation of their own.  Phi / phi: the standard normal CDF / density; all math fp32. */
  XP_EPI_BIAS_GELU_ERF = 8, /* aux = acc + bias[n];  C = 0.5 aux (1 + erf(aux / sqrt 2)) = aux Phi(aux); aux == NULL as for kind 3 */
  XP_EPI_GELU_ERF_BWD = 9   /* C = acc * (Phi(r) + r phi(r)), r = resid[m,n]:  d/dx of the above                                  */
};

typedef struct XpGemmDesc {
  const void* A; const void* B; void* C;
  int64_t M, N, K;
  int64_t lda, ldb, ldc;
  int32_t a_kstrided, b_kstrided;
  int32_t in_dtype, out_dtype;          /* XP_BF16 / XP_F32 (out may be F32 with BF16 inputs)     */
  int32_t epilogue;
  int32_t split_k;                      /* >1: writes split_k fp32 slabs [split][M][N] to C, EPI_NONE */
  /* optional row remap  r -> (r / grp) * grp_stride + off + r % grp   (grp == 0: identity)        */
  int64_t a_grp, a_grp_stride, a_off;   /* applied to A's m index (row, or k-row when a_kstrided)  */
  int64_t c_grp, c_grp_stride, c_off;   /* applied to the output row (C, aux, resid)               */
  const float* bias;
  float scale; int64_t scale_cols;
  const void* resid; int64_t ldr;       /* dtype = in_dtype                                        */
  void* aux; int64_t ldaux;             /* dtype = out_dtype                                       */
  const float* tab1; const float* tab2; int64_t tab_L;
  /* optional: column sums of the FINISHED outputs (fp32, before rounding), one partial row per half tile height of rows:
   * colsum_partials[r*N + n], r < xp_gemm_colsum_rows(desc).  This is the bias gradient of the Linear whose output
   * gradient this GEMM produces (autograd computes it as grad.sum(0), CLIP_ViP.py:383-396) without re-reading it.
   * Only where xp_gemm_colsum_rows() > 0 (large bf16 problems, EPI_NONE / EPI_GELU_BWD / EPI_GELU_ERF_BWD); finish with
   * xp_reduce_rows_batch. */
  float* colsum_partials;
  /* reserved (round 3 selected a second kernel set of the 256-wide family here; since round 4 there is one): ignored */
  int32_t reserved0;
  int32_t side_M;
  /* optional, EPI_BIAS_RESID: fp32 "side rows" of the residual stream.  Output rows m with m % side_S < side_M (the video tower's
   * proxy tokens: rows [0, M) of every sample of S tokens, CLIP_ViP.py:187-197) take their residual operand from
   * resid_side[((m / side_S) * side_M + m % side_S) * N + n] (fp32) instead of resid, and their fp32 result is ALSO written to
   * out_side (same indexing) next to the rounded C row.  The pooled feature is token 0 of the last layer: keeping the residual
   * stream of these few rows in fp32 halves the feature error of the bf16 path (tools/residual_precision_experiment.py). */
  const float* resid_side; float* out_side; int64_t side_S;
  /* optional: A is not a matrix in memory but the patch matrix of a frame tensor, gathered by the operand loader -- the conv-as-GEMM
   * of CLIPVisionViPEmbeddings.patch_embedding (CLIP_ViP.py:157-159,178) without the im2col round trip.  a_frames: [BT,3,H,W], fp32 or
   * (a_frames_u8 = 1) decoded uint8 with the collate arithmetic (x / 255 - fr_mean[c]) / fr_std[c] (datasets/dataloader.py:209-233)
   * fused in; M = BT * (H/P) * (W/P) patches in (bt, gy, gx) order, K = 3*P*P in (c, dy, dx) order; A / lda are ignored.  The gathered
   * values are rounded to bf16 exactly as xp_im2col / xp_im2col_u8 round them (same result as the materialised matrix, bit for
   * bit).  bf16 compute, P % 8 == 0, no split-K. */
  const void* a_frames; int32_t a_frames_u8; int32_t fr_H, fr_W, fr_P; float fr_mean[3], fr_std[3];
  /* optional tile lists (all zero: the dense launch).  For operands that are zero outside a few tiles by construction: the launch
   * is PLANNED as the dense problem of the same M, N, K (family, split, slab length, grid order, epilogue) and only the listed
   * tiles are walked, so what it writes is bit-identical to the dense launch over such operands -- every skipped term is
   * acc + (+-0).  256-wide-family plans only, no row remap, no a_frames; anything else is refused.
   *   m_tiles (device, n_m_tiles ascending indices of 256-row tiles of M; the dX form: A k-contiguous, B k-strided): only these row
   *     tiles are computed; the output, aux and colsum_partials rows of every other tile are NOT written.
   *   k_tiles + k_tile_begin (device; the dW form: both operands k-strided): slab z (z < max(split_k, 1)) walks the 64-row k-tiles
   *     k_tiles[k_tile_begin[z] .. k_tile_begin[z + 1]) -- indices into the whole K, ascending, inside the slab's own k range.
   *     Every slab lists at least 2 (the pipeline depth; pad with k-tiles whose A rows are zero) and writes its output slab.
   *     k_tile_begin_host: the same split + 1 numbers in host memory, which the call validates. */
  const int32_t* m_tiles; int32_t n_m_tiles; int32_t reserved1;
  const int32_t* k_tiles; const int32_t* k_tile_begin; const int32_t* k_tile_begin_host;
} XpGemmDesc;

/* align[xp_gemm]: all need 16 */
/* (every pointer field of the descriptor, under the name "desc.<field>"; desc.a_frames of decoded uint8 frames, a_frames_u8 = 1,
 * need 8 as xp_im2col_u8's; k_tile_begin_host is host memory) */
int xp_gemm(const XpGemmDesc* desc, void* stream);

/* Split-K factor xp_gemm should be given for a weight-gradient-shaped problem (dW = dY^T X as computed by the
 * backward of nn.Linear inside CLIPEncoderLayer, modeling/CLIP_ViP.py:383-396,444-460): the 256-wide family's split that
 * fills one resident round of its workgroups, if the plan xp_gemm launches for `desc` with that split is 256-wide; else
 * the 128x128 family's split, which the plan may still run on the 256-wide family (desc->split_k and the data pointers
 * are ignored).  The value is always accepted by xp_gemm (whole k-steps per slab, no empty slab); 1 = no split. */
int32_t xp_gemm_auto_split(const XpGemmDesc* desc);
/* The same for a split-K launch that has SLACK: it runs on another stream beside the caller's work and nothing waits for it soon --
 * the first three weight-gradient GEMMs of an encoder layer's backward (fc2, fc1, out_proj: issued on the weight-gradient stream
 * while the dX chain of the layer still has attention and two GEMMs to go); the last one (q/k/v) is what the layer's join waits
 * for and takes xp_gemm_auto_split.  Fewer, longer slabs: less fp32 slab traffic beside the work it shares the chip with. */
int32_t xp_gemm_auto_split_slack(const XpGemmDesc* desc);
/* CUs the split-K planning may fill (64..256, default 256 or $XPRETRAIN_CU_BUDGET).  A data-parallel run lowers it by the number
 * of workgroups its collective library keeps resident during the backward pass (hvd.DistributedOptimizer's all-reduce,
 * run_pretrain.py:224-227,379; RCCL's gfx950 kernels own a CU per workgroup) so that a dW launch still fits one round. */
int xp_set_cu_budget(int32_t cus);
int32_t xp_get_cu_budget(void);
/* number of partial rows xp_gemm writes to desc->colsum_partials, read from the plan xp_gemm launches, or 0 if the fused
 * column sums are not available for this problem (desc->colsum_partials itself is ignored here) */
int64_t xp_gemm_colsum_rows(const XpGemmDesc* desc);
/* Output-tile height (rows) of the kernel family in the plan xp_gemm launches for `desc`: 256 for the 256-wide ping-pong family (the four
 * Linear layers of CLIPEncoderLayer at video-tower sizes, modeling/CLIP_ViP.py:341-343,379,393-395), 128 for the 128x128 family.
 * desc->split_k is honoured; the data pointers are ignored. */
int32_t xp_gemm_tile_rows(const XpGemmDesc* desc);

/* out[i] (+)= sum_z slabs[z*n + i], fp32; accumulate != 0 adds into out (gradient accumulation). */
/* align[xp_splitk_reduce]: all need 16 */
int xp_splitk_reduce(const float* slabs, float* out, int64_t n, int32_t splits, int32_t accumulate, void* stream);

/* Bias gradient: out[n] (+)= sum_m X[m*ldx + n]; workspace >= xp_colsum_workspace_bytes(). */
size_t xp_colsum_workspace_bytes(int64_t rows, int64_t cols);
/* align[xp_colsum]: all need 16 */
int xp_colsum(const void* X, int64_t rows, int64_t cols, int64_t ldx, int32_t dtype, float* out,
              int32_t accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* Deferred form: first level only.  partials[r*cols + n] = sum over the r-th chunk of rows of X[.][n];
 * xp_colsum_partial_rows(rows, cols) chunks.  Finish with xp_reduce_rows_batch. */
int64_t xp_colsum_partial_rows(int64_t rows, int64_t cols);
/* align[xp_colsum_partials]: all need 16 */
int xp_colsum_partials(const void* X, int64_t rows, int64_t cols, int64_t ldx, int32_t dtype, float* partials,
                       size_t partials_bytes, void* stream);

/* Batched deterministic column sums of up to XP_REDUCE_MAX_SEGS fp32 partial-row arrays in TWO launches:
 * out[c] (+)= sum_r in[r*stride + c], r < nrows, c < width.  Used to finish all bias and LayerNorm-parameter
 * gradients of one CLIPEncoderLayer backward (modeling/CLIP_ViP.py:444-460) at once.  segs_host is a HOST array. */
#define XP_REDUCE_MAX_SEGS 16
typedef struct {
  const float* in; float* out;
  int64_t stride;                        /* row pitch of `in`, elements                                  */
  int32_t nrows, width;
  int32_t accumulate, reserved;
} XpReduceSeg;
size_t xp_reduce_rows_batch_workspace_bytes(const XpReduceSeg* segs_host, int32_t n);
/* align[xp_reduce_rows_batch]: any: segs_host[].in segs_host[].out workspace */
int xp_reduce_rows_batch(const XpReduceSeg* segs_host, int32_t n, void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------- LayerNorm
 * nn.LayerNorm(eps=1e-5) of modeling/CLIP_ViP.py:404-406,855-857,720 (pre_layrnorm, layer_norm1/2,
 * post_layernorm, final_layer_norm).  Statistics in fp32; mean/rstd saved for the backward.
 */
/* align[xp_layernorm_fwd]: need 8/16: x y; all need 16 */
int xp_layernorm_fwd(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                     float* mean, float* rstd, int64_t rows, int64_t cols, float eps, int32_t dtype, void* stream);
/* The same with fp32 side rows of the residual stream (see XpGemmDesc::resid_side): row r with r % side_S < side_M is READ from
 * x_side[((r / side_S) * side_stride + r % side_S) * cols] (fp32) instead of x when x_side != NULL, and its fp32 result is ALSO
 * written to y_side (same indexing) when y_side != NULL (pre_layrnorm, CLIP_ViP.py:881: its output is the residual stream). */
/* align[xp_layernorm_fwd_side]: need 8/16: x y; all need 16 */
int xp_layernorm_fwd_side(const void* x, int64_t ldx, const float* gamma, const float* beta, void* y, int64_t ldy,
                          float* mean, float* rstd, int64_t rows, int64_t cols, float eps, int32_t dtype,
                          const float* x_side, float* y_side, int64_t side_S, int32_t side_M, int32_t side_stride, void* stream);
size_t xp_layernorm_bwd_workspace_bytes(int64_t rows, int64_t cols);
/* Deferred form: dx is final, the parameter gradients stay as xp_layernorm_bwd_partial_rows(rows) partial rows in
 * the workspace -- [dgamma(cols) | dbeta(cols)] (pitch 2*cols); with with_dx_colsum == 1
 * [dgamma | dbeta | colsum(dx)] (pitch 3*cols; the column sums of the dx just written = the bias gradient of the
 * Linear in front of this residual add); with with_dx_colsum == 2 (needs dres) [dgamma | dbeta | colsum(dx) | colsum(dres)]
 * (pitch 4*cols; in CLIPEncoderLayer's second LayerNorm, CLIP_ViP.py:455-458, dres is the layer's incoming gradient, whose
 * column sums are fc2's bias gradient) -- for xp_reduce_rows_batch.
 * colsum(dx) sums the fp32 values of dx BEFORE they are rounded to `dtype` (as the GEMM's fused column sums do): with bf16 it is
 * not the column sum of the stored dx.  dres may alias dx here too (same pointer and pitch: every row is read before it is written). */
int64_t xp_layernorm_bwd_partial_rows(int64_t rows);
/* align[xp_layernorm_bwd_partials]: need 8/16: dy x dres dx; all need 16 */
int xp_layernorm_bwd_partials(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                              const float* mean, const float* rstd, const void* dres, int64_t lddres,
                              void* dx, int64_t lddx, int32_t with_dx_colsum, int64_t rows, int64_t cols,
                              int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);
/* dx = (dres ? dres : 0) + LN'(dy);  dgamma/dbeta (+)= column sums.  dres may alias dx. */
/* align[xp_layernorm_bwd]: need 8/16: dy x dres dx; all need 16 */
int xp_layernorm_bwd(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                     const float* mean, const float* rstd, const void* dres, int64_t lddres,
                     void* dx, int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                     int64_t rows, int64_t cols, int32_t dtype,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The two backward forms with the fp32 side rows of x the forward normalised (xp_layernorm_fwd_side's x_side, same indexing): those
 * rows' x-hat is recomputed from the fp32 values, so the backward differentiates exactly the function the forward computed. */
/* align[xp_layernorm_bwd_partials_side]: need 8/16: dy x dres dx; all need 16 */
int xp_layernorm_bwd_partials_side(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                                   const float* mean, const float* rstd, const void* dres, int64_t lddres,
                                   void* dx, int64_t lddx, int32_t with_dx_colsum, int64_t rows, int64_t cols,
                                   int32_t dtype, const float* x_side, int64_t side_S, int32_t side_M, int32_t side_stride,
                                   void* workspace, size_t workspace_bytes, void* stream);
/* align[xp_layernorm_bwd_side]: need 8/16: dy x dres dx; all need 16 */
int xp_layernorm_bwd_side(const void* dy, int64_t lddy, const void* x, int64_t ldx, const float* gamma,
                          const float* mean, const float* rstd, const void* dres, int64_t lddres,
                          void* dx, int64_t lddx, float* dgamma, float* dbeta, int32_t accumulate,
                          int64_t rows, int64_t cols, int32_t dtype,
                          const float* x_side, int64_t side_S, int32_t side_M, int32_t side_stride,
                          void* workspace, size_t workspace_bytes, void* stream);

/* --------------------------------------------------------------------------------------- Attention
 * Fused attention on the packed projection output qkv[B, S, 3, H, 64] (row stride ldqkv elements; q is
 * already scaled).  head_dim is fixed at 64 (every CLIP ViT-B/L and text tower).
 *
 *  mode XP_ATTN_PROXY : CLIPAttention.forward2 (modeling/CLIP_ViP.py:332-381).  S = M + N*L; frame-n
 *                       queries attend [M proxies | frame n]; proxy queries attend everything.
 *  mode XP_ATTN_CAUSAL: CLIPAttention.forward text path (:266-330) with the additive -inf causal mask
 *                       (:788-797) and the finfo.min padding mask (_expand_mask :50-61); pad_mask is
 *                       int64 [B,S] (1 = keep) or NULL.  M,N,L ignored (pass 0,1,S).
 *
 * out[B,S,H*64] (row stride ldo).  stats[B,H,S,2] fp32 = (row max, log row sum) for the backward.
 *
 * Addressing limit (bf16; xp_attn_fwd, xp_attn_bwd, xp_attn_bwd2): the kernels reach one sample's rows through 32-bit offsets, so
 * S*ldqkv*2 and S*ldo*2 (the bytes from a sample's first row to its last) must both be < 4 GiB - 256 (0xFFFFFF00); a larger pitch
 * is refused with XP_ERR_ARG before any launch.  The whole operand (B samples) may be of any size.  fp32 mode has no such limit.
 */
enum { XP_ATTN_PROXY = 0, XP_ATTN_CAUSAL = 1 };
size_t xp_attn_workspace_bytes(int32_t mode, int64_t B, int64_t H, int64_t M, int64_t N, int64_t L);
/* align[xp_attn_fwd]: all need 16 */
int xp_attn_fwd(const void* qkv, int64_t ldqkv, void* out, int64_t ldo, float* stats,
                const int64_t* pad_mask, int32_t mode, int64_t B, int64_t H, int64_t S,
                int64_t M, int64_t N, int64_t L, int32_t dtype,
                void* workspace, size_t workspace_bytes, void* stream);
/* dqkv[B,S,3,H,64] (same layout as qkv; dq already multiplied by q_scale so it is the gradient of the
 * un-scaled projection output).  PROXY problems that fit one LDS group (M + L <= 208, M <= 16, no padding mask: 224^2 frames at patch
 * 16, any frame count) run as ONE persistent launch for dQ, dK and dV (attn_bwd5_kernel, round 6); its workgroups take problems from
 * a 4-byte device counter at the end of `workspace`, which this call resets with hipMemsetAsync on `stream` (the one operation of the
 * library besides kernel launches, event records and waits).  Everything else runs the dQ kernel, then the dK/dV kernel -- unless
 * the wide one-launch backward is switched on (below). */
/* align[xp_attn_bwd]: all need 16 */
int xp_attn_bwd(const void* qkv, int64_t ldqkv, const void* out, const void* dout, int64_t ldo,
                const float* stats, const int64_t* pad_mask, void* dqkv, float q_scale,
                int32_t mode, int64_t B, int64_t H, int64_t S, int64_t M, int64_t N, int64_t L, int32_t dtype,
                void* workspace, size_t workspace_bytes, void* stream);
/* Opt-in, off by default, process-global planning state like the CU budget: PROXY problems with 208 < M + L <= 1152 (M <= 16, no
 * padding mask, bf16: 448^2 frames at patch 16 have M + L = 788) run their backward as ONE persistent launch too (attn_bwd6_kernel:
 * one workgroup does a whole problem, walking 192-row groups of the other dimension; same workspace, counter and column-sum rows as
 * above) instead of the kernel pair.  The initial value is $XPRETRAIN_ATTN_BWD_WIDE (unset, empty or 0: off); the setter wins over
 * the environment.  With the switch off every plan, launch and output bit is what it was without this kernel. */
int xp_set_attn_bwd_wide(int32_t on);
int32_t xp_get_attn_bwd_wide(void);
/* The same with the bias gradients of q_proj / k_proj / v_proj on the way (autograd computes them as dqkv.sum(0),
 * CLIP_ViP.py:341-343): every backward workgroup also leaves the column sums of the dqkv rows it stores (as stored, i.e. rounded)
 * as one partial row: dqkv_colsum_partials[r * 3*H*64 + c], r < xp_attn_bwd_colsum_rows(...) -- finish with xp_reduce_rows_batch.
 * Saves the separate pass over dqkv.  xp_attn_bwd_colsum_rows() == 0 (fp32 mode): not available, pass NULL. */
int64_t xp_attn_bwd_colsum_rows(int32_t mode, int64_t B, int64_t H, int64_t S, int64_t M, int64_t N, int64_t L, int32_t dtype);
/* align[xp_attn_bwd2]: all need 16 */
int xp_attn_bwd2(const void* qkv, int64_t ldqkv, const void* out, const void* dout, int64_t ldo,
                 const float* stats, const int64_t* pad_mask, void* dqkv, float q_scale,
                 int32_t mode, int64_t B, int64_t H, int64_t S, int64_t M, int64_t N, int64_t L, int32_t dtype,
                 void* workspace, size_t workspace_bytes, float* dqkv_colsum_partials, void* stream);

/* The attention weights themselves (csrc/attention_probs.hip; `output_attentions=True`): what xp_attn_fwd never stores, rebuilt
 * from the qkv it read (same layout, q already scaled), the stats it wrote and the pad_mask it was given: entry (i, j) =
 * exp((s'_ij - max_i) - logsum_i), s' = finfo.min for a padded key (as _expand_mask adds it, :50-61) and the score otherwise.
 * Outputs are fp32 and contiguous, every element is written:
 *  XP_ATTN_CAUSAL: probs[B,H,S,S] = CLIPAttention.forward's attn_weights_reshaped (:303-311); entries above the diagonal are
 *                  exactly 0, a padded key of a row that sees a kept key is exactly 0, a row that sees only padded keys is uniform
 *                  over its i+1 visible keys (the reference's own behaviour).  probs_proxy must be NULL; M,N,L ignored.
 *  XP_ATTN_PROXY : probs[B,H,N,L,M+L] = forward2's first attn_weights (:350-358: frame-n queries over [M proxies | frame n], in
 *                  that column order), probs_proxy[B,H,M,S] = its second (:365-370: proxy queries over all keys).  The reference
 *                  computes both and drops them.  pad_mask must be NULL.
 * `dtype` is the storage of qkv; arithmetic is fp32.  No workspace; launches only on `stream`. */
/* align[xp_attn_probs]: all need 16 */
int xp_attn_probs(const void* qkv, int64_t ldqkv, const float* stats, const int64_t* pad_mask,
                  float* probs, float* probs_proxy, int32_t mode, int64_t B, int64_t H, int64_t S,
                  int64_t M, int64_t N, int64_t L, int32_t dtype, void* stream);

/* Single-query proxy attention (csrc/attention_pooled.hip): what the LAST layer of the video tower needs when only the pooled
 * feature leaves it (pooled_output = last_hidden_state[:, 0], modeling/CLIP_ViP.py:360-366).  Query row 0 of every sample is a
 * proxy row and attends all S keys (CLIPAttention.forward2): B*H problems of one query against S keys, a memory-bound pass over
 * K and V.  q[B, H*64] (already scaled); kv[B, S, 2, H, 64] = the packed K/V projection output (row stride ldkv elements);
 * out[B, H*64]; stats[B, H, 2] fp32 = (row max, log row sum).  Keys are cut into chunks so that B*H*chunks workgroups fill the
 * chip; chunk partials are combined in chunk order (no atomics: bit-identical run to run).  bf16 storage or fp32, fp32
 * arithmetic either way.  head_dim 64; no padding mask, no XP_ATTN_CAUSAL (the text tower pools at a per-sample EOS index and
 * is 0.6 % of the step's FLOPs). */
size_t xp_attn_pooled_workspace_bytes(int64_t B, int64_t H, int64_t S, int32_t dtype);
/* align[xp_attn_pooled_fwd]: all need 16 */
int xp_attn_pooled_fwd(const void* q, const void* kv, int64_t ldkv, void* out, float* stats, int64_t B, int64_t H, int64_t S,
                       int32_t dtype, void* workspace, size_t workspace_bytes, void* stream);
/* dq[b*lddq + h*64 + d] (already multiplied by q_scale, as xp_attn_bwd defines dq) and dkv[B, S, 2, H, 64] (row stride lddkv) for
 * ALL keys, in one pass over K/V.  dkv_colsum_partials (NULL: skipped): the column sums of the dkv rows as stored, one partial
 * row of 2*H*64 floats per (sample, chunk) -- xp_attn_pooled_colsum_rows() rows on the current device (0: no device), never more
 * than xp_attn_pooled_colsum_rows_max(); finish with xp_reduce_rows_batch (the k_proj / v_proj bias gradients). */
int64_t xp_attn_pooled_colsum_rows(int64_t B, int64_t H, int64_t S, int32_t dtype);
int64_t xp_attn_pooled_colsum_rows_max(int64_t B, int64_t S);
/* align[xp_attn_pooled_bwd]: all need 16 */
int xp_attn_pooled_bwd(const void* q, const void* kv, int64_t ldkv, const void* out, const void* dout, const float* stats,
                       void* dq, int64_t lddq, void* dkv, int64_t lddkv, float q_scale, int64_t B, int64_t H, int64_t S,
                       int32_t dtype, void* workspace, size_t workspace_bytes, float* dkv_colsum_partials, void* stream);

/* --------------------------------------------------------------------------------- Embeddings / glue
 * CLIPVisionViPEmbeddings.forward (modeling/CLIP_ViP.py:168-197).
 */
/* frames fp32 [BT,3,H,W] -> patch matrix [BT*gh*gw, 3*P*P] (dtype), k = (c,py,px): the conv-as-GEMM A operand */
/* align[xp_im2col]: all need 16 */
int xp_im2col(const float* video, void* patches, int64_t BT, int64_t H, int64_t W, int64_t P, int32_t dtype, void* stream);
/* Same patch matrix straight from DECODED uint8 frames [BT,3,H,W]: (x/255 - mean[c]) / std[c] -- the host collate's
 * /255 + transforms.Normalize (datasets/dataloader.py:209-233) resp. ImageNorm on the device
 * (datasets/data_utils.py:256-281) -- fused with the cast and the patch gather.  mean/std: HOST
 * float[3]. */
/* align[xp_im2col_u8]: need 8: frames; all need 16 */
int xp_im2col_u8(const uint8_t* frames, const float* mean3_host, const float* std3_host, void* patches, int64_t BT,
                 int64_t H, int64_t W, int64_t P, int32_t dtype, void* stream);
/* Raw decoded uint8 frames of ANY source resolution -> the fp32 model input, in one launch for a batch of videos: the CPU-worker
 * arithmetic of both dataset classes (datasets/dataset_video_retrieval.py:102-105: `.permute(0, 3, 1, 2).float() / 255.`, then
 * init_transform_dict_simple, datasets/dataloader.py:209-233: Resize(input_res, BICUBIC), CenterCrop(input_res), Normalize) on the
 * float image: bicubic overshoot outside [0, 1] is kept, nothing is re-quantised, no antialias filter (the reference's torch
 * predates it).  Each video has its own resolution and memory layout; out is fp32 [sum of T, 3, oh, ow], contiguous, in video
 * order, every element written and nothing else.  For output pixel (y, x) of a frame, X = flip ? ow-1-x : x:
 *     ry = top + y, rx = left + X                                     coordinates in the (never materialised) resized box
 *     sy = (ry + 0.5) * box_h / rh - 0.5;  iy = floor(sy), t = sy - iy   formed from the exact rational ((2 ry + 1) box_h - rh) / (2 rh)
 *     taps iy-1 .. iy+2, each clamped to [0, box_h-1], then + box_y;  Keys cubic-convolution weights, A = -0.75;  the same in x
 *     v = sum_j wy[j] * (sum_i wx[i] * u8[tap_y j][tap_x i])          fp32, the row sums first, fixed order: bit-reproducible
 *     out = (v / 255 - mean[c]) / std[c]
 * i.e. F.interpolate(box / 255, size=(rh, rw), mode="bicubic", align_corners=False)[top:top+oh, left:left+ow], normalised.
 * The descriptor table, mean and std are HOST arrays (copied into the kernel-argument block, so a call takes at most
 * XP_FRAMES_MAX_VIDEOS videos; callers with more issue several calls).  Refused before any launch, naming the argument: a null
 * pointer, n_videos outside [1, XP_FRAMES_MAX_VIDEOS], a non-positive size, a size above XP_FRAMES_MAX_SIZE, a box outside the
 * image, a window outside the resized image (there is no padding path), std <= 0, and a descriptor one of whose taps lies in
 * front of `src` or at or beyond `src + src_bytes`. */
#define XP_FRAMES_MAX_VIDEOS 32
#define XP_FRAMES_MAX_SIZE 16384              /* H, W, rh, rw, oh, ow: keeps (2 r + 1) * box inside int32 */
typedef struct {
  const uint8_t* src; int64_t src_bytes;        /* first byte of frame 0; extent of the allocation from there   */
  int64_t stride_t, stride_y, stride_x, stride_c; /* bytes: THWC, TCHW and sliced views are all just strides   */
  int32_t T, H, W;                              /* frames, source size                                          */
  int32_t box_y, box_x, box_h, box_w;           /* source region that is resized; taps clamp to ITS edges        */
  int32_t rh, rw;                               /* size of the (never materialised) resized image of the box     */
  int32_t top, left;                            /* where the oh x ow output window sits in the resized image     */
  int32_t flip;                                 /* != 0: output column x shows resized column left + ow-1-x      */
} XpFrameSrc;
/* align[xp_frames_resize_norm]: any: videos_host[].src out */
int xp_frames_resize_norm(const XpFrameSrc* videos_host, int32_t n_videos, const float* mean3_host,
                          const float* std3_host, float* out, int32_t oh, int32_t ow, void* stream);
/* The same launch with a choice of filter and an optional colour stage: the other two transform factories of the reference
 * (datasets/dataloader.py:180-207 init_transform_dict, :235-260 init_transform_dict_image).  xp_frames_resize_norm is untouched;
 * with XP_FRAMES_FILTER_BICUBIC and n_color = 0 this entry point returns its bits.
 *   filter XP_FRAMES_FILTER_BICUBIC    src.* read as above: RandomResizedCrop(BICUBIC) is box = the drawn crop, (rh, rw) = the output
 *                                      size, RandomHorizontalFlip is src.flip.  mid_*, crop_* are ignored.
 *   filter XP_FRAMES_FILTER_BILINEAR2  Resize(video_res), CenterCrop, Resize(input_res), all bilinear, without an intermediate image:
 *       the box is resized to mid_h x mid_w, the crop_h x crop_w window at (crop_y, crop_x) of THAT image is resized to rh x rw, and
 *       the output is the oh x ow window at (top, left) of the result.  Per axis, for resized coordinate r:
 *           s2 = max(0, ((2 r + 1) crop - out) / (2 out));  i = floor(s2), l2 = s2 - i;  m0 = crop0 + i, m1 = crop0 + min(i + 1, crop - 1)
 *           for m in (m0, m1): s1 = max(0, ((2 m + 1) box - mid) / (2 mid));  j = floor(s1), l1 = s1 - j;  taps box0 + j, box0 + min(j + 1, box - 1)
 *       (floor and fraction from integer division of the exact rational, as for the cubic) -- four taps per axis with the product
 *       weights (1-l2)(1-l1), (1-l2) l1, l2 (1-l1'), l2 l1': F.interpolate(mode="bilinear", align_corners=False) twice with the crop
 *       between, no antialias.  Accumulated exactly like the cubic: row sums first, fixed order.
 *   colour stage, n_color = 0 .. 3 ops applied in the order of color_op[] to x = v / 255 (overshoot kept up to here), before Normalize;
 *   torchvision's tensor backend (ColorJitter without contrast):
 *       XP_FRAMES_COLOR_BRIGHTNESS  x = clamp(f x, 0, 1)
 *       XP_FRAMES_COLOR_SATURATION  x = clamp(f x + (1 - f) gray, 0, 1),  gray = 0.2989 r + 0.587 g + 0.114 b
 *       XP_FRAMES_COLOR_HUE         x = hsv2rgb(h + f mod 1, s, v) of (h, s, v) = rgb2hsv(clamp(x, 0, 1)), |f| <= 0.5.  The clamp in front
 *                                   is this library's: torchvision's _rgb2hsv divides by maxc, which bicubic overshoot can make <= 0
 *                                   (a non-finite pixel); on in-range input the clamp is the identity.
 *       color_factor[k] belongs to color_op[k].  An op kind may appear once.
 * Calling rules and refusals are xp_frames_resize_norm's (at most XP_FRAMES_TRANSFORM_MAX_VIDEOS videos a call: the descriptor is
 * larger; the videos of one call share one filter, their colour stages may differ); in addition: an unknown filter, a filter that
 * differs from video 0's, a stage-1 size outside [1, XP_FRAMES_MAX_SIZE], a crop window outside the stage-1 image,
 * n_color outside [0, 3], an unknown or repeated colour op, a negative or non-finite brightness / saturation factor, a hue factor
 * outside [-0.5, 0.5]. */
#define XP_FRAMES_TRANSFORM_MAX_VIDEOS 24     /* 24 x (152 + 4) bytes of table in the 4 KiB kernel-argument block */
enum { XP_FRAMES_FILTER_BICUBIC = 0, XP_FRAMES_FILTER_BILINEAR2 = 1 };
/* (torchvision's ColorJitter op indices; 1 is contrast, which the reference never sets and this library does not provide) */
enum { XP_FRAMES_COLOR_BRIGHTNESS = 0, XP_FRAMES_COLOR_SATURATION = 2, XP_FRAMES_COLOR_HUE = 3 };
typedef struct {
  XpFrameSrc src;
  int32_t filter;                               /* XP_FRAMES_FILTER_*                                            */
  int32_t mid_h, mid_w;                         /* BILINEAR2: size of the (never materialised) stage-1 image     */
  int32_t crop_y, crop_x, crop_h, crop_w;       /* BILINEAR2: the window of the stage-1 image stage 2 resizes    */
  int32_t n_color;                              /* colour ops, 0 .. 3                                            */
  int32_t color_op[3];                          /* XP_FRAMES_COLOR_*, in the order of application                */
  float color_factor[3];                        /* the factor of color_op[k]                                     */
} XpFrameTransform;
/* align[xp_frames_transform]: any: videos_host[].src out */
int xp_frames_transform(const XpFrameTransform* videos_host, int32_t n_videos, const float* mean3_host,
                        const float* std3_host, float* out, int32_t oh, int32_t ow, void* stream);
/* xp_frames_transform with an antialias filter: what torchvision >= 0.17 computes for Resize / RandomResizedCrop on a float tensor
 * (antialias=True), i.e. F.interpolate(..., align_corners=False, antialias=True).  A SECOND definition, not a correction of the
 * first: the support widens with the scale, the weights are normalised per output coordinate, the window is truncated (not
 * clamped) at the box edge, and the cubic is Keys' with A = -0.5.  Per axis, `box` source pixels resized to `out`, k = 4 (BICUBIC)
 * or 2 (BILINEAR2):
 *     scale = box / out;  support = (k / 2) max(scale, 1);  inv = 1 / max(scale, 1)
 *     for resized coordinate r:  c = scale (r + 0.5);  x0 = max(int(c - support + 0.5), 0);  n = min(int(c + support + 0.5), box) - x0
 *     w_j = f((j + x0 - c + 0.5) inv) / sum_j f(...),  j = 0 .. n - 1;  f: Keys' cubic (A = -0.5) or the triangle
 *     resized pixel = sum_j w_j u8[box0 + x0 + j]: the horizontal pass first, then the vertical, taps in ascending order
 * (x0 and n come from integer arithmetic on (2 r + 1) box +- k max(box, out) + out over 2 out; where that quotient is an integer the
 * tap it adds or drops has weight f(k / 2) = 0.)  XP_FRAMES_FILTER_BILINEAR2 is box -> mid, the crop window, -> (rh, rw), each by
 * the rule above; both stages are separable and linear, so the library applies the composite per-axis rows W2[r, :] W1[crop0 + ., :]
 * and no intermediate image exists.  The window (top, left), the flip, the colour stage, /255 and Normalize are xp_frames_transform's.
 * Two launches on `stream` inside the one call: a table kernel writes x0, n and the weights -- formed in fp64, rounded once to
 * fp32 -- of every needed output coordinate of every video into `workspace`; the apply kernel stages the uint8 footprint of an
 * output tile in LDS and runs the horizontal pass, the vertical pass, the colour stage and Normalize in a fixed summation order
 * (two runs agree to the bit).  No allocation, no host synchronisation, no atomics.  `workspace` is device memory, 4-byte aligned,
 * of at least xp_frames_transform_aa_workspace_bytes(...) bytes (0 where the arguments would be refused); nothing outside
 * workspace[0, workspace_bytes) and `out` is written, nothing outside [src, src + src_bytes) is read.
 * Refused before any launch, naming the argument: everything xp_frames_transform refuses (the tap extent being this filter's), a
 * null or misaligned workspace, workspace_bytes below the sizing function's value, and a per-axis tap count above
 * XP_FRAMES_AA_MAX_TAPS.  The tap count of an axis is the width of its table rows, 2 ceil(support) + 1 (n never exceeds it); for
 * BILINEAR2 the composite's, ceil(scale1 (taps2 - 1)) + taps1.  3840 -> 224 bicubic has 71. */
#define XP_FRAMES_AA_MAX_TAPS 128
size_t xp_frames_transform_aa_workspace_bytes(const XpFrameTransform* videos_host, int32_t n_videos, int32_t oh, int32_t ow);
/* align[xp_frames_transform_aa]: any: videos_host[].src out; need 4: workspace */
int xp_frames_transform_aa(const XpFrameTransform* videos_host, int32_t n_videos, const float* mean3_host,
                           const float* std3_host, float* out, int32_t oh, int32_t ow, void* workspace, size_t workspace_bytes,
                           void* stream);
/* proxy rows: x[b, 0] = class_emb + pos[0]; x[b, 1+i] = added_cls[i] + pos[0]   (:187-191) */
/* align[xp_vip_proxy_rows]: all need 16 */
int xp_vip_proxy_rows(const float* class_emb, const float* added_cls, const float* pos, void* x,
                      int64_t B, int64_t S, int64_t M, int64_t D, int32_t dtype, void* stream);
/* gradients of class_embedding, added_cls, position_embedding[1+L], time table [T,D] from dx[B,S,D], S = M + T*L; each is an
 * fp32 sum in a fixed order (bit-reproducible) that is stored (accumulate == 0) or added to the destination with one add
 * (accumulate != 0).  LIMIT: D % 4 == 0 and D <= 1024 (one 256-thread block, four columns per lane); a larger D is refused.
 * d_added may be NULL when M == 1; d_time may be NULL (then no workspace is needed), otherwise `workspace` holds at least
 * xp_vip_embed_bwd_workspace_bytes(B, T, L, D) bytes.  Every refusal comes before the first launch: a refused call writes nothing. */
size_t xp_vip_embed_bwd_workspace_bytes(int64_t B, int64_t T, int64_t L, int64_t D);
/* align[xp_vip_embed_bwd]: all need 16 */
int xp_vip_embed_bwd(const void* dx, float* d_class, float* d_added, float* d_pos, float* d_time,
                     int64_t B, int64_t M, int64_t T, int64_t L, int64_t D, int32_t dtype, int32_t accumulate,
                     void* workspace, size_t workspace_bytes, void* stream);
/* The position table resampled to a patch grid it was not trained for: transformers' CLIPVisionEmbeddings.interpolate_pos_encoding
 * (the reference has no such step: its table must match the frame).  pos fp32 [1 + g0*g0, D] -> out fp32 [1 + gh*gw, D], every
 * element written and nothing else:
 *     out[0] = pos[0]                                                  bit for bit
 *     out[1 + y*gw + x] = sum_j wy[j] * (sum_i wx[i] * pos[1 + ty[j]*g0 + tx[i]])      fp32, the row sums first, fixed order
 *     per axis (length g, coordinate d): s = (d + 0.5) * g0 / g - 0.5;  i = floor(s), t = s - i from the exact rational
 *     ((2 d + 1) g0 - g) / (2 g);  taps i-1 .. i+2, each clamped to [0, g0-1];  Keys cubic-convolution weights, A = -0.75
 * i.e. F.interpolate(pos[1:].view(1,g0,g0,D).permute(0,3,1,2), size=(gh,gw), mode="bicubic", align_corners=False), no antialias.
 * xp_pos_resample_bwd is the transpose: d_out fp32 [1 + gh*gw, D] -> d_pos fp32 [1 + g0*g0, D] (overwritten, every element),
 *     d_pos[0] = d_out[0];   d_pos[1 + sy*g0 + sx] = sum_y sum_x (Wy[y,sy] * Wx[x,sx]) * d_out[1 + y*gw + x]
 * with Wy[y,sy] the sum (taps ascending) of row y's tap weights whose clamped index is sy; y ascending, then x ascending, zero
 * weights skipped, one thread per element, no atomics: bit-reproducible.  gh == gw == g0 is an exact identity (weights 0, 1, 0, 0),
 * but callers are expected not to launch it.  No workspace.  Refused before any launch: a null or not 16-byte aligned pointer,
 * g0 / gh / gw outside [1, 16384], D not a positive multiple of 4. */
/* align[xp_pos_resample_fwd]: all need 16 */
int xp_pos_resample_fwd(const float* pos, float* out, int32_t g0, int32_t gh, int32_t gw, int32_t D, void* stream);
/* align[xp_pos_resample_bwd]: all need 16 */
int xp_pos_resample_bwd(const float* d_out, float* d_pos, int32_t g0, int32_t gh, int32_t gw, int32_t D, void* stream);
/* CLIPTextEmbeddings.forward (:210-227): x[b,t] = tok[ids[b,t]] + pos[t] */
/* align[xp_text_embed_fwd]: all need 16 */
int xp_text_embed_fwd(const int64_t* ids, const float* tok, const float* pos, void* x,
                      int64_t B, int64_t Lt, int64_t D, int64_t vocab, int32_t dtype, void* stream);
/* d_tok[id] (+)= sum of dx[b,t] over the occurrences of id in (b,t) order (fixed order, no atomics: bit-reproducible);
 * d_pos[t] (+)= sum_b dx[b,t].  The rows of d_tok whose id does not occur in ids are zero with accumulate == 0 (all `vocab` rows
 * are cleared by one hipMemsetAsync on `stream`) and are left untouched with accumulate != 0.  Only rows 0 .. Lt-1 of d_pos are
 * written, in either mode: a longer position table keeps its other rows.  ids are not range-checked on the device. */
/* align[xp_text_embed_bwd]: all need 16 */
int xp_text_embed_bwd(const int64_t* ids, const void* dx, float* d_tok, float* d_pos,
                      int64_t B, int64_t Lt, int64_t D, int64_t vocab, int32_t dtype, int32_t accumulate, void* stream);
/* The same two with caller-given position_ids (:221-227, position_embedding(position_ids)); csrc/text_embed_pos.hip.  pos_ids is
 * int64 [pos_B, Lt] with pos_B == 1 (one map shared by every sample) or pos_B == B (a map per sample); pos is the fp32 table
 * [n_pos, D].  Lt is not bound by n_pos: only the ids are.
 *     x[b,t] = tok[ids[b,t]] + pos[pos_ids[b % pos_B, t]]        one fp32 add, one rounding to `dtype`: xp_text_embed_fwd's
 * so pos_ids[., t] == t gives xp_text_embed_fwd's bits.  A position id outside [0, n_pos) is decided on the device (no host
 * synchronisation, no read outside the table): every element of that output row is NaN and the other rows are not affected; in
 * the backward such a row adds to no row of d_pos and writes nowhere in it (d_tok does not look at pos_ids).  Token ids are not
 * range-checked on the device, as in xp_text_embed_fwd / _bwd.
 *     d_tok: the contract and the bits of xp_text_embed_bwd (all `vocab` rows cleared first with accumulate == 0)
 *     d_pos[p] (+)= sum of dx[b,t] over the occurrences of p in pos_ids as the rows read it, in (b,t) row order: the first row that
 *                  holds p adds all of p's rows, found 256 rows at a time -- fixed order, no atomics: bit-reproducible.
 * accumulate == 0: all n_pos rows of d_pos are written (one hipMemsetAsync on `stream` clears them; the rows no id names stay
 * zero); accumulate != 0: the rows no id names are untouched, the others take one add of the ordered sum.
 * Refused before any launch (or memset): a null pointer, B / Lt / vocab < 1, pos_B not in {1, B}, D not a positive multiple of 4,
 * n_pos < 1, B * Lt > INT32_MAX, a bad dtype. */
/* align[xp_text_embed_fwd_pos]: all need 16 */
int xp_text_embed_fwd_pos(const int64_t* ids, const int64_t* pos_ids, int64_t pos_B, const float* tok, const float* pos, void* x,
                          int64_t B, int64_t Lt, int64_t D, int64_t vocab, int64_t n_pos, int32_t dtype, void* stream);
/* align[xp_text_embed_bwd_pos]: all need 16 */
int xp_text_embed_bwd_pos(const int64_t* ids, const int64_t* pos_ids, int64_t pos_B, const void* dx, float* d_tok, float* d_pos,
                          int64_t B, int64_t Lt, int64_t D, int64_t vocab, int64_t n_pos, int32_t dtype, int32_t accumulate,
                          void* stream);
/* pooled[b] = x[b, idx[b]] (text: idx = ids.argmax(-1), :776 ; vision: idx = 0, :892) and its scatter */
/* align[xp_argmax_rows]: all need 16 */
int xp_argmax_rows(const int64_t* ids, int64_t* idx, int64_t B, int64_t Lt, void* stream);
/* align[xp_gather_rows]: all need 16 */
int xp_gather_rows(const void* x, const int64_t* idx, void* out, int64_t B, int64_t S, int64_t D, int32_t dtype, void* stream);
/* align[xp_scatter_rows]: all need 16 */
int xp_scatter_rows(const void* dout, const int64_t* idx, void* dx, int64_t B, int64_t S, int64_t D, int32_t dtype, void* stream);
/* x / ||x||_2 per row (:1148-1149); in `dtype`, out fp32 features; inv_norm saved.  No epsilon, like the reference's
 * x / x.norm(dim=-1, keepdim=True): a row of zeros gives inv_norm = +inf and a row of NaN in y (and in xp_l2norm_bwd's dx); the
 * other rows are not affected. */
/* align[xp_l2norm_fwd]: all need 16 */
int xp_l2norm_fwd(const void* x, float* y, float* inv_norm, int64_t rows, int64_t cols, int32_t dtype, void* stream);
/* align[xp_l2norm_bwd]: all need 16 */
int xp_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, void* dx, int64_t rows, int64_t cols,
                  int32_t dtype, void* stream);
/* fp32 master -> compute dtype copy (n % 4 == 0).  To bf16 it is round-to-nearest-even: ties to the even mantissa, a carry may
 * reach the exponent, values from 0x7F7F8000 up round to infinity, infinities and the sign of zero are kept, a NaN stays a NaN, and
 * fp32 subnormals are NOT flushed: they round onto the bf16 subnormals (measured on MI355X, tests/test_embed_contract_gpu.py).
 * xp_cast_back widens exactly; with accumulate != 0 it is dst = src + dst, one add per element. */
/* align[xp_cast]: all need 16 */
int xp_cast(const float* src, void* dst, int64_t n, int32_t dtype, void* stream);
/* align[xp_cast_back]: all need 16 */
int xp_cast_back(const void* src, float* dst, int64_t n, int32_t dtype, int32_t accumulate, void* stream);

/* ------------------------------------------------------------------------------------- Optimizer
 * On-device optimizer step: torch.nn.utils.clip_grad_norm_ as the training loops call it
 * (tasks/run_video_retrieval.py:390-392; coef = min(1, max_norm / (||g||_2 + 1e-6))) fused with AdamW.step
 * (optimization/adamw.py:40-103: denom = sqrt(v) + eps, step_size = lr * sqrt(1-b2^t) / (1-b1^t) when
 * correct_bias, decoupled weight decay p -= lr * wd * p AFTER the Adam update), over every parameter tensor in
 * one launch.  fp32 masters / moments / gradients; each tensor may name a shadow copy (bf16 or f32) that is
 * rewritten in the same pass (the compute-dtype weights the GEMMs read).  The clipped gradients themselves are
 * NOT written back (nothing on the path reads them after the step).
 *
 * Work is cut into chunks of XP_OPT_CHUNK elements of one tensor; `chunk_map` holds (tensor index, chunk index)
 * int32 pairs, one per workgroup, built once by the caller.  `table` and `chunk_map` are DEVICE arrays;
 * `grads_host`, `group_of_host` and `groups_host` are HOST arrays (copied into the kernel-argument block, so a
 * call takes at most XP_OPT_MAX_TENSORS tensors and XP_OPT_MAX_GROUPS hyper-parameter groups; callers with more
 * tensors issue several calls that share one partials array). */
#define XP_OPT_CHUNK 65536
#define XP_OPT_MAX_TENSORS 256
#define XP_OPT_MAX_GROUPS 16
typedef struct {
  void* p; void* m; void* v;            /* fp32 parameter, exp_avg, exp_avg_sq (xp_optim_step, XP_OPT_ADAMAX: exp_inf) */
  void* shadow;                         /* optional copy of p in shadow_dtype (NULL: none)              */
  int64_t numel;
  int32_t shadow_dtype;                 /* XP_BF16 / XP_F32                                             */
  int32_t reserved;
} XpAdamTensor;
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  float step_size;                      /* lr * sqrt(1-beta2^t) / (1-beta1^t) (or lr if !correct_bias)  */
} XpAdamGroup;
/* partials[c] = sum of squares of chunk c's gradient elements (fixed order, deterministic). */
/* align[xp_grad_sqnorm_partials]: any: table[].p table[].m table[].v table[].shadow grads_host[] partials; all need 16 */
int xp_grad_sqnorm_partials(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                            const void* const* grads_host, int32_t n_tensors, float* partials, void* stream);
/* norm_partials (nullable): ALL chunks' partial sums of squares (n_norm_partials of them); max_norm <= 0: no
 * clipping; grad_norm_out (nullable): receives ||g||_2 before clipping. */
/* align[xp_adamw_step]: any: table[].p table[].m table[].v table[].shadow grads_host[]; all need 16 */
int xp_adamw_step(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                  const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                  const XpAdamGroup* groups_host, int32_t n_groups, const float* norm_partials,
                  int32_t n_norm_partials, float max_norm, float* grad_norm_out, void* stream);

/* The other two values of the drivers' `optim` key (configs/config.py:135-137; optimization/utils.py:111-120 hands them to
 * torch.optim.Adam / torch.optim.Adamax with the grouped parameters, lr and betas): the same multi-tensor launch, clip, shadow
 * copies and tables as xp_adamw_step, with torch's single-tensor arithmetic (amsgrad = maximize = False); t = step count after the
 * increment, coef = the clip coefficient or 1:
 *     g = coef * g;  if (weight_decay != 0) g = g + weight_decay * p        coupled L2 on the CLIPPED gradient, before the moments
 *     m = beta1 * m + (1 - beta1) * g                                       evaluated as torch's lerp: m + one_minus_beta1 * (g - m)
 *   XP_OPT_ADAM     v = beta2 * v + (1 - beta2) * g * g
 *                   p = p - step_size * m / (sqrt(v) / bias2_sqrt + eps)
 *   XP_OPT_ADAMAX   u = max(beta2 * u, |g| + eps)                           eps inside the max operand; a NaN on either side stays
 *                   p = p - step_size * m / u
 * XpAdamTensor::v holds exp_avg_sq (Adam) or exp_inf (Adamax).  An element whose gradient is exactly 0 stays finite from the
 * first step on (Adam: 0 / (0 + eps); Adamax: u = eps) as long as eps > 0. */
enum XpOptKind { XP_OPT_ADAM, XP_OPT_ADAMAX };
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
  float step_size;                      /* lr / (1-beta1^t)                                             */
  float bias2_sqrt;                     /* sqrt(1-beta2^t); read by XP_OPT_ADAM only                    */
  float one_minus_beta1;                /* 1-beta1 formed in double, then rounded: the weight torch's lerp_ gets (1 - 0.8f is not 0.2f) */
} XpOptGroup;
/* Arguments as for xp_adamw_step.  An unknown kind is refused before any launch. */
/* align[xp_optim_step]: any: table[].p table[].m table[].v table[].shadow grads_host[]; all need 16 */
int xp_optim_step(int32_t kind, const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                  const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                  const XpOptGroup* groups_host, int32_t n_groups, const float* norm_partials,
                  int32_t n_norm_partials, float max_norm, float* grad_norm_out, void* stream);

/* The step guard (opt-in): a step whose global gradient norm is not finite leaves p, m, v untouched.  What apex's dynamic loss
 * scaling did beside scaling (a step with overflowing gradients is skipped; run_pretrain.py:234-236, 374-377 under amp), decided
 * on the device: no host synchronisation between the partials and the update.  Three kinds of call on ONE stream, in this order:
 *   xp_grad_sqnorm_partials   per launch table, into one partials array (always, also without clipping: the verdict needs it)
 *   xp_step_verdict           once, over ALL n_partials chunks of the step
 *   xp_*_step_guarded         per launch table, all reading the same verdict (a stream that forks behind xp_step_verdict may run some)
 * xp_step_verdict sums partials[0..n) in the order xp_adamw_step / xp_optim_step sum them, so `norm` has the bits their
 * grad_norm_out gets.  A gradient element that is finite but whose square overflows fp32 makes its partial, and the norm, infinite:
 * that step is skipped too.  `verdict` is a DEVICE struct the caller zeroes once and then only reads (copy it to the host behind
 * the launch to learn what happened); the counters are plain loads and stores by one lane, ordered by the stream. */
typedef struct {
  float norm;                           /* ||g||_2 over every chunk of the step, before clipping                              */
  int32_t finite;                       /* 1 iff isfinite(norm)                                                               */
  int32_t first_bad_chunk;              /* lowest chunk index whose OWN partial is not finite; -1: only the sum overflowed    */
  int32_t reserved;
  int64_t applied, skipped;             /* monotonic: each xp_step_verdict call adds 1 to exactly one of them                 */
} XpStepVerdict;
/* align[xp_step_verdict]: all need 16 */
int xp_step_verdict(const float* partials, int32_t n_partials, XpStepVerdict* verdict, void* stream);
/* Arguments as for xp_adamw_step / xp_optim_step, plus the verdict (device pointer, written by an earlier launch on an ordered stream).
 *   finite == 1: the twin's arithmetic, element for element, in the same rounding order; coef = min(1, max_norm / (verdict->norm + 1e-6)),
 *                max_norm <= 0: coef = 1.  norm_partials is not read again: it is here so that a caller swaps twin for twin, and
 *                max_norm > 0 without it is refused as in the twin.
 *   finite == 0: a workgroup neither reads nor writes m, v or the gradient and does not write p.  It rewrites its chunk of the shadow
 *                copy from the unchanged p (one read, a half-width write): whoever relies on "this step rewrote every shadow" still may.
 * grad_norm_out (nullable) receives verdict->norm in both cases.  The step count behind XpAdamGroup::step_size / XpOptGroup's bias
 * factors is the caller's: a skipped step must not count (optimization/multi_tensor.py takes the increment back).
 * A null verdict, an unknown kind and every argument error of the twin are refused before any launch. */
/* align[xp_adamw_step_guarded]: any: table[].p table[].m table[].v table[].shadow grads_host[]; all need 16 */
int xp_adamw_step_guarded(const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                          const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                          const XpAdamGroup* groups_host, int32_t n_groups, const float* norm_partials,
                          int32_t n_norm_partials, float max_norm, float* grad_norm_out,
                          const XpStepVerdict* verdict, void* stream);
/* align[xp_optim_step_guarded]: any: table[].p table[].m table[].v table[].shadow grads_host[]; all need 16 */
int xp_optim_step_guarded(int32_t kind, const XpAdamTensor* table, const int32_t* chunk_map, int32_t n_chunks,
                          const void* const* grads_host, const uint8_t* group_of_host, int32_t n_tensors,
                          const XpOptGroup* groups_host, int32_t n_groups, const float* norm_partials,
                          int32_t n_norm_partials, float max_norm, float* grad_norm_out,
                          const XpStepVerdict* verdict, void* stream);

/* ------------------------------------------------------------------------------------------- Loss (csrc/loss_family.hip)
 * The whole family of learnable-temperature contrastive losses of optimization/loss.py behind one entry: loss and every
 * gradient in one call (the backward just scales them), fp32, fixed reduction order (bit-reproducible), all launches on `stream`.
 * vis, txt [n,d]; img, cap [m,d]: gathered unit-norm features; log_scale: the LOG scale parameter (a device scalar).
 * With s = exp(*log_scale), S1 = s V T^T, S2 = s V C^T,
 * S3 = s I C^T, "rows(S)" = mean over i of (lse_j S_ij - S_ii) and "cols(S)" the same over columns:
 *   XP_LOSS_NCE            rows(S1) + cols(S1)                                         NCELearnableTempLoss          :134-141
 *   XP_LOSS_VS_VC          rows + cols of S1 and of S2                                 NCELearnableTempLoss_vs_vc    :212-225
 *   XP_LOSS_VS_VC_FC       VS_VC + rows(S3) + cols(S3)                                 NCELearnableTempLoss_vs_vc_fc :235-254
 *   XP_LOSS_VSC            cols(S1) + cols(S2) + mean_i(ra_i - S1_ii) + mean_i(rb_i - S2_ii) with merged negatives:
 *                          ra_i = lse(S1[i,:] U S2[i,j!=i]), rb_i = lse(S1[i,j!=i] U S2[i,:])    NCELearnableTempLoss_vsc :264-286
 *   XP_LOSS_VSC_FC         VSC + rows(S3) + cols(S3)                                   NCELearnableTempLoss_vsc_fc   :296-324
 *   XP_LOSS_VIDIMG         rows + cols of the [n+m, n+m] logits of [V;I] against [T;C]  VidImgNCELearnableTempLoss    :151-160
 *   XP_LOSS_VIDIMG_DIVIDE  rows + cols of S1 (mean over n) + rows + cols of S3 [m,m] (mean over m)
 *                                                                                      VidImgDivideNCELearnableTempLoss :170-183
 *   XP_LOSS_DSL            dual softmax, the prior NOT detached                        NCELearnableTempDSLLoss       :193-202
 *       A = S1, Pc = softmax over i of A (per column), Pr = softmax over j of A (per row), B1 = A o Pc, B2 = A o Pr
 *       loss = mean_i[lse_j B1_ij - B1_ii] + mean_j[lse_i B2_ij - B2_jj]
 *       G1 = (softmax_rows(B1) - I)/n, G2 = (softmax_cols(B2) - I)/n, u_j = sum_k G1_kj B1_kj, w_i = sum_k G2_ik B2_ik
 *       dloss/dA = Pc o (G1 o (1 + A) - u_j) + Pr o (G2 o (1 + A) - w_i);  dV = s G T, dT = s G^T V, d ls = sum(G o A)
 * Every gradient follows the same way: d loss / d S* from the softmaxes, then two GEMMs per logit matrix and
 * d log_scale = sum over the matrices of sum(G o S).
 * A kind that does not read an operand takes NULL for it and for its gradient (they are ignored): NCE and DSL read neither
 * img nor cap; VS_VC and VSC do not read img: xp_contrastive_loss_operands says which of the two a kind reads (1 / 0; an unknown
 * kind is refused).  Only VIDIMG and VIDIMG_DIVIDE accept m != n.  n, m (n + m for VIDIMG) <= 16384. */
enum XpLossKind { XP_LOSS_NCE, XP_LOSS_VSC_FC, XP_LOSS_DSL, XP_LOSS_VS_VC, XP_LOSS_VS_VC_FC,
                  XP_LOSS_VSC, XP_LOSS_VIDIMG, XP_LOSS_VIDIMG_DIVIDE };
int xp_contrastive_loss_operands(int32_t kind, int32_t* reads_img, int32_t* reads_cap);
size_t xp_contrastive_loss_workspace_bytes(int32_t kind, int64_t n, int64_t m, int64_t d);
/* align[xp_contrastive_loss]: all need 16 */
int xp_contrastive_loss(int32_t kind, const float* vis, const float* txt, const float* img, const float* cap,
                        const float* log_scale, float* loss, float* d_vis, float* d_txt, float* d_img, float* d_cap,
                        float* d_log_scale, int64_t n, int64_t m, int64_t d,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The four two-argument, fixed-temperature losses of optimization/loss.py (the drivers' `else: loss_func(vis_feat, text_feat)`
 * branch) behind one entry: loss and both feature gradients in one call, fp32, fixed reduction order (bit-reproducible), every
 * launch on `stream`, no allocation, no synchronisation, no host-to-device copy (the parameters travel as kernel arguments).
 * vis [n,d], txt [n*bag,d] (bag = 1 except for XP_PAIR_MILNCE), n*bag <= 16384.  rows(S) / cols(S) as for the family above.
 *   XP_PAIR_NCE      S = V T^T / temp ; loss = rows(S) + cols(S)                                   NCEContrastiveLoss    :67-83
 *   XP_PAIR_TRIPLET  S = V T^T, or with order_measure S_ij = -|max(0, t_j - v_i)|_2 (order_sim :13-19)  TripletContrastiveLoss :22-64
 *                    cs_ij = max(0, margin + S_ij - S_ii), ci_ij = max(0, margin + S_ij - S_jj), both diagonals cleared
 *                    loss = sum cs + sum ci (sums, not means); with max_violation  sum_i max_j cs_ij + sum_j max_i ci_ij.
 *                    A hinge is active where its cost is > 0.  The gradient of a maximum goes to ONE element, on an exact tie
 *                    to the lowest index; a line without a positive cost has no gradient.  A NaN cost counts as active and as
 *                    the largest of its line, and max(0, x) keeps a NaN, as torch's clamp(min=0) and max() do: a non-finite
 *                    feature makes the loss non-finite instead of vanishing in a comparison that is false for NaN.
 *                    Order measure: dS_ij/dv_i = max(0, t_j - v_i) / (-S_ij) = -dS_ij/dt_j, a kernel of its own (no GEMM).  A
 *                    pair at distance exactly 0 contributes ZERO gradient -- the one deliberate deviation: torch gives NaN there.
 *   XP_PAIR_HARDNEG  S = T V^T (no temperature).  Each row of S and each row of S^T keeps its k = hard_negative_num largest
 *                    entries after the diagonal entry was lowered by 10000 (in fp32, as the reference subtracts it):
 *                    loss = mean_i[lse(S_ii U top-k of row i) - S_ii] over both directions.                 HardNegLoss :86-105
 *                    1 <= k <= n; with k = n the lowered diagonal entry S_ii - 10000 is selected too (last), as in the
 *                    reference.  On an exact tie at the k-th value the lowest indices are taken (-0 counts as +0).
 *   XP_PAIR_MILNCE   x = (V T^T / temp) viewed as [n, n, bag] ; nom_i = lse_b x[i,i,b] ;              MILNCEContrastiveLoss :109-124
 *                    den_i = lse({x[i,j,b] : j != i} U {x[j,i,b] : all j}) ; loss = mean_i(den_i - nom_i)
 * Gradients: G = dloss/dS (of V T^T, before the temperature), then dV = c G T and dT = c G^T V with c = 1/temp (NCE, MILNCE) or 1
 * through the fp32 GEMM kernels of the family; the order measure goes through its own backward kernel instead.
 * Every element of loss, d_vis [n,d] and d_txt [n*bag,d] is written on every call (zeros where there is no gradient, e.g. the
 * triplet loss at n = 1).  Refused before any launch: an unknown kind, a null pointer, temp <= 0 (NCE, MILNCE),
 * hard_negative_num outside [1, n] (HARDNEG), bag < 1 or bag != 1 for a kind other than MILNCE, n*bag > 16384, a workspace
 * below xp_pair_loss_workspace_bytes (which is exact; 0 for arguments that would be refused).  Fields a kind does not read are
 * ignored.  No time was measured for these losses. */
enum XpPairLossKind { XP_PAIR_NCE, XP_PAIR_TRIPLET, XP_PAIR_HARDNEG, XP_PAIR_MILNCE };
typedef struct {
  float temp, margin;
  int32_t max_violation, order_measure, hard_negative_num, bag;
} XpPairLossParams;
size_t xp_pair_loss_workspace_bytes(int32_t kind, const XpPairLossParams* params, int64_t n, int64_t d);
/* align[xp_pair_loss]: all need 16 */
int xp_pair_loss(int32_t kind, const XpPairLossParams* params, const float* vis, const float* txt, float* loss,
                 float* d_vis, float* d_txt, int64_t n, int64_t d, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------- Retrieval evaluation
 * validate() of tasks/run_video_retrieval.py:123-203 on gathered unit-norm features (fp32):
 *   sim = text . vis^T                     cal_cossim, utils/metrics.py:3-5
 *   sim *= softmax(theta * sim, axis 0)    DSL re-rank, run_video_retrieval.py:170-171 / np_softmax metrics.py:7-39
 *                                          (multiply == 0: sim = softmax(theta * sim, axis 0) only)
 *   rank of each query's labelled entry    compute_metrics / compute_metrics_multi, metrics.py:41-69
 * xp_retrieval_ranks: query i = row i (transpose = 0) or column i (transpose != 0, the v2t direction, which the
 * reference evaluates on sim.T); label = labels[i] or i; greater[i] / equal[i] = number of candidates with a score
 * above / equal to the labelled one (the label sits at sorted positions greater .. greater+equal-1). */
/* align[xp_sim_matrix]: any: a b sim */
int xp_sim_matrix(const float* a, const float* b, float* sim, int64_t na, int64_t nb, int64_t d, void* stream);
/* align[xp_dsl_rerank]: all need 16 */
int xp_dsl_rerank(float* sim, int64_t n, int64_t m, float theta, int32_t multiply, void* stream);
/* align[xp_retrieval_ranks]: all need 16 */
int xp_retrieval_ranks(const float* sim, const int64_t* labels, int64_t n, int64_t m, int32_t transpose,
                       int32_t* greater, int32_t* equal, void* stream);

/* ----------------------------------------------------------------------- Retrieval at gallery scale (csrc/retrieval_stream.hip)
 * The same evaluation, and top-k search, straight from the features: q [nq, d] (queries: text), g [ng, d] (gallery: videos), both
 * row-major fp32, any d >= 1.  The score s_ij = sum_k q[i,k] g[j,k] is an fp32 fmaf chain in a k order that depends on d alone
 * (f32-input MFMA), so its bits depend on row i of q, row j of g and d only -- not on where the rows lie, on nq, ng, tiles or
 * splits: duplicate gallery rows tie exactly, and a label's own entry always counts as equal.  No score is ever written to global
 * memory; the workspaces have no nq * ng term.  Outputs are identical from run to run (no float atomics).
 *
 * xp_retrieval_ranks_streamed: x_ij = s_ij (dsl == 0) or s_ij * exp(theta s_ij - mx_j) / sum_j with mx_j = max_i theta s_ij and
 *   sum_j = sum_i exp(theta s_ij - mx_j) (dsl != 0: the arithmetic of xp_dsl_rerank, streamed over query tiles in a fixed order).
 *   Row direction (t2v): greater_q[i] / equal_q[i] = #{j : x_ij > x_il} / #{j : x_ij == x_il}, l = labels_q[i] (NULL: l = i, needs
 *   nq <= ng).  Column direction (v2t): greater_g[j] / equal_g[j] = the same over i against x_lj, l = labels_g[j] (NULL: l = j,
 *   needs ng <= nq).  Either pair of outputs may be NULL (not both); both directions come from one pass.  Counts are exact int32.
 *   Labels in memory the host can read (ordinary, pinned or managed) are range-checked before anything is launched, and ordinary
 *   host memory is copied to the device by the call; the range of labels in DEVICE memory is the caller's duty -- an out-of-range
 *   one reads nothing and gives greater = equal = 0.
 * xp_retrieval_topk: vals [nq, k] / idx [nq, k] = each query's k best (score, index_base + j), score descending, ties to the lowest
 *   index; 1 <= k <= min(XP_RETRIEVAL_MAX_K, ng).  accumulate != 0: the incoming vals / idx (a previous call's result) are
 *   candidates under the same order -- a gallery fed shard by shard (index_base = the shard's first row) gives exactly the
 *   one-shot result, values bit for bit.
 * Both return XP_ERR_ARG before any launch for null or empty operands, k out of range, host-readable labels out of range or a
 * workspace below *_workspace_bytes (which return 0 and set xp_last_error for shapes they refuse).
 * xp_retrieval_stream_plan: the tiling the calls use, for tests that place rows on its boundaries: scores are computed in tiles of
 *   XP_RETRIEVAL_TILE x XP_RETRIEVAL_TILE; the DSL statistics split the query tiles into runs of *stat_tiles_per_split, the top-k
 *   search splits the gallery tiles into runs of *topk_tiles_per_split.
 *
 * DSL-weighted search: top-k on the re-ranked score x = s * exp(theta s - mx) / sum, the statistics as a call of their own.
 * xp_retrieval_dsl_stats: for every row j of `of` [n_of, d], over the rows i of `over` [n_over, d]:  mx[j] = max_i theta (over_i .
 *   of_j),  sum[j] = sum_i exp(theta (over_i . of_j) - mx[j]).  The split plan is that of xp_retrieval_ranks_streamed(nq = n_over,
 *   ng = n_of, dsl = 1), and with accumulate == 0 the outputs are bit for bit the statistics that call forms internally for
 *   q = over, g = of.  accumulate != 0: the incoming (mx, sum) -- an earlier call's result for other rows of `over` -- lead the fold
 *   of this call's splits under (m, s) + (m', s') = (max, s e^(m - max) + s' e^(m' - max)): an `over` set that arrives in shards
 *   folds in shard order.  mx is exact either way (a maximum of the same products); the bits of sum depend on (n_over, n_of) through
 *   the plan and on the shard boundaries of an accumulated fold (each changes the order of the sum, not its terms).
 * xp_retrieval_topk_dsl: xp_retrieval_topk on x_ij = s_ij * exp(theta s_ij - mx_.) / sum_. -- the one expression the rank counts use
 *   -- with the statistics of the candidate's gallery row (stats_of == XP_DSL_OF_GALLERY: mx, sum [ng]; the t2v direction of
 *   validate(), statistics from xp_retrieval_dsl_stats(over = q, of = g)) or of the query row (XP_DSL_OF_QUERIES: mx, sum [nq]; the
 *   v2t direction, queries = videos, statistics from xp_retrieval_dsl_stats(over = g, of = q) over the WHOLE gallery).  Workspace:
 *   xp_retrieval_topk_workspace_bytes.  The result is EXACT GIVEN THE STATISTICS: the bits of x_ij depend on row i, row j, d, theta
 *   and the two statistics alone, the order is total (x descending, index ascending) -- a gallery fed shard by shard gives the
 *   one-shot result bit for bit when each shard is fed its slice of a per-gallery (mx, sum), or every shard the same per-query
 *   (mx, sum).  How close x is to the real-valued re-rank is the statistics' matter (sum: see above).
 * Both return XP_ERR_ARG before any launch for whatever xp_retrieval_topk refuses, null statistics, a theta that is not finite,
 * a stats_of that is neither constant or a workspace below its *_workspace_bytes. */
#define XP_RETRIEVAL_TILE 128
#define XP_RETRIEVAL_MAX_K 128
#define XP_DSL_OF_GALLERY 1
#define XP_DSL_OF_QUERIES 2
int xp_retrieval_stream_plan(int64_t nq, int64_t ng, int32_t k, int32_t* stat_tiles_per_split, int32_t* topk_tiles_per_split);
size_t xp_retrieval_ranks_streamed_workspace_bytes(int64_t nq, int64_t ng, int64_t d, int32_t dsl);
/* align[xp_retrieval_ranks_streamed]: any: q g; all need 16 */
int xp_retrieval_ranks_streamed(const float* q, const float* g, const int64_t* labels_q, const int64_t* labels_g, int64_t nq,
                                int64_t ng, int64_t d, int32_t dsl, float theta, int32_t* greater_q, int32_t* equal_q,
                                int32_t* greater_g, int32_t* equal_g, void* workspace, size_t workspace_bytes, void* stream);
size_t xp_retrieval_topk_workspace_bytes(int64_t nq, int64_t ng, int64_t d, int32_t k);
/* align[xp_retrieval_topk]: any: q g; all need 16 */
int xp_retrieval_topk(const float* q, const float* g, int64_t nq, int64_t ng, int64_t d, int32_t k, int64_t index_base,
                      int32_t accumulate, float* vals, int64_t* idx, void* workspace, size_t workspace_bytes, void* stream);
size_t xp_retrieval_dsl_stats_workspace_bytes(int64_t n_over, int64_t n_of, int64_t d);
/* align[xp_retrieval_dsl_stats]: any: over of; all need 16 */
int xp_retrieval_dsl_stats(const float* over, const float* of, int64_t n_over, int64_t n_of, int64_t d, float theta,
                           int32_t accumulate, float* mx, float* sum, void* workspace, size_t workspace_bytes, void* stream);
/* align[xp_retrieval_topk_dsl]: any: q g mx sum; all need 16 */
int xp_retrieval_topk_dsl(const float* q, const float* g, int64_t nq, int64_t ng, int64_t d, int32_t k, int64_t index_base,
                          int32_t accumulate, float theta, int32_t stats_of, const float* mx, const float* sum, float* vals,
                          int64_t* idx, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------ Encoder layer
 * One CLIPEncoderLayer.forward / backward per call (modeling/CLIP_ViP.py:444-460: x + Attn(LN1(x)), then x + MLP(LN2(x));
 * attention = CLIPAttention.forward2 :332-381 (XP_ATTN_PROXY) or .forward :266-330 (XP_ATTN_CAUSAL); MLP = CLIPMLP :392-396).
 * Host-side sequencing of the entry points above -- launch for launch the same arithmetic as calling them one by one -- so
 * that a training step costs ~50 native calls instead of ~800 foreign-function calls.  Activations are [rows = B*S, D]
 * row-major in `dtype`; weights are the `dtype` copies in the reference's [out, in] layout with q/k/v concatenated row-wise
 * (Wqkv [3D, D], bqkv [3D]); biases, LayerNorm parameters, statistics and all parameter gradients are float. */
typedef struct XpLayerDims {
  int64_t rows, D, Dff, B, S, heads;    /* rows == B*S, D == heads*64                                               */
  int64_t M, N, L;                      /* XP_ATTN_PROXY: S == M + N*L; XP_ATTN_CAUSAL: pass 0, 1, S                 */
  int32_t attn_mode, dtype;
  float q_scale, ln_eps;                /* head_dim^-0.5 (:341), 1e-5                                                */
  int32_t act;                          /* the MLP's activation (config.hidden_act, :388): XP_ACT_QUICK_GELU (0, what a zero-
                                         * initialised struct means) or XP_ACT_GELU (erf GELU: the fc1 / dpre GEMMs take
                                         * XP_EPI_BIAS_GELU_ERF / XP_EPI_GELU_ERF_BWD); any other value is an error         */
} XpLayerDims;
enum { XP_ACT_QUICK_GELU = 0, XP_ACT_GELU = 1 };

typedef struct XpLayerFwd {
  XpLayerDims dims;
  const void* x; const void* Wqkv; const void* Wo; const void* W1; const void* W2;
  const float* ln1_w; const float* ln1_b; const float* bqkv; const float* bo;
  const float* ln2_w; const float* ln2_b; const float* b1; const float* b2;
  const int64_t* pad_mask;              /* [B,S] 1/0 or NULL (text tower)                                            */
  /* outputs -- everything the backward needs stays in caller-owned buffers; pre == NULL: forward-only pass, the MLP
   * pre-activation (needed by the backward alone) is not written */
  void* h1; void* qkv; void* attn_o; void* x2; void* h2; void* pre; void* act; void* x3;
  float* mean1; float* rstd1; float* mean2; float* rstd2; float* stats;   /* stats [B,heads,S,2]                    */
  void* workspace; size_t workspace_bytes;                                /* >= xp_encoder_layer_fwd_workspace_bytes */
  /* optional (bf16): fp32 side rows of the residual stream -- rows r with r % side_S < side_M, stored at side row
   * (r / side_S) * side_M + r % side_S of a [.., D] fp32 buffer: the M proxy tokens of every video sample (side_S = S, side_M = M),
   * or the whole stream of the small text tower (side_S = side_M = 1).  side_in = those rows of x in fp32 (read by LayerNorm 1 and as
   * out_proj's residual operand), side_out = those rows of x3 in fp32, side_x2 = those rows of the intermediate x2 (kept for the
   * backward's second LayerNorm; NULL: they live in the workspace, forward-only pass).  side_in NULL: plain bf16 stream.  See
   * XpGemmDesc::resid_side. */
  const float* side_in; float* side_out; int64_t side_S; int32_t side_M; int32_t reserved;
  float* side_x2;
} XpLayerFwd;
size_t xp_encoder_layer_fwd_workspace_bytes(const XpLayerDims* dims);
/* align[xp_encoder_layer_fwd]: all need 16 */
int xp_encoder_layer_fwd(const XpLayerFwd* args, void* stream);

/* The rows of a layer's dx3 that can be non-zero, as tile lists (xp_encoder_layer_bwd_listed).  m_tiles: every 256-row tile that holds a listed k-tile of ANY of the three lists (padding tiles included: dW1 reads dpre, which is
 * written in those tiles only).  Weight gradient w (0: dW2, 1: dW1, 2: dWo): split[w] must be the split the call will use -- split_k of
 * entries XP_LAYER_GEMM_DW2 / _DW1 / _DWO of xp_debug_layer_bwd_gemms, whose plans (xp_debug_gemm_plan) give the slabs the lists are
 * cut by; k_tiles[w] / k_tile_begin[w] (device) and k_tile_begin_host[w] as in XpGemmDesc. */
typedef struct XpDx3Support {
  const int32_t* m_tiles; int32_t n_m_tiles; int32_t reserved;
  const int32_t* k_tiles[3]; const int32_t* k_tile_begin[3]; const int32_t* k_tile_begin_host[3];
  int32_t split[3]; int32_t reserved1;
} XpDx3Support;
typedef struct XpLayerBwd {
  XpLayerDims dims;
  /* saved by the forward */
  const void* x; const void* h1; const void* qkv; const void* attn_o; const void* x2; const void* h2; const void* pre;
  const void* act; const void* Wqkv; const void* Wo; const void* W1; const void* W2;
  const float* ln1_w; const float* ln2_w; const float* mean1; const float* rstd1; const float* mean2; const float* rstd2;
  const float* stats; const int64_t* pad_mask;
  const void* dx3;                      /* gradient of the layer output                                               */
  void* dx;                             /* gradient of the layer input                                                */
  /* parameter gradients (float); a NULL pointer skips that gradient's kernels (frozen parameters, VidCLIP.py:96-103) */
  float* dln1_w; float* dln1_b; float* dwqkv; float* dbqkv; float* dwo; float* dbo;
  float* dln2_w; float* dln2_b; float* dw1; float* db1; float* dw2; float* db2;
  void* workspace; size_t workspace_bytes;                                /* >= xp_encoder_layer_bwd_workspace_bytes */
  /* optional: the forward's fp32 side rows of x (side_in) and x2 (side_x2), read by the two LayerNorm backward passes */
  const float* side_in; const float* side_x2; int64_t side_S; int32_t side_M; int32_t reserved;
} XpLayerBwd;
size_t xp_encoder_layer_bwd_workspace_bytes(const XpLayerDims* dims);
/* align[xp_encoder_layer_bwd]: all need 16 */
int xp_encoder_layer_bwd(const XpLayerBwd* args, void* stream);
/* xp_encoder_layer_bwd for a dx3 that is zero outside a few rows, given as tile lists.  The caller vouches that args->dx3 is +-0
 * outside the 64-row k-tiles listed; the MLP / out_proj part of the backward then runs its three dX GEMMs (dpre, dh2, dattn) over
 * m_tiles and its three weight gradients (dW2, dW1, dWo) over k-tile lists (XpGemmDesc::m_tiles / k_tiles): bit-identical to
 * xp_encoder_layer_bwd for finite activations.  (With a non-finite activation in a row that carries no gradient the dense
 * product 0 * Inf poisons a weight gradient; the listed one never forms it.)  LayerNorm 2', attention', dh1, dWqkv, LayerNorm 1'
 * and the reductions stay dense.  Same workspace.  Needs the 256-wide-family plans of all six GEMMs (bf16, large shapes): an
 * error otherwise, nothing is launched dense in its place. */
/* align[xp_encoder_layer_bwd_listed]: all need 16 */
int xp_encoder_layer_bwd_listed(const XpLayerBwd* args, const XpDx3Support* dx3_support, void* stream);
/* The LAST video-tower layer when only the pooled feature (token 0 of every sample, a proxy row) leaves the tower: the same
 * function of x as row b*S of xp_encoder_layer_fwd's x3, computed without the dead rows.  LayerNorm 1 and the K/V projection
 * (Wqkv rows D..3D) see every row, because token 0 attends all S keys; the Q projection, the single-query attention
 * (xp_attn_pooled_fwd), out_proj + residual, LayerNorm 2 and the MLP run on the B pooled rows.  XP_ATTN_PROXY only (M >= 1), no
 * padding mask.  Same conventions as xp_encoder_layer_fwd / _bwd: caller-owned saved activations, pre == NULL for a forward-only
 * pass, NULL gradient pointer = frozen parameter, the weight-gradient GEMMs on the library's stream joined before return.
 * The backward's dx is dense [rows, D]: LayerNorm 1' over all rows, fed by dkv . Wkv on all rows plus dq . Wq and the residual
 * on the pooled rows; every parameter of the layer receives its gradient.
 * Side rows (bf16): side_in is the layer's usual [B*M, D] fp32 buffer (read by LayerNorm 1; its row b*M is the pooled row's
 * residual operand); side_x2 / side_out are [B, D] fp32, one row per sample (side_x2 NULL: kept in the workspace). */
typedef struct XpLayerPooledFwd {
  XpLayerDims dims;
  const void* x; const void* Wqkv; const void* Wo; const void* W1; const void* W2;
  const float* ln1_w; const float* ln1_b; const float* bqkv; const float* bo;
  const float* ln2_w; const float* ln2_b; const float* b1; const float* b2;
  /* every row: h1 [rows, D], kv [rows, 2D], mean1 / rstd1 [rows] */
  void* h1; void* kv; float* mean1; float* rstd1;
  /* the pooled rows: h1p, q, attn_o, x2, h2, x3 [B, D]; pre, act [B, Dff]; mean1p, rstd1p, mean2, rstd2 [B]; stats [B, heads, 2] */
  void* h1p; void* q; void* attn_o; void* x2; void* h2; void* pre; void* act; void* x3;
  float* mean1p; float* rstd1p; float* mean2; float* rstd2; float* stats;
  void* workspace; size_t workspace_bytes;                        /* >= xp_encoder_layer_pooled_fwd_workspace_bytes */
  const float* side_in; float* side_out; float* side_x2;
} XpLayerPooledFwd;
size_t xp_encoder_layer_pooled_fwd_workspace_bytes(const XpLayerDims* dims);
/* align[xp_encoder_layer_pooled_fwd]: all need 16 */
int xp_encoder_layer_pooled_fwd(const XpLayerPooledFwd* args, void* stream);

typedef struct XpLayerPooledBwd {
  XpLayerDims dims;
  /* saved by the forward */
  const void* x; const void* h1; const void* kv; const void* h1p; const void* q; const void* attn_o; const void* x2;
  const void* h2; const void* pre; const void* act; const void* Wqkv; const void* Wo; const void* W1; const void* W2;
  const float* ln1_w; const float* ln2_w; const float* mean1; const float* rstd1; const float* mean1p; const float* rstd1p;
  const float* mean2; const float* rstd2; const float* stats;
  const void* dx3;                      /* gradient of the pooled output rows [B, D]                                   */
  void* dx;                             /* gradient of the layer input [rows, D]                                      */
  float* dln1_w; float* dln1_b; float* dwqkv; float* dbqkv; float* dwo; float* dbo;
  float* dln2_w; float* dln2_b; float* dw1; float* db1; float* dw2; float* db2;
  void* workspace; size_t workspace_bytes;                        /* >= xp_encoder_layer_pooled_bwd_workspace_bytes */
  const float* side_in; const float* side_x2;
} XpLayerPooledBwd;
size_t xp_encoder_layer_pooled_bwd_workspace_bytes(const XpLayerDims* dims);
/* align[xp_encoder_layer_pooled_bwd]: all need 16 */
int xp_encoder_layer_pooled_bwd(const XpLayerPooledBwd* args, void* stream);
/* The library's second stream of the current device (the one xp_encoder_layer_bwd and xp_encoder_layer_pooled_bwd issue the
 * weight-gradient GEMMs on; created at the DEFAULT priority on first use -- a high-priority queue starves the critical chain as soon
 * as a collective library's streams run beside it), or NULL when XPRETRAIN_WGRAD_STREAM=0.  It is idle outside those
 * two calls: the host side runs the second half-batch chain of the video tower's forward on it instead of creating one more stream
 * (a process gets few hardware queues). */
void* xp_side_stream(void);

/* -------------------------------------------------------------------------------------- Diagnostics
 * Hardware-layout probes used by tests/test_probe_gpu.py to pin the MFMA / LDS-transpose lane maps
 * this library relies on (out buffers are small device arrays; see csrc/probe.hip). */
/* cycle-stamp trace of the 128x128 GEMM main loop (tools/gemm_trace.py); pass NULL to disable.  buffer: >= 1 KiB */
/* align[xp_debug_set_gemm_trace]: all need 16 */
int xp_debug_set_gemm_trace(void* device_buffer);
/* In-step timing of ONE GEMM shape: while armed, every xp_gemm call with these (M, N, K, epilogue, operand layouts, split_k) is
 * bracketed by a pair of HIP events on the stream it is launched on (up to max_launches calls); ..._read disarms, waits for the events and
 * returns the elapsed times in ms (return value: number of bracketed launches, -1 on error).  bench.py times the dominant kernel of
 * the step with it INSIDE training steps (isolated launches run at a different power / cache operating point). */
int xp_debug_gemm_timer_arm(int64_t M, int64_t N, int64_t K, int32_t epilogue, int32_t a_kstrided, int32_t b_kstrided, int32_t split_k,
                            int32_t max_launches);
int32_t xp_debug_gemm_timer_read(float* ms, int32_t cap);
/* cycle stamps of one attention-forward workgroup (start, loads issued, loads landed, loop end); NULL disables */
/* align[xp_debug_set_attn_trace]: all need 16 */
int xp_debug_set_attn_trace(void* device_buffer);
/* resident workgroups per CU of the default bf16 GEMM kernel at `lds_bytes` of dynamic LDS (occupancy API) */
int xp_debug_gemm_occupancy(int lds_bytes);
/* The plan xp_gemm launches for `desc` (desc->split_k honoured), from the same planner: host only, launches nothing, reads the
 * environment switches (XPRETRAIN_GEMM256, XPRETRAIN_DEBUG) and the CU budget as xp_gemm would.  The data pointers are read only as
 * present / absent (resid, aux, colsum_partials, a_frames).  The descriptor's arguments are not validated: a descriptor xp_gemm
 * rejects still gets the plan it would have had. */
enum { XP_GEMM_FAMILY_256 = 0,       /* 256x256 ping-pong tiles (gemm256.hip) */
       XP_GEMM_FAMILY_DIRECT = 1,    /* 128x128, operands staged global -> LDS directly */
       XP_GEMM_FAMILY_STAGED = 2,    /* 128x128, operands staged through registers */
       XP_GEMM_FAMILY_FRAMES = 3 };  /* 128x128, A gathered from a frame tensor (XpGemmDesc::a_frames) */
enum { XP_GEMM_EPI_FAST = 0,         /* straight-line buffer-addressed epilogue, 8 columns per lane */
       XP_GEMM_EPI_ROW8 = 1,         /* generic epilogue, 8 columns per lane */
       XP_GEMM_EPI_ROW4 = 2 };       /* generic epilogue, 4 columns per lane */
typedef struct XpGemmPlanInfo {
  int32_t family, tile_rows;            /* XP_GEMM_FAMILY_*; output tile height (as xp_gemm_tile_rows)      */
  int32_t split, flat_split;            /* k slabs; > 0: split-K on the 1-D chunk-major grid (256 family)   */
  int64_t k_per_split;                  /* k of every slab but the last                                     */
  int32_t tiles_m, tiles_n, group_n;    /* output tiles; tile columns per L2 group                           */
  int32_t epi_impl;                     /* XP_GEMM_EPI_*                                                     */
  int32_t grid[3];                      /* launch grid (x, y, z)                                            */
  int32_t reserved;
  int64_t colsum_rows;                  /* partial rows of the fused column sums (as xp_gemm_colsum_rows)    */
} XpGemmPlanInfo;
int xp_debug_gemm_plan(const XpGemmDesc* desc, XpGemmPlanInfo* out);
/* The plan xp_attn_fwd (backward == 0) / xp_attn_bwd2 (backward != 0) launches for these arguments, from the same planner: host
 * only, launches nothing, reads XPRETRAIN_DEBUG as the call would.  cus > 0: planned for a device of that many CUs that grants every
 * dynamic-LDS opt-in (no GPU needed); cus <= 0: for the current device, as a launch plans it (XP_ERR_LAUNCH if there is none or it
 * refuses the planned kernel's opt-in).  The arguments are not validated. */
enum { XP_ATTN_KERNEL_FWD = 0,        /* attn_fwd_kernel: one 7-wave workgroup per (problem, 112 query rows) */
       XP_ATTN_KERNEL_FWD3 = 1,       /* attn_fwd3_kernel: persistent, problems of one LDS group (M + L <= 208) */
       XP_ATTN_KERNEL_FWD4 = 2,       /* attn_fwd4_kernel: persistent, wider problems, one workgroup per CU */
       XP_ATTN_KERNEL_BWD_PAIR = 3,   /* attn_bwd_dq_kernel, then attn_bwd_dkv_kernel */
       XP_ATTN_KERNEL_BWD5 = 4,       /* attn_bwd5_kernel: dQ, dK, dV in one persistent launch */
       XP_ATTN_KERNEL_F32 = 5 };      /* the fp32 compute mode's kernels (attention_f32.hip, which sizes their grids) */
/* kernels only an opt-in switch plans (same number space as above; no default plan names them) */
enum { XP_ATTN_OPTIN_BWD6 = 6 };      /* attn_bwd6_kernel: attn_bwd5's one launch for wider windows; xp_set_attn_bwd_wide */
typedef struct XpAttnPlanInfo {
  int32_t kernel;                       /* XP_ATTN_KERNEL_* / XP_ATTN_OPTIN_*                                     */
  int32_t grid, lds_bytes;              /* main launch (each kernel of the pair): workgroups, dynamic LDS; f32: 0  */
  int32_t reduce_grid;                  /* proxy merge (forward) / proxy reduce (backward) workgroups; 0: none     */
  int32_t uses_counter;                 /* a fused backward's problem counter is reset and used                   */
  int32_t reserved;
  int64_t part[2], delta[2], dq[2], dkv[2], counter[2];  /* workspace regions (byte offset, bytes); 0 bytes: not used   */
  int64_t workspace_bytes;              /* this direction's regions (xp_attn_workspace_bytes: the larger direction) */
  int64_t colsum_rows;                  /* as xp_attn_bwd_colsum_rows                                             */
} XpAttnPlanInfo;
int xp_debug_attn_plan(int32_t mode, int64_t B, int64_t H, int64_t S, int64_t M, int64_t N, int64_t L, int32_t dtype,
                       int32_t has_pad_mask, int32_t backward, int32_t cus, XpAttnPlanInfo* out);
/* The plan xp_attn_pooled_fwd (backward == 0) / xp_attn_pooled_bwd (backward != 0) launches: host only, launches nothing.
 * cus > 0: planned for a device of that many CUs (no GPU needed); cus <= 0: for the current device (XP_ERR_LAUNCH if none). */
typedef struct XpAttnPooledPlanInfo {
  int32_t chunks, chunk_keys;           /* chunk c covers keys [c*chunk_keys, min(S, (c+1)*chunk_keys))             */
  int32_t grid, combine_grid;           /* main launch: B*H*chunks workgroups; combine launch: B*H                  */
  int64_t part_ml[2], part_acc[2];      /* forward workspace regions (byte offset, bytes): (m, l) and O partials    */
  int64_t part_dq[2];                   /* backward workspace region: dq partials; 0 bytes: not used                */
  int64_t workspace_bytes;              /* this direction's regions (<= xp_attn_pooled_workspace_bytes)             */
  int64_t colsum_rows;                  /* as xp_attn_pooled_colsum_rows                                            */
} XpAttnPooledPlanInfo;
int xp_debug_attn_pooled_plan(int64_t B, int64_t H, int64_t S, int32_t dtype, int32_t backward, int32_t cus,
                              XpAttnPooledPlanInfo* out);
/* The GEMMs of xp_encoder_layer_bwd (pooled == 0) / xp_encoder_layer_pooled_bwd (pooled != 0) for `dims`, in issue order: the table
 * the call sizes its workspace by and launches from (csrc/layer.hip), so what a caller plans from it is what runs.  Host only,
 * launches nothing, needs no device; reads the CU budget and the planning switches as the call would.  Every out[i] is the launched
 * descriptor without its operands: A, B, C, bias and the tile lists are NULL; resid and colsum_partials are non-NULL (never to be
 * dereferenced) exactly where the launch passes them with every gradient asked for; a weight gradient's split_k is the split the
 * call uses (>= 1; xp_gemm_auto_split_slack for dW2, dW1, dWo and the pooled dWq, xp_gemm_auto_split for dWqkv and dWkv).  Returns
 * the number of descriptors written (XP_LAYER_GEMM_DENSE_COUNT / _POOLED_COUNT); XP_ERR_ARG, nothing written, for dims the call
 * refuses or cap below that number. */
enum { XP_LAYER_GEMM_DPRE = 0,        /* dpre = (dx3 . W2) * act'(pre), with fc1's bias-gradient partial rows where fused */
       XP_LAYER_GEMM_DW2 = 1,         /* dW2 = dx3^T . act                                                                */
       XP_LAYER_GEMM_DH2 = 2,         /* dh2 = dpre . W1                                                                  */
       XP_LAYER_GEMM_DW1 = 3,         /* dW1 = dpre^T . h2                                                                */
       XP_LAYER_GEMM_DATTN = 4,       /* dattn = dx2 . Wo                                                                 */
       XP_LAYER_GEMM_DWO = 5,         /* dWo = dx2^T . attn_o                                                             */
       XP_LAYER_GEMM_DH1 = 6,         /* dense: dh1 = dqkv . Wqkv                                                         */
       XP_LAYER_GEMM_DWQKV = 7,       /* dense: dWqkv = dqkv^T . h1                                                       */
       XP_LAYER_GEMM_DENSE_COUNT = 8,
       XP_LAYER_GEMM_DH1_KV = 6,      /* pooled: dh1 = dkv . Wkv on every row                                             */
       XP_LAYER_GEMM_DH1_Q = 7,       /* pooled: dh1[b*S] = dqkv[b*S] . Wqkv on the pooled rows                           */
       XP_LAYER_GEMM_DWQ = 8,         /* pooled: dWq = dq^T . h1p                                                         */
       XP_LAYER_GEMM_DWKV = 9,        /* pooled: dWkv = dkv^T . h1                                                        */
       XP_LAYER_GEMM_POOLED_COUNT = 10,
       XP_LAYER_GEMM_MAX = 10 };
int32_t xp_debug_layer_bwd_gemms(const XpLayerDims* dims, int32_t pooled, XpGemmDesc* out, int32_t cap);
/* align[xp_probe_mfma_bf16]: all need 16 */
int xp_probe_mfma_bf16(const void* a, const void* b, float* c, void* stream);
/* align[xp_probe_mfma_f32]: all need 16 */
int xp_probe_mfma_f32(const float* a, const float* b, float* c, void* stream);
/* packed-fp32 self-check (csrc/probe.hip): err[(variant*64 + lane)*2 + half] += mismatches between one v_pk_*_f32 form and
 * the same arithmetic in unpacked VALU instructions; 15 variants */
/* align[xp_probe_pk_f32]: all need 16 */
int xp_probe_pk_f32(void* err /*15*64*2 u32, zeroed by the caller*/, int32_t iters, int32_t blocks, uint32_t seed, void* stream);
/* memory-bound copy of nbytes (multiple of 16) repeated iters times by `blocks` 256-thread workgroups: a one-GPU stand-in for a
 * collective's channel kernels beside the backward pass (hvd.DistributedOptimizer's all-reduce, run_pretrain.py:224-227) */
/* align[xp_probe_stream_copy]: all need 16 */
int xp_probe_stream_copy(void* dst, const void* src, int64_t nbytes, int32_t blocks, int32_t iters, void* stream);
/* the same copy in a kernel with the register / LDS footprint of RCCL's gfx950 collective kernel (one wave per SIMD, 19,744 B LDS) */
/* align[xp_probe_stream_copy_fat]: all need 16 */
int xp_probe_stream_copy_fat(void* dst, const void* src, int64_t nbytes, int32_t blocks, int32_t iters, void* stream);
/* align[xp_probe_tr16]: all need 16 */
int xp_probe_tr16(const void* in /*4096 u16*/, const int32_t* lane_byte_off /*64*/, void* out /*64*4 u16*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif
