/*
 * libclipmi — MI355X-native (gfx950 / CDNA4) kernels for the CLIP dual-encoder +
 * adapter contrastive fine-tuning step of Quillboltcode/VLM-CLIP.
 *
 * C ABI only: plain pointers, sizes and dtype codes; no torch types.  Every entry point
 * enqueues work on the caller's hipStream_t (passed as void*) and returns 0 on success
 * or a negative status; clipmi_last_error() returns a thread-local message.  The
 * library never allocates or frees caller memory; scratch comes from caller workspace.
 *
 * The reference has no native boundary: its hot path is PyTorch/HF
 * module calls.  Each entry point below names the reference op it replaces.
 *
 * Collectives: clipmi_allgather_embed / clipmi_reducescatter_grad /
 * clipmi_allreduce_grads below run the data-parallel exchanges over RCCL for FFI hosts with one process
 * per GPU (communicator from clipmi_comm_unique_id + clipmi_comm_init).  The PyTorch host issues the same
 * exchanges through torch.distributed (backend "nccl" = RCCL over xGMI) in clipmi/towers.py (ContrastiveFn)
 * and clipmi/trainer.py (GradBucketReducer), on the same HIP streams these entry points run on.
 * Workspaces are sized per call by the *_ws() queries (no context object).
 */
#ifndef CLIPMI_H
#define CLIPMI_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CLIPMI_OK 0
#define CLIPMI_ERR_INVALID -1   /* bad shape/arg -> Python ValueError */
#define CLIPMI_ERR_HIP -2       /* HIP runtime error -> RuntimeError */
#define CLIPMI_ERR_UNSUPPORTED -3

enum clipmi_dtype { CLIPMI_F32 = 0, CLIPMI_BF16 = 1, CLIPMI_FP8 = 2 /* MXFP8: OCP e4m3 + E8M0 per 32 k */ };

/* 2: clipmi_encoder_desc gained first_token (appended); clipmi_encoder_act_bytes
 * 3: evaluation entry points (clipmi_rank_pick, clipmi_rank_count, clipmi_classify_accumulate)
 * 4: clipmi_topk_merge
 * 5: clipmi_encoder_desc gained cls_last (appended); clipmi_attention_cls_fwd / _bwd, clipmi_layernorm_bwd4
 * 6: clipmi_resize_crop_u8 (ragged image batches)
 * 7: clipmi_contrastive_keyed_* (multi-positive contrastive head), clipmi_row_hash64
 * 8: clipmi_group_pick, clipmi_group_count, clipmi_topk_hits (group-aware retrieval evaluation)
 * 9: clipmi_color_u8 (colour augmentation of the input step)
 * 10: clipmi_gemm_plan
 * 11: clipmi_sigmoid_pairs, clipmi_sigmoid_reduce (pairwise sigmoid contrastive head)
 * 12: clipmi_affine_u8 (affine / rotation augmentation of the input step)
 * 13: clipmi_enhance_u8 (posterize, solarize, autocontrast, equalize, sharpness: the policy ops of the input step)
 * 14: clipmi_class_bce, clipmi_class_bias_grad (multi-label sigmoid / BCE head), clipmi_ap_count,
 *     clipmi_multilabel_accumulate (average precision counts and thresholded multi-label tallies) */
int clipmi_version(void);
const char* clipmi_last_error(void);
/* sha256 (hex) of the sources this library was compiled from (vlm-clip_amd/Makefile DIGEST_SRC) */
const char* clipmi_build_digest(void);

/* ---- GEMM:  C[m,n] = epi( alpha * sum_k A(m,k) B(n,k) )  --------------------------
 * Replaces nn.Linear forward/backward inside HF CLIPAttention/CLIPMLP
 * ([HF] modeling_clip.py:313-315,332,348-350), the adapters' down/up projections
 * (adapter/clip_adapter.py:19-21,146-148) and the CLIP projections (model_m.py:103,123).
 * A(m,k) = A[m*lda+k] if a_kmajor else A[k*lda+m]; same for B with n.
 * flags: bit0 bias[n] | bit1 quick_gelu | bit2 gelu_erf | bit3 += residual[m,n]
 *        bit4 *= quick_gelu'(aux[m,n]) | bit5 *= gelu_erf'(aux[m,n])
 *        bit6 C += result (beta = 1) | bit7 store pre-activation to aux[m,n]
 *        bit8 store act'(pre-activation) to aux[m,n] | bit9 *= aux[m,n]
 * dtypes: A/B bf16 (MFMA path) or f32 (exact-f32 parity path); C/residual/aux in c_dtype.
 * split_k > 1 (fp32 C, beta flag only) uses workspace of split_k*M*N floats (+ split_k*M with
 * bias_grad: per-split bias partials summed in split order, so results are run-to-run identical).
 */
typedef struct clipmi_gemm_desc {
  int M, N, K;
  const void* A; int64_t lda; int a_kmajor;
  const void* B; int64_t ldb; int b_kmajor;
  void* C; int64_t ldc;
  const void* bias;
  const void* residual; int64_t ldr;
  void* aux; int64_t ldaux;
  float alpha;
  int flags;
  int ab_dtype;   /* clipmi_dtype */
  int c_dtype;    /* clipmi_dtype */
  int bias_dtype; /* clipmi_dtype */
  int split_k;
  void* workspace; int64_t workspace_bytes;
  float* bias_grad;     /* wgrad only: bias_grad[m] += sum_k A(m,k) (fused Linear bias gradient, fp32) */
  int force_small_tile; /* kernel override for tests and bench tools; 0: the production rule.  1: the 128x128
                         * register-staged kernel; other codes name a schedule (4, 9, 28, 32, 1xx; 40 / 41 with MXFP8
                         * operands): the one decode table is gemm_force() in csrc/gemm_plan.cpp, the names in
                         * clipmi/_lib.py (FORCE_*).  clipmi_gemm_plan() reports what a descriptor selects. */
  /* ab_dtype == CLIPMI_FP8 (BASELINE config 5, forward GEMMs of the frozen towers): A, B are OCP e4m3
   * bytes, both k-major, K % 128 == 0; a_scale / b_scale are E8M0 bytes [rows][K/32] (OCP MX:
   * element value = fp8 * 2^(scale - 127)); v_mfma_scale_f32_32x32x64_f8f6f4, fp32 accumulation,
   * the bf16 epilogues.  c_dtype == CLIPMI_FP8 (flags bias and/or quick_gelu / gelu only, ldc == N,
   * N % 32 == 0, C 16-byte and c_scale 2-byte aligned): C is written as MXFP8 too, e4m3 bytes [M, N]
   * and E8M0 scales c_scale [M, N/32] (fc1 -> fc2 without a bf16 round trip). */
  const uint8_t* a_scale;
  const uint8_t* b_scale;
  uint8_t* c_scale;
} clipmi_gemm_desc;

#define CLIPMI_EPI_BIAS 1
#define CLIPMI_EPI_QGELU 2
#define CLIPMI_EPI_GELU 4
#define CLIPMI_EPI_RESID 8
#define CLIPMI_EPI_DQGELU 16
#define CLIPMI_EPI_DGELU 32
#define CLIPMI_EPI_BETA 64
#define CLIPMI_EPI_STORE_PRE 128
/* store the activation's derivative at the pre-activation to aux[m,n] (quick_gelu' with bit1,
 * gelu_erf' with bit2), computed from the fp32 pre-activation beside the activation itself, so
 * the backward is a plain product (bit9) instead of a load + derivative per element */
#define CLIPMI_EPI_STORE_DACT 256
/* C *= aux[m,n] (the stored derivative: d_pre = d_act * act'(pre)) */
#define CLIPMI_EPI_MUL_AUX 512

/* Not an epilogue: ab_dtype and c_dtype CLIPMI_F32, computed on the bf16 MFMA kernels as a split-operand
 * product (precision "bf16x3"): x = bf16(x) + bf16(x - bf16(x)) for both operands and
 * A.B^T ~ Ah.Bh^T + Ah.Bl^T + Al.Bh^T in one bf16 GEMM over 3K (fp32 accumulation), ~2^-16 relative
 * error per product instead of bf16's 2^-8.  Any epilogue flag except bias_grad; K % 8 == 0 when an operand
 * is k-major (the bf16 kernels' layout rules apply to the split images: row-major A needs M % 8 == 0); workspace
 * >= clipmi_gemm_split3_ws(...) bytes, 256-byte aligned (it also holds the split-K slabs). */
#define CLIPMI_GEMM_SPLIT3 1024
int64_t clipmi_gemm_split3_ws(int M, int N, int K, int a_kmajor, int b_kmajor, int split_k);

int clipmi_gemm(void* stream, const clipmi_gemm_desc* d);
/* The kernel selection of clipmi_gemm (x3out 0) or clipmi_gemm_x3out (x3out != 0) for d, without launching
 * anything (clipmi_version() >= 10): the same validation and the same plan the launch uses, so the same errors.
 * Operand pointers are read for null-ness and alignment only; no GPU is needed.  Strings are static. */
typedef struct clipmi_gemm_plan_info {
  const char* kernel; /* "none" (M or N == 0), "f32", "bf16_128", "pp8", "asm8", "w4p", "w4p_pf", "fp8_8w", "fp8_w4p";
                       * "experiment" in a CLIPMI_GEMM_EXPERIMENTS build's extra schedules */
  const char* label;  /* the live profiler's label of the launch (clipmi_prof_*; bench.py's families) */
  int tile, tiles_n, ntiles; /* tile edge; column tiles; tiles */
  int splits, k_per_split;   /* effective split-K count and each split's k range */
  int raster;                /* tile-rows per raster group (0: row-major) */
  int stagger;               /* first-round stagger of "pp8" (force 1xx), else 0 */
  int specialised;           /* the epilogue is a compile-time instance (0: the runtime-flag instance) */
  int bias_grad;             /* the fused bias-gradient instance */
  int reduce;                /* split-K second stage: 0 none, 1 the 16-byte form (deferrable), 2 the scalar form */
} clipmi_gemm_plan_info;
int clipmi_gemm_plan(const clipmi_gemm_desc* d, int x3out, clipmi_gemm_plan_info* out);
/* Strided batch of nb1 x nb2 fp32 products (exact f32; flags: beta only): product z = i1 * nb2 + i2 reads
 * A + i1 * sa1 + i2 * sa2, B + i1 * sb1 + i2 * sb2 and writes C + i1 * sc1 + i2 * sc2 (elements), the
 * rest as clipmi_gemm.  One launch for the per-(sample, head) score / context products of attention at
 * head widths the flash kernels do not take (peclip ContextAdapter / SharedAdapter, adapter/peclip.py:21-48). */
int clipmi_gemm_batched(void* stream, const clipmi_gemm_desc* d, int nb1, int nb2, int64_t sa1, int64_t sa2,
                        int64_t sb1, int64_t sb2, int64_t sc1, int64_t sc2);
/* Diagnostic (no reference counterpart): arm / disarm (nullptr) the in-kernel s_memtime stamps of
 * the 4-wave GEMM's timing variant (force_small_tile = 22); buf holds 512 * 4 * 128 u64 of device
 * memory (layout: csrc/gemm4.hip, reader: tools/w4_stamps.py). */
int clipmi_gemm_stamps(void* buf);
/* MXFP8 quantisation of a [R, K] bf16/f32 matrix (row stride ldx elements) into OCP e4m3 bytes
 * q [R, K] and E8M0 block scales [R, K/32]: per 32-element block the smallest power of two that
 * brings the block's max |x| to <= 448, round-to-nearest-even. */
int clipmi_quant_mxfp8(void* stream, int dtype, const void* x, int64_t ldx, int64_t R, int K, uint8_t* q,
                       uint8_t* scales);

/* ---- LayerNorm ([HF] modeling_clip.py:357,359,605,642,559; adapter/clip_adapter.py:15,142) -------
 * y = LN(x [+ pos[row % period] (+ cls at row % period == 0)]) * w + b; mean/rstd saved (fp32).
 * With pos != NULL the sum is written back to x: the vision embedding ([HF] :209-219) fused
 * into pre_layrnorm. Weights in the activation dtype. 1 <= D <= 4096: register-resident kernels for D / 64
 * in {1, 2, 3, 4, 6, 8, 12, 16} (every CLIP width), a one-wave-per-row kernel for any other width.  Leading
 * dimensions (>= D) and base pointers need no alignment beyond the element's: the register-resident kernels move
 * pieces of 4 (D % 256 == 0), 2 (D % 128 == 0) or 1 elements as one vector, and a call whose pointers or leading
 * dimensions are no multiple of that piece runs the one-wave-per-row kernel instead (forward and backward). */
int clipmi_layernorm_fwd(void* stream, int dtype, void* x, int64_t ldx, void* y, int64_t ldy, const void* w,
                         const void* b, float* mean, float* rstd, int R, int D, float eps, const void* pos,
                         const void* cls, int period);
/* The same with the input x (and pos / cls) in x_dtype and y, w, b in dtype: x_dtype == dtype, or an fp32 x
 * normalised into a bf16 y (the bf16 mode's fp32 residual stream -> the next GEMM's bf16 operand). */
int clipmi_layernorm_fwd2(void* stream, int x_dtype, int dtype, void* x, int64_t ldx, void* y, int64_t ldy,
                          const void* w, const void* b, float* mean, float* rstd, int R, int D, float eps,
                          const void* pos, const void* cls, int period);
/* The same LayerNorm (bf16 x, no embedding add) with its output written as MXFP8, quantised
 * from the fp32 result as clipmi_quant_mxfp8 does: q8 [R, D] e4m3, s8 [R, D/32] E8M0.  Feeds the
 * fp8 tower GEMMs (BASELINE config 5) without a bf16 round trip. D % 256 == 0, D <= 1024. */
int clipmi_layernorm_fwd_mxfp8(void* stream, int dtype, const void* x, int64_t ldx, uint8_t* q8, uint8_t* s8,
                               const void* w, const void* b, float* mean, float* rstd, int R, int D, float eps);
int64_t clipmi_layernorm_bwd_ws(int R, int D);
/* dx = [dres +] LN'(dy); dw/db (fp32, may be NULL) accumulate when beta_wb.  Widths as clipmi_layernorm_fwd. */
int clipmi_layernorm_bwd(void* stream, int dtype, const void* dy, int64_t lddy, const void* x, int64_t ldx,
                         const float* mean, const float* rstd, const void* w, void* dx, int64_t lddx, const void* dres,
                         int64_t ldres, float* dw, float* db, int beta_wb, void* ws, int64_t ws_bytes, int R, int D);
/* The same with x in x_dtype (fp32 residual stream) and dy, dx, dres, w in dtype (bf16 gradients). */
int clipmi_layernorm_bwd2(void* stream, int x_dtype, int dtype, const void* dy, int64_t lddy, const void* x,
                          int64_t ldx, const float* mean, const float* rstd, const void* w, void* dx, int64_t lddx,
                          const void* dres, int64_t ldres, float* dw, float* db, int beta_wb, void* ws,
                          int64_t ws_bytes, int R, int D);
/* the same with the affine weight's dtype given: w_dtype = dtype, or CLIPMI_F32 with fp32 x (the vision
   pre_layrnorm on the fp32 residual stream normalises with the fp32 master weights in its forward) */
int clipmi_layernorm_bwd3(void* stream, int x_dtype, int dtype, int w_dtype, const void* dy, int64_t lddy,
                          const void* x, int64_t ldx, const float* mean, const float* rstd, const void* w, void* dx,
                          int64_t lddx, const void* dres, int64_t ldres, float* dw, float* db, int beta_wb, void* ws,
                          int64_t ws_bytes, int R, int D);
/* the same with a compact residual gradient (clipmi_version() >= 5): res_period > 0 makes dres
   [ceil(R / res_period)][ldres], its row b added to row b * res_period alone and nothing to the other rows (the
   encoder's cls_last layer, whose residual gradient exists at the CLS rows only); res_period == 0 is
   clipmi_layernorm_bwd3.  One rounding of dx either way. */
int clipmi_layernorm_bwd4(void* stream, int x_dtype, int dtype, int w_dtype, const void* dy, int64_t lddy,
                          const void* x, int64_t ldx, const float* mean, const float* rstd, const void* w, void* dx,
                          int64_t lddx, const void* dres, int64_t ldres, int res_period, float* dw, float* db,
                          int beta_wb, void* ws, int64_t ws_bytes, int R, int D);
/* out[n] (+)= sum_r x[r][n]  (bias gradients of every Linear on the path).  Any N, ldx >= N and alignment: the
 * 4-column vector kernels run when N % 4 == 0, ldx % 4 == 0, x is aligned to 4 elements (8 bytes bf16, 16 bytes
 * fp32) and ws to 16 bytes; otherwise the call falls to the one-column-per-thread kernels, which need none of it.
 * Two fixed-order stages (per-chunk partial rows in ws, then their sum): bitwise reproducible. */
int64_t clipmi_colsum_ws(int R, int N);
int clipmi_colsum(void* stream, int dtype, const void* x, int64_t ldx, int R, int N, float* out, int beta, void* ws,
                  int64_t ws_bytes);
/* out[t][c] (+)= sum_b x[(b*period+t)][c] for t < nt  (position / class embedding gradients); rows t >= nt of out
 * are not touched.  4-element vector accesses throughout: D % 4 == 0, ldx % 4 == 0, x aligned to 4 elements
 * (8 bytes bf16, 16 bytes fp32) and out to 16 bytes, else CLIPMI_ERR_INVALID. */
int clipmi_period_sum(void* stream, int dtype, const void* x, int64_t ldx, int nb, int period, int nt, int D,
                      float* out, int beta);

/* ---- Bottleneck adapter (adapter/clip_adapter.py:17-23 TextAdapter.forward, :144-150
 * VisionAdapter.forward; adapter/peclip.py:13-18 TextualAdapter with ln = 0) --------------------
 * y = LN(up(gelu_erf(down(x))) + x) * ln_w + ln_b (ln = 0: without the LayerNorm) for R rows
 * (row strides ldx / ldy): w_down [A, D], b_down [A], w_up [D, A], b_up [D] (nn.Linear layout,
 * activation dtype).  One call sequences the library's own kernels on the stream (csrc/adapter.cpp):
 * down GEMM (+ bias + gelu_erf; pre-activation stored when pre != NULL), up GEMM (+ bias + residual),
 * LayerNorm -- the path the Python mirror runs.  act [R, A] is required (it carries the bottleneck
 * between the GEMMs); with ln also z [R, D] (the pre-LN sum) and mean / rstd [R] (fp32).  pre [R, A]
 * is saved for the backward (NULL in inference).  D % 8 == 0, A % 8 == 0; with ln D <= 4096. */
int clipmi_adapter_fwd(void* stream, int dtype, int R, int D, int A, const void* x, int64_t ldx, const void* w_down,
                       const void* b_down, const void* w_up, const void* b_up, const void* ln_w, const void* ln_b,
                       float eps, int ln, void* y, int64_t ldy, void* pre, void* act, void* z, float* mean,
                       float* rstd);
int64_t clipmi_adapter_bwd_ws(int R, int D, int A);
/* dx = dL/dx given dy = dL/dy (the forward's saved tensors); the fp32 parameter gradients g_*
 * (each may be NULL; g_ln_* ignored when ln = 0) ACCUMULATE (+=, AccumulateGrad): LN backward, the
 * up / down weight-gradient GEMMs (bias gradients fused in bf16, a column sum in fp32), the
 * gelu_erf'-fused input-gradient GEMM and the residual-fused dx GEMM; no atomics across tiles, so a
 * replay is bitwise equal. */
int clipmi_adapter_bwd(void* stream, int dtype, int R, int D, int A, const void* dy, int64_t lddy, const void* x,
                       int64_t ldx, const void* pre, const void* act, const void* z, const float* mean,
                       const float* rstd, const void* w_down, const void* w_up, const void* ln_w, int ln, void* dx,
                       int64_t lddx, float* g_w_down, float* g_b_down, float* g_w_up, float* g_b_up, float* g_ln_w,
                       float* g_ln_b, void* ws, int64_t ws_bytes);

/* ---- Embeddings ------------------------------------------------------------------------------
 * text: x0[r] = tok[ids[r]] + pos[r % S]   ([HF] CLIPTextEmbeddings.forward :232-256);
 * *bad_flag |= 1 on an out-of-vocabulary id (Python raises IndexError like nn.Embedding; the row then reads
 * tok[0]).  4-element vector accesses: D % 4 == 0 and tok, pos, x0 aligned to 4 elements (8 bytes bf16, 16 bytes
 * fp32), else CLIPMI_ERR_INVALID.  R = 0 is a no-op. */
int clipmi_text_embed(void* stream, int dtype, const int64_t* ids, const void* tok, const void* pos, void* x0, int R,
                      int S, int D, int V, int* bad_flag);
int64_t clipmi_text_embed_bwd_ws(int R, int V);
/* gtok[v] (+)= sum_{r: ids[r]==v} dx0[r]; rows with an id outside [0, V) contribute nothing.  A counting sort of
 * the ids, then one wave per 64 rows of the sorted order, which adds its run of each id onto gtok with fp32
 * atomicAdd whenever the id changes: the sum's order, and so its last bits, may differ between replays (the one
 * gradient DESIGN.md exempts from bitwise replay).  D % 4 == 0, dx0 aligned to 4 elements; ws need not be
 * initialised. */
int clipmi_text_embed_bwd(void* stream, int dtype, const int64_t* ids, const void* dx0, int R, int D, int V,
                          float* gtok, int beta, void* ws, int64_t ws_bytes);
/* vision: Conv2d(k=s=P, no bias) as im2col + GEMM ([HF] :148-154, :211-212).  X is
 * [B*(G*G+1), Kp] with a zero row in each image's CLS slot, K index c*P*P+ky*P+kx. */
int clipmi_im2col(void* stream, int dtype, const float* pixels, void* X, int B, int C, int H, int P, int Kp);
/* The input step (CLIPImageProcessor's center_crop + rescale + normalize, [HF]
 * image_processing_clip.py) fused into the same im2col: uint8 images [B, Hin, Win, 3]
 * (channels last), centre-cropped to image_size, (u/255 - mean[c]) / std[c].  The shortest-edge
 * resize before it is clipmi_resize_u8 below.  P even (16/32: 8 pixels per thread; ViT-L/14: 2), Kp == 3*P*P or padded
 * to a multiple of 8 (the pad columns are zeroed: L/14's 588 -> 640); mean/std are 3 host floats. */
int clipmi_im2col_u8(void* stream, int dtype, const uint8_t* images, void* X, int B, int Hin, int Win, int image_size,
                     int P, int Kp, const float* mean, const float* std);
/* Input-step resize (dataset.py:152-164 -> CLIPImageProcessor, shortest edge = image size):
 * PIL Image.resize(BICUBIC) of channels-last RGB uint8 [B, Hin, Win, 3] -> [B, Hout, Wout, 3],
 * bit-exact (fp64 tap weights -> 22-bit fixed point, horizontal then vertical 8-bit pass; a pass
 * whose size is unchanged is skipped).  Workspace: clipmi_resize_u8_ws bytes. */
int64_t clipmi_resize_u8_ws(int B, int Hin, int Win, int Hout, int Wout);
int clipmi_resize_u8(void* stream, const uint8_t* in, int B, int Hin, int Win, uint8_t* out, int Hout, int Wout,
                     void* ws, int64_t ws_bytes);
/* Ragged input step (csrc/images.hip; clipmi_version() >= 6): B channels-last RGB uint8 images of different sizes in
 * one packed device buffer -> out uint8 [B, S, S, 3], which clipmi_im2col_u8 takes with Hin = Win = S.  Item b is
 * image b ([h, w, 3] at byte `offset`), an integer crop box (x0, y0, cw, ch) inside it (the whole image: 0, 0, w, h)
 * and flip in {0, 1}.  Semantics: crop, then PIL Image.resize(BICUBIC) of the crop, then the rest; bit-exact with the
 * same fixed-point scheme as clipmi_resize_u8 (taps clamp at the crop's edges, not the image's; a pass whose size
 * does not change is the identity).
 *   mode 0 (processor): the crop's short edge -> S, the long edge -> int(S * long / short); of that image only the
 *                       centre S x S window (offsets (out - S) / 2, clipmi_im2col_u8's) is computed
 *   mode 1 (square):    the crop straight to S x S (a random-resized-crop)
 * flip mirrors the output's columns after the resize (out[y][x] = resized[y][S-1-x]); flipping the source is not
 * bit-identical (tap ranges truncate asymmetrically).  Downscales up to 32 per axis (129 taps); larger ones, a box
 * outside its image, an image outside [0, packed_bytes), flip or mode out of range return CLIPMI_ERR_INVALID naming
 * the item, before any launch.  `items` is host memory: the library validates it, derives the per-image launch
 * records and uploads those into the workspace on the stream; the kernels read nothing else of the caller's but
 * the pixels.  Three launches whatever B is.  clipmi_resize_crop_u8_ws returns the workspace bytes (a negative
 * status on invalid items). */
typedef struct clipmi_image_item {
  int64_t offset;
  int32_t h, w, x0, y0, cw, ch, flip;
} clipmi_image_item;
int64_t clipmi_resize_crop_u8_ws(const clipmi_image_item* items, int B, int S, int mode);
int clipmi_resize_crop_u8(void* stream, const uint8_t* packed, int64_t packed_bytes, const clipmi_image_item* items,
                          int B, uint8_t* out, int S, int mode, void* ws, int64_t ws_bytes);
/* Colour augmentation (csrc/color.hip; clipmi_version() >= 9): torchvision's ColorJitter and RandomGrayscale on PIL
 * images, bit for bit, on channels-last RGB uint8 [B, H, W, 3] in place; each image has its own factors and its own
 * order of the ops.  It runs on clipmi_resize_crop_u8's output: after the resize, the window and the flip.
 *   L(R, G, B)     = (19595 R + 38470 G + 7471 B + 32768) >> 16                             (PIL convert("L"))
 *   blend(d, x, a) = t = fl32(fl32(d) + fl32(a * fl32(x - d))): x - d an integer, the product and the sum two
 *                    separately rounded float32 operations (no fma); trunc(t) when 0 <= a <= 1, else 0 where t <= 0,
 *                    255 where t >= 255, trunc(t) between                                   (PIL Image.blend)
 *   brightness f:  blend(0, x, f) per channel                                               (ImageEnhance.Brightness)
 *   contrast f:    blend(m, x, f), m = floor((2 sum L + n) / (2n)) = int(mean L + 0.5) over the image's n pixels in
 *                  their state after the ops in front of it; an integer sum                 (ImageEnhance.Contrast)
 *   saturation f:  blend(L(pixel), x, f)                                                    (ImageEnhance.Color)
 *   hue shift k:   PIL RGB -> HSV, H = (H + k) mod 256, PIL HSV -> RGB; a listed hue op does the round trip at k = 0
 *                  too (it is not the identity).  float32 unless marked:
 *                  RGB -> HSV: V = mx; mx == mn: H = S = 0; else cr = fl32(mx - mn), s = cr / fl32(mx),
 *                    rc, gc, bc = fl32(mx - c) / cr; h = bc - gc if R == mx, else 2.0 + rc - bc (double) if G == mx,
 *                    else 4.0 + gc - rc (double), rounded to float32; h = fl32(fmod(double(h) / 6.0 + 1.0, 1.0));
 *                    H = clip(int(double(h) * 255.0)), S = clip(int(double(s) * 255.0))
 *                  HSV -> RGB: S == 0: R = G = B = V; else x = double(fl32(H)) * 6.0 / 255.0, i = floor(x),
 *                    f = fl32(x - i), fs = fl32(double(S) / 255.0); in double, rounded half away from zero and
 *                    clipped: p = V (1 - fs), q = V (1 - fs f), t = V (1 - fs (1 - f)); (R, G, B) by i mod 6:
 *                    (V,t,p) (q,V,p) (p,V,t) (p,q,V) (t,p,V) (V,p,q)
 *   gray:          after the list, R = G = B = L(pixel)                                     (convert("L") x 3)
 * `order` lists up to four op codes, 4 bits each, the first op in the low nibble, 0 ends the list; a code appears at
 * most once (so an image has at most one contrast mean).  An item with an empty list and gray = 0 leaves its image's
 * bytes untouched.  `items` is host memory: every item is validated before any launch (NaN, an infinity or a negative
 * factor, hue_shift outside 0..255, an unknown or repeated code, a code after the terminator, gray outside {0, 1}
 * return CLIPMI_ERR_INVALID naming the item; H * W > 2^24, the range of the 32-bit luma sum, is rejected too) and the
 * per-image records are uploaded into the workspace on the stream; the kernels read that copy only.  Two launches
 * whatever B is: the luma sums of the images with a contrast (integer atomics: bitwise reproducible), then every
 * pixel through its image's list.  B == 0 returns.  clipmi_color_u8_ws returns the workspace bytes (a negative status
 * on invalid items); the workspace must be 16-byte aligned. */
typedef struct clipmi_color_item {
  float   brightness, contrast, saturation; /* blend factors: finite, >= 0 */
  int32_t hue_shift;                        /* 0..255 */
  int32_t order;   /* up to four op codes, 4 bits each, first op in the low nibble, 0 ends the list;
                      1 brightness, 2 contrast, 3 saturation, 4 hue; a code at most once */
  int32_t gray;    /* 0 | 1 */
} clipmi_color_item;
int64_t clipmi_color_u8_ws(const clipmi_color_item* items, int B, int H, int W);
int clipmi_color_u8(void* stream, uint8_t* images /* [B,H,W,3], in place */, const clipmi_color_item* items,
                    int B, int H, int W, void* ws, int64_t ws_bytes);
/* Geometric augmentation (csrc/affine.hip; clipmi_version() >= 12): PIL's Image.transform(size, AFFINE, m, NEAREST |
 * BILINEAR, fillcolor=...) bit for bit, which is what torchvision's RandomAffine / RandomRotation do to a PIL image:
 * src uint8 [B, H, W, 3] -> dst of the same shape, image b through items[b].  It runs on clipmi_resize_crop_u8's
 * output and in front of clipmi_color_u8.  m = (a0..a5) maps an output pixel to a source coordinate; every output
 * byte is written, with a sampled value or with the fill colour.  All coefficient arithmetic is IEEE double, each
 * operation rounded on its own (no fma).  For output pixel (x, y):
 *   bilinear (filter 1; PIL affine_transform + bilinear_filter32RGB):
 *     xin = x + 0.5, yin = y + 0.5; xo = (a0 xin + a1 yin) + a2; yo = (a3 xin + a4 yin) + a5;
 *     xo < 0 or xo >= W or yo < 0 or yo >= H: the fill.  Else xo -= 0.5, yo -= 0.5, xi = floor(xo), yi = floor(yo),
 *     dx = xo - xi, dy = yo - yi; x0 = clamp(xi, 0, W - 1), x1 = clamp(xi + 1, 0, W - 1), row = clamp(yi, 0, H - 1);
 *     per channel v1 = p[row][x0] + (p[row][x1] - p[row][x0]) dx (the difference an integer); v2 the same on row
 *     yi + 1 when 0 <= yi + 1 < H, else v2 = v1; v = v1 + (v2 - v1) dy; the byte is trunc(v), inside [0, 255].
 *   nearest (filter 0) with a1 != 0 or a3 != 0 (PIL affine_fixed, 16.16 fixed point, 32-bit integers):
 *     FIX(v) = floor(v * 65536.0 + 0.5); A0 = FIX(a0), A1 = FIX(a1), A3 = FIX(a3), A4 = FIX(a4),
 *     A2 = FIX((a2 + a0 * 0.5) + a1 * 0.5), A5 = FIX((a5 + a3 * 0.5) + a4 * 0.5); the source pixel is
 *     ((A2 + A0 x + A1 y) >> 16, (A5 + A3 x + A4 y) >> 16), arithmetic shifts; outside the image: the fill.
 *   nearest with a1 == 0 and a3 == 0 exactly (PIL ImagingScaleAffine): a column table from a running double sum,
 *     xo = a2 + a0 * 0.5; for x = 0 .. W - 1: xtab[x] = xo < 0 ? -1 : (int)xo, xo += a0; a row table likewise from
 *     a5 + a4 * 0.5 and a4; the output is src[ytab[y]][xtab[x]] when both entries are inside the image, else the
 *     fill.  The running sum is not a2 + a0 (x + 0.5), and that closed form changes bytes.
 * The identity (1, 0, 0, 0, 1, 0) copies the image under either filter.  `items` is host memory: every item is
 * validated before any launch (a non-finite coefficient, a filter outside {0, 1}, a fill outside 0..0xFFFFFF, and,
 * for either coefficient row (a, b, c), |a| W + |b| H + |c| >= 16384 -- below that bound PIL's 32-bit fixed point
 * cannot overflow: 16384 * 65536 = 2^30 -- return CLIPMI_ERR_INVALID naming the item; so do H or W outside 1..4096
 * and src and dst that overlap).  The fixed-point integers are derived on the host and uploaded with the per-image
 * records into the workspace on the stream, in one copy; the kernels read that copy and src only.  One launch whatever
 * B is, plus a pre-pass (one thread per image and axis) that fills the tables behind the records when some item takes
 * the third path; no host synchronisation.  B == 0 returns.  clipmi_affine_u8_ws returns the workspace bytes (a
 * negative status on invalid items); the workspace must be 16-byte aligned. */
typedef struct clipmi_affine_item {
  double  m[6];     /* output pixel -> source coordinate, PIL's AFFINE data (a0..a5) */
  int32_t filter;   /* 0 nearest, 1 bilinear */
  int32_t fill;     /* 0xRRGGBB, the colour where no source pixel is hit */
} clipmi_affine_item;
int64_t clipmi_affine_u8_ws(const clipmi_affine_item* items, int B, int H, int W);
int clipmi_affine_u8(void* stream, const uint8_t* src, uint8_t* dst, const clipmi_affine_item* items, int B, int H,
                     int W, void* ws, int64_t ws_bytes);
/* Policy ops without an affine or a colour kernel (csrc/enhance.hip; clipmi_version() >= 13): PIL's ImageOps.posterize /
 * solarize / autocontrast / equalize and ImageEnhance.Sharpness bit for bit: src uint8 [B, H, W, 3] -> dst of the same
 * shape, image b through items[b]'s one op.  With clipmi_affine_u8 and clipmi_color_u8 these are the fourteen ops of
 * torchvision's RandAugment and TrivialAugmentWide on PIL images (clipmi/images.py apply_policy_u8 runs a per-image
 * sequence of them).  h_c is channel c's 256-bin histogram over the image; the LUTs are per channel.
 *   0 none:         dst = src
 *   1 posterize:    value = bits, an integer in 1..8; i & ~(2^(8 - bits) - 1)               (ImageOps.posterize)
 *   2 solarize:     value = threshold; (float)i < value ? i : 255 - i                       (ImageOps.solarize)
 *   3 autocontrast: lo, hi = the first, last non-empty bin; hi <= lo: the identity; else, in double, each operation
 *                   rounded on its own (no fma): scale = 255.0 / (hi - lo), offset = -lo * scale,
 *                   lut[i] = clamp((int)(i * scale + offset), 0, 255), truncated toward zero: a channel that holds
 *                   only 0 and 200 maps 200 to 254                                          (ImageOps.autocontrast, cutoff 0)
 *   4 equalize:     fewer than two non-empty bins: the identity; step = (sum h - the last non-empty bin) / 255
 *                   (integers); 0: the identity; else n = step / 2 and for i = 0..255: lut[i] = min(n / step, 255),
 *                   n += h[i] (Image.point stores a list LUT's entries clipped to a byte)   (ImageOps.equalize)
 *   5 sharpness:    value = factor >= 0.  d = ImageFilter.SMOOTH of the image: k = (1,1,1,1,5,1,1,1,1) / 13 as float32
 *                   quotients; a float32 accumulator ss = 0.5 takes the three rows one after the other,
 *                   ss += (k0 left + k1 mid) + k2 right, every product and sum a float32 operation of its own; d = 0
 *                   where ss <= 0, 255 where ss >= 255, else trunc(ss); the one-pixel frame of the image is the
 *                   source's, so an image with H < 3 or W < 3 is left whole.  dst = blend(d, src, value), the blend of
 *                   clipmi_color_u8                                                         (ImageEnhance.Sharpness)
 * `items` is host memory: every item is validated before any launch (an unknown op, a non-finite value, posterize bits
 * that are no integer in 1..8, a negative sharpness factor return CLIPMI_ERR_INVALID naming the item; so do B < 0,
 * B > 65535, H or W < 1, H * W > 2^24 -- the range of the 32-bit bins and sums -- null pointers and src and dst that
 * overlap) and the records are uploaded into the workspace on the stream; the kernels read that copy and src only.  At
 * most three launches whatever B is: the histograms of the autocontrast and equalize images (integer atomics into a
 * [B][768] table zeroed by a memset node: bitwise reproducible), their LUTs (one block per image), then every pixel
 * through its image's op; one launch when no item needs a histogram.  No host synchronisation.  B == 0 returns.
 * clipmi_enhance_u8_ws returns the workspace bytes (a negative status on invalid items); the workspace must be 16-byte
 * aligned. */
typedef struct clipmi_enhance_item {
  int32_t op;      /* 0 none, 1 posterize, 2 solarize, 3 autocontrast, 4 equalize, 5 sharpness */
  float   value;   /* posterize: bits; solarize: threshold; sharpness: factor; else ignored (finite) */
} clipmi_enhance_item;
int64_t clipmi_enhance_u8_ws(const clipmi_enhance_item* items, int B, int H, int W);
int clipmi_enhance_u8(void* stream, const uint8_t* src, uint8_t* dst, const clipmi_enhance_item* items, int B, int H,
                      int W, void* ws, int64_t ws_bytes);
/* pooled token per row: mode 0 first token (model_m.py:102), 1 first EOS (0 when the row has none), 2 argmax id,
 * the first of tied maxima ([HF] :561-581).  gather: out[b] = src[b*S + idx[b]]; scatter: dst[b*S + idx[b]] (+)=
 * src[b], the other rows of dst untouched; idx NULL: token 0.  B = 0 is a no-op. */
int clipmi_pool_index(void* stream, const int64_t* ids, int B, int S, int64_t eos, int mode, int* idx);
int clipmi_gather_rows(void* stream, int dtype, const void* src, const int* idx, int B, int S, int D, void* out);
int clipmi_scatter_rows(void* stream, int dtype, const void* src, const int* idx, int B, int S, int D, void* dst,
                        int beta);

/* ---- Attention (head_dim 64, N <= 4096: K/V resident in LDS up to N = 288, K/V streamed above;
 * [HF] CLIPAttention :298-335, eager core :259-277) -----
 * qkv: [B*N, 3D] (q | k | v, head h at h*64), o: [B*N, D], lse: [B*H*N] fp32.
 * attention_mask: int64 [B, N] key padding (1 keep) or NULL; causal for the text tower. */
int clipmi_attention_fwd(void* stream, int dtype, const void* qkv, void* o, float* lse, const int64_t* attention_mask,
                         int causal, int B, int H, int N, int D);
/* The K/V-streaming forward with O written as MXFP8 (OCP e4m3 o8 [B*N, D], 4-byte aligned + E8M0 s8 [B*N, D/32],
 * clipmi_quant_mxfp8's rule applied to the fp32 O): the fp8 towers' out-projection operand without a
 * bf16 round trip (BASELINE config 5).  bf16 q/k/v. */
int clipmi_attention_fwd_mxfp8(void* stream, const void* qkv, uint8_t* o8, uint8_t* s8, float* lse,
                               const int64_t* attention_mask, int causal, int B, int H, int N, int D);
int clipmi_attention_bwd(void* stream, int dtype, const void* qkv, const void* o, const float* lse, const void* dout,
                         void* dqkv, const int64_t* attention_mask, int causal, int B, int H, int N, int D);
/* Single-query attention (csrc/attention_cls.hip; clipmi_version() >= 5): one query per (sequence, head) -- the
 * CLS row of the vision tower's last layer -- against all N keys / values.  For hosts that pool one row (inference
 * or their own training loop); the encoder engine does not call it: its cls_last mode keeps the MFMA attention
 * kernels so that a step computes the bits of the full mode, and these kernels keep the probabilities in fp32 where
 * those round them to bf16.  Head dim 64 (D == 64 H), 1 <= N <= 4096,
 * no mask, dtype bf16 or fp32.  q [B][ldq], kv [B*N][2D] (K | V, head h at h*64 in each half), o [B][ldo],
 * lse [B][H] fp32.  Per (b, h), scale = 1/8: s_j = scale q.k_j, p = softmax(s), o = sum_j p_j v_j,
 * lse = log sum_j e^{s_j}.  Backward (p recomputed from lse): dkv [B*N][2D] (dK | dV), dq [B][lddq]; dkv0 (may be
 * NULL) [B][ld0] receives a second copy of row 0's dK | dV at columns [0, 2D), so a caller can lay
 * dq | dK_0 | dV_0 out as one [B][3D] operand.  Scores, probabilities and sums are fp32, each output is rounded
 * once; fixed-order sums, so a replay is bitwise equal.  Pointers 16-byte aligned, leading dimensions multiples of
 * 16 bytes.  Arguments are checked before any HIP call; B = 0 is a no-op. */
int clipmi_attention_cls_fwd(void* stream, int dtype, const void* q, int64_t ldq, const void* kv, void* o, int64_t ldo,
                             float* lse, int B, int H, int N, int D);
int clipmi_attention_cls_bwd(void* stream, int dtype, const void* q, int64_t ldq, const void* kv, const void* o,
                             int64_t ldo, const float* lse, const void* dout, int64_t lddo, void* dkv, void* dq,
                             int64_t lddq, void* dkv0, int64_t ld0, int B, int H, int N, int D);
/* bf16x3 split images (the layout of CLIPMI_GEMM_SPLIT3's operands): clipmi_split3 writes the image of an fp32
   operand -- k-major X [rows][K] -> bf16 [rows][3K], else X [K][rows] -> [3K][round8(rows)] -- with segments
   (h, h, l) for pattern 0 or (h, l, h) for pattern 1, h = bf16(x), l = bf16(x - h); clipmi_split3_elems gives its
   size in elements.  clipmi_split3_colsum writes the k-major image of x [R, N] and, with colsum, adds x's column
   sums to colsum[N] (+= when beta; ws >= clipmi_split3_colsum_ws(R, N) bytes, 16-byte aligned). */
int64_t clipmi_split3_elems(int rows, int K, int kmajor);
int clipmi_split3(void* stream, const float* X, int64_t ldx, int rows, int K, int kmajor, void* out, int pattern);
int64_t clipmi_split3_colsum_ws(int R, int N);
int clipmi_split3_colsum(void* stream, const float* x, int64_t ldx, int R, int N, void* out, int pattern,
                         float* colsum, int beta, void* ws, int64_t ws_bytes);
/* A bf16 GEMM (d->ab_dtype CLIPMI_BF16, d->c_dtype CLIPMI_F32: the epilogue computes in fp32) whose result is
   written as its split image instead -- d->C bf16 [M][d->ldc], ldc >= 3N, segments at columns n, N + n, 2N + n in
   the pattern above -- by the producing kernel's epilogue (the bf16x3 mode's fc1 output and fc2 input gradient,
   which clipmi_split3_colsum would otherwise split from an fp32 copy).  Flags: bias + quick_gelu (+ store_dact:
   the derivative to fp32 aux), or mul_aux (fp32 aux).  colsum (+= when beta): the column sums of the fp32 result,
   ws >= clipmi_gemm_x3out_ws(M, N) bytes, 256-byte aligned.  clipmi_gemm_x3out_ok: whether a shape / layout /
   flag set has this form (k-major A, M >= 256, N >= 128, N % 8 == 0, K % 64 == 0). */
int64_t clipmi_gemm_x3out_ws(int M, int N);
int clipmi_gemm_x3out_ok(int M, int N, int K, int a_kmajor, int b_kmajor, int flags);
int clipmi_gemm_x3out(void* stream, const clipmi_gemm_desc* d, int pattern, float* colsum, int beta, void* ws,
                      int64_t ws_bytes);
/* bf16x3 engine: the fp32 LayerNorm backward (as clipmi_layernorm_bwd with dtype CLIPMI_F32, dw / db required) that
   also writes dx as its pattern-1 split image dimg bf16 [R][3D] and adds dx's column sums onto colsum[D] (+= when
   beta_cs) -- the next GEMMs' operand and a Linear's bias gradient without a split pass.  D / 64 in
   {1, 2, 3, 4, 6, 8, 12, 16}; ws >= clipmi_layernorm_bwd_x3_ws(R, D) bytes, 16-byte aligned. */
int64_t clipmi_layernorm_bwd_x3_ws(int R, int D);
int clipmi_layernorm_bwd_x3(void* stream, const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* mean,
                            const float* rstd, const float* w, float* dx, int64_t lddx, const float* dres,
                            int64_t ldres, float* dw, float* db, int beta_wb, void* dimg, float* colsum, int beta_cs,
                            void* ws, int64_t ws_bytes, int R, int D);
/* LayerNorm of fp32 x with fp32 affine weights written as the bf16x3 split image y3 [R][3D] of its output
   (pattern as above); mean / rstd saved as in clipmi_layernorm_fwd.  D / 64 in {1, 2, 3, 4, 6, 8, 12, 16}. */
int clipmi_layernorm_fwd_x3(void* stream, const float* x, int64_t ldx, void* y3, int pattern, const float* w,
                            const float* b, float* mean, float* rstd, int R, int D, float eps);
/* The bf16x3 precision mode's attention (csrc/attention_x3.hip): fp32 operands and outputs exactly as
   clipmi_attention_fwd / _bwd with dtype CLIPMI_F32, every product (q k^T, P v, dO v^T, dS k, dS^T q, P^T dO)
   run as three bf16 MFMA products of the hi / lo operand splits (~2^-16 relative per product).  N > 288 falls
   back to the exact-f32 kernels. */
int clipmi_attention_fwd_x3(void* stream, const void* qkv, void* o, float* lse, const int64_t* attention_mask,
                            int causal, int B, int H, int N, int D);
int clipmi_attention_bwd_x3(void* stream, const void* qkv, const void* o, const float* lse, const void* dout,
                            void* dqkv, const int64_t* attention_mask, int causal, int B, int H, int N, int D);
/* clipmi_attention_fwd_x3 that also writes O's pattern-0 split image oimg bf16 [B*N][3D] (8-byte aligned) beside the
   fp32 O: the out-projection's operand in the bf16x3 engine without a split pass.  N <= 288. */
int clipmi_attention_fwd_x3img(void* stream, const void* qkv, void* o, void* oimg, float* lse,
                               const int64_t* attention_mask, int causal, int B, int H, int N, int D);
/* clipmi_attention_bwd_x3 with d_qkv written as its pattern-1 split image dimg bf16 [B*N][9D] (the layout of
   clipmi_split3_colsum) and d_qkv's column sums (the q / k / v bias gradient) added onto colsum[3D] (+= when beta),
   instead of the fp32 dqkv; N <= 288, ws >= clipmi_attention_bwd_x3img_ws(B, D) bytes, 256-byte aligned. */
int64_t clipmi_attention_bwd_x3img_ws(int B, int D);
int clipmi_attention_bwd_x3img(void* stream, const void* qkv, const void* o, const float* lse, const void* dout,
                               void* dimg, float* colsum, int beta, void* ws, int64_t ws_bytes,
                               const int64_t* attention_mask, int causal, int B, int H, int N, int D);

/* ---- Encoder engine: whole CLIPEncoder fwd/bwd in one call ([HF] :477-482, :362-383) ---------- */
typedef struct clipmi_layer_w { /* activation dtype; qkv_w = [q;k;v] rows, [3D, D] */
  const void *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} clipmi_layer_w;
typedef struct clipmi_layer_grad { /* fp32, accumulated */
  float *ln1_w, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_w, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
} clipmi_layer_grad;
typedef struct clipmi_layer_act { /* saved activations; pre == NULL in inference.  The fp8 encoder
  * (dtype CLIPMI_FP8) with N > 288 sends the attention output straight to the out-projection's
  * MXFP8 operand and does NOT write o: read act[l].o only after a bf16 / f32 forward or N <= 288. */
  void *x_in, *ln1, *qkv, *o, *h, *ln2, *pre, *act;
  float *mean1, *rstd1, *lse, *mean2, *rstd2;
} clipmi_layer_act;
typedef struct clipmi_layer_w8 { /* MXFP8 GEMM weights: e4m3 [out, in] + E8M0 scales [out, in/32] */
  const void *qkv_w, *qkv_s, *out_w, *out_s, *fc1_w, *fc1_s, *fc2_w, *fc2_s;
} clipmi_layer_w8;
typedef struct clipmi_encoder_desc {
  int dtype, B, N, D, F, H, L;  /* dtype CLIPMI_FP8: bf16 activations / LN / attention, MXFP8 GEMMs (forward only) */
  float eps;
  int causal;
  const int64_t* attention_mask;
  const clipmi_layer_w* layers;  /* [L] (bf16 LN weights and biases also for CLIPMI_FP8) */
  clipmi_layer_grad* grads;      /* [L], backward only */
  clipmi_layer_act* act;         /* [L]; layer l writes its output to act[l+1].x_in (x_out for the last) */
  void* x_out;
  void* workspace;
  int64_t workspace_bytes;
  const clipmi_layer_w8* layers8; /* [L], CLIPMI_FP8 only */
  void* q8;                       /* CLIPMI_FP8: MXFP8 activation scratch, align256(R*D) + R*F bytes (R = B*N) */
  void* s8;                       /* CLIPMI_FP8: its block scales, align256(R*D/32) + R*F/32 bytes */
  /* dtype CLIPMI_BF16 only: the residual stream in fp32 -- act[l].x_in, act[l].h and x_out are fp32
   * (LayerNorms read them as fp32, the out-projection / fc2 epilogues add and write fp32), every GEMM
   * operand stays bf16.  The reference is fp32 end to end (trainer.py:81-99); rounding the residual sum
   * to bf16 at each of the 2L residual adds was the largest bf16-mode error (profiles/r05_bf16_error_sources.log). */
  int resid_f32;
  /* dtype CLIPMI_F32 only (precision "bf16x3"): every GEMM of the forward and backward runs as three bf16
   * products of hi / lo operand splits, over split images (clipmi_split3) that each activation's and activation
   * gradient's producer writes once; attention as clipmi_attention_fwd_x3 / _bwd_x3; LayerNorm, softmax,
   * residual stream and all accumulation fp32.  Scratch in x3_ws (x3_ws_bytes >= clipmi_encoder_x3_ws, 256-byte
   * aligned; one scratch per concurrently running encoder).  The saved activations change form in this mode:
   * act[l].ln1 / .ln2 hold the bf16 [R][3D] images of the LayerNorm outputs, act[l].o the fp32 [R][D] attention
   * output followed (at the next 256-byte boundary) by its [R][3D] image, act[l].act the bf16 [R][3F] image of
   * fc1's output; x_in, qkv, h and pre stay fp32 (csrc/engine.cpp encoder_fwd_x3). */
  int gemm_x3;
  void* x3_ws;
  int64_t x3_ws_bytes;
  /* causal encoders only (clipmi_version() >= 2): compute token 0 of every sequence and nothing else.  Under a
   * causal mask token 0 attends only to itself in every layer, so its output depends on row 0 of the input alone
   * and, when only token 0 is pooled (model_m.py:102), every gradient at the other rows is exactly zero.
   * Layout: the engine works on B rows, row b = token 0 of sequence b -- x_in, x_out, every act[l] buffer and dx
   * are compact [B][.]; N stays the real sequence length and attention_mask stays [B, N] (mask[b * N] is read).
   * Per layer: LN1, the V projection alone (rows [2D, 3D) of qkv_w, bias qkv_b + 2D; output [B][D] in act[l].qkv),
   * O = V (a softmax over one key is 1; O = 0 where mask[b * N] == 0, as the attention kernels give a row with no
   * valid key; act[l].qkv then holds O), out-projection + residual, LN2, fc1, fc2 on B rows.  act[l].o and
   * act[l].lse are neither read nor written and may be NULL.  The backward mirrors it: dV = dO (same row select),
   * the V weight / bias gradients into grads[l].qkv_w + 2D*D / grads[l].qkv_b + 2D; the q and k slots of both
   * are NOT touched (gradients accumulate, and their exact value is zero).  Not with CLIPMI_FP8 or gemm_x3. */
  int first_token;
  /* clipmi_version() >= 5: the caller reads row 0 (CLS) of each sequence's output and nothing else (model_m.py:122,
   * no post-LayerNorm: quirk Q2).  Layers 0 .. L-2 run as usual; in layer L-1 the other rows matter only as keys and
   * values for the CLS query, so it runs LN1, the q | k | v projection and the attention on all R = B*N rows, with
   * the full mode's kernels (the CLS row of the attention output keeps the full mode's bits), and everything after
   * the attention -- out-projection + residual, LN2, fc1, fc2 -- on the B CLS rows (rows b*N, read in place with a
   * leading dimension of N*D).  x_out is compact [B][D].
   * Not with causal (such towers use first_token), first_token, CLIPMI_FP8, gemm_x3 or an attention_mask; N <= 4096.
   * act[L-1] keeps the sizes clipmi_encoder_act_bytes gives for the full mode (cls_last does not change them):
   *   x_in, ln1, mean1, rstd1, qkv, o, lse   all R rows, as in the full mode
   *   h, ln2, pre, act, mean2, rstd2         the first B rows
   * Backward: the dx buffer always holds R*D elements; when the call's layer range includes layer L-1
   * (layer_hi == L) its first B rows hold dL/dx_out on entry; on exit it holds the [R][D] gradient of
   * act[layer_lo].x_in as in the full mode.  The MLP's and the out-projection's gradients run on B rows; the attention
   * backward, the qkv weight gradient and d_ln1 run on all rows with d_o zero outside the CLS rows (the values the
   * full mode computes there), and LN1's backward adds the compact residual gradient at the CLS rows
   * (clipmi_layernorm_bwd4).  Activations and activation gradients are bitwise those of the full mode given a
   * gradient that is zero outside the CLS rows; weight gradients differ by the order of their fp32 sums. */
  int cls_last;
} clipmi_encoder_desc;
/* Bytes of each clipmi_layer_act member for one layer in the descriptor's mode (dtype, resid_f32, gemm_x3,
 * first_token; B, N, D, F, H; cls_last does not change them), in member order: x_in, ln1, qkv, o, h, ln2, pre, act, mean1, rstd1, lse, mean2,
 * rstd2.  0: the member is not used in this mode (may be NULL); pre is needed by a training forward only.
 * Only the shape / mode fields of d are read. */
int clipmi_encoder_act_bytes(const clipmi_encoder_desc* d, int64_t out[13]);
int clipmi_encoder_fwd(void* stream, const clipmi_encoder_desc* d);
int64_t clipmi_encoder_bwd_ws(const clipmi_encoder_desc* d);
/* the split-image scratch of a gemm_x3 encoder (forward and backward; 0 when gemm_x3 is off) */
int64_t clipmi_encoder_x3_ws(const clipmi_encoder_desc* d);
/* dx: dL/d(encoder output) in, dL/d(encoder input) out */
int clipmi_encoder_bwd(void* stream, const clipmi_encoder_desc* d, void* dx);
/* the same for layers layer_hi-1 .. layer_lo only (chunked backward: each chunk's gradient slice
 * can be all-reduced while the next chunk runs) */
int clipmi_encoder_bwd_layers(void* stream, const clipmi_encoder_desc* d, void* dx, int layer_hi, int layer_lo);

/* ---- Contrastive head (model_m.py:146-171), fp32; every entry point is a no-op at B = 0 ------ */
int clipmi_l2norm_fwd(void* stream, const float* x, float* y, float* nrm, int B, int E);
int clipmi_l2norm_bwd(void* stream, const float* dy, const float* y, const float* nrm, float* dx, int B, int E);
/* logits = exp(*logit_scale) * S over a [B, Bg] cosine block; lse, ce per row (label0 + i) */
int clipmi_contrastive_ce_fwd(void* stream, const float* S, float* logits, const float* logit_scale, int B, int Bg,
                              int label0, float* lse, float* ce);
/* dS = g*exp(ls)*(softmax - onehot)*norm ; dls_row = sum_j dlogit*logit */
int clipmi_contrastive_ce_bwd(void* stream, const float* logits, const float* lse, const float* logit_scale,
                              const float* grad_out, int B, int Bg, int label0, float norm, float* dS, float* dls_row);
/* Column-streamed form (the [B, Bg] blocks never materialised): the caller walks chunks
 * [col0, col0 + C) of the cosine block S (row stride C).  fwd_chunk merges the chunk into the
 * running per-row (max, sum-of-exp) pairs run [B][2] (col0 == 0 initialises them) and stores
 * the label logit lab[i] when column label0 + i lies in the chunk; finish turns them into lse, ce.
 * bwd_chunk writes the chunk's dS [B][C] and sets (beta = 0) or accumulates dls_row. */
int clipmi_contrastive_ce_fwd_chunk(void* stream, const float* S, const float* logit_scale, int B, int C, int col0,
                                    int Bg, int label0, float* run, float* lab);
int clipmi_contrastive_ce_finish(void* stream, const float* run, const float* lab, int B, float* lse, float* ce);
int clipmi_contrastive_ce_bwd_chunk(void* stream, const float* S, const float* lse, const float* logit_scale,
                                    const float* grad_out, int B, int C, int col0, int Bg, int label0, float norm,
                                    float* dS, float* dls_row, int beta);
int clipmi_sum2(void* stream, const float* a, const float* b, int n, float scale, float* out, int beta);

/* ---- Multi-positive contrastive head (csrc/contrastive_keys.hip), fp32 -------------------------
 * keys_all int64 [Bg]: one key per pair of the global batch.  Row i (global index label0 + i) of a [B, Bg] score
 * block has the positives P_i = { j : keys_all[j] == keys_all[label0 + i] }, and
 *   ce_i = lse_i - winv_i * sum_{j in P_i} logit_ij,  winv_i = 1 / |P_i|
 *   dlogit_ij = g * norm * (softmax_ij - [j in P_i] winv_i);  dls_row as in clipmi_contrastive_ce_bwd.
 * With all keys distinct every output is bit for bit that of the clipmi_contrastive_ce_* entry point of the same
 * form (winv = 1).  Guards: keys_all non-null, 0 <= label0, label0 + B <= Bg, chunk inside [0, Bg); B = 0 returns. */
int clipmi_contrastive_keyed_fwd(void* stream, const float* S, float* logits, const float* logit_scale,
                                 const int64_t* keys_all, int B, int Bg, int label0, float* lse, float* ce,
                                 float* winv);
int clipmi_contrastive_keyed_bwd(void* stream, const float* logits, const float* lse, const float* winv,
                                 const float* logit_scale, const float* grad_out, const int64_t* keys_all, int B,
                                 int Bg, int label0, float norm, float* dS, float* dls_row);
/* Column-streamed form, as clipmi_contrastive_ce_fwd_chunk / _finish / _bwd_chunk: the running state is
 * run [B][4] = (max, sum-of-exp, positive-logit sum, positive count as an int32 bit pattern); col0 == 0 initialises
 * it, a chunk without a positive of a row leaves that row's last two unchanged.  finish writes lse, ce and winv. */
int clipmi_contrastive_keyed_fwd_chunk(void* stream, const float* S, const float* logit_scale, const int64_t* keys_all,
                                       int B, int C, int col0, int Bg, int label0, float* run);
int clipmi_contrastive_keyed_finish(void* stream, const float* run, int B, float* lse, float* ce, float* winv);
int clipmi_contrastive_keyed_bwd_chunk(void* stream, const float* S, const float* lse, const float* winv,
                                       const float* logit_scale, const float* grad_out, const int64_t* keys_all, int B,
                                       int C, int col0, int Bg, int label0, float norm, float* dS, float* dls_row,
                                       int beta);
/* out[r] = 64-bit FNV-1a over ids[r][0:N), each token one uint64: h = (h ^ v) * 0x100000001b3 from
 * 0xcbf29ce484222325 ("same caption" as a key, on the device) */
int clipmi_row_hash64(void* stream, const int64_t* ids, int B, int N, int64_t* out);

/* ---- Pairwise sigmoid contrastive head (csrc/contrastive_sigmoid.hip), fp32 --------------------
 * Every (text, image) pair of the global batch is one binary problem (Zhai et al. 2023).  A rank scores its B text
 * rows (global indices label0 + i) against all Bg image rows; S holds the cosines of columns [col0, col0 + C), row
 * stride C.  With sc = exp(*logit_scale), b = *logit_bias:
 *   l_ij = sc * s_ij + b
 *   z_ij = +1 if keys_all[j] == keys_all[label0 + i] (keys_all null: if j == label0 + i), else -1
 *   loss = norm * sum_ij softplus(-z_ij l_ij)
 *   u_ij = d loss / d l_ij = -z_ij sigmoid(-z_ij l_ij) norm
 *   dS_ij = u_ij sc;   d logit_scale = sum_ij u_ij sc s_ij;   d logit_bias = sum_ij u_ij
 * clipmi_sigmoid_pairs handles one chunk and keeps the row sums rows [B][3] = (sum_j softplus, sum_j u sc s,
 * sum_j u): col0 == 0 sets them, later chunks add to them.  A materialised block is the chunk C == Bg, col0 == 0.
 * logits (null, or [B][C]) receives l; dS (null, or [B][C]; may be S itself) receives dS.  dS == null is the no-grad
 * form: only rows[.][0] is formed and rows[.][1:3] are left as they are.  softplus and sigmoid go through
 * exp(-|x|) alone, so any finite logit gives finite outputs.  keys_all null and all-distinct keys give the same bits.
 * Guards: logit_bias, rows non-null; 0 <= label0, label0 + B <= Bg; the chunk inside [0, Bg); B = 0 returns.
 * clipmi_sigmoid_reduce sums rows [n][3] over n in a fixed tree: loss[0] = norm * sum_0; dls[0] = g * sum_1 and
 * db[0] = g * sum_2 with g = *gscale (null: 1), set (beta = 0) or accumulated (beta = 1, e.g. straight into the
 * gradient arenas).  Each of loss, dls, db may be null (not all three); with dls and db both null columns 1, 2 of
 * rows are not read.  n = 1 scales and accumulates sums that are already reduced. */
int clipmi_sigmoid_pairs(void* stream, const float* S, const float* logit_scale, const float* logit_bias,
                         const int64_t* keys_all, int B, int C, int col0, int Bg, int label0, float norm,
                         float* logits, float* dS, float* rows);
int clipmi_sigmoid_reduce(void* stream, const float* rows, int n, float norm, const float* gscale, float* loss,
                          float* dls, float* db, int beta);

/* ---- Optimizer (trainer.py:95,98; [HF] optimization.py:101-129) ------------------------------ */
int64_t clipmi_grad_norm_ws(void);
/* norm_out[0] = ||g||_2, norm_out[1] = min(1, max_norm/(norm+1e-6)) (device memory) */
int clipmi_grad_norm(void* stream, const float* g, int64_t n, float max_norm, float* norm_out, void* ws,
                     int64_t ws_bytes);
int64_t clipmi_grad_norm_multi_ws(int count);
int clipmi_grad_norm_multi(void* stream, const float* const* gs, const int64_t* ns, int count, float max_norm,
                           float* norm_out, void* ws, int64_t ws_bytes);
int clipmi_grad_scale(void* stream, float* g, int64_t n, const float* norm_out);
/* torch.optim.AdamW step on a flat fp32 arena; grads scaled by clip[1] when clip != NULL;
 * shadow (bf16, may be NULL) refreshed from the new parameters. */
int clipmi_adamw(void* stream, float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, double lr,
                 double beta1, double beta2, double eps, double weight_decay, int step, const float* clip);
int clipmi_cast_f32_bf16(void* stream, const float* src, void* dst, int64_t n);

/* ---- Feature-level adapter heads (model_t.py CLIPAdapter / ZeroShot) -----
 * All fp32, rows of E <= 1024 features, bottleneck A <= 256, C <= 1024 classes.
 * clipmi_feature_adapter_fwd replaces VisualAdapter/TextAdapter.forward (model_t.py:13-33) fused
 * with the residual blend and renormalisation of model_t.py:186-197 (visual, norm_in = 1: the
 * input is normalised first, model_t.py:182-183) and :113-119 / :200-207 (text prototypes,
 * norm_in = 0): xn = norm_in ? x/|x| : x; h = relu(W1 xn + b1); z = alpha (W2 h + b2) +
 * (1 - alpha) xn; out = z/|z|; rz = 1/|z|.  W1 [A, E], W2 [E, A] (nn.Linear layout). */
int clipmi_feature_adapter_fwd(void* stream, const float* x, int B, int E, int A, const float* W1, const float* b1,
                               const float* W2, const float* b2, float alpha, int norm_in, float* xn, float* h,
                               float* out, float* rz, const uint8_t* keep, float keep_scale);
/* keep (uint8 [B, A], may be NULL): training-mode nn.Dropout on the ReLU output (model_v.py:18-27:
 * fc2(dropout(relu(fc1(x))))), h *= keep * keep_scale with keep_scale = 1/(1-p). */
int clipmi_feature_adapter_bwd_ws(int B, int E, int A);
/* grads = [dW1 | db1 | dW2 | db2] (flat, fp32) += the batch's gradients given dout = dL/dout;
 * keep_scale: the forward's (1 when it ran without dropout). */
int clipmi_feature_adapter_bwd(void* stream, const float* dout, const float* out, const float* rz, const float* xn,
                               const float* h, int B, int E, int A, const float* W2, float alpha, float* grads,
                               void* workspace, int64_t workspace_bytes, float keep_scale);
/* Dropout masks (nn.Dropout(p) in model_v.BaseAdapter and SharedMHSAttentionAdapter,
 * adapter/clip_adapter.py:84,96): keep[i] = u(seed, offset + i) >= p with a counter-based hash,
 * so a (seed, offset) pair reproduces its mask; apply: y = x * keep * scale (+ res, may be NULL). */
int clipmi_dropout_mask(void* stream, uint8_t* keep, int64_t n, float p, uint64_t seed, uint64_t offset);
int clipmi_dropout_apply(void* stream, const float* x, const uint8_t* keep, int64_t n, float scale, const float* res,
                         float* y);
/* Average fusion of model_v.EnhancedCLIPAdapter (model_v.py:310-315): out = normalise((a + b) / 2),
 * ru = 1/|(a+b)/2|; backward d a = d b = dab. */
int clipmi_fuse_avg(void* stream, const float* a, const float* b, int B, int E, float* out, float* ru);
int clipmi_fuse_avg_bwd(void* stream, const float* dout, const float* out, const float* ru, int B, int E, float* dab);
/* Class scores (model_t.py:200-203 logits, :240-247 predict, :252-298 predict_with_all_descriptions):
 * s[b, c] = max over descriptions j in [off[c], off[c+1]) of scale * img[b] . desc[j]; probs =
 * softmax_c.  Any output may be NULL.  With labels (int64 [B]): loss_rows[b] = CE of row b,
 * dscore = softmax - onehot, *bad = 1 on an out-of-range label. */
int clipmi_class_scores(void* stream, const float* img, int B, int E, const float* desc, const int* off, int C,
                        float scale, float* scores, float* probs, const int64_t* labels, float* loss_rows,
                        float* dscore, int* bad);
int clipmi_row_mean(void* stream, const float* v, int B, float* out);
/* Mean-CE backward through prototype scores (one description per class): d = dscore * gscale[0] / B;
 * dimg = scale d P, dprotos = scale d^T img.  gscale may be NULL (1). */
int clipmi_class_ce_bwd(void* stream, const float* dscore, const float* img, const float* protos, int B, int C, int E,
                        float scale, const float* gscale, float* dimg, float* dprotos);
/* Multi-label class scores (csrc/multilabel.hip; clipmi_version() >= 14): the scores of clipmi_class_scores, the
 * same device function and so the same bits, plus bias[c] when bias is given ([C] or NULL), with a sigmoid / binary
 * cross-entropy tail (torch.nn.BCEWithLogitsLoss) in place of the softmax / cross-entropy one: probs = sigmoid(z).
 * With targets (fp32 [B, C] in [0, 1], soft labels allowed) and pw = pos_weight[c] ([C] or NULL = 1):
 *   l[b, c]      = (1 - y) z + (1 + (pw - 1) y) (log1p(exp(-|z|)) + max(-z, 0))
 *   loss_rows[b] = (1 / C) sum_c l[b, c]     (clipmi_row_mean of it = BCEWithLogitsLoss(pos_weight, "mean"))
 *   dscore[b, c] = ((1 - y) sigmoid(z) - pw y (1 - sigmoid(z))) / C
 * so clipmi_class_ce_bwd (which divides by B) turns dscore into dimg and dprotos unchanged.  A target outside
 * [0, 1] or NaN sets *bad = 1 and contributes neither loss nor gradient.  Any output may be NULL; targets need bad,
 * pos_weight needs targets.  B >= 1, E <= 1024, C <= 1024.  z = +-100 gives probs 1 / 0 and a finite loss. */
int clipmi_class_bce(void* stream, const float* img, int B, int E, const float* desc, const int* off, int C,
                     float scale, const float* bias, const float* targets, const float* pos_weight, float* scores,
                     float* probs, float* loss_rows, float* dscore, int* bad);
/* The bias gradient of the mean loss: dbias[c] = (gscale ? gscale[0] : 1) / B * sum_b dscore[b, c].  Fixed summation
 * order (no float atomics): two runs give the same bits.  (clipmi_colsum has no scale and needs a workspace.) */
int clipmi_class_bias_grad(void* stream, const float* dscore, int B, int C, const float* gscale, float* dbias);

/* Row softmax of scale*x (fp32, y may alias x) and its backward dx = scale*y*(dy - <dy, y>):
 * the shared cross-attention adapter's probabilities (adapter/clip_adapter.py:117). */
int clipmi_softmax_rows(void* stream, const float* x, float* y, int R, int N, float scale);
int clipmi_softmax_rows_bwd(void* stream, const float* y, const float* dy, float* dx, int R, int N, float scale);

/* ---- Evaluation (csrc/eval.hip; clipmi_version() >= 3) -----------------------------------------
 * Retrieval ranks of N queries against M candidates without the [N, M] score matrix (the recall@K /
 * median-rank metrics of a dual encoder; the reference has none, its trainer.py:101-118 evaluate() is a mean
 * batch loss).  The caller walks blocks S = Q[row0 : row0 + rows] . C[col0 : col0 + cols]^T (fp32, row stride
 * lds >= cols, from clipmi_gemm) in a bounded scratch.  Query i's target candidate is target[i] (int64 [N]) or i
 * when target == NULL (paired data, N == M).  Outputs are indexed by the global query row:
 *   rank_pick   target_score[i] = S[i - row0][t_i - col0] for the rows whose target lies in the block's columns;
 *   rank_count  greater[i] / equal[i] (+)= #{ j in the block, j != t_i : S[i, j] > / == target_score[i] } and
 *               (top1[i], top1_score[i]) = the row maximum so far, lowest candidate index on ties; first != 0
 *               (the row range's first block) stores instead of accumulating.
 * Run rank_pick over every block that can hold a target before rank_count over all blocks, with the SAME
 * clipmi_gemm call (shape, split_k) per block in both passes: the counts then compare target_score against the
 * bits it was read from, so a duplicate of the target counts in `equal`, never in `greater`.  Blocks of one row
 * range must be serialised on one stream (no atomics).  A target outside [0, M) sets *bad = 1 and leaves -1 in
 * all five outputs of its row.  Row loads are 16-byte vectors when S is 16-byte aligned and lds % 4 == 0. */
int clipmi_rank_pick(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols,
                     const int64_t* target, float* target_score, int* bad);
int clipmi_rank_count(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols,
                      const int64_t* target, const float* target_score, int first, int* greater, int* equal,
                      int* top1, float* top1_score);
/* Top-K retrieval over the same streamed blocks (csrc/topk.hip; clipmi_version() >= 4): after the call, rows
 * row0 .. row0 + rows - 1 of top_score / top_idx ([N, k] contiguous, indexed by the global query row) hold the k
 * best candidates of every block merged so far, best first.  S, lds, N, M and the block ranges are as for
 * clipmi_rank_count.  The order is strict and total: candidate a precedes b iff s_a > s_b, or s_a == s_b and
 * j_a < j_b, with -0.0 == +0.0 (reported as +0.0); scores are expected to be finite, a NaN is ordered and
 * reported as -inf.  The result therefore does not depend on the block size or on the order of the column
 * blocks, given equal score bits.  first != 0 starts the row range's lists from empty, otherwise the block is
 * merged into the lists already in the outputs.  Slots beyond the number of candidates seen hold idx -1 and
 * score -inf.  exclude (int64 [N] or NULL): candidate exclude[i] never enters query i's list (the positive, for
 * hard-negative mining; pass it with every block); a value outside [0, M) excludes nothing.
 * 1 <= k <= CLIPMI_TOPK_MAX.  Rows outside the block's row range are not touched.  Blocks of one row range must
 * be serialised on one stream (no atomics); nothing is allocated or synchronised.  Row loads are 16-byte
 * vectors when S is 16-byte aligned and lds % 4 == 0. */
#define CLIPMI_TOPK_MAX 256
int clipmi_topk_merge(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols,
                      int k, int first, const int64_t* exclude, float* top_score, int* top_idx);
/* Group-aware ranks over the same streamed blocks (csrc/eval_keys.hip; clipmi_version() >= 8): the positives of
 * query i are all candidates j with ckeys[j] == qkeys[i] (int64 [M] / [N], both non-null, compared as full 64-bit
 * values), the keys of the multi-positive contrastive head.  exclude (int64 [N] or NULL): candidate exclude[i] is
 * neither a positive nor a negative nor a top1 of query i (the query itself when both sides are one set); a
 * value outside [0, M) excludes nothing, as in clipmi_topk_merge.  S, lds, N, M, the block ranges, `first`, the
 * output indexing, the stream rule and the load paths are those of clipmi_rank_count.
 *   group_pick   over the block's positives, (pos_score[i], pos_idx[i]) = the best positive so far (highest score,
 *                lowest candidate index on equal scores) and n_pos[i] = the number of positives so far; a row with
 *                none yet holds pos_idx -1, pos_score -inf, n_pos 0.
 *   group_count  after group_pick has seen every column block of the row range: greater[i] / equal[i] (+)=
 *                #{ j in the block, not excluded, ckeys[j] != qkeys[i] : S[i, j] > / == pos_score[i] }, and
 *                (top1[i], top1_score[i]) = the row maximum over the non-excluded candidates so far, lowest index
 *                on ties (with exclude == NULL exactly clipmi_rank_count's).  A row with n_pos[i] == 0 gets
 *                greater = equal = -1 on `first` and keeps them; its top1 is still maintained.
 * Both passes need the SAME clipmi_gemm call per block, as rank_pick / rank_count: pos_score is a copy of an
 * element of the block the counts compare against, so a negative that duplicates the best positive counts in
 * `equal`, never in `greater`. */
int clipmi_group_pick(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols,
                      const int64_t* qkeys, const int64_t* ckeys, const int64_t* exclude, int first,
                      float* pos_score, int* pos_idx, int* n_pos);
int clipmi_group_count(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols,
                       const int64_t* qkeys, const int64_t* ckeys, const int64_t* exclude, const float* pos_score,
                       const int* n_pos, int first, int* greater, int* equal, int* top1, float* top1_score);
/* Relevance of the lists clipmi_topk_merge wrote: hits[i][r] (int32 [N, k]) = #{ r' <= r : top_idx[i][r'] in
 * [0, M) and ckeys[top_idx[i][r']] == qkeys[i] }, the inclusive prefix count behind precision@k and average
 * precision.  An empty slot (-1) or an index >= M is no hit and is never used to read ckeys.
 * 1 <= k <= CLIPMI_TOPK_MAX. */
int clipmi_topk_hits(void* stream, const int* top_idx, int N, int k, int M, const int64_t* qkeys,
                     const int64_t* ckeys, int* hits);
/* One batch of the reference's classification loops (evaluation.py:43-54, utils.py:48-61): pred[b] = argmax_c
 * probs[b, c] (lowest index on ties), conf[b] its probability (torch.max(probs, 1)), and
 * confusion[labels[b] * C + pred[b]] += 1 (int64 [C, C], rows = true class as sklearn's confusion_matrix;
 * integer atomics, summed per workgroup first, so the result does not depend on the order).  A label outside
 * [0, C) sets *bad = 1 and is not counted.  probs [B, C] fp32 contiguous, labels int64 [B]. */
int clipmi_classify_accumulate(void* stream, const float* probs, const int64_t* labels, int B, int C, int* pred,
                               float* conf, int64_t* confusion, int* bad);
/* Multi-label metrics (csrc/eval_multilabel.hip; clipmi_version() >= 14).
 * clipmi_ap_count: the integer counts behind average precision.  All four arrays are CLASS-MAJOR with one leading
 * dimension ld >= N: element (sample i, class c) is at [c * ld + i] (scores fp32, targets uint8 0 / 1, ge_all and
 * ge_pos int32).  For every class c and every positive i (target 1), with s the class's scores:
 *   ge_all[i] = #{j : s[j] >= s[i]},   ge_pos[i] = #{j : target[j] == 1 and s[j] >= s[i]}     (both count i itself)
 * entries of non-positives are written as 0, elements i >= N of a row are not touched, n_pos[c] (int32 [C]) = the
 * number of positives.  Then AP_c = (1 / n_pos[c]) sum_{i positive} ge_pos[i] / ge_all[i] is exactly
 * sklearn.metrics.average_precision_score, ties included.  A NaN score or a target other than 0 / 1 sets *bad = 1
 * (+-inf scores are legal).  N * n_pos compares per class; integer results, independent of the launch geometry.
 * clipmi_multilabel_accumulate: pred = probs >= thr[c] (thr fp32 [C], or NULL = 0.5), probs fp32 [B, C] and
 * targets uint8 [B, C] row-major contiguous; counts[c * 4 + {0, 1, 2, 3}] += (tp, fp, fn, tn) (int64 [C, 4]) and
 * exact_rows[0] += the rows whose whole prediction vector equals the target vector (integer atomics, summed per
 * workgroup first).  A target other than 0 / 1 or a NaN probability sets *bad = 1.  C <= 1024. */
int clipmi_ap_count(void* stream, const float* scores, const uint8_t* targets, int N, int C, int64_t ld, int* ge_all,
                    int* ge_pos, int* n_pos, int* bad);
int clipmi_multilabel_accumulate(void* stream, const float* probs, const uint8_t* targets, int B, int C,
                                 const float* thr, int64_t* counts, int64_t* exact_rows, int* bad);

/* ---- Live kernel timing (bench.py roofline) --------------------------------------------------
 * While armed, every launch whose variant label is in the comma-separated list `variants`
 * (e.g. "gemm256_fwd_bias_qgelu_pre,gemm256_dgrad", "gemm256_wgrad", "attn_fwd") is bracketed by
 * hipEvents on its own stream, up to max_launches.  clipmi_prof_read (after a synchronize)
 * returns the launch count and fills per-launch milliseconds and algorithmic FLOPs;
 * clipmi_prof_read_labels gives each launch's index in the list. */
int clipmi_prof_arm(const char* variants, int max_launches);
int clipmi_prof_read_labels(int max, int* which);
int clipmi_prof_disarm(void);
/* Restrict the armed profiler to launches on one HIP stream (which may be the null stream):
 * with the towers on
 * two streams, launches on the side stream share the GPU with the other tower's kernels and
 * their event-bracketed durations are not the kernel's own. */
int clipmi_prof_stream(void* stream);
int clipmi_prof_read(int max, float* ms, double* flops);

/* ---- Data-parallel collectives over RCCL --------------------------------------------
 * One communicator per process / GPU.  Rank 0 creates the 128-byte id, the host distributes it (any channel)
 * and every rank calls clipmi_comm_init with it; librccl is opened on first use (CLIPMI_ERR_UNSUPPORTED when
 * it is absent).  All enqueue on `stream`; counts are elements.
 *   allgather_embed     global[r * count + i] = local_r[i]  (the L2-normalised [B, E] features of every rank
 *                       before the [B, Bg] similarities; model_m.py:146-171 on one device)   dtype f32 / bf16
 *   reducescatter_grad  local_r[i] = sum_s global_s[r * count + i]  (the column-direction feature gradients back
 *                       to their owners)
 *   allreduce_grads     grads[i] = sum_s grads_s[i], in place, fp32  (a bucket of the gradient arena: the
 *                       data-parallel sum of trainer.py:92's loss.backward) */
int clipmi_comm_unique_id(void* id /* 128 bytes */);
int clipmi_comm_init(void** comm, const void* id, int nranks, int rank);
int clipmi_comm_destroy(void* comm);
int clipmi_allgather_embed(void* stream, void* comm, int dtype, const void* local, void* global, int64_t count);
int clipmi_reducescatter_grad(void* stream, void* comm, int dtype, const void* global, void* local, int64_t count);
int clipmi_allreduce_grads(void* stream, void* comm, float* grads, int64_t count);
/* in-place sum over the ranks, fp32 or bf16 (the product path's optional bf16 gradient buckets: half the
   bytes per ring, ~2^-9 relative rounding of each rank's contribution) */
int clipmi_allreduce(void* stream, void* comm, int dtype, void* buf, int64_t count);

#ifdef __cplusplus
}
#endif
#endif
