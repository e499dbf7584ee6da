// GEMM kernel selection, host only: clipmi_gemm's validation and the choice of kernel, instance and launch
// geometry as a named plan (gemm_plan.cpp).  Nothing here calls HIP or dereferences an operand; gemm.hip and
// gemm4.hip launch what the plan names and decide nothing.
#pragma once
#include <stdint.h>
#include "../../include/clipmi.h"

namespace cmg {

constexpr int E_B = CLIPMI_EPI_BIAS, E_R = CLIPMI_EPI_RESID, E_Q = CLIPMI_EPI_QGELU, E_G = CLIPMI_EPI_GELU;
constexpr int E_P = CLIPMI_EPI_STORE_PRE, E_DQ = CLIPMI_EPI_DQGELU, E_DG = CLIPMI_EPI_DGELU, E_BETA = CLIPMI_EPI_BETA;
constexpr int E_DA = CLIPMI_EPI_STORE_DACT, E_MA = CLIPMI_EPI_MUL_AUX;

// tile edges and k-steps of the kernel families (static_asserted against the kernels' constants in gemm.hip)
constexpr int PLAN_T256 = 256, PLAN_T128 = 128, PLAN_TF32 = 64, PLAN_KSTEP_BF16 = 64, PLAN_KSTEP_F32 = 16;
constexpr int PLAN_FP8_PAIR = 256;  // k per scale load of the 4-wave fp8 kernel (whole pairs only)

// Every schedule the library can launch.  name: gemm_kernel_name().
enum class GemmKernel : int {
  NONE,      // nothing to launch (M or N == 0)
  F32_SIMT,  // exact fp32, SIMT                                                   "f32"
  BF16_128,  // 128x128 register-staged; the only kernel with a runtime-flag form   "bf16_128"
  PP8,       // 256x256, 8 waves, ping-pong LDS stages                              "pp8"
  ASM8,      // 256x256, 8 waves, one group, interleaved asm DMAs (round 2's wgrad) "asm8"
  W4P,       // 256x256, 4 waves, persistent (gemm4.hip)                            "w4p"
  W4P_PF,    // the same with the L2 prefetch of the activation operand            "w4p_pf"
  FP8_8W,    // MXFP8, 8 waves                                                      "fp8_8w"
  FP8_W4P,   // MXFP8, 4 waves, persistent                                          "fp8_w4p"
#ifdef CLIPMI_GEMM_EXPERIMENTS
  // measured-and-rejected schedules and timing builds (tools/gemm_bench.py, w4_stamps.py)
  X_G256_DMA_FRONT,    // gemm256_kernel, all DMAs up front
  X_G256_DMA_BUILTIN,  // gemm256_kernel, builtin DMAs
  X_PP_V1, X_PP_V2, X_PP_V3, X_PP_V4,  // gemm_pp_kernel PPV 1-4
  X_PPS,               // persistent 8-wave
  X_HP,                // half-tile pipeline (k-major A)
  X_PP_NO_EPILOGUE,    // timing
  X_PP_DMA_BETWEEN,    // DMAs between MFMAs
  X_PP_DMA_BETWEEN_NOPRIO,
  X_PP_STORE_LDS,      // stores through LDS
  X_PP_STORE_DIRECT,   // direct stores only
  X_W4_ONE,            // 4 waves, one tile per workgroup
  X_W4_STAMP0, X_W4_STAMP1, X_W4_STAMP2, X_W4_STAMP3,  // its stamped timing builds (stamp buffer armed)
#endif
};
const char* gemm_kernel_name(GemmKernel k);

// operand layout code: 2 (A k-major) | 1 (B k-major); 3 forward, 2 dgrad, 0 wgrad
constexpr int sel_of(bool a_kmajor, bool b_kmajor) { return (a_kmajor ? 2 : 0) | (b_kmajor ? 1 : 0); }

// ---- instance lists: every (layout, output type, compile-time epilogue) a kernel family is compiled for, with
// the profiler label bench.py groups its roofline families by.  Each list is the only place its labels are
// spelled; gemm_plan.cpp reads it as a table ("is this combination specialised?"), gemm.hip / gemm4.hip expand
// it into the launch switch, so the two cannot disagree.  EPI -1: the runtime-flag instance.

// which form of the persistent 4-wave kernel a 256-tile instance also has
constexpr int W4 = 1;    // persistent
constexpr int W4PF = 2;  // persistent, with and without the L2 prefetch
constexpr int W4X3 = 3;  // persistent, for the image-output products only (clipmi_gemm_x3out; CLIPMI_GEMM_X3_W4=0: off)

// 256x256 tiles: the 8-wave kernels (PP8, ASM8, experiments) have every row; the 4-wave ones as the W4 column
// says.  SPLITK rows serve split-K slabs (fp32, no epilogue; the reduce applies alpha / beta).  The wgrad rows
// (neither operand k-major) also exist with the fused bias gradient.
//   X(a_kmajor, b_kmajor, out, EPI, SPLITK, W4 form, label)
#define CLIPMI_GEMM256_INSTANCES(X)                                                              \
  X(false, false, CLIPMI_F32, 0, true, W4, "gemm256_wgrad_splitk")                               \
  X(false, false, CLIPMI_F32, E_BETA, false, W4, "gemm256_wgrad")                                \
  /* fp32 output of a bf16 product: the fp32 residual stream, the patch embedding, bf16x3 */     \
  X(true, true, CLIPMI_F32, E_B, false, W4, "gemm256_fwd_bias_f32")                              \
  X(true, true, CLIPMI_F32, E_B | E_R, false, W4, "gemm256_fwd_bias_resid_f32")                  \
  X(true, true, CLIPMI_F32, 0, false, W4, "gemm256_fwd_f32")                                     \
  X(true, true, CLIPMI_F32, E_B | E_Q | E_DA, false, W4X3, "gemm256_fwd_bias_qgelu_dact_f32")    \
  X(true, true, CLIPMI_F32, E_B | E_Q, false, W4X3, "gemm256_fwd_bias_qgelu_f32")                \
  X(true, false, CLIPMI_F32, 0, false, W4, "gemm256_dgrad_f32")                                  \
  X(true, false, CLIPMI_F32, E_MA, false, W4X3, "gemm256_dgrad_mulaux_f32")                      \
  X(true, true, CLIPMI_BF16, E_B, false, W4PF, "gemm256_fwd_bias")                               \
  X(true, true, CLIPMI_BF16, E_B | E_R, false, W4PF, "gemm256_fwd_bias_resid")                   \
  X(true, true, CLIPMI_BF16, E_B | E_Q | E_P, false, W4PF, "gemm256_fwd_bias_qgelu_pre")         \
  X(true, true, CLIPMI_BF16, E_B | E_Q | E_DA, false, W4PF, "gemm256_fwd_bias_qgelu_dact")       \
  X(true, true, CLIPMI_BF16, E_B | E_Q, false, W4PF, "gemm256_fwd_bias_qgelu")                   \
  X(true, true, CLIPMI_BF16, 0, false, W4PF, "gemm256_fwd")                                      \
  X(true, false, CLIPMI_BF16, 0, false, W4PF, "gemm256_dgrad")                                   \
  X(true, false, CLIPMI_BF16, E_DQ, false, W4PF, "gemm256_dgrad_dqgelu")                         \
  X(true, false, CLIPMI_BF16, E_MA, false, W4PF, "gemm256_dgrad_mulaux")

// 128x128 tiles (BF16_128).  The runtime-flag rows (EPI -1) take whatever the specialised rows do not.
//   X(a_kmajor, b_kmajor, out, EPI, SPLITK, label)
#define CLIPMI_GEMM128_INSTANCES(X)                                         \
  X(false, false, CLIPMI_F32, 0, true, "gemm_wgrad_splitk")                 \
  X(true, true, CLIPMI_F32, -1, false, "gemm_generic")                      \
  X(true, true, CLIPMI_BF16, E_B, false, "gemm_fwd_bias")                   \
  X(true, true, CLIPMI_BF16, E_B | E_R, false, "gemm_fwd_bias_resid")       \
  X(true, true, CLIPMI_BF16, E_B | E_Q | E_P, false, "gemm_fwd_bias_qgelu_pre") \
  X(true, true, CLIPMI_BF16, E_B | E_Q, false, "gemm_fwd_bias_qgelu")       \
  X(true, true, CLIPMI_BF16, E_B | E_G | E_P, false, "gemm_fwd_bias_gelu_pre") \
  X(true, true, CLIPMI_BF16, E_B | E_G, false, "gemm_fwd_bias_gelu")        \
  X(true, true, CLIPMI_BF16, 0, false, "gemm_fwd")                          \
  X(true, false, CLIPMI_BF16, 0, false, "gemm_dgrad")                       \
  X(true, false, CLIPMI_BF16, E_DQ, false, "gemm_dgrad_dqgelu")             \
  X(true, false, CLIPMI_BF16, E_DG, false, "gemm_dgrad_dgelu")              \
  X(true, false, CLIPMI_BF16, E_R, false, "gemm_dgrad_resid")               \
  X(false, false, CLIPMI_F32, E_BETA, false, "gemm_wgrad")                  \
  X(true, false, CLIPMI_F32, -1, false, "gemm_generic")                     \
  X(false, true, CLIPMI_F32, -1, false, "gemm_generic")                     \
  X(false, false, CLIPMI_F32, -1, false, "gemm_generic")                    \
  X(true, true, CLIPMI_BF16, -1, false, "gemm_generic")                     \
  X(true, false, CLIPMI_BF16, -1, false, "gemm_generic")                    \
  X(false, true, CLIPMI_BF16, -1, false, "gemm_generic")                    \
  X(false, false, CLIPMI_BF16, -1, false, "gemm_generic")

// MXFP8 (both operands k-major).  Output CLIPMI_FP8: the MXFP8 output epilogue.  W4 false: FP8_8W only.
//   X(out, EPI, W4, label)
#define CLIPMI_GEMM_FP8_INSTANCES(X)                                  \
  X(CLIPMI_FP8, E_B | E_Q, true, "gemm_fp8_fwd_bias_qgelu_q8")        \
  X(CLIPMI_F32, -1, true, "gemm_fp8")                                 \
  X(CLIPMI_BF16, E_B, true, "gemm_fp8_fwd_bias")                      \
  X(CLIPMI_BF16, E_B | E_R, true, "gemm_fp8_fwd_bias_resid")          \
  X(CLIPMI_BF16, E_B | E_Q, true, "gemm_fp8_fwd_bias_qgelu")          \
  X(CLIPMI_BF16, 0, true, "gemm_fp8")                                 \
  X(CLIPMI_BF16, -1, false, "gemm_fp8_generic")

// ---- the caller's kernel override: clipmi_gemm_desc.force_small_tile and the environment, decoded by
// gemm_force() and nowhere else
struct GemmForce {
  GemmKernel kernel;  // meaningful when forced
  bool forced;        // false: the production rule chooses
  int stagger;        // PP8's first-round stagger (s_sleep count), 0 off
};

// The environment switches of the GEMM path, read by gemm_env() and nowhere else.
struct GemmEnv {
  int var, wvar, fp8_var;  // CLIPMI_GEMM_VAR / _WVAR / CLIPMI_FP8_VAR (-1 unset): read once per process
  int raster;              // CLIPMI_RASTER (< 0: the defaults): read per call (tests switch it at run time)
  bool raster_set;         // CLIPMI_RASTER present at all (any value turns the tall-wgrad default off)
  bool x3_w4;              // CLIPMI_GEMM_X3_W4 != 0: read per call
  bool stamps;             // clipmi_gemm_stamps armed (not an environment variable; per call)
};
GemmEnv gemm_env();

// force code (force_small_tile or, when that is 0, the layout's environment value) -> kernel
GemmForce gemm_force(int code, bool fp8, bool wlayout, const GemmEnv& env);

struct GemmPlan {
  GemmKernel kernel;
  bool split3;      // CLIPMI_GEMM_SPLIT3: the caller splits the operands and plans the derived bf16 product
  int sel;          // the launched instance's operand layout: 2 (A k-major) | 1 (B k-major)
  int out;          // its output type (CLIPMI_F32 for split-K slabs, CLIPMI_FP8 for the MXFP8 epilogue)
  int epi;          // its compile-time epilogue set, or -1: runtime flags
  bool specialised; // epi >= 0 (F32_SIMT: false)
  bool bias_grad;   // the fused bias gradient instance
  int splits, k_per_split;
  int tile, tiles_n, ntiles;
  int raster;       // tile-rows per raster group (0 row-major)
  int stagger;
  int vec;          // GemmP::vec / vec8: the epilogue operands' alignment classes
  int vec8;
  int reduce;       // the split-K second stage: 0 none, 1 the 16-byte form (deferrable), 2 the scalar form
  const char* label;
};

// clipmi_gemm's validation and selection (x3o: clipmi_gemm_x3out's image output, 0 off).  Reads the descriptor's
// pointers for null-ness and alignment only.  CLIPMI_OK, or CLIPMI_ERR_INVALID with clipmi_last_error() set.
int gemm_plan(const clipmi_gemm_desc* d, int x3o, const GemmEnv& env, GemmPlan* out);
// tile counts of an M x N product on `tile`-edge tiles
void gemm_plan_tiles(GemmPlan* pl, int M, int N, int tile);

}  // namespace cmg
