// clipmi_gemm's validation and kernel selection (gemm_plan.h).  Host only: no HIP call, no operand dereferenced.
#include "gemm_plan.h"

#include <stdlib.h>
#include <string>

int clipmi_invalid(const std::string& msg);  // capi.cpp

namespace cmg {
unsigned long long* gemm_stamp_buffer();  // gemm.hip: the buffer armed by clipmi_gemm_stamps

namespace {
// the messages keep the prefix they have carried since validation lived in gemm.hip's gemm_impl
#define PLAN_REQUIRE(cond, msg) \
  do { if (!(cond)) return clipmi_invalid(std::string("gemm_impl: ") + (msg)); } while (0)

struct Inst256 { bool ak, bkm; int out, epi; bool splitk; int w4; const char* label; };
struct Inst128 { bool ak, bkm; int out, epi; bool splitk; const char* label; };
struct InstFp8 { int out, epi; bool w4; const char* label; };
#define ROW256(AK, BKM, OUT, EPI, SPLITK, W4F, LABEL) {AK, BKM, OUT, EPI, SPLITK, W4F, LABEL},
#define ROW128(AK, BKM, OUT, EPI, SPLITK, LABEL) {AK, BKM, OUT, EPI, SPLITK, LABEL},
#define ROWFP8(OUT, EPI, W4F, LABEL) {OUT, EPI, W4F, LABEL},
constexpr Inst256 k256[] = {CLIPMI_GEMM256_INSTANCES(ROW256)};
constexpr Inst128 k128[] = {CLIPMI_GEMM128_INSTANCES(ROW128)};
constexpr InstFp8 kfp8[] = {CLIPMI_GEMM_FP8_INSTANCES(ROWFP8)};
#undef ROW256
#undef ROW128
#undef ROWFP8

int env_int(const char* name) {
  const char* e = getenv(name);
  return e ? atoi(e) : -1;
}

using K = GemmKernel;

// The one decode table of the bf16 force codes >= 2 (clipmi_gemm_desc.force_small_tile, CLIPMI_GEMM_VAR / _WVAR).
// Any other value, and an experiment code in a product build, is the 8-wave ping-pong kernel for every shape.
K force_code_kernel(int code) {
  switch (code) {
    case 4: return K::ASM8;
    case 28: return K::W4P;
    case 32: return K::W4P_PF;
#ifdef CLIPMI_GEMM_EXPERIMENTS
    case 2: return K::X_G256_DMA_FRONT;
    case 3: return K::X_G256_DMA_BUILTIN;
    case 5: return K::X_PP_V1;
    case 6: return K::X_PP_V2;
    case 7: return K::X_PP_V3;
    case 8: return K::X_PP_V4;
    case 10: return K::X_PPS;
    case 11: return K::X_HP;
    case 12: return K::X_PP_NO_EPILOGUE;
    case 13: return K::X_PP_DMA_BETWEEN;
    case 14: return K::X_PP_DMA_BETWEEN_NOPRIO;
    case 15: return K::X_PP_STORE_LDS;
    case 16: return K::X_PP_STORE_DIRECT;
    case 20: return K::X_W4_ONE;
    case 22: return K::X_W4_STAMP0;
    case 23: return K::X_W4_STAMP1;
    case 24: return K::X_W4_STAMP2;
    case 25: return K::X_W4_STAMP3;
#endif
    default: return K::PP8;  // 9 by convention
  }
}

// Which kernel of the 256-tile family runs instance r.  The production rule, with the measurements behind it:
//  * every weight gradient: persistent 4-wave (5-11 % over ASM8, profiles/r03_wgrad_4wave.log);
//  * K >= 1536: persistent 4-wave, whose main loop is 3-7 % faster than the ping-pong kernel's; at K = 768 / 512
//    the ping-pong kernel's 8 waves run the VALU-heavy epilogues twice as fast per SIMD (tools/w4_stamps.py,
//    profiles/r03_*), so K < 1536 stays on PP8;
//  * MUL_AUX (fc2's input gradient with the stored-derivative product, K = 768): persistent 4-wave, 1182 vs
//    1215 us (profiles/r03_gemm_dact_shapes.log);
//  * the short-K bf16 input gradients (MUL_AUX, and plain ones with K <= 768: out-proj's): 4-wave with the L2
//    prefetch of the activation operand, 1.2-1.5 % and 3-4 % over the kernel without it
//    (profiles/r04_gemm_variants.log); forward shapes and long-K products measured equal or slower with it.
// A kernel that has no such instance leaves it to PP8, which has every row.
K kernel256(const Inst256& r, const GemmForce& f, const GemmEnv& env, int flags, int Kd, int x3o, bool slabs,
            int splits, bool bias_grad) {
  const bool f32o = r.out == CLIPMI_F32, wgrad = !r.ak && !r.bkm;
  K want;
  if (f.forced) want = f.kernel;
  else if (wgrad) want = K::W4P;
  else if (!f32o && !r.bkm && (flags == E_MA || (flags == 0 && Kd <= 768))) want = K::W4P_PF;
  else want = (Kd >= 1536 || flags == E_MA) ? K::W4P : K::PP8;

  const bool has_w4 = r.w4 != W4X3 || (x3o && env.x3_w4);
  bool has_pf = r.w4 == W4PF;
#ifdef CLIPMI_GEMM_EXPERIMENTS
  has_pf = has_pf || r.splitk;  // L2 prefetch of both wgrad operands (measured 5-8 % slower on the CLIP shapes)
#endif
  const bool one_launch = !bias_grad && !slabs && splits == 1;
  switch (want) {
    case K::W4P: return has_w4 ? K::W4P : K::PP8;
    case K::W4P_PF: return has_pf ? K::W4P_PF : wgrad ? K::W4P : K::PP8;
#ifdef CLIPMI_GEMM_EXPERIMENTS
    case K::X_W4_ONE: return r.w4 == W4PF ? want : K::PP8;
    case K::X_W4_STAMP0: case K::X_W4_STAMP1: case K::X_W4_STAMP2: case K::X_W4_STAMP3:
      return r.w4 == W4PF && env.stamps ? want : K::PP8;
    case K::X_PPS: return one_launch ? want : K::PP8;
    case K::X_HP: return r.ak && one_launch ? want : K::PP8;
#endif
    default: return want;  // the 8-wave kernels
  }
}

void set_instance(GemmPlan* pl, K kernel, int sel, int out, int epi, const char* label) {
  pl->kernel = kernel;
  pl->sel = sel;
  pl->out = out;
  pl->epi = epi;
  pl->specialised = epi >= 0;
  pl->label = label;
}
}  // namespace

const char* gemm_kernel_name(GemmKernel k) {
  switch (k) {
    case K::NONE: return "none";
    case K::F32_SIMT: return "f32";
    case K::BF16_128: return "bf16_128";
    case K::PP8: return "pp8";
    case K::ASM8: return "asm8";
    case K::W4P: return "w4p";
    case K::W4P_PF: return "w4p_pf";
    case K::FP8_8W: return "fp8_8w";
    case K::FP8_W4P: return "fp8_w4p";
    default: return "experiment";
  }
}

GemmEnv gemm_env() {
  static const int var = env_int("CLIPMI_GEMM_VAR"), wvar = env_int("CLIPMI_GEMM_WVAR");
  static const int fp8_var = env_int("CLIPMI_FP8_VAR");
  GemmEnv e;
  e.var = var;
  e.wvar = wvar;
  e.fp8_var = fp8_var;
  const char* r = getenv("CLIPMI_RASTER");
  e.raster_set = r != nullptr;
  e.raster = r ? atoi(r) : -1;
  const char* x = getenv("CLIPMI_GEMM_X3_W4");
  e.x3_w4 = !(x && x[0] == '0');
  e.stamps = gemm_stamp_buffer() != nullptr;
  return e;
}

// force_small_tile:  0 the production rule (or the environment's code: CLIPMI_GEMM_VAR for the forward / dgrad
// layouts, CLIPMI_GEMM_WVAR for the wgrad layout, CLIPMI_FP8_VAR = 40 / 41 for MXFP8);  1 BF16_128;  4 ASM8;
// 9 PP8;  28 W4P;  32 W4P_PF;  1xx PP8 with first-round stagger xx;  40 FP8_8W, 41 the MXFP8 rule (MXFP8
// operands only);  2-25 otherwise: the experiment schedules of force_code_kernel().  A forced kernel applies
// where it has the instance (kernel256); below 1 and unknown codes are as documented there.
GemmForce gemm_force(int code, bool fp8, bool wlayout, const GemmEnv& env) {
  const GemmForce rule = {K::NONE, false, 0};
  if (fp8) {
    if (code == 0 && (env.fp8_var == 40 || env.fp8_var == 41)) code = env.fp8_var;
    return code == 40 ? GemmForce{K::FP8_8W, true, 0} : rule;
  }
  if (code >= 100 && code < 200) return {K::PP8, true, code % 100};
  if (code == 1) return {K::BF16_128, true, 0};
  if (code < 0) return rule;
  if (code == 0) {
    code = wlayout ? env.wvar : env.var;
    // the environment's 0: the rule for forward / dgrad, PP8 for the wgrad layout (whose rule is W4P)
    if (code < 0 || (code == 0 && !wlayout)) return rule;
  }
  return {force_code_kernel(code), true, 0};
}

void gemm_plan_tiles(GemmPlan* pl, int M, int N, int tile) {
  pl->tile = tile;
  pl->tiles_n = (N + tile - 1) / tile;
  pl->ntiles = pl->tiles_n * ((M + tile - 1) / tile);
}

int gemm_plan(const clipmi_gemm_desc* d, int x3o, const GemmEnv& env, GemmPlan* out) {
  GemmPlan pl = {};
  pl.kernel = K::NONE;
  pl.splits = 1;
  pl.label = "";
  PLAN_REQUIRE(d && d->M >= 0 && d->N >= 0 && d->K >= 0, "bad shape");
  // every operand an epilogue flag reads or writes must be given (a null one would fault the GPU)
  {
    constexpr int AUXF = CLIPMI_EPI_DQGELU | CLIPMI_EPI_DGELU | CLIPMI_EPI_STORE_PRE | CLIPMI_EPI_STORE_DACT |
                         CLIPMI_EPI_MUL_AUX;
    PLAN_REQUIRE(!(d->flags & AUXF) || (d->aux && d->ldaux >= d->N), "epilogue flags need aux (ldaux >= N)");
    PLAN_REQUIRE(!(d->flags & CLIPMI_EPI_RESID) || (d->residual && d->ldr >= d->N), "residual flag needs residual (ldr >= N)");
    PLAN_REQUIRE(!(d->flags & CLIPMI_EPI_BIAS) || d->bias, "bias flag needs bias");
    PLAN_REQUIRE(!(d->flags & CLIPMI_EPI_STORE_DACT) || (d->flags & (CLIPMI_EPI_QGELU | CLIPMI_EPI_GELU)),
                 "store_dact needs an activation flag");
    PLAN_REQUIRE((d->flags & ~(1023 | CLIPMI_GEMM_SPLIT3)) == 0, "unknown epilogue flag");
    // aux has one role per launch, and the epilogues read one input stream besides it
    constexpr int AUXR = CLIPMI_EPI_DQGELU | CLIPMI_EPI_DGELU | CLIPMI_EPI_MUL_AUX;
    constexpr int AUXW = CLIPMI_EPI_STORE_PRE | CLIPMI_EPI_STORE_DACT;
    PLAN_REQUIRE((d->flags & AUXW) != AUXW, "store_pre and store_dact both write aux");
    PLAN_REQUIRE(!((d->flags & AUXR) && (d->flags & AUXW)), "aux cannot be both read and written");
    PLAN_REQUIRE(__builtin_popcount(d->flags & AUXR) <= 1, "at most one aux-reading flag");
    PLAN_REQUIRE(!((d->flags & CLIPMI_EPI_MUL_AUX) && (d->flags & (CLIPMI_EPI_RESID | CLIPMI_EPI_BETA))),
                 "mul_aux cannot be combined with residual / beta");
  }
  if (d->flags & CLIPMI_GEMM_SPLIT3) {
    pl.split3 = true;
    *out = pl;
    return CLIPMI_OK;
  }
  const int M = d->M, N = d->N, Kd = d->K, flags = d->flags;
  auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
  pl.vec = d->ldc % 4 == 0 && d->ldr % 4 == 0 && d->ldaux % 4 == 0 && al16(d->C) && al16(d->residual) && al16(d->aux);
  pl.vec8 = d->c_dtype == CLIPMI_BF16 && N % 8 == 0 && d->ldc % 8 == 0 && d->ldr % 8 == 0 && d->ldaux % 8 == 0 &&
            al16(d->C) && al16(d->residual) && al16(d->aux) && al16(d->bias);

  if (d->ab_dtype == CLIPMI_FP8) {  // MXFP8 operands (see include/clipmi.h)
    PLAN_REQUIRE(d->a_kmajor && d->b_kmajor, "fp8: both operands k-major");
    PLAN_REQUIRE(Kd % 128 == 0 && d->lda % 16 == 0 && d->ldb % 16 == 0, "fp8: K % 128 == 0, lda/ldb % 16 == 0");
    PLAN_REQUIRE(d->a_scale && d->b_scale, "fp8: block scales required");
    PLAN_REQUIRE(al16(d->A) && al16(d->B), "fp8: A/B 16-byte aligned");
    PLAN_REQUIRE(d->c_dtype == CLIPMI_F32 || d->c_dtype == CLIPMI_BF16 || d->c_dtype == CLIPMI_FP8, "c_dtype");
    PLAN_REQUIRE(d->split_k <= 1 && !d->bias_grad, "fp8: forward GEMMs only");
    // epilogue_q8 writes each row's e4m3 bytes as 16-B stores and a row's two scale bytes as one 16-bit store
    PLAN_REQUIRE(d->c_dtype != CLIPMI_FP8 || (d->c_scale && d->ldc == N && N % 32 == 0 && al16(d->C) &&
                                              ((uintptr_t)d->c_scale & 1) == 0),
                 "fp8 output: c_scale (2-byte aligned), ldc == N, N % 32 == 0, C 16-byte aligned");
    if (M == 0 || N == 0) {
      *out = pl;
      return CLIPMI_OK;
    }
    // The persistent 4-wave kernel for every shape it covers: K in whole scale pairs, at least one full tile, and
    // for bf16 output rows its 16-byte stores can take.  (Round 4 kept the residual / activation epilogues at
    // K = 1024 on the 8-wave kernel, equal or 5 % slower here in isolation, profiles/r04_fp8_gemm.log; in config
    // 5's step the 4-wave kernel for all of them measured equal throughput and a 3.5 % shorter mean fp8 launch,
    // profiles/r05_cfg5_fp8_kernel_ab.log.)
    const GemmForce f = gemm_force(d->force_small_tile, true, false, env);
    const bool w4 = !f.forced && Kd % PLAN_FP8_PAIR == 0 && M >= PLAN_T256 && N >= PLAN_T256 &&
                    (d->c_dtype != CLIPMI_BF16 || pl.vec8);
    for (int pass = w4 ? 0 : 1; pass < 2 && pl.kernel == K::NONE; ++pass)
      for (const InstFp8& r : kfp8)
        if (r.out == d->c_dtype && (r.epi == flags || r.epi < 0) && (pass == 1 || r.w4)) {
          set_instance(&pl, pass ? K::FP8_8W : K::FP8_W4P, 3, r.out, r.epi, r.label);
          break;
        }
    if (pl.kernel == K::NONE) return clipmi_invalid("fp8 output: supported epilogue flags are bias + quick_gelu");
    pl.k_per_split = Kd;
    gemm_plan_tiles(&pl, M, N, PLAN_T256);
    // groups of 8 tile-rows (fc1 +10 %, the rest neutral: profiles/r02_raster_ab.log)
    pl.raster = env.raster >= 0 ? env.raster : 8;
    *out = pl;
    return CLIPMI_OK;
  }

  const bool bf = d->ab_dtype == CLIPMI_BF16;
  PLAN_REQUIRE(bf || d->ab_dtype == CLIPMI_F32, "ab_dtype");
  if (M == 0 || N == 0) {
    *out = pl;
    return CLIPMI_OK;
  }
  PLAN_REQUIRE(bf == false || d->b_kmajor || N % 8 == 0, "row-major B needs N % 8 == 0");
  PLAN_REQUIRE(d->c_dtype == CLIPMI_F32 || d->c_dtype == CLIPMI_BF16, "c_dtype");
  if (bf) {
    PLAN_REQUIRE(!d->a_kmajor || Kd % 8 == 0, "k-major A needs K % 8 == 0");
    PLAN_REQUIRE(!d->b_kmajor || Kd % 8 == 0, "k-major B needs K % 8 == 0");
    PLAN_REQUIRE(d->a_kmajor || M % 8 == 0, "row-major A needs M % 8 == 0");
    PLAN_REQUIRE(d->a_kmajor || M >= 8, "M >= 8");
    PLAN_REQUIRE(al16(d->A) && al16(d->B), "A/B must be 16-byte aligned");
    PLAN_REQUIRE((d->lda % 8) == 0 && (d->ldb % 8) == 0, "lda/ldb must be multiples of 8");
  }
  const bool ak = d->a_kmajor != 0, bkm = d->b_kmajor != 0, wlayout = !ak && !bkm;
  const GemmForce f = gemm_force(d->force_small_tile, false, wlayout, env);
  pl.stagger = f.stagger;
  // the 256x256 LDS-DMA kernels for the big shapes (k-major operands need K % 64 == 0: the buffer range check
  // zero-fills rows, not a row's k tail); below M 256 / N 128 the 128x128 kernel
  const bool kok = (!ak || Kd % 64 == 0) && (!bkm || Kd % 64 == 0);
  const bool use256 = bf && kok && ((M >= 256 && N >= 128) || d->bias_grad) && !(f.forced && f.kernel == K::BF16_128);
  PLAN_REQUIRE(!d->bias_grad || use256, "bias_grad fusion needs the 256 kernel (bf16, wgrad layout)");
  int splits = d->split_k > 1 ? d->split_k : 1;
  PLAN_REQUIRE(!x3o || (use256 && splits == 1), "x3out: needs the 256-tile kernels (M >= 256, N >= 128, K % 64 == 0)");
  bool slabs = false;
  if (splits > 1) {
    PLAN_REQUIRE(d->c_dtype == CLIPMI_F32, "split_k needs fp32 C");
    PLAN_REQUIRE((flags & ~CLIPMI_EPI_BETA) == 0, "split_k supports only the beta flag");
    PLAN_REQUIRE(d->workspace && d->workspace_bytes >= (int64_t)splits * M * (N + (d->bias_grad ? 1 : 0)) * 4,
                 "split_k workspace too small (split_k * M * (N + bias_grad ? 1 : 0) floats)");
    const int kstep = bf ? PLAN_KSTEP_BF16 : PLAN_KSTEP_F32;
    int per = (Kd + splits - 1) / splits;
    per = (per + kstep - 1) / kstep * kstep;
    splits = (Kd + per - 1) / per;
    pl.k_per_split = per;
    slabs = true;
    pl.reduce = (N % 4 == 0 && d->ldc % 4 == 0 && al16(d->C) && al16(d->workspace)) ? 1 : 2;
  } else {
    pl.k_per_split = Kd > 0 ? Kd : 1;
  }
  pl.splits = splits;
  pl.raster = env.raster >= 0 ? env.raster : 0;  // row-major (groups of 4/8/16 within +-3 %: profiles/r02_raster_ab.log)
  const int outc = (d->c_dtype == CLIPMI_F32 || slabs) ? CLIPMI_F32 : CLIPMI_BF16;
  const int sel = sel_of(ak, bkm);
  if (!bf) {
    set_instance(&pl, K::F32_SIMT, sel, outc, -1, "gemm_f32");
    gemm_plan_tiles(&pl, M, N, PLAN_TF32);
    *out = pl;
    return CLIPMI_OK;
  }
  const int epi = slabs ? 0 : flags;  // slabs carry no epilogue: the reduce applies alpha and beta
  if (use256) {
    const Inst256* r = nullptr;
    if (!d->bias_grad || wlayout)
      for (const Inst256& c : k256)
        if (sel_of(c.ak, c.bkm) == sel && c.out == outc && c.epi == epi && c.splitk == slabs) r = &c;
    PLAN_REQUIRE(r || !x3o, "x3out: no image-output kernel for these flags");
    if (r) {
      set_instance(&pl, kernel256(*r, f, env, flags, Kd, x3o, slabs, splits, d->bias_grad != nullptr), sel, outc, epi,
                   r->label);
      pl.bias_grad = d->bias_grad != nullptr;
      gemm_plan_tiles(&pl, M, N, PLAN_T256);
      // weight gradients with more column than row tiles (fc2: M = 768, N = 3072) walk each k-slab's tiles
      // column-major, so the ~32 items an XCD holds at once share the few row panels instead of spanning every
      // column panel (L2 fetch modelled 1.66x -> 1.25x of the compulsory panels, tools/gemm_l2_model.py);
      // CLIPMI_RASTER overrides
      const int tiles_m = pl.ntiles / pl.tiles_n;
      if (wlayout && !env.raster_set && pl.tiles_n > tiles_m) pl.raster = tiles_m;
      *out = pl;
      return CLIPMI_OK;
    }
  }
  // the 128x128 kernel: a specialised instance, else the runtime-flag one
  PLAN_REQUIRE(!d->bias_grad, "bias_grad needs the wgrad layout (both operands row-major in k)");
  const Inst128* r = nullptr;
  for (const Inst128& c : k128)
    if (!r && c.epi >= 0 && sel_of(c.ak, c.bkm) == sel && c.out == outc && c.epi == epi && c.splitk == slabs) r = &c;
  // slabs of another layout have always gone to the k-major runtime-flag instance
  const int gsel = (slabs && sel != 0) ? 3 : sel;
  for (const Inst128& c : k128)
    if (!r && c.epi < 0 && sel_of(c.ak, c.bkm) == gsel && c.out == outc) r = &c;
  set_instance(&pl, K::BF16_128, sel_of(r->ak, r->bkm), outc, r->epi, r->label);
  gemm_plan_tiles(&pl, M, N, PLAN_T128);
  *out = pl;
  return CLIPMI_OK;
}

}  // namespace cmg
