// Pairwise sigmoid contrastive head (Zhai et al. 2023, "Sigmoid Loss for Language Image Pre-Training"):
// every (text, image) pair of the global batch is one binary problem, "same key" or "different key".
//
// A rank holds B text rows (global indices label0 .. label0 + B) and scores them against all Bg image rows:
//   l_ij = sc * s_ij + b                            sc = exp(logit_scale), b = logit_bias, s = cosine
//   z_ij = +1 if key[j] == key[label0 + i] (keys null: if j == label0 + i), else -1
//   loss = norm * sum_ij softplus(-z_ij l_ij)       norm = 1 / Bg; summed over the ranks, the global loss
//   u_ij = d loss / d l_ij = -z_ij sigmoid(-z_ij l_ij) norm
//   dS_ij = u_ij sc      d logit_scale = sum_ij u_ij sc s_ij      d logit_bias = sum_ij u_ij
// A pair's term depends on nothing but the pair: there is no row normalisation, so the gradient of a pair is known
// the moment its logit is and ONE pass over the score block gives the loss and dS.  The block may come in column
// chunks [col0, col0 + C); the only state carried between chunks is rows [B][3], the three row sums above
// (col0 == 0 initialises them).  A materialised block is the one chunk C == Bg, col0 == 0: the same kernel, so a
// single chunk over all of Bg is the materialised form bit for bit.
//
// Saturation: with x = -z l, softplus(x) = max(x, 0) + log1p(exp(-|x|)) and sigmoid(x) = (x >= 0 ? 1 : e) / (1 + e)
// with e = exp(-|x|) <= 1: no exponential of a positive argument anywhere, so logits of +-100 and beyond give finite
// losses and gradients.
//
// keys null and all-distinct keys give the same bits: the key compare only chooses the sign of x.  Contraction is
// switched off and each fused operation is written out as fmaf, so the rounding of every intermediate does not
// depend on which of the optional outputs (logits, dS) share the loop.  All arithmetic is fp32 with the accurate
// expf / log1pf, for the reason at the top of contrastive.hip.
//
// As contrastive_keys.hip: one wave per row, four rows per 256-thread block; column keys read straight from global
// memory, coalesced across the lanes; no LDS, no atomics.  dS may be S itself: a lane reads s_ij before it writes
// dS_ij and no other lane touches that element.
#include "common.h"
#include "internal.h"

namespace {

__global__ __launch_bounds__(256) void sigmoid_pairs_kernel(const float* S, const float* logit_scale,
                                                            const float* logit_bias, const int64_t* keys_all, int B,
                                                            int C, int col0, int label0, float norm, float* logits,
                                                            float* dS, float* rows) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float sc = expf(*logit_scale);
  const float b = *logit_bias;
  const int g = label0 + row;
  const int64_t key = keys_all ? keys_all[g] : 0;
  const int64_t* kc = keys_all ? keys_all + col0 : nullptr;
  const float* s = S + (int64_t)row * C;
  float* lo = logits ? logits + (int64_t)row * C : nullptr;
  float* d = dS ? dS + (int64_t)row * C : nullptr;
  float sp = 0.f, dls = 0.f, db = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float v = s[j];
    const float l = fmaf(v, sc, b);
    const bool pos = kc ? kc[j] == key : col0 + j == g;
    const float x = pos ? -l : l;  // -z l
    const float e = expf(-fabsf(x));
    sp += fmaxf(x, 0.f) + log1pf(e);
    if (lo) lo[j] = l;
    if (d) {
      const float sig = (x >= 0.f ? 1.f : e) / (1.f + e);
      const float u = (pos ? -sig : sig) * norm;
      const float ds = u * sc;
      dls = fmaf(ds, v, dls);
      db += u;
      d[j] = ds;
    }
  }
  sp = wave_sum(sp);
  if (d) {
    dls = wave_sum(dls);
    db = wave_sum(db);
  }
  if (lane == 0) {
    float* r = rows + 3 * (int64_t)row;
    r[0] = col0 == 0 ? sp : r[0] + sp;
    if (d) {
      r[1] = col0 == 0 ? dls : r[1] + dls;
      r[2] = col0 == 0 ? db : r[2] + db;
    }
  }
}

// column sums of rows [n][3] in a fixed tree: per-thread strided sums, the wave butterfly, then the 16 wave
// partials in order.  loss = norm * sum_0; dls / db = g * sum_1 / g * sum_2, set or (beta) accumulated.  With dls
// and db both null (the no-grad form) columns 1 and 2 of rows are unset and are not read.
__global__ __launch_bounds__(1024) void sigmoid_reduce_kernel(const float* rows, int n, float norm,
                                                              const float* gscale, float* loss, float* dls, float* db,
                                                              int beta) {
#pragma clang fp contract(off)
  __shared__ float red[3][16];
  const bool grads = dls != nullptr || db != nullptr;
  float a[3] = {0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < n; i += 1024) {
    const float* r = rows + 3 * (int64_t)i;
    a[0] += r[0];
    if (grads) {
      a[1] += r[1];
      a[2] += r[2];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = wave_sum(a[c]);
    if ((threadIdx.x & 63) == 0) red[c][threadIdx.x >> 6] = a[c];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float t[3] = {0.f, 0.f, 0.f};
    for (int w = 0; w < 16; ++w) {
      t[0] += red[0][w];
      t[1] += red[1][w];
      t[2] += red[2][w];
    }
    const float g = gscale ? *gscale : 1.f;
    if (loss) loss[0] = t[0] * norm;
    if (dls) dls[0] = beta ? dls[0] + t[1] * g : t[1] * g;
    if (db) db[0] = beta ? db[0] + t[2] * g : t[2] * g;
  }
}

}  // namespace

extern "C" int clipmi_sigmoid_pairs(void* stream, const float* S, const float* logit_scale, const float* logit_bias,
                                    const int64_t* keys_all, int B, int C, int col0, int Bg, int label0, float norm,
                                    float* logits, float* dS, float* rows) {
  CLIPMI_REQUIRE(logit_bias != nullptr, "logit_bias is null");
  CLIPMI_REQUIRE(rows != nullptr, "rows is null");
  CLIPMI_REQUIRE(B >= 0 && label0 >= 0 && (int64_t)label0 + B <= Bg, "label offset out of range");
  CLIPMI_REQUIRE(C > 0 && col0 >= 0 && (int64_t)col0 + C <= Bg, "chunk out of range");
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(S != nullptr && logit_scale != nullptr, "S / logit_scale is null");
  hipLaunchKernelGGL(sigmoid_pairs_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, logit_scale,
                     logit_bias, keys_all, B, C, col0, label0, norm, logits, dS, rows);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_sigmoid_reduce(void* stream, const float* rows, int n, float norm, const float* gscale,
                                     float* loss, float* dls, float* db, int beta) {
  CLIPMI_REQUIRE(rows != nullptr, "rows is null");
  CLIPMI_REQUIRE(n >= 0, "negative row count");
  CLIPMI_REQUIRE(loss != nullptr || dls != nullptr || db != nullptr, "loss, dls and db are all null");
  if (n == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(sigmoid_reduce_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, rows, n, norm, gscale, loss,
                     dls, db, beta);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
