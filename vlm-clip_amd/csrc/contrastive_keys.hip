// Multi-positive contrastive head: the symmetric InfoNCE of contrastive.hip with the positives of a row
// given by a 64-bit key per pair instead of the diagonal alone.
//
// Each pair p of the global batch carries key[p]; for row i (global index g = label0 + i) of either
// [B, Bg] score block the positives are P_i = { j : key[j] == key[g] } (the diagonal always is one), and
//   ce_i  = lse_i - (1/|P_i|) sum_{j in P_i} L_ij              L = exp(logit_scale) * S
//   dL_ij = g * norm * (softmax_ij - [j in P_i] / |P_i|)
// (SupCon's "L_out", Khosla et al. 2020 eq. 2, over both directions as in UniCL, Yang et al. 2022).
// d logit_scale keeps the lse-centred form of ce_bwd_kernel: sum_j dL_ij (L_ij - lse_i).
//
// With all keys distinct this is the loss of contrastive.hip BIT FOR BIT: the logits, the row maximum, the sum of
// exponentials and the lse are formed by the same operations in the same order as ce_fwd_kernel /
// ce_fwd_chunk_kernel / ce_bwd_kernel / ce_bwd_chunk_kernel; the weight is 1.f / 1 = 1.f; and the positive sum goes
// through the same per-lane accumulation and wave reduction with zeros in every other place, which is exact.  The
// compiler contracts some of those kernels' multiply-adds (the chunk kernels form s * sc - mx and s * sc - lse as one
// fma; every kernel accumulates dls with an fma), so here contraction is switched off and each fused operation is
// written out as fmaf: the rounding of every intermediate is that of the unkeyed kernel's code and does not depend on
// what else shares the loop.  (As for the unkeyed pair, a single chunk over all of Bg therefore agrees with the
// materialised kernels to rounding, not bitwise: the materialised form rounds the logit before it subtracts.)
// All arithmetic is fp32 with the accurate expf / logf, for the reason at the top of contrastive.hip.
//
// Column keys are read straight from global memory, coalesced across the lanes (8 B per logit next to the 4 B cosine;
// at Bg = 32768 the keys are 256 KiB and stay in L2); no LDS, no atomics.
#include "common.h"
#include "internal.h"

namespace {

// logits = exp(ls) * S (written to L); lse[i]; winv[i] = 1 / |P_i|; ce[i] = lse[i] - winv[i] * sum_{P_i} L[i][j]
__global__ __launch_bounds__(256) void cek_fwd_kernel(const float* S, float* L, const float* logit_scale,
                                                      const int64_t* keys_all, int B, int Bg, int label0,
                                                      float* lse_out, float* ce_out, float* winv_out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float sc = expf(*logit_scale);
  const int64_t key = keys_all[label0 + row];
  const float* s = S + (int64_t)row * Bg;
  float* l = L + (int64_t)row * Bg;
  float mx = -__builtin_huge_valf();
  float psum = 0.f;
  int cnt = 0;
  for (int j = lane; j < Bg; j += 64) {
    float v = s[j] * sc;
    l[j] = v;
    mx = fmaxf(mx, v);
    const bool pos = keys_all[j] == key;
    psum += pos ? v : 0.f;
    cnt += pos ? 1 : 0;
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < Bg; j += 64) sum += expf(l[j] - mx);
  sum = wave_sum(sum);
  psum = wave_sum(psum);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    const float lse = mx + logf(sum);
    const float w = 1.f / (float)cnt;
    lse_out[row] = lse;
    winv_out[row] = w;
    ce_out[row] = lse - w * psum;
  }
}

// dS = gout * exp(ls) * (softmax(L) - [key match] winv) * norm ; dls_row = sum_j dL_ij (L_ij - lse_i)
__global__ __launch_bounds__(256) void cek_bwd_kernel(const float* L, const float* lse, const float* winv,
                                                      const float* logit_scale, const float* gout,
                                                      const int64_t* keys_all, int B, int Bg, int label0, float norm,
                                                      float* dS, float* dls_row) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float sc = expf(*logit_scale);
  const float g = (gout ? *gout : 1.f) * norm;
  const int64_t key = keys_all[label0 + row];
  const float* l = L + (int64_t)row * Bg;
  float* d = dS + (int64_t)row * Bg;
  const float ls = lse[row];
  const float w = winv[row];
  float acc = 0.f;
  for (int j = lane; j < Bg; j += 64) {
    const float x = l[j] - ls;
    const float dl = g * (expf(x) - (keys_all[j] == key ? w : 0.f));
    acc = fmaf(x, dl, acc);
    d[j] = dl * sc;
  }
  acc = wave_sum(acc);
  if (lane == 0) dls_row[row] = acc;
}

// Column-streamed form: the running state per row is run[row] = (max, sum of exponentials, positive-logit sum,
// positive count); the positive sum is a sum of logits and needs no rescaling when the maximum moves, and a chunk
// without a positive of the row adds 0.f and 0 to the last two.  The count is kept as an integer's bit pattern.
__global__ __launch_bounds__(256) void cek_fwd_chunk_kernel(const float* S, const float* logit_scale,
                                                            const int64_t* keys_all, int B, int C, int col0,
                                                            int label0, float* run) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float sc = expf(*logit_scale);
  const int64_t key = keys_all[label0 + row];
  const int64_t* kc = keys_all + col0;
  const float* s = S + (int64_t)row * C;
  float mx = -__builtin_huge_valf();
  float psum = 0.f;
  int cnt = 0;
  for (int j = lane; j < C; j += 64) {
    const float v = s[j] * sc;
    mx = fmaxf(mx, v);
    const bool pos = kc[j] == key;
    psum += pos ? v : 0.f;
    cnt += pos ? 1 : 0;
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int j = lane; j < C; j += 64) sum += expf(fmaf(s[j], sc, -mx));
  sum = wave_sum(sum);
  psum = wave_sum(psum);
  cnt = wave_sum(cnt);
  if (lane == 0) {
    float* r = run + 4 * (int64_t)row;
    if (col0 == 0) {
      r[0] = mx;
      r[1] = sum;
      r[2] = psum;
      r[3] = __int_as_float(cnt);
    } else {
      const float m = fmaxf(r[0], mx);
      r[1] = fmaf(r[1], expf(r[0] - m), sum * expf(mx - m));
      r[0] = m;
      r[2] = r[2] + psum;
      r[3] = __int_as_float(__float_as_int(r[3]) + cnt);
    }
  }
}

__global__ __launch_bounds__(256) void cek_finish_kernel(const float* run, int B, float* lse_out, float* ce_out,
                                                         float* winv_out) {
#pragma clang fp contract(off)
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  const float* r = run + 4 * (int64_t)row;
  const float lse = r[0] + logf(r[1]);
  const float w = 1.f / (float)__float_as_int(r[3]);
  lse_out[row] = lse;
  winv_out[row] = w;
  ce_out[row] = lse - w * r[2];
}

// one chunk of cek_bwd_kernel from the cosines: dS[:, 0:C) of columns col0.., dls_row (+)= its share
__global__ __launch_bounds__(256) void cek_bwd_chunk_kernel(const float* S, const float* lse, const float* winv,
                                                            const float* logit_scale, const float* gout,
                                                            const int64_t* keys_all, int B, int C, int col0,
                                                            int label0, float norm, float* dS, float* dls_row,
                                                            int beta) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= B) return;
  const float sc = expf(*logit_scale);
  const float g = (gout ? *gout : 1.f) * norm;
  const int64_t key = keys_all[label0 + row];
  const int64_t* kc = keys_all + col0;
  const float* s = S + (int64_t)row * C;
  float* d = dS + (int64_t)row * C;
  const float ls = lse[row];
  const float w = winv[row];
  float acc = 0.f;
  for (int j = lane; j < C; j += 64) {
    const float x = fmaf(s[j], sc, -ls);
    const float dl = g * (expf(x) - (kc[j] == key ? w : 0.f));
    acc = fmaf(x, dl, acc);
    d[j] = dl * sc;
  }
  acc = wave_sum(acc);
  if (lane == 0) dls_row[row] = beta ? dls_row[row] + acc : acc;
}

// out[r] = FNV-1a (64 bit) over the row's N tokens, each taken as one uint64
__global__ __launch_bounds__(256) void row_hash64_kernel(const int64_t* ids, int B, int N, int64_t* out) {
  const int row = blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= B) return;
  const int64_t* p = ids + (int64_t)row * N;
  uint64_t h = 0xcbf29ce484222325ull;
  for (int k = 0; k < N; ++k) h = (h ^ (uint64_t)p[k]) * 0x100000001b3ull;
  out[row] = (int64_t)h;
}

}  // namespace

extern "C" int clipmi_contrastive_keyed_fwd(void* stream, const float* S, float* logits, const float* logit_scale,
                                            const int64_t* keys_all, int B, int Bg, int label0, float* lse, float* ce,
                                            float* winv) {
  CLIPMI_REQUIRE(keys_all != nullptr, "keys_all is null");
  CLIPMI_REQUIRE(B >= 0 && label0 >= 0 && (int64_t)label0 + B <= Bg, "label offset out of range");
  if (B == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(cek_fwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, logits, logit_scale,
                     keys_all, B, Bg, label0, lse, ce, winv);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_contrastive_keyed_bwd(void* stream, const float* logits, const float* lse, const float* winv,
                                            const float* logit_scale, const float* grad_out, const int64_t* keys_all,
                                            int B, int Bg, int label0, float norm, float* dS, float* dls_row) {
  CLIPMI_REQUIRE(keys_all != nullptr, "keys_all is null");
  CLIPMI_REQUIRE(B >= 0 && label0 >= 0 && (int64_t)label0 + B <= Bg, "label offset out of range");
  if (B == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(cek_bwd_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, lse, winv,
                     logit_scale, grad_out, keys_all, B, Bg, label0, norm, dS, dls_row);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_contrastive_keyed_fwd_chunk(void* stream, const float* S, const float* logit_scale,
                                                  const int64_t* keys_all, int B, int C, int col0, int Bg, int label0,
                                                  float* run) {
  CLIPMI_REQUIRE(keys_all != nullptr, "keys_all is null");
  CLIPMI_REQUIRE(B >= 0 && label0 >= 0 && (int64_t)label0 + B <= Bg, "label offset out of range");
  CLIPMI_REQUIRE(C > 0 && col0 >= 0 && (int64_t)col0 + C <= Bg, "chunk out of range");
  if (B == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(cek_fwd_chunk_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, logit_scale,
                     keys_all, B, C, col0, label0, run);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_contrastive_keyed_finish(void* stream, const float* run, int B, float* lse, float* ce,
                                               float* winv) {
  if (B <= 0) return CLIPMI_OK;
  hipLaunchKernelGGL(cek_finish_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, run, B, lse, ce,
                     winv);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_contrastive_keyed_bwd_chunk(void* stream, const float* S, const float* lse, const float* winv,
                                                  const float* logit_scale, const float* grad_out,
                                                  const int64_t* keys_all, int B, int C, int col0, int Bg, int label0,
                                                  float norm, float* dS, float* dls_row, int beta) {
  CLIPMI_REQUIRE(keys_all != nullptr, "keys_all is null");
  CLIPMI_REQUIRE(B >= 0 && label0 >= 0 && (int64_t)label0 + B <= Bg, "label offset out of range");
  CLIPMI_REQUIRE(C > 0 && col0 >= 0 && (int64_t)col0 + C <= Bg, "chunk out of range");
  if (B == 0) return CLIPMI_OK;
  hipLaunchKernelGGL(cek_bwd_chunk_kernel, dim3((B + 3) / 4), dim3(256), 0, (hipStream_t)stream, S, lse, winv,
                     logit_scale, grad_out, keys_all, B, C, col0, label0, norm, dS, dls_row, beta);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_row_hash64(void* stream, const int64_t* ids, int B, int N, int64_t* out) {
  CLIPMI_REQUIRE(B >= 0 && N >= 0, "negative shape");
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(ids != nullptr && out != nullptr, "ids / out is null");
  hipLaunchKernelGGL(row_hash64_kernel, dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)stream, ids, B, N, out);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
