// Single-query attention: the CLS query of each sequence against all N keys / values (head dim 64, no mask).
//
// The vision tower's last encoder layer under CLS pooling (model_m.py:122): only row 0 of that layer's output is
// read, so its attention ([HF] modeling_clip.py:298-335) has one query per (sequence, head).  Entry points for hosts
// that pool one row; the encoder engine's cls_last mode does not call them (it keeps the MFMA attention kernels, whose
// bf16 rounding of the probabilities these fp32 kernels do not reproduce, so that a step computes the full mode's bits).
// Per (b, h), scale = 1/8:  s_j = scale q.k_j,  p = softmax(s),  o = sum_j p_j v_j,  lse = log sum_j e^{s_j};
// backward with p recomputed from lse:  delta = dO.o,  dS_j = p_j (dO.v_j - delta),  dq = scale sum_j dS_j k_j,
// dK_j = scale dS_j q,  dV_j = p_j dO.  Scores, probabilities and every sum are fp32; outputs are rounded once.
//
// Pure HBM traffic (the forward reads K|V once, the backward reads K|V and writes dK|dV once), no MFMA.  One
// workgroup per sequence (and per group of 256 / LPH heads when a row has more): a lane owns one 16-byte piece of
// a head (LPH = 8 lanes per head in bf16, 16 in fp32), the lanes of a row slot cover the K half and the V half of a
// K|V row as whole contiguous runs, and 256 / (heads * LPH) row slots walk the sequence.  A head's dot products
// are summed over its LPH lanes by shuffles; the row slots' partial (max, sum, o) or dq are merged through LDS in
// slot order, so a replay is bitwise equal (no atomics).
#include "common.h"
#include "internal.h"

namespace {

template <typename T> struct V16;
template <> struct V16<bf16> { typedef bf16x8 type; static constexpr int N = 8; };
template <> struct V16<float> { typedef f32x4 type; static constexpr int N = 4; };

template <typename T>
__device__ __forceinline__ void ld16(const T* p, float* o) {
  const typename V16<T>::type v = *(const typename V16<T>::type*)p;
#pragma unroll
  for (int j = 0; j < V16<T>::N; ++j) o[j] = (float)v[j];
}
template <typename T>
__device__ __forceinline__ void st16(T* p, const float* o) {
  typename V16<T>::type v;
#pragma unroll
  for (int j = 0; j < V16<T>::N; ++j) v[j] = (T)o[j];
  *(typename V16<T>::type*)p = v;
}
// sum += x with the running compensation c (Kahan); no reassociation: the build has no fast-math
__device__ __forceinline__ void kahan_add(float& sum, float& c, float x) {
  const float y = x - c;
  const float t = sum + y;
  c = (t - sum) - y;
  sum = t;
}
// sum over the LPH consecutive lanes of a head (LPH divides 64 and the groups are LPH-aligned in the block)
template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
  for (int o = LPH / 2; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

constexpr int CLS_THREADS = 256;
constexpr int CLS_ROWS = 4;  // K|V rows a lane loads before the first use (bytes in flight)

// the block's geometry: heads [h0, h0 + nh), cpr lanes per row, rif row slots; this lane's slot r and column col
struct ClsGeo {
  int b, h0, cpr, rif, r, c, col;
  bool active;
};
template <int LPH, int VEC>
__device__ __forceinline__ ClsGeo cls_geo(int H, int hpb) {
  ClsGeo g;
  g.b = blockIdx.x;
  g.h0 = blockIdx.y * hpb;
  const int nh = min(hpb, H - g.h0);
  g.cpr = nh * LPH;
  g.rif = CLS_THREADS / g.cpr;
  g.r = threadIdx.x / g.cpr;
  g.c = threadIdx.x - g.r * g.cpr;
  g.active = g.r < g.rif;
  if (!g.active) { g.r = 0; }  // idle lanes shadow slot 0 (loads only, nothing stored)
  g.col = g.h0 * 64 + g.c * VEC;
  return g;
}

// q [B][ldq], kv [B*N][2D] (K | V), o [B][ldo], lse [B][H]
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void attn_cls_fwd_kernel(const T* q, int64_t ldq, const T* kv, T* o,
                                                                   int64_t ldo, float* lse, int H, int N, int D,
                                                                   int hpb) {
  constexpr int VEC = V16<T>::N, LPH = 64 / VEC;
  __shared__ float part[CLS_THREADS][VEC + 2];
  const ClsGeo g = cls_geo<LPH, VEC>(H, hpb);
  float qs[VEC];
  ld16<T>(q + (int64_t)g.b * ldq + g.col, qs);
#pragma unroll
  for (int i = 0; i < VEC; ++i) qs[i] *= 0.125f;
  const T* base = kv + (int64_t)g.b * N * 2 * D + g.col;
  // l and acc are compensated (Kahan) sums: a slot adds up to N / rif terms in sequence, and at N = 4096 a plain
  // fp32 chain leaves ~1e-7 on a mean of values of size 1 (the structured tests hold fp32 O to 2^-21 |o| + 2.8e-8)
  float m = -INFINITY, l = 0.f, lc = 0.f, acc[VEC], cmp[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) acc[i] = cmp[i] = 0.f;
  for (int j0 = g.r; j0 < N; j0 += CLS_ROWS * g.rif) {
    float kf[CLS_ROWS][VEC], vf[CLS_ROWS][VEC];
#pragma unroll
    for (int u = 0; u < CLS_ROWS; ++u) {
      const int j = min(j0 + u * g.rif, N - 1);  // a clamped duplicate row is computed, not accumulated
      ld16<T>(base + (int64_t)j * 2 * D, kf[u]);
      ld16<T>(base + (int64_t)j * 2 * D + D, vf[u]);
    }
#pragma unroll
    for (int u = 0; u < CLS_ROWS; ++u) {
      float dot = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) dot += qs[i] * kf[u][i];
      const float s = head_sum<LPH>(dot);
      if (j0 + u * g.rif < N) {
        const float mn = fmaxf(m, s);
        const float a = expf(m - mn), p = expf(s - mn);
        l = l * a;
        lc = lc * a;
        kahan_add(l, lc, p);
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          acc[i] *= a;
          cmp[i] *= a;
          kahan_add(acc[i], cmp[i], p * vf[u][i]);
        }
        m = mn;
      }
    }
  }
  part[threadIdx.x][0] = m;
  part[threadIdx.x][1] = l;
#pragma unroll
  for (int i = 0; i < VEC; ++i) part[threadIdx.x][2 + i] = acc[i];
  __syncthreads();
  if (!g.active || g.r != 0) return;
  float M = -INFINITY;
  for (int rr = 0; rr < g.rif; ++rr) M = fmaxf(M, part[rr * g.cpr + g.c][0]);
  float L = 0.f, out[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) out[i] = 0.f;
  for (int rr = 0; rr < g.rif; ++rr) {  // slot order: deterministic (a slot without rows has m = -inf, l = 0)
    const float* pr = part[rr * g.cpr + g.c];
    const float a = expf(pr[0] - M);
    L += pr[1] * a;
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] += pr[2 + i] * a;
  }
  const float inv = 1.0f / L;
#pragma unroll
  for (int i = 0; i < VEC; ++i) out[i] *= inv;
  st16<T>(o + (int64_t)g.b * ldo + g.col, out);
  if (g.c % LPH == 0) lse[(int64_t)g.b * H + g.h0 + g.c / LPH] = M + logf(L);
}

// dout [B][lddo]; dkv [B*N][2D] (dK | dV); dq [B][lddq]; dkv0 (may be NULL) [B][ld0]: a second copy of row 0's
// dK | dV at columns [0, D) | [D, 2D)
template <typename T>
__global__ __launch_bounds__(CLS_THREADS) void attn_cls_bwd_kernel(const T* q, int64_t ldq, const T* kv, const T* o,
                                                                   int64_t ldo, const float* lse, const T* dout,
                                                                   int64_t lddo, T* dkv, T* dq, int64_t lddq, T* dkv0,
                                                                   int64_t ld0, int H, int N, int D, int hpb) {
  constexpr int VEC = V16<T>::N, LPH = 64 / VEC;
  __shared__ float part[CLS_THREADS][VEC];
  const ClsGeo g = cls_geo<LPH, VEC>(H, hpb);
  float qs[VEC], dov[VEC], ov[VEC];
  ld16<T>(q + (int64_t)g.b * ldq + g.col, qs);
  ld16<T>(dout + (int64_t)g.b * lddo + g.col, dov);
  ld16<T>(o + (int64_t)g.b * ldo + g.col, ov);
  float dd = 0.f;
#pragma unroll
  for (int i = 0; i < VEC; ++i) {
    qs[i] *= 0.125f;
    dd += dov[i] * ov[i];
  }
  const float delta = head_sum<LPH>(dd);
  const float L = lse[(int64_t)g.b * H + g.h0 + g.c / LPH];
  const int64_t row0 = (int64_t)g.b * N * 2 * D + g.col;
  float dqa[VEC], dqc[VEC];  // compensated, as the forward's sums
#pragma unroll
  for (int i = 0; i < VEC; ++i) dqa[i] = dqc[i] = 0.f;
  for (int j0 = g.r; j0 < N; j0 += CLS_ROWS * g.rif) {
    float kf[CLS_ROWS][VEC], vf[CLS_ROWS][VEC];
#pragma unroll
    for (int u = 0; u < CLS_ROWS; ++u) {
      const int j = min(j0 + u * g.rif, N - 1);
      ld16<T>(kv + row0 + (int64_t)j * 2 * D, kf[u]);
      ld16<T>(kv + row0 + (int64_t)j * 2 * D + D, vf[u]);
    }
#pragma unroll
    for (int u = 0; u < CLS_ROWS; ++u) {
      float dot = 0.f, dv = 0.f;
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        dot += qs[i] * kf[u][i];
        dv += dov[i] * vf[u][i];
      }
      const float s = head_sum<LPH>(dot);
      const float dpv = head_sum<LPH>(dv);
      const int j = j0 + u * g.rif;
      if (j < N && g.active) {
        const float p = expf(s - L);
        const float ds = p * (dpv - delta);
        float dk[VEC], dvv[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i) {
          kahan_add(dqa[i], dqc[i], ds * kf[u][i]);
          dk[i] = ds * qs[i];
          dvv[i] = p * dov[i];
        }
        st16<T>(dkv + row0 + (int64_t)j * 2 * D, dk);
        st16<T>(dkv + row0 + (int64_t)j * 2 * D + D, dvv);
        if (j == 0 && dkv0) {
          st16<T>(dkv0 + (int64_t)g.b * ld0 + g.col, dk);
          st16<T>(dkv0 + (int64_t)g.b * ld0 + D + g.col, dvv);
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < VEC; ++i) part[threadIdx.x][i] = dqa[i];
  __syncthreads();
  if (!g.active || g.r != 0) return;
  float out[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) out[i] = 0.f;
  for (int rr = 0; rr < g.rif; ++rr)  // slot order: deterministic
#pragma unroll
    for (int i = 0; i < VEC; ++i) out[i] += part[rr * g.cpr + g.c][i];
#pragma unroll
  for (int i = 0; i < VEC; ++i) out[i] *= 0.125f;
  st16<T>(dq + (int64_t)g.b * lddq + g.col, out);
}

bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

static int cls_check(const char* who, int dtype, int B, int H, int N, int D) {
  if (dtype != CLIPMI_BF16 && dtype != CLIPMI_F32) return clipmi_invalid(std::string(who) + ": dtype (bf16 or fp32)");
  if (B < 0 || H < 1 || D != H * 64) return clipmi_invalid(std::string(who) + ": B >= 0, H >= 1, D == 64 * H (head dim 64)");
  if (N < 1 || N > 4096) return clipmi_invalid(std::string(who) + ": 1 <= N <= 4096");
  return CLIPMI_OK;
}

extern "C" int clipmi_attention_cls_fwd(void* stream, int dtype, const void* q, int64_t ldq, const void* kv, void* o,
                                        int64_t ldo, float* lse, int B, int H, int N, int D) {
  CLIPMI_TRY(cls_check("attention_cls_fwd", dtype, B, H, N, D));
  CLIPMI_REQUIRE(q && kv && o && lse, "null pointer");
  const int vec = dtype == CLIPMI_BF16 ? 8 : 4;
  CLIPMI_REQUIRE(ldq >= D && ldo >= D && ldq % vec == 0 && ldo % vec == 0 && al16(q) && al16(kv) && al16(o),
                 "q / kv / o 16-byte aligned, ldq / ldo >= D and multiples of 16 bytes");
  if (B == 0) return CLIPMI_OK;
  hipStream_t s = (hipStream_t)stream;
  const int hpb = std::min(H, CLS_THREADS / (64 / vec));
  const dim3 grid(B, (H + hpb - 1) / hpb);
  ProfScope ps(s, "attn_cls_fwd", 4.0 * B * N * D);
  if (dtype == CLIPMI_BF16)
    hipLaunchKernelGGL(attn_cls_fwd_kernel<bf16>, grid, dim3(CLS_THREADS), 0, s, (const bf16*)q, ldq, (const bf16*)kv,
                       (bf16*)o, ldo, lse, H, N, D, hpb);
  else
    hipLaunchKernelGGL(attn_cls_fwd_kernel<float>, grid, dim3(CLS_THREADS), 0, s, (const float*)q, ldq, (const float*)kv,
                       (float*)o, ldo, lse, H, N, D, hpb);
  ps.finish("attn_cls_fwd", 4.0 * B * N * D);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_attention_cls_bwd(void* stream, int dtype, const void* q, int64_t ldq, const void* kv,
                                        const void* o, int64_t ldo, const float* lse, const void* dout, int64_t lddo,
                                        void* dkv, void* dq, int64_t lddq, void* dkv0, int64_t ld0, int B, int H, int N,
                                        int D) {
  CLIPMI_TRY(cls_check("attention_cls_bwd", dtype, B, H, N, D));
  CLIPMI_REQUIRE(q && kv && o && lse && dout && dkv && dq, "null pointer");
  const int vec = dtype == CLIPMI_BF16 ? 8 : 4;
  CLIPMI_REQUIRE(ldq >= D && ldo >= D && lddo >= D && lddq >= D && ldq % vec == 0 && ldo % vec == 0 &&
                     lddo % vec == 0 && lddq % vec == 0 && al16(q) && al16(kv) && al16(o) && al16(dout) && al16(dkv) &&
                     al16(dq),
                 "operands 16-byte aligned, leading dimensions >= D and multiples of 16 bytes");
  CLIPMI_REQUIRE(!dkv0 || (ld0 >= 2 * (int64_t)D && ld0 % vec == 0 && al16(dkv0)),
                 "dkv0 16-byte aligned, ld0 >= 2 D and a multiple of 16 bytes");
  if (B == 0) return CLIPMI_OK;
  hipStream_t s = (hipStream_t)stream;
  const int hpb = std::min(H, CLS_THREADS / (64 / vec));
  const dim3 grid(B, (H + hpb - 1) / hpb);
  ProfScope ps(s, "attn_cls_bwd", 8.0 * B * N * D);
  if (dtype == CLIPMI_BF16)
    hipLaunchKernelGGL(attn_cls_bwd_kernel<bf16>, grid, dim3(CLS_THREADS), 0, s, (const bf16*)q, ldq, (const bf16*)kv,
                       (const bf16*)o, ldo, lse, (const bf16*)dout, lddo, (bf16*)dkv, (bf16*)dq, lddq, (bf16*)dkv0, ld0,
                       H, N, D, hpb);
  else
    hipLaunchKernelGGL(attn_cls_bwd_kernel<float>, grid, dim3(CLS_THREADS), 0, s, (const float*)q, ldq,
                       (const float*)kv, (const float*)o, ldo, lse, (const float*)dout, lddo, (float*)dkv, (float*)dq,
                       lddq, (float*)dkv0, ld0, H, N, D, hpb);
  ps.finish("attn_cls_bwd", 8.0 * B * N * D);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
