// Multi-label class-score head: the class scores of heads.hip with a sigmoid / binary-cross-entropy tail instead
// of the softmax / cross-entropy one (EMOTIC: 26 categories, several per person; torch's BCEWithLogitsLoss).
//
//   z[b, c]      = max over the class's descriptions of scale * img[b] . desc[j]  (+ bias[c])   class_score.h
//   probs        = sigmoid(z)
//   l[b, c]      = (1 - y) z + (1 + (pw - 1) y) (log1p(exp(-|z|)) + max(-z, 0))      torch's stable form
//   loss_rows[b] = (1 / C) sum_c l[b, c]          clipmi_row_mean of it = BCEWithLogitsLoss(reduction="mean")
//   dscore[b, c] = ((1 - y) sigmoid(z) - pw y (1 - sigmoid(z))) / C      clipmi_class_ce_bwd divides by B
//
// One workgroup of 256 threads per image row, as clipmi_class_scores: the row and its C scores live in LDS, the
// tail is one thread per class, the row's loss one fixed-order workgroup sum.  sigmoid(z) and 1 - sigmoid(z) are
// both formed from e = exp(-|z|) as 1 / (1 + e) and e / (1 + e), so neither loses digits where the other
// saturates (z = +-100 gives 0 / 1 and a finite loss).  The bias gradient is a fixed-order column sum, one
// workgroup per class: no float atomics anywhere, two runs give the same bits.
#include "common.h"
#include "internal.h"
#include "class_score.h"

namespace {

constexpr int HT = CLASS_THREADS;

__device__ __forceinline__ float block_sum(float v, float* red) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  return red[0] + red[1] + red[2] + red[3];
}

__global__ __launch_bounds__(HT) void class_bce_kernel(const float* img, int E, const float* desc, const int* off,
                                                      int C, float scale, const float* bias, const float* targets,
                                                      const float* pos_weight, float* scores, float* probs,
                                                      float* loss_rows, float* dscore, int* bad) {
  __shared__ float simg[CLASS_MAXE];
  __shared__ float sc[CLASS_MAXC];
  __shared__ float red[4];
  const int t = threadIdx.x;
  const int64_t row = blockIdx.x;
  class_max_scores(img, row, E, desc, off, C, scale, simg, sc);
  const float inv_c = 1.f / (float)C;
  float lsum = 0.f;
  bool flag = false;
  for (int c = t; c < C; c += HT) {
    const float z = bias ? sc[c] + bias[c] : sc[c];
    const float e = expf(-fabsf(z));
    const float big = 1.f / (1.f + e), small = e / (1.f + e);  // sigmoid(|z|), sigmoid(-|z|)
    const float p = z >= 0.f ? big : small, q = z >= 0.f ? small : big;  // sigmoid(z), 1 - sigmoid(z)
    if (scores) scores[row * C + c] = z;
    if (probs) probs[row * C + c] = p;
    if (targets) {
      const float y = targets[row * C + c];
      const float pw = pos_weight ? pos_weight[c] : 1.f;
      float l = 0.f, d = 0.f;
      if (y >= 0.f && y <= 1.f) {
        l = (1.f - y) * z + (1.f + (pw - 1.f) * y) * (log1pf(e) + fmaxf(-z, 0.f));
        d = ((1.f - y) * p - pw * y * q) * inv_c;
      } else {
        flag = true;  // outside [0, 1] or NaN: counted as no loss and no gradient
      }
      lsum += l;
      if (dscore) dscore[row * C + c] = d;
    }
  }
  if (flag) *bad = 1;
  if (targets && loss_rows) {
    lsum = block_sum(lsum, red);
    if (t == 0) loss_rows[row] = lsum * inv_c;
  }
}

// dbias[c] = k / B * sum_b dscore[b, c], k = gscale[0] or 1: a workgroup per class, thread t sums rows t, t + 256,
// ... in order, then the fixed tree of block_sum
__global__ __launch_bounds__(HT) void class_bias_grad_kernel(const float* dscore, int B, int C, const float* gscale,
                                                            float* dbias) {
  __shared__ float red[4];
  const int c = blockIdx.x;
  float s = 0.f;
  for (int b = threadIdx.x; b < B; b += HT) s += dscore[(int64_t)b * C + c];
  s = block_sum(s, red);
  if (threadIdx.x == 0) dbias[c] = s * ((gscale ? gscale[0] : 1.f) / (float)B);
}

}  // namespace

extern "C" int clipmi_class_bce(void* stream, const float* img, int B, int E, const float* desc, const int* off, int C,
                                float scale, const float* bias, const float* targets, const float* pos_weight,
                                float* scores, float* probs, float* loss_rows, float* dscore, int* bad) {
  CLIPMI_REQUIRE(B >= 1 && E >= 1 && E <= CLASS_MAXE && C >= 1 && C <= CLASS_MAXC,
                 "B >= 1, 1 <= E <= 1024, 1 <= C <= 1024");
  CLIPMI_REQUIRE(img && desc && off, "null input");
  CLIPMI_REQUIRE(!targets || bad, "targets need bad");
  CLIPMI_REQUIRE(targets || !pos_weight, "pos_weight needs targets");
  hipLaunchKernelGGL(class_bce_kernel, dim3(B), dim3(HT), 0, (hipStream_t)stream, img, E, desc, off, C, scale, bias,
                     targets, pos_weight, scores, probs, loss_rows, dscore, bad);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_class_bias_grad(void* stream, const float* dscore, int B, int C, const float* gscale,
                                      float* dbias) {
  CLIPMI_REQUIRE(B >= 1 && C >= 1, "B and C must be positive");
  CLIPMI_REQUIRE(dscore && dbias, "null pointer");
  hipLaunchKernelGGL(class_bias_grad_kernel, dim3(C), dim3(HT), 0, (hipStream_t)stream, dscore, B, C, gscale, dbias);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
