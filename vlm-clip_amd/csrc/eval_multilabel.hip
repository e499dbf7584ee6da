// Multi-label evaluation: the integer counts behind average precision, and thresholded per-class tallies.
//
// clipmi_ap_count.  For class c and every positive sample i (target 1):
//   ge_all[i] = #{j : s[j] >= s[i]},  ge_pos[i] = #{j : target[j] == 1 and s[j] >= s[i]}   (both include i)
// and AP_c = (1 / n_pos) sum_{i positive} ge_pos[i] / ge_all[i] is sklearn's average_precision_score, ties
// included: one threshold per distinct score, precision at a threshold counts every sample at or above it, and
// each positive contributes 1 / n_pos of recall at its own score's threshold.  The counts are integers, so the
// result does not depend on the launch geometry; the float64 sum is the host's.
//
// Layout: CLASS-MAJOR.  scores[c * ld + i], targets[c * ld + i] and the outputs ge_all / ge_pos[c * ld + i], with
// ld >= N the distance between two classes' rows (one value for all four arrays), so that lanes read consecutive
// samples of one class.  n_pos is [C].
//
// Tiles (the two sizes a test must straddle):
//   AP_ROWS = 1024  samples of one class per workgroup on the i side.  The workgroup scans them once, checks them
//                   (NaN score, target not 0 / 1 -> *bad), writes the zeros of the non-positives and compacts the
//                   positives' indices into LDS with wave ballots: EMOTIC rows carry about two labels of 26, so
//                   only about one sample in thirteen needs counts, and after compaction every lane has one.
//   AP_COLS = 2048  samples of the class staged in LDS per step on the j side, as two fp32 arrays: the score, and
//                   the score where the target is 1 / NaN where it is not (NaN >= x is false, and a NaN score is
//                   an input error anyway), so ge_pos is the same compare on the second array.  Lanes read them as
//                   16-byte broadcasts (every lane the same address): four j per read.
// Grid (ceil(N / AP_ROWS), C), 256 threads, one positive i per lane per pass; a workgroup with more than 256
// positives (a dense class) takes further passes over the j tiles.  Work is n_pos * N compares per class.
//
// clipmi_multilabel_accumulate.  pred = probs >= thr (0.5 without thr); counts[c] = (tp, fp, fn, tn) and the
// number of rows predicted exactly: one wave per row, lanes over classes, tallies in an LDS table per workgroup
// and one global integer atomic per non-zero cell, as clipmi_classify_accumulate.
#include <algorithm>
#include "common.h"
#include "internal.h"

namespace {

constexpr int AT = 256;        // threads per workgroup
constexpr int AP_ROWS = 1024;  // i side: samples scanned (and positives held) per workgroup
constexpr int AP_COLS = 2048;  // j side: samples staged in LDS per step
constexpr int ML_MAXC = 1024;  // classes of the tally table

__global__ __launch_bounds__(AT) void ap_count_kernel(const float* scores, const uint8_t* targets, int N, int64_t ld,
                                                     int* ge_all, int* ge_pos, int* n_pos, int* bad) {
  __shared__ __attribute__((aligned(16))) float sall[AP_COLS];
  __shared__ __attribute__((aligned(16))) float spos[AP_COLS];
  __shared__ int plist[AP_ROWS];
  __shared__ int wcnt[AT / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int c = blockIdx.y;
  const int64_t i0 = (int64_t)blockIdx.x * AP_ROWS;
  const float* s = scores + (int64_t)c * ld;
  const uint8_t* tg = targets + (int64_t)c * ld;
  int* ga = ge_all + (int64_t)c * ld;
  int* gp = ge_pos + (int64_t)c * ld;
  const float nan = __builtin_nanf("");

  // scan this workgroup's samples: check, zero the non-positives, compact the positives
  int np = 0;  // uniform
  bool flag = false;
  for (int k = 0; k < AP_ROWS; k += AT) {
    const int64_t i = i0 + k + t;
    const bool valid = i < N;
    const int tv = valid ? tg[i] : 0;
    const float sv = valid ? s[i] : 0.f;
    flag |= valid && (tv > 1 || sv != sv);
    const bool pos = valid && tv == 1;
    if (valid && !pos) { ga[i] = 0; gp[i] = 0; }
    const unsigned long long m = __ballot(pos);
    const int before = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) wcnt[w] = __popcll(m);
    __syncthreads();
    int base = np, total = 0;
    for (int q = 0; q < AT / 64; ++q) {
      if (q < w) base += wcnt[q];
      total += wcnt[q];
    }
    if (pos) plist[base + before] = (int)i;  // base + before < np + total <= AP_ROWS
    np += total;
    __syncthreads();
  }
  if (flag) *bad = 1;
  if (t == 0 && np) atomicAdd(&n_pos[c], np);

  for (int g = 0; g < np; g += AT) {
    const int p = g + t;
    const bool active = p < np;
    const int ii = active ? plist[p] : 0;
    const float si = active ? s[ii] : nan;
    const bool wave_active = g + w * 64 < np;  // uniform over the wave
    int ca = 0, cp = 0;
    for (int j0 = 0; j0 < N; j0 += AP_COLS) {
      const int cols = min(AP_COLS, N - j0);
      const int cols4 = (cols + 3) & ~3;  // <= AP_COLS
      __syncthreads();  // the previous tile has been read
      for (int jj = t; jj < cols4; jj += AT) {
        float v = nan, vp = nan;
        if (jj < cols) {
          v = s[j0 + jj];
          vp = tg[j0 + jj] == 1 ? v : nan;
        }
        sall[jj] = v;
        spos[jj] = vp;
      }
      __syncthreads();
      if (wave_active) {
#pragma unroll 4
        for (int jj = 0; jj < cols4; jj += 4) {
          const f32x4 a = *(const f32x4*)(sall + jj);
          const f32x4 b = *(const f32x4*)(spos + jj);
          ca += (a[0] >= si) + (a[1] >= si) + (a[2] >= si) + (a[3] >= si);
          cp += (b[0] >= si) + (b[1] >= si) + (b[2] >= si) + (b[3] >= si);
        }
      }
    }
    if (active) { ga[ii] = ca; gp[ii] = cp; }
  }
}

// one wave per row, rows strided over the grid; hist[c * 4 + {tp, fp, fn, tn}] and hist[4 C] = exact rows
__global__ __launch_bounds__(AT) void multilabel_kernel(const float* probs, const uint8_t* targets, int B, int C,
                                                       const float* thr, unsigned long long* counts,
                                                       unsigned long long* exact_rows, int* bad) {
  __shared__ int hist[4 * ML_MAXC + 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int k = threadIdx.x; k < 4 * C + 1; k += AT) hist[k] = 0;
  __syncthreads();
  bool flag = false;
  for (int64_t row = (int64_t)blockIdx.x * (AT / 64) + w; row < B; row += (int64_t)gridDim.x * (AT / 64)) {
    const float* p = probs + row * C;
    const uint8_t* y = targets + row * C;
    bool differs = false;
    for (int c = lane; c < C; c += 64) {
      const float v = p[c];
      const int yv = y[c];
      flag |= yv > 1 || v != v;
      const bool pred = v >= (thr ? thr[c] : 0.5f);
      const bool truth = yv == 1;
      differs |= pred != truth;
      atomicAdd(&hist[c * 4 + (pred ? (truth ? 0 : 1) : (truth ? 2 : 3))], 1);
    }
    if (__ballot(differs) == 0ull && lane == 0) atomicAdd(&hist[4 * C], 1);
  }
  if (flag) *bad = 1;
  __syncthreads();
  for (int k = threadIdx.x; k < 4 * C + 1; k += AT) {
    const int n = hist[k];
    if (n) atomicAdd(k < 4 * C ? &counts[k] : exact_rows, (unsigned long long)n);
  }
}

}  // namespace

extern "C" int clipmi_ap_count(void* stream, const float* scores, const uint8_t* targets, int N, int C, int64_t ld,
                               int* ge_all, int* ge_pos, int* n_pos, int* bad) {
  CLIPMI_REQUIRE(N > 0 && C > 0, "N and C must be positive");
  CLIPMI_REQUIRE(C <= 65535, "C must be at most 65535");
  CLIPMI_REQUIRE(ld >= N, "leading dimension smaller than N (the arrays are class-major)");
  CLIPMI_REQUIRE(scores && targets, "null input");
  CLIPMI_REQUIRE(ge_all && ge_pos && n_pos && bad, "null output");
  const hipStream_t s = (hipStream_t)stream;
  CLIPMI_HIP(hipMemsetAsync(n_pos, 0, (size_t)C * sizeof(int), s));
  hipLaunchKernelGGL(ap_count_kernel, dim3((unsigned)(((int64_t)N + AP_ROWS - 1) / AP_ROWS), (unsigned)C), dim3(AT), 0,
                     s, scores, targets, N, ld, ge_all, ge_pos, n_pos, bad);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_multilabel_accumulate(void* stream, const float* probs, const uint8_t* targets, int B, int C,
                                            const float* thr, int64_t* counts, int64_t* exact_rows, int* bad) {
  CLIPMI_REQUIRE(B > 0 && C > 0, "B and C must be positive");
  CLIPMI_REQUIRE(C <= ML_MAXC, "C must be at most 1024");
  CLIPMI_REQUIRE(probs && targets, "null input");
  CLIPMI_REQUIRE(counts && exact_rows && bad, "null output");
  // enough workgroups to cover the chip, few enough that each combines many rows before its flush
  const int grid = (int)std::min<int64_t>(((int64_t)B + AT / 64 - 1) / (AT / 64), 512);
  hipLaunchKernelGGL(multilabel_kernel, dim3(grid), dim3(AT), 0, (hipStream_t)stream, probs, targets, B, C, thr,
                     (unsigned long long*)counts, (unsigned long long*)exact_rows, bad);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
