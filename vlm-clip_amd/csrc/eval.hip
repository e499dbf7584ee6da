// On-device evaluation: retrieval ranks over streamed score blocks and classification tallies.
//
// Retrieval (recall@K / median rank of a dual encoder over a whole validation set): for query row i
// with target candidate t_i the rank of the target is 1 + #{ j != t_i : S[i, j] > S[i, t_i] }.  The
// [N, M] score matrix is never materialised: the caller walks blocks S_block = Q_block . C_block^T of the
// exact-f32 GEMM (the cosines the contrastive head trains on) in a bounded scratch, twice.  Pass 1
// (rank_pick_kernel) copies S[i, t_i] out of the block that holds it; pass 2 (rank_count_kernel) adds every
// block's share of the counts and merges the running row maximum.  The target score is compared against
// scores from the same GEMM output it was read from -- never recomputed another way -- so a duplicate of
// the target (this project's data repeats captions) lands in `equal` exactly and never in `greater`.
// Blocks of one row range are serialised on the stream and a row has one owner per launch: no atomics.
//
// Classification (the torch.max(probs, 1) + sklearn confusion_matrix of the reference's evaluate_model /
// evaluate_enhanced_model loops): row argmax with its probability and confusion[label][pred] += 1 with
// integer atomics (order-independent, so a replay is bitwise equal), combined per workgroup in LDS first.
//
// All fp32 / int32 / int64, no allocation, no synchronisation; an out-of-range target or label raises a
// device flag (the Python mirror turns it into IndexError) instead of being read.
#include <algorithm>
#include "eval_common.h"
#include "internal.h"

namespace {

constexpr int ET = 256;        // threads per workgroup
constexpr int HIST_MAXC = 64;  // confusion tallies combine in LDS up to C = 64 (16 KiB of int32)

// target index of global query row i, or -1 when out of [0, M)
__device__ __forceinline__ int64_t target_of(const int64_t* target, int64_t i, int M) {
  const int64_t t = target ? target[i] : i;
  return (t < 0 || t >= M) ? -1 : t;
}

// pass 1: target_score[row0 + r] = S[r][t - col0] when the target column lies in this block
__global__ __launch_bounds__(ET) void rank_pick_kernel(const float* S, int64_t lds, int rows, int cols, int row0,
                                                       int col0, const int64_t* target, int M, float* target_score,
                                                       int* bad) {
  const int r = blockIdx.x * ET + threadIdx.x;
  if (r >= rows) return;
  const int64_t i = (int64_t)row0 + r;
  const int64_t t = target_of(target, i, M);
  if (t < 0) {
    *bad = 1;
    target_score[i] = -1.f;
    return;
  }
  const int64_t c = t - col0;
  if (c >= 0 && c < cols) target_score[i] = S[(int64_t)r * lds + c];
}

struct Tally { int gt, eq; Best b; };

__device__ __forceinline__ void tally1(Tally& a, float s, int j, float ts, int t) {
  if (j != t) {
    a.gt += s > ts;
    a.eq += s == ts;
  }
  if (a.b.i < 0 || s > a.b.s) { a.b.s = s; a.b.i = j; }  // j ascends per thread: the lowest index stays on ties
}

// columns [lane0, cols) of one block row in steps of `stride` threads; VEC: 16-B loads (row 16-B aligned,
// cols % 4 handled by the scalar tail)
template <bool VEC>
__device__ __forceinline__ Tally tally_row(const float* s, int cols, int col0, float ts, int t, int tid, int stride) {
  Tally a{0, 0, {0.f, -1}};
  if (VEC) {
    const int c4 = cols & ~3;
    for (int j = tid * 4; j < c4; j += stride * 4) {
      const f32x4 v = *(const f32x4*)(s + j);
#pragma unroll
      for (int k = 0; k < 4; ++k) tally1(a, v[k], col0 + j + k, ts, t);
    }
    for (int j = c4 + tid; j < cols; j += stride) tally1(a, s[j], col0 + j, ts, t);
  } else {
    for (int j = tid; j < cols; j += stride) tally1(a, s[j], col0 + j, ts, t);
  }
  return a;
}

// merge a row's block tally into its running outputs (first: this is the row's first block)
__device__ __forceinline__ void merge_row(const Tally& a, int64_t i, int first, int* greater, int* equal, int* top1,
                                          float* top1_score) {
  if (first) {
    greater[i] = a.gt;
    equal[i] = a.eq;
    top1[i] = a.b.i;
    top1_score[i] = a.b.s;
  } else {
    greater[i] += a.gt;
    equal[i] += a.eq;
    const Best run{top1_score[i], top1[i]};
    if (better(a.b.s, a.b.i, run)) {
      top1[i] = a.b.i;
      top1_score[i] = a.b.s;
    }
  }
}

__device__ __forceinline__ void mark_bad_row(int64_t i, int first, int* greater, int* equal, int* top1,
                                             float* top1_score) {
  if (!first) return;
  greater[i] = -1;
  equal[i] = -1;
  top1[i] = -1;
  top1_score[i] = -1.f;
}

// pass 2.  WAVES = 1: one wave per row, 4 rows per workgroup; WAVES = 4: one workgroup per row (wide blocks), its
// waves' tallies combined in LDS
template <int WAVES, bool VEC>
__global__ __launch_bounds__(ET) void rank_count_kernel(const float* S, int64_t lds, int rows, int cols, int row0,
                                                        int col0, const int64_t* target, int M,
                                                        const float* target_score, int first, int* greater, int* equal,
                                                        int* top1, float* top1_score) {
  __shared__ Tally part[WAVES];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = WAVES == 1 ? blockIdx.x * (ET / 64) + w : blockIdx.x;
  if (WAVES == 1 && r >= rows) return;  // its waves share no barrier; the wide grid is exact
  const int tid = WAVES == 1 ? lane : (int)threadIdx.x;
  const int64_t i = (int64_t)row0 + r;
  const int64_t t = target_of(target, i, M);  // uniform over the row's threads
  if (t < 0) {
    if (tid == 0) mark_bad_row(i, first, greater, equal, top1, top1_score);
    return;
  }
  Tally a = tally_row<VEC>(S + (int64_t)r * lds, cols, col0, target_score[i], (int)t, tid, WAVES * 64);
  a.gt = wave_sum(a.gt);
  a.eq = wave_sum(a.eq);
  a.b = wave_best(a.b);
  if (WAVES > 1) {
    if (lane == 0) part[w] = a;
    __syncthreads();
  }
  if (tid == 0) {
    for (int k = 1; k < WAVES; ++k) {
      a.gt += part[k].gt;
      a.eq += part[k].eq;
      if (better(part[k].b.s, part[k].b.i, a.b)) a.b = part[k].b;
    }
    merge_row(a, i, first, greater, equal, top1, top1_score);
  }
}

// pred / conf per row (one wave per row, rows strided over the grid) and the confusion tallies.  HIST: the
// workgroup's tallies are summed in an LDS [C][C] table and flushed with one global atomic per non-zero
// cell; else (C > HIST_MAXC: C^2 >= 4225 cells, so little contention per cell) one global atomic per row.
template <bool HIST>
__global__ __launch_bounds__(ET) void classify_kernel(const float* probs, const int64_t* labels, int B, int C,
                                                      int* pred, float* conf, unsigned long long* confusion,
                                                      int* bad) {
  __shared__ int hist[HIST ? HIST_MAXC * HIST_MAXC : 1];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (HIST) {
    for (int k = threadIdx.x; k < C * C; k += ET) hist[k] = 0;
    __syncthreads();
  }
  for (int64_t row = (int64_t)blockIdx.x * (ET / 64) + w; row < B; row += (int64_t)gridDim.x * (ET / 64)) {
    const float* p = probs + row * C;
    Best b{0.f, -1};
    for (int c = lane; c < C; c += 64) {
      const float v = p[c];
      if (b.i < 0 || v > b.s) { b.s = v; b.i = c; }
    }
    b = wave_best(b);
    if (lane == 0) {
      pred[row] = b.i;
      conf[row] = b.s;
      const int64_t lab = labels[row];
      if (lab < 0 || lab >= C) {
        *bad = 1;
      } else if (HIST) {
        atomicAdd(&hist[(int)lab * C + b.i], 1);
      } else {
        atomicAdd(&confusion[lab * C + b.i], 1ull);
      }
    }
  }
  if (HIST) {
    __syncthreads();
    for (int k = threadIdx.x; k < C * C; k += ET) {
      const int n = hist[k];
      if (n) atomicAdd(&confusion[k], (unsigned long long)n);
    }
  }
}

}  // namespace

int check_block(const char* who, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0, int cols) {
  const std::string f(who);
  if (!(N > 0 && M > 0)) return clipmi_invalid(f + ": N and M must be positive");
  if (!(rows > 0 && cols > 0)) return clipmi_invalid(f + ": block rows and cols must be positive");
  if (!(row0 >= 0 && (int64_t)row0 + rows <= N)) return clipmi_invalid(f + ": block rows out of [0, N)");
  if (!(col0 >= 0 && (int64_t)col0 + cols <= M)) return clipmi_invalid(f + ": block columns out of [0, M)");
  if (!(lds >= cols)) return clipmi_invalid(f + ": leading dimension smaller than the block width");
  if (!S) return clipmi_invalid(f + ": null score block");
  return CLIPMI_OK;
}

extern "C" int clipmi_rank_pick(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0,
                                int cols, const int64_t* target, float* target_score, int* bad) {
  CLIPMI_TRY(check_block(__func__, S, lds, N, M, row0, rows, col0, cols));
  CLIPMI_REQUIRE(target || N == M, "paired targets (target == NULL) need N == M");
  CLIPMI_REQUIRE(target_score && bad, "null output");
  hipLaunchKernelGGL(rank_pick_kernel, dim3((rows + ET - 1) / ET), dim3(ET), 0, (hipStream_t)stream, S, lds, rows, cols,
                     row0, col0, target, M, target_score, bad);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_rank_count(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0,
                                 int cols, const int64_t* target, const float* target_score, int first, int* greater,
                                 int* equal, int* top1, float* top1_score) {
  CLIPMI_TRY(check_block(__func__, S, lds, N, M, row0, rows, col0, cols));
  CLIPMI_REQUIRE(target || N == M, "paired targets (target == NULL) need N == M");
  CLIPMI_REQUIRE(target_score && greater && equal && top1 && top1_score, "null input or output");
  const bool vec = block_vec_ok(S, lds);
  const hipStream_t s = (hipStream_t)stream;
  if (cols > WIDE_COLS) {
    auto k = vec ? rank_count_kernel<4, true> : rank_count_kernel<4, false>;
    hipLaunchKernelGGL(k, dim3(rows), dim3(ET), 0, s, S, lds, rows, cols, row0, col0, target, M, target_score, first,
                       greater, equal, top1, top1_score);
  } else {
    auto k = vec ? rank_count_kernel<1, true> : rank_count_kernel<1, false>;
    hipLaunchKernelGGL(k, dim3((rows + ET / 64 - 1) / (ET / 64)), dim3(ET), 0, s, S, lds, rows, cols, row0, col0, target,
                       M, target_score, first, greater, equal, top1, top1_score);
  }
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_classify_accumulate(void* stream, const float* probs, const int64_t* labels, int B, int C,
                                          int* pred, float* conf, int64_t* confusion, int* bad) {
  CLIPMI_REQUIRE(B > 0 && C > 0, "B and C must be positive");
  CLIPMI_REQUIRE((int64_t)C * C <= INT32_MAX, "C * C must fit an int");
  CLIPMI_REQUIRE(probs && labels, "null input");
  CLIPMI_REQUIRE(pred && conf && confusion && bad, "null output");
  // enough workgroups to cover the chip, few enough that each combines many rows before its flush
  const int grid = (int)std::min<int64_t>(((int64_t)B + ET / 64 - 1) / (ET / 64), 512);
  auto k = C <= HIST_MAXC ? classify_kernel<true> : classify_kernel<false>;
  hipLaunchKernelGGL(k, dim3(grid), dim3(ET), 0, (hipStream_t)stream, probs, labels, B, C, pred, conf,
                     (unsigned long long*)confusion, bad);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
