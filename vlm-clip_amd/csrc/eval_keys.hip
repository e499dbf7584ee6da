// Group-aware retrieval ranks over streamed score blocks: the positives of query i are all candidates that carry
// its 64-bit key (the multi-positive loss of contrastive_keys.hip, evaluated), not the one candidate i.
//
// For query row i with key q_i the rank of its best positive is 1 + #{ j : key_j != q_i, S[i, j] > best_i } with
// best_i = max { S[i, j] : key_j == q_i }.  As in eval.hip the [N, M] matrix is never materialised and the blocks
// S_block = Q_block . C_block^T are walked twice: pass 1 (group_pick) keeps the best positive of every row (highest
// score, lowest candidate index on equal scores) and counts the positives; pass 2 (group_count) counts the
// negatives above / equal to it and merges the row maximum.  pos_score is only ever a copy of an element of the
// GEMM output the counts are compared against, so a negative that duplicates the best positive lands in `equal`
// exactly.  A candidate named by exclude[i] (the query itself when queries and candidates are one set) is neither
// a positive nor a negative nor a top1.
//
// Kernel shape.  One wave per row would read an 8-byte candidate key next to every 4-byte score.  Here a wave
// (blocks up to WIDE_COLS columns; four strips per workgroup) or a workgroup (wider blocks) owns a strip of R = 16
// rows: a thread loads the keys of its four columns once, then the scores of those columns in all R rows (R
// independent 16-byte loads in flight) and compares them against R wave-uniform query keys.  Key traffic is 1 / R
// of what one wave per row reads: 2 / R = 1 / 8 of the score bytes.  The R partial tallies of a thread stay in
// registers and are reduced across the wave (and through LDS across the workgroup) once per strip.  A row has
// one owner per launch and the blocks of a row range are serialised on the stream: no atomics, no allocation, no
// synchronisation.
//
// topk_hits turns the candidate lists of topk.hip into relevance prefix counts (precision@k, average precision):
// one wave per row, ballot and popcount.
#include "eval_common.h"
#include "internal.h"

namespace {

constexpr int GT = 256;  // threads per workgroup (4 waves)
constexpr int R = 16;    // rows per strip

// a thread's tallies of one row.  COUNT = false (pick): a = positives seen, best = the best positive.
// COUNT = true: a / b = negatives above / equal to the row's pos_score, best = the row maximum.
struct Tally { int a, b; Best best; };

template <bool COUNT>
__device__ __forceinline__ void tally1(Tally& t, float s, int j, bool same, int ex, float ts) {
  // selects, no branches: the loop body is R x 4 of these
  const bool live = j != ex;
  const bool pass = (t.best.i < 0) | (s > t.best.s);  // j ascends per thread: the lowest index stays on ties
  bool up;
  if (COUNT) {
    const bool neg = live & !same;
    t.a += (int)(neg & (s > ts));
    t.b += (int)(neg & (s == ts));
    up = live & pass;
  } else {
    const bool pos = live & same;
    t.a += (int)pos;
    up = pos & pass;
  }
  t.best.s = up ? s : t.best.s;
  t.best.i = up ? j : t.best.i;
}

struct Args {
  const float* S;
  int64_t lds;
  int rows, cols, row0, col0, M, first;
  const int64_t *qkeys, *ckeys, *exclude;
  // pick: outputs; count: inputs
  float* pos_score;
  int* pos_idx;
  int* n_pos;
  // count: outputs
  int *greater, *equal, *top1;
  float* top1_score;
};

// merge one row's strip tally into the running outputs
template <bool COUNT>
__device__ __forceinline__ void merge_row(const Args& p, const Tally& t, int64_t i) {
  if (COUNT) {
    if (p.first) {
      const bool has = p.n_pos[i] > 0;
      p.greater[i] = has ? t.a : -1;
      p.equal[i] = has ? t.b : -1;
      p.top1[i] = t.best.i;
      p.top1_score[i] = t.best.i >= 0 ? t.best.s : -__builtin_inff();
    } else {
      if (p.n_pos[i] > 0) {
        p.greater[i] += t.a;
        p.equal[i] += t.b;
      }
      const Best run{p.top1_score[i], p.top1[i]};
      if (better(t.best.s, t.best.i, run)) {
        p.top1[i] = t.best.i;
        p.top1_score[i] = t.best.s;
      }
    }
  } else {
    if (p.first) {
      p.n_pos[i] = t.a;
      p.pos_idx[i] = t.best.i;
      p.pos_score[i] = t.best.i >= 0 ? t.best.s : -__builtin_inff();
    } else {
      p.n_pos[i] += t.a;
      const Best run{p.pos_score[i], p.pos_idx[i]};
      if (better(t.best.s, t.best.i, run)) {
        p.pos_idx[i] = t.best.i;
        p.pos_score[i] = t.best.s;
      }
    }
  }
}

// WAVES = 1: one wave per strip, 4 strips per workgroup; WAVES = 4: one workgroup per strip.  VEC: 16-B row loads
// (S 16-B aligned, lds % 4 == 0; cols % 4 handled by the scalar tail).
template <bool COUNT, int WAVES, bool VEC>
__global__ __launch_bounds__(GT) void group_strip_kernel(const Args p) {
  __shared__ Tally part[WAVES > 1 ? WAVES : 1][R];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int strip = WAVES == 1 ? blockIdx.x * (GT / 64) + w : blockIdx.x;
  const int r0 = strip * R;
  if (r0 >= p.rows) return;  // WAVES = 1 only (its waves share no barrier); the wide grid is exact
  const int nr = min(R, p.rows - r0);
  const int tid = WAVES == 1 ? lane : (int)threadIdx.x;
  constexpr int stride = WAVES * 64;

  // per row of the strip, wave-uniform; the rows past the strip's end repeat its last row and are not written
  int64_t qk[R];
  int ex[R];
  float ts[R];
  Tally t[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int rr = min(r, nr - 1);
    const int64_t i = (int64_t)p.row0 + r0 + rr;
    qk[r] = p.qkeys[i];
    ex[r] = -1;
    if (p.exclude) {
      const int64_t e = p.exclude[i];
      if (e >= 0 && e < p.M) ex[r] = (int)e;
    }
    ts[r] = COUNT ? p.pos_score[i] : 0.f;
    t[r] = Tally{0, 0, {0.f, -1}};
  }

  // row r of the strip: the address is formed at the load (one base and the stride, not R row pointers held)
  const float* const sbase = p.S + (int64_t)r0 * p.lds;
  const int last = nr - 1;
  const int64_t* ck = p.ckeys + p.col0;
  const int c4 = VEC ? (p.cols & ~3) : 0;
  if (VEC) {
    for (int j = tid * 4; j < c4; j += stride * 4) {
      int64_t key[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) key[k] = ck[j + k];
      f32x4 v[R];
#pragma unroll
      for (int r = 0; r < R; ++r) v[r] = *(const f32x4*)(sbase + (int64_t)min(r, last) * p.lds + j);
#pragma unroll
      for (int r = 0; r < R; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) tally1<COUNT>(t[r], v[r][k], p.col0 + j + k, key[k] == qk[r], ex[r], ts[r]);
    }
  }
  for (int j = c4 + tid; j < p.cols; j += stride) {
    const int64_t key = ck[j];
    float v[R];
#pragma unroll
    for (int r = 0; r < R; ++r) v[r] = sbase[(int64_t)min(r, last) * p.lds + j];
#pragma unroll
    for (int r = 0; r < R; ++r) tally1<COUNT>(t[r], v[r], p.col0 + j, key == qk[r], ex[r], ts[r]);
  }

#pragma unroll
  for (int r = 0; r < R; ++r) {
    t[r].a = wave_sum(t[r].a);
    if (COUNT) t[r].b = wave_sum(t[r].b);
    t[r].best = wave_best(t[r].best);
  }
  if (WAVES == 1) {
    // every lane holds the strip's R results: lane r writes row r
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (lane == r && r < nr) merge_row<COUNT>(p, t[r], (int64_t)p.row0 + r0 + r);
  } else {
    if (lane == 0) {
#pragma unroll
      for (int r = 0; r < R; ++r) part[w][r] = t[r];
    }
    __syncthreads();
    const int r = threadIdx.x;
    if (r < nr) {
      Tally a = part[0][r];
      for (int k = 1; k < WAVES; ++k) {
        const Tally b = part[k][r];
        a.a += b.a;
        a.b += b.b;
        if (better(b.best.s, b.best.i, a.best)) a.best = b.best;
      }
      merge_row<COUNT>(p, a, (int64_t)p.row0 + r0 + r);
    }
  }
}

// the fields both passes read, in Args' order; the pass's own pointers start null
Args block_args(const float* S, int64_t lds, int M, int row0, int rows, int col0, int cols, const int64_t* qkeys,
                const int64_t* ckeys, const int64_t* exclude, int first) {
  return Args{S, lds, rows, cols, row0, col0, M, first, qkeys, ckeys, exclude};
}

template <bool COUNT>
void launch_strips(hipStream_t s, const Args& p) {
  const bool vec = block_vec_ok(p.S, p.lds);
  const int strips = (p.rows + R - 1) / R;
  if (p.cols > WIDE_COLS) {
    auto k = vec ? group_strip_kernel<COUNT, 4, true> : group_strip_kernel<COUNT, 4, false>;
    hipLaunchKernelGGL(k, dim3(strips), dim3(GT), 0, s, p);
  } else {
    auto k = vec ? group_strip_kernel<COUNT, 1, true> : group_strip_kernel<COUNT, 1, false>;
    hipLaunchKernelGGL(k, dim3((strips + GT / 64 - 1) / (GT / 64)), dim3(GT), 0, s, p);
  }
}

// one wave per row: hits[i][r] = #{ r' <= r : top_idx[i][r'] in [0, M) and ckeys[top_idx[i][r']] == qkeys[i] }
__global__ __launch_bounds__(GT) void topk_hits_kernel(const int* top_idx, int N, int k, int M, const int64_t* qkeys,
                                                       const int64_t* ckeys, int* hits) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * (GT / 64) + (threadIdx.x >> 6);
  if (i >= N) return;
  const int64_t q = qkeys[i];
  int run = 0;
  for (int base = 0; base < k; base += 64) {
    const int r = base + lane;
    bool hit = false;
    if (r < k) {
      const int j = top_idx[i * k + r];
      hit = j >= 0 && j < M && ckeys[j] == q;
    }
    const unsigned long long mask = __ballot(hit);
    const int upto = __popcll(mask & (~0ull >> (63 - lane)));  // lanes <= this one
    if (r < k) hits[i * k + r] = run + upto;
    run += __popcll(mask);
  }
}

}  // namespace

extern "C" int clipmi_group_pick(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0,
                                 int cols, const int64_t* qkeys, const int64_t* ckeys, const int64_t* exclude,
                                 int first, float* pos_score, int* pos_idx, int* n_pos) {
  CLIPMI_TRY(check_block(__func__, S, lds, N, M, row0, rows, col0, cols));
  CLIPMI_REQUIRE(qkeys && ckeys, "null keys");
  CLIPMI_REQUIRE(pos_score && pos_idx && n_pos, "null output");
  Args p = block_args(S, lds, M, row0, rows, col0, cols, qkeys, ckeys, exclude, first);
  p.pos_score = pos_score, p.pos_idx = pos_idx, p.n_pos = n_pos;
  launch_strips<false>((hipStream_t)stream, p);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_group_count(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0,
                                  int cols, const int64_t* qkeys, const int64_t* ckeys, const int64_t* exclude,
                                  const float* pos_score, const int* n_pos, int first, int* greater, int* equal,
                                  int* top1, float* top1_score) {
  CLIPMI_TRY(check_block(__func__, S, lds, N, M, row0, rows, col0, cols));
  CLIPMI_REQUIRE(qkeys && ckeys, "null keys");
  CLIPMI_REQUIRE(pos_score && n_pos, "null input");
  CLIPMI_REQUIRE(greater && equal && top1 && top1_score, "null output");
  Args p = block_args(S, lds, M, row0, rows, col0, cols, qkeys, ckeys, exclude, first);
  p.pos_score = const_cast<float*>(pos_score), p.n_pos = const_cast<int*>(n_pos);
  p.greater = greater, p.equal = equal, p.top1 = top1, p.top1_score = top1_score;
  launch_strips<true>((hipStream_t)stream, p);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}

extern "C" int clipmi_topk_hits(void* stream, const int* top_idx, int N, int k, int M, const int64_t* qkeys,
                                const int64_t* ckeys, int* hits) {
  CLIPMI_REQUIRE(N > 0 && M > 0, "N and M must be positive");
  CLIPMI_REQUIRE(k >= 1 && k <= CLIPMI_TOPK_MAX, "k out of [1, CLIPMI_TOPK_MAX]");
  CLIPMI_REQUIRE(top_idx && qkeys && ckeys, "null input");
  CLIPMI_REQUIRE(hits, "null output");
  const int64_t grid = ((int64_t)N + GT / 64 - 1) / (GT / 64);
  hipLaunchKernelGGL(topk_hits_kernel, dim3((unsigned)grid), dim3(GT), 0, (hipStream_t)stream, top_idx, N, k, M, qkeys,
                     ckeys, hits);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
