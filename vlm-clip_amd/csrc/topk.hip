// On-device top-K retrieval over streamed score blocks: each query row keeps its k best candidates while the
// column blocks of S = Q . C^T (the exact-f32 GEMM blocks eval.hip's rank kernels read) go by.
//
// Order.  Candidate a precedes b iff s_a > s_b, or s_a == s_b and j_a < j_b (-0.0 == +0.0; a NaN orders and is
// reported as -inf).  Each candidate is one 64-bit key: the order-preserving uint32 image of the canonical score
// (NaN -> -inf, -0.0 -> +0.0) in the high word and ~j in the low word, so "precedes" is one unsigned compare and
// the order is strict and total: the result does not depend on the block size or on the order of the blocks.  Key
// 0 is below every real key and marks an empty slot (idx -1, score -inf).
//
// Kernel.  A wave owns a list of k keys and a candidate buffer in LDS (P = 2 max(64, pow2(k)) keys in all) and
// the list's k-th key as a threshold.  Lanes stream the row (two 16-B loads per lane and step when the block
// allows, scalar loads otherwise) and test `!(s < threshold score)`, one float compare per element; a step in
// which no lane passes costs one ballot and nothing else, which is every step but a few once the first block
// has gone by.  Otherwise the exact keys above the threshold are compacted into the buffer (ballot + lane prefix
// count); a full buffer is merged by a bitonic sort of list + buffer in LDS, which raises the threshold.  Narrow
// blocks (cols <= 1024) run one wave per row, four rows per workgroup; wide blocks one workgroup per row, whose
// four waves each select from a quarter of the columns against the running list's threshold; at the end the
// first wave takes the others' survivors into its own buffer, so a row with few of them (every later block) is
// sorted once.  A row that gained nothing is not sorted or written back.  LDS is 4 P keys per workgroup (4 KiB at
// k <= 64, 16 KiB at k = 256).  A row has one owner per launch and the blocks of a row range are serialised on
// the stream: no atomics, no allocation, no synchronisation.
#include "eval_common.h"
#include "internal.h"

namespace {

constexpr int TT = 256;    // threads per workgroup (4 waves)
constexpr int UNROLL = 2;  // 16-B loads in flight per lane and step

typedef unsigned long long tkey;

__device__ __forceinline__ tkey make_key(float s, int j) {
  if (s != s) s = -__builtin_inff();
  if (s == 0.f) s = 0.f;  // -0.0 -> +0.0
  uint32_t u = __float_as_uint(s);
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return ((tkey)u << 32) | (uint32_t)~j;
}
__device__ __forceinline__ float key_score(tkey key) {
  const uint32_t u = (uint32_t)(key >> 32);
  return key ? __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u) : -__builtin_inff();
}
__device__ __forceinline__ int key_index(tkey key) { return key ? (int)~(uint32_t)key : -1; }

// orders this wave's LDS accesses across its lanes (the LDS executes a wave's instructions in order)
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// bitonic sort of a[0, P) by one wave, best (largest key) first; P a power of two >= 128
__device__ __forceinline__ void wave_sort(tkey* a, int P, int lane) {
  for (int size = 2; size <= P; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      wave_sync();
      for (int t = lane; t < (P >> 1); t += 64) {
        const int lo = 2 * t - (t & (stride - 1));
        const int hi = lo + stride;
        const bool desc = (lo & size) == 0;
        const tkey x = a[lo], y = a[hi];
        if ((x < y) == desc) {
          a[lo] = y;
          a[hi] = x;
        }
      }
    }
  }
  wave_sync();
}

// one wave's selection state: seg[0, k) the list (sorted between flushes), seg[k, k + cnt) the buffer
struct Sel {
  tkey* seg;
  int k, P, lane, cnt, ex;
  tkey thr0, thr;  // thr0: the running list's k-th key at launch; thr = max(thr0, this wave's k-th key)
  float ts;        // thr's score: no key above thr has a score below it
  bool dirty;

  __device__ __forceinline__ void set_thr(tkey t) {
    thr = t > thr0 ? t : thr0;
    ts = key_score(thr);
  }
  // merge the buffer into the list
  __device__ __forceinline__ void flush() {
    for (int p = k + cnt + lane; p < P; p += 64) seg[p] = 0;
    wave_sort(seg, P, lane);
    set_thr(seg[k - 1]);
    cnt = 0;
    dirty = true;
  }
  // every lane of the wave calls this together; valid: this lane holds score s of candidate j
  __device__ __forceinline__ void offer(bool valid, float s, int j) {
    const tkey key = make_key(s, j);
    bool p = valid && j != ex && key > thr;
    unsigned long long mask = __ballot(p);
    if (!mask) return;
    int n = __popcll(mask);
    if (cnt + n > P - k) {  // n <= 64 <= P - k: fits after the flush
      flush();
      p = p && key > thr;
      mask = __ballot(p);
      n = __popcll(mask);
    }
    if (p) {
      const int before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0));
      seg[k + cnt + before] = key;
    }
    cnt += n;
  }
  // append n <= P - k keys of another wave (its list or its buffer) to the buffer
  __device__ __forceinline__ void take(const tkey* src, int n) {
    if (n == 0) return;
    if (cnt + n > P - k) flush();
    for (int p = lane; p < n; p += 64) seg[k + cnt + p] = src[p];
    cnt += n;
  }
};

// WAVES = 1: one wave per row, 4 rows per workgroup; WAVES = 4: one workgroup per row.  VEC: 16-B loads (S 16-B
// aligned, lds % 4 == 0; cols % 4 handled by the scalar tail).  Dynamic LDS: 4 P keys + 8 ints.
template <int WAVES, bool VEC>
__global__ __launch_bounds__(TT) void topk_merge_kernel(const float* S, int64_t lds, int rows, int cols, int row0,
                                                        int col0, int M, int k, int P, int first,
                                                        const int64_t* exclude, float* top_score, int* top_idx) {
  extern __shared__ __attribute__((aligned(16))) unsigned char topk_lds[];
  tkey* const keys = (tkey*)topk_lds;
  int* const flags = (int*)(keys + 4 * P);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int r = WAVES == 1 ? blockIdx.x * (TT / 64) + w : blockIdx.x;
  if (r >= rows) return;  // WAVES = 1 only (its waves share no barrier)
  const int64_t i = (int64_t)row0 + r;
  const bool head = WAVES == 1 || w == 0;  // the wave that holds the running list and writes the row
  const int tid = WAVES == 1 ? lane : (int)threadIdx.x;
  constexpr int stride = WAVES * 64;
  float* const out_s = top_score + i * k;
  int* const out_i = top_idx + i * k;

  Sel sel;
  sel.seg = keys + w * P;
  sel.k = k;
  sel.P = P;
  sel.lane = lane;
  sel.cnt = 0;
  sel.dirty = false;
  sel.ex = -1;
  if (exclude) {
    const int64_t e = exclude[i];
    if (e >= 0 && e < M) sel.ex = (int)e;
  }
  sel.thr0 = 0;
  if (!first) {
    const int ki = out_i[k - 1];
    if (ki >= 0) sel.thr0 = make_key(out_s[k - 1], ki);
  }
  sel.set_thr(0);
  for (int p = lane; p < k; p += 64) {
    tkey key = 0;
    if (head && !first) {
      const int ji = out_i[p];
      if (ji >= 0) key = make_key(out_s[p], ji);
    }
    sel.seg[p] = key;
  }

  const float* s = S + (int64_t)r * lds;
  const int c4 = VEC ? (cols & ~3) : 0;
  if (VEC) {
    for (int base = 0; base < c4; base += stride * 4 * UNROLL) {
      f32x4 v[UNROLL];
      int j[UNROLL];
      bool any = false;
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        j[u] = base + (u * stride + tid) * 4;
        v[u] = *(const f32x4*)(s + min(j[u], c4 - 4));  // clamped: always inside the row
      }
#pragma unroll
      for (int u = 0; u < UNROLL; ++u) {
        const bool c = !(v[u][0] < sel.ts) | !(v[u][1] < sel.ts) | !(v[u][2] < sel.ts) | !(v[u][3] < sel.ts);
        any |= c && j[u] < c4;
      }
      if (__ballot(any)) {
#pragma unroll
        for (int u = 0; u < UNROLL; ++u)
#pragma unroll
          for (int e = 0; e < 4; ++e) sel.offer(j[u] < c4, v[u][e], col0 + j[u] + e);
      }
    }
  }
  for (int base = c4; base < cols; base += stride) {
    const int j = base + tid;
    const float v = s[min(j, cols - 1)];
    if (__ballot(j < cols && !(v < sel.ts))) sel.offer(j < cols, v, col0 + j);
  }

  if (WAVES > 1) {
    // the head wave takes the other waves' lists (where they flushed) and unsorted buffers into its own buffer:
    // a row whose few survivors fit there is sorted once
    if (lane == 0) {
      flags[w] = sel.dirty;
      flags[4 + w] = sel.cnt;
    }
    __syncthreads();
    if (!head) return;
    for (int o = 1; o < WAVES; ++o) {
      if (flags[o]) sel.take(keys + o * P, k);
      sel.take(keys + o * P + k, flags[4 + o]);
    }
  }
  if (sel.cnt) sel.flush();
  if (!(first || sel.dirty)) return;  // the row gained nothing
  for (int p = lane; p < k; p += 64) {
    const tkey key = sel.seg[p];
    out_s[p] = key_score(key);
    out_i[p] = key_index(key);
  }
}

}  // namespace

extern "C" int clipmi_topk_merge(void* stream, const float* S, int64_t lds, int N, int M, int row0, int rows, int col0,
                                 int cols, int k, int first, const int64_t* exclude, float* top_score, int* top_idx) {
  CLIPMI_TRY(check_block(__func__, S, lds, N, M, row0, rows, col0, cols));
  CLIPMI_REQUIRE(k >= 1 && k <= CLIPMI_TOPK_MAX, "k out of [1, CLIPMI_TOPK_MAX]");
  CLIPMI_REQUIRE(top_score && top_idx, "null output");
  int P = 128;  // 2 max(64, pow2(k)): list + buffer, the buffer holds at least one wave's survivors of a step
  while (P < 2 * k) P <<= 1;
  const size_t shmem = (size_t)4 * P * sizeof(tkey) + 8 * sizeof(int);
  const bool vec = block_vec_ok(S, lds);
  const hipStream_t s = (hipStream_t)stream;
  if (cols > WIDE_COLS) {
    auto kern = vec ? topk_merge_kernel<4, true> : topk_merge_kernel<4, false>;
    hipLaunchKernelGGL(kern, dim3(rows), dim3(TT), shmem, s, S, lds, rows, cols, row0, col0, M, k, P, first, exclude,
                       top_score, top_idx);
  } else {
    auto kern = vec ? topk_merge_kernel<1, true> : topk_merge_kernel<1, false>;
    hipLaunchKernelGGL(kern, dim3((rows + TT / 64 - 1) / (TT / 64)), dim3(TT), shmem, s, S, lds, rows, cols, row0, col0,
                       M, k, P, first, exclude, top_score, top_idx);
  }
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
