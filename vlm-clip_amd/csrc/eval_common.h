// Shared by the kernels that read streamed score blocks (eval.hip, eval_keys.hip, topk.hip): the one definition
// of the tie rule and the block width at which a row (or strip) goes from one wave to one workgroup.
#pragma once
#include "common.h"

constexpr int WIDE_COLS = 1024;  // wider blocks: one workgroup per row (or strip) instead of one wave

// a row's best score so far: the largest, lowest candidate index on ties; idx < 0 = none yet
struct Best { float s; int i; };
__device__ __forceinline__ bool better(float s, int i, const Best& b) {
  return i >= 0 && (b.i < 0 || s > b.s || (s == b.s && i < b.i));
}
__device__ __forceinline__ Best wave_best(Best b) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float s = __shfl_xor(b.s, o, 64);
    const int i = __shfl_xor(b.i, o, 64);
    if (better(s, i, b)) { b.s = s; b.i = i; }
  }
  return b;
}
