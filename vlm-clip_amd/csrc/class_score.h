// Shared by the class-score heads (heads.hip clipmi_class_scores, multilabel.hip clipmi_class_bce): the one
// definition of a row's class scores, so the softmax head and the sigmoid head read the same bits.
#pragma once
#include "common.h"

constexpr int CLASS_THREADS = 256;                  // threads per workgroup of both kernels
constexpr int CLASS_MAXE = 1024, CLASS_MAXC = 1024;  // the LDS row and score tables

// One workgroup of CLASS_THREADS per image row: stages img[row] in simg[E], then sc[c] = max over the class's
// descriptions j in [off[c], off[c+1]) of scale * img[row] . desc[j] (a wave per class, lanes over E, fixed
// order).  Ends with a barrier: every thread may read sc[0 .. C) afterwards.
__device__ __forceinline__ void class_max_scores(const float* img, int64_t row, int E, const float* desc,
                                                 const int* off, int C, float scale, float* simg, float* sc) {
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (int e = t; e < E; e += CLASS_THREADS) simg[e] = img[row * E + e];
  __syncthreads();
  for (int c = w; c < C; c += CLASS_THREADS / 64) {
    float best = -__builtin_huge_valf();
    for (int j = off[c]; j < off[c + 1]; ++j) {
      float acc = 0.f;
      for (int e = lane; e < E; e += 64) acc = fmaf(desc[(int64_t)j * E + e], simg[e], acc);
      best = fmaxf(best, scale * wave_sum(acc));
    }
    if (lane == 0) sc[c] = best;
  }
  __syncthreads();
}
