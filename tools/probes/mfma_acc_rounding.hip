// Probe: how does v_mfma_f32_16x16x32_bf16 round an accumulator input far below its products (gfx950)?
// Every row of A is a[], every column of B is b[], so every output element is acc + sum_k a[k] b[k].
// hipcc --offload-arch=gfx950 mfma_acc_rounding.hip -o mfma_acc_rounding && ./mfma_acc_rounding
// Observed on MI355X, the same for t = 1e-10, 1e-20, 1e-36, 1e-39:
//   acc -t + 4*1 -> 3.99999976 (4 - 2^-22)   acc +t + 4*1 -> 4   acc +-t - 4*1 -> -4
//   acc +t - 4 + 4 -> 0                      acc -t - 4 + 4 -> -2.38418579e-07 (-2^-22)
// i.e. the accumulator input is aligned to the largest addend and truncated toward -inf.  Tiny *products* beside a
// large one (4*1 + 31 * (-t * 1)) leave no trace.  csrc/attention_x3.hip p_flush rests on this.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void k(const float* a, const float* b, float c0, float* out) {
  const int g = threadIdx.x >> 4;
  bf16x8 fa, fb;
  for (int j = 0; j < 8; ++j) { fa[j] = (__bf16)a[8 * g + j]; fb[j] = (__bf16)b[8 * g + j]; }
  f32x4 acc = {c0, c0, c0, c0};
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, acc, 0, 0, 0);
  if (threadIdx.x == 0) out[0] = acc[0];
}

#define CK(x) do { if ((x) != hipSuccess) { printf("hip error at %s\n", #x); exit(1); } } while (0)

static float run(const float* a, const float* b, float c0) {
  float *da, *db, *dout, r = 0;
  CK(hipMalloc(&da, 128)); CK(hipMalloc(&db, 128)); CK(hipMalloc(&dout, 4));
  CK(hipMemcpy(da, a, 128, hipMemcpyHostToDevice)); CK(hipMemcpy(db, b, 128, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k, dim3(1), dim3(64), 0, 0, da, db, c0, dout);
  CK(hipMemcpy(&r, dout, 4, hipMemcpyDeviceToHost));
  CK(hipFree(da)); CK(hipFree(db)); CK(hipFree(dout));
  return r;
}

int main() {
  float a[32], b[32];
  const float ts[] = {1e-10f, 1e-20f, 1e-36f, 1e-39f};
  for (float t : ts) {
    auto fill = [&](float av, float bv) { for (int i = 0; i < 32; ++i) { a[i] = av; b[i] = bv; } };
    printf("t = %g\n", t);
    fill(t, -1.f); a[0] = 1.f; b[0] = 4.f;
    printf("  4*1 + 31 * (-t * 1)  -> %.9g\n", run(a, b, 0.f));
    fill(0.f, 0.f); a[0] = 1.f; b[0] = 4.f;
    printf("  acc -t + 4*1         -> %.9g\n", run(a, b, -t));
    printf("  acc +t + 4*1         -> %.9g\n", run(a, b, t));
    b[0] = -4.f;
    printf("  acc +t - 4*1         -> %.9g\n", run(a, b, t));
    printf("  acc -t - 4*1         -> %.9g\n", run(a, b, -t));
    a[1] = 1.f; b[1] = 4.f;
    printf("  acc +t - 4 + 4       -> %.9g\n", run(a, b, t));
    printf("  acc -t - 4 + 4       -> %.9g\n", run(a, b, -t));
  }
  return 0;
}
