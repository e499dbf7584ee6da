// Geometric augmentation of the input step: PIL's Image.transform(size, AFFINE, m, NEAREST | BILINEAR,
// fillcolor=...) on uint8 [B, H, W, 3], each image with its own matrix, filter and fill colour (include/clipmi.h
// clipmi_affine_u8; tests/affine_ref.py restates the arithmetic in numpy and tests/test_cpu_affine.py pins that to
// PIL).  It is what torchvision's RandomAffine / RandomRotation do to a PIL image, and it runs where a torchvision
// user puts them: on clipmi_resize_crop_u8's output, in front of clipmi_color_u8.
//
// Bit-exact, so each of PIL's three paths is the one PIL's C code takes (Geometry.c):
//   * bilinear (ImagingGenericTransform, affine_transform, bilinear_filter32RGB): IEEE doubles per pixel, every
//     product and sum rounded on its own.  Contraction is off for the whole file: a fused a0 * xin + a1 * yin rounds
//     once and moves source coordinates across a pixel edge.
//   * nearest with a1 != 0 or a3 != 0 (affine_fixed): 16.16 fixed point.  The six integers are derived on the host;
//     the kernel's A2 + A0 x + A1 y equals PIL's running sums because nothing overflows below the validated bound.
//   * nearest with a1 == a3 == 0 (ImagingScaleAffine): PIL fills a column and a row table from *running* double sums,
//     which a closed form does not reproduce.  A pre-pass runs the same sums, one thread per image and axis, into the
//     workspace behind the records (W + H entries per such image; shipping host-built tables instead cost a 460 KB
//     copy per call at B = 256, S = 224: 0.125 ms against 0.069 ms, profiles/affine_bench.log).
//
// One launch whatever B is, and the pre-pass in front of it when some item takes the third path.  The image is the
// grid's second dimension, so the record sits in scalar registers and the choice of path is a scalar branch.  A thread
// produces four consecutive output pixels (they may wrap to the next row) and stores them as three aligned dwords;
// the gather reads bytes, from an image that fits in L2.
//
// Addressing of dst is color.hip's: an image's base takes every byte alignment, pixel p is dword-aligned exactly
// when p == base (mod 4), and the up to three pixels in front of the first such pixel and behind the last whole group
// go byte by byte: nothing outside the image is written.
#include "common.h"
#include "internal.h"
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

enum { PATH_FIXED = 0, PATH_BILINEAR = 1, PATH_SCALE = 2 };
constexpr int AFFINE_MAX_SIDE = 4096;
constexpr double AFFINE_COORD_BOUND = 16384.0;  // 16384 * 65536 = 2^30: PIL's 32-bit fixed point cannot overflow
// Blocks per image; the kernel strides over the rest (color.hip's grid: 32 x B blocks of 256 threads).
constexpr int AFFINE_MAX_BLOCKS = 32;

struct AffineRec {  // 96 bytes, one per image, in the workspace
  double m[6];
  int32_t A[6];    // PATH_FIXED: FIX(a0), FIX(a1), FIX(a2 + a0 / 2 + a1 / 2), FIX(a3), FIX(a4), FIX(a5 + ...)
  int32_t path;
  uint32_t fill;   // R | G << 8 | B << 16: a pixel as the kernel packs it
  int32_t tab;     // PATH_SCALE: index of the image's W column entries, then its H row entries, in the tables
  int32_t pad[3];
};
static_assert(sizeof(AffineRec) == 96, "AffineRec layout");

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* img, int W, int y, int x) {
  const uint8_t* p = img + ((int64_t)y * W + x) * 3;
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16;
}

// bilinear_filter32RGB's BILINEAR(v, a, b, d): a + (b - a) * d, b - a an integer
__device__ __forceinline__ double lerp8(int a, int b, double d) { return (double)a + (double)(b - a) * d; }

__device__ __forceinline__ uint32_t sample_bilinear(const uint8_t* img, const AffineRec& c, int H, int W, int x, int y) {
  const double xin = (double)x + 0.5, yin = (double)y + 0.5;
  double xo = (c.m[0] * xin + c.m[1] * yin) + c.m[2];
  double yo = (c.m[3] * xin + c.m[4] * yin) + c.m[5];
  if (xo < 0.0 || xo >= (double)W || yo < 0.0 || yo >= (double)H) return c.fill;
  xo -= 0.5, yo -= 0.5;
  const double xf = floor(xo), yf = floor(yo);
  const double dx = xo - xf, dy = yo - yf;
  const int xi = (int)xf, yi = (int)yf;  // in [-1, W - 1] and [-1, H - 1]
  const int x0 = max(xi, 0), x1 = min(xi + 1, W - 1);
  const int row = max(yi, 0);
  const uint32_t p00 = load_pixel(img, W, row, x0), p01 = load_pixel(img, W, row, x1);
  const bool second = yi + 1 < H;  // yi + 1 >= 0 always
  uint32_t p10 = 0, p11 = 0;
  if (second) p10 = load_pixel(img, W, yi + 1, x0), p11 = load_pixel(img, W, yi + 1, x1);
  uint32_t out = 0;
#pragma unroll
  for (int ch = 0; ch < 3; ++ch) {
    const int s = 8 * ch;
    const double v1 = lerp8((int)(p00 >> s & 255), (int)(p01 >> s & 255), dx);
    const double v2 = second ? lerp8((int)(p10 >> s & 255), (int)(p11 >> s & 255), dx) : v1;
    const double v = v1 + (v2 - v1) * dy;
    out |= ((uint32_t)(int)v & 255u) << s;  // v lies between its four taps
  }
  return out;
}

__device__ __forceinline__ uint32_t sample_fixed(const uint8_t* img, const AffineRec& c, int H, int W, int x, int y) {
  const int sx = (c.A[2] + c.A[0] * x + c.A[1] * y) >> 16;
  const int sy = (c.A[5] + c.A[3] * x + c.A[4] * y) >> 16;
  if (sx < 0 || sx >= W || sy < 0 || sy >= H) return c.fill;
  return load_pixel(img, W, sy, sx);
}

__device__ __forceinline__ uint32_t sample_scale(const uint8_t* img, const AffineRec& c, const int32_t* xtab,
                                                 const int32_t* ytab, int H, int W, int x, int y) {
  const int sx = xtab[x], sy = ytab[y];
  if (sx < 0 || sx >= W || sy < 0 || sy >= H) return c.fill;
  return load_pixel(img, W, sy, sx);
}

template <int PATH>
__device__ __forceinline__ void affine_image(const uint8_t* img, uint8_t* out, const AffineRec& c, const int32_t* tabs,
                                             int H, int W) {
  const int n = H * W;  // <= 2^24
  const int32_t* xtab = PATH == PATH_SCALE ? tabs + c.tab : nullptr;
  const int32_t* ytab = PATH == PATH_SCALE ? xtab + W : nullptr;
  auto sample = [&](int x, int y) -> uint32_t {
    if (PATH == PATH_BILINEAR) return sample_bilinear(img, c, H, W, x, y);
    if (PATH == PATH_FIXED) return sample_fixed(img, c, H, W, x, y);
    return sample_scale(img, c, xtab, ytab, H, W, x, y);
  };
  const int head = min((int)((uintptr_t)out & 3), n);
  const int groups = (n - head) >> 2;
  const int tail = n - head - groups * 4;
  uint32_t* words = (uint32_t*)(out + head * 3);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < groups; i += gridDim.x * 256) {
    const int p = head + i * 4;
    int y = p / W, x = p - y * W;
    uint32_t px[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      px[j] = sample(x, y);
      if (++x == W) x = 0, ++y;
    }
    words[i * 3] = px[0] | px[1] << 24;
    words[i * 3 + 1] = px[1] >> 8 | px[2] << 16;
    words[i * 3 + 2] = px[2] >> 16 | px[3] << 8;
  }
  // the single pixels go to block 0: thread t takes head pixel t, thread 64 + t takes tail pixel t
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    int p = -1;
    if (t < head) p = t;
    else if (t >= 64 && t - 64 < tail) p = head + groups * 4 + (t - 64);
    if (p >= 0) {
      const int y = p / W, x = p - y * W;
      const uint32_t v = sample(x, y);
      out[p * 3] = (uint8_t)v, out[p * 3 + 1] = (uint8_t)(v >> 8), out[p * 3 + 2] = (uint8_t)(v >> 16);
    }
  }
}

// ImagingScaleAffine's tables: n entries from the running sum that starts at c + a / 2.  Thread 2b fills image b's
// W column entries, thread 2b + 1 its H row entries; the sum is sequential, at most 4096 additions.
__global__ __launch_bounds__(64) void affine_tables_kernel(const AffineRec* recs, int32_t* tabs, int B, int H, int W) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= 2 * B) return;
  const AffineRec& c = recs[t >> 1];
  if (c.path != PATH_SCALE) return;
  const bool rows = t & 1;
  const double a = rows ? c.m[4] : c.m[0];
  const int n = rows ? H : W;
  int32_t* tab = tabs + c.tab + (rows ? W : 0);
  double o = (rows ? c.m[5] : c.m[2]) + a * 0.5;
  for (int i = 0; i < n; ++i) {
    tab[i] = o < 0.0 ? -1 : (int32_t)o;
    o += a;
  }
}

__global__ __launch_bounds__(256) void affine_kernel(const uint8_t* src, uint8_t* dst, const AffineRec* recs,
                                                     const int32_t* tabs, int H, int W) {
  const int b = blockIdx.y;
  const AffineRec c = recs[b];
  const int64_t bytes = (int64_t)H * W * 3;
  const uint8_t* img = src + b * bytes;
  uint8_t* out = dst + b * bytes;
  if (c.path == PATH_BILINEAR) affine_image<PATH_BILINEAR>(img, out, c, tabs, H, W);
  else if (c.path == PATH_FIXED) affine_image<PATH_FIXED>(img, out, c, tabs, H, W);
  else affine_image<PATH_SCALE>(img, out, c, tabs, H, W);
}

int affine_bad(const char* who, int b, const char* what) {
  return clipmi_invalid(std::string(who) + ": item " + std::to_string(b) + ": " + what);
}

// PIL's FLOOR and FIX
int32_t pil_floor(double v) { return v < 0.0 ? (int32_t)std::floor(v) : (int32_t)v; }
int32_t pil_fix(double v) { return pil_floor(v * 65536.0 + 0.5); }

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }

// Validate the caller's items; with `stage`, also derive the records the kernels read.  tab_entries: the int32
// entries of the tables that the pre-pass writes behind the records (256-byte aligned).
int affine_plan(const char* who, const clipmi_affine_item* items, int B, int H, int W, std::vector<uint8_t>* stage,
                int64_t& tab_entries) {
  tab_entries = 0;
  if (B < 0) return clipmi_invalid(std::string(who) + ": B < 0");
  if (H < 1 || W < 1 || H > AFFINE_MAX_SIDE || W > AFFINE_MAX_SIDE)
    return clipmi_invalid(std::string(who) + ": H, W must be in 1..4096");
  if (B > 0 && !items) return clipmi_invalid(std::string(who) + ": null items");
  for (int b = 0; b < B; ++b) {
    const clipmi_affine_item& it = items[b];
    for (double v : it.m)
      if (!std::isfinite(v)) return affine_bad(who, b, "the coefficients must be finite");
    if (it.filter != 0 && it.filter != 1) return affine_bad(who, b, "filter must be 0 (nearest) or 1 (bilinear)");
    if (it.fill < 0 || it.fill > 0xFFFFFF) return affine_bad(who, b, "fill must be in 0..0xFFFFFF");
    for (int r = 0; r < 2; ++r) {
      const double* a = it.m + 3 * r;
      if (std::fabs(a[0]) * W + std::fabs(a[1]) * H + std::fabs(a[2]) >= AFFINE_COORD_BOUND)
        return affine_bad(who, b, "|a| * W + |b| * H + |c| must be < 16384 in both coefficient rows (the range of "
                                  "PIL's 32-bit fixed point)");
    }
    if (it.filter == 0 && it.m[1] == 0.0 && it.m[3] == 0.0) tab_entries += (int64_t)W + H;
  }
  if (!stage) return CLIPMI_OK;
  stage->assign((size_t)B * sizeof(AffineRec), 0);
  AffineRec* recs = (AffineRec*)stage->data();
  int64_t next = 0;
  for (int b = 0; b < B; ++b) {
    const clipmi_affine_item& it = items[b];
    AffineRec& r = recs[b];
    const double* a = it.m;
    for (int k = 0; k < 6; ++k) r.m[k] = a[k];
    r.fill = (uint32_t)(it.fill >> 16 & 255) | (uint32_t)(it.fill & 0xFF00) | (uint32_t)(it.fill & 255) << 16;
    if (it.filter == 1) {
      r.path = PATH_BILINEAR;
    } else if (a[1] == 0.0 && a[3] == 0.0) {
      r.path = PATH_SCALE;
      r.tab = (int32_t)next;
      next += (int64_t)W + H;
    } else {
      r.path = PATH_FIXED;
      r.A[0] = pil_fix(a[0]), r.A[1] = pil_fix(a[1]), r.A[2] = pil_fix((a[2] + a[0] * 0.5) + a[1] * 0.5);
      r.A[3] = pil_fix(a[3]), r.A[4] = pil_fix(a[4]), r.A[5] = pil_fix((a[5] + a[3] * 0.5) + a[4] * 0.5);
    }
  }
  return CLIPMI_OK;
}

int64_t affine_ws_bytes(int B, int64_t tab_entries) {
  return align256((int64_t)B * sizeof(AffineRec)) + align256(tab_entries * 4);
}

}  // namespace

extern "C" int64_t clipmi_affine_u8_ws(const clipmi_affine_item* items, int B, int H, int W) {
  int64_t tab_entries;
  const int st = affine_plan(__func__, items, B, H, W, nullptr, tab_entries);
  if (st != CLIPMI_OK) return st;
  return B == 0 ? 0 : affine_ws_bytes(B, tab_entries);
}

extern "C" int clipmi_affine_u8(void* stream, const uint8_t* src, uint8_t* dst, const clipmi_affine_item* items, int B,
                                int H, int W, void* ws, int64_t ws_bytes) {
  // the staged records are the library's own and outlive the call (the upload below is ordered on the stream)
  static thread_local std::vector<uint8_t> stage;
  int64_t tab_entries;
  CLIPMI_TRY(affine_plan(__func__, items, B, H, W, &stage, tab_entries));
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(B <= 65535, "B must be <= 65535 (the grid's second dimension)");
  CLIPMI_REQUIRE(src && dst, "null images");
  const int64_t bytes = (int64_t)B * H * W * 3;
  CLIPMI_REQUIRE((uintptr_t)src + (uintptr_t)bytes <= (uintptr_t)dst || (uintptr_t)dst + (uintptr_t)bytes <= (uintptr_t)src,
                 "src and dst must not overlap (every output pixel gathers from the whole source image)");
  CLIPMI_REQUIRE(ws && ws_bytes >= affine_ws_bytes(B, tab_entries), "workspace too small");
  CLIPMI_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  CLIPMI_HIP(hipMemcpyAsync(ws, stage.data(), stage.size(), hipMemcpyHostToDevice, s));
  const AffineRec* drecs = (const AffineRec*)ws;
  int32_t* dtabs = (int32_t*)((uint8_t*)ws + align256((int64_t)B * sizeof(AffineRec)));
  if (tab_entries > 0)
    hipLaunchKernelGGL(affine_tables_kernel, dim3((unsigned)((2 * B + 63) / 64)), dim3(64), 0, s, drecs, dtabs, B, H, W);
  const int64_t groups = ((int64_t)H * W) >> 2;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>((groups + 255) / 256, AFFINE_MAX_BLOCKS));
  hipLaunchKernelGGL(affine_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(256), 0, s, src, dst, drecs, dtabs, H, W);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
