// The policy ops of the input step that are neither affine nor a blend against a per-image constant: PIL's
// ImageOps.posterize / solarize / autocontrast / equalize and ImageEnhance.Sharpness on uint8 [B, H, W, 3], out of
// place, each image with its own op (include/clipmi.h clipmi_enhance_u8; tests/enhance_ref.py restates the arithmetic
// in numpy and tests/test_cpu_enhance.py pins that to PIL).  With clipmi_affine_u8 and clipmi_color_u8 they are the
// fourteen ops of torchvision's RandAugment and TrivialAugmentWide on PIL images (clipmi/images.py apply_policy_u8).
//
// Bit-exact, so every operation below is the one PIL performs, in its width:
//   * autocontrast (cutoff 0): per channel lo / hi = the first / last non-empty bin; hi <= lo: the identity; else in
//     double scale = 255.0 / (hi - lo), offset = -lo * scale, lut[i] = clamp((int)(i * scale + offset)): the product
//     and the sum rounded separately (contraction is off for the whole file), truncated toward zero.
//   * equalize: per channel, fewer than two non-empty bins: the identity; step = (sum h - last non-empty bin) / 255,
//     0: the identity; else n = step / 2; lut[i] = n / step, n += h[i].  All integers, 32 bits (H * W <= 2^24).
//     n / step passes 255 when the last non-empty bin is 255 and the bins below it hold more than 255.5 steps (a
//     1 x 400 image whose bytes run 0..255 and then stay at 254 has step 1 and entries up to 399); PIL hands the list
//     to Image.point, whose C side stores each entry clipped to a byte (CLIP8), so the entry is stored as 255.
//   * sharpness: the degenerate image is ImageFilter.SMOOTH, (1,1,1,1,5,1,1,1,1) / 13 as float32 quotients; a float32
//     accumulator starts at 0.5 and takes the three rows one after the other, each as (k0 * left + k1 * mid) +
//     k2 * right; <= 0 -> 0, >= 255 -> 255, else truncated.  (The exact sum, 0.5 + s / 13 with s an integer, is never
//     closer than 1 / 26 to an integer, so neither the order of the rows nor the width of the sum can show.)  The
//     one-pixel frame is the source's (so an image with H < 3 or W < 3 is left whole).  Then Image.blend(degenerate,
//     image, value): color.hip's blend, float32 d + a * float32(x - d), two roundings.
//   * posterize: i & ~(2^(8 - bits) - 1).  solarize: (float)i < value ? i : 255 - i.
//
// At most three launches whatever B is, one when no item is an autocontrast or an equalize:
//   1. histogram (those images only): a block keeps 3 x 256 uint32 bins in LDS and adds its non-zero ones into the
//      image's row of a [B][768] table in the workspace, zeroed by a memset node in front of it.  Integer counts: the
//      table does not depend on the order of the adds.
//   2. LUT (those images only): one block per image scans its row (256 threads, LDS) into 768 bytes behind the table.
//      Building the LUT at the head of each of the 32 apply blocks instead saves this launch and repeats the scan 32
//      times per image; measured at B = 256, S = 224 (profiles/policy_bench.log) that form took 0.149 ms against
//      0.056 ms for a batch of equalizes and 0.088 ms against 0.077 ms for the five ops in turn, so the kernel of its
//      own is the one kept.
//   3. apply: every pixel through its image's op.  The image is the grid's second dimension, so the record sits in
//      scalar registers and the op is a scalar branch.
//
// Addressing of dst is color.hip's and affine.hip's: an image's base takes every byte alignment, pixel p is
// dword-aligned exactly when p == base (mod 4); a thread stores four pixels as three aligned dwords and the up to
// three pixels in front of the first such pixel and behind the last whole group go byte by byte: nothing outside the
// image is written.  The source is read as dwords when src and dst sit alike modulo 4, else byte by byte.
#include "common.h"
#include "internal.h"
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

enum { OP_NONE = 0, OP_POSTERIZE = 1, OP_SOLARIZE = 2, OP_AUTOCONTRAST = 3, OP_EQUALIZE = 4, OP_SHARPNESS = 5 };
constexpr int64_t ENHANCE_MAX_PIXELS = (int64_t)1 << 24;  // a bin, and equalize's n + step / 2, fit 32 bits
// Blocks per image; the kernels stride over the rest (color.hip's grid: 32 x B blocks of 256 threads).
constexpr int ENHANCE_MAX_BLOCKS = 32;

static_assert(sizeof(clipmi_enhance_item) == 8, "clipmi_enhance_item layout");

__device__ __forceinline__ bool needs_hist(int op) { return op == OP_AUTOCONTRAST || op == OP_EQUALIZE; }

__device__ __forceinline__ uint32_t load_pixel(const uint8_t* img, int64_t p) {
  const uint8_t* s = img + p * 3;
  return (uint32_t)s[0] | (uint32_t)s[1] << 8 | (uint32_t)s[2] << 16;
}

// Image.blend per byte (color.hip's blend; ImageEnhance takes any factor, so the clip stays)
__device__ __forceinline__ int blend(int d, int x, float a) {
  const float prod = a * (float)(x - d);
  const float t = (float)d + prod;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

// ------------------------------------------------------------------------------------------------ pass 1: histogram
__global__ __launch_bounds__(256) void enhance_hist_kernel(const uint8_t* src, const clipmi_enhance_item* recs,
                                                           uint32_t* table, int64_t n) {
  const int b = blockIdx.y;
  if (!needs_hist(recs[b].op)) return;
  __shared__ uint32_t bins[768];
  for (int i = threadIdx.x; i < 768; i += 256) bins[i] = 0;
  __syncthreads();
  const uint8_t* img = src + (int64_t)b * n * 3;
  int64_t head = (int64_t)((uintptr_t)img & 3);
  if (head > n) head = n;
  const int64_t groups = (n - head) >> 2;
  const int64_t tail = n - head - groups * 4;
  const uint32_t* words = (const uint32_t*)(img + head * 3);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < groups; i += (int64_t)gridDim.x * 256) {
    const uint32_t w[3] = {words[i * 3], words[i * 3 + 1], words[i * 3 + 2]};
#pragma unroll
    for (int k = 0; k < 12; ++k) atomicAdd(&bins[(k % 3) * 256 + (w[k >> 2] >> (8 * (k & 3)) & 255)], 1u);
  }
  // the single pixels go to block 0: thread t takes head pixel t, thread 64 + t takes tail pixel t
  if (blockIdx.x == 0) {
    const int t = threadIdx.x;
    int64_t p = -1;
    if (t < head) p = t;
    else if (t >= 64 && t - 64 < tail) p = head + groups * 4 + (t - 64);
    if (p >= 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) atomicAdd(&bins[c * 256 + img[p * 3 + c]], 1u);
    }
  }
  __syncthreads();
  uint32_t* row = table + (int64_t)b * 768;
  for (int i = threadIdx.x; i < 768; i += 256)
    if (bins[i] != 0) atomicAdd(&row[i], bins[i]);
}

// ------------------------------------------------------------------------------------------------ pass 2: LUT
struct LutScratch {
  uint32_t h[768];
  uint32_t s[2][768];  // equalize's inclusive scan, double-buffered
  int lo[3], hi[3];
};

// 256 threads, thread t = bin t of the three channels; hist: the image's 768 counts; lut: 768 bytes.  `op` is the
// same for the whole block.
__device__ __forceinline__ void build_lut(const uint32_t* hist, int op, uint8_t* lut, LutScratch& w) {
  const int t = threadIdx.x;
  if (t < 3) w.lo[t] = 256, w.hi[t] = -1;
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t v = hist[c * 256 + t];
    w.h[c * 256 + t] = v;
    w.s[0][c * 256 + t] = v;
    if (v != 0) atomicMin(&w.lo[c], t), atomicMax(&w.hi[c], t);
  }
  __syncthreads();
  int cur = 0;
  if (op == OP_EQUALIZE) {
    for (int off = 1; off < 256; off <<= 1) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int i = c * 256 + t;
        uint32_t v = w.s[cur][i];
        if (t >= off) v += w.s[cur][i - off];
        w.s[cur ^ 1][i] = v;
      }
      __syncthreads();
      cur ^= 1;
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int lo = w.lo[c], hi = w.hi[c];  // hi >= lo >= 0: an image has at least one pixel
    int out = t;
    if (hi > lo) {  // at least two non-empty bins
      if (op == OP_AUTOCONTRAST) {
        const double scale = 255.0 / (double)(hi - lo);
        const double offset = (double)(-lo) * scale;
        const double prod = (double)t * scale;
        const int v = (int)(prod + offset);
        out = v < 0 ? 0 : v > 255 ? 255 : v;
      } else {
        const uint32_t total = w.s[cur][c * 256 + 255];
        const uint32_t step = (total - w.h[c * 256 + hi]) / 255u;
        if (step != 0) {
          const uint32_t below = w.s[cur][c * 256 + t] - w.h[c * 256 + t];  // h[0] + ... + h[t - 1]
          const uint32_t v = (step / 2 + below) / step;
          out = v > 255u ? 255 : (int)v;
        }
      }
    }
    lut[c * 256 + t] = (uint8_t)out;
  }
}

__global__ __launch_bounds__(256) void enhance_lut_kernel(const clipmi_enhance_item* recs, const uint32_t* table,
                                                          uint8_t* luts) {
  const int b = blockIdx.x;
  const int op = recs[b].op;
  if (!needs_hist(op)) return;
  __shared__ LutScratch w;
  __shared__ uint8_t lut[768];
  build_lut(table + (int64_t)b * 768, op, lut, w);
  // every thread stores the three entries it wrote itself
#pragma unroll
  for (int c = 0; c < 3; ++c) luts[(int64_t)b * 768 + c * 256 + threadIdx.x] = lut[c * 256 + threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ pass 3: apply
// one pixel (R | G << 8 | B << 16) through a per-byte op
template <int OP>
__device__ __forceinline__ uint32_t map_pixel(uint32_t px, float value, uint32_t mask, const uint8_t* lut) {
  if (OP == OP_NONE) return px;
  if (OP == OP_POSTERIZE) return px & mask;
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const uint32_t v = px >> (8 * c) & 255u;
    uint32_t r;
    if (OP == OP_SOLARIZE) r = (float)v < value ? v : 255u - v;
    else r = lut[c * 256 + v];
    out |= r << (8 * c);
  }
  return out;
}

// ImageEnhance.Sharpness of pixel (x, y)
__device__ __forceinline__ uint32_t sharp_pixel(const uint8_t* img, int H, int W, int x, int y, float value) {
  const int64_t p = (int64_t)y * W + x;
  const uint32_t centre = load_pixel(img, p);
  if (x == 0 || y == 0 || x == W - 1 || y == H - 1) return centre;  // the frame: SMOOTH copies it, the blend keeps it
  constexpr float k1 = 1.0f / 13.0f, k5 = 5.0f / 13.0f;
  float ss[3] = {0.5f, 0.5f, 0.5f};
#pragma unroll
  for (int dy = 1; dy >= -1; --dy) {
    const int64_t q = p + (int64_t)dy * W;
    const uint32_t l = load_pixel(img, q - 1), m = dy == 0 ? centre : load_pixel(img, q), r = load_pixel(img, q + 1);
    const float km = dy == 0 ? k5 : k1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float fl = (float)(l >> (8 * c) & 255u), fm = (float)(m >> (8 * c) & 255u), fr = (float)(r >> (8 * c) & 255u);
      const float a = fl * k1, bm = fm * km, cr = fr * k1;
      const float row = (a + bm) + cr;
      ss[c] = ss[c] + row;
    }
  }
  uint32_t out = 0;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const int d = ss[c] <= 0.f ? 0 : ss[c] >= 255.f ? 255 : (int)ss[c];
    out |= (uint32_t)blend(d, (int)(centre >> (8 * c) & 255u), value) << (8 * c);
  }
  return out;
}

template <int OP>
__device__ __forceinline__ void enhance_image(const uint8_t* img, uint8_t* out, float value, const uint8_t* lut, int H,
                                              int W) {
  const int n = H * W;  // <= 2^24
  const uint32_t mask = OP == OP_POSTERIZE ? (~((1u << (8 - (int)value)) - 1u) & 255u) * 0x010101u : 0u;
  const int head = min((int)((uintptr_t)out & 3), n);
  const int groups = (n - head) >> 2;
  const int tail = n - head - groups * 4;
  uint32_t* words = (uint32_t*)(out + head * 3);
  const bool alike = (((uintptr_t)img ^ (uintptr_t)out) & 3) == 0;  // then the source's groups are aligned dwords too
  const uint32_t* swords = (const uint32_t*)(img + head * 3);
  for (int i = blockIdx.x * 256 + threadIdx.x; i < groups; i += gridDim.x * 256) {
    const int p = head + i * 4;
    uint32_t px[4];
    if (OP == OP_SHARPNESS) {
      int y = p / W, x = p - y * W;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        px[j] = sharp_pixel(img, H, W, x, y, value);
        if (++x == W) x = 0, ++y;
      }
    } else {
      if (alike) {
        const uint32_t w0 = swords[i * 3], w1 = swords[i * 3 + 1], w2 = swords[i * 3 + 2];
        px[0] = w0 & 0xFFFFFFu, px[1] = w0 >> 24 | (w1 & 0xFFFFu) << 8, px[2] = w1 >> 16 | (w2 & 0xFFu) << 16, px[3] = w2 >> 8;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) px[j] = load_pixel(img, p + j);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) px[j] = map_pixel<OP>(px[j], value, mask, lut);
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
      uint32_t v;
      if (OP == OP_SHARPNESS) {
        const int y = p / W, x = p - y * W;
        v = sharp_pixel(img, H, W, x, y, value);
      } else {
        v = map_pixel<OP>(load_pixel(img, p), value, mask, lut);
      }
      out[p * 3] = (uint8_t)v, out[p * 3 + 1] = (uint8_t)(v >> 8), out[p * 3 + 2] = (uint8_t)(v >> 16);
    }
  }
}

__global__ __launch_bounds__(256) void enhance_apply_kernel(const uint8_t* src, uint8_t* dst,
                                                            const clipmi_enhance_item* recs, const uint8_t* luts, int H,
                                                            int W) {
  const int b = blockIdx.y;
  const clipmi_enhance_item c = recs[b];
  const int64_t bytes = (int64_t)H * W * 3;
  const uint8_t* img = src + b * bytes;
  uint8_t* out = dst + b * bytes;
  __shared__ uint8_t lut[768];
  if (needs_hist(c.op)) {
    for (int i = threadIdx.x; i < 768; i += 256) lut[i] = luts[(int64_t)b * 768 + i];
    __syncthreads();
    enhance_image<OP_AUTOCONTRAST>(img, out, c.value, lut, H, W);
  } else if (c.op == OP_NONE) {
    enhance_image<OP_NONE>(img, out, c.value, lut, H, W);
  } else if (c.op == OP_POSTERIZE) {
    enhance_image<OP_POSTERIZE>(img, out, c.value, lut, H, W);
  } else if (c.op == OP_SOLARIZE) {
    enhance_image<OP_SOLARIZE>(img, out, c.value, lut, H, W);
  } else {
    enhance_image<OP_SHARPNESS>(img, out, c.value, lut, H, W);
  }
}

// ------------------------------------------------------------------------------------------------ host
int enhance_bad(const char* who, int b, const char* what) {
  return clipmi_invalid(std::string(who) + ": item " + std::to_string(b) + ": " + what);
}

// Validate the caller's items; hist: whether some item needs the histogram pass.
int enhance_plan(const char* who, const clipmi_enhance_item* items, int B, int H, int W, bool& hist) {
  hist = false;
  if (B < 0) return clipmi_invalid(std::string(who) + ": B < 0");
  if (H < 1 || W < 1) return clipmi_invalid(std::string(who) + ": H, W must be >= 1");
  if ((int64_t)H * W > ENHANCE_MAX_PIXELS)
    return clipmi_invalid(std::string(who) + ": H * W must be <= 2^24 (the 32-bit histogram bins and equalize sums)");
  if (B > 65535) return clipmi_invalid(std::string(who) + ": B must be <= 65535 (the grid's second dimension)");
  if (B > 0 && !items) return clipmi_invalid(std::string(who) + ": null items");
  for (int b = 0; b < B; ++b) {
    const clipmi_enhance_item it = items[b];
    if (it.op < OP_NONE || it.op > OP_SHARPNESS) return enhance_bad(who, b, "unknown op");
    if (!std::isfinite(it.value)) return enhance_bad(who, b, "value must be finite");
    if (it.op == OP_POSTERIZE && !(it.value >= 1.f && it.value <= 8.f && it.value == std::floor(it.value)))
      return enhance_bad(who, b, "posterize bits must be an integer in 1..8");
    if (it.op == OP_SHARPNESS && it.value < 0.f) return enhance_bad(who, b, "sharpness factor must be >= 0");
    hist |= it.op == OP_AUTOCONTRAST || it.op == OP_EQUALIZE;
  }
  return CLIPMI_OK;
}

int64_t align256(int64_t v) { return (v + 255) & ~(int64_t)255; }
// the records; with a histogram pass, the [B][768] uint32 table and the [B][768] byte LUTs behind them
int64_t enhance_ws_bytes(int B, bool hist) {
  return align256((int64_t)B * sizeof(clipmi_enhance_item)) + (hist ? (int64_t)B * 768 * 4 + align256((int64_t)B * 768) : 0);
}

}  // namespace

extern "C" int64_t clipmi_enhance_u8_ws(const clipmi_enhance_item* items, int B, int H, int W) {
  bool hist;
  const int st = enhance_plan(__func__, items, B, H, W, hist);
  if (st != CLIPMI_OK) return st;
  return B == 0 ? 0 : enhance_ws_bytes(B, hist);
}

extern "C" int clipmi_enhance_u8(void* stream, const uint8_t* src, uint8_t* dst, const clipmi_enhance_item* items,
                                 int B, int H, int W, void* ws, int64_t ws_bytes) {
  // the records are the library's own and outlive the call (the upload below is ordered on the stream)
  static thread_local std::vector<clipmi_enhance_item> recs;
  bool hist;
  CLIPMI_TRY(enhance_plan(__func__, items, B, H, W, hist));
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(src && dst, "null images");
  const int64_t bytes = (int64_t)B * H * W * 3;
  CLIPMI_REQUIRE((uintptr_t)src + (uintptr_t)bytes <= (uintptr_t)dst || (uintptr_t)dst + (uintptr_t)bytes <= (uintptr_t)src,
                 "src and dst must not overlap (sharpness reads every pixel's neighbours)");
  CLIPMI_REQUIRE(ws && ws_bytes >= enhance_ws_bytes(B, hist), "workspace too small");
  CLIPMI_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  recs.assign(items, items + B);
  clipmi_enhance_item* drecs = (clipmi_enhance_item*)ws;
  CLIPMI_HIP(hipMemcpyAsync(drecs, recs.data(), (size_t)B * sizeof(clipmi_enhance_item), hipMemcpyHostToDevice, s));
  uint32_t* table = (uint32_t*)((uint8_t*)ws + align256((int64_t)B * sizeof(clipmi_enhance_item)));
  uint8_t* luts = (uint8_t*)(table + (int64_t)B * 768);
  const int64_t n = (int64_t)H * W;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((n >> 2) + 255) / 256, ENHANCE_MAX_BLOCKS));
  const dim3 grid((unsigned)blocks, (unsigned)B);
  if (hist) {
    CLIPMI_HIP(hipMemsetAsync(table, 0, (size_t)B * 768 * 4, s));
    hipLaunchKernelGGL(enhance_hist_kernel, grid, dim3(256), 0, s, src, drecs, table, n);
    hipLaunchKernelGGL(enhance_lut_kernel, dim3((unsigned)B), dim3(256), 0, s, drecs, table, luts);
  }
  hipLaunchKernelGGL(enhance_apply_kernel, grid, dim3(256), 0, s, src, dst, drecs, luts, H, W);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
