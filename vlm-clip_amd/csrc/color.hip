// Colour augmentation of the input step: PIL's ImageEnhance.Brightness / Contrast / Color, the 8-bit HSV hue shift of
// torchvision's PIL path and the final grayscale, on uint8 [B, H, W, 3] in place, each image with its own factors and
// its own order of the ops (include/clipmi.h clipmi_color_u8; tests/color_ref.py restates the arithmetic in numpy and
// tests/test_cpu_color.py pins that to PIL).  It runs after clipmi_resize_crop_u8, where a torchvision user puts
// ColorJitter: after the resize, the window and the flip.
//
// Bit-exact, so every float operation below is the one PIL's C code performs, in its width:
//   * Image.blend: float32 d + a * float32(x - d), the product and the sum rounded separately.  Contraction is off
//     for the whole file (a fused multiply-add rounds once and differs in thousands of the 65,536 byte pairs), and
//     where PIL's C promotes to double the double is written out.
//   * the float32 divisions of RGB -> HSV are IEEE divisions (hipcc's default; the v_div_scale / v_div_fmas /
//     v_div_fixup sequence in the ISA, not a reciprocal multiply).
//   * the contrast mean is an integer: floor((2 sum L + n) / (2n)) == int(mean + 0.5).
//
// Two launches whatever B is.  Pass 1 (images with a contrast only): every pixel through the ops before the contrast
// in registers, its luma summed as integers: a wave reduction, then one atomic add per wave into a uint32 per
// image, so the sum does not depend on the order of the adds.  Pass 2: every pixel through its image's whole list
// with the mean from pass 1, then the grayscale, stored in place.  The image is the grid's second dimension: the op
// list is wave-uniform and its branches are scalar.
//
// Addressing: an image's base is images + b * H * W * 3, of any alignment when H * W * 3 is no multiple of 4.  Pixel
// p sits at base + 3p, which is 4-byte aligned exactly when p == base (mod 4); from the first such pixel on, every
// group of four pixels is three aligned dwords.  The up to three pixels before it and after the last whole group go
// byte by byte: nothing outside the image is read or written.
#include "common.h"
#include "internal.h"
#include <cmath>
#include <vector>

#pragma clang fp contract(off)

namespace {

enum { OP_END = 0, OP_BRIGHTNESS = 1, OP_CONTRAST = 2, OP_SATURATION = 3, OP_HUE = 4 };
constexpr int64_t COLOR_MAX_PIXELS = (int64_t)1 << 24;  // 255 * 2^24 < 2^32: the luma sum fits uint32
// Blocks per image; the kernels stride over the rest.  The grid is 32 x B blocks of 256 threads: a training batch
// (B >= 8) fills the 256 CUs; above 32768 pixels (S = 224: 50176) threads take more than one group.
constexpr int COLOR_MAX_BLOCKS = 32;

struct ColorRec {  // 32 bytes, one per image, in the workspace
  float brightness, contrast, saturation;
  int32_t hue_shift;
  int32_t order;       // the caller's nibbles
  int32_t gray;
  int32_t has_contrast;
  uint32_t sum;        // pass 1's luma sum; uploaded as 0
};
static_assert(sizeof(ColorRec) == 32, "ColorRec layout");

__device__ __forceinline__ int luma(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

// Image.blend per byte.  PIL truncates without a clip when 0 <= a <= 1; there the clip below never acts: a * (x - d)
// rounds to something between 0 and x - d, so the sum lies between d and x before and after its rounding.
__device__ __forceinline__ int blend(int d, int x, float a) {
  const float prod = a * (float)(x - d);
  const float t = (float)d + prod;
  return t <= 0.f ? 0 : t >= 255.f ? 255 : (int)t;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }

// PIL Convert.c rgb2hsv_row, the hue shift, hsv2rgb_row
__device__ __forceinline__ void hue_shift(int& r, int& g, int& b, int shift) {
  const int mx = max(r, max(g, b)), mn = min(r, min(g, b));
  int H = 0, S = 0;
  const int V = mx;
  if (mx != mn) {
    const float cr = (float)(mx - mn);
    const float s = cr / (float)mx;
    const float rc = (float)(mx - r) / cr, gc = (float)(mx - g) / cr, bc = (float)(mx - b) / cr;
    float h;
    if (r == mx) h = bc - gc;
    else if (g == mx) h = (float)((2.0 + (double)rc) - (double)bc);
    else h = (float)((4.0 + (double)gc) - (double)rc);
    const double w = (double)h / 6.0 + 1.0;  // in [5/6, 11/6]: fmod(w, 1.0) is w - floor(w), exactly
    h = (float)(w - floor(w));
    H = clip8((int)((double)h * 255.0));
    S = clip8((int)((double)s * 255.0));
  }
  H = (H + shift) & 255;
  if (S == 0) {
    r = g = b = V;
    return;
  }
  const double x = (double)(float)H * 6.0 / 255.0;
  const double fi = floor(x);
  const double f = (double)(float)(x - fi);
  const double fs = (double)(float)((double)S / 255.0);
  const double v = (double)V;
  const int p = clip8((int)round(v * (1.0 - fs)));
  const int q = clip8((int)round(v * (1.0 - fs * f)));
  const int t = clip8((int)round(v * (1.0 - fs * (1.0 - f))));
  switch ((int)fi % 6) {
    case 0: r = V, g = t, b = p; break;
    case 1: r = q, g = V, b = p; break;
    case 2: r = p, g = V, b = t; break;
    case 3: r = p, g = q, b = V; break;
    case 4: r = t, g = p, b = V; break;
    default: r = V, g = p, b = q; break;
  }
}

// One pixel through the image's list.  PRE: stop in front of the contrast (pass 1).  Every branch is on the record,
// which is the same for the whole block.
template <bool PRE>
__device__ __forceinline__ void run_ops(int& r, int& g, int& b, const ColorRec& c, int mean) {
  int order = c.order;
  for (int k = 0; k < 4; ++k, order >>= 4) {
    const int op = order & 15;
    if (op == OP_END) break;
    if (op == OP_BRIGHTNESS) {
      r = blend(0, r, c.brightness), g = blend(0, g, c.brightness), b = blend(0, b, c.brightness);
    } else if (op == OP_CONTRAST) {
      if (PRE) break;
      r = blend(mean, r, c.contrast), g = blend(mean, g, c.contrast), b = blend(mean, b, c.contrast);
    } else if (op == OP_SATURATION) {
      const int l = luma(r, g, b);
      r = blend(l, r, c.saturation), g = blend(l, g, c.saturation), b = blend(l, b, c.saturation);
    } else {
      hue_shift(r, g, b, c.hue_shift);
    }
  }
  if (!PRE && c.gray) r = g = b = luma(r, g, b);
}

// The pixels of one image as this thread sees them: `head` single pixels, then whole groups of four at aligned
// dwords, then `tail` single pixels.
struct Span {
  uint8_t* base;
  int64_t head, groups, tail;
};
__device__ __forceinline__ Span span_of(uint8_t* images, int b, int64_t n) {
  Span s;
  s.base = images + (int64_t)b * n * 3;
  s.head = (int64_t)((uintptr_t)s.base & 3);
  if (s.head > n) s.head = n;
  s.groups = (n - s.head) >> 2;
  s.tail = n - s.head - s.groups * 4;
  return s;
}
// the single pixels go to block 0: thread t takes head pixel t, thread 64 + t takes tail pixel t (-1: none)
__device__ __forceinline__ int64_t single_pixel(const Span& s) {
  if (blockIdx.x != 0) return -1;
  const int t = threadIdx.x;
  if (t < s.head) return t;
  if (t >= 64 && t - 64 < s.tail) return s.head + s.groups * 4 + (t - 64);
  return -1;
}

__device__ __forceinline__ void unpack4(uint32_t w0, uint32_t w1, uint32_t w2, int r[4], int g[4], int b[4]) {
  r[0] = w0 & 255, g[0] = (w0 >> 8) & 255, b[0] = (w0 >> 16) & 255, r[1] = w0 >> 24;
  g[1] = w1 & 255, b[1] = (w1 >> 8) & 255, r[2] = (w1 >> 16) & 255, g[2] = w1 >> 24;
  b[2] = w2 & 255, r[3] = (w2 >> 8) & 255, g[3] = (w2 >> 16) & 255, b[3] = w2 >> 24;
}

// pass 1: sum over the image of luma(pixel after the ops before the contrast)
__global__ __launch_bounds__(256) void color_sum_kernel(const uint8_t* images, ColorRec* recs, int64_t n) {
  const int b = blockIdx.y;
  const ColorRec c = recs[b];
  if (!c.has_contrast) return;
  const Span s = span_of(const_cast<uint8_t*>(images), b, n);
  uint32_t acc = 0;
  const uint32_t* words = (const uint32_t*)(s.base + s.head * 3);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.groups; i += (int64_t)gridDim.x * 256) {
    int r[4], g[4], bl[4];
    unpack4(words[i * 3], words[i * 3 + 1], words[i * 3 + 2], r, g, bl);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      run_ops<true>(r[j], g[j], bl[j], c, 0);
      acc += (uint32_t)luma(r[j], g[j], bl[j]);
    }
  }
  const int64_t p = single_pixel(s);
  if (p >= 0) {
    int r = s.base[p * 3], g = s.base[p * 3 + 1], bl = s.base[p * 3 + 2];
    run_ops<true>(r, g, bl, c, 0);
    acc += (uint32_t)luma(r, g, bl);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += (uint32_t)__shfl_xor((int)acc, o, 64);
  if ((threadIdx.x & 63) == 0 && acc != 0) atomicAdd(&recs[b].sum, acc);
}

// pass 2: the whole list and the grayscale, in place
__global__ __launch_bounds__(256) void color_apply_kernel(uint8_t* images, const ColorRec* recs, int64_t n) {
  const int b = blockIdx.y;
  const ColorRec c = recs[b];
  if ((c.order & 15) == OP_END && !c.gray) return;  // nothing to do: the bytes are not touched
  const int mean = c.has_contrast ? (int)((2 * (uint64_t)c.sum + (uint64_t)n) / (2 * (uint64_t)n)) : 0;
  const Span s = span_of(images, b, n);
  uint32_t* words = (uint32_t*)(s.base + s.head * 3);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < s.groups; i += (int64_t)gridDim.x * 256) {
    int r[4], g[4], bl[4];
    unpack4(words[i * 3], words[i * 3 + 1], words[i * 3 + 2], r, g, bl);
#pragma unroll
    for (int j = 0; j < 4; ++j) run_ops<false>(r[j], g[j], bl[j], c, mean);
    words[i * 3] = (uint32_t)r[0] | (uint32_t)g[0] << 8 | (uint32_t)bl[0] << 16 | (uint32_t)r[1] << 24;
    words[i * 3 + 1] = (uint32_t)g[1] | (uint32_t)bl[1] << 8 | (uint32_t)r[2] << 16 | (uint32_t)g[2] << 24;
    words[i * 3 + 2] = (uint32_t)bl[2] | (uint32_t)r[3] << 8 | (uint32_t)g[3] << 16 | (uint32_t)bl[3] << 24;
  }
  const int64_t p = single_pixel(s);
  if (p >= 0) {
    int r = s.base[p * 3], g = s.base[p * 3 + 1], bl = s.base[p * 3 + 2];
    run_ops<false>(r, g, bl, c, mean);
    s.base[p * 3] = (uint8_t)r, s.base[p * 3 + 1] = (uint8_t)g, s.base[p * 3 + 2] = (uint8_t)bl;
  }
}

int color_bad(const char* who, int b, const char* what) {
  return clipmi_invalid(std::string(who) + ": item " + std::to_string(b) + ": " + what);
}

// Validate the caller's items and derive the launch records.
int color_plan(const char* who, const clipmi_color_item* items, int B, int H, int W, std::vector<ColorRec>& recs) {
  if (B < 0) return clipmi_invalid(std::string(who) + ": B < 0");
  if (H < 1 || W < 1) return clipmi_invalid(std::string(who) + ": H, W must be >= 1");
  if ((int64_t)H * W > COLOR_MAX_PIXELS)
    return clipmi_invalid(std::string(who) + ": H * W must be <= 2^24 (the 32-bit luma sum of the contrast mean)");
  if (B > 0 && !items) return clipmi_invalid(std::string(who) + ": null items");
  recs.resize(B);
  for (int b = 0; b < B; ++b) {
    const clipmi_color_item it = items[b];
    const float fs[3] = {it.brightness, it.contrast, it.saturation};
    for (float f : fs)
      if (!std::isfinite(f) || f < 0.f) return color_bad(who, b, "blend factors must be finite and >= 0");
    if (it.hue_shift < 0 || it.hue_shift > 255) return color_bad(who, b, "hue_shift must be in [0, 255]");
    if (it.gray != 0 && it.gray != 1) return color_bad(who, b, "gray must be 0 or 1");
    uint32_t order = (uint32_t)it.order;
    if (order >> 16) return color_bad(who, b, "order holds more than four op codes");
    unsigned seen = 0;
    bool ended = false;
    for (int k = 0; k < 4; ++k, order >>= 4) {
      const unsigned op = order & 15;
      if (op == OP_END) {
        ended = true;
        continue;
      }
      if (ended) return color_bad(who, b, "op code after the end of the list");
      if (op > OP_HUE) return color_bad(who, b, "unknown op code");
      if (seen & (1u << op)) return color_bad(who, b, "op code repeated");
      seen |= 1u << op;
    }
    ColorRec& r = recs[b];
    r.brightness = it.brightness, r.contrast = it.contrast, r.saturation = it.saturation;
    r.hue_shift = it.hue_shift, r.order = it.order, r.gray = it.gray;
    r.has_contrast = (seen >> OP_CONTRAST) & 1;
    r.sum = 0;
  }
  return CLIPMI_OK;
}

int64_t color_ws_bytes(int B) { return ((int64_t)B * sizeof(ColorRec) + 255) & ~(int64_t)255; }

}  // namespace

extern "C" int64_t clipmi_color_u8_ws(const clipmi_color_item* items, int B, int H, int W) {
  std::vector<ColorRec> recs;
  const int st = color_plan(__func__, items, B, H, W, recs);
  if (st != CLIPMI_OK) return st;
  return B == 0 ? 0 : color_ws_bytes(B);
}

extern "C" int clipmi_color_u8(void* stream, uint8_t* images, const clipmi_color_item* items, int B, int H, int W,
                               void* ws, int64_t ws_bytes) {
  // the records are the library's own and outlive the call (the upload below is ordered on the stream)
  static thread_local std::vector<ColorRec> recs;
  CLIPMI_TRY(color_plan(__func__, items, B, H, W, recs));
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(B <= 65535, "B must be <= 65535 (the grid's second dimension)");
  CLIPMI_REQUIRE(images, "null images");
  CLIPMI_REQUIRE(ws && ws_bytes >= color_ws_bytes(B), "workspace too small");
  CLIPMI_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  ColorRec* drecs = (ColorRec*)ws;
  CLIPMI_HIP(hipMemcpyAsync(drecs, recs.data(), (size_t)B * sizeof(ColorRec), hipMemcpyHostToDevice, s));
  const int64_t n = (int64_t)H * W;
  const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(((n >> 2) + 255) / 256, COLOR_MAX_BLOCKS));
  const dim3 grid((unsigned)blocks, (unsigned)B);
  hipLaunchKernelGGL(color_sum_kernel, grid, dim3(256), 0, s, images, drecs, n);
  hipLaunchKernelGGL(color_apply_kernel, grid, dim3(256), 0, s, images, drecs, n);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
