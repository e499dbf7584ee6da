// Ragged input step: B channels-last RGB uint8 images of different sizes, packed in one buffer, each with an
// integer crop box and a flip bit -> uint8 [B, S, S, 3] for clipmi_im2col_u8 (dataset.py:152-164 hands the
// processor one PIL image at a time; a random-resized-crop is the same resize of another box).
//
// Semantics: crop, then PIL Image.resize(BICUBIC) of the crop, then the centre window (mode 0) and the flip:
// the arithmetic of data.hip's resize (fp64 tap weights without contraction -> 22-bit fixed point, a horizontal
// 8-bit pass, then a vertical one; oracle/resize_ref.py) with the crop's length in place of the image's, so taps
// clamp at the crop's edges.  Only what the S x S output reads is computed: the S output columns' coefficients
// (at coordinates left .. left + S - 1 of the resized width), the source rows the S output rows' vertical taps
// reach, and the S x S window itself.  A pass whose size does not change is a one-tap table entry (weight 2^22:
// (2^21 + 2^22 v) >> 22 == v), so every image takes the same two passes.
//
// Three launches whatever B is: coefficients (both axes, every image), horizontal pass, vertical pass.  The host
// validates the caller's items, derives one RcImage per image and uploads those into the workspace; the kernels
// read no table of the caller's.
#include "common.h"
#include "internal.h"
#include <cmath>
#include <vector>

namespace {

constexpr int RC_PREC = 22;
constexpr int RC_MAX_SCALE = 32;   // largest downscale per axis: ceil(2 * 32) * 2 + 1 = 129 taps
constexpr int RC_MAX_S = 16384;    // S * edge stays exact in fp64 (shortest-edge size) and in 32-bit row counts

struct RcImage {    // 64 bytes, one per image, in the workspace
  int64_t src;      // byte offset of the crop's first pixel in the packed buffer
  int64_t pitch;    // bytes per image row
  int64_t tmp;      // byte offset of this image's rows [nr, S, 3] in the intermediate
  int32_t cw, ch;   // crop size: the resize's input size
  int32_t ow, oh;   // size of the whole resized crop
  int32_t left, top;  // the S x S window's origin in it
  int32_t r0, nr;   // crop rows [r0, r0 + nr) the vertical taps of the S output rows reach
  int32_t flip, pad_;
};
static_assert(sizeof(RcImage) == 64, "RcImage layout");

__host__ __device__ inline double rc_bicubic(double x) {
#pragma clang fp contract(off)
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
  if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
  return 0.0;
}

// taps [lo, lo + n) of output coordinate xx (PIL precompute_coeffs); host and device run the same IEEE operations
__host__ __device__ inline void rc_taps(int in_size, int out_size, int xx, int* lo, int* n, double* center,
                                        double* ss) {
#pragma clang fp contract(off)
  const double scale = (double)in_size / (double)out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = 2.0 * filterscale;
  *ss = 1.0 / filterscale;
  *center = (xx + 0.5) * scale;
  int xmin = (int)(*center - support + 0.5);
  if (xmin < 0) xmin = 0;
  int xmax = (int)(*center + support + 0.5);
  if (xmax > in_size) xmax = in_size;
  *lo = xmin;
  *n = xmax - xmin;
}

// one thread per (axis, image, output coordinate): [lo, n, k_0 .. k_{ksize-1}] int32, as resize_coeffs_kernel
__global__ __launch_bounds__(256) void rc_coeffs_kernel(const RcImage* recs, int B, int S, int kw, int kh, int* htab,
                                                        int* vtab) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t per = (int64_t)B * S;
  if (i >= 2 * per) return;
  const bool vert = i >= per;
  const int64_t j = vert ? i - per : i;
  const int b = (int)(j / S), o = (int)(j - (int64_t)b * S);
  const RcImage r = recs[b];
  const int in_size = vert ? r.ch : r.cw, out_size = vert ? r.oh : r.ow, ksize = vert ? kh : kw;
  const int xx = (vert ? r.top : r.left) + o;
  int* t = (vert ? vtab : htab) + j * (2 + ksize);
  if (in_size == out_size) {  // PIL skips the pass: the pixel itself
    t[0] = xx;
    t[1] = 1;
    t[2] = 1 << RC_PREC;
    for (int x = 1; x < ksize; ++x) t[2 + x] = 0;
    return;
  }
  int xmin, xmax;
  double center, ss;
  rc_taps(in_size, out_size, xx, &xmin, &xmax, &center, &ss);
  if (xmax > ksize) xmax = ksize;  // never taken: PIL's ksize bounds the tap count
  double ww = 0.0;
  for (int x = 0; x < xmax; ++x) ww += rc_bicubic((x + xmin - center + 0.5) * ss);
  for (int x = 0; x < ksize; ++x) {
    int k = 0;
    if (x < xmax) {
      double w = rc_bicubic((x + xmin - center + 0.5) * ss);
      if (ww != 0.0) w /= ww;
      k = w < 0 ? (int)(-0.5 + w * (double)(1 << RC_PREC)) : (int)(0.5 + w * (double)(1 << RC_PREC));
    }
    t[2 + x] = k;
  }
  t[0] = xmin;
  t[1] = xmax;
}

__device__ __forceinline__ uint8_t rc_clip8(int acc) {
  const int v = acc >> RC_PREC;
  return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// horizontal pass: block column b = image, one thread per (row of [r0, r0 + nr), output column), grid-strided
__global__ __launch_bounds__(256) void rc_horiz_kernel(const uint8_t* packed, const RcImage* recs, const int* htab,
                                                       int kw, int S, uint8_t* tmp) {
  const int b = blockIdx.x;
  const RcImage r = recs[b];
  const int64_t total = (int64_t)r.nr * S;
  const int* tb = htab + (int64_t)b * S * (2 + kw);
  const uint8_t* img = packed + r.src;
  uint8_t* dst = tmp + r.tmp;
  for (int64_t i = (int64_t)blockIdx.y * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.y * 256) {
    const int row = (int)(i / S), xo = (int)(i - (int64_t)row * S);
    const int* t = tb + (int64_t)xo * (2 + kw);
    const int lo = t[0], n = t[1];
    const uint8_t* src = img + (int64_t)(r.r0 + row) * r.pitch + (int64_t)lo * 3;
    int a0 = 1 << (RC_PREC - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j) {
      const int k = t[2 + j];
      a0 += k * (int)src[0];
      a1 += k * (int)src[1];
      a2 += k * (int)src[2];
      src += 3;
    }
    uint8_t* d = dst + i * 3;
    d[0] = rc_clip8(a0);
    d[1] = rc_clip8(a1);
    d[2] = rc_clip8(a2);
  }
}

// vertical pass over the intermediate + the flip: one thread per output pixel, grid-strided
__global__ __launch_bounds__(256) void rc_vert_kernel(const uint8_t* tmp, const RcImage* recs, const int* vtab, int kh,
                                                      int B, int S, uint8_t* out) {
  const int64_t total = (int64_t)B * S * S;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int xo = (int)(i % S);
    const int64_t q = i / S;  // b * S + yo
    const int b = (int)(q / S);
    const RcImage r = recs[b];
    const int* t = vtab + q * (2 + kh);
    const int n = t[1];
    int row = t[0] - r.r0;  // in [0, nr - n] by the host's row range (the same rc_taps)
    const uint8_t* src = tmp + r.tmp + (int64_t)xo * 3;
    const int64_t step = (int64_t)S * 3;
    int a0 = 1 << (RC_PREC - 1), a1 = a0, a2 = a0;
    for (int j = 0; j < n; ++j, ++row) {
      const int rr = row < 0 ? 0 : row >= r.nr ? r.nr - 1 : row;  // never outside the image's rows
      const uint8_t* p = src + rr * step;
      const int k = t[2 + j];
      a0 += k * (int)p[0];
      a1 += k * (int)p[1];
      a2 += k * (int)p[2];
    }
    const int xd = r.flip ? S - 1 - xo : xo;
    uint8_t* d = out + (q * S + xd) * 3;
    d[0] = rc_clip8(a0);
    d[1] = rc_clip8(a1);
    d[2] = rc_clip8(a2);
  }
}

int rc_ksize(int in, int out) {
  if (in == out) return 1;
  const double scale = (double)in / (double)out;
  const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
  return (int)ceil(support) * 2 + 1;
}
int64_t rc_al(int64_t x) { return (x + 255) & ~(int64_t)255; }

struct RcPlan {
  std::vector<RcImage> recs;
  int kw = 1, kh = 1;     // the batch's largest tap counts
  int max_nr = 0;         // and largest horizontal-pass row count
  int64_t tmp_bytes = 0;  // the intermediate
  int64_t htab_off() const { return rc_al((int64_t)recs.size() * sizeof(RcImage)); }
  int64_t vtab_off(int S) const { return htab_off() + rc_al((int64_t)recs.size() * S * (2 + kw) * 4); }
  int64_t tmp_off(int S) const { return vtab_off(S) + rc_al((int64_t)recs.size() * S * (2 + kh) * 4); }
  int64_t bytes(int S) const { return tmp_off(S) + rc_al(tmp_bytes); }
};

int rc_bad(const char* who, int b, const char* what) {
  return clipmi_invalid(std::string(who) + ": item " + std::to_string(b) + ": " + what);
}

// Validate the items (packed_bytes < 0: size unknown, the workspace query) and derive the launch records.
int rc_plan(const char* who, const clipmi_image_item* items, int B, int S, int mode, int64_t packed_bytes,
            RcPlan& p) {
  if (S < 1 || S > RC_MAX_S)
    return clipmi_invalid(std::string(who) + ": S must be in [1, " + std::to_string(RC_MAX_S) + "]");
  if (mode != 0 && mode != 1) return clipmi_invalid(std::string(who) + ": mode must be 0 (processor) or 1 (square)");
  if (B < 0) return clipmi_invalid(std::string(who) + ": B < 0");
  if (B > 0 && !items) return clipmi_invalid(std::string(who) + ": null items");
  p.recs.resize(B);
  for (int b = 0; b < B; ++b) {
    const clipmi_image_item it = items[b];
    if (it.h < 1 || it.w < 1) return rc_bad(who, b, "h, w must be >= 1");
    if (it.cw < 1 || it.ch < 1) return rc_bad(who, b, "empty crop box");
    if (it.x0 < 0 || it.y0 < 0 || it.x0 > it.w - it.cw || it.y0 > it.h - it.ch)
      return rc_bad(who, b, "crop box outside the image");
    if (it.flip != 0 && it.flip != 1) return rc_bad(who, b, "flip must be 0 or 1");
    if (it.offset < 0) return rc_bad(who, b, "negative offset");
    if (packed_bytes >= 0 && (it.offset > packed_bytes || (int64_t)it.h * it.w > (packed_bytes - it.offset) / 3))
      return rc_bad(who, b, "image outside the packed buffer");
    int64_t ow = S, oh = S;
    if (mode == 0) {  // shortest edge -> S, long edge -> int(S * long / short) (fp64 division, as the processor)
      if (it.cw <= it.ch) oh = (int64_t)((double)((int64_t)S * it.ch) / (double)it.cw);
      else ow = (int64_t)((double)((int64_t)S * it.cw) / (double)it.ch);
    }
    if (ow > INT32_MAX || oh > INT32_MAX) return rc_bad(who, b, "resized long edge does not fit 32 bits");
    if (it.cw > RC_MAX_SCALE * ow || it.ch > RC_MAX_SCALE * oh)
      return rc_bad(who, b, "downscale above 32x (129 taps) is not supported");
    RcImage& r = p.recs[b];
    r.pitch = (int64_t)it.w * 3;
    r.src = it.offset + (int64_t)it.y0 * r.pitch + (int64_t)it.x0 * 3;
    r.cw = it.cw, r.ch = it.ch, r.ow = (int)ow, r.oh = (int)oh;
    r.left = (int)((ow - S) / 2), r.top = (int)((oh - S) / 2);
    r.flip = it.flip, r.pad_ = 0;
    if (r.ch == r.oh) {
      r.r0 = r.top, r.nr = S;
    } else {
      int lo0, n0, lo1, n1;
      double c, ss;
      rc_taps(r.ch, r.oh, r.top, &lo0, &n0, &c, &ss);
      rc_taps(r.ch, r.oh, r.top + S - 1, &lo1, &n1, &c, &ss);
      r.r0 = lo0, r.nr = lo1 + n1 - lo0;
    }
    r.tmp = p.tmp_bytes;
    p.tmp_bytes += ((int64_t)r.nr * S * 3 + 15) & ~(int64_t)15;
    p.kw = std::max(p.kw, rc_ksize(r.cw, r.ow));
    p.kh = std::max(p.kh, rc_ksize(r.ch, r.oh));
    p.max_nr = std::max(p.max_nr, r.nr);
  }
  return CLIPMI_OK;
}

}  // namespace

extern "C" int64_t clipmi_resize_crop_u8_ws(const clipmi_image_item* items, int B, int S, int mode) {
  RcPlan p;
  const int st = rc_plan(__func__, items, B, S, mode, -1, p);
  if (st != CLIPMI_OK) return st;
  return B == 0 ? 0 : p.bytes(S);
}

extern "C" int clipmi_resize_crop_u8(void* stream, const uint8_t* packed, int64_t packed_bytes,
                                     const clipmi_image_item* items, int B, uint8_t* out, int S, int mode, void* ws,
                                     int64_t ws_bytes) {
  CLIPMI_REQUIRE(packed_bytes >= 0, "packed_bytes < 0");
  // the records are the library's own and outlive the call (the upload below is ordered on the stream)
  static thread_local RcPlan p;
  p.kw = p.kh = 1, p.max_nr = 0, p.tmp_bytes = 0;
  CLIPMI_TRY(rc_plan(__func__, items, B, S, mode, packed_bytes, p));
  if (B == 0) return CLIPMI_OK;
  CLIPMI_REQUIRE(packed && out, "null packed / out");
  CLIPMI_REQUIRE(ws && ws_bytes >= p.bytes(S), "workspace too small");
  CLIPMI_REQUIRE(((uintptr_t)ws & 15) == 0, "workspace must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  char* w = (char*)ws;
  RcImage* recs = (RcImage*)w;
  int* htab = (int*)(w + p.htab_off());
  int* vtab = (int*)(w + p.vtab_off(S));
  uint8_t* tmp = (uint8_t*)(w + p.tmp_off(S));
  CLIPMI_HIP(hipMemcpyAsync(recs, p.recs.data(), (size_t)B * sizeof(RcImage), hipMemcpyHostToDevice, s));
  const int64_t nc = 2 * (int64_t)B * S;
  hipLaunchKernelGGL(rc_coeffs_kernel, dim3((unsigned)((nc + 255) / 256)), dim3(256), 0, s, recs, B, S, p.kw, p.kh,
                     htab, vtab);
  const int64_t chunks = ((int64_t)p.max_nr * S + 255) / 256;
  hipLaunchKernelGGL(rc_horiz_kernel, dim3((unsigned)B, (unsigned)std::min<int64_t>(chunks, 1024)), dim3(256), 0, s,
                     packed, recs, htab, p.kw, S, tmp);
  const int64_t nv = ((int64_t)B * S * S + 255) / 256;
  hipLaunchKernelGGL(rc_vert_kernel, dim3((unsigned)std::min<int64_t>(nv, 1 << 20)), dim3(256), 0, s, tmp, recs, vtab,
                     p.kh, B, S, out);
  CLIPMI_CHECK_LAUNCH();
  return CLIPMI_OK;
}
