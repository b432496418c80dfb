// Device-side RandAugment of the RSP v2 pipeline (Pretraining_v2/models/randaugment.py:38-190): the twelve Pillow ops of its pool
// on a uint8 batch in HBM, one op SLOT of a whole batch per call -- every image carries its own op code and parameters, an image
// whose code is COPY passes through unchanged.  The host makes every random draw (ssl_cr_histo_amd/augment.py); the kernels are
// deterministic and reproduce Pillow byte for byte: same number formats, same operation order, and no multiply-add contraction
// (this file is built with -ffp-contract=off, and the roundings that matter are spelled with the _rn intrinsics besides).
//
//   augv2_stats_kernel   per image and channel a 256-bin histogram, per image the sum of L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16,
//                        for the images whose op needs them (contrast / autocontrast / equalize): LDS integer atomics per wave,
//                        then integer global adds -- exact and order-free, so the results stay bit-deterministic
//   augv2_lut_kernel     per image 3 x 256 bytes: ImageOps.autocontrast / ImageOps.equalize, and -- a blend against a CONSTANT
//                        degenerate image being a function of the byte alone -- ImageEnhance.Brightness / Contrast; for a
//                        translated image the column and row index tables of Pillow's scale path instead
//   augv2_apply_kernel   reads src once and writes dst once, either layout on either side: LUT apply, ImageEnhance.Color (blend
//                        with L), ImageEnhance.Sharpness (blend with ImageFilter.SMOOTH), the nearest gathers (rotate's
//                        fixed-point walk, translate's index tables) and the float64 bicubic gather (shear)
// All three are HBM-bound byte kernels (3 B in + 3 B out per pixel and slot; the statistics pass reads 3 B more for the images
// that need it).  The point ops move 16 pixels per thread as 16-byte words when H*W is a multiple of 16; the neighbourhood ops
// write 4 pixels per thread and gather their taps through the L1.
//
// The two histopathology ops of the pool, hed and hsv, run IN PLACE on the slot's output (sslcr_randaug_v2_colour):
//   augv2c_sum_kernel    per HED image the sum of its 3 H W bytes (16-byte words, wave shuffles, one integer global add per wave):
//                        the mean of HedColorAugmenter.transform's cutoff test, exact and order-free
//   augv2c_apply_kernel  4 pixels per thread as dwords of the byte planes (CHW) or one 12-byte group (HWC), no LDS.  hsv is float64
//                        (+ - x / floor and an exact remainder only: bit-reproducible), hed float32 with the accurate logf / expf
#include "kernels.hpp"
#include "px_bytes.hpp"    // Px, load_px, store_px, byte_of

namespace sslcr {
namespace {

__device__ inline bool needs_hist(int op) { return op == SSLCR_AUGV2_AUTOCONTRAST || op == SSLCR_AUGV2_EQUALIZE; }
__device__ inline bool needs_stats(int op) { return op == SSLCR_AUGV2_CONTRAST || needs_hist(op); }
__device__ inline bool uses_lut(int op) { return op == SSLCR_AUGV2_BRIGHTNESS || needs_stats(op); }
__device__ inline bool uses_factor(int op) {
  return op == SSLCR_AUGV2_BRIGHTNESS || op == SSLCR_AUGV2_CONTRAST || op == SSLCR_AUGV2_COLOR || op == SSLCR_AUGV2_SHARPNESS;
}

// Image.blend(degenerate, image, f) for one byte: float32 product, float32 sum, clip, truncate.  For 0 <= f <= 1 Pillow skips the
// clip; t then lies between the two bytes, where the clip is the identity.
__device__ inline uint32_t blend8(int d, int p, float f) {
  const float t = __fadd_rn((float)d, __fmul_rn(f, (float)(p - d)));
  return t <= 0.f ? 0u : t >= 255.f ? 255u : (uint32_t)(int)t;
}

__device__ inline uint32_t luma8(uint32_t r, uint32_t g, uint32_t b) { return (19595u * r + 38470u * g + 7471u * b + 0x8000u) >> 16; }

__device__ inline int tap(const uint8_t* img, int hwc, size_t hw, int W, int x, int y, int c) {
  const size_t p = (size_t)y * W + x;
  return img[hwc ? p * 3 + c : c * hw + p];
}

// Pillow's BICUBIC macro, float64, evaluated in its order
__device__ inline double cubic(double v1, double v2, double v3, double v4, double d) {
  const double p2 = __dadd_rn(-v1, v3);
  const double p3 = __dadd_rn(__dadd_rn(__dmul_rn(2.0, __dadd_rn(v1, -v2)), v3), -v4);
  const double p4 = __dadd_rn(__dadd_rn(__dadd_rn(-v1, v2), -v3), v4);
  return __dadd_rn(v2, __dmul_rn(d, __dadd_rn(p2, __dmul_rn(d, __dadd_rn(p3, __dmul_rn(d, p4))))));
}

}  // namespace

__global__ __launch_bounds__(256) void augv2_stats_kernel(const sslcr_augv2_desc a, const int vec) {
  const int n = blockIdx.y;
  const int op = a.op[n];
  if (!needs_stats(op)) return;                      // block-uniform
  __shared__ uint32_t h[4][3][256];                  // one histogram set per wave: a flat channel does not serialise the block
  __shared__ unsigned long long ls[256];
  for (int i = threadIdx.x; i < 4 * 3 * 256; i += 256) (&h[0][0][0])[i] = 0;
  __syncthreads();
  const size_t hw = (size_t)a.H * a.W;
  const uint8_t* img = a.src + (size_t)n * 3 * hw;
  const size_t units = (hw + 15) / 16;
  const int wave = threadIdx.x >> 6;
  const bool hist = needs_hist(op);
  unsigned long long lsum = 0;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (size_t)gridDim.x * 256) {
    const size_t p0 = u * 16;
    const int cnt = hw - p0 < 16 ? (int)(hw - p0) : 16;
    Px<16> p;
    load_px<16>(p, img, a.src_hwc, hw, p0, cnt, vec);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      if (e < cnt) {
        const uint32_t r = byte_of(p.w[0][e >> 2], e & 3), g = byte_of(p.w[1][e >> 2], e & 3), b = byte_of(p.w[2][e >> 2], e & 3);
        if (hist) {
          atomicAdd(&h[wave][0][r], 1u);
          atomicAdd(&h[wave][1][g], 1u);
          atomicAdd(&h[wave][2][b], 1u);
        } else {
          lsum += luma8(r, g, b);
        }
      }
    }
  }
  __syncthreads();
  if (hist) {
    for (int i = threadIdx.x; i < 3 * 256; i += 256) {
      const uint32_t s = (&h[0][0][0])[i] + (&h[1][0][0])[i] + (&h[2][0][0])[i] + (&h[3][0][0])[i];
      if (s) atomicAdd(a.hist + (size_t)n * 768 + i, s);
    }
  } else {
    ls[threadIdx.x] = lsum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) ls[threadIdx.x] += ls[threadIdx.x + o];
      __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(a.lsum + n, ls[0]);
  }
}

// one workgroup per image, thread i builds entry i of the three tables
__global__ __launch_bounds__(256) void augv2_lut_kernel(const sslcr_augv2_desc a) {
  const int n = blockIdx.x;
  const int op = a.op[n];
  const int i = threadIdx.x;
  if (op == SSLCR_AUGV2_NEAREST_TABLE) {
    // Pillow's ImagingScaleAffine: the source coordinate starts at shift + 0.5 and grows by REPEATED addition of 1.0 (its rounding is
    // not that of shift + 0.5 + i), index = coordinate < 0 ? -1 : (int)coordinate.  One lane walks the columns, one the rows.
    if (!(a.shift && a.tab) || (i != 0 && i != 64)) return;
    const int len = i ? a.H : a.W;
    int32_t* t = a.tab + (size_t)n * (a.W + a.H) + (i ? a.W : 0);
    double o = __dadd_rn(a.shift[n * 2 + (i ? 1 : 0)], 0.5);
    for (int k = 0; k < len; ++k) {
      const int idx = o < 0.0 ? -1 : o >= (double)len ? -1 : (int)o;
      t[k] = idx;
      o = __dadd_rn(o, 1.0);
    }
    return;
  }
  if (!uses_lut(op) || !a.lut || (uses_factor(op) && !a.factor) || (needs_stats(op) && !(a.hist && a.lsum))) return;      // block-uniform
  uint8_t* lut = a.lut + (size_t)n * 768;
  if (!needs_hist(op)) {
    // brightness: the degenerate image is black.  contrast: the constant int(mean(L) + 0.5), the mean a float64 quotient
    int d = 0;
    if (op == SSLCR_AUGV2_CONTRAST) d = (int)((double)a.lsum[n] / (double)((size_t)a.H * a.W) + 0.5);
    const uint8_t v = (uint8_t)blend8(d, i, a.factor[n]);
    lut[i] = v; lut[256 + i] = v; lut[512 + i] = v;
    return;
  }
  __shared__ uint32_t h[3][256];
  __shared__ int lo[3], hi[3];
  __shared__ uint32_t step[3];
  for (int c = 0; c < 3; ++c) h[c][i] = a.hist[(size_t)n * 768 + c * 256 + i];
  __syncthreads();
  if (i < 3) {
    int l = -1, u = -1, nz = 0;
    uint32_t total = 0;
    for (int k = 0; k < 256; ++k)
      if (h[i][k]) { if (l < 0) l = k; u = k; ++nz; total += h[i][k]; }
    lo[i] = l; hi[i] = u;
    step[i] = nz <= 1 ? 0u : (total - h[i][u]) / 255u;     // equalize: (sum(histo) - histo[-1]) // 255 over the non-empty bins
  }
  __syncthreads();
  for (int c = 0; c < 3; ++c) {
    int v = i;
    if (op == SSLCR_AUGV2_AUTOCONTRAST) {
      if (hi[c] > lo[c]) {
        const double scale = 255.0 / (double)(hi[c] - lo[c]);
        const double offset = __dmul_rn((double)(-lo[c]), scale);
        v = (int)__dadd_rn(__dmul_rn((double)i, scale), offset);
        v = v < 0 ? 0 : v > 255 ? 255 : v;
      }
    } else if (step[c]) {
      uint32_t nn = step[c] / 2;
      for (int k = 0; k < i; ++k) nn += h[c][k];
      const uint32_t q = nn / step[c];
      v = q > 255u ? 255 : (int)q;
    }
    lut[c * 256 + i] = (uint8_t)v;
  }
}

__global__ __launch_bounds__(256) void augv2_apply_kernel(const sslcr_augv2_desc a, const int vec) {
  const int n = blockIdx.y;
  int op = a.op[n];
  // a code whose table the caller did not pass (ops_mask and op disagree) or an unknown code writes black instead of reading through NULL
  if ((op == SSLCR_AUGV2_NEAREST_FIXED && !a.fixed) || (op == SSLCR_AUGV2_NEAREST_TABLE && !(a.shift && a.tab)) ||
      (op == SSLCR_AUGV2_BICUBIC && !a.affine) || (uses_lut(op) && !a.lut) || (uses_factor(op) && !a.factor) || op > SSLCR_AUGV2_BICUBIC)
    op = SSLCR_AUGV2_BICUBIC + 1;
  const int H = a.H, W = a.W;
  const size_t hw = (size_t)H * W;
  const uint8_t* img = a.src + (size_t)n * 3 * hw;
  uint8_t* out = a.dst + (size_t)n * 3 * hw;
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, tstep = (size_t)gridDim.x * 256;

  if (op <= SSLCR_AUGV2_EQUALIZE) {                  // ---- point ops, 16 pixels per thread
    __shared__ uint8_t lut[768];
    const bool lut_op = uses_lut(op);
    if (lut_op) {
      for (int i = threadIdx.x; i < 768; i += 256) lut[i] = a.lut[(size_t)n * 768 + i];
      __syncthreads();
    }
    const float f = op == SSLCR_AUGV2_COLOR ? a.factor[n] : 0.f;
    const size_t units = (hw + 15) / 16;
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 16;
      const int cnt = hw - p0 < 16 ? (int)(hw - p0) : 16;
      Px<16> p;
      load_px<16>(p, img, a.src_hwc, hw, p0, cnt, vec);
      if (lut_op) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            uint32_t v = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) v |= (uint32_t)lut[c * 256 + byte_of(p.w[c][q], e)] << (8 * e);
            p.w[c][q] = v;
          }
      } else if (op == SSLCR_AUGV2_COLOR) {          // the degenerate image is L on all three channels
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          uint32_t v[3] = {0, 0, 0};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const uint32_t r = byte_of(p.w[0][q], e), g = byte_of(p.w[1][q], e), b = byte_of(p.w[2][q], e);
            const int l = (int)luma8(r, g, b);
            v[0] |= blend8(l, (int)r, f) << (8 * e);
            v[1] |= blend8(l, (int)g, f) << (8 * e);
            v[2] |= blend8(l, (int)b, f) << (8 * e);
          }
          p.w[0][q] = v[0]; p.w[1][q] = v[1]; p.w[2][q] = v[2];
        }
      }
      store_px<16>(p, out, a.dst_hwc, hw, p0, cnt, vec);
    }
    return;
  }

  // ---- neighbourhood ops: 4 output pixels per thread, taps gathered from src
  const float f = op == SSLCR_AUGV2_SHARPNESS ? a.factor[n] : 0.f;
  const float k1 = __fdiv_rn(1.f, 13.f), k5 = __fdiv_rn(5.f, 13.f);      // ImageFilter.SMOOTH: float32 (1 1 1 / 1 5 1 / 1 1 1) / 13
  int fx[6] = {0, 0, 0, 0, 0, 0};
  double af[6] = {0, 0, 0, 0, 0, 0};
  if (op == SSLCR_AUGV2_NEAREST_FIXED)
    for (int i = 0; i < 6; ++i) fx[i] = a.fixed[n * 6 + i];
  if (op == SSLCR_AUGV2_BICUBIC)
    for (int i = 0; i < 6; ++i) af[i] = a.affine[n * 6 + i];
  const size_t units = (hw + 3) / 4;
  for (size_t u = t0; u < units; u += tstep) {
    const size_t p0 = u * 4;
    const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
    Px<4> o;
    o.w[0][0] = o.w[1][0] = o.w[2][0] = 0;
    for (int e = 0; e < cnt; ++e) {
      const size_t p = p0 + e;
      const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
      uint32_t v[3] = {0, 0, 0};
      if (op == SSLCR_AUGV2_SHARPNESS) {
        if (x == 0 || y == 0 || x == W - 1 || y == H - 1) {            // the filter copies the one-pixel border; blend(p, p) = p
          for (int c = 0; c < 3; ++c) v[c] = tap(img, a.src_hwc, hw, W, x, y, c);
        } else {
          for (int c = 0; c < 3; ++c) {
            float ss = 0.5f;
            for (int j = 0; j < 3; ++j) {                               // row y+1, then y, then y-1; each tap sum left to right
              const int yy = y + 1 - j;
              const float kc = j == 1 ? k5 : k1;
              float t = __fmul_rn((float)tap(img, a.src_hwc, hw, W, x - 1, yy, c), k1);
              t = __fadd_rn(t, __fmul_rn((float)tap(img, a.src_hwc, hw, W, x, yy, c), kc));
              t = __fadd_rn(t, __fmul_rn((float)tap(img, a.src_hwc, hw, W, x + 1, yy, c), k1));
              ss = __fadd_rn(ss, t);
            }
            const int d = ss <= 0.f ? 0 : ss >= 255.f ? 255 : (int)ss;
            v[c] = blend8(d, tap(img, a.src_hwc, hw, W, x, y, c), f);
          }
        }
      } else if (op == SSLCR_AUGV2_BICUBIC) {
        double xin = __dadd_rn(__dadd_rn(__dmul_rn(af[0], x + 0.5), __dmul_rn(af[1], y + 0.5)), af[2]);
        double yin = __dadd_rn(__dadd_rn(__dmul_rn(af[3], x + 0.5), __dmul_rn(af[4], y + 0.5)), af[5]);
        if (!(xin < 0.0 || xin >= (double)W || yin < 0.0 || yin >= (double)H)) {
          xin -= 0.5; yin -= 0.5;
          const double xf = floor(xin), yf = floor(yin);
          const double dx = xin - xf, dy = yin - yf;
          const int x0 = (int)xf, y0 = (int)yf;
          int xs[4], ys[4];
          for (int k = 0; k < 4; ++k) {
            const int xx = x0 - 1 + k, yy = y0 - 1 + k;
            xs[k] = xx < 0 ? 0 : xx >= W ? W - 1 : xx;
            ys[k] = yy < 0 ? 0 : yy >= H ? H - 1 : yy;
          }
          for (int c = 0; c < 3; ++c) {
            double r[4];
            for (int k = 0; k < 4; ++k)
              r[k] = cubic((double)tap(img, a.src_hwc, hw, W, xs[0], ys[k], c), (double)tap(img, a.src_hwc, hw, W, xs[1], ys[k], c),
                           (double)tap(img, a.src_hwc, hw, W, xs[2], ys[k], c), (double)tap(img, a.src_hwc, hw, W, xs[3], ys[k], c), dx);
            const double s = cubic(r[0], r[1], r[2], r[3], dy);
            v[c] = s <= 0.0 ? 0u : s >= 255.0 ? 255u : (uint32_t)(int)s;      // no rounding offset
          }
        }
      } else {
        int xs, ys;
        if (op == SSLCR_AUGV2_NEAREST_FIXED) {                         // Pillow's 16.16 walk; the host checked the 16-bit range
          xs = (fx[2] + fx[0] * x + fx[1] * y) >> 16;
          ys = (fx[5] + fx[3] * x + fx[4] * y) >> 16;
        } else if (op == SSLCR_AUGV2_NEAREST_TABLE) {                   // per-image column / row tables, -1 = outside
          xs = a.tab[(size_t)n * (W + H) + x];
          ys = a.tab[(size_t)n * (W + H) + W + y];
        } else {
          xs = ys = -1;
        }
        if (xs >= 0 && xs < W && ys >= 0 && ys < H)
          for (int c = 0; c < 3; ++c) v[c] = tap(img, a.src_hwc, hw, W, xs, ys, c);
      }
      o.w[0][0] |= v[0] << (8 * e); o.w[1][0] |= v[1] << (8 * e); o.w[2][0] |= v[2] << (8 * e);
    }
    store_px<4>(o, out, a.dst_hwc, hw, p0, cnt, vec);
  }
}

// ---- hed / hsv ------------------------------------------------------------------------------------------------------------------
namespace {

// numpy's x % 1.0 for a float64: fmod, then + 1.0 where the remainder is negative.  fmod(x, 1.0) IS x - trunc(x): the difference of a
// double and its integer part is representable, so the subtraction is exact (the zero's sign may differ; nothing downstream reads it)
__device__ inline double mod1(double x) {
  const double m = __dsub_rn(x, trunc(x));
  return m < 0.0 ? __dadd_rn(m, 1.0) : m;
}

// HsbColorAugmenter.transform (hsbcoloraugmenter.py:80-125) for one pixel: scikit-image 0.15.0 rgb2hsv, the hue and saturation edits, hsv2rgb
__device__ inline void hsv_pixel(uint32_t& R, uint32_t& G, uint32_t& B, double hshift, double ss) {
  const double k = 1.0 / 255;                        // img_as_float: uint8 * (1 / 255)
  const double r = __dmul_rn((double)R, k), g = __dmul_rn((double)G, k), b = __dmul_rn((double)B, k);
  const double v = fmax(r, fmax(g, b)), mn = fmin(r, fmin(g, b));
  const double delta = __dsub_rn(v, mn);
  double s = 0.0, h = 0.0;
  if (delta != 0.0) {
    s = __ddiv_rn(delta, v);
    double hue = 0.0;                                // red, then green, then blue: the later case overwrites the earlier one on a tie
    if (r == v) hue = __ddiv_rn(__dsub_rn(g, b), delta);
    if (g == v) hue = __dadd_rn(2.0, __ddiv_rn(__dsub_rn(b, r), delta));
    if (b == v) hue = __dadd_rn(4.0, __ddiv_rn(__dsub_rn(r, g), delta));
    h = mod1(__ddiv_rn(hue, 6.0));
  }
  h = mod1(__dadd_rn(h, hshift));
  if (ss < 0.0) s = __dmul_rn(s, __dadd_rn(1.0, ss));
  else if (ss > 0.0) s = __dmul_rn(s, __dadd_rn(1.0, __dmul_rn(__dsub_rn(1.0, s), ss)));
  const double h6 = __dmul_rn(h, 6.0);
  const double hi = floor(h6);
  const double f = __dsub_rn(h6, hi);
  const double p = __dmul_rn(v, __dsub_rn(1.0, s));
  const double q = __dmul_rn(v, __dsub_rn(1.0, __dmul_rn(f, s)));
  const double t = __dmul_rn(v, __dsub_rn(1.0, __dmul_rn(__dsub_rn(1.0, f), s)));
  const int sel = (int)hi % 6;                       // hi is 0 .. 6
  const double x0 = sel == 0 || sel == 5 ? v : sel == 1 ? q : sel == 4 ? t : p;
  const double x1 = sel == 1 || sel == 2 ? v : sel == 0 ? t : sel == 3 ? q : p;
  const double x2 = sel == 3 || sel == 4 ? v : sel == 2 ? t : sel == 5 ? q : p;
  R = (uint32_t)(int)__dmul_rn(x0, 255.0) & 255u;    // (x * 255.0).astype(uint8): truncation
  G = (uint32_t)(int)__dmul_rn(x1, 255.0) & 255u;
  B = (uint32_t)(int)__dmul_rn(x2, 255.0) & 255u;
}

struct HedArgs { float mi[9], m[9], sig[3], bias[3]; };

// HedColorAugmenter.transform (hedcoloraugmenter.py:164-202) on custom_hed_transform.py:22-37 for one pixel, float32
__device__ inline void hed_pixel(uint32_t& R, uint32_t& G, uint32_t& B, const HedArgs& a) {
  const double k = 1.0 / 255;
  float L[3], st[3];
  const uint32_t in[3] = {R, G, B};
#pragma unroll
  for (int c = 0; c < 3; ++c) L[c] = -logf(__fadd_rn((float)__dmul_rn((double)in[c], k), 2.0f));
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    const float d = __fadd_rn(__fadd_rn(__fmul_rn(L[0], a.mi[j]), __fmul_rn(L[1], a.mi[3 + j])), __fmul_rn(L[2], a.mi[6 + j]));
    st[j] = -__fadd_rn(__fmul_rn(d, a.sig[j]), a.bias[j]);
  }
  uint32_t out[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const float l = __fadd_rn(__fadd_rn(__fmul_rn(st[0], a.m[c]), __fmul_rn(st[1], a.m[3 + c])), __fmul_rn(st[2], a.m[6 + c]));
    float x = __fsub_rn(expf(l), 2.0f);
    x = fminf(fmaxf(x, -1.0f), 1.0f);                // rescale_intensity(in_range=(-1, 1)) of a float image: clip, normalise, scale back
    x = __fadd_rn(__fmul_rn(__fdiv_rn(__fadd_rn(x, 1.0f), 2.0f), 2.0f), -1.0f);
    x = fminf(fmaxf(x, 0.0f), 1.0f);
    out[c] = (uint32_t)(int)__fmul_rn(x, 255.0f) & 255u;
  }
  R = out[0]; G = out[1]; B = out[2];
}

}  // namespace

__global__ __launch_bounds__(256) void augv2c_sum_kernel(const sslcr_augv2_colour_desc a) {
  const int n = blockIdx.y;
  if (a.op[n] != SSLCR_AUGV2C_HED) return;           // block-uniform
  const size_t total = (size_t)3 * a.H * a.W;        // the mean is over every byte: layout-blind
  const uint8_t* img = a.img + (size_t)n * total;
  const bool vec = ((uintptr_t)img & 15) == 0;
  const size_t units = (total + 15) / 16;
  unsigned long long sum = 0;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (size_t)gridDim.x * 256) {
    const size_t b0 = u * 16;
    if (vec && b0 + 16 <= total) {
      const uint4 v = *reinterpret_cast<const uint4*>(img + b0);
      const uint32_t w[4] = {v.x, v.y, v.z, v.w};
      uint32_t s = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) s += (w[i] & 0x00ff00ffu) + ((w[i] >> 8) & 0x00ff00ffu);      // two 16-bit lanes, at most 8 * 255 each
      sum += (s & 0xffffu) + (s >> 16);
    } else {
      const size_t b1 = b0 + 16 < total ? b0 + 16 : total;
      for (size_t b = b0; b < b1; ++b) sum += img[b];
    }
  }
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_down(sum, o, 64);
  if ((threadIdx.x & 63) == 0 && sum) atomicAdd(a.bsum + n, sum);
}

__global__ __launch_bounds__(256) void augv2c_apply_kernel(const sslcr_augv2_colour_desc a, const int vec) {
  const int n = blockIdx.y;
  const int op = a.op[n];
  // block-uniform: COPY, any code the entry does not know, and a code whose bit ops_mask lacks (for HED the sum pass did not run and
  // bsum may be NULL) leave the image as it is
  if ((op != SSLCR_AUGV2C_HED && op != SSLCR_AUGV2C_HSV) || !(a.ops_mask & 1u << op)) return;
  const size_t hw = (size_t)a.H * a.W;
  uint8_t* img = a.img + (size_t)n * 3 * hw;
  const double* prm = a.param + (size_t)n * 6;
  const size_t units = (hw + 3) / 4;
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, tstep = (size_t)gridDim.x * 256;
  if (op == SSLCR_AUGV2C_HSV) {
    const double hshift = prm[0], ss = prm[1];
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      Px<4> p;
      load_px<4>(p, img, a.hwc, hw, p0, cnt, vec);
      uint32_t o[3] = {0, 0, 0};
#pragma unroll 2
      for (int e = 0; e < 4; ++e) {                  // a lane past cnt computes on zero bytes; store_px drops it
        uint32_t r = (p.w[0][0] >> (8 * e)) & 255u, g = (p.w[1][0] >> (8 * e)) & 255u, b = (p.w[2][0] >> (8 * e)) & 255u;
        hsv_pixel(r, g, b, hshift, ss);
        o[0] |= r << (8 * e); o[1] |= g << (8 * e); o[2] |= b << (8 * e);
      }
      p.w[0][0] = o[0]; p.w[1][0] = o[1]; p.w[2][0] = o[2];
      store_px<4>(p, img, a.hwc, hw, p0, cnt, vec);
    }
    return;
  }
  // hed: HedColorAugmenter.transform's cutoff (:162-163), np.mean(patch) / 255.0 -- the integer sum is exact in a double
  const double mean = __ddiv_rn(__ddiv_rn((double)a.bsum[n], (double)(3 * hw)), 255.0);
  if (!(a.cutoff_lo <= mean && mean <= a.cutoff_hi)) return;
  HedArgs ha;
#pragma unroll
  for (int i = 0; i < 9; ++i) { ha.mi[i] = a.hed_from_rgb[i]; ha.m[i] = a.rgb_from_hed[i]; }
#pragma unroll
  for (int j = 0; j < 3; ++j) { ha.sig[j] = (float)prm[j]; ha.bias[j] = (float)prm[3 + j]; }
  for (size_t u = t0; u < units; u += tstep) {
    const size_t p0 = u * 4;
    const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
    Px<4> p;
    load_px<4>(p, img, a.hwc, hw, p0, cnt, vec);
    uint32_t o[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      uint32_t r = (p.w[0][0] >> (8 * e)) & 255u, g = (p.w[1][0] >> (8 * e)) & 255u, b = (p.w[2][0] >> (8 * e)) & 255u;
      hed_pixel(r, g, b, ha);
      o[0] |= r << (8 * e); o[1] |= g << (8 * e); o[2] |= b << (8 * e);
    }
    p.w[0][0] = o[0]; p.w[1][0] = o[1]; p.w[2][0] = o[2];
    store_px<4>(p, img, a.hwc, hw, p0, cnt, vec);
  }
}

hipError_t launch_augv2_colour(const sslcr_augv2_colour_desc& a, hipStream_t st) {
  const size_t hw = (size_t)a.H * a.W;
  const int vec = hw % 4 == 0 && ((uintptr_t)a.img & 3) == 0;      // every plane / every 12-byte pixel group of every image on a dword
  hipError_t e;
  if (a.ops_mask & 1u << SSLCR_AUGV2C_HED) {
    if ((e = hipMemsetAsync(a.bsum, 0, (size_t)a.N * sizeof(unsigned long long), st)) != hipSuccess) return e;
    const size_t units = (3 * hw + 15) / 16;
    int bx = (int)((units + 255) / 256);
    if (bx > 16) bx = 16;
    hipLaunchKernelGGL(augv2c_sum_kernel, dim3(bx, a.N), dim3(256), 0, st, a);
  }
  if (a.ops_mask & (1u << SSLCR_AUGV2C_HED | 1u << SSLCR_AUGV2C_HSV)) {
    const size_t units = (hw + 3) / 4;
    int bx = (int)((units + 255) / 256);             // one pass of 4 pixels per thread up to 256 x 256, a grid-stride loop beyond
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(augv2c_apply_kernel, dim3(bx, a.N), dim3(256), 0, st, a, vec);
  }
  return hipGetLastError();
}

hipError_t launch_augv2(const sslcr_augv2_desc& a, hipStream_t st) {
  const size_t hw = (size_t)a.H * a.W;
  const int vec = hw % 16 == 0 && ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)a.dst & 15) == 0;
  const unsigned m = a.ops_mask;
  const unsigned stats_ops = 1u << SSLCR_AUGV2_CONTRAST | 1u << SSLCR_AUGV2_AUTOCONTRAST | 1u << SSLCR_AUGV2_EQUALIZE;
  const size_t units = (hw + 15) / 16;
  int bx = (int)((units + 255) / 256);               // one pass of 16 pixels per thread, at most 16 workgroups per image
  if (bx > 16) bx = 16;
  hipError_t e;
  if (m & stats_ops) {
    if ((e = hipMemsetAsync(a.hist, 0, (size_t)a.N * 768 * sizeof(uint32_t), st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(a.lsum, 0, (size_t)a.N * sizeof(unsigned long long), st)) != hipSuccess) return e;
    hipLaunchKernelGGL(augv2_stats_kernel, dim3(bx, a.N), dim3(256), 0, st, a, vec);
  }
  if (m & (stats_ops | 1u << SSLCR_AUGV2_BRIGHTNESS | 1u << SSLCR_AUGV2_NEAREST_TABLE)) hipLaunchKernelGGL(augv2_lut_kernel, dim3(a.N), dim3(256), 0, st, a);
  hipLaunchKernelGGL(augv2_apply_kernel, dim3(bx, a.N), dim3(256), 0, st, a, vec);
  return hipGetLastError();
}

}  // namespace sslcr
