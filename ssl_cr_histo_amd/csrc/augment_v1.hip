// Device-side RandAugment of the consistency-training pipeline (models/randaugment.py:51-110): the six OpenCV-style ops of its pool
// -- HSV, Noise, Scale_Resize_Crop, Shift_Scale_Rotate, Blur_img, Rotate_Crop -- on a uint8 batch in HBM, one op SLOT of a whole
// batch per call: every image carries its own op code, parameters and apply flag; COPY passes through.  The host makes every random
// draw (ssl_cr_histo_amd/augment.py); the kernels are the deterministic arithmetic include/sslcr.h DEFINES, integer or float32 with
// + - x in a fixed order (this file is built with -ffp-contract=off), so that the NumPy restatement (tests/_cv_ref.py) has their
// bits.  PARITY UNPINNED against OpenCV / albumentations / imgaug.
//
//   augv1_resize1_kernel  the first resize of Scale_Resize_Crop, S -> S', into the planar uint8 workspace (RESIZE images only)
//   augv1_slot_kernel<OP> reads src once per tap and writes dst once, either layout on either side.  The op is block-uniform
//                         (blockIdx.y is the image); one instance per op code, launched when the slot's mask names the code, the
//                         workgroups of other images leaving at once.  A thread owns 4 consecutive output pixels: whole-dword stores per plane or one
//                         12-byte group, a scalar tail when H*W % 4 != 0 (COPY moves 16 pixels per thread).  BLUR shares its column
//                         sums among the 4 windows; HSV keeps the two division tables in LDS; WARP stages the 32 KiB weight table
//                         into LDS once per workgroup and gathers its 16 taps per channel through the L1; RESIZE computes only the
//                         cropped window of the second resize from the workspace; NOISE draws one Philox block per thread.
//   augv1_philox_kernel   the integer stream of NOISE alone, for the tests
#include <limits.h>

#include "kernels.hpp"
#include "px_bytes.hpp"    // Px, load_px, store_px, byte_of

namespace sslcr {

namespace {

constexpr int OP_BLACK = -1;
constexpr int WTAB_BYTES = 1024 * 16 * 2;

// the A = -0.75 cubic of include/sslcr.h, float32, one rounding per operation (no contraction in this file)
__host__ __device__ inline void cubic4(float x, float c[4]) {
  const float A = -0.75f;
  const float x1 = x + 1.f;
  c[0] = ((A * x1 - 5.f * A) * x1 + 8.f * A) * x1 - 4.f * A;
  c[1] = ((A + 2.f) * x - (A + 3.f)) * x * x + 1.f;
  const float y = 1.f - x;
  c[2] = ((A + 2.f) * y - (A + 3.f)) * y * y + 1.f;
  c[3] = 1.f - c[0] - c[1] - c[2];
}

__host__ __device__ inline int sat_short(float v) { return v <= -32768.f ? -32768 : v >= 32767.f ? 32767 : (int)v; }

__device__ inline int reflect101(int p, int n) {
  if ((unsigned)p < (unsigned)n) return p;
  if (n == 1) return 0;
  const int period = 2 * n - 2;
  int m = p % period;
  if (m < 0) m += period;
  return m >= n ? period - m : m;
}

__device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : v > hi ? hi : v; }

__device__ inline int at(const uint8_t* img, int hwc, size_t hw, int W, int x, int y, int c) {
  const size_t p = (size_t)y * W + x;
  return img[hwc ? p * 3 + c : c * hw + p];
}

// The gathers address a channel as base[off * step] with off = y W + x: H, W <= 16384 keeps 3 off inside 32 bits, so a tap costs one
// 32-bit multiply-add and one pointer add
struct Chan { const uint8_t* base; uint32_t step; };
__device__ inline Chan chan(const uint8_t* img, int hwc, size_t hw, int c) { return hwc ? Chan{img + c, 3u} : Chan{img + c * hw, 1u}; }
__device__ inline int at(const Chan& ch, uint32_t off) { return ch.base[off * ch.step]; }

// Four horizontally consecutive taps at pixel offset off, all channels: byte k of q[c] = channel c of pixel off + k.  One unaligned
// dword per plane, or the 12 interleaved bytes at once: a byte gather costs the texture path as much as a dword.  The caller has
// checked that the four pixels lie in one row of the image, so the bytes read are the image's
__device__ inline void taps4(const uint8_t* img, int hwc, size_t hw, uint32_t off, uint32_t q[3]) {
  if (hwc) {
    uint32_t r[3];
    __builtin_memcpy(r, img + (size_t)off * 3, 12);
#pragma unroll
    for (int c = 0; c < 3; ++c) q[c] = wsi_plane(r, c);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) __builtin_memcpy(&q[c], img + c * hw + off, 4);
  }
}

// ---- 1. box blur: 4 consecutive pixels.  In one row the K + cnt - 1 column sums serve all windows
template <int K>
__device__ inline void blur_unit(const uint8_t* img, int hwc, size_t hw, int H, int W, size_t p0, int cnt, Px<4>& o) {
  constexpr int R = K / 2, KK = K * K;
  const int y0 = (int)(p0 / W), x0 = (int)(p0 - (size_t)y0 * W);
  if (x0 + cnt <= W) {
    int xs[K + 3], col[3][K + 3];
#pragma unroll
    for (int j = 0; j < K + 3; ++j) {                // a column past the last window is reflected too: in range, and read
      xs[j] = reflect101(x0 - R + j, W);
      col[0][j] = col[1][j] = col[2][j] = 0;
    }
#pragma unroll 1
    for (int i = 0; i < K; ++i) {                    // row after row: 3 (K + 3) byte loads in flight, not 3 K (K + 3)
      const int yy = reflect101(y0 - R + i, H);
      const uint32_t row = (uint32_t)yy * (uint32_t)W;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const Chan ch = chan(img, hwc, hw, c);
#pragma unroll
        for (int j = 0; j < K + 3; ++j) col[c][j] += at(ch, row + (uint32_t)xs[j]);
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        int s = 0;
#pragma unroll
        for (int j = 0; j < K; ++j) s += col[c][e + j];
        v |= (uint32_t)((2 * s + KK) / (2 * KK)) << (8 * e);
      }
      o.w[c][0] = v;
    }
    return;
  }
  for (int e = 0; e < cnt; ++e) {                    // the unit crosses a row end (W % 4 != 0)
    const size_t p = p0 + e;
    const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
    for (int c = 0; c < 3; ++c) {
      int s = 0;
      for (int i = 0; i < K; ++i) {
        const int yy = reflect101(y - R + i, H);
        for (int j = 0; j < K; ++j) s += at(img, hwc, hw, W, reflect101(x - R + j, W), yy, c);
      }
      o.w[c][0] |= (uint32_t)((2 * s + KK) / (2 * KK)) << (8 * e);
    }
  }
}

// ---- 2. the 8-bit HSV shift for one pixel
__device__ inline uint32_t sat_u8f(float x) {
  const float r = rintf(x);
  return r <= 0.f ? 0u : r >= 255.f ? 255u : (uint32_t)(int)r;
}

__device__ inline void hsv_shift_px(uint32_t& R, uint32_t& G, uint32_t& B, const int* sdiv, const int* hdiv, int dh, int ds, int dv) {
  const int r = (int)R, g = (int)G, b = (int)B;
  int v = max(r, max(g, b));
  const int diff = v - min(r, min(g, b));
  int s = (diff * sdiv[v] + 2048) >> 12;
  int h = v == r ? g - b : v == g ? b - r + 2 * diff : r - g + 4 * diff;
  h = (h * hdiv[diff] + 2048) >> 12;
  if (h < 0) h += 180;
  h += dh;
  if (h < 0) h = 255 - h;
  if (h > 255) h -= 255;
  s = clampi(s + ds, 0, 255);
  v = clampi(v + dv, 0, 255);
  float hf = (float)h * (6.f / 180.f);
  while (hf >= 6.f) hf = hf - 6.f;
  const float sec = floorf(hf);
  float f = hf - sec;
  int sector = (int)sec;
  if ((unsigned)sector >= 6u) { sector = 0; f = 0.f; }
  const float k = 1.f / 255.f;
  const float sf = (float)s * k, vf = (float)v * k;
  const float t1 = vf * (1.f - sf), t2 = vf * (1.f - sf * f), t3 = vf * (1.f - sf * (1.f - f));
  // {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}} -> (b, g, r)
  const float fb = sector == 0 || sector == 1 ? t1 : sector == 2 ? t3 : sector == 5 ? t2 : vf;
  const float fg = sector == 0 ? t3 : sector == 1 || sector == 2 ? vf : sector == 3 ? t2 : t1;
  const float fr = sector == 0 || sector == 5 ? vf : sector == 1 ? t2 : sector == 4 ? t3 : t1;
  R = sat_u8f(fr * 255.f); G = sat_u8f(fg * 255.f); B = sat_u8f(fb * 255.f);
}

// ---- 3. the fixed-point bicubic warp for one pixel
__device__ inline int sat32(double v) {
  const double r = rint(v);
  return r <= -2147483648.0 ? INT_MIN : r >= 2147483647.0 ? INT_MAX : (int)r;
}

__device__ inline void warp_px(const uint8_t* img, int hwc, size_t hw, int H, int W, const double* M, int fx, int fy, const uint32_t* wl,
                               int x, int y, uint32_t v[3]) {
  const long long X0 = (long long)sat32(__dmul_rn(__dadd_rn(__dmul_rn(M[1], (double)y), M[2]), 1024.0)) + 16;
  const long long Y0 = (long long)sat32(__dmul_rn(__dadd_rn(__dmul_rn(M[4], (double)y), M[5]), 1024.0)) + 16;
  const int X = (int)((X0 + sat32(__dmul_rn(__dmul_rn(M[0], (double)x), 1024.0))) >> 5);
  const int Y = (int)((Y0 + sat32(__dmul_rn(__dmul_rn(M[3], (double)x), 1024.0))) >> 5);
  const int sx = X >> 5, sy = Y >> 5;
  const int phase = (Y & 31) * 32 + (X & 31);
  int xs[4], ys[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int xx = reflect101(sx - 1 + k, W), yy = reflect101(sy - 1 + k, H);
    xs[k] = fx ? W - 1 - xx : xx;
    ys[k] = (fy ? H - 1 - yy : yy) * W;                // the row's offset
  }
  const uint4 q0 = *reinterpret_cast<const uint4*>(wl + phase * 8), q1 = *reinterpret_cast<const uint4*>(wl + phase * 8 + 4);
  const uint32_t wd[8] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w};
  int wt[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const uint32_t half = (wd[k >> 1] >> (16 * (k & 1))) & 0xffffu;
    wt[k] = k == 5 ? (int)half : (int)(int16_t)half;           // entry 5 is read unsigned (include/sslcr.h)
  }
  const int run = xs[3] - xs[0];                     // 3: no reflected tap; -3: the same under the horizontal flip
  if (run == 3 || run == -3) {
    int acc[3] = {16384, 16384, 16384};
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      uint32_t q[3];
      taps4(img, hwc, hw, (uint32_t)(ys[ky] + (run > 0 ? xs[0] : xs[3])), q);
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int kx = 0; kx < 4; ++kx) acc[c] += (int)byte_of(q[c], run > 0 ? kx : 3 - kx) * wt[ky * 4 + kx];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (uint32_t)clampi(acc[c] >> 15, 0, 255);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const Chan ch = chan(img, hwc, hw, c);
    int acc = 16384;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky)
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) acc += at(ch, (uint32_t)(ys[ky] + xs[kx])) * wt[ky * 4 + kx];
    v[c] = (uint32_t)clampi(acc >> 15, 0, 255);
  }
}

// ---- 4. the fixed-point bicubic resize: one axis of one output index
struct Axis { int idx[4], co[4]; };

// scale = double(src) / double(dst), the same for every pixel of the image: the caller divides once
__device__ inline void resize_axis(int d, int src, double scale, Axis& a) {
  const float f = (float)__dadd_rn(__dmul_rn(__dadd_rn((double)d, 0.5), scale), -0.5);
  const float s = floorf(f);
  float c[4];
  cubic4(f - s, c);
  const int si = (int)s;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a.idx[j] = clampi(si - 1 + j, 0, src - 1);
    a.co[j] = sat_short(rintf(c[j] * 2048.f));
  }
}

__device__ inline void resize_px(const uint8_t* img, int hwc, size_t hw, int W, const Axis& ax, const Axis& ay, uint32_t v[3]) {
  if (ax.idx[3] - ax.idx[0] == 3) {                  // no clamped tap: four consecutive pixels of a row
    int acc[3] = {1 << 21, 1 << 21, 1 << 21};
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      uint32_t q[3];
      taps4(img, hwc, hw, (uint32_t)ay.idx[ky] * (uint32_t)W + (uint32_t)ax.idx[0], q);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        acc[c] += ((int)byte_of(q[c], 0) * ax.co[0] + (int)byte_of(q[c], 1) * ax.co[1] + (int)byte_of(q[c], 2) * ax.co[2] +
                   (int)byte_of(q[c], 3) * ax.co[3]) * ay.co[ky];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (uint32_t)clampi(acc[c] >> 22, 0, 255);
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    const Chan ch = chan(img, hwc, hw, c);
    int acc = 1 << 21;
#pragma unroll
    for (int ky = 0; ky < 4; ++ky) {
      const uint32_t ro = (uint32_t)ay.idx[ky] * (uint32_t)W;
      int row = 0;
#pragma unroll
      for (int kx = 0; kx < 4; ++kx) row += at(ch, ro + (uint32_t)ax.idx[kx]) * ax.co[kx];
      acc += row * ay.co[ky];
    }
    v[c] = (uint32_t)clampi(acc >> 22, 0, 255);
  }
}

// ---- 5. Philox4x32-10, counter (c0, 0, 0, 0)
__device__ inline void philox4x32_10(uint32_t c0, uint32_t k0, uint32_t k1, uint32_t w[4]) {
  uint32_t c[4] = {c0, 0u, 0u, 0u};
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0; c[1] = lo1; c[2] = n2; c[3] = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  w[0] = c[0]; w[1] = c[1]; w[2] = c[2]; w[3] = c[3];
}

__device__ inline void box_muller(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f, u2 = (float)(b >> 8) * 0x1p-24f;
  const float r = sqrtf(-2.f * logf(u1));
  const float th = 6.2831853071795864769f * u2;
  z0 = r * cosf(th);
  z1 = r * sinf(th);
}

}  // namespace

__global__ __launch_bounds__(256) void augv1_resize1_kernel(const sslcr_augv1_desc a) {
  const int n = blockIdx.y;
  if (a.op[n] != SSLCR_AUGV1_RESIZE || (a.apply && !a.apply[n]) || !a.iparam || !a.work || a.H != a.W) return;      // block-uniform
  const int s1 = a.iparam[n * 4];
  if (s1 < 1 || s1 > a.work_smax) return;            // the slot kernel writes this image black
  const int S = a.H;
  const size_t hw = (size_t)S * S, hw1 = (size_t)s1 * s1;
  const uint8_t* img = a.src + (size_t)n * 3 * hw;
  uint8_t* wimg = a.work + (size_t)n * augv1_work_stride(a.work_smax);
  const bool vec = (hw1 & 3) == 0 && ((uintptr_t)wimg & 3) == 0;
  const double scale = __ddiv_rn((double)S, (double)s1);
  const size_t units = (hw1 + 3) / 4;
  for (size_t u = (size_t)blockIdx.x * 256 + threadIdx.x; u < units; u += (size_t)gridDim.x * 256) {
    const size_t p0 = u * 4;
    const int cnt = hw1 - p0 < 4 ? (int)(hw1 - p0) : 4;
    Px<4> o;
    o.w[0][0] = o.w[1][0] = o.w[2][0] = 0;
    Axis ax, ay;
    int ylast = -1;
    for (int e = 0; e < cnt; ++e) {
      const size_t p = p0 + e;
      const int y = (int)(p / s1), x = (int)(p - (size_t)y * s1);
      resize_axis(x, S, scale, ax);
      if (y != ylast) { resize_axis(y, S, scale, ay); ylast = y; }
      uint32_t v[3];
      resize_px(img, a.src_hwc, hw, S, ax, ay, v);
      o.w[0][0] |= v[0] << (8 * e); o.w[1][0] |= v[1] << (8 * e); o.w[2][0] |= v[2] << (8 * e);
    }
    store_px<4>(o, wimg, 0, hw1, p0, cnt, vec);
  }
}

namespace {

// The op image n takes in this slot, block-uniform, with its three integers.  A code the entry does not know, a code whose bit ops_mask
// lacks (the launches of this slot were chosen by the mask), a NULL table or a parameter out of its range is OP_BLACK: the image is
// written black instead of reading through a bad pointer.
__device__ inline int effective_op(const sslcr_augv1_desc& a, int n, int& i0, int& i1, int& i2) {
  int op = a.op[n];
  i0 = i1 = i2 = 0;
  if (op == SSLCR_AUGV1_COPY || (a.apply && !a.apply[n])) return SSLCR_AUGV1_COPY;
  if (op < 0 || op > SSLCR_AUGV1_NOISE || !(a.ops_mask & 1u << op) || !a.iparam) return OP_BLACK;
  i0 = a.iparam[n * 4]; i1 = a.iparam[n * 4 + 1]; i2 = a.iparam[n * 4 + 2];
  if ((op == SSLCR_AUGV1_BLUR && i0 != 3 && i0 != 5 && i0 != 7) || (op == SSLCR_AUGV1_WARP && !(a.dparam && a.wtab)) ||
      (op == SSLCR_AUGV1_NOISE && !a.dparam) ||
      (op == SSLCR_AUGV1_RESIZE && (!a.work || a.H != a.W || i0 < 1 || i0 > a.work_smax || i1 < 0 || i1 > 20 || i2 < 0 || i2 > 20)))
    return OP_BLACK;
  return op;
}

}  // namespace

// One instance per op code, so that each gets the registers ITS arithmetic needs (the 7 x 7 blur's column sums would otherwise set
// the occupancy of the point ops); a slot launches the instances its ops_mask names, and every workgroup whose image takes another
// op leaves at once.  The COPY instance, always launched, also serves the black images.
// vec: bit 0 = the batch is 4-byte tileable (H*W % 4 == 0, dword-aligned bases), bit 1 = 16-byte tileable
template <int OP>
__global__ __launch_bounds__(256) void augv1_slot_kernel(const sslcr_augv1_desc a, const int vec) {
  extern __shared__ __align__(16) unsigned char smem[];
  const int n = blockIdx.y;
  int i0, i1, i2;
  const int op = effective_op(a, n, i0, i1, i2);
  if (OP == SSLCR_AUGV1_COPY ? (op != SSLCR_AUGV1_COPY && op != OP_BLACK) : op != OP) return;      // block-uniform
  const int H = a.H, W = a.W;
  const size_t hw = (size_t)H * W;
  const uint8_t* img = a.src + (size_t)n * 3 * hw;
  uint8_t* out = a.dst + (size_t)n * 3 * hw;
  const size_t t0 = (size_t)blockIdx.x * 256 + threadIdx.x, tstep = (size_t)gridDim.x * 256;

  if constexpr (OP == SSLCR_AUGV1_COPY) {            // ---- 16 pixels per thread
    const size_t units = (hw + 15) / 16;
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 16;
      const int cnt = hw - p0 < 16 ? (int)(hw - p0) : 16;
      Px<16> p;
      if (op == OP_BLACK) {
#pragma unroll
        for (int c = 0; c < 3; ++c)
#pragma unroll
          for (int q = 0; q < 4; ++q) p.w[c][q] = 0;
      } else {
        load_px<16>(p, img, a.src_hwc, hw, p0, cnt, vec & 2);
      }
      store_px<16>(p, out, a.dst_hwc, hw, p0, cnt, vec & 2);
    }
    return;
  }

  const bool v4 = vec & 1;
  const size_t units = (hw + 3) / 4;
  if constexpr (OP == SSLCR_AUGV1_HSV) {
    int* sdiv = reinterpret_cast<int*>(smem);
    int* hdiv = sdiv + 256;
    {
      const int i = threadIdx.x;
      sdiv[i] = i ? (int)rint(__ddiv_rn((double)(255 << 12), (double)i)) : 0;
      hdiv[i] = i ? (int)rint(__ddiv_rn((double)(180 << 12), __dmul_rn(6.0, (double)i))) : 0;
    }
    __syncthreads();
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      Px<4> p;
      load_px<4>(p, img, a.src_hwc, hw, p0, cnt, v4);
      uint32_t o[3] = {0, 0, 0};
#pragma unroll
      for (int e = 0; e < 4; ++e) {                  // a lane past cnt computes on zero bytes; store_px drops it
        uint32_t r = byte_of(p.w[0][0], e), g = byte_of(p.w[1][0], e), b = byte_of(p.w[2][0], e);
        hsv_shift_px(r, g, b, sdiv, hdiv, i0, i1, i2);
        o[0] |= r << (8 * e); o[1] |= g << (8 * e); o[2] |= b << (8 * e);
      }
      p.w[0][0] = o[0]; p.w[1][0] = o[1]; p.w[2][0] = o[2];
      store_px<4>(p, out, a.dst_hwc, hw, p0, cnt, v4);
    }
  } else if constexpr (OP == SSLCR_AUGV1_NOISE) {
    const double sigma = a.dparam[n * 6];
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      Px<4> p;
      load_px<4>(p, img, a.src_hwc, hw, p0, cnt, v4);
      uint32_t w[4];
      philox4x32_10((uint32_t)u, (uint32_t)i0, (uint32_t)i1, w);
      float z[4];
      box_muller(w[0], w[1], z[0], z[1]);
      box_muller(w[2], w[3], z[2], z[3]);
      uint32_t o[3] = {0, 0, 0};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double t = rint(__dmul_rn(sigma, (double)z[e]));
        const int d = !(t > -256.0) ? -256 : t >= 256.0 ? 256 : (int)t;    // a NaN (the host refuses a non-finite sigma) takes the first branch
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] |= (uint32_t)clampi((int)byte_of(p.w[c][0], e) + d, 0, 255) << (8 * e);
      }
      p.w[0][0] = o[0]; p.w[1][0] = o[1]; p.w[2][0] = o[2];
      store_px<4>(p, out, a.dst_hwc, hw, p0, cnt, v4);
    }
  } else if constexpr (OP == SSLCR_AUGV1_BLUR) {     // ---- the neighbourhood ops: taps gathered through the L1
    for (size_t u = t0; u < units; u += tstep) {
      const size_t p0 = u * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      Px<4> o;
      o.w[0][0] = o.w[1][0] = o.w[2][0] = 0;
      if (i0 == 3) blur_unit<3>(img, a.src_hwc, hw, H, W, p0, cnt, o);
      else if (i0 == 5) blur_unit<5>(img, a.src_hwc, hw, H, W, p0, cnt, o);
      else blur_unit<7>(img, a.src_hwc, hw, H, W, p0, cnt, o);
      store_px<4>(o, out, a.dst_hwc, hw, p0, cnt, v4);
    }
  } else {                                           // WARP, RESIZE
    const uint32_t* wl = reinterpret_cast<const uint32_t*>(smem);
    double M[6] = {0, 0, 0, 0, 0, 0};
    const uint8_t* wimg = nullptr;
    size_t hw1 = 0;
    double scale = 0.0;
    if constexpr (OP == SSLCR_AUGV1_WARP) {
      const uint4* g = reinterpret_cast<const uint4*>(a.wtab);
      uint4* l = reinterpret_cast<uint4*>(smem);
      for (int i = threadIdx.x; i < WTAB_BYTES / 16; i += 256) l[i] = g[i];
      __syncthreads();
      for (int i = 0; i < 6; ++i) M[i] = a.dparam[n * 6 + i];
    } else {
      wimg = a.work + (size_t)n * augv1_work_stride(a.work_smax);
      hw1 = (size_t)i0 * i0;
      scale = __ddiv_rn((double)i0, (double)(W + 20));      // H == W
    }
    // Which 4-pixel unit a thread takes.  W % 4 == 0: a wave covers a 16 x 16 pixel tile (4 units by 16 rows), the workgroup four
    // tiles side by side, so that the taps of one gather instruction fall into a compact patch of the source however the map turns
    // it -- a 256 x 1 strip under a rotation touches a cache line per lane.  Otherwise the units run flat over the image.
    const bool tiled = (W & 3) == 0;
    const int uw = W >> 2, tiles_x = (uw + 15) >> 4, tiles_y = (H + 15) >> 4;
    const size_t trips = tiled ? (size_t)tiles_x * tiles_y : (units + 255) / 256;
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
      size_t u;
      if (tiled) {
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const int ux = (int)(trip % tiles_x) * 16 + wv * 4 + (lane & 3), uy = (int)(trip / tiles_x) * 16 + (lane >> 2);
        if (ux >= uw || uy >= H) continue;
        u = (size_t)uy * uw + ux;
      } else {
        u = trip * 256 + threadIdx.x;
        if (u >= units) continue;
      }
      const size_t p0 = u * 4;
      const int cnt = hw - p0 < 4 ? (int)(hw - p0) : 4;
      Px<4> o;
      o.w[0][0] = o.w[1][0] = o.w[2][0] = 0;
      Axis ax, ay;
      int ylast = -1;
      for (int e = 0; e < cnt; ++e) {
        const size_t p = p0 + e;
        const int y = (int)(p / W), x = (int)(p - (size_t)y * W);
        uint32_t v[3];
        if constexpr (OP == SSLCR_AUGV1_WARP) {
          warp_px(img, a.src_hwc, hw, H, W, M, i0 != 0, i1 != 0, wl, x, y, v);
        } else {                                     // the second resize, S' -> S + 20, at the window's pixel
          resize_axis(x + i2, i0, scale, ax);
          if (y != ylast) { resize_axis(y + i1, i0, scale, ay); ylast = y; }
          resize_px(wimg, 0, hw1, i0, ax, ay, v);
        }
        o.w[0][0] |= v[0] << (8 * e); o.w[1][0] |= v[1] << (8 * e); o.w[2][0] |= v[2] << (8 * e);
      }
      store_px<4>(o, out, a.dst_hwc, hw, p0, cnt, v4);
    }
  }
}

__global__ __launch_bounds__(256) void augv1_philox_kernel(uint32_t k0, uint32_t k1, uint32_t first, int count, uint32_t* words) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  uint32_t w[4];
  philox4x32_10(first + (uint32_t)i, k0, k1, w);
  *reinterpret_cast<uint4*>(words + (size_t)4 * i) = make_uint4(w[0], w[1], w[2], w[3]);
}

hipError_t launch_augv1_philox(unsigned long long seed, uint32_t first, int count, uint32_t* words, hipStream_t st) {
  hipLaunchKernelGGL(augv1_philox_kernel, dim3((count + 255) / 256), dim3(256), 0, st, (uint32_t)seed, (uint32_t)(seed >> 32), first, count, words);
  return hipGetLastError();
}

hipError_t launch_augv1(const sslcr_augv1_desc& a, hipStream_t st) {
  const size_t hw = (size_t)a.H * a.W;
  const bool al4 = ((uintptr_t)a.src & 3) == 0 && ((uintptr_t)a.dst & 3) == 0, al16 = ((uintptr_t)a.src & 15) == 0 && ((uintptr_t)a.dst & 15) == 0;
  const int vec = (hw % 4 == 0 && al4 ? 1 : 0) | (hw % 16 == 0 && al16 ? 2 : 0);
  const unsigned m = a.ops_mask;
  const dim3 block(256);
  hipError_t e;
  if (m & 1u << SSLCR_AUGV1_RESIZE) {
    const size_t units = ((size_t)a.work_smax * a.work_smax + 3) / 4;
    int bx = (int)((units + 255) / 256);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(augv1_resize1_kernel, dim3(bx, a.N), block, 0, st, a);
  }
  const size_t units = (hw + 3) / 4;
  int bx = (int)((units + 255) / 256);               // one pass of 4 pixels per thread up to 256 x 256, a grid-stride loop beyond
  if (bx > 64) bx = 64;
  const dim3 grid(bx, a.N), grid16((bx + 3) / 4, a.N);
  // every image is written by exactly one instance: the COPY instance takes the passed-through and the black ones
  hipLaunchKernelGGL(augv1_slot_kernel<SSLCR_AUGV1_COPY>, grid16, block, 0, st, a, vec);
  if (m & 1u << SSLCR_AUGV1_BLUR) hipLaunchKernelGGL(augv1_slot_kernel<SSLCR_AUGV1_BLUR>, grid, block, 0, st, a, vec);
  if (m & 1u << SSLCR_AUGV1_RESIZE) hipLaunchKernelGGL(augv1_slot_kernel<SSLCR_AUGV1_RESIZE>, grid, block, 0, st, a, vec);
  if (m & 1u << SSLCR_AUGV1_NOISE) hipLaunchKernelGGL(augv1_slot_kernel<SSLCR_AUGV1_NOISE>, grid, block, 0, st, a, vec);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  if (m & 1u << SSLCR_AUGV1_HSV)
    if ((e = launch_lds<augv1_slot_kernel<SSLCR_AUGV1_HSV>>(grid, block, 2048, 2048, st, a, vec)) != hipSuccess) return e;
  if (m & 1u << SSLCR_AUGV1_WARP)
    if ((e = launch_lds<augv1_slot_kernel<SSLCR_AUGV1_WARP>>(grid, block, WTAB_BYTES, WTAB_BYTES, st, a, vec)) != hipSuccess) return e;
  return hipSuccess;
}

void cv_warp_table(int16_t* table) {
  float c[32][4];
  for (int i = 0; i < 32; ++i) cubic4((float)i * (1.f / 32.f), c[i]);
  for (int fy = 0; fy < 32; ++fy)
    for (int fx = 0; fx < 32; ++fx) {
      int it[4][4], sum = 0;
      for (int k1 = 0; k1 < 4; ++k1)
        for (int k2 = 0; k2 < 4; ++k2) {
          const float v = c[fy][k1] * c[fx][k2];
          it[k1][k2] = sat_short(rintf(v * 32768.f));
          sum += it[k1][k2];
        }
      const int diff = sum - 32768;
      if (diff) {
        int mk1 = 1, mk2 = 1, Mk1 = 1, Mk2 = 1;
        for (int k1 = 1; k1 <= 2; ++k1)
          for (int k2 = 1; k2 <= 2; ++k2) {
            if (it[k1][k2] < it[mk1][mk2]) { mk1 = k1; mk2 = k2; }
            else if (it[k1][k2] > it[Mk1][Mk2]) { Mk1 = k1; Mk2 = k2; }
          }
        if (diff < 0) it[Mk1][Mk2] -= diff;
        else it[mk1][mk2] -= diff;
      }
      for (int k = 0; k < 16; ++k) table[(fy * 32 + fx) * 16 + k] = (int16_t)(uint16_t)(it[k >> 2][k & 3] & 0xffff);
    }
}

}  // namespace sslcr
