// Device-side tile mining for RSP pretraining: what Vectorize_WSIs.get_wsi_patches + sorted_sequence do on the host
// (dataset.py:27-70, 386-446 with util.py:18-23; Pretraining_v2/dataset.py:22-60, 219-316 with Pretraining_v2/util.py:9-13), on pyramid
// levels that already sit in HBM as uint8 [H][W][3].  Four entries (include/sslcr.h has the contracts):
//   tissue_bits    the per-pixel foreground predicate of isforeground() -- a* > (1 + mu_percent) mu (v1, CIELAB) or s > mu_percent (v2,
//                  HSV) -- evaluated ONCE per pixel of the level-2 image and kept as one bit per pixel.  The reference converts every
//                  candidate tile on its own, so at stride = tile / 2 every pixel is converted four times.
//   lab_a_sum      mu's numerator, sum of a* over the overview image (dataset.py:400-403), as one double: fixed slices, fixed trees.
//   tile_popcount  np.count_nonzero(window) of every candidate of the grid, from the bit plane: funnel shifts + popcounts.
//   rsp_gather     the three tiles of a triplet AND the ordering sorted_sequence applies, for a batch of sample indices, in one launch:
//                  the six-fold copy of every tile that sorted_sequence builds in host memory never exists.
// Built with -ffp-contract=off: the float64 chains are the reference's operations one rounding each (a contracted multiply-add rounds
// once where NumPy rounds twice), which is what makes the hsv_s plane EQUAL to a NumPy restatement.
// No floating-point atomics, no integer atomics, no byte stores to the bit plane.
#include "kernels.hpp"
#include "map_common.hpp"   // wave_sum
#include "wsi_bytes.hpp"   // wsi_fetch12, wsi_plane: the read side of the tile gathers

namespace sslcr {

// ------------------------------------------------------------------------------------------------ the per-pixel predicates
// skimage 0.15 rgb2lab's a*, D65 / 2 degree observer, from the linearised channels (lin[] = the 256-entry sRGB table the host computes:
// c > 0.04045 ? ((c + 0.055) / 1.055) ** 2.4 : c / 12.92 with c = u8 * (1 / 255)).  The dot product in the order of a row-by-column
// loop; Z is not needed for a*.
__device__ __forceinline__ double lab_f(double t) { return t > 0.008856 ? pow(t, 1.0 / 3.0) : 7.787 * t + 16.0 / 116.0; }
__device__ __forceinline__ double lab_a_star(const double* __restrict__ lin, unsigned r, unsigned g, unsigned b) {
  const double lr = lin[r], lg = lin[g], lb = lin[b];
  const double X = (lr * 0.412453 + lg * 0.357580) + lb * 0.180423;
  const double Y = (lr * 0.212671 + lg * 0.715160) + lb * 0.072169;
  return 500.0 * (lab_f(X / 0.95047) - lab_f(Y / 1.0));
}
// skimage 0.15 rgb2hsv's s on img_as_float(u8): v = max, delta = max - min, s = delta / v, 0 where delta == 0 (black included).
// Multiplication by the rounded reciprocal is monotone, so max / min of the bytes pick the operands NumPy's max / min pick.
__device__ __forceinline__ double hsv_s(unsigned r, unsigned g, unsigned b) {
  const unsigned mx = max(r, max(g, b)), mn = min(r, min(g, b));
  const double k = 1.0 / 255;
  const double v = (double)mx * k, delta = v - (double)mn * k;
  return delta == 0.0 ? 0.0 : delta / v;
}

// ------------------------------------------------------------------------------------------------ 1. bit plane
// The float32 screen of the lab_a predicate.  a* in float32 from the float32 table: the three-term sums of positive products carry
// <= 5 roundings (relative 5 u, u = 2^-24), the division one more, cbrtf <= 2 ulp = 4 u on a value <= 1 whose operand error enters
// divided by three, the linear branch less; the two branches of f meet at t = 0.008856 to 3.3e-7 (an operand the two precisions put on
// different sides).  |f32(f) - f| <= 7 u + 3.3e-7 < 8e-7 per term, so |a32 - a*| <= 500 (2 * 8e-7 + u) < 9e-4.  LAB_SCREEN_BAND =
// 1 / 64 leaves a factor of 17: outside the band around the
// threshold the float32 value decides, inside it the float64 chain does.
constexpr double LAB_SCREEN_BAND = 1.0 / 64;
__device__ __forceinline__ float lab_f32(float t) { return t > 0.008856f ? cbrtf(t) : 7.787f * t + 16.0f / 116.0f; }
__device__ __forceinline__ bool lab_a_above(const double* lin, const float* linf, unsigned r, unsigned g, unsigned b, double thr) {
  const float lr = linf[r], lg = linf[g], lb = linf[b];
  const float X = (lr * 0.412453f + lg * 0.357580f) + lb * 0.180423f;
  const float Y = (lr * 0.212671f + lg * 0.715160f) + lb * 0.072169f;
  const double d = (double)(500.0f * (lab_f32(X / 0.95047f) - lab_f32(Y))) - thr;
  if (fabs(d) > LAB_SCREEN_BAND) return d > 0.0;
  return lab_a_star(lin, r, g, b) > thr;                                   // (a NaN threshold lands here too: false, as in NumPy)
}

// eight bits -> every fourth bit of a dword: bit k to bit 4 k
__device__ __forceinline__ uint32_t spread4(uint32_t x) {
  x = (x | (x << 12)) & 0x000f000fu;
  x = (x | (x << 6)) & 0x03030303u;
  x = (x | (x << 3)) & 0x11111111u;
  return x;
}

// A wave owns 256 consecutive pixels of one row = eight dwords of the plane.  Lane l reads pixels 4 l .. 4 l + 3 as the gathers read
// theirs (wsi_fetch12: the aligned dwords that cover 12 unaligned bytes; per byte, bounds-checked, in the group that holds the row's
// end) and evaluates them; ballot e holds pixel 4 l + e of every lane, so dword d of the eight is byte d of the four ballots with
// their bits interleaved, which lane d builds (spread4) and stores.  Whole dwords, one writer each; lanes past W vote 0, so the pad
// bits are zero, and every dword below `pitch` is written.  lab_a stages the 256-entry table in LDS, as float64 and as float32.
template <int MODE>
__global__ __launch_bounds__(256) void tissue_bits_kernel(const sslcr_tissue_bits_desc a) {
  __shared__ double lin[MODE == SSLCR_TISSUE_LAB_A ? 256 : 1];
  __shared__ float linf[MODE == SSLCR_TISSUE_LAB_A ? 256 : 1];
  if constexpr (MODE == SSLCR_TISSUE_LAB_A) {
    lin[threadIdx.x] = a.lin[threadIdx.x];
    linf[threadIdx.x] = (float)a.lin[threadIdx.x];
    __syncthreads();
  }
  const int lane = threadIdx.x & 63;
  const int cpr = (a.pitch + 7) >> 3;                                      // 256-pixel chunks per row, covering `pitch` dwords
  const size_t waves = (size_t)a.H * cpr;
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(a.img) & 3);
  double thr = a.threshold;
  if (a.thr_sum) thr = a.factor * (*a.thr_sum / a.count);
  for (size_t w = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6); w < waves; w += (size_t)gridDim.x * 4) {
    const int chunk = (int)(w % cpr);
    const size_t y = w / cpr;
    const int64_t x0 = (int64_t)chunk * 256 + 4 * lane;
    const int64_t off = ((int64_t)y * a.W + x0) * 3;
    uint32_t d[3] = {0u, 0u, 0u};                                          // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
    if (x0 + 4 <= a.W) {
      wsi_fetch12(a.img, off, mis, d);
    } else {
#pragma unroll
      for (int k = 0; k < 12; ++k)
        if (x0 + k / 3 < a.W) d[k >> 2] |= (uint32_t)a.img[off + k] << (8 * (k & 3));
    }
    unsigned long long m[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const unsigned r = (d[(3 * e) >> 2] >> (8 * ((3 * e) & 3))) & 0xffu;
      const unsigned g = (d[(3 * e + 1) >> 2] >> (8 * ((3 * e + 1) & 3))) & 0xffu;
      const unsigned b = (d[(3 * e + 2) >> 2] >> (8 * ((3 * e + 2) & 3))) & 0xffu;
      bool p;
      if constexpr (MODE == SSLCR_TISSUE_LAB_A) p = lab_a_above(lin, linf, r, g, b, thr);
      else p = hsv_s(r, g, b) > thr;
      m[e] = __ballot(p && x0 + e < a.W);
    }
    const int dw = 8 * chunk + lane;                                       // lanes 0..7: one dword of the plane each
    if (lane < 8 && dw < a.pitch) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) v |= spread4((uint32_t)(m[e] >> (8 * lane)) & 0xffu) << e;
      a.bits[y * a.pitch + dw] = v;
    }
  }
}

hipError_t launch_tissue_bits(const sslcr_tissue_bits_desc& a, hipStream_t st) {
  const size_t waves = (size_t)a.H * ((a.pitch + 7) >> 3);
  size_t blocks = (waves + 3) / 4;
  if (blocks > 16384) blocks = 16384;
  if (a.mode == SSLCR_TISSUE_LAB_A) hipLaunchKernelGGL(tissue_bits_kernel<SSLCR_TISSUE_LAB_A>, dim3((int)blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(tissue_bits_kernel<SSLCR_TISSUE_HSV_S>, dim3((int)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 2. sum of a*
// the block fold of both stages: a fixed tree over 256 doubles in LDS
__device__ __forceinline__ double block_sum_f64(double v, double* red) {
  red[threadIdx.x] = v;
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
    __syncthreads();
  }
  return red[0];
}
// workgroup b owns the contiguous pixels [b per, (b + 1) per); a thread walks its pixels of the slice at stride 256, in order
__global__ __launch_bounds__(256) void lab_a_partial_kernel(const sslcr_lab_a_sum_desc a) {
  __shared__ double red[256];
  const size_t n = (size_t)a.H * a.W;
  const size_t per = (n + SSLCR_LAB_SUM_PARTIALS - 1) / SSLCR_LAB_SUM_PARTIALS;
  size_t p0 = per * blockIdx.x, p1 = p0 + per;
  if (p0 > n) p0 = n;
  if (p1 > n) p1 = n;
  double acc = 0.0;
  for (size_t p = p0 + threadIdx.x; p < p1; p += 256) {
    const uint8_t* px = a.img + p * 3;
    acc += lab_a_star(a.lin, px[0], px[1], px[2]);
  }
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) a.partials[blockIdx.x] = s;
}
__global__ __launch_bounds__(256) void lab_a_fold_kernel(const double* __restrict__ partials, double* __restrict__ sum) {
  __shared__ double red[256];
  constexpr int PER = SSLCR_LAB_SUM_PARTIALS / 256;
  double acc = 0.0;
#pragma unroll
  for (int j = 0; j < PER; ++j) acc += partials[threadIdx.x * PER + j];
  const double s = block_sum_f64(acc, red);
  if (threadIdx.x == 0) *sum = s;
}

hipError_t launch_lab_a_sum(const sslcr_lab_a_sum_desc& a, hipStream_t st) {
  static_assert(SSLCR_LAB_SUM_PARTIALS % 256 == 0, "the fold gives every thread the same number of partials");
  hipLaunchKernelGGL(lab_a_partial_kernel, dim3(SSLCR_LAB_SUM_PARTIALS), dim3(256), 0, st, a);
  hipLaunchKernelGGL(lab_a_fold_kernel, dim3(1), dim3(256), 0, st, a.partials, a.sum);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 3. candidate counts
// A wave owns one candidate: lane l takes the window rows l, l + 64, ...; a row is ceil(pw / 32) funnel-shifted dwords (the window
// starts at any bit offset), the last one masked to the window's width.  The second dword of a funnel is read only when the shift is
// not zero and it lies inside the row's pitch: no load leaves the plane.  Integer sums: any fold order gives the same count.
__global__ __launch_bounds__(256) void tile_popcount_kernel(const sslcr_tile_popcount_desc a) {
  const int lane = threadIdx.x & 63;
  const int cand = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cand >= a.ny * a.nx) return;                                         // wave-uniform
  const int j = cand / a.nx, i = cand - j * a.nx;
  const int x0 = a.sw * (i + 1), y0 = a.sh * (j + 1);
  const int nd = (a.pw + 31) >> 5;
  int cnt = 0;
  for (int r = lane; r < a.ph; r += 64) {
    const uint32_t* row = a.bits + (size_t)(y0 + r) * a.pitch;
    for (int c = 0; c < nd; ++c) {
      const int bit = x0 + 32 * c;
      const int k = bit >> 5;
      const unsigned sh = (unsigned)bit & 31u;
      const uint32_t lo = row[k];
      const uint32_t hi = (sh && k + 1 < a.pitch) ? row[k + 1] : 0u;
      uint32_t v = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
      const int left = a.pw - 32 * c;
      if (left < 32) v &= (1u << left) - 1u;
      cnt += __popc(v);
    }
  }
  cnt = wave_sum(cnt);
  if (lane == 0) {
    a.count[cand] = cnt;
    a.keep[cand] = (uint8_t)((double)cnt / (double)((int64_t)a.ph * a.pw) >= a.thresh);
  }
}

hipError_t launch_tile_popcount(const sslcr_tile_popcount_desc& a, hipStream_t st) {
  const int cands = a.ny * a.nx;
  if (cands == 0) return hipSuccess;
  hipLaunchKernelGGL(tile_popcount_kernel, dim3((cands + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ 4. triplet gather
// sorted_sequence's orderings over (hr, lr1, lr2) = levels (0, 1, 2): slot s of ordering o shows level (RSP_ORDER[o] >> 2 s) & 3
//   [0,1,2] [0,2,1] [1,2,0] [1,0,2] [2,0,1] [2,1,0]
constexpr uint32_t RSP_ORDER[6] = {0 | 1 << 2 | 2 << 4, 0 | 2 << 2 | 1 << 4, 1 | 2 << 2 | 0 << 4,
                                    1 | 0 << 2 | 2 << 4, 2 | 0 << 2 | 1 << 4, 2 | 1 << 2 | 0 << 4};
// ... the six 6-bit codes in one register: no table in memory
constexpr uint64_t RSP_ORDER_BITS = (uint64_t)RSP_ORDER[0] | (uint64_t)RSP_ORDER[1] << 6 | (uint64_t)RSP_ORDER[2] << 12 |
                                    (uint64_t)RSP_ORDER[3] << 18 | (uint64_t)RSP_ORDER[4] << 24 | (uint64_t)RSP_ORDER[5] << 30;

// wsi_gather_kernel's thread (four consecutive output pixels of one tile row, one dword per colour plane; the per-byte path for tiles
// that leave the level, S % 4 != 0 and unaligned bases) over three outputs at once: output slot s of sample n shows the tile of
// triplet idx[n] / 6 from the level the ordering idx[n] % 6 puts there.  An index outside [0, 6 T) reads nothing: its three tiles
// are `fill` and its label is -1.
__global__ __launch_bounds__(256) void rsp_gather_kernel(const sslcr_rsp_gather_desc a, const int dword_out) {
  const int S = a.S;
  const int qw = (S + 3) / 4;
  const size_t per_slot = (size_t)a.N * S * qw;
  const size_t total = 3 * per_slot;
  const size_t plane = (size_t)S * S;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int slot = (int)(t / per_slot);
    const size_t u = t - slot * per_slot;
    const int q = (int)(u % qw);
    const size_t r = u / qw;
    const int i = (int)(r % S);
    const size_t n = r / S;
    const int64_t k = a.idx[n];
    const bool valid = k >= 0 && k < 6 * (int64_t)a.T;
    const int64_t trip = valid ? k / 6 : 0;
    const int ord = valid ? (int)(k - 6 * trip) : 0;
    if (slot == 0 && i == 0 && q == 0) a.label[n] = valid ? ord : -1;
    const int lvl = (int)(RSP_ORDER_BITS >> (6 * ord + 2 * slot)) & 3;
    const uint8_t* src = lvl == 0 ? a.src[0] : lvl == 1 ? a.src[1] : a.src[2];
    const int32_t* xy = lvl == 0 ? a.xy[0] : lvl == 1 ? a.xy[1] : a.xy[2];
    const int RH = lvl == 0 ? a.RH[0] : lvl == 1 ? a.RH[1] : a.RH[2];
    const int RW = lvl == 0 ? a.RW[0] : lvl == 1 ? a.RW[1] : a.RW[2];
    uint8_t* out = slot == 0 ? a.dst[0] : slot == 1 ? a.dst[1] : a.dst[2];
    const int64_t x0 = (int64_t)xy[2 * trip] + 4 * q;                      // level-pixel column of the thread's first pixel
    const int64_t y = (int64_t)xy[2 * trip + 1] + i;
    uint8_t* dst = out + (n * 3 * S + i) * (size_t)S + 4 * q;
    const bool row_in = valid && y >= 0 && y < RH;
    if (dword_out && row_in && x0 >= 0 && x0 + 4 <= RW) {                  // (dword_out implies 4 q + 4 <= S)
      uint32_t d[3];
      wsi_fetch12(src, (y * RW + x0) * 3, (int64_t)(reinterpret_cast<uintptr_t>(src) & 3), d);
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(dst + c * plane) = wsi_plane(d, c);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (4 * q + e >= S) break;
        const int64_t x = x0 + e;
        const bool in = row_in && x >= 0 && x < RW;
        const int64_t b = in ? (y * RW + x) * 3 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint8_t v = (uint8_t)a.fill;
          if (in) v = src[b + c];
          dst[c * plane + e] = v;
        }
      }
    }
  }
}

hipError_t launch_rsp_gather(const sslcr_rsp_gather_desc& a, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const size_t total = 3 * (size_t)a.N * a.S * ((a.S + 3) / 4);
  size_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const uintptr_t bases = reinterpret_cast<uintptr_t>(a.dst[0]) | reinterpret_cast<uintptr_t>(a.dst[1]) | reinterpret_cast<uintptr_t>(a.dst[2]);
  const int dword_out = (a.S & 3) == 0 && (bases & 3) == 0;
  hipLaunchKernelGGL(rsp_gather_kernel, dim3((int)blocks), dim3(256), 0, st, a, dword_out);
  return hipGetLastError();
}

}  // namespace sslcr
