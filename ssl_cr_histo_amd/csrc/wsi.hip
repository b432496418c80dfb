// Device-side WSI tiling (row f3): DatasetCamelyon16_test.__getitem__ (dataset.py:983-996) -- slide.read_region((x, y), 0, (S, S)),
// .convert('RGB'), np.array(...).transpose((2, 0, 1)) -- for a whole batch of tiles at once, from one slide region that already sits in
// HBM as uint8 [RH][RW][3]:
//     dst[n][c][i][j] = src[top - origin_y + i][left - origin_x + j][c]      inside the region, `fill` elsewhere.
// The reference reads every tile from the file and hands over 786 KB of float32 per 256x256 tile; neighbouring tiles overlap by
// (1 - resolution / S) of their area, so here the slide's bytes cross the host link once and a tile costs 3 S^2 bytes read + 3 S^2 written.
//
// A byte gather, HBM-bound; weak_augment_kernel (augment.hip) is the model for the store side: a thread owns four consecutive output
// pixels of one tile row and writes one dword per colour plane, consecutive lanes consecutive dwords.  The new part is the read: the four
// pixels are 12 contiguous, UNALIGNED source bytes (a row of 3 * RW bytes starts anywhere).  The form kept is the register one:
//   * the thread loads the 3 or 4 ALIGNED dwords that cover its 12 bytes (never a byte load; a dword that holds at least one wanted
//     byte lies in that byte's page, so no load leaves the pages of the region), neighbouring lanes re-reading the dword they share
//     from the same cache line: 16 B requested per 12 B used, HBM traffic once;
//   * three funnel shifts by the byte misalignment give the 12 bytes as three dwords R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3;
//   * the 3-byte deinterleave is byte selects in registers (v_perm_b32 / v_bfe + v_lshl_or), four bytes per plane.
// The LDS form (the wave stages the aligned row segment with coalesced dword loads, lanes then pick their 12 bytes at a 12-byte stride)
// was NOT built: it would replace the one re-read dword per lane, which the L1 serves from the line it already holds, by an LDS round
// trip and a row-sized staging buffer per wave for every S.  Measured, register form, 1024 tiles of 256 x 256 from a 16384^2 slide
// (profiles/wsi_device_kernel_stats.csv, tools/wsi_bench.py --kernel-leg): 89.6 us per launch (84-101) for 2 x 196 608 bytes per tile =
// 403 MB requested, 4.5 TB/s; an element-wise byte compare of two such batches (torch.eq, 604 MB with its output) runs 103 us =
// 5.8 TB/s in the same trace, and the byte compare the README quotes for 151 MB ran at 4.4 TB/s: the gather sits at the rate of the
// byte kernels around it, so nothing was left for the LDS form to win.  (Tiles at resolution 64 overlap their neighbours by 3/4, so
// much of the source side is served by the L2 / Infinity Cache; the 4.5 TB/s are requested bytes, not HBM traffic.)
// Tiles that leave the region, and tile sides that are no multiple of four (or an output base that is not dword-aligned), take the
// per-byte path of the same kernel: a bounds check per pixel, `fill` outside.  All source offsets are int64_t.
#include "kernels.hpp"
#include "wsi_bytes.hpp"   // wsi_fetch12, wsi_plane: shared with the oriented gather of tta.hip

namespace sslcr {

__global__ __launch_bounds__(256) void wsi_gather_kernel(const sslcr_wsi_gather_desc a, const int dword_out) {
  const int S = a.S;
  const int qw = (S + 3) / 4;                                     // dwords per output row
  const size_t total = (size_t)a.N * S * qw;
  const size_t plane = (size_t)S * S;
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(a.src) & 3);
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int q = (int)(t % qw);
    const size_t r = t / qw;
    const int i = (int)(r % S);
    const size_t n = r / S;
    const int64_t x0 = (int64_t)a.xy[2 * n] - a.origin_x + 4 * q;          // source column of the thread's first pixel
    const int64_t y = (int64_t)a.xy[2 * n + 1] - a.origin_y + i;           // source row
    uint8_t* dst = a.dst + (n * 3 * S + i) * (size_t)S + 4 * q;            // plane 0; planes 1, 2 follow at + S * S
    const bool row_in = y >= 0 && y < a.RH;
    if (dword_out && row_in && x0 >= 0 && x0 + 4 <= a.RW) {                // (dword_out implies 4 q + 4 <= S)
      uint32_t d[3];
      wsi_fetch12(a.src, (y * a.RW + x0) * 3, mis, d);
#pragma unroll
      for (int c = 0; c < 3; ++c) *reinterpret_cast<uint32_t*>(dst + c * plane) = wsi_plane(d, c);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        if (4 * q + e >= S) break;
        const int64_t x = x0 + e;
        const bool in = row_in && x >= 0 && x < a.RW;
        const int64_t b = in ? (y * a.RW + x) * 3 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint8_t v = (uint8_t)a.fill;
          if (in) v = a.src[b + c];
          dst[c * plane + e] = v;
        }
      }
    }
  }
}

hipError_t launch_wsi_gather(const sslcr_wsi_gather_desc& a, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const size_t total = (size_t)a.N * a.S * ((a.S + 3) / 4);
  size_t blocks = (total + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  const int dword_out = (a.S & 3) == 0 && (reinterpret_cast<uintptr_t>(a.dst) & 3) == 0;
  hipLaunchKernelGGL(wsi_gather_kernel, dim3((int)blocks), dim3(256), 0, st, a, dword_out);
  return hipGetLastError();
}

}  // namespace sslcr
