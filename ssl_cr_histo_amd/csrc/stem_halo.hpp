// What the stem kernels of stem.hip (stem_fwd_kernel, stem_wgrad_kernel, stem_wgrad_pool2_kernel) and stem_pool.hip
// (stem_pool_fwd_kernel) share: the input halo of a tile of conv1 (7x7 stride 2 pad 3) outputs -- HR rows x STEM_HC columns x 4 channels
// of the planar NCHW image, 4th channel = 0.  The halo rows HR (21 for an 8-row tile, 37 for a 16-row one) are a template argument:
// every bound is a compile-time constant.
// NOT here, although both files have one: the halo WRITES (stem_commit4 / sp_commit4, stem_load_halo / sp_load_halo), the weight
// staging and the bf16 MFMA loop over the 7 filter rows.  The two files form the LDS address and the stored value in opposite
// order, the instruction scheduler keeps that order, and a hot instance's registers and schedule are part of its interface
// (DESIGN.md): one text for both changes the code of stem_fwd_kernel<bf16, uint8> or of stem_pool_fwd_kernel, whichever order it
// takes (checked with tools/device_code_diff.sh, function by function).
#pragma once
#include "common.hpp"

namespace sslcr {

constexpr int STEM_HC = 2 * 16 + 6;            // 38 halo columns of a 16-column tile (even, covers the zero-weight tap s=7)

// kout owned by MFMA tile t, fragment row group q (= lane>>2 for the A fragment, lane>>4 for the accumulator), element j:
// a lane's 16 channels form two 8-channel runs 32 channels apart, so the four lane groups of one pixel write contiguous
// 64-byte segments (16 consecutive channels per lane would leave every 16-byte store half of a 32-byte stride)
#define STEM_CH(t, q, j) ((((t) >> 1) * 32) + ((q) * 8) + (((t) & 1) * 4) + (j))

// Image n of a (possibly two-segment) input batch: the reference's torch.cat((inputs_x, inputs_u_s)) is an address select here.
template <typename A>
__device__ __forceinline__ const void* stem_seg(const A& a, int& n) {
  if (a.x2 && n >= a.n_split) { n -= a.n_split; return a.x2; }
  return a.x;
}

// uint8 fast path (W % 4 == 0): the halo window starts 3 pixels left of a 32-pixel boundary, so the aligned dwords from
// one pixel further left cover it exactly: thread (row rr = tid/10, dword d = tid%10) of the first 10 HR loads ONE dword per
// colour plane = 4 pixels x 3 channels, and the commit writes them as four 8-byte (c0,c1,c2,0) pixels.  12 bytes per load-triple and
// 4 LDS stores per thread per tile instead of 10 byte loads + 10 two-byte stores with per-element address arithmetic.
// The issue puts the next tile's input bytes in flight; the commit converts and writes them into the OTHER LDS halo buffer after the
// current tile's MFMAs -- the HBM latency of the planar uint8 gather hides under compute instead of sitting between two barriers.
struct StemRaw { uint32_t d[3]; };
template <int HR>
__device__ __forceinline__ StemRaw stem_issue4(const void* xv, int n, int H, int W, int hi0, int wi0, int tid = threadIdx.x) {
  StemRaw r{{0u, 0u, 0u}};
  if (tid < HR * 10) {
    const int rr = tid / 10, d = tid - rr * 10;
    const int h = hi0 + rr, w = wi0 - 1 + 4 * d;
    if (h >= 0 && h < H && w >= 0 && w < W) {
      const uint8_t* p = reinterpret_cast<const uint8_t*>(xv) + ((size_t)(n * 3) * H + h) * W + w;
      const size_t plane = (size_t)H * W;
#pragma unroll
      for (int c = 0; c < 3; ++c) r.d[c] = *reinterpret_cast<const uint32_t*>(p + c * plane);
    }
  }
  return r;
}

}  // namespace sslcr
