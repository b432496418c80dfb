// Bytes in registers.  byte_of: byte i of a little-endian dword, for every kernel that keeps pixels as dwords (augment_v2.hip,
// resample.hip, the gathers below).  The read side of the WSI tile gathers (wsi.hip: wsi_gather_kernel, tta.hip: the oriented gather): four RGB pixels of one region row
// are 12 contiguous, UNALIGNED source bytes; they are fetched as the 3 or 4 ALIGNED dwords that cover them, shifted into three dwords
// and deinterleaved into one dword per colour plane in registers.  wsi.hip's header comment has the reasoning and the measurements.
#pragma once
#include "common.hpp"

namespace sslcr {

// byte i (0..3) of a little-endian dword
__device__ __forceinline__ uint32_t byte_of(uint32_t v, int i) { return (v >> (8 * i)) & 255u; }

// the 12 bytes at src + off as three dwords R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3.  mis = (address of src) & 3.  Never a byte load:
// a dword that holds at least one wanted byte lies in that byte's page, so no load leaves the pages of the region.  The pointer stays
// derived from src (a global-memory kernel argument): plain global loads, not flat ones.
__device__ __forceinline__ void wsi_fetch12(const uint8_t* src, int64_t off, int64_t mis, uint32_t (&d)[3]) {
  const int64_t b = off + mis;                                            // byte offset from the dword-aligned address below src
  const uint32_t* w = reinterpret_cast<const uint32_t*>(src + ((b & ~(int64_t)3) - mis));
  const unsigned sh = 8u * (unsigned)(b & 3);
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
  const uint32_t w3 = w[sh ? 3 : 2];                                      // aligned: the 12 bytes end with w2, and w[3] may lie past the region
  d[0] = (uint32_t)((((uint64_t)w1 << 32) | w0) >> sh);
  d[1] = (uint32_t)((((uint64_t)w2 << 32) | w1) >> sh);
  d[2] = (uint32_t)((((uint64_t)w3 << 32) | w2) >> sh);
}

// bytes k = 0..11 of the three dwords d[0..2] (little endian), picked at stride 3 starting at c: one plane's four pixels
__device__ __forceinline__ uint32_t wsi_plane(const uint32_t d[3], int c) {
  uint32_t v = 0;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int k = 3 * e + c;
    v |= byte_of(d[k >> 2], k & 3) << (8 * e);
  }
  return v;
}

}  // namespace sslcr
