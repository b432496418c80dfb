// Pixels as bytes in registers: P consecutive pixels of one image, one dword per colour plane and four pixels, loaded from and
// stored to either layout (planar [3][H][W] or interleaved [H][W][3]).  Shared by the byte kernels that own four or sixteen
// consecutive output pixels per thread (augment_v2.hip, augment_v1.hip).
#pragma once
#include "wsi_bytes.hpp"   // byte_of

namespace sslcr {

// P consecutive pixels of one image, planar in registers: byte e of w[c] is channel c of pixel p0 + e.  vec: the whole batch is
// P-byte tileable (H*W % P == 0 and a P-byte aligned base: 16 bytes for P = 16, a dword for P = 4), so cnt == P and the accesses are
// P-byte (CHW) / 3P-byte (HWC) words
template <int P>
struct Px { uint32_t w[3][P / 4]; };

template <int P>
__device__ inline void load_px(Px<P>& p, const uint8_t* img, int hwc, size_t hw, size_t p0, int cnt, bool vec) {
  constexpr int Q = P / 4;
  if (vec) {
    if (!hwc) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const uint32_t* s = reinterpret_cast<const uint32_t*>(img + c * hw + p0);
        if constexpr (Q == 4) {
          const uint4 v = *reinterpret_cast<const uint4*>(s);
          p.w[c][0] = v.x; p.w[c][1] = v.y; p.w[c][2] = v.z; p.w[c][3] = v.w;
        } else {
          p.w[c][0] = s[0];
        }
      }
    } else {
      uint32_t raw[3 * Q];
      const uint32_t* s = reinterpret_cast<const uint32_t*>(img + p0 * 3);
      if constexpr (Q == 4) {
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          const uint4 v = reinterpret_cast<const uint4*>(s)[i];
          raw[4 * i] = v.x; raw[4 * i + 1] = v.y; raw[4 * i + 2] = v.z; raw[4 * i + 3] = v.w;
        }
      } else {
        raw[0] = s[0]; raw[1] = s[1]; raw[2] = s[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          uint32_t v = 0;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int k = 3 * (4 * q + e) + c;         // byte k of the interleaved run
            v |= byte_of(raw[k >> 2], k & 3) << (8 * e);
          }
          p.w[c][q] = v;
        }
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      uint32_t v = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int i = 4 * q + e;
        if (i < cnt) v |= (uint32_t)img[hwc ? (p0 + i) * 3 + c : c * hw + p0 + i] << (8 * e);
      }
      p.w[c][q] = v;
    }
}

template <int P>
__device__ inline void store_px(const Px<P>& p, uint8_t* img, int hwc, size_t hw, size_t p0, int cnt, bool vec) {
  constexpr int Q = P / 4;
  if (vec) {
    if (!hwc) {
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        uint32_t* d = reinterpret_cast<uint32_t*>(img + c * hw + p0);
        if constexpr (Q == 4) *reinterpret_cast<uint4*>(d) = make_uint4(p.w[c][0], p.w[c][1], p.w[c][2], p.w[c][3]);
        else d[0] = p.w[c][0];
      }
    } else {
      uint32_t raw[3 * Q];
#pragma unroll
      for (int i = 0; i < 3 * Q; ++i) {
        uint32_t v = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int k = 4 * i + b;                     // byte k of the interleaved run = channel k % 3 of pixel k / 3
          v |= byte_of(p.w[k % 3][(k / 3) >> 2], (k / 3) & 3) << (8 * b);
        }
        raw[i] = v;
      }
      uint32_t* d = reinterpret_cast<uint32_t*>(img + p0 * 3);
      if constexpr (Q == 4) {
#pragma unroll
        for (int i = 0; i < 3; ++i) reinterpret_cast<uint4*>(d)[i] = make_uint4(raw[4 * i], raw[4 * i + 1], raw[4 * i + 2], raw[4 * i + 3]);
      } else {
        d[0] = raw[0]; d[1] = raw[1]; d[2] = raw[2];
      }
    }
    return;
  }
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int i = 0; i < P; ++i)
      if (i < cnt) img[hwc ? (p0 + i) * 3 + c : c * hw + p0 + i] = (uint8_t)byte_of(p.w[c][i >> 2], i & 3);
}

}  // namespace sslcr
