// Test-time augmentation over the dihedral group D4 (library version 13): the eight flips and quarter turns of a square tile, applied
// to bytes that already sit in HBM, and the reduction of G sets of logits to one score per tile.  include/sslcr.h pins the codes:
//     d4(t, g)[i][j] = t[si][sj],  k = g & 3, f = g >> 2,  (a, b) = (k & 1) ? (j, i) : (i, j),
//     si = (k >> 1) ? S-1-a : a,   sj = ((((k + 1) >> 1) & 1) ^ f) ? S-1-b : b
// = np.rot90(t[..., ::-1] if f else t, k).  A code is uniform over a tile, so every branch on it is uniform over a workgroup.
//
// Byte planes (d4_bytes_kernel: the oriented WSI gather and the uint8 batch transform share it; they differ in how four source pixels
// of a row are fetched).  A workgroup step is one 64 x 64 pixel block of one tile, all of its planes.
//   * Even k (no transpose): the register form of wsi_gather_kernel.  A thread owns four consecutive output pixels of a row = one
//     dword per plane; its source is four consecutive pixels of ONE source row, fetched in whole dwords, byte-reversed (one v_perm)
//     when the columns run backwards.  No LDS, and the step is a strip of whole rows, not a square (see the branch).
//   * Odd k (a transpose of byte planes): the source block is read along its rows exactly as above and written to LDS one dword per
//     plane; after a barrier a thread turns one 4 x 4 pixel block: it reads the four LDS dwords (4 q + k, cq), k = 0..3 -- four
//     source rows, one column dword -- transposes the 16 bytes in registers and writes output dword q of four consecutive output
//     rows, one plane at a time.  Neither side of HBM sees a column walk, and LDS sees no byte access: a byte-granular column read
//     (ds_read_u8, four per output dword) has a row stride of 4 * pitch dwords between a wave's neighbouring lanes, which no pitch
//     spreads over more than 8 of the 32 banks a ds_read_b32-class access is banked on.
//     LDS row pitch: 17 dwords (64 pixels + 1), word address (4 q + k) * 17 + cq.  ds_read_b32 is served in two groups of 32 lanes on
//     (address / 4) mod 32.  With the lane order q = lane[2:0] + 8 lane[5], rq = lane[4:3] (+ 4 per wave) a group holds q = 8 h .. 8 h + 7
//     and four rq: banks (68 q + 17 k + cq) mod 32 = (4 q + cq + const) mod 32 with cq four consecutive values (either direction) --
//     32 distinct banks; a pitch of 16 would put a group's eight q on one bank.  The store side is ds_write_b32 at ar * 17 + q',
//     a group = two source rows of 16 dwords: banks 0..15 and 17..32, one bank hit twice, which costs a ds_write_b32 nothing (the
//     store's register transfer, not the array, sets its time).  A wave's global store is 4 rows x 64 contiguous bytes either way.
//     13 KB of LDS per workgroup.
//   * Sides that are no multiple of four, or bases that are not dword aligned, take the per-element path: one byte per plane and
//     pixel with the same index arithmetic (as wsi_gather_kernel's per-byte path).
// 4-byte elements (d4_words_kernel, float32 batches of a host loader): the classic 32 x 32 dword transpose through LDS at pitch 33 for
// odd k, a plain reversed copy for even k; every side is served by the one path since an element is a dword.
// All offsets are int64_t / size_t; operands stay kernel-argument globals.  No floating point, no atomics.
// Measured, 1024 tiles of 256 x 256 from a 16384^2 slide, per launch, one profiler trace each (profiles/wsi_tta_kernel_stats.csv,
// profiles/wsi_tta_kernel_stats_warm.csv; tools/wsi_bench.py --kernel-leg --tta d4 [--tta-warm]), beside the plain gather of the same
// trace (91 us, 86-100):
//   source not in the caches (every launch the next batch, as the plain gather's loop):  even k 89-91 us, odd k 134-135 us
//   source read just before (the G - 1 later members of a batch in camelyon16_test):     even k 63-69 us, odd k  89-91 us
// The transposes pay 45 us for a cold source where the reversals pay 26: a workgroup's 64 source rows (192 bytes each, 49 KB apart)
// must all have arrived before its barrier lets the first store go, so the slowest row's latency is exposed once per block, where the
// register form lets every wave store as soon as ITS rows are there.  Two blocks in flight per workgroup would hide it; not built --
// with args.tta = "d4" the cold member is code 0, and 8 members cost 1.006 x 8 plain batches of stream time (profiles/wsi_tta_bench.json).
//
// predict_tta_kernel: one row per thread.  The members' softmax statistics first (the device function of sslcr_predict, softmax_row.hpp),
// then per class the left-to-right fp32 sum of the members and ONE division by (float)G.  This file is built with -ffp-contract=off
// (build.py): the sum and the quotient are plain IEEE operations, so a host restatement in float32 has the same bits.
#include "kernels.hpp"
#include "softmax_row.hpp"
#include "wsi_bytes.hpp"

namespace sslcr {

struct D4 { int T, ri, rj; };   // transpose, then: source row reversed, source column reversed
__device__ __forceinline__ D4 d4_decode(int g) {
  const int k = g & 3, f = (g >> 2) & 1;
  return {k & 1, k >> 1, (((k + 1) >> 1) & 1) ^ f};
}

// ---- the two sources of d4_bytes_kernel.  unit: what locates unit u; load4: four consecutive source pixels (row, col0 .. col0 + 3) of it, one dword per plane
// (pixel e in byte e); load1: one byte.  `row` and `col0 .. col0 + 3` lie inside the tile.
struct D4GatherSrc {            // unit = tile, three planes, HWC source region with `fill` outside
  static constexpr int P = 3;
  sslcr_wsi_gather_desc a;
  struct Unit { int64_t x, y; };          // region coordinates of the tile's pixel (0, 0)
  __device__ __forceinline__ size_t code_index(size_t u) const { return u; }
  __device__ __forceinline__ Unit unit(size_t u) const { return {(int64_t)a.xy[2 * u] - a.origin_x, (int64_t)a.xy[2 * u + 1] - a.origin_y}; }
  __device__ __forceinline__ void load4(const Unit& t, int row, int col0, int64_t mis, uint32_t (&v)[3]) const {
    const int64_t x0 = t.x + col0;
    const int64_t y = t.y + row;
    const bool row_in = y >= 0 && y < a.RH;
    if (row_in && x0 >= 0 && x0 + 4 <= a.RW) {
      uint32_t d[3];
      wsi_fetch12(a.src, (y * a.RW + x0) * 3, mis, d);
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = wsi_plane(d, c);
    } else {
#pragma unroll
      for (int c = 0; c < 3; ++c) v[c] = 0;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int64_t x = x0 + e;
        const bool in = row_in && x >= 0 && x < a.RW;
        const int64_t b = in ? (y * a.RW + x) * 3 : 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          uint32_t byte = (uint32_t)a.fill;
          if (in) byte = a.src[b + c];
          v[c] |= byte << (8 * e);
        }
      }
    }
  }
  __device__ __forceinline__ uint32_t load1(const Unit& t, int row, int col, int c) const {
    const int64_t x = t.x + col;
    const int64_t y = t.y + row;
    uint32_t byte = (uint32_t)a.fill;
    if (y >= 0 && y < a.RH && x >= 0 && x < a.RW) byte = a.src[(y * a.RW + x) * 3 + c];
    return byte;
  }
};
struct D4PlaneSrc {             // unit = one plane of one image of a uint8 batch [N][Cn][S][S]
  static constexpr int P = 1;
  const uint8_t* src;
  int S, Cn;
  struct Unit { size_t base; };           // offset of the plane
  __device__ __forceinline__ size_t code_index(size_t u) const { return u / (size_t)Cn; }
  __device__ __forceinline__ Unit unit(size_t u) const { return {u * S * (size_t)S}; }
  __device__ __forceinline__ void load4(const Unit& t, int row, int col0, int64_t, uint32_t (&v)[1]) const {   // dword path only: aligned
    v[0] = *reinterpret_cast<const uint32_t*>(src + t.base + (size_t)row * S + col0);
  }
  __device__ __forceinline__ uint32_t load1(const Unit& t, int row, int col, int) const { return src[t.base + (size_t)row * S + col]; }
};

constexpr int D4_BLK = 64;                // pixels per side of a staged block
constexpr int D4_PITCH = D4_BLK / 4 + 1;  // LDS row pitch in dwords (see the header comment)

template <class Src>
__global__ __launch_bounds__(256) void d4_bytes_kernel(const Src s, uint8_t* dst, const int32_t* orient, const int S, const int64_t units,
                                                       const int dword_io, const int64_t mis) {
  constexpr int P = Src::P;
  __shared__ uint32_t lds[P][D4_BLK * D4_PITCH];
  const int nb = (S + D4_BLK - 1) / D4_BLK;
  const size_t plane = (size_t)S * S;
  const int64_t work = units * nb * nb;
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int bj = (int)(w % nb), bi = (int)((w / nb) % nb);
    const size_t u = (size_t)(w / ((int64_t)nb * nb));
    // the tile's coordinates are fetched BESIDE its code, not behind it: one dependent round trip before the first source load, as in
    // wsi_gather_kernel.  (Behind it, the reversals of a cold batch of 1024 tiles of 256 x 256 ran 101-102 us per launch beside a plain
    // gather of 87 us; beside it, 82-83 us in the next trace.)
    const typename Src::Unit tile = s.unit(u);
    const D4 o = d4_decode(orient[s.code_index(u)]);
    const int i0 = bi * D4_BLK, j0 = bj * D4_BLK;
    const int bh = min(D4_BLK, S - i0), bw = min(D4_BLK, S - j0);       // the output block: rows i0 .. i0 + bh, columns j0 .. j0 + bw
    uint8_t* d = dst + u * P * plane;
    if (!dword_io) {
      for (int e = tid; e < bh * bw; e += 256) {
        const int i = i0 + e / bw, j = j0 + e % bw;
        const int a = o.T ? j : i, b = o.T ? i : j;
        const int si = o.ri ? S - 1 - a : a, sj = o.rj ? S - 1 - b : b;
#pragma unroll
        for (int c = 0; c < P; ++c) d[c * plane + (size_t)i * S + j] = (uint8_t)s.load1(tile, si, sj, c);
      }
    } else if (!o.T) {
      // nothing is staged, so the step need not be square: the tile's nb * nb steps are strips of whole rows instead, and a wave
      // reads and writes a row's full width in one piece, as wsi_gather_kernel does
      const int rows = (S + nb * nb - 1) / (nb * nb), r0 = (bi * nb + bj) * rows, r1 = min(S, r0 + rows);
      const int qw = S / 4;
      for (int e = tid; e < (r1 - r0) * qw; e += 256) {
        const int i = r0 + e / qw, j = 4 * (e % qw);
        const int si = o.ri ? S - 1 - i : i, sj0 = o.rj ? S - 4 - j : j;
        uint32_t v[P];
        s.load4(tile, si, sj0, mis, v);
#pragma unroll
        for (int c = 0; c < P; ++c)
          *reinterpret_cast<uint32_t*>(d + c * plane + (size_t)i * S + j) = o.rj ? __builtin_bswap32(v[c]) : v[c];
      }
    } else {
      // source block: its rows are the output's columns (bw of them), its columns the output's rows (bh)
      const int a0 = o.ri ? S - j0 - bw : j0, b0 = o.rj ? S - i0 - bh : i0;
      const int qb = bh / 4, qw = bw / 4;
      for (int e = tid; e < bw * qb; e += 256) {
        const int ar = e / qb, q = e % qb;
        uint32_t v[P];
        s.load4(tile, a0 + ar, b0 + 4 * q, mis, v);
#pragma unroll
        for (int c = 0; c < P; ++c) lds[c][ar * D4_PITCH + q] = v[c];
      }
      __syncthreads();
      for (int e = tid; e < qb * qw; e += 256) {
        // a thread turns one 4 x 4 pixel block: output dword q of the output rows 4 rq .. 4 rq + 3
        int q = e % qw, rq = e / qw;
        if (qw == 16 && qb == 16) {                                                 // a full block width: the bank-free lane order (header comment)
          q = (e & 7) | ((e >> 5 & 1) << 3);
          rq = (e >> 6) * 4 + (e >> 3 & 3);
        }
        const int cq = o.rj ? qb - 1 - rq : rq;                          // the LDS column dword that holds those four output rows
#pragma unroll
        for (int c = 0; c < P; ++c) {
          uint32_t r[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) r[k] = lds[c][(o.ri ? bw - 1 - (4 * q + k) : 4 * q + k) * D4_PITCH + cq];
#pragma unroll
          for (int m = 0; m < 4; ++m) {
            const int sh = 8 * (o.rj ? 3 - m : m);
            const uint32_t x = ((r[0] >> sh) & 0xffu) | ((r[1] >> sh) & 0xffu) << 8 | ((r[2] >> sh) & 0xffu) << 16 | (r[3] >> sh) << 24;
            *reinterpret_cast<uint32_t*>(d + c * plane + (size_t)(i0 + 4 * rq + m) * S + j0 + 4 * q) = x;
          }
        }
      }
      __syncthreads();                                                  // the next step of this workgroup overwrites the block
    }
  }
}

constexpr int D4W_BLK = 32, D4W_PITCH = 33;

__global__ __launch_bounds__(256) void d4_words_kernel(const uint32_t* src, uint32_t* dst, const int32_t* orient, const int S, const int Cn,
                                                       const int64_t units) {
  __shared__ uint32_t lds[D4W_BLK * D4W_PITCH];
  const int nb = (S + D4W_BLK - 1) / D4W_BLK;
  const size_t plane = (size_t)S * S;
  const int64_t work = units * nb * nb;
  const int tid = threadIdx.x;
  for (int64_t w = blockIdx.x; w < work; w += gridDim.x) {
    const int bj = (int)(w % nb), bi = (int)((w / nb) % nb);
    const size_t u = (size_t)(w / ((int64_t)nb * nb));
    const D4 o = d4_decode(orient[u / (size_t)Cn]);
    const int i0 = bi * D4W_BLK, j0 = bj * D4W_BLK;
    const int bh = min(D4W_BLK, S - i0), bw = min(D4W_BLK, S - j0);
    const uint32_t* sp = src + u * plane;
    uint32_t* dp = dst + u * plane;
    if (!o.T) {
      for (int e = tid; e < bh * bw; e += 256) {
        const int i = i0 + e / bw, j = j0 + e % bw;
        const int si = o.ri ? S - 1 - i : i, sj = o.rj ? S - 1 - j : j;
        dp[(size_t)i * S + j] = sp[(size_t)si * S + sj];
      }
    } else {
      const int a0 = o.ri ? S - j0 - bw : j0, b0 = o.rj ? S - i0 - bh : i0;
      for (int e = tid; e < bw * bh; e += 256) {
        const int ar = e / bh, bc = e % bh;
        lds[ar * D4W_PITCH + bc] = sp[(size_t)(a0 + ar) * S + b0 + bc];
      }
      __syncthreads();
      for (int e = tid; e < bh * bw; e += 256) {
        const int li = e / bw, lj = e % bw;
        const int ar = o.ri ? bw - 1 - lj : lj, bc = o.rj ? bh - 1 - li : li;
        dp[(size_t)(i0 + li) * S + j0 + lj] = lds[ar * D4W_PITCH + bc];
      }
      __syncthreads();
    }
  }
}

static int d4_grid(int64_t units, int S, int blk) {
  const int64_t nb = (S + blk - 1) / blk;
  const int64_t work = units * nb * nb;
  return (int)(work < (1 << 18) ? work : (1 << 18));
}

hipError_t launch_wsi_gather_d4(const sslcr_wsi_gather_desc& a, const int32_t* orient, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const int dword_io = (a.S & 3) == 0 && (reinterpret_cast<uintptr_t>(a.dst) & 3) == 0;
  const int64_t mis = (int64_t)(reinterpret_cast<uintptr_t>(a.src) & 3);
  hipLaunchKernelGGL(d4_bytes_kernel<D4GatherSrc>, dim3(d4_grid(a.N, a.S, D4_BLK)), dim3(256), 0, st, D4GatherSrc{a}, a.dst, orient, a.S,
                     (int64_t)a.N, dword_io, mis);
  return hipGetLastError();
}

hipError_t launch_d4_transform(const sslcr_d4_desc& a, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const int S = a.H;
  const int64_t units = (int64_t)a.N * a.Cn;
  if (a.elem_bytes == 4) {
    hipLaunchKernelGGL(d4_words_kernel, dim3(d4_grid(units, S, D4W_BLK)), dim3(256), 0, st, static_cast<const uint32_t*>(a.src),
                       static_cast<uint32_t*>(a.dst), a.orient, S, a.Cn, units);
  } else {
    const int dword_io = (S & 3) == 0 && ((reinterpret_cast<uintptr_t>(a.src) | reinterpret_cast<uintptr_t>(a.dst)) & 3) == 0;
    hipLaunchKernelGGL(d4_bytes_kernel<D4PlaneSrc>, dim3(d4_grid(units, S, D4_BLK)), dim3(256), 0, st,
                       D4PlaneSrc{static_cast<const uint8_t*>(a.src), S, a.Cn}, static_cast<uint8_t*>(a.dst), a.orient, S, units, dword_io,
                       (int64_t)0);
  }
  return hipGetLastError();
}

// sslcr_predict_tta.  The confusion matrix as predict_kernel counts it (softmax_row.hpp) -- one count per ROW, whatever G.
__global__ __launch_bounds__(256) void predict_tta_kernel(const sslcr_predict_tta_desc t) {
  __shared__ unsigned cells[CONFUSION_MAX_C * CONFUSION_MAX_C];
  const sslcr_predict_desc& a = t.p;
  const int C = a.C, G = t.G;
  if (a.confusion) confusion_clear(cells, C * C);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i < a.n) {
    const size_t set = (size_t)a.n * C;                                  // floats between two members' logits
    const float* l0 = a.logits + i * C;
    float m[SSLCR_TTA_MAX], s[SSLCR_TTA_MAX];
#pragma unroll
    for (int g = 0; g < SSLCR_TTA_MAX; ++g) {
      m[g] = 0.f;
      s[g] = 1.f;
      if (t.mode == 0 && g < G) softmax_row_stats(l0 + g * set, C, m[g], s[g]);
    }
    const float div = (float)G;
    int b = 0;
    float best = 0.f;
    for (int c = 0; c < C; ++c) {
      float acc = 0.f;
#pragma unroll
      for (int g = 0; g < SSLCR_TTA_MAX; ++g) {
        if (g < G) {
          const float* l = l0 + g * set;
          const float p = t.mode == 0 ? softmax_value(l, c, m[g], s[g]) : l[c];
          acc = g == 0 ? p : acc + p;                                    // left to right, one IEEE add per member
        }
      }
      const float v = acc / div;
      if (a.scores) a.scores[i * C + c] = v;
      if (a.map && c == a.col) {
        const int64_t k = a.map_index[i];
        if (k >= 0 && k < a.map_size) a.map[k] = v;
      }
      const float key = G == 1 ? l0[c] : v;                              // G == 1: sslcr_predict's own argmax, over the logits
      if (c == 0) {
        best = key;
      } else {
        argmax_step(best, b, key, c);
      }
    }
    if (a.pred) a.pred[i] = b;
    if (a.confusion) confusion_count(cells, C, a.target[i], b);
  }
  if (a.confusion) confusion_flush(cells, C * C, a.confusion);
}

hipError_t launch_predict_tta(const sslcr_predict_tta_desc& a, hipStream_t st) {
  if (a.p.n == 0) return hipSuccess;
  hipLaunchKernelGGL(predict_tta_kernel, dim3(cdiv(a.p.n, 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace sslcr
