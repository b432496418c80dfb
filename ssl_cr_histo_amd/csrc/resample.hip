// Pillow-exact resize of uint8 L / RGB batches in HBM (include/sslcr.h, "Pillow-exact image resize"): Image.resize(size, resample, box)
// byte for byte.  Replaces the transforms.Resize(size=args.image_size) that every BreastPathQ validation / test patch passes through on
// the host, one PIL image at a time (eval_BreastPathQ_SSL_CR.py:325,365, eval_BreastPathQ_SSL.py:290,319, dataset.py:575-599).
//
// The coefficient tables are made on the host (sslcr_resample_coeffs, capi.cpp: the double arithmetic and the libm Pillow itself uses);
// everything here is integer: a pass is out = clip((sum_x in[xmin + x] * k[x] + 2^21) >> 22), horizontal first, rounded to a byte, then
// vertical.  sslcr_resample_table_ok is the precondition that lets a pass accumulate in int32 and multiply with v_mul_i32_i24
// (pixel < 2^8, |k| < 2^23: both inside the signed 24-bit operands, the product exact in 32 bits).
//
// Forms (resample_plan, the one place that decides):
//   fused     a workgroup owns RS_TH x RS_TW output pixels of one image.  (1) the tile's slices of kx / bx / ky / by go to LDS;
//             (2) the source rows [by[first].min, by[last].end) x columns [bx[first].min, bx[last].end) -- both ranges are monotone in
//             the output index -- are staged with whole ALIGNED dword loads, segment by segment (a row of HWC, a row of one plane of
//             CHW), each segment keeping its own misalignment: a row pitch of 53 * 3 bytes starts anywhere, and a dword that holds
//             one wanted byte lies in that byte's page (wsi.hip's argument); (3) the horizontal pass reads bytes from that image and
//             writes the rounded intermediate PLANAR, four pixels per lane as one dword; (4) barrier; the vertical pass reads one
//             dword per tap and lane -- lanes run along a row, so the coefficient is the same LDS word for 16 lanes, a broadcast -- and
//             stores whole dwords: 4 pixels of a plane (CHW), or 4 RGB pixels = 3 dwords (HWC; augment_v2.hip's apply pass reads
//             them the same way).  Rows and row ends whose address is no multiple of 4, or that hold fewer than 4 pixels, take byte
//             stores.  HBM sees each source byte once apart from the overlap of neighbouring tiles; the intermediate stays in the CU.
//   two-pass  horizontal launch into a planar workspace, vertical launch from it: every descriptor whose fused tile would not fit
//             SSLCR_RESAMPLE_LDS_CAP (large down-scales).  The same pass kernel serves the single-axis descriptors.
//   gather    NEAREST (bx / by hold source indices) and the copy between layouts (no table).
// Every range read from a device table is clamped to the image and to the staged tile: a wrong table cannot leave the buffers.
#include <string.h>

#include "kernels.hpp"
#include "wsi_bytes.hpp"   // byte_of

namespace sslcr {
namespace {

constexpr int RS_TW = 64, RS_TH = 16;      // the fused tile: 16 lanes of pixel quads x 16 rows = one item per thread in the vertical pass
constexpr int RS_BITS = 22;                // Pillow's PRECISION_BITS = 32 - 8 - 2
constexpr int RS_HALF = 1 << (RS_BITS - 1);

struct Lay { int64_t img, row, cs; int ps; };        // byte strides of an image, a row, a channel and a pixel
__host__ __device__ inline Lay lay_of(int chw, int C, int H, int W) {
  Lay l;
  l.img = (int64_t)C * H * W;
  if (chw) { l.row = W; l.ps = 1; l.cs = (int64_t)H * W; }
  else { l.row = (int64_t)W * C; l.ps = C; l.cs = 1; }
  return l;
}
// clip(acc >> 22, 0, 255), written as clamp-then-shift: v_med3_i32 + v_lshrrev_b32.  The shift-then-clamp spelling selects
// v_ashr_pk_u8_i32, which packs two results into bits 15:0 of its destination, and the ORs that add bytes 2 and 3 of a quad rely on
// bits 31:16 of that register being zero, which this kernel's bytes 2 and 3 showed they are not.  To check: spell it
// min(max(acc >> RS_BITS, 0), 255), look for the instruction in the fused kernel's ISA, run tests/test_resize_gpu.py.
__device__ inline uint32_t clip8(int acc) { return (uint32_t)min(max(acc, 0), (256 << RS_BITS) - 1) >> RS_BITS; }
__device__ inline int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
__device__ inline int table_of(const int32_t* table_index, int T, int64_t n) { return table_index ? clampi(table_index[n], 0, T - 1) : 0; }

// pixels x .. x + 3 (x % 4 == 0; those below OW) of row y of one image: v[c] holds the four bytes of channel c
__device__ inline void store_quad(uint8_t* img, int chw, int C, int OH, int OW, int y, int x, const uint32_t (&v)[3]) {
  const int n = min(4, OW - x);
  if (chw || C == 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= C) break;
      uint8_t* p = img + ((int64_t)c * OH + y) * OW + x;
      if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {
        *reinterpret_cast<uint32_t*>(p) = v[c];
      } else {
        for (int e = 0; e < n; ++e) p[e] = (uint8_t)byte_of(v[c], e);
      }
    }
  } else {
    uint8_t* p = img + ((int64_t)y * OW + x) * 3;
    if (n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) {      // R0 G0 B0 R1 | G1 B1 R2 G2 | B2 R3 G3 B3
      uint32_t* q = reinterpret_cast<uint32_t*>(p);
      q[0] = byte_of(v[0], 0) | byte_of(v[1], 0) << 8 | byte_of(v[2], 0) << 16 | byte_of(v[0], 1) << 24;
      q[1] = byte_of(v[1], 1) | byte_of(v[2], 1) << 8 | byte_of(v[0], 2) << 16 | byte_of(v[1], 2) << 24;
      q[2] = byte_of(v[2], 2) | byte_of(v[0], 3) << 8 | byte_of(v[1], 3) << 16 | byte_of(v[2], 3) << 24;
    } else {
      for (int e = 0; e < n; ++e) {
#pragma unroll
        for (int c = 0; c < 3; ++c) p[3 * e + c] = (uint8_t)byte_of(v[c], e);
      }
    }
  }
}

// n <= 4 pixels at pixel stride ps from p, as the bytes of one dword: one aligned load where the four are one
__device__ inline uint32_t load_quad(const uint8_t* p, int ps, int n) {
  if (ps == 1 && n == 4 && (reinterpret_cast<uintptr_t>(p) & 3) == 0) return *reinterpret_cast<const uint32_t*>(p);
  uint32_t d = 0;
  for (int e = 0; e < n; ++e) d |= (uint32_t)p[(int64_t)e * ps] << (8 * e);
  return d;
}

__global__ __launch_bounds__(256) void resample_gather_kernel(const sslcr_resample_desc a) {
  const int qw = (a.OW + 3) / 4;
  const size_t total = (size_t)a.N * a.OH * qw;
  const Lay s = lay_of(a.src_chw, a.C, a.IH, a.IW);
  const int64_t dimg = (int64_t)a.C * a.OH * a.OW;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int q = (int)(i % qw);
    const size_t r = i / qw;
    const int y = (int)(r % a.OH);
    const int64_t n = (int64_t)(r / a.OH);
    const int ti = table_of(a.table_index, a.T, n);
    const int sy = clampi(a.by ? a.by[((int64_t)ti * a.OH + y) * 2] : y, 0, a.IH - 1);
    const uint8_t* row = a.src + n * s.img + sy * s.row;
    uint32_t v[3] = {0, 0, 0};
    for (int e = 0; e < 4; ++e) {
      const int xx = 4 * q + e;
      if (xx >= a.OW) break;
      const int sx = clampi(a.bx ? a.bx[((int64_t)ti * a.OW + xx) * 2] : xx, 0, a.IW - 1);
#pragma unroll
      for (int c = 0; c < 3; ++c)
        if (c < a.C) v[c] |= (uint32_t)row[(int64_t)sx * s.ps + c * s.cs] << (8 * e);
    }
    store_quad(a.dst + n * dimg, a.dst_chw, a.C, a.OH, a.OW, y, 4 * q, v);
  }
}

// One pass, global memory to global memory.  AXIS 0: horizontal, [SH][SW] -> [SH][OW] (OH == SH); AXIS 1: vertical, [SH][SW] -> [OH][SW]
// (OW == SW).  A thread owns four consecutive output pixels of a row, all channels.
template <int AXIS>
__global__ __launch_bounds__(256) void resample_pass_kernel(const uint8_t* src, const Lay s, uint8_t* dst, const int dst_chw, const int32_t* k,
                                                            const int32_t* b, const int32_t* table_index, const int T, const int ks, const int N,
                                                            const int C, const int SH, const int SW, const int OH, const int OW) {
  const int qw = (OW + 3) / 4;
  const size_t total = (size_t)N * OH * qw;
  const int64_t dimg = (int64_t)C * OH * OW;
  const int on = AXIS == 0 ? OW : OH;             // rows of the table set
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int q = (int)(i % qw);
    const size_t r = i / qw;
    const int y = (int)(r % OH);
    const int64_t n = (int64_t)(r / OH);
    const int ti = table_of(table_index, T, n);
    const uint8_t* img = src + n * s.img;
    const int nq = min(4, OW - 4 * q);
    uint32_t v[3] = {0, 0, 0};
    if (AXIS == 0) {
      const uint8_t* row = img + y * s.row;
      for (int e = 0; e < nq; ++e) {
        const int64_t t0 = (int64_t)ti * on + 4 * q + e;
        const int lo = clampi(b[2 * t0], 0, SW);
        const int cnt = clampi(b[2 * t0 + 1], 0, min(SW - lo, ks));
        const int32_t* kk = k + t0 * ks;
        int acc[3] = {RS_HALF, RS_HALF, RS_HALF};
        for (int t = 0; t < cnt; ++t) {
          const uint8_t* p = row + (int64_t)(lo + t) * s.ps;
          const int w = kk[t];
#pragma unroll
          for (int c = 0; c < 3; ++c)
            if (c < C) acc[c] += __mul24((int)p[c * s.cs], w);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] |= clip8(acc[c]) << (8 * e);
      }
    } else {
      const int64_t t0 = (int64_t)ti * on + y;
      const int lo = clampi(b[2 * t0], 0, SH);
      const int cnt = clampi(b[2 * t0 + 1], 0, min(SH - lo, ks));
      const int32_t* kk = k + t0 * ks;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        if (c >= C) break;
        int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
        const uint8_t* p = img + c * s.cs + (int64_t)lo * s.row + (int64_t)(4 * q) * s.ps;
        for (int t = 0; t < cnt; ++t, p += s.row) {
          const uint32_t d = load_quad(p, s.ps, nq);
          const int w = kk[t];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[e] += __mul24((int)byte_of(d, e), w);
        }
        v[c] = clip8(acc[0]) | clip8(acc[1]) << 8 | clip8(acc[2]) << 16 | clip8(acc[3]) << 24;
      }
    }
    store_quad(dst + n * dimg, dst_chw, C, OH, OW, y, 4 * q, v);
  }
}

// the fused kernel's LDS image, from the plan's (rows, cols): every offset a multiple of 16
struct FusedCarve { int64_t kx, bx, ky, by, in, tmp, total; int seg_stride; };
__host__ __device__ inline FusedCarve fused_carve(int C, int src_chw, int ksx, int ksy, int rows, int cols) {
  FusedCarve f;
  int64_t o = 0;
  f.kx = o; o += ((int64_t)RS_TW * ksx * 4 + 15) & ~(int64_t)15;
  f.bx = o; o += RS_TW * 2 * 4;
  f.ky = o; o += ((int64_t)RS_TH * ksy * 4 + 15) & ~(int64_t)15;
  f.by = o; o += RS_TH * 2 * 4;
  // a staged segment: its bytes, up to 3 bytes of misalignment in front, rounded up to whole dwords (and to 16 for the carve)
  const int64_t seg = (((int64_t)(src_chw ? cols : (int64_t)cols * C) + 3 + 3) & ~(int64_t)3);
  f.seg_stride = (int)(seg < ((int64_t)1 << 30) ? seg : ((int64_t)1 << 30));
  f.in = o; o += ((int64_t)rows * (src_chw ? C : 1) * seg + 15) & ~(int64_t)15;
  f.tmp = o; o += ((int64_t)C * rows * RS_TW + 15) & ~(int64_t)15;
  f.total = o;
  return f;
}

__global__ __launch_bounds__(256) void resample_fused_kernel(const sslcr_resample_desc a, const int rows_cap, const int cols_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const FusedCarve f = fused_carve(a.C, a.src_chw, a.ksx, a.ksy, rows_cap, cols_cap);
  int32_t* s_kx = reinterpret_cast<int32_t*>(smem + f.kx);
  int32_t* s_bx = reinterpret_cast<int32_t*>(smem + f.bx);
  int32_t* s_ky = reinterpret_cast<int32_t*>(smem + f.ky);
  int32_t* s_by = reinterpret_cast<int32_t*>(smem + f.by);
  uint32_t* s_in = reinterpret_cast<uint32_t*>(smem + f.in);
  const unsigned char* s_inb = smem + f.in;
  uint32_t* s_tmp = reinterpret_cast<uint32_t*>(smem + f.tmp);
  const int tid = threadIdx.x;
  const int ntx = (a.OW + RS_TW - 1) / RS_TW, nty = (a.OH + RS_TH - 1) / RS_TH;
  int blk = blockIdx.x;
  const int x0 = (blk % ntx) * RS_TW;
  blk /= ntx;
  const int y0 = (blk % nty) * RS_TH;
  const int64_t n = blk / nty;
  const int nx = min(RS_TW, a.OW - x0), ny = min(RS_TH, a.OH - y0);
  const int ti = table_of(a.table_index, a.T, n);
  {
    const int32_t* gkx = a.kx + ((int64_t)ti * a.OW + x0) * a.ksx;
    const int32_t* gbx = a.bx + ((int64_t)ti * a.OW + x0) * 2;
    const int32_t* gky = a.ky + ((int64_t)ti * a.OH + y0) * a.ksy;
    const int32_t* gby = a.by + ((int64_t)ti * a.OH + y0) * 2;
    for (int i = tid; i < nx * a.ksx; i += 256) s_kx[i] = gkx[i];
    for (int i = tid; i < nx * 2; i += 256) s_bx[i] = gbx[i];
    for (int i = tid; i < ny * a.ksy; i += 256) s_ky[i] = gky[i];
    for (int i = tid; i < ny * 2; i += 256) s_by[i] = gby[i];
  }
  __syncthreads();
  // the source window of the tile: both bounds grow with the output index, so the first entry's start and the last one's end
  const int r0 = clampi(s_by[0], 0, a.IH);
  const int r1 = clampi(s_by[2 * (ny - 1)], 0, a.IH) + clampi(s_by[2 * (ny - 1) + 1], 0, a.ksy);
  const int rows = clampi(r1 - r0, 0, min(rows_cap, a.IH - r0));
  const int c0 = clampi(s_bx[0], 0, a.IW);
  const int c1 = clampi(s_bx[2 * (nx - 1)], 0, a.IW) + clampi(s_bx[2 * (nx - 1) + 1], 0, a.ksx);
  const int cols = clampi(c1 - c0, 0, min(cols_cap, a.IW - c0));
  const Lay s = lay_of(a.src_chw, a.C, a.IH, a.IW);
  const uint8_t* simg = a.src + n * s.img + (int64_t)r0 * s.row + (int64_t)c0 * s.ps;
  const int per = a.src_chw ? a.C : 1;                 // staged segments per source row
  const int seg_len = a.src_chw ? cols : cols * a.C;
  const int sd = f.seg_stride / 4;
  for (int i = tid; i < rows * per * sd; i += 256) {
    const int seg = i / sd, j = i % sd;
    const uint8_t* g = simg + (int64_t)(seg / per) * s.row + (a.src_chw ? (seg % per) * s.cs : 0);
    const int m = (int)(reinterpret_cast<uintptr_t>(g) & 3);
    if (4 * j < m + seg_len) s_in[i] = *reinterpret_cast<const uint32_t*>(g - m + 4 * j);
  }
  __syncthreads();
  constexpr int qn = RS_TW / 4;
  // horizontal: staged bytes -> planar rounded bytes, tmp[c][row][RS_TW]
  for (int i = tid; i < rows * a.C * qn; i += 256) {
    const int q = i % qn, rc = i / qn;
    const int c = rc % a.C, r = rc / a.C;
    if (4 * q >= nx) continue;
    const int seg = a.src_chw ? r * a.C + c : r;
    const uint8_t* g = simg + (int64_t)r * s.row + (a.src_chw ? c * s.cs : 0);
    const unsigned char* base = s_inb + (int64_t)seg * f.seg_stride + (reinterpret_cast<uintptr_t>(g) & 3) + (a.src_chw ? 0 : c);
    uint32_t d = 0;
    for (int e = 0; e < 4; ++e) {
      const int xx = 4 * q + e;
      if (xx >= nx) break;
      const int xmin = clampi(s_bx[2 * xx], 0, a.IW);
      const int lo = max(xmin, c0), hi = min(xmin + clampi(s_bx[2 * xx + 1], 0, a.ksx), c0 + cols);
      const int32_t* kk = s_kx + xx * a.ksx - xmin;
      int acc = RS_HALF;
      for (int t = lo; t < hi; ++t) acc += __mul24((int)base[(t - c0) * s.ps], kk[t]);
      d |= clip8(acc) << (8 * e);
    }
    s_tmp[(c * rows_cap + r) * qn + q] = d;
  }
  __syncthreads();
  // vertical: one dword of four pixels per tap; the coefficient is uniform over the 16 lanes of a row
  uint8_t* dimg = a.dst + n * ((int64_t)a.C * a.OH * a.OW);
  for (int i = tid; i < ny * qn; i += 256) {
    const int q = i % qn, yy = i / qn;
    if (4 * q >= nx) continue;
    const int ymin = clampi(s_by[2 * yy], 0, a.IH);
    const int lo = max(ymin, r0), hi = min(ymin + clampi(s_by[2 * yy + 1], 0, a.ksy), r0 + rows);
    const int32_t* kk = s_ky + yy * a.ksy - ymin;
    uint32_t v[3] = {0, 0, 0};
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      if (c >= a.C) break;
      int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
      const uint32_t* col = s_tmp + (c * rows_cap - r0) * qn + q;
      for (int t = lo; t < hi; ++t) {
        const uint32_t d = col[t * qn];
        const int w = kk[t];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += __mul24((int)byte_of(d, e), w);
      }
      v[c] = clip8(acc[0]) | clip8(acc[1]) << 8 | clip8(acc[2]) << 16 | clip8(acc[3]) << 24;
    }
    store_quad(dimg, a.dst_chw, a.C, a.OH, a.OW, y0 + yy, x0 + 4 * q, v);
  }
}

// the widest source range [b[first].min, b[last].end) over the aligned groups of `tile` outputs, all T sets (host tables)
int64_t widest_window(const int32_t* b, int T, int on, int tile) {
  int64_t w = 0;
  for (int t = 0; t < T; ++t) {
    const int32_t* bt = b + (int64_t)t * on * 2;
    for (int o0 = 0; o0 < on; o0 += tile) {
      const int o1 = (o0 + tile < on ? o0 + tile : on) - 1;
      const int64_t span = (int64_t)bt[2 * o1] + bt[2 * o1 + 1] - bt[2 * o0];
      if (span > w) w = span;
    }
  }
  return w;
}

int pass_blocks(int64_t quads) {
  const int64_t b = (quads + 255) / 256;
  return (int)(b < 65536 ? b : 65536);
}

}  // namespace

const char* resample_plan(const sslcr_resample_desc& a, ResamplePlan* out) {
  if (!(a.N >= 0)) return "N < 0";
  if (!(a.C == 1 || a.C == 3)) return "C outside {1, 3}";
  if (!(a.IH >= 1 && a.IW >= 1 && a.OH >= 1 && a.OW >= 1)) return "empty image";
  if ((int64_t)a.C * a.IH * a.IW >= (int64_t)1 << 31 || (int64_t)a.C * a.OH * a.OW >= (int64_t)1 << 31 ||
      (int64_t)a.C * a.IH * a.OW >= (int64_t)1 << 31) return "an image of 2^31 bytes or more";
  if (!(a.T >= 1)) return "T < 1";
  if ((a.kx == nullptr) != (a.bx == nullptr) && !a.nearest) return "kx without bx (or bx without kx)";
  if ((a.ky == nullptr) != (a.by == nullptr) && !a.nearest) return "ky without by (or by without ky)";
  if (!(a.form >= 0 && a.form <= 2)) return "form outside {0, 1, 2}";
  const bool h = a.bx != nullptr, v = a.by != nullptr;
  if (!h && a.OW != a.IW) return "no horizontal table and OW != IW";
  if (!v && a.OH != a.IH) return "no vertical table and OH != IH";
  if (!a.nearest && ((h && a.ksx < 1) || (v && a.ksy < 1))) return "ksize < 1";
  if (a.T > 1 && !a.table_index) return "T > 1 without table_index";
  memset(out, 0, sizeof(*out));
  const int qw = (a.OW + 3) / 4;
  const int64_t quads = (int64_t)a.N * a.OH * qw;
  if (a.nearest || h != v || !h) {
    if (a.form != 0) return "form 1 / 2 (fused / two-pass) is for a descriptor that needs both passes";
    out->form = a.nearest || (!h && !v) ? SSLCR_RESAMPLE_GATHER : h ? SSLCR_RESAMPLE_HORIZONTAL : SSLCR_RESAMPLE_VERTICAL;
    out->grid[0] = pass_blocks(quads);
    return nullptr;
  }
  const int64_t tiles = (int64_t)((a.OW + RS_TW - 1) / RS_TW) * ((a.OH + RS_TH - 1) / RS_TH) * a.N;
  int64_t rows = 0, cols = 0, lds = 0;
  if (a.bx_host && a.by_host) {
    rows = widest_window(a.by_host, a.T, a.OH, RS_TH);
    cols = widest_window(a.bx_host, a.T, a.OW, RS_TW);
    if (rows < 0 || cols < 0 || rows > a.IH || cols > a.IW) return "bx_host / by_host are not the tables of this image size";
    lds = fused_carve(a.C, a.src_chw, a.ksx, a.ksy, (int)rows, (int)cols).total;
    out->fused_ok = lds <= SSLCR_RESAMPLE_LDS_CAP && tiles < (int64_t)1 << 31;
  }
  if (a.form == 1 && !out->fused_ok) return "form = 1 (fused): the tile does not fit SSLCR_RESAMPLE_LDS_CAP (or bx_host / by_host are missing)";
  if (out->fused_ok && a.form != 2) {
    out->form = SSLCR_RESAMPLE_FUSED;
    out->tile_w = RS_TW; out->tile_h = RS_TH;
    out->rows = (int)rows; out->cols = (int)cols;
    out->lds_bytes = (size_t)lds;
    out->grid[0] = (int)tiles;
  } else {
    out->form = SSLCR_RESAMPLE_TWO_PASS;
    out->workspace_bytes = (size_t)a.N * a.C * a.IH * a.OW;
    out->grid[0] = pass_blocks((int64_t)a.N * a.IH * qw);
    out->grid[1] = pass_blocks(quads);
  }
  return nullptr;
}

hipError_t launch_resample(const sslcr_resample_desc& a, const ResamplePlan& p, hipStream_t st) {
  if (a.N == 0) return hipSuccess;
  const Lay s = lay_of(a.src_chw, a.C, a.IH, a.IW);
  switch (p.form) {
    case SSLCR_RESAMPLE_GATHER:
      hipLaunchKernelGGL(resample_gather_kernel, dim3(p.grid[0]), dim3(256), 0, st, a);
      break;
    case SSLCR_RESAMPLE_FUSED:
      return launch_lds<resample_fused_kernel>(dim3(p.grid[0]), dim3(256), p.lds_bytes, SSLCR_RESAMPLE_LDS_CAP, st, a, p.rows, p.cols);
    case SSLCR_RESAMPLE_HORIZONTAL:
      hipLaunchKernelGGL(resample_pass_kernel<0>, dim3(p.grid[0]), dim3(256), 0, st, a.src, s, a.dst, a.dst_chw, a.kx, a.bx, a.table_index,
                         a.T, a.ksx, a.N, a.C, a.IH, a.IW, a.OH, a.OW);
      break;
    case SSLCR_RESAMPLE_VERTICAL:
      hipLaunchKernelGGL(resample_pass_kernel<1>, dim3(p.grid[0]), dim3(256), 0, st, a.src, s, a.dst, a.dst_chw, a.ky, a.by, a.table_index,
                         a.T, a.ksy, a.N, a.C, a.IH, a.IW, a.OH, a.OW);
      break;
    case SSLCR_RESAMPLE_TWO_PASS: {
      if (!a.workspace) return hipErrorInvalidValue;
      hipLaunchKernelGGL(resample_pass_kernel<0>, dim3(p.grid[0]), dim3(256), 0, st, a.src, s, a.workspace, 1, a.kx, a.bx, a.table_index,
                         a.T, a.ksx, a.N, a.C, a.IH, a.IW, a.IH, a.OW);
      hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
      hipLaunchKernelGGL(resample_pass_kernel<1>, dim3(p.grid[1]), dim3(256), 0, st, a.workspace, lay_of(1, a.C, a.IH, a.OW), a.dst, a.dst_chw,
                         a.ky, a.by, a.table_index, a.T, a.ksy, a.N, a.C, a.IH, a.OW, a.OH, a.OW);
      break;
    }
    default:
      return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace sslcr
