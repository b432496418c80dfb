// 3x3 / stride 1 / pad 1 NHWC convolution on 256-pixel tiles -- a 16x16 patch of one image, or (TW = 8) four whole 8x8 images:
// persistent, DMA-fed form of the LDS-halo kernel (ResNet18 layer1-4 block convs forward and their dgrads through tap-flipped
// packs; conv_halo256.hip is the fallback for the shapes this one does not take).
//
// What the previous form lost, measured by ablation on the layer2 shape (N=640, 32x32, 128->128: 220 us, MFMA-only ~95 us):
// removing the MFMAs left 137 us, the halo loads 47 us, the weight loads 50 us, the epilogue 52 us, the barriers 31 us --
// i.e. the parts ran back to back instead of under each other.  The ISA showed why: (1) the compiler sank every weight
// prefetch down to its LDS store, so each tap waited a full L2 round trip; (2) s_waitcnt vmcnt counts IN ORDER, so the first
// wait on a (young, short) weight load also waited for the (older, long) HBM halo loads and for the epilogue stores of the
// previous tile; (3) ~55 VGPRs held per-tap LDS addresses, leaving no room to double-buffer fragments, so the wave ran
// ds_read -> wait -> 4 MFMA -> ds_read ...
//
// This kernel is built around those three facts:
//   * weights go global -> LDS by DMA (buffer_load_dwordx4 ... lds -- LdsDma, common.hpp; no registers, no ds_write; issued by the
//     younger wave of each SIMD's pair): a whole ring half (3 taps) is
//     issued right after the barrier that frees it and waited for once, just before the barrier that publishes it, three
//     taps later.  The lane picks its SOURCE chunk so that the linear DMA placement is the swizzled, fragment-ordered tile.
//   * the halo of the next stage is requested after the first weight wait of a stage, so the only vmcnt waits in the
//     stream are >= 3 taps (~3000 clk) behind every load and store they cover; BatchNorm+ReLU of the producer is applied to
//     the halo IN REGISTERS under the MFMAs of the last three taps, and only six ds_write_b128 sit between the two barriers
//     of a stage boundary.
//   * the halo rows are pitched 24 pixels (18 used) so that the XOR swizzle key (pixel & 7) depends on the lane and the
//     filter column only: all nine taps, four pixel groups and TK weight tiles are immediate offsets on 6 + 2 address
//     registers, and fragments are double-buffered in the registers this frees.
//   * persistent workgroups (one per CU) walk items (tile, kout block) b, b+G, ...: the epilogue's stores drain under the
//     next item's taps and the next item's first halo is already in LDS when the last tap retires.
#include "kernels.hpp"

namespace sslcr {

// inverse of wperm<TK> (common.hpp): LDS row -> kout row of the block
template <int TK>
__device__ __forceinline__ int wperm_inv(int rr) {
  constexpr int B = 16 * TK;
  const int blk = rr / B, x = rr - blk * B;
  const int t = x >> 4, q = (x >> 2) & 3, j = x & 3;
  return blk * B + q * (4 * TK) + t * 4 + j;
}

#define SSLCR_WAIT_VM0() __builtin_amdgcn_s_waitcnt(0x0f70) /* vmcnt(0), lgkmcnt/expcnt untouched */

// phase timing for tools/microbench/h16_phase_bench.hip (-DSSLCR_H16_PROF; compiled out otherwise): per wave of workgroup 0, shader
// cycles of a stage spent waiting for the weight DMA, at the publish (P) and free (F) barriers, in the stage-end halo swap and in
// the item epilogue
#ifdef SSLCR_H16_PROF
__device__ unsigned long long g_h16_prof[16][8];
#define H16_T(v) const unsigned long long v = __builtin_readcyclecounter()
#define H16_ACC(i, d) h16_t[i] += (d)
#else
#define H16_T(v)
#define H16_ACC(i, d)
#endif

// XF: the producer's BatchNorm(+ReLU) is applied to the input on its way into LDS (a.in_scale != nullptr)
// WR: the whole filter bank stays resident in LDS (C == one slab and K == BKO, i.e. the 64->64 layer1 convs: 9 x 64 x 128 B
//     = 72 KB next to the 54 KB halo).  A stage then has no weight DMA, no publish/free barriers and no vmcnt wait before its
//     15th step, so the next halo (and the residual) is requested at the TOP of the stage and has ~14 steps to land; with
//     the ring, the short 8-MFMA steps of this shape left the HBM round trip of the halo half exposed and paid 8 barriers
//     per 144 MFMAs.
// RAW: the output stage of the train-mode forward -- no bias, no residual, no ReLU, no mask, statistics wanted (checked by the
//     launcher): pack + store + the BatchNorm partial sums, as an instance of its own.  An output-stage instruction costs ~4 cycles
//     (no MFMA runs beside it), so the 64 bias adds and 64 clamps of the general body are worth an instance; as run-time cases
//     INSIDE one instance the duplicated bodies spilled (round 3).
// TW = 8 (round 4): the tile is FOUR WHOLE 8x8 IMAGES (ResNet18 layer4 at 256x256 input) instead of a 16x16 patch of one -- the same
//     256 pixels x BKO kouts, wave wp owns image wp, a fragment's 16 lanes are two image rows.  Every halo-ring pixel is padding, so
//     the ring is zeroed once and a stage stages the 256 interior pixels only (4 loads per thread, no edge logic); halo rows are
//     pitched 10 pixels with the swizzle key = halo column & 7 (conflict-free over the lane groups of ds_read_b128, enumerated for
//     conv3x3_halo256's 8-wide form).  row0: first statistics row of this launch (a shape served by two launches, see launch_ht).
// OSC (round 6): sslcr_conv_desc.out_scale -- eval-mode BatchNorm with its scale kept out of the filters, y = epilogue(acc * scale + bias).
//     An instance (and a kernel name, conv3x3_h16s_kernel) of its own: as a run-time case inside the plain instance the sixteen scale
//     values took the dominant instance of the step from 251 registers to 256 + 120 B of scratch (all of its launches, the dgrads too).
//     Its output stage walks 16-byte chunks with the chunk's bias and scale loaded from LDS next to each other -- the same live set as
//     the plain body's bias[16] + v[16].
template <typename T, int BKO, int WK, bool XF, bool WR, bool RAW = false, int TW = 16>
__global__ __launch_bounds__(256 * WK, WK == 1 ? 1 : 2) void conv3x3_h16_kernel(const ConvArgs a, const int tiles_total, const int n_items, const int kshift,
                                                                                const int row0) {
  constexpr bool OSC = false;
#include "conv_h16_body.hpp"
}
// ... with sslcr_conv_desc.out_scale (no input transform, no statistics: the eval forms)
template <typename T, int BKO, int WK, bool WR, int TW>
__global__ __launch_bounds__(256 * WK, WK == 1 ? 1 : 2) void conv3x3_h16s_kernel(const ConvArgs a, const int tiles_total, const int n_items, const int kshift,
                                                                                 const int row0) {
  constexpr bool OSC = true, XF = false, RAW = false;
#include "conv_h16_body.hpp"
}

// bf16 64 -> 64: one 128-byte slab of input channels and one kout block, the filter bank fits LDS whole
static bool h16_resident(const ConvArgs& a) { return a.C == 64 && a.K == 64; }
// dynamic LDS of an instance: the halo of the tile form, `filter_stages` x 3 taps of a kout block (ring: 2, resident bank: 3), the
// input transform's 2 C floats, 8 floats per kout of the block, and k_arrays K-float arrays (bias; + output scale; mask_x: 3)
static size_t h16_lds_bytes(int tile, int bko, int filter_stages, int C, int K, int k_arrays) {
  return (size_t)(tile == 16 ? 18 * 24 : 4 * 10 * 10) * 128 + (size_t)filter_stages * 3 * bko * 128 + 2 * (size_t)C * sizeof(float) +
         8 * (size_t)bko * sizeof(float) + (size_t)k_arrays * K * sizeof(float);
}
constexpr size_t H16_LDS_CAP = 160 * 1024;

// 16: 16x16 tiles of one image; 8: four whole 8x8 images per tile (128-kout blocks: ResNet18 layer4 at 256x256 input); 0: not served.
// q: the conv3x3_halo256 tiling of the descriptor that both dtypes agree on (conv_plan: the launches must tile identically)
int conv_h16_mode(const ConvArgs& a, int q) {
  const bool on8 = sw::on(sw::H16_TW8);                // (the switch: A/B runs against conv3x3_halo256)
  const int mode = q == 16 ? 16 : (q == 8 && on8 && a.K % 128 == 0 && !a.mask_x && (a.seg_images <= 0 || a.seg_images % 4 == 0)) ? 8 : 0;
  if (mode == 0) return 0;
  if (a.in_scale && a.residual) return 0;              // not a ResNet combination; the older halo kernels take it
  // The LDS checks below have no dtype to go by: a 64 -> 64 descriptor is counted with the resident bank's three filter stages, which
  // launch_h uses in bf16 only (fp32 keeps the ring's two).  Either count fits, so the answer is the launcher's for both.
  const int bko = a.K % 128 == 0 ? 128 : 64, stages = h16_resident(a) ? 3 : 2;
  if (a.mask_x) {
    // (a.stats is checked at launch: sslcr_conv2d_partial_rows asks before the rows buffer exists)
    if (!a.mask_scale || !a.mask_shift || !a.mask_mean || a.in_scale || a.bias || a.residual || a.relu || a.out_scale) return 0;
    // (mask_x: 16x16 tiles only.)  This predicate has always counted the 8 floats per kout for a 128-kout block whatever the block:
    // 2 KiB more than launch_h asks for a 64-kout one.  Kept, so that no descriptor changes its route.
    if (h16_lds_bytes(16, bko, stages, a.C, a.K, 3) + 8 * (128 - bko) * sizeof(float) > H16_LDS_CAP) return 0;
  }
  if (a.out_scale) {
    // one more K-float array in LDS (the input-transform and train-forward instances have no output scale: bias forms only)
    if (a.in_scale || a.stats || !a.bias) return 0;
    if (h16_lds_bytes(mode, bko, stages, a.C, a.K, 2) > H16_LDS_CAP) return 0;
  }
  return mode;
}
// The launch's geometry for kout blocks of bko, read by the row count and the launcher alike: segments, tiles and (tile, kout block)
// items per segment, and workgroups -- one per CU, or per item where there are fewer; with segments, nseg equal groups.
// Partial-statistics rows the launch will write: four per workgroup (see s_stat)
struct H16Geom { int nseg, tiles, n_items, grid; };
static H16Geom h16_geom(const ConvArgs& a, int bko) {
  const int nseg = a.seg_images > 0 ? a.N / a.seg_images : 1;
  const int tiles = a.H == 8 ? (a.N / nseg) / 4 : (a.N / nseg) * (a.H / 16) * (a.W / 16);
  const int n_items = tiles * (a.K / bko), per = device_cus() / nseg;
  return {nseg, tiles, n_items, (n_items < per ? n_items : per) * nseg};
}
static int h16_grid(const ConvArgs& a, int bko) { return h16_geom(a, bko).grid; }
// Four-image tiles (layer4): with one workgroup per CU walking (tile, 128-kout block) items, a last round that would occupy at most
// half the CUs (N = 640: 640 items = 2.5 rounds of 256) runs its tiles as 64-kout items on all of them instead, in a second launch
// over the tail images (the split conv3x3_halo256 makes for this shape).  -> tiles of the tail launch (0: one launch)
static int h16_tail8(const ConvArgs& a) {
  if (a.H != 8 || a.seg_images > 0) return 0;
  const int cus = device_cus(), tiles = a.N / 4, kb = a.K / 128, rem = (tiles * kb) % cus;
  if (rem == 0 || 2 * rem > cus || rem % kb != 0 || tiles <= rem / kb) return 0;
  return rem / kb;
}
static ConvArgs h16_head8(const ConvArgs& a, int tail) { ConvArgs h = a; h.N = a.N - 4 * tail; return h; }
static ConvArgs h16_tailargs8(const ConvArgs& a, int tail, int dtype) {
  ConvArgs t = a;
  const int n0 = a.N - 4 * tail;
  const size_t es = dtype == DT_BF16 ? 2 : 4, px = (size_t)n0 * a.H * a.W;
  t.N = 4 * tail;
  t.x = reinterpret_cast<const char*>(a.x) + px * a.C * es;
  t.y = reinterpret_cast<char*>(a.y) + px * a.K * es;
  if (a.residual) t.residual = reinterpret_cast<const char*>(a.residual) + px * a.K * es;
  return t;
}
int conv_h16_rows(const ConvArgs& a) {
  const int tail = h16_tail8(a);
  if (tail) return (h16_grid(h16_head8(a, tail), 128) + h16_grid(h16_tailargs8(a, tail, DT_BF16), 64)) * 4;
  return h16_grid(a, a.K % 128 == 0 ? 128 : 64) * 4;
}

// the train-mode forward's output stage (the RAW instance); SSLCR_H16_RAW=0 keeps the general body for same-box A/B runs
static bool h16_raw(const ConvArgs& a) {
  return sw::on(sw::H16_RAW) && a.stats && !a.bias && !a.relu && !a.residual && !a.mask_x;
}

// one tag per template instance of the two kernels (OSC: conv3x3_h16s_kernel<T, BKO, WK, WR, TW>)
template <typename T, int BKO, int WK, bool XF, bool WR, bool RAW, int TW, bool OSC>
struct H16Inst {
  static std::string spell() {
    return OSC ? kname("conv3x3_h16s_kernel", ktype<T>(), BKO, WK, WR, TW) : kname("conv3x3_h16_kernel", ktype<T>(), BKO, WK, XF, WR, RAW, TW);
  }
};

template <typename T, int BKO, int WK, bool XF, bool WR, bool RAW, int TW, bool OSC>
static hipError_t launch_h(H16Inst<T, BKO, WK, XF, WR, RAW, TW, OSC>, const ConvArgs& a, hipStream_t st, int row0) {
  static_assert(!OSC || (!XF && !RAW), "output scale: eval forms only");
  if (OSC != (a.out_scale != nullptr)) return hipErrorInvalidValue;
  const size_t lds = h16_lds_bytes(TW, BKO, WR ? 3 : 2, a.C, a.K, a.mask_x ? 3 : (a.out_scale ? 2 : 1));
  const H16Geom g = h16_geom(a, BKO);                                   // one 8-wave workgroup per CU
  const int kbn = a.K / BKO, gseg = g.grid / g.nseg;
  const int kshift = (kbn > 1 && (kbn & (kbn - 1)) == 0 && (gseg & (kbn - 1)) == 0) ? __builtin_ctz(kbn) : -1;
  const dim3 grid(g.grid), block(256 * WK);
  if constexpr (OSC) return launch_lds<conv3x3_h16s_kernel<T, BKO, WK, WR, TW>>(grid, block, lds, H16_LDS_CAP, st, a, g.tiles, g.n_items, kshift, row0);
  else return launch_lds<conv3x3_h16_kernel<T, BKO, WK, XF, WR, RAW, TW>>(grid, block, lds, H16_LDS_CAP, st, a, g.tiles, g.n_items, kshift, row0);
}

// The instance of one (kout block, tile, filter residency) form that a's operands select: f(H16Inst<...>{}).  The RAW output stage
// exists in the bf16 128-kout forms.
template <typename T, int BKO, int TW, bool WR, class F>
static auto h16_pick_form(const ConvArgs& a, F&& f) {
  const bool xf = a.in_scale != nullptr;
  if (a.out_scale) return f(H16Inst<T, BKO, 2, false, WR, false, TW, true>{});
  if constexpr (sizeof(T) == 2 && BKO == 128)
    if (h16_raw(a)) return xf ? f(H16Inst<T, BKO, 2, true, WR, true, TW, false>{}) : f(H16Inst<T, BKO, 2, false, WR, true, TW, false>{});
  return xf ? f(H16Inst<T, BKO, 2, true, WR, false, TW, false>{}) : f(H16Inst<T, BKO, 2, false, WR, false, TW, false>{});
}
// ... and the form: the launch's instance -- of a four-image shape's two launches (launch_ht) the first, 128-kout one
template <typename T, class F>
static auto h16_pick(const ConvArgs& a, int mode, F&& f) {
  if (mode == 8) return h16_pick_form<T, 128, 8, false>(a, f);         // (K % 128 == 0: conv_h16_mode)
  if (a.K % 128 == 0) return h16_pick_form<T, 128, 16, false>(a, f);
  if constexpr (sizeof(T) == 2)
    if (h16_resident(a)) return h16_pick_form<T, 64, 16, true>(a, f);
  return h16_pick_form<T, 64, 16, false>(a, f);
}

template <typename T>
static hipError_t launch_ht(const ConvArgs& a, int mode, hipStream_t st) {
  const int tail = h16_tail8(a);
  if (!tail) return h16_pick<T>(a, mode, [&](auto inst) { return launch_h(inst, a, st, 0); });
  // four-image tiles with a thin last round: the head's items in 128-kout blocks, the tail images' in 64-kout blocks
  const ConvArgs head = h16_head8(a, tail), tl = h16_tailargs8(a, tail, Elem<T>::DT);
  hipError_t e = h16_pick<T>(head, mode, [&](auto inst) { return launch_h(inst, head, st, 0); });
  if (e != hipSuccess) return e;
  const int row0 = h16_grid(head, 128) * 4;                             // the tail's statistics rows follow the head's
  return h16_pick_form<T, 64, 8, false>(tl, [&](auto inst) { return launch_h(inst, tl, st, row0); });
}

hipError_t launch_conv_h16(int dtype, const ConvArgs& a, int mode, hipStream_t st) {
  if (a.mask_x && !a.stats) return hipErrorInvalidValue;
  return dtype == DT_BF16 ? launch_ht<bf16_t>(a, mode, st) : launch_ht<float>(a, mode, st);
}

const char* conv_h16_name(int dtype, const ConvArgs& a, int mode) {
  return dtype == DT_BF16 ? h16_pick<bf16_t>(a, mode, InstName{}) : h16_pick<float>(a, mode, InstName{});
}

}  // namespace sslcr
