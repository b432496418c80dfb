// Which kernel serves a convolution or weight-gradient descriptor: decided here, once.  launch_conv / launch_wgrad switch on the plan;
// the reported kernel name, the statistics-row count and the segment check (kernels.hpp, capi.cpp, engine.cpp) are fields of the same
// plan.  The families keep their own predicates (what a kernel can serve) and their own choice of template instance (*_pick in their
// files); the ORDER in which they are asked, and the rule that a family serves a dtype only where it tiles the descriptor as it does
// in bf16, live nowhere else.
#include "kernels.hpp"

namespace sslcr {

// Segments (sslcr_conv_desc.seg_images): which kernels have the form, and where the row ranges come out right.
//   conv3x3_h16 / conv3x3_pp64: the grid is split into nseg groups of workgroups (their statistics rows are per workgroup; with mask_x:
//                    mask_scale / mask_shift / mask_mean + s * seg_stride)
//   conv3x3_halo256: one workgroup per tile, rows in tile order; a tile's images must not straddle a segment
//   conv_s2:         rows in tile order, a tile lies in one image
//   conv_dma:        rows in pixel order, no prologue; a pixel block must not straddle a segment
ConvPlan conv_plan(int dtype, const ConvArgs& a) {
  // sslcr_conv2d_partial_rows has no dtype: a tiled family serves a descriptor only where its fp32 and bf16 launches tile identically
  auto both = [&](int (*tiling)(int, const ConvArgs&)) {
    const int t = tiling(dtype, a);
    return t == tiling(DT_BF16, a) ? t : 0;
  };
  const bool segs = a.seg_images > 0;
  const bool seg_common = segs && dtype == DT_BF16 && a.N % a.seg_images == 0 && !a.transposed && !a.par4 && a.N / a.seg_images <= 8;
  bool seg_form = false;                                           // the route has a segment form for this descriptor
  bool ok = !(a.out_scale && (!a.bias || a.stats || a.mask_x));    // the output scale exists in the bias (eval) epilogues only
  ConvPlan p{};
  const int q = both(conv_halo256_mode);
  if (const int mode = conv_h16_mode(a, q)) {
    const bool pp = conv_pp64_ok(dtype, a);                        // the ping-pong form of the 64 -> 64 shape
    p.route = pp ? ConvRoute::PP64 : ConvRoute::H16;
    p.param = mode;
    // (the grids divide the CUs among the segments: asked for only where there is at least one)
    p.rows = segs && a.N < a.seg_images ? -1 : (pp ? conv_pp64_rows(a) : conv_h16_rows(a));
    p.name = pp ? conv_pp64_name(a) : conv_h16_name(dtype, a, mode);
    seg_form = true;
  } else if (q) {
    p.route = ConvRoute::HALO256;
    p.param = q;
    p.rows = conv_halo256_tiles(a, q) * 4;
    p.name = conv_halo256_name(dtype, a, q);
    seg_form = q == 16 || a.seg_images % 4 == 0;
  } else if (const int tw = both(conv_halo_tw)) {
    p.route = ConvRoute::HALO;
    p.param = tw;
    p.rows = conv_halo_tiles(a, tw) * 2;
    p.name = conv_halo_name(dtype, a, tw);
  } else if (conv_s2_ok(dtype, a)) {                               // 3x3 / 2 on 16x16 output tiles
    p.route = ConvRoute::S2;
    p.rows = conv_s2_rows(a);
    p.name = conv_s2_name(a, false);
    seg_form = true;
  } else if (conv_s2d_ok(dtype, a)) {                              // ... and its dgrad, the four parity classes in one pass
    p.route = ConvRoute::S2D;
    const int bp = both(conv_dma_bp);
    p.rows = bp ? conv_dma_rows(a, bp) : conv_igemm_rows(a);      // (writes none: the count the public call has always answered here)
    p.name = conv_s2d_name();
    p.par4_one_launch = bp != 0;
  } else if (const int bp = both(conv_dma_bp)) {
    p.route = ConvRoute::DMA;
    p.param = bp;
    p.rows = conv_dma_rows(a, bp);
    p.name = conv_dma_name(dtype, bp);
    p.par4_one_launch = a.par4 != 0;
    seg_form = !a.in_scale && ((long)a.seg_images * a.PH * a.PW) % bp == 0;
  } else {
    p.route = ConvRoute::IGEMM;
    p.rows = conv_igemm_rows(a);
    p.name = conv_igemm_name(dtype, a);
    if (a.par4) ok = false;               // the one-launch parity form exists in the DMA-gather kernels only
  }
  if (a.mask_x && p.route != ConvRoute::H16 && p.route != ConvRoute::PP64) ok = seg_form = false;      // the BatchNorm-backward front end: 16x16-tile kernels only
  p.seg_ok = !segs || (seg_common && seg_form);
  p.ok = ok && p.seg_ok;
  return p;
}

hipError_t launch_conv(int dtype, const ConvArgs& a, const ConvPlan& p, hipStream_t st) {
  if (!p.ok) return hipErrorInvalidValue;
  switch (p.route) {
    case ConvRoute::H16: return launch_conv_h16(dtype, a, p.param, st);
    case ConvRoute::PP64: return launch_conv_pp64(a, st);
    case ConvRoute::HALO256: return launch_conv_halo256(dtype, a, p.param, st);
    case ConvRoute::HALO: return launch_conv_halo(dtype, a, p.param, st);
    case ConvRoute::S2: return launch_conv_s2(a, nullptr, st);
    case ConvRoute::S2D: return launch_conv_s2d(a, st);
    case ConvRoute::DMA: return launch_conv_dma(dtype, a, p.param, st);
    case ConvRoute::IGEMM: return launch_igemm(dtype, a, st);
  }
  return hipErrorInvalidValue;
}

WgradPlan wgrad_plan(int dtype, const WgradArgs& a) {
  if (const int tw = wgrad_halo_tw(a)) {
    const int kh = dtype == DT_BF16 && a.K % 128 == 0 ? 2 : 1;     // the 128-kout block, 8-wave form
    if (kh == 2 && wgrad_dma_ok(dtype, a, wgrad_halo_splits(a, tw, 2))) return {WgradRoute::HALO_DMA, tw, 2, true, wgrad_dma_name(a, tw)};
    return {WgradRoute::HALO, tw, kh, true, wgrad_halo_name(dtype, tw, kh)};
  }
  // 3x3 / 2 on 4x16-tileable output maps: parity-plane halo form (whole-batch prologue, like the generic kernel: wgrad_s2_ok)
  if (wgrad_s2_ok(dtype, a)) return {WgradRoute::S2, 0, 0, true, wgrad_s2_name(a)};
  const bool segs = a.seg_images > 0 && a.seg_images < a.N;        // per-segment prologue: halo kernels only
  return {WgradRoute::GENERIC, 0, 0, !segs, wgrad_generic_name(dtype, a)};
}

hipError_t launch_wgrad(int dtype, const WgradArgs& a, const WgradPlan& p, hipStream_t st) {
  if (!p.ok) return hipErrorInvalidValue;
  switch (p.route) {
    case WgradRoute::HALO:
    case WgradRoute::HALO_DMA: return launch_wgrad_halo(dtype, a, p, st);
    case WgradRoute::S2: return launch_wgrad_s2(a, st);
    case WgradRoute::GENERIC: return launch_wgrad_generic(dtype, a, st);
  }
  return hipErrorInvalidValue;
}

}  // namespace sslcr
