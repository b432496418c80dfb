// Internal kernel launch interface of the engine (host side).  The argument structs ARE the C-ABI
// descriptors of include/sslcr.h.  Every launcher is asynchronous on `st`; no allocation, no sync.
#pragma once
#include <string>

#include "common.hpp"
#include "launch.hpp"
#include "switches.hpp"
#include "../../include/sslcr.h"

namespace sslcr {

using ConvArgs = sslcr_conv_desc;
using WgradArgs = sslcr_wgrad_desc;
using StemArgs = sslcr_stem_desc;
using StemWgradArgs = sslcr_stem_wgrad_desc;
using BnFinalizeArgs = sslcr_bn_finalize_desc;
using BnActArgs = sslcr_bn_act_desc;
using PoolFwdArgs = sslcr_pool_fwd_desc;
using PoolBwdArgs = sslcr_pool_bwd_desc;
using BnBwdArgs = sslcr_bn_bwd_desc;
using LossArgs = sslcr_loss_desc;
using LossOpts = sslcr_loss_opts;
using TensorDesc = sslcr_tensor_desc;
using OptArgs = sslcr_opt_desc;
using PackArgs = sslcr_pack_desc;
using Fp8Args = sslcr_fp8_desc;
using PackFp8Args = sslcr_pack_fp8_desc;

// ---- kernel names, in the profiler's spelling ("sslcr::conv_dma_kernel<unsigned short, 128, 128>"): every family has one tag type per
// template instance, which spells the name from its template arguments; a family's *_pick() hands the tag of the instance it chooses to
// a callable -- one that launches it, or InstName, which keeps the string in a function-local static per instance -- so that the
// launch and the reported name cannot be two decisions
inline std::string karg(const char* s) { return s; }
inline std::string karg(bool v) { return v ? "true" : "false"; }
inline std::string karg(int v) { return std::to_string(v); }
template <class... A>
std::string kname(const char* kernel, A... args) {
  std::string s = std::string("sslcr::") + kernel;
  const char* sep = "<";
  ((s += sep + karg(args), sep = ", "), ...);
  return sizeof...(A) ? s + ">" : s;
}
template <typename T> constexpr const char* ktype() { return sizeof(T) == 2 ? "unsigned short" : "float"; }
struct InstName {
  template <class I> const char* operator()(I) const {
    static const std::string s = I::spell();
    return s.c_str();
  }
};

// conv_route.cpp: which kernel serves a descriptor, decided ONCE -- the launch, the reported name, the statistics rows and the segment
// check all read this plan (and the engine, where it has to know the route)
enum class ConvRoute { H16, PP64, HALO256, HALO, S2, S2D, DMA, IGEMM };
struct ConvPlan {
  ConvRoute route;      // the family the descriptor maps to (also where !ok: the name has always been answered for those)
  int param;            // H16 / HALO256: tile mode (16 | 8); HALO: tile width; DMA: pixel block; else 0
  int rows;             // partial-statistics rows the launch writes (-1: a grid split among segments, and seg_images > N)
  bool seg_ok;          // the descriptor's seg_images (0 = none) has a form on this route
  bool ok;              // launch_conv() takes it
  bool par4_one_launch; // a par4 descriptor (the stride-2 dgrad's four parity classes at once) that conv_dma serves -- itself, or conv_s2d
                        // in its place; where conv_dma would not, the engine keeps its four per-parity launches, conv_s2d or not
  const char* name;     // the template instance, as the profiler prints it (minus the argument list)
};
ConvPlan conv_plan(int dtype, const ConvArgs& a);
hipError_t launch_conv(int dtype, const ConvArgs& a, const ConvPlan& p, hipStream_t st);
inline hipError_t launch_conv(int dtype, const ConvArgs& a, hipStream_t st) { return launch_conv(dtype, a, conv_plan(dtype, a), st); }
inline const char* conv_kernel_name(int dtype, const ConvArgs& a) { return conv_plan(dtype, a).name; }
inline int conv_partials_rows(const ConvArgs& a) { return conv_plan(DT_BF16, a).rows; }      // (the public call has no dtype)
inline bool conv_segments_ok(int dtype, const ConvArgs& a) { return conv_plan(dtype, a).seg_ok; }
enum class WgradRoute { HALO, HALO_DMA, S2, GENERIC };
struct WgradPlan {
  WgradRoute route;
  int tw, KH;           // HALO / HALO_DMA: tile width and 64-kout halves per workgroup (else 0)
  bool ok;              // launch_wgrad() takes it
  const char* name;
};
WgradPlan wgrad_plan(int dtype, const WgradArgs& a);
hipError_t launch_wgrad(int dtype, const WgradArgs& a, const WgradPlan& p, hipStream_t st);
inline hipError_t launch_wgrad(int dtype, const WgradArgs& a, hipStream_t st) { return launch_wgrad(dtype, a, wgrad_plan(dtype, a), st); }
inline const char* wgrad_kernel_name(int dtype, const WgradArgs& a) { return wgrad_plan(dtype, a).name; }
inline bool wgrad_dma_used(int dtype, const WgradArgs& a) { return wgrad_plan(dtype, a).route == WgradRoute::HALO_DMA; }
// conv_igemm.hip: the generic gather kernel
int conv_igemm_rows(const ConvArgs& a);
hipError_t launch_igemm(int dtype, const ConvArgs& a, hipStream_t st);
const char* conv_igemm_name(int dtype, const ConvArgs& a);
// conv_halo.hip
int conv_halo_tw(int dtype, const ConvArgs& a);
int conv_halo_tiles(const ConvArgs& a, int tw);
hipError_t launch_conv_halo(int dtype, const ConvArgs& a, int tw, hipStream_t st);
const char* conv_halo_name(int dtype, const ConvArgs& a, int tw);
// conv_halo256.hip
int conv_halo256_mode(int dtype, const ConvArgs& a);
int conv_halo256_tiles(const ConvArgs& a, int mode);
hipError_t launch_conv_halo256(int dtype, const ConvArgs& a, int mode, hipStream_t st);
const char* conv_halo256_name(int dtype, const ConvArgs& a, int mode);
// conv_h16.hip (mode: 16 | 8, 0 = not served; q = the conv3x3_halo256 tiling both dtypes agree on)
int conv_h16_mode(const ConvArgs& a, int q);
int conv_h16_rows(const ConvArgs& a);
hipError_t launch_conv_h16(int dtype, const ConvArgs& a, int mode, hipStream_t st);
const char* conv_h16_name(int dtype, const ConvArgs& a, int mode);
// conv_pp64.hip: ping-pong form of the bf16 64 -> 64 resident-filter shape, for the descriptors conv_h16 serves
bool conv_pp64_ok(int dtype, const ConvArgs& a);
hipError_t launch_conv_pp64(const ConvArgs& a, hipStream_t st);
const char* conv_pp64_name(const ConvArgs& a);
int conv_pp64_rows(const ConvArgs& a);
// conv_dma.hip
int conv_dma_bp(int dtype, const ConvArgs& a);
int conv_dma_rows(const ConvArgs& a, int bp);
hipError_t launch_conv_dma(int dtype, const ConvArgs& a, int bp, hipStream_t st);
const char* conv_dma_name(int dtype, int bp);
// conv_s2.hip: 3x3 / 2 on 16x16 output tiles by plane-gathering LDS DMA, optionally with the 1x1 / 2 projection of the same input (bf16)
bool conv_s2_ok(int dtype, const ConvArgs& a);
bool conv_s2_pair_ok(int dtype, const ConvArgs& a, const ConvArgs& d);
int conv_s2_rows(const ConvArgs& a);
hipError_t launch_conv_s2(const ConvArgs& a, const ConvArgs* d, hipStream_t st);
const char* conv_s2_name(const ConvArgs& a, bool pair);
// conv_s2d.hip: the stride-2 3x3 dgrad, all four output-parity classes in one pass over dY (the par4 descriptor; bf16, 16x16-tileable dY)
bool conv_s2d_ok(int dtype, const ConvArgs& a);
hipError_t launch_conv_s2d(const ConvArgs& a, hipStream_t st);
const char* conv_s2d_name();
// conv_fp8.hip
int conv_fp8_mode(const ConvArgs& a);
int conv_fp8_rows(const ConvArgs& a);
const char* conv_fp8_name(const ConvArgs& a);
hipError_t launch_conv_fp8(const ConvArgs& a, const Fp8Args& q, hipStream_t st);
hipError_t launch_pack_fp8(const PackFp8Args& a, hipStream_t st);
hipError_t launch_fp8_scale_update(float* slots, int n, hipStream_t st);
// conv_wgrad.hip: the generic gather form
hipError_t launch_wgrad_generic(int dtype, const WgradArgs& a, hipStream_t st);
const char* wgrad_generic_name(int dtype, const WgradArgs& a);
int wgrad_halo_tw(const WgradArgs& a);
// wgrad_halo.hip (and the fold launches, launch.hpp)
int wgrad_halo_splits(const WgradArgs& a, int tw, int kh);      // pixel splits of the halo launch (the DMA form wants more than one)
hipError_t launch_wgrad_halo(int dtype, const WgradArgs& a, const WgradPlan& p, hipStream_t st);
const char* wgrad_halo_name(int dtype, int tw, int kh);
// wgrad_dma.hip: the halo kernel's 128-kout bf16 instances with the operands staged by LDS DMA (same tiles, slabs and bits)
bool wgrad_dma_ok(int dtype, const WgradArgs& a, int splits);
const char* wgrad_dma_name(const WgradArgs& a, int tw);
hipError_t launch_wgrad_dma(const WgradArgs& a, int tw, int tps, int ntiles, int splits, void* slabs, hipStream_t st);
hipError_t launch_probe_tr16(const uint16_t* in, const int* byte_addr, uint16_t* out, hipStream_t st);
// wgrad_s2.hip: 3x3 / 2 weight gradient with the input region staged once per tile as parity planes (bf16, no producer transform)
bool wgrad_s2_ok(int dtype, const WgradArgs& a);
hipError_t launch_wgrad_s2(const WgradArgs& a, hipStream_t st);
const char* wgrad_s2_name(const WgradArgs& a);
// stem.hip
hipError_t launch_stem(int dtype, const StemArgs& a, hipStream_t st);
int stem_partials_rows(const StemArgs& a);
hipError_t launch_stem_wgrad(int dtype, const StemWgradArgs& a, hipStream_t st);
hipError_t launch_stem_wgrad_pool(int dtype, const StemWgradArgs& a, const sslcr_bn_bwd_desc& b, hipStream_t st);
const char* stem_wgrad_pool_name(int dtype, const StemWgradArgs& a);       // the instance launch_stem_wgrad_pool runs, as rocprofv3 spells it
// stem_pool.hip: eval-mode stem + max-pool in one kernel (bf16)
bool stem_pool_ok(int dtype, const StemArgs& a, int POH, int POW);
hipError_t launch_stem_pool(int dtype, const StemArgs& a, int POH, int POW, hipStream_t st);
// bn_eltwise.hip
hipError_t launch_bn_finalize(const BnFinalizeArgs& a, hipStream_t st);
hipError_t launch_bn_act(int dtype, const BnActArgs& a, hipStream_t st);
hipError_t launch_bn_relu_maxpool(int dtype, const PoolFwdArgs& a, hipStream_t st);
hipError_t launch_maxpool_relu_bwd(int dtype, const PoolBwdArgs& a, hipStream_t st);
hipError_t launch_avgpool_fwd(int dtype, const void* x, float* y, int N, int HW, int C, hipStream_t st);
hipError_t launch_avgpool_bwd(int dtype, const float* dy, void* dx, int N, int HW, int C, hipStream_t st);
hipError_t launch_bn_bwd_reduce(int dtype, const BnBwdArgs& a, hipStream_t st);
hipError_t launch_bn_bwd_apply(int dtype, const BnBwdArgs& a, hipStream_t st);
// a downsampling block's two BatchNorms on one gradient (bn2 + the projection's): one reduce and one apply pass for both
bool bn_bwd_pair_ok(const BnBwdArgs& a, const BnBwdArgs& b);
// keep_g / from_g = 0: g is never written; the apply pass forms it again from (dy, mask)
hipError_t launch_bn_bwd_reduce_pair(int dtype, const BnBwdArgs& a, const BnBwdArgs& b, int keep_g, hipStream_t st);
hipError_t launch_bn_bwd_apply_pair(int dtype, const BnBwdArgs& a, const BnBwdArgs& b, int from_g, hipStream_t st);
hipError_t launch_bn_param_grads(const double* sums, const float* invstd, float* dgamma, float* dbeta, int C, hipStream_t st);
hipError_t launch_bn_param_grads_scaled(const double* sums, const float* invstd, float* dgamma, float* dbeta, int C, float scale, hipStream_t st);
// heads.hip
hipError_t launch_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int relu, hipStream_t st);
hipError_t launch_linear_bwd(const float* x, const float* w, const float* dy, const float* yact, float* dx, float* dw, float* db,
                             int M, int N, int K, int dx_accumulate, float* scratch, hipStream_t st);
hipError_t launch_loss(const LossArgs& a, hipStream_t st);
// the loss with options (sslcr_loss_ex): its own single-workgroup kernel, launch_loss keeps its bits and its launch
hipError_t launch_loss_ex(const LossArgs& a, const LossOpts& o, hipStream_t st);
hipError_t launch_ce_denominator(const int64_t* y, int n, int C, const float* w, int ignore_index, float* out2, hipStream_t st);
inline LossOpts loss_opts_default() {
  LossOpts o;
  o.class_weight = nullptr; o.label_smoothing = 0.f; o.ignore_index = -100; o.threshold = 0.f; o.temperature = 0.f;
  o.denominator = nullptr; o.stats = nullptr;
  return o;
}
// nothing set that launch_loss does not already compute: the caller then issues launch_loss itself
inline bool loss_opts_is_default(const LossOpts& o) {
  return !o.class_weight && o.label_smoothing == 0.f && o.ignore_index == -100 && o.threshold == 0.f && o.temperature == 0.f &&
         !o.denominator && !o.stats;
}
// nullptr, or what is wrong with the options for a loss of this kind and class count (decided on the host, before any launch)
inline const char* loss_opts_error(int kind, int C, const LossOpts& o) {
  if (loss_opts_is_default(o)) return nullptr;
  if (kind != 1 && kind != 2) return "loss options apply to the cross-entropy kinds (1, 2) only, not to the MSE kinds (0, 3)";
  if (C > 64) return "C > 64";
  if (!(o.label_smoothing >= 0.f && o.label_smoothing < 1.f)) return "label_smoothing outside [0, 1)";
  if (!(o.threshold >= 0.f && o.threshold <= 1.f)) return "threshold outside [0, 1]";
  if (!(o.temperature >= 0.f)) return "temperature < 0";
  if (kind == 2 && (o.threshold != 0.f || o.temperature != 0.f)) return "threshold / temperature need the consistency term (kind 1)";
  return nullptr;
}
hipError_t launch_softmax_col(const float* logits, float* out, int n, int C, int col, hipStream_t st);
hipError_t launch_predict(const sslcr_predict_desc& a, hipStream_t st);
// wsi.hip
hipError_t launch_wsi_gather(const sslcr_wsi_gather_desc& a, hipStream_t st);
// tta.hip
hipError_t launch_wsi_gather_d4(const sslcr_wsi_gather_desc& a, const int32_t* orient, hipStream_t st);
hipError_t launch_d4_transform(const sslcr_d4_desc& a, hipStream_t st);
hipError_t launch_predict_tta(const sslcr_predict_tta_desc& a, hipStream_t st);
// mining.hip
hipError_t launch_tissue_bits(const sslcr_tissue_bits_desc& a, hipStream_t st);
hipError_t launch_lab_a_sum(const sslcr_lab_a_sum_desc& a, hipStream_t st);
hipError_t launch_tile_popcount(const sslcr_tile_popcount_desc& a, hipStream_t st);
hipError_t launch_rsp_gather(const sslcr_rsp_gather_desc& a, hipStream_t st);
// annotation.hip
hipError_t launch_points_in_polygons(const sslcr_pip_desc& a, hipStream_t st);
hipError_t launch_map_confusion(const sslcr_map_confusion_desc& a, hipStream_t st);
// froc.hip
hipError_t launch_label_components(const sslcr_label_desc& a, hipStream_t st);
hipError_t launch_gaussian_smooth(const sslcr_smooth_desc& a, hipStream_t st);
hipError_t launch_nms_candidates(const sslcr_nms_desc& a, hipStream_t st);
hipError_t launch_nms_rounds(const sslcr_nms_desc& a, int rounds, hipStream_t st);
hipError_t launch_nms_collect(const sslcr_nms_desc& a, hipStream_t st);
hipError_t launch_lesion_hits(const sslcr_hits_desc& a, hipStream_t st);
// evalmask.hip
hipError_t launch_edt_squared(const sslcr_edt_desc& a, hipStream_t st);
hipError_t launch_fill_holes(const sslcr_fill_desc& a, hipStream_t st);
hipError_t launch_region_moments(const sslcr_moments_desc& a, hipStream_t st);
// rank.hip
hipError_t launch_sort_pairs(const sslcr_sort_desc& a, hipStream_t st);
hipError_t launch_rank_keys(const sslcr_rank_keys_desc& a, hipStream_t st);
hipError_t launch_auc_counts(const sslcr_auc_desc& a, hipStream_t st);
// resample.hip: which form serves a descriptor is decided ONCE, here -- the launch, sslcr_resample_plan and the tests read this plan
using ResamplePlan = sslcr_resample_plan_info;
// nullptr and *out filled, or what is wrong with the descriptor (host only: no device call, no device pointer read)
const char* resample_plan(const sslcr_resample_desc& a, ResamplePlan* out);
hipError_t launch_resample(const sslcr_resample_desc& a, const ResamplePlan& p, hipStream_t st);
// knn.hip: the tile shape and the slice count are decided ONCE, here -- the launch, sslcr_knn_plan, the Python layer and the tests read this plan
using KnnPlan = sslcr_knn_plan_info;
// nullptr and *out filled, or what is wrong with the arguments (host only)
const char* knn_plan(int nq, int nb, int D, int k, int slices_hint, KnnPlan* out);
hipError_t launch_knn_topk(const sslcr_knn_desc& a, const KnnPlan& p, hipStream_t st);
hipError_t launch_l2_normalize(const float* x, float* y, int n, int D, float eps, hipStream_t st);
hipError_t launch_knn_vote(const sslcr_knn_vote_desc& a, hipStream_t st);
// tsne.hip: the row tile, the chunk and the slice count are decided ONCE, here -- the launches, sslcr_tsne_plan, the Python layer and the tests read this plan
using TsnePlan = sslcr_tsne_plan_info;
// nullptr and *out filled, or what is wrong with the arguments (host only)
const char* tsne_plan(int n, int slices_hint, TsnePlan* out);
hipError_t launch_tsne_pair_dist2(const float* x, const int32_t* indices, float* dist2, int n, int D, int k, hipStream_t st);
hipError_t launch_tsne_affinities(const float* dist2, float* P, double* beta, int n, int k, float perplexity, hipStream_t st);
hipError_t launch_tsne_repulsion(const sslcr_tsne_grad_desc& a, const TsnePlan& p, hipStream_t st);
hipError_t launch_tsne_update(const sslcr_tsne_grad_desc& a, const TsnePlan& p, hipStream_t st);
hipError_t launch_tsne_kl(const double* kl_rows, const float* grad, const double* Z, double* log_row, int n, int iteration, hipStream_t st);
// linprobe.hip: tile rows, workgroups, column slices and the form are decided ONCE, here -- the launch, sslcr_linprobe_plan, the Python layer and the tests read this plan
using LinprobePlan = sslcr_linprobe_plan_info;
// nullptr and *out filled, or what is wrong with the arguments (host only)
const char* linprobe_plan(int n, int D, int C, int loss, int groups_hint, LinprobePlan* out);
// fwd_only: the logits alone (sslcr_linprobe_logits)
hipError_t launch_linprobe(const sslcr_linprobe_desc& a, const LinprobePlan& p, bool fwd_only, hipStream_t st);
// augment.hip
hipError_t launch_weak_augment(const sslcr_weak_aug_desc& a, hipStream_t st);
hipError_t launch_hed_colour(const sslcr_colour_aug_desc& a, hipStream_t st);
hipError_t launch_brightness_contrast(const sslcr_brightness_contrast_desc& a, hipStream_t st);
hipError_t launch_augv2(const sslcr_augv2_desc& a, hipStream_t st);
hipError_t launch_augv2_colour(const sslcr_augv2_colour_desc& a, hipStream_t st);
// augment_v1.hip
hipError_t launch_augv1(const sslcr_augv1_desc& a, hipStream_t st);
hipError_t launch_augv1_philox(unsigned long long seed, uint32_t first, int count, uint32_t* words, hipStream_t st);
void cv_warp_table(int16_t* table);                       // host only
// bytes per image of the RESIZE workspace: a planar S' x S' image for S' <= smax, rounded up to 16
__host__ __device__ inline size_t augv1_work_stride(int smax) { return (((size_t)3 * smax * smax) + 15) & ~(size_t)15; }
// optim.hip
struct OptTable { OptArgs row[SSLCR_MAX_OPT_GROUPS]; };   // the kernels' by-value table: a tensor's row is row[TensorDesc.group]
// every row a no-op (SGD with lr 0, momentum 1 and gradient scale 0: p and the momentum buffer are rewritten with their own values;
// the SGD form because it touches only s1, which every descriptor has), so that a descriptor whose group lies past the caller's rows
// -- the device-resident descriptors of sslcr_optimizer_step_groups cannot be checked on the host -- leaves its tensor as it was
inline OptTable opt_table_noop() {
  OptTable t;
  for (OptArgs& o : t.row) { o.kind = 1; o.lr = 0.f; o.beta1 = 0.f; o.beta2 = 0.f; o.eps = 0.f; o.wd = 0.f; o.momentum = 1.f; o.bc1 = 1.f; o.bc2 = 1.f; o.first_step = 0; o.grad_scale = 0.f; }
  return t;
}
// coef: NULL, or a device float the gradient scale is multiplied with (the clipping coefficient of launch_grad_norm)
hipError_t launch_optimizer(const TensorDesc* d_descs, int ntensors, int max_n, const OptTable& tab, const float* coef, hipStream_t st);
constexpr int OPT_CHUNK = 2048;     // elements per work-list entry
constexpr int OPT_TILE = 16 * 16 * 9; // ... and per LDS-transposed 3x3 filter tile (chunk.y = -(tile + 1))
constexpr int OPT_CHUNK_GROUP_SHIFT = 24;   // chunk.x = tensor index | TensorDesc.group << 24
hipError_t launch_optimizer_chunks(const TensorDesc* d_descs, const void* d_chunks /* int2 {tensor | group << 24, first element} */, int nchunks,
                                   const OptTable& tab, const float* coef, hipStream_t st);
constexpr int GRAD_NORM_BLOCKS = 1024;   // workgroups of the sum-of-squares pass = doubles in `partials` (a multiple of 256)
hipError_t launch_grad_norm(const float* g, size_t n, float max_norm, double* partials /* [GRAD_NORM_BLOCKS] */, float* out2, hipStream_t st);
// dst[i] = dst[i] + src[i], i < n: any n, any two 4-byte-aligned bases (sslcr_grad_accumulate)
hipError_t launch_grad_accumulate(float* dst, const float* src, size_t n, hipStream_t st);
hipError_t launch_axpby(float* p, float* q, size_t n, float alpha, int copy_back, hipStream_t st);
hipError_t launch_fill(float* p, size_t n, float v, hipStream_t st);
hipError_t launch_pack_conv(int dtype, const PackArgs& a, hipStream_t st);
hipError_t launch_pack_stem(int dtype, const PackArgs& a, hipStream_t st);
hipError_t launch_copy2d(float* dst, long ldd, const float* src, long lds, int rows, int w, int accumulate, hipStream_t st);
hipError_t launch_copy2d_multi(float* dst, long ldd, int ndst, long dstep, const float* src, long lds, int nsrc, long sstep, int rows, int w,
                               hipStream_t st);
hipError_t launch_unpack_grad(const float* g, float* out, int K, int C, int RS, hipStream_t st);
// capi.cpp
int fail(const char* fmt, ...);
int check(hipError_t e, const char* what);

}  // namespace sslcr
