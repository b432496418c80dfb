// extern "C" boundary of libsslcr.so: argument checks, error strings, no exceptions across the ABI.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <new>

#include "kernels.hpp"

namespace sslcr {
thread_local char g_err[512] = "";
int fail(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return -1;
}
int check(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  return fail("%s: %s", what, hipGetErrorString(e));
}
}  // namespace sslcr

using namespace sslcr;

#define NEED(cond, what) \
  do {                   \
    if (!(cond)) return fail("%s: invalid argument (%s)", __func__, what); \
  } while (0)
#define DT_OK(dt) NEED((dt) == SSLCR_F32 || (dt) == SSLCR_BF16, "dtype")
// the alignment include/sslcr.h states for a pointer ("Alignment (...)": the widest access a kernel makes through it); NULL passes
#define ALIGNED(p, mask) ((reinterpret_cast<uintptr_t>(p) & (mask)) == 0)
#define NEED_AL(p, n) NEED(ALIGNED(p, (n) - 1), #p " must be " #n "-byte aligned")
#define CONV_DESC_ALIGNED(d)                                                                                          \
  NEED_AL(d->x, 16); NEED_AL(d->w, 16); NEED_AL(d->y, 16); NEED_AL(d->residual, 16); NEED_AL(d->mask_x, 16);          \
  NEED_AL(d->bias, 16); NEED_AL(d->stats, 16); NEED_AL(d->out_scale, 16);                                             \
  NEED_AL(d->in_scale, 4); NEED_AL(d->in_shift, 4); NEED_AL(d->mask_scale, 4); NEED_AL(d->mask_shift, 4); NEED_AL(d->mask_mean, 4)
#define STEM_DESC_ALIGNED(d)                                                                                          \
  NEED_AL(d->w, 16); NEED_AL(d->y, 16);                                                                               \
  NEED_AL(d->x, 4); NEED_AL(d->x2, 4); NEED_AL(d->bias, 4); NEED_AL(d->stats, 4); NEED_AL(d->out_scale, 4)
#define STEM_WGRAD_DESC_ALIGNED(d) NEED_AL(d->dy, 16); NEED_AL(d->x, 4); NEED_AL(d->x2, 4); NEED_AL(d->dw, 4)
#define BN_BWD_DESC_ALIGNED(d)                                                                                        \
  NEED_AL(d->dy, 16); NEED_AL(d->x, 16); NEED_AL(d->yact, 16); NEED_AL(d->dx, 16); NEED_AL(d->gout, 16);              \
  NEED_AL(d->pool_dy, 16); NEED_AL(d->pool_y, 16); NEED_AL(d->sums, 8); NEED_AL(d->pool_argmax, 8);                   \
  NEED_AL(d->scale, 4); NEED_AL(d->shift, 4); NEED_AL(d->mean, 4); NEED_AL(d->invstd, 4); NEED_AL(d->dgamma, 4); NEED_AL(d->dbeta, 4)
#define LOSS_DESC_ALIGNED(d)                                                                                          \
  NEED_AL(d->logits, 4); NEED_AL(d->logits_t, 4); NEED_AL(d->target_f, 4); NEED_AL(d->target_i, 8); NEED_AL(d->dlogits, 4); NEED_AL(d->out, 4)

extern "C" {

int sslcr_version(void) { return 16; }      // = the build round; the ABI notes in include/sslcr.h name the version a behaviour changed in
const char* sslcr_last_error(void) { return g_err; }

int sslcr_switch_count(void) { return sw::COUNT; }
int sslcr_switch_info(int i, sslcr_switch_row* out) {
  NEED(out && i >= 0 && i < sw::COUNT, "index");
  static const char* const kRule[] = {"ATOI", "LEAD0", "INT", "PRESENT"};
  const sw::Row& r = sw::row(i);
  const sw::Value v = sw::get(r.id);
  *out = {r.name, r.group, kRule[r.rule], r.when == sw::CALL ? "call" : "process", r.meaning, r.dflt, v.v, v.set ? 1 : 0};
  return 0;
}

int sslcr_conv2d(int dtype, const sslcr_conv_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->w && d->y, "null tensor");
  CONV_DESC_ALIGNED(d);
  NEED(d->N > 0 && d->C > 0 && d->K > 0 && d->R > 0 && d->S > 0 && d->stride > 0, "shape");
  NEED(d->C % (dtype == SSLCR_BF16 ? 64 : 32) == 0, "C must be a multiple of the 128-byte channel slab");
  NEED(d->K % 64 == 0, "K % 64");
  NEED(d->osh >= 1 && d->PH > 0 && d->PW > 0, "pixel space");
  const ConvPlan p = conv_plan(dtype, *d);
  NEED(p.seg_ok, "seg_images: no segment form for this shape / dtype (sslcr_conv2d_segments_ok)");
  return check(launch_conv(dtype, *d, p, (hipStream_t)stream), "conv2d");
}
// (-1 also where seg_images > N on a kernel whose grid is split among the segments: ConvPlan::rows)
int sslcr_conv2d_partial_rows(const sslcr_conv_desc* d) { return d ? conv_partials_rows(*d) : -1; }
int sslcr_conv2d_segments_ok(int dtype, const sslcr_conv_desc* d) { return (d && (dtype == DT_F32 || dtype == DT_BF16) && conv_segments_ok(dtype, *d)) ? 1 : 0; }
const char* sslcr_conv2d_kernel_name(int dtype, const sslcr_conv_desc* d) { return d ? conv_kernel_name(dtype, *d) : ""; }
int sslcr_conv2d_s2_pair_ok(int dtype, const sslcr_conv_desc* c1, const sslcr_conv_desc* ds) {
  return (c1 && ds && conv_s2_pair_ok(dtype, *c1, *ds)) ? 1 : 0;
}
int sslcr_conv2d_s2_pair(int dtype, const sslcr_conv_desc* c1, const sslcr_conv_desc* ds, void* stream) {
  DT_OK(dtype);
  NEED(c1 && ds && c1->x && c1->w && c1->y && ds->w && ds->y, "null tensor");
  CONV_DESC_ALIGNED(c1);
  CONV_DESC_ALIGNED(ds);
  NEED(conv_s2_pair_ok(dtype, *c1, *ds), "pair not served (sslcr_conv2d_s2_pair_ok)");
  return check(launch_conv_s2(*c1, ds, (hipStream_t)stream), "conv2d_s2_pair");
}

int sslcr_conv2d_fp8(const sslcr_conv_desc* d, const sslcr_fp8_desc* q, void* stream) {
  NEED(d && q && d->x && d->y && q->w8 && q->w_dequant, "null tensor");
  CONV_DESC_ALIGNED(d);
  NEED_AL(q->w8, 16); NEED_AL(q->w_dequant, 16); NEED_AL(q->x_scale_dev, 4); NEED_AL(q->amax_out, 4);
  NEED(q->x_scale > 0.f, "x_scale must be positive");
  NEED(!d->in_scale || d->in_shift, "in_scale without in_shift (the load path reads both)");
  NEED(conv_fp8_mode(*d) != 0, "shape not served by the fp8 kernel (3x3/1, C % 128, K % 128, 16x16-tileable or 8x8 with N % 4)");
  return check(launch_conv_fp8(*d, *q, (hipStream_t)stream), "conv2d_fp8");
}
int sslcr_conv2d_fp8_partial_rows(const sslcr_conv_desc* d) { return (d && conv_fp8_mode(*d)) ? conv_fp8_rows(*d) : 0; }
const char* sslcr_conv2d_fp8_kernel_name(const sslcr_conv_desc* d) { return (d && conv_fp8_mode(*d)) ? conv_fp8_name(*d) : ""; }
int sslcr_fp8_scale_update(float* slots, int n, void* stream) {
  NEED(slots && n > 0, "slots");
  return check(launch_fp8_scale_update(slots, n, (hipStream_t)stream), "fp8_scale_update");
}
int sslcr_pack_conv_fp8(const sslcr_pack_fp8_desc* d, void* stream) {
  NEED(d && d->w && d->w8 && d->w_dequant && d->K > 0 && d->C > 0, "args");
  NEED(!d->gamma || (d->beta && d->rmean && d->rvar), "BatchNorm fold needs gamma, beta, running mean and var");
  return check(launch_pack_fp8(*d, (hipStream_t)stream), "pack_conv_fp8");
}

const char* sslcr_conv2d_wgrad_kernel_name(int dtype, const sslcr_wgrad_desc* d) { return d ? wgrad_kernel_name(dtype, *d) : ""; }
int sslcr_conv2d_wgrad(int dtype, const sslcr_wgrad_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->dy && d->dw, "null tensor");
  NEED_AL(d->x, 16); NEED_AL(d->dy, 16); NEED_AL(d->dw, 4); NEED_AL(d->in_scale, 4); NEED_AL(d->in_shift, 4);
  NEED(d->C % 64 == 0 && d->K % 64 == 0, "C,K % 64");
  NEED((d->R == 3 && d->S == 3) || (d->R == 1 && d->S == 1), "3x3 or 1x1");
  return check(launch_wgrad(dtype, *d, (hipStream_t)stream), "conv2d_wgrad");
}

int sslcr_probe_tr16(const uint16_t* in, const int* byte_addr, uint16_t* out, void* stream) {
  NEED(in && byte_addr && out, "null");
  return check(launch_probe_tr16(in, byte_addr, out, (hipStream_t)stream), "probe_tr16");
}

int sslcr_stem_conv(int dtype, const sslcr_stem_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->w && d->y, "null tensor");
  STEM_DESC_ALIGNED(d);
  NEED(d->OH == (d->H + 6 - 7) / 2 + 1 && d->OW == (d->W + 6 - 7) / 2 + 1, "7x7/2 pad 3 output dims");
  NEED(!d->x2 || (d->n_split >= 0 && d->n_split <= d->N), "n_split outside the batch");
  return check(launch_stem(dtype, *d, (hipStream_t)stream), "stem_conv");
}
int sslcr_stem_conv_pool(int dtype, const sslcr_stem_desc* d, int POH, int POW, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->w && d->y, "null");
  STEM_DESC_ALIGNED(d);
  NEED(stem_pool_ok(dtype, *d, POH, POW), "shape / mode not served by the fused stem + max-pool kernel");
  return check(launch_stem_pool(dtype, *d, POH, POW, (hipStream_t)stream), "stem_conv_pool");
}
int sslcr_stem_partial_rows(const sslcr_stem_desc* d) { return d ? stem_partials_rows(*d) : -1; }
int sslcr_stem_wgrad(int dtype, const sslcr_stem_wgrad_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->dy && d->dw, "null tensor");
  STEM_WGRAD_DESC_ALIGNED(d);
  NEED(!d->x2 || (d->n_split >= 0 && d->n_split <= d->N), "n_split outside the batch");
  return check(launch_stem_wgrad(dtype, *d, (hipStream_t)stream), "stem_wgrad");
}
const char* sslcr_stem_wgrad_pool_kernel_name(int dtype, const sslcr_stem_wgrad_desc* w) { return w ? stem_wgrad_pool_name(dtype, *w) : ""; }
int sslcr_stem_wgrad_pool(int dtype, const sslcr_stem_wgrad_desc* w, const sslcr_bn_bwd_desc* bn, void* stream) {
  DT_OK(dtype);
  NEED(w && w->x && w->dw && bn && bn->pool_dy && bn->pool_argmax && bn->x && bn->sums && bn->mean && bn->invstd && bn->scale && bn->shift, "null tensor");
  STEM_WGRAD_DESC_ALIGNED(w);
  BN_BWD_DESC_ALIGNED(bn);
  NEED(!w->x2 || (w->n_split >= 0 && w->n_split <= w->N), "n_split outside the batch");
  NEED(bn->C == 64 && bn->pH == w->OH && bn->pW == w->OW && bn->pixels == (size_t)w->N * w->OH * w->OW, "bn descriptor is not this stem's");
  NEED(!bn->g_in_reduce && !bn->gout, "pool form has no g output");
  return check(launch_stem_wgrad_pool(dtype, *w, *bn, (hipStream_t)stream), "stem_wgrad_pool");
}

int sslcr_bn_finalize(const sslcr_bn_finalize_desc* d, void* stream) {
  NEED(d && d->C > 0, "desc");
  NEED_AL(d->partials, 4); NEED_AL(d->gamma, 4); NEED_AL(d->beta, 4); NEED_AL(d->scale, 4); NEED_AL(d->shift, 4); NEED_AL(d->mean, 4);
  NEED_AL(d->invstd, 4); NEED_AL(d->running_mean, 4); NEED_AL(d->running_var, 4); NEED_AL(d->tickets, 4);
  NEED_AL(d->num_batches_tracked, 8); NEED_AL(d->sums_out, 8); NEED_AL(d->sums_in, 8); NEED_AL(d->stage, 8);
  NEED(d->sums_in || (d->partials && d->stage && d->rows > 0), "partials/stage");
  NEED(d->sums_out || (d->gamma && d->beta && d->scale && d->shift && d->count > 0), "finalize outputs");
  return check(launch_bn_finalize(*d, (hipStream_t)stream), "bn_finalize");
}
int sslcr_bn_act(int dtype, const sslcr_bn_act_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->y && d->scale && d->shift, "null");
  NEED_AL(d->x, 16); NEED_AL(d->res, 16); NEED_AL(d->y, 16);
  NEED_AL(d->scale, 4); NEED_AL(d->shift, 4); NEED_AL(d->rscale, 4); NEED_AL(d->rshift, 4);      // (ybits: bytes, any address)
  NEED(d->C % 8 == 0, "C % 8");
  return check(launch_bn_act(dtype, *d, (hipStream_t)stream), "bn_act");
}
int sslcr_bn_relu_maxpool(int dtype, const sslcr_pool_fwd_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->y, "null");
  NEED_AL(d->x, 16); NEED_AL(d->y, 16); NEED_AL(d->argmax, 8); NEED_AL(d->scale, 4); NEED_AL(d->shift, 4);
  if (!d->scale || !d->shift) {
    const int cols = d->C / (dtype == SSLCR_BF16 ? 8 : 4);
    NEED(!d->scale && !d->shift && !d->argmax, "plain max-pool (scale = shift = NULL) records no argmax");
    NEED(cols >= 1 && cols <= 256 && 256 % cols == 0 && d->C % (dtype == SSLCR_BF16 ? 8 : 4) == 0, "plain max-pool: unsupported channel count");
  }
  return check(launch_bn_relu_maxpool(dtype, *d, (hipStream_t)stream), "bn_relu_maxpool");
}
int sslcr_maxpool_relu_bwd(int dtype, const sslcr_pool_bwd_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->x && d->dy && d->dx && d->argmax, "null");
  NEED_AL(d->dy, 16); NEED_AL(d->x, 16); NEED_AL(d->dx, 16); NEED_AL(d->argmax, 8); NEED_AL(d->scale, 4); NEED_AL(d->shift, 4);
  return check(launch_maxpool_relu_bwd(dtype, *d, (hipStream_t)stream), "maxpool_relu_bwd");
}
int sslcr_avgpool_fwd(int dtype, const void* x, float* y, int N, int HW, int C, void* stream) {
  DT_OK(dtype);
  NEED(x && y && N > 0 && HW > 0 && C % 8 == 0, "args");
  NEED_AL(x, 16); NEED_AL(y, 4);
  return check(launch_avgpool_fwd(dtype, x, y, N, HW, C, (hipStream_t)stream), "avgpool_fwd");
}
int sslcr_avgpool_bwd(int dtype, const float* dy, void* dx, int N, int HW, int C, void* stream) {
  DT_OK(dtype);
  NEED(dy && dx && N > 0 && HW > 0 && C % 8 == 0, "args");
  NEED_AL(dy, 4); NEED_AL(dx, 16);
  return check(launch_avgpool_bwd(dtype, dy, dx, N, HW, C, (hipStream_t)stream), "avgpool_bwd");
}
int sslcr_bn_bwd_reduce(int dtype, const sslcr_bn_bwd_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && (d->dy || (d->pool_dy && d->pool_argmax)) && d->x && d->sums && d->mean, "null");
  BN_BWD_DESC_ALIGNED(d);
  NEED(!d->g_in_reduce || (d->yact && d->gout && d->dy && !d->pool_dy), "g_in_reduce needs dy, yact and gout");
  return check(launch_bn_bwd_reduce(dtype, *d, (hipStream_t)stream), "bn_bwd_reduce");
}
int sslcr_bn_bwd_apply(int dtype, const sslcr_bn_bwd_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && (d->dy || (d->pool_dy && d->pool_argmax)) && d->x && d->sums && d->dx && d->mean && d->invstd && d->scale, "null");
  BN_BWD_DESC_ALIGNED(d);
  NEED(!d->g_in_reduce || (d->yact && d->gout && d->dy && !d->pool_dy), "g_in_reduce needs dy, yact and gout");
  return check(launch_bn_bwd_apply(dtype, *d, (hipStream_t)stream), "bn_bwd_apply");
}
int sslcr_bn_param_grads(const double* sums, const float* invstd, float* dgamma, float* dbeta, int C, void* stream) {
  NEED(sums && invstd && dgamma && dbeta, "null");
  NEED_AL(sums, 8); NEED_AL(invstd, 4); NEED_AL(dgamma, 4); NEED_AL(dbeta, 4);
  return check(launch_bn_param_grads(sums, invstd, dgamma, dbeta, C, (hipStream_t)stream), "bn_param_grads");
}

int sslcr_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int relu, void* stream) {
  NEED(x && w && y && M > 0 && N > 0 && K > 0, "args");
  NEED_AL(x, 4); NEED_AL(w, 4); NEED_AL(b, 4); NEED_AL(y, 4);
  return check(launch_linear_fwd(x, w, b, y, M, N, K, relu, (hipStream_t)stream), "linear_fwd");
}
int sslcr_linear_bwd(const float* x, const float* w, const float* dy, const float* yact, float* dx, float* dw, float* db,
                     int M, int N, int K, int dx_accumulate, float* scratch, void* stream) {
  NEED(x && w && dy && scratch && M > 0 && N > 0 && K > 0, "args");
  NEED_AL(x, 4); NEED_AL(w, 4); NEED_AL(dy, 4); NEED_AL(yact, 4); NEED_AL(dx, 4); NEED_AL(dw, 4); NEED_AL(db, 4); NEED_AL(scratch, 4);
  return check(launch_linear_bwd(x, w, dy, yact, dx, dw, db, M, N, K, dx_accumulate, scratch, (hipStream_t)stream), "linear_bwd");
}
int sslcr_loss(const sslcr_loss_desc* d, void* stream) {
  NEED(d && d->logits && d->out && d->nx > 0 && d->C > 0 && d->C <= 64, "args");
  LOSS_DESC_ALIGNED(d);
  return check(launch_loss(*d, (hipStream_t)stream), "loss");
}

int sslcr_loss_ex(const sslcr_loss_desc* d, const sslcr_loss_opts* o, void* stream) {
  if (!o) return sslcr_loss(d, stream);
  NEED(d && d->logits && d->out && d->nx > 0 && d->C > 0 && d->C <= 64, "args");
  LOSS_DESC_ALIGNED(d);
  NEED_AL(o->class_weight, 4); NEED_AL(o->denominator, 4); NEED_AL(o->stats, 4);
  const char* why = loss_opts_error(d->kind, d->C, *o);
  if (why) return fail("sslcr_loss_ex: invalid argument (%s)", why);
  // the MSE kinds have no options: sslcr_loss's own launch.  The cross-entropy kinds take the new kernel whenever opts is given --
  // its default arithmetic is loss_kernel's, bit for bit, and rows that carry the default ignore_index are honoured
  if (d->kind != 1 && d->kind != 2) return check(launch_loss(*d, (hipStream_t)stream), "loss");
  NEED(d->target_i && (d->kind == 2 || d->nu == 0 || d->logits_t), "cross-entropy needs target_i (and logits_t for the consistency rows)");
  NEED(d->nu >= 0, "nu");
  return check(launch_loss_ex(*d, *o, (hipStream_t)stream), "loss_ex");
}
int sslcr_ce_denominator(const int64_t* target_i, int n, int C, const float* class_weight, int ignore_index, float* out2, void* stream) {
  NEED(out2 && (target_i || n == 0) && n >= 0 && C > 0 && C <= 64, "args");
  NEED_AL(target_i, 8); NEED_AL(class_weight, 4); NEED_AL(out2, 4);
  return check(launch_ce_denominator(target_i, n, C, class_weight, ignore_index, out2, (hipStream_t)stream), "ce_denominator");
}

int sslcr_softmax_col(const float* logits, float* out, int n, int C, int col, void* stream) {
  NEED(logits && out && n > 0 && C > 0 && C <= 64 && col >= 0 && col < C, "args");
  NEED_AL(logits, 4); NEED_AL(out, 4);
  return check(launch_softmax_col(logits, out, n, C, col, (hipStream_t)stream), "softmax_col");
}

// the argument rules sslcr_predict and sslcr_predict_tta share; NULL = fine.  (n == 0 is a no-op the callers return from first.)
static const char* predict_args_error(const sslcr_predict_desc& d) {
  if (!d.logits) return "null logits";
  if (d.confusion && !d.target) return "confusion needs target";
  if (reinterpret_cast<uintptr_t>(d.confusion) & 7) return "confusion alignment";
  if (d.map && !(d.map_index && d.map_size >= 0)) return "map needs map_index and map_size >= 0";
  if (d.map && !(d.col >= 0 && d.col < d.C)) return "col outside [0, C)";
  return nullptr;
}
int sslcr_predict(const sslcr_predict_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->n >= 0 && d->C >= 1 && d->C <= 64, "n >= 0 and 1 <= C <= 64");
  if (d->n == 0) return 0;
  const char* why = predict_args_error(*d);
  NEED(!why, why);
  return check(launch_predict(*d, (hipStream_t)stream), "predict");
}
int sslcr_predict_tta(const sslcr_predict_tta_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->p.n >= 0 && d->p.C >= 1 && d->p.C <= 64, "n >= 0 and 1 <= C <= 64");
  NEED(d->G >= 1 && d->G <= SSLCR_TTA_MAX, "G outside [1, 8]");
  NEED(d->mode == 0 || d->mode == 1, "mode outside {0, 1}");
  NEED(d->mode == 0 || (!d->p.map && !d->p.pred && !d->p.confusion), "mode 1 (raw outputs) has no map, pred or confusion");
  if (d->p.n == 0) return 0;
  const char* why = predict_args_error(d->p);
  NEED(!why, why);
  return check(launch_predict_tta(*d, (hipStream_t)stream), "predict_tta");
}
// the argument rules the two gathers share
static const char* wsi_gather_args_error(const sslcr_wsi_gather_desc& d) {
  if (!(d.S >= 1 && d.N >= 0)) return "S >= 1 and N >= 0";
  if (!(d.RH >= 1 && d.RW >= 1)) return "empty region";
  if (!(d.fill >= 0 && d.fill <= 255)) return "fill outside [0, 255]";
  if (d.N == 0) return nullptr;
  if (!(d.src && d.xy && d.dst)) return "null tensor";
  if (reinterpret_cast<uintptr_t>(d.xy) & 3) return "xy alignment";
  return nullptr;
}
int sslcr_wsi_gather(const sslcr_wsi_gather_desc* d, void* stream) {
  NEED(d, "null descriptor");
  const char* why = wsi_gather_args_error(*d);
  NEED(!why, why);
  if (d->N == 0) return 0;
  return check(launch_wsi_gather(*d, (hipStream_t)stream), "wsi_gather");
}
int sslcr_wsi_gather_d4(const sslcr_wsi_gather_desc* d, const int32_t* orient, void* stream) {
  if (!orient) return sslcr_wsi_gather(d, stream);                        // the plain gather's own launch
  NEED(d, "null descriptor");
  const char* why = wsi_gather_args_error(*d);
  NEED(!why, why);
  NEED((reinterpret_cast<uintptr_t>(orient) & 3) == 0, "orient alignment");
  if (d->N == 0) return 0;
  return check(launch_wsi_gather_d4(*d, orient, (hipStream_t)stream), "wsi_gather_d4");
}
// ---- tile mining for RSP pretraining (mining.hip)
static int grid_len(int size, int tile, int stride) {                      // len(range(stride, size - 1 - tile, stride))
  const int64_t stop = (int64_t)size - 1 - tile;
  return stop > stride ? (int)((stop - stride + stride - 1) / stride) : 0;
}
int sslcr_tissue_bits(const sslcr_tissue_bits_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->H >= 1 && d->W >= 1, "empty image");
  NEED(d->pitch >= (d->W + 31) / 32, "pitch < ceil(W / 32)");
  NEED(d->mode == SSLCR_TISSUE_HSV_S || d->mode == SSLCR_TISSUE_LAB_A, "mode outside {0, 1}");
  NEED(d->img && d->bits, "null tensor");
  NEED((reinterpret_cast<uintptr_t>(d->bits) & 3) == 0, "bits alignment");
  NEED(d->mode != SSLCR_TISSUE_LAB_A || d->lin, "mode lab_a needs lin");
  NEED(((reinterpret_cast<uintptr_t>(d->lin) | reinterpret_cast<uintptr_t>(d->thr_sum)) & 7) == 0, "lin / thr_sum alignment");
  NEED(!d->thr_sum || d->count > 0.0, "thr_sum needs count > 0");
  return check(launch_tissue_bits(*d, (hipStream_t)stream), "tissue_bits");
}
int sslcr_lab_a_sum(const sslcr_lab_a_sum_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->H >= 1 && d->W >= 1, "empty image");
  NEED(d->img && d->lin && d->partials && d->sum, "null tensor");
  NEED(((reinterpret_cast<uintptr_t>(d->lin) | reinterpret_cast<uintptr_t>(d->partials) | reinterpret_cast<uintptr_t>(d->sum)) & 7) == 0,
       "lin / partials / sum alignment");
  return check(launch_lab_a_sum(*d, (hipStream_t)stream), "lab_a_sum");
}
int sslcr_tile_popcount(const sslcr_tile_popcount_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->H >= 1 && d->W >= 1, "empty image");
  NEED(d->ph >= 1 && d->pw >= 1 && d->sh >= 1 && d->sw >= 1, "tile and stride >= 1");
  NEED(d->pitch >= (d->W + 31) / 32, "pitch < ceil(W / 32)");
  NEED(d->ny == grid_len(d->H, d->ph, d->sh) && d->nx == grid_len(d->W, d->pw, d->sw), "ny / nx are not the lengths of the grid's ranges");
  if (d->ny == 0 || d->nx == 0) return 0;
  NEED((int64_t)d->ny * d->nx < (int64_t)1 << 31, "grid too large");
  NEED(d->bits && d->count && d->keep, "null tensor");
  NEED(((reinterpret_cast<uintptr_t>(d->bits) | reinterpret_cast<uintptr_t>(d->count)) & 3) == 0, "bits / count alignment");
  return check(launch_tile_popcount(*d, (hipStream_t)stream), "tile_popcount");
}
int sslcr_rsp_gather(const sslcr_rsp_gather_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->S >= 1 && d->N >= 0 && d->T >= 1, "S >= 1, N >= 0 and T >= 1");
  for (int l = 0; l < 3; ++l) NEED(d->RH[l] >= 1 && d->RW[l] >= 1, "empty level");
  NEED(d->fill >= 0 && d->fill <= 255, "fill outside [0, 255]");
  if (d->N == 0) return 0;
  NEED(d->idx && d->label, "null tensor");
  for (int l = 0; l < 3; ++l) {
    NEED(d->src[l] && d->xy[l] && d->dst[l], "null tensor");
    NEED((reinterpret_cast<uintptr_t>(d->xy[l]) & 3) == 0, "xy alignment");
  }
  NEED(((reinterpret_cast<uintptr_t>(d->idx) | reinterpret_cast<uintptr_t>(d->label)) & 7) == 0, "idx / label alignment");
  return check(launch_rsp_gather(*d, (hipStream_t)stream), "rsp_gather");
}
// ---- Camelyon16 annotations (annotation.hip)
int sslcr_points_in_polygons(const sslcr_pip_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->N >= 0 && d->N < (int64_t)1 << 31, "N outside [0, 2^31)");
  NEED(d->P >= 0 && d->V >= 0, "P >= 0 and V >= 0");
  NEED(d->exact == 0 || d->exact == 1, "exact outside {0, 1}");
  if (!d->points) {
    const int64_t lim = (int64_t)1 << 53;
    NEED(d->nx >= 0 && d->ny >= 0 && (int64_t)d->nx * d->ny == d->N, "grid: nx * ny != N");
    NEED(d->step >= 0 && d->step < (int64_t)1 << 31 && d->x0 > -lim && d->x0 < lim && d->y0 > -lim && d->y0 < lim, "grid: coordinate magnitude");
    NEED(d->x0 + (int64_t)d->nx * d->step < lim && d->y0 + (int64_t)d->ny * d->step < lim, "grid: coordinate magnitude");
  }
  if (d->N == 0) return 0;
  NEED(d->inside && d->offsets, "null tensor");
  NEED(d->V == 0 || d->vertices, "null vertices");
  NEED(((reinterpret_cast<uintptr_t>(d->vertices) | reinterpret_cast<uintptr_t>(d->points)) & 15) == 0, "vertices / points alignment");
  NEED((reinterpret_cast<uintptr_t>(d->bounds) & 7) == 0, "bounds alignment");
  NEED(((reinterpret_cast<uintptr_t>(d->offsets) | reinterpret_cast<uintptr_t>(d->first)) & 3) == 0, "offsets / first alignment");
  return check(launch_points_in_polygons(*d, (hipStream_t)stream), "points_in_polygons");
}
int sslcr_map_confusion(const sslcr_map_confusion_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->X >= 1 && d->Y >= 1 && (int64_t)d->X * d->Y < (int64_t)1 << 31, "map shape");
  NEED(d->T >= 1 && d->T <= 64, "T outside [1, 64]");
  NEED(d->map && d->truth && d->tissue && d->thresholds && d->confusion, "null tensor");
  NEED(((reinterpret_cast<uintptr_t>(d->map) | reinterpret_cast<uintptr_t>(d->thresholds)) & 3) == 0, "map / thresholds alignment");
  NEED((reinterpret_cast<uintptr_t>(d->confusion) & 7) == 0, "confusion alignment");
  return check(launch_map_confusion(*d, (hipStream_t)stream), "map_confusion");
}
// ---- Camelyon16 lesion scoring (froc.hip)
#define MAP_SHAPE_OK(d) NEED((d)->X >= 1 && (d)->Y >= 1 && (int64_t)(d)->X * (d)->Y < (int64_t)1 << 31, "map shape")
int sslcr_label_components(const sslcr_label_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  NEED(d->connectivity == 1 || d->connectivity == 2, "connectivity outside {1, 2}");
  NEED(d->mask && d->labels && d->count && d->work, "null tensor");
  NEED(ALIGNED(d->mask, 3) && ALIGNED(d->labels, 3) && ALIGNED(d->count, 3) && ALIGNED(d->work, 3), "mask / labels / count / work alignment");
  return check(launch_label_components(*d, (hipStream_t)stream), "label_components");
}
int sslcr_gaussian_smooth(const sslcr_smooth_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  NEED(d->R >= 0 && d->R <= SSLCR_SMOOTH_MAX_R, "R outside [0, 64]");
  NEED(d->src && d->tmp && d->dst && d->weights, "null tensor");
  NEED(ALIGNED(d->src, 3) && ALIGNED(d->tmp, 3) && ALIGNED(d->dst, 3) && ALIGNED(d->weights, 3), "src / tmp / dst / weights alignment");
  NEED(d->tmp != d->src && d->tmp != d->dst, "tmp aliases src or dst");
  return check(launch_gaussian_smooth(*d, (hipStream_t)stream), "gaussian_smooth");
}
static int nms_desc_ok(const sslcr_nms_desc* d) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  NEED(d->radius >= 1, "radius < 1");
  NEED(d->max_detections >= 1, "max_detections < 1");
  NEED(d->ncand >= 0 && d->ncand <= (int64_t)d->X * d->Y, "ncand outside [0, X * Y]");
  NEED(d->map && d->state && d->cand && d->stage && d->counters && d->det_xy && d->det_prob, "null tensor");
  NEED(ALIGNED(d->map, 3) && ALIGNED(d->state, 3) && ALIGNED(d->cand, 3) && ALIGNED(d->stage, 3) && ALIGNED(d->counters, 3) &&
           ALIGNED(d->det_xy, 3) && ALIGNED(d->det_prob, 3), "map / state / cand / stage / counters / det_xy / det_prob alignment");
  return 0;
}
int sslcr_nms_candidates(const sslcr_nms_desc* d, void* stream) {
  if (nms_desc_ok(d)) return -1;
  return check(launch_nms_candidates(*d, (hipStream_t)stream), "nms_candidates");
}
int sslcr_nms_rounds(const sslcr_nms_desc* d, int rounds, void* stream) {
  if (nms_desc_ok(d)) return -1;
  NEED(rounds >= 0, "rounds < 0");
  return check(launch_nms_rounds(*d, rounds, (hipStream_t)stream), "nms_rounds");
}
int sslcr_nms_collect(const sslcr_nms_desc* d, void* stream) {
  if (nms_desc_ok(d)) return -1;
  return check(launch_nms_collect(*d, (hipStream_t)stream), "nms_collect");
}
int sslcr_lesion_hits(const sslcr_hits_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  NEED(d->L >= 0 && d->max_detections >= 1 && d->n_ignore >= 0, "L >= 0, max_detections >= 1 and n_ignore >= 0");
  NEED(d->labels && d->det_xy && d->det_prob && d->n_det && d->hit, "null tensor");
  NEED(d->L == 0 || d->tp_prob, "null tp_prob");
  NEED(d->n_ignore == 0 || d->ignore, "null ignore");
  NEED(ALIGNED(d->labels, 3) && ALIGNED(d->det_xy, 3) && ALIGNED(d->det_prob, 3) && ALIGNED(d->n_det, 3) && ALIGNED(d->ignore, 3) &&
           ALIGNED(d->hit, 3) && ALIGNED(d->tp_prob, 3), "labels / det_xy / det_prob / n_det / ignore / hit / tp_prob alignment");
  NEED(ALIGNED(d->areas, 7), "areas alignment");
  return check(launch_lesion_hits(*d, (hipStream_t)stream), "lesion_hits");
}
// ---- the Camelyon16 evaluation mask (evalmask.hip)
#define SQ_SHAPE_OK(d) NEED((int64_t)(d)->X * (d)->X + (int64_t)(d)->Y * (d)->Y < (int64_t)1 << 31, "X^2 + Y^2 >= 2^31")
int sslcr_edt_squared(const sslcr_edt_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  SQ_SHAPE_OK(d);
  NEED(d->limit >= 0, "limit < 0");
  NEED(d->invert == 0 || d->invert == 1, "invert outside {0, 1}");
  NEED(d->mask && d->out && d->work, "null tensor");
  NEED(ALIGNED(d->mask, 3) && ALIGNED(d->out, 3) && ALIGNED(d->work, 3), "mask / out / work alignment");
  NEED(d->out != d->work, "out aliases work");
  return check(launch_edt_squared(*d, (hipStream_t)stream), "edt_squared");
}
int sslcr_fill_holes(const sslcr_fill_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  NEED(d->mask && d->out && d->labels && d->count && d->work, "null tensor");
  NEED(d->out != d->mask, "out aliases mask");
  NEED(ALIGNED(d->out, 3) && ALIGNED(d->labels, 3) && ALIGNED(d->count, 3) && ALIGNED(d->work, 3), "out / labels / count / work alignment");
  return check(launch_fill_holes(*d, (hipStream_t)stream), "fill_holes");
}
int sslcr_region_moments(const sslcr_moments_desc* d, void* stream) {
  NEED(d, "null descriptor");
  MAP_SHAPE_OK(d);
  SQ_SHAPE_OK(d);
  NEED(d->L >= 0, "L < 0");
  NEED(d->labels, "null tensor");
  NEED(d->L == 0 || d->moments, "null moments");
  NEED(ALIGNED(d->labels, 3) && ALIGNED(d->moments, 7), "labels / moments alignment");
  return check(launch_region_moments(*d, (hipStream_t)stream), "region_moments");
}
// ---- ranking metrics (rank.hip)
static int64_t rank_tiles(int n) { return ((int64_t)n + SSLCR_SORT_TILE - 1) / SSLCR_SORT_TILE; }
size_t sslcr_sort_workspace_bytes(int B, int n) {
  if (B < 1 || B > 65535 || n < 1) return 0;
  return (size_t)B * 256 * (size_t)(rank_tiles(n) + 1) * sizeof(int);        // hist [B][256][tiles], then tot [B][256]
}
int sslcr_sort_pairs(const sslcr_sort_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->B >= 1 && d->B <= 65535, "B outside [1, 65535]");
  NEED(d->n >= 1, "n < 1");
  NEED(d->lo >= 0 && d->lo <= d->hi && d->hi <= 32, "not 0 <= lo <= hi <= 32");
  NEED(d->keys[0] && d->keys[1] && d->values[0] && d->values[1] && d->workspace, "null tensor");
  NEED(d->keys[0] != d->keys[1] && d->values[0] != d->values[1] && d->keys[0] != d->values[0] && d->keys[0] != d->values[1] &&
           d->keys[1] != d->values[0] && d->keys[1] != d->values[1], "the four buffers must be distinct");
  NEED(ALIGNED(d->keys[0], 3) && ALIGNED(d->keys[1], 3) && ALIGNED(d->values[0], 3) && ALIGNED(d->values[1], 3) && ALIGNED(d->workspace, 3),
       "keys / values / workspace alignment");
  return check(launch_sort_pairs(*d, (hipStream_t)stream), "sort_pairs");
}
int sslcr_rank_keys(const sslcr_rank_keys_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->n >= 1, "n < 1");
  NEED(d->C >= 1 && d->C <= 65535, "C outside [1, 65535]");
  NEED(d->scores && d->target && d->keys && d->values && d->nan, "null tensor");
  NEED(ALIGNED(d->scores, 3) && ALIGNED(d->keys, 3) && ALIGNED(d->values, 3), "scores / keys / values alignment");
  NEED(ALIGNED(d->target, 7) && ALIGNED(d->positive, 7) && ALIGNED(d->nan, 7), "target / positive / nan alignment");
  return check(launch_rank_keys(*d, (hipStream_t)stream), "rank_keys");
}
size_t sslcr_auc_workspace_bytes(int C, int n) {
  if (C < 1 || C > 65535 || n < 1) return 0;
  return (size_t)C * (size_t)rank_tiles(n) * 8 * sizeof(int);
}
int sslcr_auc_counts(const sslcr_auc_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->n >= 1, "n < 1");
  NEED(d->C >= 1 && d->C <= 65535, "C outside [1, 65535]");
  NEED(d->keys && d->values && d->counts && d->work, "null tensor");
  NEED(ALIGNED(d->keys, 3) && ALIGNED(d->values, 3) && ALIGNED(d->work, 3), "keys / values / work alignment");
  NEED(ALIGNED(d->counts, 7) && ALIGNED(d->nan, 7), "counts / nan alignment");
  return check(launch_auc_counts(*d, (hipStream_t)stream), "auc_counts");
}
// ---- Pillow-exact resize (resample.hip).  The coefficient tables are host arithmetic: Pillow's precompute_coeffs and
// normalize_coeffs_8bpc (Resample.c) in plain double with the libm Pillow itself calls, in its order of operations.
namespace {
constexpr double RS_PI = 3.14159265358979323846;      // M_PI
double rs_box(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }
double rs_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
double rs_hamming(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * RS_PI;
  return sin(x) / x * (0.54f + 0.46f * cos(x));       // float32 constants, as Resample.c spells them
}
double rs_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
double rs_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * RS_PI;
  return sin(x) / x;
}
double rs_lanczos(double x) { return -3.0 <= x && x < 3.0 ? rs_sinc(x) * rs_sinc(x / 3) : 0.0; }
struct RsFilter { double (*f)(double); double support; };
bool rs_filter(int code, RsFilter* out) {
  switch (code) {
    case SSLCR_RESAMPLE_BOX: *out = {rs_box, 0.5}; return true;
    case SSLCR_RESAMPLE_BILINEAR: *out = {rs_bilinear, 1.0}; return true;
    case SSLCR_RESAMPLE_HAMMING: *out = {rs_hamming, 1.0}; return true;
    case SSLCR_RESAMPLE_BICUBIC: *out = {rs_bicubic, 2.0}; return true;
    case SSLCR_RESAMPLE_LANCZOS: *out = {rs_lanczos, 3.0}; return true;
  }
  return false;
}
}  // namespace
int sslcr_resample_ksize(double in0, double in1, int outSize, int filter) {
  RsFilter f;
  if (filter == SSLCR_RESAMPLE_NEAREST) return outSize >= 1 && in1 > in0 ? 1 : -1;
  if (!rs_filter(filter, &f) || outSize < 1 || !(in1 > in0)) return -1;
  double filterscale = (in1 - in0) / outSize;
  if (filterscale < 1.0) filterscale = 1.0;
  const double ks = 2.0 * ceil(f.support * filterscale) + 1;
  return ks < (double)(1 << 30) ? (int)ks : -1;
}
int sslcr_resample_table_ok(const int32_t* k, int outSize, int k_stride) {
  if (!k || outSize < 1 || k_stride < 1) return 0;
  const int64_t limit = ((int64_t)1 << 31) - ((int64_t)1 << 21);       // 255 * sum|k| + 2^21 < 2^31
  for (int xx = 0; xx < outSize; ++xx) {
    int64_t sum = 0;
    for (int x = 0; x < k_stride; ++x) {
      const int64_t v = k[(size_t)xx * k_stride + x];
      const int64_t m = v < 0 ? -v : v;
      if (m >= (int64_t)1 << 23) return 0;
      sum += m;
    }
    if (255 * sum >= limit) return 0;
  }
  return 1;
}
int sslcr_resample_coeffs(int inSize, double in0, double in1, int outSize, int filter, int32_t* k, int k_stride, int32_t* bounds) {
  NEED(k && bounds, "null table");
  NEED(inSize >= 1 && outSize >= 1, "empty axis");
  NEED(in0 >= 0.0 && in1 <= (double)inSize && in1 > in0, "box outside the image, or empty");
  const int ksize = sslcr_resample_ksize(in0, in1, outSize, filter);
  NEED(ksize >= 1, "unknown filter, or ksize >= 2^30");
  NEED(k_stride >= ksize, "k_stride < ksize");
  const double scale = (in1 - in0) / outSize;
  const size_t cells = (size_t)outSize * k_stride;
  int32_t* kk = new (std::nothrow) int32_t[cells]();
  int32_t* bb = new (std::nothrow) int32_t[(size_t)outSize * 2];
  double* w = new (std::nothrow) double[ksize];
  int rc = 0;
  if (!kk || !bb || !w) {
    rc = fail("sslcr_resample_coeffs: out of host memory");
  } else if (filter == SSLCR_RESAMPLE_NEAREST) {
    // Pillow's ImagingScaleAffine (Geometry.c): the source position is WALKED, xo += scale per output pixel from in0 + scale / 2,
    // and truncated.  The closed form floor(in0 + (xx + 0.5) * scale) rounds differently where scale is inexact (512 -> 257).
    double xo = in0 + scale * 0.5;
    for (int xx = 0; xx < outSize; ++xx, xo += scale) {
      bb[2 * xx] = xo < inSize - 1 ? (int)xo : inSize - 1;
      bb[2 * xx + 1] = 1;
      kk[(size_t)xx * k_stride] = 1 << 22;
    }
  } else {
    RsFilter f;
    rs_filter(filter, &f);
    double filterscale = scale;
    if (filterscale < 1.0) filterscale = 1.0;
    const double support = f.support * filterscale;
    const double ss = 1.0 / filterscale;
    for (int xx = 0; xx < outSize; ++xx) {
      const double center = in0 + (xx + 0.5) * scale;
      double ww = 0.0;
      int xmin = (int)(center - support + 0.5);
      if (xmin < 0) xmin = 0;
      int xmax = (int)(center + support + 0.5);
      if (xmax > inSize) xmax = inSize;
      xmax -= xmin;
      for (int x = 0; x < xmax; ++x) {
        w[x] = f.f((x + xmin - center + 0.5) * ss);
        ww += w[x];
      }
      for (int x = 0; x < xmax; ++x) {
        if (ww != 0.0) w[x] /= ww;
        kk[(size_t)xx * k_stride + x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << 22)) : (int)(0.5 + w[x] * (1 << 22));
      }
      bb[2 * xx] = xmin;
      bb[2 * xx + 1] = xmax;
    }
    if (!sslcr_resample_table_ok(kk, outSize, k_stride))
      rc = fail("sslcr_resample_coeffs: a row of the table has 255 * sum|k| + 2^21 >= 2^31 or a |k| >= 2^23: no int32 pass");
  }
  if (rc == 0) {
    memcpy(k, kk, cells * sizeof(int32_t));
    memcpy(bounds, bb, (size_t)outSize * 2 * sizeof(int32_t));
  }
  delete[] kk;
  delete[] bb;
  delete[] w;
  return rc;
}
int sslcr_resample_plan(const sslcr_resample_desc* d, sslcr_resample_plan_info* out) {
  NEED(d && out, "null");
  const char* why = resample_plan(*d, out);
  NEED(!why, why);
  return 0;
}
int sslcr_resample(const sslcr_resample_desc* d, void* stream) {
  NEED(d, "null descriptor");
  ResamplePlan p;
  const char* why = resample_plan(*d, &p);
  NEED(!why, why);
  if (d->N == 0) return 0;
  NEED(d->src && d->dst, "null tensor");
  NEED(ALIGNED(d->kx, 3) && ALIGNED(d->bx, 3) && ALIGNED(d->ky, 3) && ALIGNED(d->by, 3) && ALIGNED(d->table_index, 3), "table alignment");
  NEED(p.form != SSLCR_RESAMPLE_TWO_PASS || d->workspace, "the two-pass form needs a workspace (sslcr_resample_plan_info.workspace_bytes)");
  const uintptr_t s = reinterpret_cast<uintptr_t>(d->src), t = reinterpret_cast<uintptr_t>(d->dst);
  const size_t sb = (size_t)d->N * d->C * d->IH * d->IW, tb = (size_t)d->N * d->C * d->OH * d->OW;
  NEED(s + sb <= t || t + tb <= s, "src and dst overlap (out of place only)");
  return check(launch_resample(*d, p, (hipStream_t)stream), "resample");
}
// ---- k-NN feature probe (knn.hip)
int sslcr_knn_plan(int nq, int nb, int D, int k, int slices_hint, sslcr_knn_plan_info* out) {
  NEED(out, "null");
  const char* why = knn_plan(nq, nb, D, k, slices_hint, out);
  NEED(!why, why);
  return 0;
}
int sslcr_knn_topk(const sslcr_knn_desc* d, void* stream) {
  NEED(d, "null descriptor");
  KnnPlan p;
  const char* why = knn_plan(d->nq, d->nb, d->D, d->k, d->slices, &p);
  NEED(!why, why);
  NEED(d->nb_valid >= 0 && d->nb_valid <= d->nb, "nb_valid outside [0, nb]");
  NEED(d->self_offset >= -1, "self_offset < -1");
  if (d->nq == 0) return 0;
  NEED(d->queries && d->bank && d->scores && d->indices && d->workspace, "null tensor");
  NEED(ALIGNED(d->queries, 15) && ALIGNED(d->bank, 15), "queries / bank must be 16-byte aligned");
  NEED(ALIGNED(d->workspace, 7) && ALIGNED(d->scores, 3) && ALIGNED(d->indices, 3), "workspace / scores / indices alignment");
  return check(launch_knn_topk(*d, p, (hipStream_t)stream), "knn_topk");
}
int sslcr_l2_normalize(const float* x, float* y, int n, int D, float eps, void* stream) {
  NEED(n >= 0 && D >= 1, "n >= 0 and D >= 1");
  NEED(eps >= 0.f, "eps must be >= 0");
  if (n == 0) return 0;
  NEED(x && y, "null tensor");
  NEED(ALIGNED(x, 3) && ALIGNED(y, 3), "x / y alignment");
  return check(launch_l2_normalize(x, y, n, D, eps, (hipStream_t)stream), "l2_normalize");
}
int sslcr_knn_vote(const sslcr_knn_vote_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->nq >= 0 && d->nb >= 1, "nq >= 0 and nb >= 1");
  NEED(d->k >= 1 && d->k <= SSLCR_KNN_MAX_K, "k outside [1, 64]");
  NEED(d->mode == SSLCR_KNN_VOTE_UNIFORM || d->mode == SSLCR_KNN_VOTE_SOFTMAX || d->mode == SSLCR_KNN_VOTE_REGRESS, "mode outside {0, 1, 2}");
  if (d->mode == SSLCR_KNN_VOTE_REGRESS) {
    NEED(!d->confusion, "the regression mode has no confusion counts");
  } else {
    NEED(d->C >= 1 && d->C <= 64, "C outside [1, 64]");
    NEED(d->mode != SSLCR_KNN_VOTE_SOFTMAX || d->temperature > 0.f, "temperature must be > 0");
    NEED(!d->confusion || d->query_labels, "confusion needs query_labels");
  }
  if (d->nq == 0) return 0;
  NEED(d->indices, "null indices");
  if (d->mode == SSLCR_KNN_VOTE_REGRESS) NEED(d->targets && d->pred_value, "the regression mode needs targets and pred_value");
  else NEED(d->labels && d->pred && d->votes, "classification needs labels, pred and votes");
  NEED(d->mode != SSLCR_KNN_VOTE_SOFTMAX || d->scores, "the softmax vote needs scores");
  NEED(ALIGNED(d->indices, 3) && ALIGNED(d->scores, 3) && ALIGNED(d->targets, 3) && ALIGNED(d->pred_value, 3) && ALIGNED(d->votes, 3),
       "indices / scores / targets / pred_value / votes alignment");
  NEED(ALIGNED(d->labels, 7) && ALIGNED(d->query_labels, 7) && ALIGNED(d->pred, 7) && ALIGNED(d->confusion, 7),
       "labels / query_labels / pred / confusion alignment");
  return check(launch_knn_vote(*d, (hipStream_t)stream), "knn_vote");
}
// ---- t-SNE embedding (tsne.hip)
int sslcr_tsne_plan(int n, int slices_hint, sslcr_tsne_plan_info* out) {
  NEED(out, "null");
  const char* why = tsne_plan(n, slices_hint, out);
  NEED(!why, why);
  return 0;
}
int sslcr_tsne_pair_dist2(const float* x, const int32_t* indices, float* dist2, int n, int D, int k, void* stream) {
  NEED(n >= 2 && n <= SSLCR_TSNE_MAX_N, "n outside [2, 2^20]");
  NEED(D >= 1, "D < 1");
  NEED(k >= 1 && k <= SSLCR_KNN_MAX_K, "k outside [1, 64]");
  NEED(x && indices && dist2, "null tensor");
  NEED(ALIGNED(x, 3) && ALIGNED(indices, 3) && ALIGNED(dist2, 3), "x / indices / dist2 alignment");
  return check(launch_tsne_pair_dist2(x, indices, dist2, n, D, k, (hipStream_t)stream), "tsne_pair_dist2");
}
int sslcr_tsne_affinities(const float* dist2, float* P, double* beta, int n, int k, float perplexity, void* stream) {
  NEED(n >= 2 && n <= SSLCR_TSNE_MAX_N, "n outside [2, 2^20]");
  NEED(k >= 1 && k <= SSLCR_KNN_MAX_K, "k outside [1, 64]");
  NEED(perplexity > 0.f, "perplexity must be > 0");
  NEED(dist2 && P && beta, "null tensor");
  NEED(ALIGNED(dist2, 3) && ALIGNED(P, 3) && ALIGNED(beta, 7), "dist2 / P / beta alignment");
  return check(launch_tsne_affinities(dist2, P, beta, n, k, perplexity, (hipStream_t)stream), "tsne_affinities");
}
static int tsne_grad_ok(const sslcr_tsne_grad_desc* d, TsnePlan* p, bool update) {
  NEED(d, "null descriptor");
  const char* why = tsne_plan(d->n, d->slices, p);
  NEED(!why, why);
  NEED(d->y && d->workspace && d->Z, "null tensor");
  NEED(ALIGNED(d->y, 7) && ALIGNED(d->workspace, 15) && ALIGNED(d->Z, 7), "y / workspace / Z alignment");
  if (!update) return 0;
  NEED(d->grad && d->rowptr && d->col && d->val, "null tensor");
  NEED(d->nnz >= 0, "nnz < 0");
  NEED(ALIGNED(d->grad, 7) && ALIGNED(d->rowptr, 3) && ALIGNED(d->col, 3) && ALIGNED(d->val, 3) && ALIGNED(d->kl_rows, 7),
       "grad / rowptr / col / val / kl_rows alignment");
  if (d->y_out) {
    NEED(d->y_out != d->y, "y_out == y (other rows still read y)");
    NEED(d->update && d->gains, "null tensor");
    NEED(ALIGNED(d->y_out, 7) && ALIGNED(d->update, 7) && ALIGNED(d->gains, 7), "y_out / update / gains alignment");
  }
  return 0;
}
int sslcr_tsne_repulsion(const sslcr_tsne_grad_desc* d, void* stream) {
  TsnePlan p;
  if (tsne_grad_ok(d, &p, false)) return -1;
  return check(launch_tsne_repulsion(*d, p, (hipStream_t)stream), "tsne_repulsion");
}
int sslcr_tsne_update(const sslcr_tsne_grad_desc* d, void* stream) {
  TsnePlan p;
  if (tsne_grad_ok(d, &p, true)) return -1;
  return check(launch_tsne_update(*d, p, (hipStream_t)stream), "tsne_update");
}
int sslcr_tsne_kl(const double* kl_rows, const float* grad, const double* Z, double* log_row, int n, int iteration, void* stream) {
  NEED(n >= 2 && n <= SSLCR_TSNE_MAX_N, "n outside [2, 2^20]");
  NEED(kl_rows && grad && Z && log_row, "null tensor");
  NEED(ALIGNED(kl_rows, 7) && ALIGNED(grad, 3) && ALIGNED(Z, 7) && ALIGNED(log_row, 7), "kl_rows / grad / Z / log_row alignment");
  return check(launch_tsne_kl(kl_rows, grad, Z, log_row, n, iteration, (hipStream_t)stream), "tsne_kl");
}
// ---- linear probe (linprobe.hip)
int sslcr_linprobe_plan(int n, int D, int C, int loss, int groups_hint, sslcr_linprobe_plan_info* out) {
  NEED(out, "null");
  const char* why = linprobe_plan(n, D, C, loss, groups_hint, out);
  NEED(!why, why);
  return 0;
}
static int linprobe_ok(const char* func, const sslcr_linprobe_desc* d, LinprobePlan* p, bool fwd_only) {
#define LP_NEED(cond, what) \
  do {                      \
    if (!(cond)) return fail("%s: invalid argument (%s)", func, what); \
  } while (0)
#define LP_NEED_AL(p, n) LP_NEED(ALIGNED(p, (n) - 1), #p " must be " #n "-byte aligned")
  LP_NEED(d, "null descriptor");
  const char* why = linprobe_plan(d->n, d->D, d->C, fwd_only ? SSLCR_LINPROBE_SOFTMAX : d->loss, d->groups, p);
  LP_NEED(!why, why);
  LP_NEED(d->x && d->w && d->b && d->workspace, "null tensor");
  if (fwd_only) {
    LP_NEED(d->logits, "null logits");
  } else {
    LP_NEED(d->value && d->grad, "null value / grad");
    LP_NEED(d->loss != SSLCR_LINPROBE_SOFTMAX || d->labels, "the softmax loss needs labels");
    LP_NEED(d->loss != SSLCR_LINPROBE_SQUARED || d->targets, "the squared loss needs targets");
  }
  LP_NEED_AL(d->x, 16); LP_NEED_AL(d->workspace, 16);
  LP_NEED_AL(d->w, 4); LP_NEED_AL(d->b, 4); LP_NEED_AL(d->logits, 4);
  if (!fwd_only) {                                  // (sslcr_linprobe_logits does not read these fields)
    LP_NEED_AL(d->labels, 8); LP_NEED_AL(d->value, 8); LP_NEED_AL(d->grad, 8);
    LP_NEED_AL(d->targets, 4); LP_NEED_AL(d->sample_weight, 4);
  }
#undef LP_NEED_AL
#undef LP_NEED
  return 0;
}
int sslcr_linprobe_eval(const sslcr_linprobe_desc* d, void* stream) {
  LinprobePlan p;
  if (linprobe_ok(__func__, d, &p, false)) return -1;
  return check(launch_linprobe(*d, p, false, (hipStream_t)stream), "linprobe_eval");
}
int sslcr_linprobe_logits(const sslcr_linprobe_desc* d, void* stream) {
  LinprobePlan p;
  if (linprobe_ok(__func__, d, &p, true)) return -1;
  return check(launch_linprobe(*d, p, true, (hipStream_t)stream), "linprobe_logits");
}
#undef SQ_SHAPE_OK
#undef MAP_SHAPE_OK
int sslcr_d4_transform(const sslcr_d4_desc* d, void* stream) {
  NEED(d, "null descriptor");
  NEED(d->N >= 0 && d->Cn >= 1 && d->H >= 1, "N >= 0, Cn >= 1 and H >= 1");
  NEED(d->H == d->W, "tiles must be square (H == W)");
  NEED(d->elem_bytes == 1 || d->elem_bytes == 4, "elem_bytes outside {1, 4}");
  if (d->N == 0) return 0;
  NEED(d->src && d->dst && d->orient, "null tensor");
  const uintptr_t s = reinterpret_cast<uintptr_t>(d->src), t = reinterpret_cast<uintptr_t>(d->dst);
  NEED((reinterpret_cast<uintptr_t>(d->orient) & 3) == 0, "orient alignment");
  NEED(d->elem_bytes == 1 || ((s | t) & 3) == 0, "a 4-byte batch must be 4-byte aligned");
  const size_t bytes = (size_t)d->N * d->Cn * d->H * d->W * d->elem_bytes;
  NEED(s + bytes <= t || t + bytes <= s, "src and dst overlap (out of place only)");
  return check(launch_d4_transform(*d, (hipStream_t)stream), "d4_transform");
}

int sslcr_optimizer_step(const sslcr_tensor_desc* device_descs, int ntensors, int max_n, const sslcr_opt_desc* o, void* stream) {
  return sslcr_optimizer_step_groups(device_descs, ntensors, max_n, o, 1, nullptr, stream);
}
int sslcr_optimizer_step_groups(const sslcr_tensor_desc* device_descs, int ntensors, int max_n, const sslcr_opt_desc* groups, int ngroups,
                                const float* coef_dev, void* stream) {
  NEED(device_descs && groups && ntensors > 0 && max_n > 0, "args");
  NEED_AL(device_descs, 8); NEED_AL(coef_dev, 4);      // (the tensors the table names live behind a device pointer: stated, not checked)
  NEED(ngroups >= 1 && ngroups <= SSLCR_MAX_OPT_GROUPS, "ngroups must be 1..8");
  OptTable tab = opt_table_noop();
  for (int i = 0; i < ngroups; ++i) {
    NEED(groups[i].kind >= 0 && groups[i].kind <= 2, "kind");
    tab.row[i] = groups[i];
  }
  return check(launch_optimizer(device_descs, ntensors, max_n, tab, coef_dev, (hipStream_t)stream), "optimizer_step");
}
int sslcr_grad_norm_partials(void) { return GRAD_NORM_BLOCKS; }
int sslcr_grad_norm(const float* g, size_t n, float max_norm, double* partials, float* out2, void* stream) {
  NEED(partials && out2 && (g || n == 0), "null");
  NEED((reinterpret_cast<uintptr_t>(g) & 3) == 0 && (reinterpret_cast<uintptr_t>(partials) & 7) == 0, "alignment");
  NEED(!(max_norm < 0.f), "max_norm");
  return check(launch_grad_norm(g, n, max_norm, partials, out2, (hipStream_t)stream), "grad_norm");
}
int sslcr_grad_accumulate(float* dst, const float* src, size_t n, void* stream) {
  NEED((dst && src) || n == 0, "null");
  NEED((reinterpret_cast<uintptr_t>(dst) & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0, "alignment");
  return check(launch_grad_accumulate(dst, src, n, (hipStream_t)stream), "grad_accumulate");
}
int sslcr_axpby(float* p, float* q, size_t n, float alpha, int copy_back, void* stream) {
  NEED(p && q, "null");
  return check(launch_axpby(p, q, n, alpha, copy_back, (hipStream_t)stream), "axpby");
}
int sslcr_fill(float* p, size_t n, float v, void* stream) {
  NEED(p, "null");
  return check(launch_fill(p, n, v, (hipStream_t)stream), "fill");
}
int sslcr_pack_conv(int dtype, const sslcr_pack_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->w && (d->w_fwd || d->w_dgrad), "null");
  return check(launch_pack_conv(dtype, *d, (hipStream_t)stream), "pack_conv");
}
int sslcr_weak_augment(const sslcr_weak_aug_desc* d, void* stream) {
  NEED(d && d->src && d->dst && d->params, "null");
  NEED(d->N > 0 && d->OH > 0 && d->OW > 0 && d->OH <= d->SH && d->OW <= d->SW, "crop larger than the source");
  return check(launch_weak_augment(*d, (hipStream_t)stream), "weak_augment");
}
int sslcr_hed_colour_augment(const sslcr_colour_aug_desc* d, void* stream) {
  NEED(d && d->src && d->dst && d->shift, "null");
  NEED(d->N > 0 && d->H > 0 && d->W > 0, "empty batch");
  return check(launch_hed_colour(*d, (hipStream_t)stream), "hed_colour_augment");
}
int sslcr_brightness_contrast(const sslcr_brightness_contrast_desc* d, void* stream) {
  NEED(d && d->src && d->dst && d->alpha_beta && d->stats, "null");
  NEED(d->N > 0 && d->H > 0 && d->W > 0, "empty batch");
  return check(launch_brightness_contrast(*d, (hipStream_t)stream), "brightness_contrast");
}
int sslcr_randaug_v2_slot(const sslcr_augv2_desc* d, void* stream) {
  NEED(d && d->src && d->dst && d->op, "null");
  NEED(d->src != d->dst, "dst aliases src");
  NEED(d->N > 0 && d->N <= 65535 && d->H > 0 && d->W > 0 && d->H <= 16384 && d->W <= 16384, "batch shape");
  const unsigned m = d->ops_mask;
  NEED(m < (1u << (SSLCR_AUGV2_BICUBIC + 1)), "ops_mask names an unknown op");
  const unsigned stats = 1u << SSLCR_AUGV2_CONTRAST | 1u << SSLCR_AUGV2_AUTOCONTRAST | 1u << SSLCR_AUGV2_EQUALIZE;
  const unsigned enhance = 1u << SSLCR_AUGV2_BRIGHTNESS | 1u << SSLCR_AUGV2_CONTRAST | 1u << SSLCR_AUGV2_COLOR | 1u << SSLCR_AUGV2_SHARPNESS;
  NEED(!(m & stats) || (d->hist && d->lsum), "hist / lsum workspace");
  NEED(!(m & (stats | 1u << SSLCR_AUGV2_BRIGHTNESS)) || d->lut, "lut workspace");
  NEED(!(m & enhance) || d->factor, "factor");
  NEED(!(m & 1u << SSLCR_AUGV2_NEAREST_FIXED) || d->fixed, "fixed");
  NEED(!(m & 1u << SSLCR_AUGV2_NEAREST_TABLE) || (d->shift && d->tab), "shift / tab workspace");
  NEED(!(m & 1u << SSLCR_AUGV2_BICUBIC) || d->affine, "affine");
  return check(launch_augv2(*d, (hipStream_t)stream), "randaug_v2_slot");
}
int sslcr_randaug_v2_colour(const sslcr_augv2_colour_desc* d, void* stream) {
  NEED(d && d->img && d->op, "null");
  NEED(d->param, "param");
  NEED(d->N > 0 && d->N <= 65535 && d->H > 0 && d->W > 0 && d->H <= 16384 && d->W <= 16384, "batch shape");
  NEED(d->ops_mask < (1u << (SSLCR_AUGV2C_HSV + 1)), "ops_mask names an unknown op");
  NEED(!(d->ops_mask & 1u << SSLCR_AUGV2C_HED) || d->bsum, "bsum workspace");
  NEED(!(d->ops_mask & 1u << SSLCR_AUGV2C_HED) || (reinterpret_cast<uintptr_t>(d->bsum) & 7) == 0, "bsum alignment");
  NEED((reinterpret_cast<uintptr_t>(d->param) & 7) == 0 && (reinterpret_cast<uintptr_t>(d->op) & 3) == 0, "alignment");
  NEED(d->cutoff_lo <= d->cutoff_hi, "cutoff range");
  return check(launch_augv2_colour(*d, (hipStream_t)stream), "randaug_v2_colour");
}
int sslcr_randaug_v1_slot(const sslcr_augv1_desc* d, void* stream) {
  NEED(d && d->src && d->dst && d->op, "null");
  NEED(d->src != d->dst, "dst aliases src");
  NEED(d->N > 0 && d->N <= 65535 && d->H > 0 && d->W > 0 && d->H <= 16384 && d->W <= 16384, "batch shape");
  const unsigned m = d->ops_mask;
  NEED(m < (1u << (SSLCR_AUGV1_NOISE + 1)), "ops_mask names an unknown op");
  NEED(!(m & ~(1u << SSLCR_AUGV1_COPY)) || d->iparam, "iparam");
  NEED(!(m & (1u << SSLCR_AUGV1_WARP | 1u << SSLCR_AUGV1_NOISE)) || d->dparam, "dparam");
  NEED(!(m & 1u << SSLCR_AUGV1_WARP) || d->wtab, "wtab");
  NEED(!(m & 1u << SSLCR_AUGV1_RESIZE) || (d->work && d->work_smax >= 1 && d->work_smax <= 32768), "resize workspace");
  NEED(!(m & 1u << SSLCR_AUGV1_RESIZE) || d->H == d->W, "Scale_Resize_Crop needs H == W");
  NEED((reinterpret_cast<uintptr_t>(d->op) & 3) == 0 && (reinterpret_cast<uintptr_t>(d->iparam) & 3) == 0 &&
       (reinterpret_cast<uintptr_t>(d->dparam) & 7) == 0 && (reinterpret_cast<uintptr_t>(d->wtab) & 15) == 0 &&
       (reinterpret_cast<uintptr_t>(d->work) & 15) == 0, "alignment");
  return check(launch_augv1(*d, (hipStream_t)stream), "randaug_v1_slot");
}
int sslcr_cv_warp_table(int16_t* table) {
  NEED(table, "null");
  cv_warp_table(table);
  return 0;
}
size_t sslcr_augv1_workspace_bytes(int N, int S, double max_scale) {
  if (N <= 0 || S <= 0 || S > 16384 || !(max_scale > 0.0) || !(max_scale <= 2.0)) return 0;
  const int smax = (int)(S * max_scale);
  return smax < 1 ? 0 : (size_t)N * augv1_work_stride(smax);
}
int sslcr_augv1_philox(unsigned long long seed, uint32_t first, int count, uint32_t* words, void* stream) {
  NEED(words, "null");
  NEED(count > 0 && count <= (1 << 24), "count");
  NEED((reinterpret_cast<uintptr_t>(words) & 15) == 0, "alignment");
  return check(launch_augv1_philox(seed, first, count, words, (hipStream_t)stream), "augv1_philox");
}
int sslcr_pack_stem(int dtype, const sslcr_pack_desc* d, void* stream) {
  DT_OK(dtype);
  NEED(d && d->w && d->w_fwd && d->K == 64 && d->C == 3 && d->R == 7 && d->S == 7, "stem shape");
  return check(launch_pack_stem(dtype, *d, (hipStream_t)stream), "pack_stem");
}

}  // extern "C"
