/* sslcr.h -- C ABI of the MI355X (gfx950) engine for the SSL_CR_Histo ResNet18 step path.
 *
 * The reference (srinidhiPY/SSL_CR_Histo) is pure Python on torch/cuDNN and has NO FFI of its own; the seam
 * this library plugs into is "the torch ops behind models/net.py + the step body of train()/validate()".
 * Each entry point below names the reference code it replaces.  Conventions:
 *   - return 0 on success, negative on error; sslcr_last_error() gives the message (thread local);
 *     no C++ exception crosses this boundary;
 *   - every pointer is a DEVICE pointer owned by the caller unless stated otherwise; the engine never frees it;
 *   - `stream` is the caller's hipStream_t (torch.cuda.current_stream().cuda_stream); all calls are asynchronous;
 *   - activations are NHWC, conv weights [K][R][S][C] ("KRSC"), dtype 0 = fp32 (exact-parity mode,
 *     v_mfma_f32_16x16x4_f32), 1 = bf16 storage with fp32 accumulate (v_mfma_f32_16x16x32_bf16);
 *   - one sslcr_ctx per process per device, not thread safe (single training thread, like the reference);
 *   - alignment: a comment "Alignment (owner): names N-byte aligned; ..." states, for every pointer of a descriptor or of a
 *     prototype, the least alignment of the address the caller may pass: the widest access a kernel makes through it.  A pointer
 *     below it is an error decided before any launch (-1, the message names the pointer); NULL, where allowed, passes.  A contiguous
 *     view into a larger allocation is fine as long as ITS first byte is aligned (tests/test_arena_gpu.py runs the training
 *     kernels at exactly these alignments and at no multiple of twice them).
 */
#ifndef SSLCR_H_
#define SSLCR_H_
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* the library is built with -fvisibility=hidden: exactly the entry points declared between this push and the pop at the end of
 * the file are exported (tests/test_abi_cpu.py compares `nm -D` with this header) */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define SSLCR_F32 0
#define SSLCR_BF16 1
#define SSLCR_FP8 2   /* engine mode only (sslcr_create): bf16 storage and backward, fp8 e4m3 forward for the eligible 3x3 convs */

/* the library round (16 here). ABI notes below name the version a behaviour changed in: 4 = sslcr_bn_bwd_reduce overwrites its sums;
 * 7 = sslcr_randaug_v2_slot added (nothing else changed); 8 = optimizer parameter groups, AdamW and the global gradient norm
 * (sslcr_tensor_desc.group, sslcr_opt_desc.kind 2, sslcr_optimizer_step_groups, sslcr_grad_norm, sslcr_net_optimizer_step_groups,
 * sslcr_net_grad_norm: all additive); 9 = gradient accumulation (sslcr_grad_accumulate, sslcr_net_set_grad_accumulate: additive,
 * off by default); 10 = loss options (sslcr_loss_opts, sslcr_loss_ex, sslcr_ce_denominator, sslcr_net_set_loss_opts: additive, the
 * defaults issue the launches of version 9); 11 = sslcr_randaug_v2_colour added (the hed / hsv ops of the v2 pool; additive,
 * sslcr_augv2_desc and sslcr_randaug_v2_slot are unchanged); 12 = device-resident inference: sslcr_wsi_gather and sslcr_predict added
 * (additive; sslcr_softmax_col keeps its launch and its bits); 13 = test-time augmentation over D4: sslcr_d4_transform,
 * sslcr_wsi_gather_d4 and sslcr_predict_tta added (additive; sslcr_wsi_gather, sslcr_predict and their descriptors keep their launches
 * and their bits); 14 = tile mining for RSP pretraining: sslcr_tissue_bits, sslcr_lab_a_sum, sslcr_tile_popcount and sslcr_rsp_gather
 * added (additive; no existing entry, descriptor or launch changes); 15 = Camelyon16 annotations: sslcr_points_in_polygons and
 * sslcr_map_confusion added (additive; no existing entry, descriptor or launch changes).  Lesion scoring (sslcr_label_components,
 * sslcr_gaussian_smooth, sslcr_nms_candidates / _rounds / _collect, sslcr_lesion_hits) is additive in the same way and came WITHOUT
 * a new number (the tests of that time held sslcr_version() to 15 by equality), so a caller tests for these entries by symbol.
 * The same holds for sslcr_conv2d_fp8_kernel_name and sslcr_fp8_scale_update (additive; the launches they name or issue are the
 * ones sslcr_conv2d_fp8 and the engine's forward issued before); sslcr_conv2d_fp8 now refuses in_scale without in_shift, a
 * descriptor whose launch read a NULL pointer on the device.  The ranking entries (sslcr_sort_pairs, sslcr_sort_workspace_bytes,
 * sslcr_rank_keys, sslcr_auc_counts, sslcr_auc_workspace_bytes) are additive in the same way, again without a new number, and so
 * are the resize entries (sslcr_resample, sslcr_resample_plan, sslcr_resample_coeffs, sslcr_resample_ksize,
 * sslcr_resample_table_ok), the k-NN probe's (sslcr_knn_plan, sslcr_knn_topk, sslcr_knn_vote, sslcr_l2_normalize) and the t-SNE
 * embedding's (sslcr_tsne_plan, sslcr_tsne_pair_dist2, sslcr_tsne_affinities, sslcr_tsne_repulsion, sslcr_tsne_update, sslcr_tsne_kl) and the linear probe's
 * (sslcr_linprobe_plan, sslcr_linprobe_eval, sslcr_linprobe_logits).
 * 16 = the switch listing: sslcr_switch_count and sslcr_switch_info added (additive; every switch keeps its default and its reading of
 * every string, no launch changes). */
int sslcr_version(void);
const char* sslcr_last_error(void);

/* ---- environment switches (library version >= 16).  The library reads the SSLCR_* variables below and no others; they exist for
 * same-box A/B measurements and for tests, and every default is the measured better form.  One row each:
 *
 *   name                    rule     when     group        default
 *   SSLCR_PP64              ATOI     process  routing      1
 *   SSLCR_H16_TW8           ATOI     process  routing      1
 *   SSLCR_H16_RAW           ATOI     process  routing      1
 *   SSLCR_S2                ATOI     process  routing      1
 *   SSLCR_S2D               ATOI     process  routing      1
 *   SSLCR_S2W               ATOI     process  routing      1
 *   SSLCR_WG_DMA            ATOI     process  routing      1
 *   SSLCR_WGRAD_WIDE        LEAD0    process  routing      1
 *   SSLCR_GEMM_LDS          ATOI     process  form         1
 *   SSLCR_STEM_POOL_FORM    INT      process  form         2
 *   SSLCR_POOL_BANDS        ATOI     process  form         0
 *   SSLCR_WG_STAGGER        INT      process  form         1
 *   SSLCR_SEGMENTS          LEAD0    process  engine       1
 *   SSLCR_BN_PAIR           ATOI     process  engine       1
 *   SSLCR_BN_PAIR_G         ATOI     process  engine       1
 *   SSLCR_YBITS             ATOI     process  engine       1
 *   SSLCR_UNFOLD_EVAL       ATOI     process  engine       1
 *   SSLCR_STEM_POOL         ATOI     process  engine       1
 *   SSLCR_BN_ONE_LAUNCH     ATOI     process  engine       0
 *   SSLCR_FUSE_STEM_BWD     ATOI     call     engine       1
 *   SSLCR_COMM_SELFTEST     PRESENT  call     engine       0
 *   SSLCR_BN_REPEAT         INT      process  measurement  1
 *   SSLCR_EW_CAP            INT      process  measurement  0
 *
 * rule, for a variable that is set (unset is the default under every rule):
 *   ATOI     on where atoi(value) != 0: "", "off" and " 0" turn the switch OFF; "01", "2" and "-1" leave it on
 *   LEAD0    off only where the first character is '0': "", "off" and " 0" leave the switch ON; "00" and "01" turn it off
 *   INT      atoi(value); SSLCR_BN_REPEAT below 1 becomes 1; SSLCR_EW_CAP is read with strtol and held to [256, 65535], and its
 *            default 0 stands for "not set": three workgroups per compute unit, which needs the device
 *   PRESENT  on where the variable is set at all, the empty string included
 * when: `process` rows are read once per process, thread-safely, at the first query of any switch (the first entry point that
 *   routes, launches or lists) -- a later putenv is not seen; `call` rows are read at every call of the entry point their meaning
 *   names (sslcr_create, sslcr_comm_init).
 * group: routing = changes which kernel instance the router answers (sslcr_conv2d_kernel_name, sslcr_conv2d_wgrad_kernel_name);
 *   form = another form of a kernel under the same routed name; engine = a decision of the step path; measurement = NOT for a run
 *   whose results are kept (SSLCR_BN_REPEAT=n updates the running statistics n times).
 * sslcr_switch_info gives each row's one-line meaning and what this process read; it needs no device. */
typedef struct sslcr_switch_row {
  const char* name;       /* with its prefix, "SSLCR_PP64"; all five strings are static */
  const char* group;      /* "routing" | "form" | "engine" | "measurement" */
  const char* rule;       /* "ATOI" | "LEAD0" | "INT" | "PRESENT" */
  const char* when;       /* "process" | "call" */
  const char* meaning;
  long long dflt;         /* the value in use where the variable is not set (0 / 1 for the on / off rules) */
  long long value;        /* the value in use: dflt where is_set == 0 */
  int is_set;
} sslcr_switch_row;
int sslcr_switch_count(void);
int sslcr_switch_info(int i, sslcr_switch_row* out);      /* 0 <= i < sslcr_switch_count(); -1 otherwise */

/* ---- conv2d forward / dgrad (replaces nn.Conv2d inside torchvision resnet18: models/net.py:32,77;
 *      BasicBlock convs K2-K4 of SURVEY 2b, and their autograd dgrad K13) */
typedef struct sslcr_conv_desc {
  const void* x;          /* gathered tensor, NHWC [N][H][W][C] */
  const void* w;          /* [K][R][S][C] */
  void* y;                /* NHWC [N][OH][OW][K] */
  const float* in_scale;  /* [C] or NULL: prologue x*scale+shift (+relu) on in-bounds pixels (producer BN fused in the load) */
  const float* in_shift;
  const float* bias;      /* [K] or NULL */
  const void* residual;   /* like y, or NULL */
  float* stats;           /* [sslcr_conv2d_partial_rows][2][K] fp32 or NULL: per-channel (sum, sumsq) partials */
  int N, H, W, C, K, R, S, stride, pad;
  int PH, PW;             /* pixel space the GEMM M dimension enumerates */
  int OH, OW, osh;        /* physical output dims; pixel (ph,pw) is stored at (ph*osh, pw*osh) */
  int transposed;         /* 0: src = p*stride-pad+r ; 1 (dgrad): src = (p+pad-r)/stride when divisible */
  int in_relu, relu, accumulate;
  int pix_mul, pix_off_h, pix_off_w;   /* sub-lattice of the pixel space: pixel (i,j) of the PH x PW grid is (i*mul+off_h, j*mul+off_w);
                                          mul = 0 means 1.  With tap_mask this runs ONE parity class of a strided dgrad */
  unsigned tap_mask;                   /* bit (r*S+s) set = visit that tap; 0 = all taps */
  /* BatchNorm-backward front end of a dgrad (optional; needs stats, excludes in_scale / bias / residual / relu; 3x3 stride 1 on
     16x16-tileable maps only -- sslcr_conv2d fails otherwise).  y is the gradient w.r.t. relu(bn(mask_x)); with these set the
     kernel writes g = y * (mask_scale[k]*mask_x + mask_shift[k] > 0) instead of y, and the stats rows hold
     (sum g, sum g*(mask_x - mask_mean[k])) -- the two sums of sslcr_bn_bwd_reduce -- instead of (sum y, sum y^2): the reduce
     pass over (dy, x) of that BatchNorm is not needed. */
  const void* mask_x; const float* mask_scale; const float* mask_shift; const float* mask_mean;
  int par4;               /* stride-2 3x3 pad-1 dgrad (transposed = 1, pix_mul = 2, PH x PW = the even-sized input / 2): all four
                             output-parity classes in ONE launch (class = grid z; offsets and tap subsets derived in the kernel)
                             instead of four launches with pix_off / tap_mask.  DMA-gather kernel shapes only. */
  /* Segments (models/net.py:50-66, TripletNet: three branches through ONE backbone, BatchNorm statistics per branch): with
     seg_images > 0 the N images are N / seg_images independent batches in one launch -- segment s reads its prologue from
     in_scale + s * seg_stride / in_shift + s * seg_stride, and the stats rows of segment s are rows
     [s * rows / nseg, (s + 1) * rows / nseg) of sslcr_conv2d_partial_rows (no workgroup's rows mix segments).  With mask_x the
     segment's BatchNorm is mask_scale / mask_shift / mask_mean + s * seg_stride.  bf16 only; sslcr_conv2d fails where the kernel
     serving the shape has no segment form (sslcr_conv2d_segments_ok). */
  int seg_images, seg_stride;
  /* library version >= 6.  [K] or NULL: y = epilogue(acc * out_scale[k] + bias[k] ...) -- eval-mode BatchNorm with its scale kept OUT
     of the filters: w is then the plain (bf16-rounded) filter, bias the BatchNorm shift (sslcr_pack_desc.scale_out).  The bf16 engine
     runs the teacher / validate() forward this way: round(w) followed by the fp32 scale leaves 3.6 x less SYSTEMATIC error in the
     logits than round(w * scale), and the consistency loss -- an average over the unlabeled batch -- keeps exactly that part
     (full-size iteration: 1.75e-3 -> 4.9e-4, tools/bf16_teacher_fold_experiment.py, profiles/r06_bf16_teacher_fold_experiment.txt).
     Only with bias (the eval forms); not with stats / mask_x. */
  const float* out_scale;
  /* Alignment (sslcr_conv_desc): x, w, y, residual, mask_x, bias, stats, out_scale 16-byte aligned (16-byte vector loads / stores and
     16-byte lanes of buffer_load ... lds; bias, out_scale and the stats rows as float4); in_scale, in_shift, mask_scale, mask_shift,
     mask_mean 4-byte aligned (scalar loads).  Errors of sslcr_conv2d, sslcr_conv2d_s2_pair (both descriptors) and sslcr_conv2d_fp8:
     a pointer below its alignment. */
} sslcr_conv_desc;
int sslcr_conv2d(int dtype, const sslcr_conv_desc* d, void* stream);
int sslcr_conv2d_partial_rows(const sslcr_conv_desc* d);                /* -1: d is NULL, or no segment fits (seg_images > N) */
int sslcr_conv2d_segments_ok(int dtype, const sslcr_conv_desc* d);      /* 1: this descriptor's seg_images is served */
/* name of the kernel instance sslcr_conv2d would launch for this descriptor, spelled as rocprofv3 prints it (static string;
   lets tests and profiles tie a shape to the code path that serves it) */
const char* sslcr_conv2d_kernel_name(int dtype, const sslcr_conv_desc* d);
/* A downsampling BasicBlock's two convolutions of ONE input in one launch (torchvision BasicBlock.forward: `out = self.conv1(x)` and
   `identity = self.downsample(x)` -- downsample[0] is the 1x1 / stride-2 projection -- of layer{2,3,4}[0], reached through
   models/net.py:32,77): c1 is the 3x3 / stride 2 / pad 1 descriptor, ds the 1x1 / stride 2 / pad 0 descriptor with the same x, N, H, W,
   C and K.  Both must be in the same mode: stats (train forward: raw output + BatchNorm partial rows, sslcr_conv2d_partial_rows(c1)
   rows each) or bias (eval forward with the BatchNorm folded; relu honoured per descriptor).  Served where
   sslcr_conv2d_s2_pair_ok returns 1 (bf16, 16x16-tileable OUTPUT maps, C % 64 == 0, K % 128 == 0, no prologue / residual); the
   results equal two sslcr_conv2d calls. */
int sslcr_conv2d_s2_pair(int dtype, const sslcr_conv_desc* c1, const sslcr_conv_desc* ds, void* stream);
int sslcr_conv2d_s2_pair_ok(int dtype, const sslcr_conv_desc* c1, const sslcr_conv_desc* ds);

/* ---- fp8 (OCP e4m3) forward conv path: BASELINE config 5, eval_Camelyon_SSL_CR.py:33-157 "fp8 MFMA conv path".
 *      Serves 3x3 / stride 1 / pad 1 convs with C % 128 == 0, K % 128 == 0 on 16x16-tileable maps (or 8x8 maps with N % 4 == 0):
 *      ResNet18 layers 2-4.  x / y / residual are bf16 NHWC exactly as in sslcr_conv2d(SSLCR_BF16, ...) (in_scale / in_shift /
 *      in_relu, bias, residual, relu, stats all honoured); the descriptor's `w` is ignored in favour of the e4m3 pack.
 *      Quantisation: activations x * x_scale clamped to +-448, round-to-nearest-even, on the way into LDS; weights
 *      w * w_scale[k] (power of two, amax -> (224, 448]) by sslcr_pack_conv_fp8; fp32 accumulate; result * w_dequant[k] / x_scale. */
typedef struct sslcr_fp8_desc {
  const uint8_t* w8;        /* [K][3][3][C] e4m3 */
  const float* w_dequant;   /* [K]: 1 / w_scale[k] */
  float x_scale;            /* per-tensor activation scale (> 0); 1 = activations used as they are (post-BatchNorm values sit in
                               e4m3's normal range [2^-6, 448]) */
  const float* x_scale_dev; /* optional device float: read instead of x_scale (delayed scaling without a host sync) */
  float* amax_out;          /* optional device float (>= 0 on entry): atomically raised to max |transformed activation| seen by this
                               launch, before scaling and clamping -- the engine turns it into the NEXT step's x_scale
                               (scale = 2^floor(log2(448 / (2 amax))): a factor 2 of headroom), the delayed-scaling recipe */
  /* Alignment (sslcr_fp8_desc): w8, w_dequant 16-byte aligned (LDS DMA lanes; the dequant scales as float4); x_scale_dev, amax_out
     4-byte aligned.  Errors of sslcr_conv2d_fp8: a pointer below its alignment. */
} sslcr_fp8_desc;
int sslcr_conv2d_fp8(const sslcr_conv_desc* d, const sslcr_fp8_desc* q, void* stream);
int sslcr_conv2d_fp8_partial_rows(const sslcr_conv_desc* d);      /* rows of d->stats the fp8 kernel writes; 0 = shape not served */
/* name of the kernel instance sslcr_conv2d_fp8 would launch for this descriptor, spelled as rocprofv3 prints it (static string);
   "" = shape not served */
const char* sslcr_conv2d_fp8_kernel_name(const sslcr_conv_desc* d);
/* delayed scaling, the update the engine runs between steps: slots [n][2] fp32 on the device = {x_scale, amax seen since the last
   update}.  Per slot: x_scale <- 2^floor(log2(224 / amax)) clamped to [2^-16, 2^16] where 0 < amax < 3e38 (left as it is for a zero,
   negative or non-finite amax), then amax <- 0. */
int sslcr_fp8_scale_update(float* slots, int n, void* stream);
typedef struct sslcr_pack_fp8_desc {
  const float* w;           /* [K][C][3][3] fp32 (PyTorch layout) */
  uint8_t* w8;              /* [K][3][3][C] e4m3 out */
  float* w_dequant;         /* [K] out */
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps; float* bias_out;   /* optional: fold BatchNorm (eval) */
  int K, C;
} sslcr_pack_fp8_desc;
int sslcr_pack_conv_fp8(const sslcr_pack_fp8_desc* d, void* stream);

/* ---- conv2d weight gradient (autograd wgrad of the same convs) */
typedef struct sslcr_wgrad_desc {
  const void* x;          /* conv input NHWC [N][H][W][C] (the raw producer output when in_scale != NULL) */
  const void* dy;         /* NHWC [N][OH][OW][K] */
  float* dw;              /* [K][R][S][C] fp32, ACCUMULATED into */
  const float* in_scale;
  const float* in_shift;
  int in_relu;
  int N, H, W, C, K, R, S, stride, pad, OH, OW;
  int seg_images;         /* optional (> 0, divides N; 3x3 stride-1 halo kernel shapes only): the batch is N / seg_images segments   */
  int seg_stride;         /* with their own producer BatchNorm -- segment s uses in_scale + s*seg_stride, in_shift + s*seg_stride    */
                          /* (the TripletNet branches as one batch: dW is linear in the pixels, their statistics are per branch)    */
  /* Alignment (sslcr_wgrad_desc): x, dy 16-byte aligned; dw, in_scale, in_shift 4-byte aligned (dW is read and written one float
     at a time by its single owner).  Errors of sslcr_conv2d_wgrad: a pointer below its alignment. */
} sslcr_wgrad_desc;
int sslcr_conv2d_wgrad(int dtype, const sslcr_wgrad_desc* d, void* stream);
/* name of the kernel instance sslcr_conv2d_wgrad would launch for this descriptor (static string, as sslcr_conv2d_kernel_name) */
const char* sslcr_conv2d_wgrad_kernel_name(int dtype, const sslcr_wgrad_desc* d);

/* diagnostics: lane l of one wave performs ds_read_b64_tr_b16 at byte_addr[l] of a 2 KiB LDS copy of `in`; out[l][0..3] */
int sslcr_probe_tr16(const uint16_t* in, const int* byte_addr, uint16_t* out, void* stream);

/* ---- stem: uint8/fp32 NCHW ingestion fused with conv1 7x7/2 (eval_BreastPathQ_SSL_CR.py:68-74 .float()/reshape
 *      + resnet18.conv1) */
typedef struct sslcr_stem_desc {
  const void* x;          /* NCHW [N][3][H][W], uint8 (in_f32=0) or fp32 (in_f32=1), values 0..255 un-normalised */
  const void* w;          /* packed [64][7][8][4] (s=7 and c=3 are zero) -- see sslcr_pack_stem */
  void* y;                /* NHWC [N][OH][OW][64] */
  const float* bias;      /* [64] or NULL */
  float* stats;           /* [sslcr_stem_partial_rows][2][64] or NULL */
  int N, H, W, OH, OW, in_f32, relu;
  const void* x2;         /* optional second input segment: images n >= n_split are read from x2[n - n_split] -- the
                             reference's torch.cat((inputs_x, inputs_u_s)) (eval_BreastPathQ_SSL_CR.py:82) without the copy */
  int n_split;
  const float* out_scale; /* [64] or NULL, as sslcr_conv_desc.out_scale (library version >= 6) */
  /* Alignment (sslcr_stem_desc): w, y 16-byte aligned; x, x2, bias, stats, out_scale 4-byte aligned (the uint8 planes are read as
     whole dwords where W % 4 == 0).  Errors of sslcr_stem_conv and sslcr_stem_conv_pool: a pointer below its alignment. */
} sslcr_stem_desc;
int sslcr_stem_conv(int dtype, const sslcr_stem_desc* d, void* stream);
int sslcr_stem_partial_rows(const sslcr_stem_desc* d);
/* eval-mode stem in one launch: conv1 (BatchNorm folded into d->w / d->bias) -> ReLU -> maxpool 3x3/2 pad 1, i.e. resnet18.conv1 ..
 * .maxpool as the teacher forward, validate() and test_Camelyon16.py reach them (models/net.py:32,77 under model.eval()).  d->y is the
 * POOLED output [N][POH][POW][64] (POH = OH / 2, POW = OW / 2); the conv output never reaches HBM.  bf16, d->relu set, d->stats NULL,
 * OH and OW multiples of 16 with 32 <= OW <= 256; other shapes fail (sslcr_stem_conv + sslcr_bn_relu_maxpool serve them, with the same
 * bits where both apply). */
int sslcr_stem_conv_pool(int dtype, const sslcr_stem_desc* d, int POH, int POW, void* stream);
typedef struct sslcr_stem_wgrad_desc {
  const void* x; const void* dy;
  float* dw;              /* [64][3][7][7] fp32 (PyTorch layout), accumulated */
  int N, H, W, OH, OW, in_f32;
  const void* x2; int n_split;   /* as in sslcr_stem_desc */
  /* Alignment (sslcr_stem_wgrad_desc): dy 16-byte aligned; x, x2, dw 4-byte aligned.  Errors of sslcr_stem_wgrad and
     sslcr_stem_wgrad_pool: a pointer below its alignment. */
} sslcr_stem_wgrad_desc;
int sslcr_stem_wgrad(int dtype, const sslcr_stem_wgrad_desc* d, void* stream);

/* ---- BatchNorm2d (train: batch stats, running update; replaces nn.BatchNorm2d x20) */
typedef struct sslcr_bn_finalize_desc {
  const float* partials;  /* [rows][2][C] */
  int rows, C;
  double count;           /* elements per channel (global) */
  const float* gamma; const float* beta;
  float* scale; float* shift; float* mean; float* invstd;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;   /* may be NULL */
  float momentum, eps; int replay;    /* replay=3 reproduces TripletNet_Finetune's 3 identical passes (models/net.py:88-90) */
  double* sums_out;       /* [2][C]: only reduce the partial rows (sharded runs all-reduce this, then call again with sums_in) */
  const double* sums_in;
  double* stage;          /* workspace [32][2][C] doubles for the two-stage row reduction ([nseg][32][2][C] with segments) */
  /* segments (sslcr_conv_desc.seg_images): nseg > 1 finalizes nseg BatchNorm batches in one call -- segment s owns partial rows
     [s * rows / nseg, (s + 1) * rows / nseg) and writes scale / shift / mean / invstd at + s * seg_stride floats; the running
     statistics take the nseg updates one after the other, segment 0 first, like nseg successive forward calls (count = elements
     per channel of ONE segment).  With sums_out (rows -> sums only) segment s writes sums_out + s * seg_stride doubles.  Not
     with sums_in. */
  int nseg, seg_stride;
  /* library version >= 6.  NULL: two launches (row reduction, finalize).  Else ceil(C / 32) ints, ZERO before the first call and
     left at zero by every call, not shared with a launch that may run concurrently; with SSLCR_BN_ONE_LAUNCH=1 in the environment
     (read once per process) the row reduction's last workgroup per channel block then finalizes it in the same launch (same
     arithmetic, same bits, one launch less per BatchNorm).  Without that variable the two launches run either way: the one-launch
     form measured slower in the stream (bn_eltwise.hip). */
  int* tickets;
  /* Alignment (sslcr_bn_finalize_desc): num_batches_tracked, sums_out, sums_in, stage 8-byte aligned; partials, gamma, beta, scale,
     shift, mean, invstd, running_mean, running_var, tickets 4-byte aligned.  Errors of sslcr_bn_finalize: a pointer below its
     alignment. */
} sslcr_bn_finalize_desc;
int sslcr_bn_finalize(const sslcr_bn_finalize_desc* d, void* stream);

typedef struct sslcr_bn_act_desc {      /* y = relu(x*scale+shift [+ res*rscale+rshift | + res])  (K5 apply, K6, K7) */
  const void* x; const float* scale; const float* shift;
  const void* res; const float* rscale; const float* rshift;
  void* y; size_t pixels; int C; int relu;
  int nseg, seg_stride;   /* nseg > 1: the pixels are nseg equal segments, segment s uses (r)scale / (r)shift + s * seg_stride */
  uint8_t* ybits;         /* optional (bf16 only): one bit per element of y in NHWC order, bit (e & 7) of byte e / 8 = (y[e] > 0) -- the
                             ReLU mask of a residual block's output as BatchNorm backward wants it (sslcr_bn_bwd_desc.yact_bits):
                             a sixteenth of the bytes of y */
  /* Alignment (sslcr_bn_act_desc): x, res, y 16-byte aligned; scale, shift, rscale, rshift 4-byte aligned; ybits 1-byte aligned (any
     address: one byte store per chunk).  Errors of sslcr_bn_act: a pointer below its alignment. */
} sslcr_bn_act_desc;
/* Widths: every C % 8 == 0, in both dtypes (16-byte chunks of 8 bf16 / 4 fp32 channels; C / 8 resp. C / 4 chunks per pixel need NOT
 * divide 256).  A thread keeps its chunk's constants across its grid-stride trips: the launch rounds its grid so that the stride is
 * a multiple of the chunks per pixel (unchanged where that count is a power of two up to 256, every ResNet width). */
int sslcr_bn_act(int dtype, const sslcr_bn_act_desc* d, void* stream);

typedef struct sslcr_pool_fwd_desc {    /* maxpool3x3/2 pad 1 of relu(bn(x))   (K8); scale = shift = argmax = NULL: plain
                                           max-pool of x as it is (the eval path: BatchNorm folded into conv1, ReLU in its epilogue) */
  const void* x; const float* scale; const float* shift; void* y; uint8_t* argmax; int N, H, W, C, OH, OW;
  /* Alignment (sslcr_pool_fwd_desc): x, y 16-byte aligned; argmax 8-byte aligned (a chunk's eight codes are one 8-byte store in
     bf16, four codes one dword in fp32); scale, shift 4-byte aligned.  Errors of sslcr_bn_relu_maxpool: a pointer below its alignment. */
} sslcr_pool_fwd_desc;
int sslcr_bn_relu_maxpool(int dtype, const sslcr_pool_fwd_desc* d, void* stream);
typedef struct sslcr_pool_bwd_desc {
  const void* dy; const uint8_t* argmax; const void* x; const float* scale; const float* shift; void* dx; int N, H, W, C, OH, OW;
  /* Alignment (sslcr_pool_bwd_desc): dy, x, dx 16-byte aligned; argmax 8-byte aligned; scale, shift 4-byte aligned.  Errors of
     sslcr_maxpool_relu_bwd: a pointer below its alignment. */
} sslcr_pool_bwd_desc;
int sslcr_maxpool_relu_bwd(int dtype, const sslcr_pool_bwd_desc* d, void* stream);

/* Alignment (sslcr_avgpool_fwd): x 16-byte aligned; y 4-byte aligned.  Alignment (sslcr_avgpool_bwd): dy 4-byte aligned; dx 16-byte
   aligned.  Errors: a pointer below its alignment. */
int sslcr_avgpool_fwd(int dtype, const void* x, float* y, int N, int HW, int C, void* stream);          /* K9 */
int sslcr_avgpool_bwd(int dtype, const float* dy, void* dx, int N, int HW, int C, void* stream);

typedef struct sslcr_bn_bwd_desc {
  const void* dy; const void* x; const void* yact;
  const float* scale; const float* shift; const float* mean; const float* invstd;
  double* sums;           /* [2][C]: OVERWRITTEN by the reduce pass (ordered sum of its workgroups' rows: same bits every run) */
  void* dx; void* gout;
  size_t pixels; int C; int relu_from_x; double count;
  const void* pool_dy;    /* optional: dy is not given directly but through maxpool3x3/2 pad 1 -- pooled gradient [N][pOH][pOW][C] ... */
  const uint8_t* pool_argmax;   /* ... and the argmax codes recorded by sslcr_bn_relu_maxpool (window position 0..8; 9 = maximum not
                                   positive, no gradient); x is then [N][pH][pW][C] */
  int pH, pW, pOH, pOW;
  const void* pool_y;     /* optional with pool_dy: the max-pool OUTPUT saved by the forward, [N][pOH][pOW][C].  With it the reduce
                             pass reads only the pooled tensors: a pooled gradient lands on exactly one input pixel, whose
                             relu(bn(x)) IS the pooled output, so (x - mean) = (y - shift) / scale - mean where y > 0 */
  int g_in_reduce;        /* with yact and gout: the REDUCE pass writes the masked gradient g = dy * (yact > 0) to gout, and the
                             apply pass reads it back instead of dy and yact (one tensor read less; the identity path of a
                             residual block needs g anyway).  Not with pool_dy. */
  float* dgamma; float* dbeta;   /* optional: the apply pass also accumulates the affine gradients (what sslcr_bn_param_grads does: */
  float pg_scale;                /*   dgamma += pg_scale * sums[1] * invstd, dbeta += pg_scale * sums[0]) -- one launch less per BatchNorm */
  /* segments (sslcr_conv_desc.seg_images): nseg > 1 runs nseg BatchNorm batches in one launch -- `pixels` is then the total and
     each segment an equal share of it (tensors contiguous across segments); segment s uses scale / shift / mean / invstd
     + s * seg_stride floats and sums + s * sums_stride doubles; count = elements per channel of ONE segment; dgamma / dbeta take
     the segments' contributions one after the other, segment 0 first.  Not with pool_dy. */
  int nseg, seg_stride, sums_stride;
  const uint8_t* yact_bits;   /* instead of yact (bf16 only): its sign mask as written by sslcr_bn_act (ybits) -- g = dy where the bit is
                                 set, 0 elsewhere: the same g, bit for bit, for 1/16 of yact's bytes */
  /* Alignment (sslcr_bn_bwd_desc): dy, x, yact, dx, gout, pool_dy, pool_y 16-byte aligned; sums, pool_argmax 8-byte aligned; scale,
     shift, mean, invstd, dgamma, dbeta 4-byte aligned; yact_bits 1-byte aligned (any address).  Errors of sslcr_bn_bwd_reduce,
     sslcr_bn_bwd_apply and sslcr_stem_wgrad_pool: a pointer below its alignment. */
} sslcr_bn_bwd_desc;
/* ABI note (library version >= 4): sslcr_bn_bwd_reduce OVERWRITES d->sums (until version 3 it accumulated into a buffer the caller had
 * zeroed) -- several reduce calls into one sums buffer keep only the last one; add them on the caller's side.  The reduce pass and the
 * weight-gradient entry points (sslcr_conv2d_wgrad, sslcr_stem_wgrad*) keep per-stream scratch for their ordered folds: the first call
 * on a stream (and any call that needs more than before) allocates with hipMalloc / hipStreamSynchronize INSIDE the call, so these
 * entry points must not be issued under hipStreamBeginCapture unless an earlier un-captured call on that stream has sized the scratch.
 * The scratch is released by sslcr_destroy. */
/* Widths: sslcr_bn_bwd_reduce serves the widths whose 16-byte chunks per pixel (C / 8 bf16, C / 4 fp32) divide 256 and fails for
 * every other; sslcr_bn_bwd_apply (plain, segment and pool forms) serves every C that is a multiple of the chunk (8 bf16, 4 fp32)
 * from sums the caller provides -- like sslcr_bn_act it rounds its grid so that a thread keeps its channels. */
int sslcr_bn_bwd_reduce(int dtype, const sslcr_bn_bwd_desc* d, void* stream);
int sslcr_bn_bwd_apply(int dtype, const sslcr_bn_bwd_desc* d, void* stream);
/* Alignment (sslcr_bn_param_grads): sums 8-byte aligned; invstd, dgamma, dbeta 4-byte aligned.  Errors: a pointer below its alignment. */
int sslcr_bn_param_grads(const double* sums, const float* invstd, float* dgamma, float* dbeta, int C, void* stream);
/* conv1 wgrad with bn0's backward apply pass computed on the fly (autograd of resnet18.conv1 <- bn1 <- relu <- maxpool,
 * models/net.py:32,77): `bn` is a pool-form descriptor (pool_dy, pool_argmax, x = the raw conv1 output, pH/pW = w->OH/OW) whose
 * reduce pass has run (sums final, all-reduced when sharded); the un-pooled gradient (bn->dx, w->dy) is never written or read --
 * each workgroup derives its 8x16 dY tile in LDS.  dgamma/dbeta are accumulated as sslcr_bn_bwd_apply would.  Same result, bit for
 * bit, as sslcr_bn_bwd_apply followed by sslcr_stem_wgrad. */
int sslcr_stem_wgrad_pool(int dtype, const sslcr_stem_wgrad_desc* w, const sslcr_bn_bwd_desc* bn, void* stream);
/* diagnostics: the kernel instance sslcr_stem_wgrad_pool launches for (dtype, w), spelled as rocprofv3 prints it */
const char* sslcr_stem_wgrad_pool_kernel_name(int dtype, const sslcr_stem_wgrad_desc* w);

/* ---- heads and losses (models/net.py:12-15,35-36,111; F.mse_loss / F.cross_entropy at
 *      eval_BreastPathQ_SSL_CR.py:92-95, eval_Camelyon_SSL_CR.py:110-116, pretrain_BreastPathQ.py:56) */
/* Alignment (sslcr_linear_fwd): x, w, b, y 4-byte aligned.  Alignment (sslcr_linear_bwd): x, w, dy, yact, dx, dw, db, scratch 4-byte
   aligned.  (The GEMMs fetch an operand as float4 only where its base is 16-byte aligned and its row stride a multiple of four
   floats, and one float at a time otherwise: the same sums in another order.)  Errors: a pointer below its alignment. */
int sslcr_linear_fwd(const float* x, const float* w, const float* b, float* y, int M, int N, int K, int relu, void* stream);
int sslcr_linear_bwd(const float* x, const float* w, const float* dy, const float* yact, float* dx, float* dw, float* db,
                     int M, int N, int K, int dx_accumulate, float* scratch, void* stream);
typedef struct sslcr_loss_desc {
  int kind;               /* 0 mse+mse (BreastPathQ CR) ; 1 ce + hard-pseudo-label ce (Camelyon/Kather CR) ; 2 ce ; 3 mse */
  const float* logits; const float* logits_t;
  const float* target_f; const int64_t* target_i;
  float* dlogits;
  float* out;             /* [4]: loss, loss_x, loss_u, #correct */
  int nx, nu, C; float lambda_u;
  float inv_nx_global, inv_nu_global;
  /* Alignment (sslcr_loss_desc): target_i 8-byte aligned; logits, logits_t, target_f, dlogits, out 4-byte aligned.  Errors of
     sslcr_loss and sslcr_loss_ex: a pointer below its alignment. */
} sslcr_loss_desc;
int sslcr_loss(const sslcr_loss_desc* d, void* stream);
/* library version >= 10.  Options of the cross-entropy kinds (1, 2); sslcr_loss and its launch are unchanged.
 * Supervised rows -- torch.nn.functional.cross_entropy(logits_x, target, weight=, label_smoothing=, ignore_index=, reduction='mean')
 * with the three taken together as torch defines them:
 *   loss_x = [ (1 - eps) * sum_i w[y_i] * (-log p_i[y_i])  +  eps / C * sum_i sum_c w[c] * (-log p_i[c]) ] / denominator
 * over the rows whose target is not ignore_index, denominator = sum_i w[y_i] over the same rows.  An ignored row has zero loss and
 * zero dlogits and is never counted in out[3].  denominator == 0 (every row ignored, or only zero-weight classes present): loss_x
 * and loss are NaN and the dlogits of the rows that are not ignored are NaN, those of ignored rows zero -- torch's 0 / 0.  A
 * target outside [0, C) that is not ignore_index (torch raises) is never read out of bounds: the row has no loss and zero dlogits,
 * and it makes the denominator -- out2[0] of sslcr_ce_denominator too -- and with it loss_x, loss and the kept rows' dlogits NaN,
 * the signal a loop can see without a sync.
 * Consistency rows (kind 1 only; weight / smoothing / ignore_index do not apply to them, as in the reference):
 *   mask_i = max_c softmax(logits_t_i)_c >= threshold          (FixMatch: `max_probs.ge(threshold)`; eval_Camelyon_SSL_CR.py:113
 *                                                               computes max_probs and drops it)
 *   loss_u = sum_i mask_i * CE_i * inv_nu_global               (`(loss * mask).mean()`: ALL unlabeled rows divide, so the term stays
 *                                                               linear over micro-batches and ranks)
 *   temperature 0: CE_i against the hard pseudo label argmax(logits_t_i) (sslcr_loss's arithmetic); T > 0: against the soft
 *   targets p = softmax(logits_t_i / T) (UDA sharpening): CE_i = -sum_c p_c log softmax(logits_s_i)_c, gradient softmax(logits_s_i) - p.
 *   The mask always reads the unsharpened softmax; at threshold 0 no test is made at all (a teacher row with a NaN propagates it,
 *   as in sslcr_loss). */
typedef struct sslcr_loss_opts {
  const float* class_weight;  /* device [C] or NULL: F.cross_entropy(weight=) */
  float label_smoothing;      /* eps in [0, 1): F.cross_entropy(label_smoothing=) */
  int ignore_index;           /* F.cross_entropy(ignore_index=); -100 = torch's default */
  float threshold;            /* tau in [0, 1]; 0 = no mask */
  float temperature;          /* T >= 0; 0 = hard pseudo labels */
  const float* denominator;   /* device [1] or NULL.  NULL: with class_weight, a non-default ignore_index or rows that carry the
                                 default -100 the kernel sums w[y_i] over the kept rows of THIS call (sslcr_ce_denominator's order
                                 and bits), else it scales by inv_nx_global as sslcr_loss does.  Non-NULL: the divisor of the supervised term, read on the device --
                                 out2 of sslcr_ce_denominator over the whole global batch (all-reduced when sharded) when this call
                                 holds a micro-batch or a shard of it. */
  float* stats;               /* device [2] or NULL: {#rows with mask_i = 1, sum_i max_c softmax(logits_t_i)_c} of this call */
  /* Alignment (sslcr_loss_opts): class_weight, denominator, stats 4-byte aligned.  Errors of sslcr_loss_ex: a pointer below its alignment. */
} sslcr_loss_opts;
/* opts == NULL: sslcr_loss.  All-default opts (NULL pointers, 0, -100, 0, 0): sslcr_loss's bits for all five kinds -- the MSE kinds
 * by its launch, the cross-entropy kinds by this entry's kernel, whose default arithmetic is the same and which, unlike sslcr_loss
 * (every target must be a class id there), leaves out rows labelled -100.  Errors, decided before any launch: kinds 0 / 3 with a non-default option, C > 64, label_smoothing outside [0, 1), threshold outside [0, 1],
 * temperature < 0, threshold / temperature with kind 2.  One single-workgroup launch; row counts of any size are served. */
int sslcr_loss_ex(const sslcr_loss_desc* d, const sslcr_loss_opts* opts, void* stream);
/* library version >= 10.  The divisor of a weighted / ignore-index mean from the targets alone:
 *   out2 = { sum_i class_weight[target_i[i]] (1 per row when class_weight is NULL), number of such rows }
 * over the rows with target != ignore_index -- `weight[target[target != ignore_index]].sum()`.  n >= 0.  One launch, no atomics, summed in
 * double in a fixed order: the same bits every run, and the bits sslcr_loss_ex derives for itself over the same rows. */
/* Alignment (sslcr_ce_denominator): target_i 8-byte aligned; class_weight, out2 4-byte aligned.  Errors: a pointer below its alignment. */
int sslcr_ce_denominator(const int64_t* target_i, int n, int C, const float* class_weight, int ignore_index, float* out2, void* stream);
/* out[i] = softmax(logits[i, 0..C-1])[col]: the per-tile 'tumor' probability of test_Camelyon16.py:58-60 (row f3) */
/* Alignment (sslcr_softmax_col): logits, out 4-byte aligned.  Errors: a pointer below its alignment. */
int sslcr_softmax_col(const float* logits, float* out, int n, int C, int col, void* stream);
/* library version >= 12.  What the reference's test() loops take from a batch of logits, in one launch, every output optional (NULL):
 *   scores[i][c]              = softmax(logits[i])[c]                      torch.softmax(output, dim=-1), eval_Kather_SSL_CR.py:211
 *   pred[i]                   = argmax_c logits[i][c]                      torch.argmax(output, dim=1), :220 / eval_Kather_SSL.py:190:
 *                               the LOWEST index of the row maximum; a NaN counts as the maximum (the lowest NaN index wins)
 *   confusion[target][pred]  += 1                                          sklearn's confusion_matrix(targets, predictions) of
 *                               eval_Kather_SSL_CR.py:646-658 / eval_Kather_SSL.py:519-530, accumulated ACROSS calls by integer
 *                               atomics (exact, order-independent); the caller zeroes it; rows with target outside [0, C) are skipped
 *   map[map_index[i]]         = softmax(logits[i])[col]                    probs_map[x_mask, y_mask] = probs, test_Camelyon16.py:58-62;
 *                               the value has the bits of sslcr_softmax_col (one device function); an index outside [0, map_size) is
 *                               skipped; duplicate indices within one call are undefined
 * Errors, decided before the launch: NULL logits, n < 0, C outside [1, 64], confusion without target, map without map_index, col outside
 * [0, C), map_size < 0.  n == 0 is a no-op.  Rows of any count are served; no float atomics. */
typedef struct sslcr_predict_desc {
  const float* logits;        /* [n][C] */
  int n, C;
  const int64_t* target;      /* [n] or NULL */
  float* scores;              /* [n][C] or NULL */
  int64_t* pred;              /* [n] or NULL */
  int64_t* confusion;         /* [C][C] or NULL (8-byte aligned) */
  int col;                    /* 0 <= col < C */
  float* map;                 /* [map_size] or NULL */
  const int64_t* map_index;   /* [n] */
  int64_t map_size;
} sslcr_predict_desc;
int sslcr_predict(const sslcr_predict_desc* d, void* stream);

/* ---- optimizers (torch.optim.Adam / SGD nesterov as the reference configures them,
 *      eval_BreastPathQ_SSL_CR.py:481, eval_Camelyon_SSL_CR.py:514, pretrain_BreastPathQ.py:245; Lookahead lookahead.py:81-106) */
typedef struct sslcr_tensor_desc {
  float* p; float* g; float* s1; float* s2;
  int n;
  int K, C, RS;           /* conv weight: g is [K][RS][C] while p/s1/s2 are [K][C][RS] ; K=0: same layout */
  void* w_fwd;            /* optional (K > 0): the update also writes the conv kernels' shadow weights of the new value -- */
  void* w_dgrad;          /* forward pack [K][RS][C] and dgrad pack [C][RS][K] (sslcr_pack_conv layouts), element type pack_dtype */
  int pack_dtype;         /* 0 fp32, 1 bf16 */
  int dgrad_flip;         /* dgrad pack with the taps reversed (stride-1 3x3 dgrad runs as a plain conv of dY) */
  int group;              /* library version >= 8: the tensor's row of the `groups` table (torch param_groups); 0 with the one-row entries */
  /* Alignment (sslcr_tensor_desc): p, g, s1, s2, w_fwd, w_dgrad 4-byte aligned (every access is one element).  The table lives in
     device memory, so no entry point can check these: stated, not enforced. */
} sslcr_tensor_desc;
typedef struct sslcr_opt_desc {
  int kind;               /* 0 adam, 1 sgd-nesterov; library version >= 8: 2 adamw (torch.optim.AdamW: p *= 1 - lr * wd first, then the
                             Adam update of the plain gradient -- wd never enters the moments) */
  float lr, beta1, beta2, eps, wd, momentum;
  float bc1, bc2;
  int first_step;
  float grad_scale;
} sslcr_opt_desc;
/* Alignment (sslcr_optimizer_step): device_descs 8-byte aligned.  Alignment (sslcr_optimizer_step_groups): device_descs 8-byte aligned;
   coef_dev 4-byte aligned.  Errors: a pointer below its alignment.  (o / groups are HOST pointers.) */
int sslcr_optimizer_step(const sslcr_tensor_desc* device_descs, int ntensors, int max_n, const sslcr_opt_desc* o, void* stream);
/* library version >= 8.  The same update with one sslcr_opt_desc row per torch param group (optimizer.param_groups: per-group lr,
 * weight_decay, betas / eps or momentum, and the bias corrections of that group's betas): tensor t takes groups[t.group], every
 * t.group < ngroups <= SSLCR_MAX_OPT_GROUPS (a tensor whose group lies past ngroups is left unchanged).  coef_dev: NULL, or a device float every gradient is multiplied with on top of
 * grad_scale -- out2 + 1 of sslcr_grad_norm, i.e. the `p.grad.mul_(clip_coef_clamped)` of torch.nn.utils.clip_grad_norm_ without a
 * pass of its own. */
#define SSLCR_MAX_OPT_GROUPS 8
int sslcr_optimizer_step_groups(const sslcr_tensor_desc* device_descs, int ntensors, int max_n, const sslcr_opt_desc* groups, int ngroups,
                                const float* coef_dev, void* stream);
/* library version >= 8.  torch.nn.utils.clip_grad_norm_(params, max_norm) (norm_type 2) up to the scaling itself: the 2-norm of the
 * n floats at g (any n >= 0, any 4-byte-aligned base) and the clamped coefficient, left on the device with no host sync:
 *   out2[0] = (float)sqrt(sum (double)g_i^2), out2[1] = min(1, max_norm / (out2[0] + 1e-6f))    (exactly 1.0f for max_norm = +inf).
 * partials: workspace of sslcr_grad_norm_partials() doubles.  Two launches, no atomics, a fixed summation order: the same bits every
 * run, and the same bits on every rank that holds the same buffer. */
int sslcr_grad_norm(const float* g, size_t n, float max_norm, double* partials, float* out2, void* stream);
int sslcr_grad_norm_partials(void);
/* library version >= 9.  What loss.backward() does to a leaf's .grad when no optimizer.zero_grad() went before it (autograd's
 * `.grad += new`): dst[i] = dst[i] + src[i] for i < n, ONE IEEE fp32 add per element (no FMA, nothing reassociated; NaN and inf
 * propagate as the add defines).  Any n >= 0, any two 4-byte-aligned bases -- dst and src may sit at different offsets mod 16; the
 * ranges must not overlap.  One launch, no atomics, one writer per element: the same bits every run. */
int sslcr_grad_accumulate(float* dst, const float* src, size_t n, void* stream);
int sslcr_axpby(float* p, float* q, size_t n, float alpha, int copy_back, void* stream);
int sslcr_fill(float* p, size_t n, float v, void* stream);

typedef struct sslcr_pack_desc {
  const float* w; void* w_fwd; void* w_dgrad;
  const float* gamma; const float* beta; const float* rmean; const float* rvar; float eps; float* bias_out;
  int K, C, R, S;
  int dgrad_flip;         /* w_dgrad taps reversed ([C][R-1-r][S-1-s][K]): a stride-1 dgrad then IS a plain conv of dY */
  float* scale_out;       /* library version >= 6, with gamma: [K] <- gamma / sqrt(rvar + eps) and w_fwd keeps the PLAIN filter (the fold's
                             scale goes to the conv's epilogue: sslcr_conv_desc.out_scale); bias_out is the shift either way.  NULL: folded */
} sslcr_pack_desc;
int sslcr_pack_conv(int dtype, const sslcr_pack_desc* d, void* stream);
int sslcr_pack_stem(int dtype, const sslcr_pack_desc* d, void* stream);

/* ---- device-side weak augmentation ("next" row f1): TransformFix.weak = RandomHorizontalFlip() + RandomCrop(image_size)
 *      (dataset.py:663-677), applied to a uint8 batch that is already in HBM.  The random draws stay on the host, in the
 *      reference's order per sample (flip: torch.rand(1) < 0.5 ; crop: randint(0, SH-OH+1), randint(0, SW-OW+1)), so a run
 *      is reproducible against the CPU transform; the kernel is the deterministic gather
 *        dst[n][c][i][j] = src[n][c][top+i][flip ? SW-1-(left+j) : left+j]
 *      writing the NCHW uint8 batch the stem ingests (eval_BreastPathQ_SSL_CR.py:68-74). */
typedef struct sslcr_weak_aug_desc {
  const uint8_t* src;     /* [N][3][SH][SW] (src_hwc=0) or [N][SH][SW][3] (src_hwc=1, the PIL/numpy layout) */
  uint8_t* dst;           /* [N][3][OH][OW] */
  const int32_t* params;  /* [N][3] device ints: flip (0/1), top, left */
  int N, SH, SW, OH, OW, src_hwc;
} sslcr_weak_aug_desc;
int sslcr_weak_augment(const sslcr_weak_aug_desc* d, void* stream);

/* ---- device-side WSI tiling (row f3): the read_region + np.array(...).transpose((2, 0, 1)) of DatasetCamelyon16_test.__getitem__
 *      (dataset.py:983-996) for a whole batch of tiles, from ONE slide region that is already in HBM (library version >= 12):
 *        dst[n][c][i][j] = src[top - origin_y + i][left - origin_x + j][c]   where that pixel lies inside the region, `fill` elsewhere
 *      with (left, top) = xy[n]: tiles partly or wholly outside the region, on any side, are served.  Source offsets are 64-bit (a
 *      region may exceed 2^32 bytes).  A byte gather: no floating point, no atomics, one launch.  Errors, decided before the launch:
 *      NULL pointers, S < 1, N < 0, RH < 1, RW < 1, fill outside [0, 255].  N == 0 is a no-op. */
typedef struct sslcr_wsi_gather_desc {
  const uint8_t* src;     /* [RH][RW][3], the PIL / numpy layout */
  const int32_t* xy;      /* [N][2] device ints: level-0 (left, top) of every tile */
  uint8_t* dst;           /* [N][3][S][S] */
  int origin_x, origin_y; /* level-0 coordinates of src[0][0] */
  int N, RH, RW, S, fill;
} sslcr_wsi_gather_desc;
int sslcr_wsi_gather(const sslcr_wsi_gather_desc* d, void* stream);

/* ---- test-time augmentation over the dihedral group D4 (library version >= 13): the eight flips and quarter turns of a SQUARE tile.
 *      An orientation code g in 0..7 is f = g >> 2, a horizontal flip applied FIRST, and k = g & 3, the number of counter-clockwise
 *      quarter turns applied SECOND; in NumPy, for t[..., S, S]:
 *        d4(t, g) = np.rot90(t[..., ::-1] if g >> 2 else t, g & 3, axes=(-2, -1))
 *      i.e. d4(t, g)[i][j] = t[si][sj] with (a, b) = (k & 1) ? (j, i) : (i, j), si = (k >> 1) ? S-1-a : a,
 *      sj = ((((k + 1) >> 1) & 1) ^ f) ? S-1-b : b.  Codes 1, 3, 5, 7 are transposes.  Only the low three bits of a code are read.
 *
 *      sslcr_d4_transform: dst[n] = d4(src[n], orient[n]) for a batch [N][Cn][S][S] of 1-byte (the uint8 batches the stem ingests) or
 *      4-byte (float32 batches of a host loader) elements.  Out of place only.  Any S >= 1, Cn >= 1; a byte batch whose side is no
 *      multiple of four, or whose bases are not dword aligned, takes the per-element path of the same kernel.  No floating point, no
 *      atomics, one launch.  Errors, decided before the launch: NULL pointers, N < 0, Cn < 1, H < 1, H != W (tiles are square),
 *      elem_bytes outside {1, 4}, a 4-byte batch that is not 4-byte aligned, orient not 4-byte aligned, src and dst ranges that overlap.
 *      N == 0 is a no-op.
 *
 *      sslcr_wsi_gather_d4: sslcr_wsi_gather writing d4(tile n, orient[n]); `fill` and tiles partly or wholly outside the region as
 *      there, the descriptor unchanged, the same errors (plus orient alignment).  orient == NULL is sslcr_wsi_gather itself (its
 *      launch); an all-zero orient gives the same bytes. */
typedef struct sslcr_d4_desc {
  const void* src;        /* [N][Cn][H][W] */
  void* dst;              /* [N][Cn][H][W] */
  const int32_t* orient;  /* [N] device ints, codes 0..7 */
  int N, Cn, H, W;        /* H == W */
  int elem_bytes;         /* 1 or 4 */
} sslcr_d4_desc;
int sslcr_d4_transform(const sslcr_d4_desc* d, void* stream);
int sslcr_wsi_gather_d4(const sslcr_wsi_gather_desc* d, const int32_t* orient, void* stream);

/* library version >= 13.  sslcr_predict over an ensemble of G sets of logits, p.logits = L[G][n][C] (set g at + g * n * C), in one launch:
 *   mode 0 (probabilities)  s[i][c] = (p_0 + p_1 + ... + p_{G-1}) / (float)G   with p_g = softmax(L[g][i])[c], the device function of
 *                           sslcr_predict; the sum left to right in fp32 with plain IEEE adds (no FMA, nothing reassociated), then ONE
 *                           fp32 division
 *   mode 1 (raw outputs)    the same with p_g = L[g][i][c] (a regression head)
 *   p.scores[i][c]           = s[i][c]
 *   p.pred[i]                = the LOWEST index of the maximum of s[i]; a NaN counts as the maximum (sslcr_predict's rule).  With G == 1
 *                              the maximum is taken over L[0][i] as sslcr_predict takes it (the same index, except where two different
 *                              logits round to one probability)
 *   p.confusion[target][pred] += 1   ONCE per row, not once per member; integer atomics, rows with target outside [0, C) skipped
 *   p.map[map_index[i]]      = s[i][col]
 * With G == 1 (mode 0) every output has the bits of sslcr_predict.  Errors, decided before the launch: those of sslcr_predict, G outside
 * [1, 8], mode outside {0, 1}, mode 1 combined with map, pred or confusion.  n == 0 is a no-op.  No float atomics. */
#define SSLCR_TTA_MAX 8
typedef struct sslcr_predict_tta_desc {
  sslcr_predict_desc p;       /* logits: [G][n][C] */
  int G;                      /* 1..SSLCR_TTA_MAX */
  int mode;                   /* 0 mean of softmax probabilities, 1 mean of the raw outputs */
} sslcr_predict_tta_desc;
int sslcr_predict_tta(const sslcr_predict_tta_desc* d, void* stream);

/* ---- device-side tile mining for RSP pretraining (library version >= 14): Vectorize_WSIs.get_wsi_patches + sorted_sequence
 *      (dataset.py:27-70, 386-446 with util.py:18-23; Pretraining_v2/dataset.py:22-60, 219-316 with Pretraining_v2/util.py:9-13) on
 *      pyramid levels that already sit in HBM as uint8 [H][W][3], the PIL / numpy layout.  Four entries, all asynchronous, no host sync
 *      between them, no floating-point atomics.
 *
 *      sslcr_tissue_bits: the per-pixel predicate of isforeground() (util.py:20-21, Pretraining_v2/util.py:11-12), one bit per pixel:
 *      bit (x & 31) of dword bits[y * pitch + (x >> 5)] is pixel (x, y); pitch >= ceil(W / 32) dwords; every dword of a row below the
 *      pitch is written and pad bits are zero.
 *        mode SSLCR_TISSUE_HSV_S  s > threshold with skimage 0.15 rgb2hsv's s in float64: a = u8 * (1.0 / 255), v = max, delta = max - min,
 *                                 s = delta / v, 0 where delta == 0.  Correctly rounded operations only: the plane EQUALS a NumPy restatement.
 *        mode SSLCR_TISSUE_LAB_A  a* > threshold with skimage 0.15 rgb2lab's a* (D65, 2 degree observer) in float64: lin[u8] per channel
 *                                 (the 256-entry table of c > 0.04045 ? ((c + 0.055) / 1.055) ** 2.4 : c / 12.92, computed by the host),
 *                                 X, Y from rows (0.412453, 0.357580, 0.180423), (0.212671, 0.715160, 0.072169), / (0.95047, 1.0),
 *                                 f(t) = t > 0.008856 ? t ** (1/3) : 7.787 t + 16/116, a* = 500 (f(X) - f(Y)).  pow is the device's
 *                                 (a few ulp): the plane equals a float64 restatement wherever |a* - threshold| exceeds ~1e-12.
 *                                 (A float32 evaluation, error < 9e-4, decides the pixels farther than 1/64 from the threshold; the
 *                                 float64 chain decides the rest.)
 *      threshold: d->threshold, or -- thr_sum != NULL -- factor * (*thr_sum / count) read on the device: (1 + mu_percent) * mean a* of
 *      the overview image (util.py:21 with dataset.py:402-403), thr_sum written by sslcr_lab_a_sum earlier on the same stream.
 *      Errors, decided before the launch: NULL pointers, H < 1, W < 1, pitch < ceil(W / 32), mode outside {0, 1}, mode 1 without lin,
 *      thr_sum with count <= 0, bits / lin / thr_sum misaligned. */
#define SSLCR_TISSUE_HSV_S 0
#define SSLCR_TISSUE_LAB_A 1
typedef struct sslcr_tissue_bits_desc {
  const uint8_t* img;       /* [H][W][3] */
  uint32_t* bits;           /* [H][pitch] dwords */
  const double* lin;        /* mode 1: [256] device doubles; unused in mode 0 */
  const double* thr_sum;    /* NULL, or one device double: threshold = factor * (*thr_sum / count) */
  double threshold;         /* used when thr_sum == NULL */
  double factor, count;     /* used when thr_sum != NULL */
  int H, W, pitch, mode;
} sslcr_tissue_bits_desc;
int sslcr_tissue_bits(const sslcr_tissue_bits_desc* d, void* stream);

/*      sslcr_lab_a_sum: *sum = the sum of a* (as above) over a uint8 [H][W][3] image, the numerator of np.mean(lab[..., 1])
 *      (dataset.py:400-403).  Deterministic: SSLCR_LAB_SUM_PARTIALS workgroups own fixed contiguous pixel slices and fold them in a
 *      fixed tree into partials[], a second stage folds the partials in a fixed order: two runs give the same bits.  Errors: NULL
 *      pointers, H < 1, W < 1, lin / partials / sum not 8-byte aligned. */
#define SSLCR_LAB_SUM_PARTIALS 1024
typedef struct sslcr_lab_a_sum_desc {
  const uint8_t* img;       /* [H][W][3] */
  const double* lin;        /* [256] device doubles */
  double* partials;         /* workspace, [SSLCR_LAB_SUM_PARTIALS] doubles, overwritten */
  double* sum;              /* one device double */
  int H, W;
} sslcr_lab_a_sum_desc;
int sslcr_lab_a_sum(const sslcr_lab_a_sum_desc* d, void* stream);

/*      sslcr_tile_popcount: the candidate grid of get_wsi_patches (dataset.py:424-425) over a bit plane of an H x W image,
 *      ypos_j = sh (j + 1) in range(sh, H - 1 - ph, sh), xpos_i = sw (i + 1) in range(sw, W - 1 - pw, sw):
 *        count[j][i] = set bits of the ph x pw window at (xpos_i, ypos_j)           = np.count_nonzero (util.py:23)
 *        keep[j][i]  = (double)count / (double)(ph * pw) >= thresh                  the reference's division and comparison
 *      ny, nx must be the lengths of the two ranges (0 where a range is empty; an empty grid is a no-op).  Errors: NULL pointers,
 *      H, W, ph, pw, sh, sw < 1, pitch < ceil(W / 32), ny / nx not the lengths of the ranges, bits / count misaligned. */
typedef struct sslcr_tile_popcount_desc {
  const uint32_t* bits;     /* [H][pitch] dwords, as sslcr_tissue_bits writes them */
  int32_t* count;           /* [ny][nx] */
  uint8_t* keep;            /* [ny][nx], 0 / 1 */
  double thresh;
  int H, W, pitch, ph, pw, sh, sw, ny, nx;
} sslcr_tile_popcount_desc;
int sslcr_tile_popcount(const sslcr_tile_popcount_desc* d, void* stream);

/*      sslcr_rsp_gather: the tiles of Vectorize_WSIs.__getitem__ (dataset.py:335-384, Pretraining_v2/dataset.py:234-266) with
 *      sorted_sequence (dataset.py:27-70) applied, for a batch of sample indices, in ONE launch.  Sample k of the virtual dataset of
 *      6 T samples is triplet k / 6 under ordering k % 6 of [[0,1,2],[0,2,1],[1,2,0],[1,0,2],[2,0,1],[2,1,0]] over (hr, lr1, lr2) =
 *      levels (0, 1, 2); with k = idx[n], o = ordering k % 6, l = o[s]:
 *        dst[s][n][c][i][j] = src[l][top + i][left + j][c]   with (left, top) = xy[l][k / 6], `fill` outside level l     s = 0, 1, 2
 *        label[n]           = k % 6
 *      The six-fold copy sorted_sequence builds is never materialised.  sslcr_wsi_gather's kernel body per output: dword stores where
 *      S % 4 == 0 and the three bases are dword aligned, its per-byte path otherwise and for tiles that leave a level.  An index outside
 *      [0, 6 T) reads nothing: three `fill` tiles, label -1.  A byte gather: no floating point, no atomics.  Errors, decided before the
 *      launch: NULL pointers, S < 1, N < 0, T < 1, RH / RW < 1, fill outside [0, 255], xy not 4-byte / idx, label not 8-byte aligned.
 *      N == 0 is a no-op. */
typedef struct sslcr_rsp_gather_desc {
  const uint8_t* src[3];    /* level l: [RH[l]][RW[l]][3] */
  const int32_t* xy[3];     /* level l: [T][2] device ints, (left, top) in the pixels of level l */
  const int64_t* idx;       /* [N] device int64: sample indices in [0, 6 T) */
  uint8_t* dst[3];          /* Data_1, Data_2, Data_3: [N][3][S][S] each */
  int64_t* label;           /* [N] */
  int RH[3], RW[3];
  int T, N, S, fill;
} sslcr_rsp_gather_desc;
int sslcr_rsp_gather(const sslcr_rsp_gather_desc* d, void* stream);

/* ---- Camelyon16 annotations on the device (library version >= 15): Polygon.inside / Annotation.inside_polygons (util.py:197-205,
 *      246-266), which every Camelyon dataset calls once per sample for its label (dataset.py:740-743) and whose truth a probability
 *      map is scored against at the mask cells' centres (dataset.py:985-988).  Two entries, asynchronous, no floating-point atomics.
 *
 *      sslcr_points_in_polygons.  Polygon.inside is skimage.measure.points_in_poly([coord], vertices)[0]; the version the reference
 *      pins (0.15.0) evaluates, per point (x, y) and polygon (xp[0..n-1], yp[0..n-1]), all float64:
 *          c = 0; j = n - 1
 *          for i in 0 .. n-1:
 *              if ((yp[i] <= y and y < yp[j]) or (yp[j] <= y and y < yp[i])) and (x < (xp[j] - xp[i]) * (y - yp[i]) / (yp[j] - yp[i]) + xp[i]):
 *                  c = not c
 *              j = i
 *          inside = c
 *      one subtraction each, one product, one correctly rounded division and one addition, in that order; the division is reached
 *      only where the y-test holds.  This restatement is the definition (unpinned against scikit-image itself: DESIGN section 8).
 *        polygons   vertices [V][2] float64 (x, y), polygon p = vertices[offsets[p] .. offsets[p + 1]), offsets [P + 1] int32,
 *                   non-decreasing from 0 to V (an entry outside [0, V] is read as the nearer end).  A polygon of fewer than 3
 *                   vertices contains nothing; P == 0 gives all zeros.
 *        bounds     NULL, or [P][4] float64 (xmin, ymin, xmax, ymax): a point outside bounds[p] is NOT tested against polygon p.  The
 *                   caller's statement: ymin / ymax the extremes of yp, xmin / xmax the extremes of xp widened by what the chain's
 *                   rounding can add (a few ulp; nothing on integer coordinates).  With such bounds the output is that of NULL.
 *        points     [N][2] float64, or NULL = the grid: point n = i * ny + j is (x0 + i * step, y0 + j * step), N = nx * ny -- the
 *                   output is the row-major [nx][ny] mask, indexed [x][y] as the reference's.
 *        inside[n]  1 where any polygon contains point n, else 0               Annotation.inside_polygons
 *        first[n]   the lowest index of a polygon that contains point n, or -1: the polygon at which the reference's loop returns
 *        exact      0: the float64 chain as written.  1: the caller states that every vertex coordinate and every point coordinate is
 *                   an integer of magnitude <= 2^24; the comparison is then decided by (x - xp[i]) d < (xp[j] - xp[i]) (y - yp[i]) for
 *                   d = yp[j] - yp[i] > 0, reversed for d < 0, every term exact.  Same decisions: the quotient is an integer or at
 *                   least 2^-25 from one, the chain's rounding error is below 2^-26.
 *      The vertex list is staged SSLCR_PIP_CHUNK vertices at a time.  Errors, decided before the launch: NULL descriptor, N < 0 or
 *      N >= 2^31, P < 0, V < 0, NULL inside / offsets (N > 0), NULL vertices with V > 0, misaligned pointers, a grid with nx * ny != N,
 *      step outside [0, 2^31) or a coordinate of magnitude >= 2^53.  N == 0 is a no-op. */
#define SSLCR_PIP_CHUNK 256
typedef struct sslcr_pip_desc {
  const double* vertices;   /* [V][2], 16-byte aligned */
  const int32_t* offsets;   /* [P + 1] */
  const double* bounds;     /* [P][4] or NULL */
  const double* points;     /* [N][2], 16-byte aligned, or NULL: the grid */
  uint8_t* inside;          /* [N] */
  int32_t* first;           /* [N] or NULL */
  int64_t x0, y0, step;     /* the grid (points == NULL) */
  int64_t N;
  int nx, ny;               /* the grid */
  int P, V;
  int exact;
} sslcr_pip_desc;
int sslcr_points_in_polygons(const sslcr_pip_desc* d, void* stream);

/*      sslcr_map_confusion: one pass over a probability map [X][Y] float32, a truth mask and a tissue mask (uint8, nonzero = set), for
 *      T <= 64 thresholds:  confusion[t][truth][map >= thresholds[t]] += 1  over the cells with tissue != 0 (a NaN is below every
 *      threshold).  int64 [T][2][2], accumulated ACROSS calls by integer atomics (exact, order-independent); the caller zeroes it.
 *      Errors: NULL pointers, X < 1, Y < 1, X * Y >= 2^31, T outside [1, 64], map / thresholds not 4-byte or confusion not 8-byte aligned. */
typedef struct sslcr_map_confusion_desc {
  const float* map;         /* [X][Y] */
  const uint8_t* truth;     /* [X][Y] */
  const uint8_t* tissue;    /* [X][Y] */
  const float* thresholds;  /* [T] device floats */
  int64_t* confusion;       /* [T][2][2] */
  int X, Y, T;
} sslcr_map_confusion_desc;
int sslcr_map_confusion(const sslcr_map_confusion_desc* d, void* stream);

/* ---- Camelyon16 lesion scoring on the device: from a probability map and a truth mask to what lesion-level FROC counts.  The
 *      reference stops at the heat map (test_Camelyon16.py), so these definitions are this library's, modelled on the challenge's
 *      published evaluation and on the greedy NMS commonly run on such maps; both are unpinned.  Maps and masks are
 *      [X][Y] as for sslcr_map_confusion; "order" over cells is the linear index x * Y + y.  All entries are asynchronous; every atomic
 *      is an integer min / max / add, so no result depends on the order in which they land.
 *
 *      sslcr_label_components.  labels[x][y] = 0 where mask is 0, else the number of the cell's connected component; connectivity 2
 *      = 8 neighbours, 1 = 4 neighbours.  Components are numbered 1..L by the order of each component's first cell (what
 *      scipy.ndimage.label gives); *count = L.  work: X * Y + ceil(X * Y / SSLCR_LABEL_RUN_CELLS) int32 of scratch.
 *      Errors: NULL pointers, X < 1, Y < 1, X * Y >= 2^31, connectivity outside {1, 2}, pointers not 4-byte aligned (the mask is read
 *      as whole dwords). */
#define SSLCR_LABEL_RUN_CELLS 1024 /* the labeller numbers the components over runs of this many cells: one int32 of work per run */
typedef struct sslcr_label_desc {
  const uint8_t* mask;      /* [X][Y], nonzero = set; 4-byte aligned */
  int32_t* labels;          /* [X][Y] */
  int32_t* count;           /* [1]: L */
  int32_t* work;            /* [X * Y + ceil(X * Y / SSLCR_LABEL_RUN_CELLS)] */
  int X, Y, connectivity;
} sslcr_label_desc;
int sslcr_label_components(const sslcr_label_desc* d, void* stream);

/*      sslcr_gaussian_smooth.  A separable Gaussian in float32, edge mode "nearest" (clamped index), axis 0 (x) first, then axis 1:
 *          pass(src)[i] = (((0 + w[0] * src[clamp(i - R)]) + w[1] * src[clamp(i - R + 1)]) + ...) + w[2R] * src[clamp(i + R)]
 *      every product and every sum rounded to float32 on its own (no fused multiply-add).  weights: 2R + 1 device floats; for a
 *      given sigma the caller computes exp(-k^2 / (2 sigma^2)), k = -R .. R, R = int(4 sigma + 0.5), in float64, normalises to sum 1
 *      and casts to float32.  tmp holds the first pass; dst may be src, tmp may be neither.
 *      Errors: NULL pointers, X < 1, Y < 1, X * Y >= 2^31, R outside [0, SSLCR_SMOOTH_MAX_R], pointers not 4-byte aligned, tmp == src
 *      or tmp == dst. */
#define SSLCR_SMOOTH_MAX_R 64
typedef struct sslcr_smooth_desc {
  const float* src;         /* [X][Y] */
  float* tmp;               /* [X][Y] */
  float* dst;               /* [X][Y] */
  const float* weights;     /* [2R + 1] */
  int X, Y, R;
} sslcr_smooth_desc;
int sslcr_gaussian_smooth(const sslcr_smooth_desc* d, void* stream);

/*      Non-maximum suppression.  A cell is a CANDIDATE iff map > threshold (a NaN is none).  Cell q PRECEDES p iff map[q] > map[p], or
 *      they are equal and q's linear index is lower.  The WINDOW of a selected cell q = (qx, qy) is [qx - r, qx + r) x [qy - r, qy + r)
 *      clipped to the map -- half-open and asymmetric on purpose.  A candidate p is SELECTED iff no selected cell q that precedes p
 *      has p in its window (well-founded along "precedes").  This equals the sequential loop: take the first maximum in order, record
 *      it, zero its window, repeat while max > threshold; the output is the selected cells in that loop's order (= "precedes" order).
 *      A selected cell never removes a cell that precedes it.
 *      Three entries over one descriptor, because the host sizes the launches and bounds the rounds by the candidate count:
 *        sslcr_nms_candidates  zeroes counters[0..3], sets state (0 none, 1 undecided) and compacts the candidates' linear indices
 *                              into cand; counters[0] = their number, which the caller reads and passes as ncand from then on
 *        sslcr_nms_rounds      `rounds` rounds, one launch each.  A round takes every undecided candidate p and reads the state of
 *                              the candidates q that precede it and whose window holds it: one selected -> p is suppressed (3); none
 *                              selected and none undecided -> p is selected (2); else p stays undecided.  A decision is final once
 *                              stored.  counters[1] = the candidates still undecided after the LAST of these rounds.  Every round
 *                              decides at least the first undecided candidate in "precedes" order, so ncand rounds always suffice;
 *                              the caller loops until counters[1] == 0 and gives up after ncand + 1 rounds.
 *        sslcr_nms_collect     counters[2] = the number of selected cells K; if K <= max_detections, det_xy[k] = (x, y) and
 *                              det_prob[k] = map[x][y] for k < K in output order.  If K > max_detections the outputs hold nothing
 *                              of use, nothing is written past max_detections entries, and the caller must raise.
 *      Errors: NULL descriptor or pointers, X < 1, Y < 1, X * Y >= 2^31, radius < 1, max_detections < 1, ncand outside [0, X * Y],
 *      rounds < 0, pointers not 4-byte aligned (state too: the rounds read it as whole dwords). */
typedef struct sslcr_nms_desc {
  const float* map;         /* [X][Y] */
  uint8_t* state;           /* [X][Y], 4-byte aligned */
  int32_t* cand;            /* [X * Y] */
  int32_t* stage;           /* [max_detections] scratch */
  int32_t* counters;        /* [4] */
  int32_t* det_xy;          /* [max_detections][2] */
  float* det_prob;          /* [max_detections] */
  float threshold;
  int X, Y, radius, max_detections, ncand;
} sslcr_nms_desc;
int sslcr_nms_candidates(const sslcr_nms_desc* d, void* stream);
int sslcr_nms_rounds(const sslcr_nms_desc* d, int rounds, void* stream);
int sslcr_nms_collect(const sslcr_nms_desc* d, void* stream);

/*      sslcr_lesion_hits.  For detection k < min(*n_det, max_detections): hit[k] = labels[x_k][y_k] (0 = a false positive; a
 *      detection outside the map hits nothing).  A hit on a label of the ignore list is neither a false nor a true positive.
 *      Otherwise tp_prob[label - 1] = max(tp_prob[label - 1], prob): an integer atomicMax on the float's bits over the probabilities
 *      above +0 (the caller zeroes tp_prob, so a lesion nothing hits keeps 0).  areas (or NULL): areas[l] += the number of cells of
 *      lesion l + 1, int64; the caller zeroes it.  L is the count sslcr_label_components returned.
 *      Errors: NULL descriptor, NULL labels / det_xy / det_prob / n_det / hit, NULL tp_prob with L > 0, NULL ignore with n_ignore > 0,
 *      X < 1, Y < 1, X * Y >= 2^31, L < 0, max_detections < 1, n_ignore < 0, pointers not 4-byte (areas: 8-byte) aligned. */
typedef struct sslcr_hits_desc {
  const int32_t* labels;    /* [X][Y] */
  const int32_t* det_xy;    /* [max_detections][2] */
  const float* det_prob;    /* [max_detections] */
  const int32_t* n_det;     /* [1], device */
  const int32_t* ignore;    /* [n_ignore] labels, or NULL */
  int32_t* hit;             /* [max_detections] */
  float* tp_prob;           /* [L] */
  int64_t* areas;           /* [L] or NULL */
  int X, Y, L, max_detections, n_ignore;
} sslcr_hits_desc;
int sslcr_lesion_hits(const sslcr_hits_desc* d, void* stream);

/* ---- The Camelyon16 evaluation mask on the device: what the challenge's computeEvaluationMask / computeITCList take from
 *      scipy.ndimage and scikit-image (csrc/evalmask.hip).  The challenge takes the Euclidean distance transform of the complement of
 *      the annotation mask, keeps the cells with distance < 75 um / (2 * cell size), fills the holes, labels the result at
 *      connectivity 2, and ignores every lesion whose major_axis_length is below 275 um / cell size as isolated tumour cells (ITC).
 *      Parity with the challenge's Evaluation_FROC.py and with scikit-image's regionprops is UNPINNED: neither was available to
 *      compare against.  PINNED instead, by equality, are the integer definitions below, restated in NumPy (tests/_evalmask_ref.py)
 *      and held there against scipy 1.15.3: sqrt(float64(edt_squared)) is distance_transform_edt bit for bit, fill_holes is
 *      binary_fill_holes.  Arrays are [X][Y] as for sslcr_map_confusion.  All entries are asynchronous and use integer arithmetic
 *      only: two calls give equal bits.  These entries were added without a new version number; a caller tells them by their symbols.
 *
 *      sslcr_edt_squared.  A cell is a ZERO cell iff mask == 0 (invert = 0) or mask != 0 (invert = 1).
 *          out[x][y] = min(limit, min over the zero cells (x', y') of (x - x')^2 + (y - y')^2)
 *      so it is 0 on a zero cell, and a mask without a zero cell gives `limit` everywhere (scipy's answer there is meaningless; this
 *      is the library's definition).  limit = INT32_MAX is the unlimited transform.  For a float64 T, sqrt(float64(k)) < T is
 *      monotone in k, so "distance < T" is out < limit(T) with limit(T) the smallest k >= 0 with sqrt(float64(k)) >= T, which the
 *      host finds once.  below (or NULL): below[x][y] = out[x][y] < limit ? 1 : 0.  work: X * Y int32 of scratch (the distances
 *      within the rows).  The rows are swept in chunks of SSLCR_EDT_ROW_CELLS cells with a carry from chunk to chunk.
 *      Errors: NULL descriptor or mask / out / work, X < 1, Y < 1, X * Y >= 2^31, X^2 + Y^2 >= 2^31 (every squared distance must
 *      fit an int32), limit < 0, invert outside {0, 1}, pointers not 4-byte aligned (the mask is read as whole dwords). */
#define SSLCR_EDT_ROW_CELLS 1024
typedef struct sslcr_edt_desc {
  const uint8_t* mask;      /* [X][Y]; 4-byte aligned */
  int32_t* out;             /* [X][Y] */
  uint8_t* below;           /* [X][Y] or NULL */
  int32_t* work;            /* [X * Y] */
  int X, Y, limit, invert;
} sslcr_edt_desc;
int sslcr_edt_squared(const sslcr_edt_desc* d, void* stream);

/*      sslcr_fill_holes.  out[x][y] = 1 where mask != 0, or where the cell's component of the BACKGROUND (mask == 0) at connectivity 1
 *      holds no cell of the array's border (row 0, row X - 1, column 0, column Y - 1); else 0.  A background cell joined to the
 *      border only diagonally is therefore filled.  The background is labelled by sslcr_label_components; labels / count / work are
 *      its outputs and scratch, of its sizes (labels [X * Y], work [X * Y + ceil(X * Y / SSLCR_LABEL_RUN_CELLS)]), and hold nothing of use afterwards.
 *      Errors: NULL descriptor or pointers, X < 1, Y < 1, X * Y >= 2^31, out == mask, pointers not 4-byte aligned. */
typedef struct sslcr_fill_desc {
  const uint8_t* mask;      /* [X][Y], nonzero = set */
  uint8_t* out;             /* [X][Y] of 0 / 1; 4-byte aligned, not mask */
  int32_t* labels;          /* [X][Y] scratch */
  int32_t* count;           /* [1] scratch */
  int32_t* work;            /* [X * Y + ceil(X * Y / SSLCR_LABEL_RUN_CELLS)] scratch */
  int X, Y;
} sslcr_fill_desc;
int sslcr_fill_holes(const sslcr_fill_desc* d, void* stream);

/*      sslcr_region_moments.  For every label l + 1 in 1..L, over the cells (x, y) with labels[x][y] == l + 1:
 *          moments[l] += (the number of cells, sum x, sum y, sum x^2, sum y^2, sum x y)
 *      int64, by integer atomics (exact, order-independent); the caller zeroes it.  Labels outside 1..L are left out.  The shape
 *      bound of sslcr_edt_squared holds here too: x, y < 46341, so every term is below 2^31 and every sum below 2^62.
 *      From these the host takes regionprops' major_axis_length in its inertia-tensor form, with A = the area:
 *          a = (A sum x^2 - (sum x)^2) / A^2,  c = (A sum y^2 - (sum y)^2) / A^2,  b = (A sum x y - sum x sum y) / A^2
 *      (exact integer numerators and denominators, each quotient rounded to float64 once),
 *          l1 = (a + c) / 2 + sqrt(((a - c) / 2)^2 + b^2),  major_axis_length = 4 sqrt(l1).
 *      Errors: NULL descriptor or labels, NULL moments with L > 0, X < 1, Y < 1, X * Y >= 2^31, X^2 + Y^2 >= 2^31, L < 0, labels not
 *      4-byte or moments not 8-byte aligned. */
typedef struct sslcr_moments_desc {
  const int32_t* labels;    /* [X][Y] */
  int64_t* moments;         /* [L][6] */
  int X, Y, L;
} sslcr_moments_desc;
int sslcr_region_moments(const sslcr_moments_desc* d, void* stream);

/* ---- Ranking metrics on the device: a radix sort, and from it the exact ROC-AUC counts (csrc/rank.hip).  The Kather main prints
 *      sklearn's roc_auc_score(targets, scores, multi_class='ovr') (eval_Kather_SSL_CR.py:658).  The area under the ROC curve of one
 *      column is the share of (positive, negative) pairs the score orders correctly, a tie counting half, so with
 *          U2 = sum over the positives i and the negatives j of (2 [s_i > s_j] + [s_i = s_j])
 *      it is U2 / (2 P N): three integers, which the device counts exactly and the host divides once.  All entries are asynchronous
 *      and use integer arithmetic only (a score is its bit pattern; there is no floating-point operation): two calls give equal bits.
 *      Work passes between workgroups at launch boundaries only: no kernel waits for another workgroup.  These entries were added
 *      without a new version number; a caller tells them by their symbols.
 *
 *      sslcr_sort_pairs.  A stable least-significant-digit radix sort of B independent rows of n uint32 keys, each with a uint32
 *      value, ascending by the bits [lo, hi) of the key: ceil((hi - lo) / 8) passes of an 8-bit digit (the last one narrower), each a
 *      per-tile digit histogram (SSLCR_SORT_TILE keys a workgroup), an exclusive scan of [digit][tile] (SSLCR_RANK_SCAN_TRIP tiles a
 *      trip, with a carry) and a stable scatter.  Keys equal in [lo, hi) keep their input order.  keys[0] / values[0] hold the input
 *      and are overwritten; the passes alternate between the two buffers and the result is in keys[p & 1] / values[p & 1], p the
 *      number of passes (lo == hi: no launch, the input is the result).  workspace: sslcr_sort_workspace_bytes(B, n) bytes of
 *      scratch (0 for arguments the sort refuses).
 *      Errors: NULL descriptor or pointers, B outside [1, 65535], n < 1, not 0 <= lo <= hi <= 32, the four buffers not distinct,
 *      pointers not 4-byte aligned. */
#define SSLCR_SORT_TILE 4096
#define SSLCR_RANK_SCAN_TRIP 64
typedef struct sslcr_sort_desc {
  uint32_t* keys[2];        /* [B][n] each */
  uint32_t* values[2];      /* [B][n] each */
  void* workspace;          /* sslcr_sort_workspace_bytes(B, n) */
  int B, n, lo, hi;
} sslcr_sort_desc;
size_t sslcr_sort_workspace_bytes(int B, int n);
int sslcr_sort_pairs(const sslcr_sort_desc* d, void* stream);

/*      sslcr_rank_keys.  scores float32 [n][C], row-major as sslcr_predict writes them (C = 1 for a vector or a map), to one sortable
 *      row per column: with b the bit pattern of scores[i][c], b = 0 if (b << 1) == 0 (so -0 ties with +0, as under a float compare),
 *          keys[c][i]   = b ^ ((b >> 31) ? 0xFFFFFFFF : 0x80000000)      unsigned order of the keys = the order of the scores
 *          values[c][i] = target[i] == positive[c] ? 1 : 0               positive NULL: positive[c] = c
 *      An element with valid[i] == 0 (valid NULL: none) gets the value 2, which sslcr_auc_counts skips.  A NaN score
 *      ((b & 0x7FFFFFFF) > 0x7F800000) on a valid element is counted into nan[c] (zeroed by this call) and gets the value 2 as well:
 *      the counts of its column are those of the other elements and claim nothing about it.
 *      Errors: NULL descriptor, scores, target, keys, values or nan, n < 1, C outside [1, 65535], scores / keys / values not 4-byte or
 *      target / positive / nan not 8-byte aligned. */
typedef struct sslcr_rank_keys_desc {
  const float* scores;      /* [n][C] */
  const int64_t* target;    /* [n] */
  const uint8_t* valid;     /* [n] or NULL */
  const int64_t* positive;  /* [C] or NULL */
  uint32_t* keys;           /* [C][n] */
  uint32_t* values;         /* [C][n] */
  int64_t* nan;             /* [C] */
  int n, C;
} sslcr_rank_keys_desc;
int sslcr_rank_keys(const sslcr_rank_keys_desc* d, void* stream);

/*      sslcr_auc_counts.  keys / values: C rows of n, every row ascending by key (sslcr_sort_pairs of what sslcr_rank_keys wrote).
 *          counts[c] = (U2, P, N, nan[c])      P / N = the elements with value 1 / 0, U2 as above over them, nan NULL: 0
 *      A run of equal keys may span any number of workgroups: a positive's pairs are A + N - Z, A the negatives before the head of its
 *      run and Z those after its tail; the exclusive count of negatives never decreases along the row, so A is its maximum over the run
 *      heads at or before the element, and Z mirrors it from the other end.  Three launches: per-block partials (SSLCR_SORT_TILE
 *      elements a block), one scan of the partials (SSLCR_RANK_SCAN_TRIP blocks a trip, with carries), one apply pass that adds each
 *      block's integer sum.  U2 <= 2 P N < 2^62.  work: sslcr_auc_workspace_bytes(C, n) bytes of scratch.
 *      Errors: NULL descriptor or keys / values / counts / work, n < 1, C outside [1, 65535], keys / values / work not 4-byte or
 *      counts / nan not 8-byte aligned. */
typedef struct sslcr_auc_desc {
  const uint32_t* keys;     /* [C][n], ascending within a row */
  const uint32_t* values;   /* [C][n]: 1 positive, 0 negative, anything else skipped */
  const int64_t* nan;       /* [C] or NULL */
  int64_t* counts;          /* [C][4] */
  int32_t* work;            /* sslcr_auc_workspace_bytes(C, n) */
  int n, C;
} sslcr_auc_desc;
size_t sslcr_auc_workspace_bytes(int C, int n);
int sslcr_auc_counts(const sslcr_auc_desc* d, void* stream);

/* ---- Pillow-exact image resize on the device (csrc/resample.hip): Image.resize(size, resample, box) of an 8-bit L or RGB image,
 *      byte for byte, for a whole batch in HBM.  Replaces the transforms.Resize(size=args.image_size) on a PIL image that every
 *      BreastPathQ validation / test patch passes through on the host (eval_BreastPathQ_SSL_CR.py:325,365, eval_BreastPathQ_SSL.py:290,
 *      319, the __getitem__ at dataset.py:575-599).  Additive, again WITHOUT a new version number: a caller tests for sslcr_resample,
 *      sslcr_resample_plan, sslcr_resample_coeffs, sslcr_resample_ksize and sslcr_resample_table_ok by symbol.
 *
 *      The definition is Pillow's Resample.c (pinned to Pillow 12.2.0 by tests/test_resize_cpu.py).  Per axis, with inSize the source
 *      length, [in0, in1) the box along the axis, outSize the target length and the filter f of support s --
 *        BOX      s = 0.5   1 if -0.5 < x <= 0.5 else 0
 *        BILINEAR s = 1     1 - |x|
 *        HAMMING  s = 1     sin(pi x) / (pi x) * (0.54f + 0.46f * cos(pi x)), 1 at x = 0   (0.54f, 0.46f: the float32 constants
 *                           Resample.c spells, widened to double)
 *        BICUBIC  s = 2     a = -0.5: ((a + 2) x - (a + 3)) x^2 + 1 for |x| < 1, (((x - 5) x + 8) x - 4) a for |x| < 2
 *        LANCZOS  s = 3     sinc(x) sinc(x / 3) on -3 <= x < 3
 *      -- everything in double, in this order:
 *        scale = filterscale = (in1 - in0) / outSize;  if (filterscale < 1) filterscale = 1
 *        support = s * filterscale;  ksize = 2 * (int)ceil(support) + 1;  ss = 1 / filterscale
 *        for xx in 0 .. outSize - 1:
 *          center = in0 + (xx + 0.5) * scale
 *          xmin = max((int)(center - support + 0.5), 0);  xmax = min((int)(center + support + 0.5), inSize) - xmin
 *          w[x] = f((x + xmin - center + 0.5) * ss), x in 0 .. xmax - 1;  ww = w[0] + w[1] + ... left to right;  if (ww != 0) w[x] /= ww
 *          k[x] = (int)(0.5 + w[x] * 2^22) if w[x] >= 0 else (int)(-0.5 + w[x] * 2^22)          (truncation toward zero)
 *          bounds[xx] = (xmin, xmax)
 *      A pass along an axis is out[xx] = clip(((sum_x in[xmin + x] * k[x]) + 2^21) >> 22, 0, 255), the shift arithmetic.  The
 *      HORIZONTAL pass runs first and is rounded to uint8; the vertical pass reads those bytes.  A pass is skipped exactly when its
 *      axis has outSize == inSize, in0 == 0 and in1 == outSize.  NEAREST is Pillow's ImagingScaleAffine (Geometry.c), a WALK per
 *      axis: xo = in0 + scale / 2; for each xx: src = min(inSize - 1, (int)xo), xo += scale.  (The closed form floor(in0 + (xx + 0.5)
 *      * scale) is NOT Pillow's: the accumulated sum rounds differently where scale is inexact; 138 of 400 random size pairs
 *      differed, none with the walk.)  Pinned without a box only: the Python layer refuses NEAREST with a box.
 *      Out of scope: RGBA / LA (Pillow premultiplies alpha), 16- and 32-bit modes, reducing_gap.
 *
 *      int32 accumulation.  sslcr_resample_table_ok holds of a table when every row has 255 * sum|k| + 2^21 < 2^31 and every
 *      |k| < 2^23.  The first makes every partial sum of a pass fit int32 in any order: |2^21 + sum over a subset of pixel * k| <=
 *      2^21 + 255 * sum|k|.  The second puts k in the signed 24-bit operand range of v_mul_i32_i24, and a pixel (< 2^8) is in it
 *      anyway, so each product is one 24-bit multiply with an exact 32-bit result (|pixel * k| < 2^31 by the first condition).  The
 *      bound derived for the five filters: the weights of a row are normalised to sum 1, so sum|w| = 1 + 2 * (the negative lobes'
 *      share); BOX, BILINEAR and HAMMING have none (sum|k| <= 2^22 + ksize / 2 from rounding).  BICUBIC and LANCZOS have them, and
 *      a window clipped at an image edge is normalised by a smaller sum: the worst rows over scales 1/600 .. 600, with and without
 *      a fractional box, reach sum|w| = 1.251 (BICUBIC) and 1.571 (LANCZOS) (tests/test_resize_cpu.py asserts < 1.5 and < 1.75):
 *      255 * 1.75 * 2^22 + 2^21 = 1.87e9 < 2^31 = 2.15e9.  The limit is sum|w| < 2.0058; a table past it is refused, not clamped. */
#define SSLCR_RESAMPLE_NEAREST 0      /* Pillow's Image.Resampling codes */
#define SSLCR_RESAMPLE_LANCZOS 1
#define SSLCR_RESAMPLE_BILINEAR 2
#define SSLCR_RESAMPLE_BICUBIC 3
#define SSLCR_RESAMPLE_BOX 4
#define SSLCR_RESAMPLE_HAMMING 5
/*      HOST-ONLY entries: no device is touched, every pointer is HOST memory.
 *      sslcr_resample_ksize: the ksize of the axis (NEAREST: 1), or -1 for an unknown filter / an empty axis.
 *      sslcr_resample_coeffs: fills k[outSize][k_stride] (k_stride >= ksize; entries past a row's xmax are 0) and bounds[outSize][2]
 *      of one axis.  NEAREST writes the gather's table: bounds[xx] = (src, 1), k[xx][0] = 2^22.  Returns 0, or -1 with NOTHING
 *      written: bad arguments, or a table that sslcr_resample_table_ok refuses.
 *      sslcr_resample_table_ok: 1 when k[outSize][k_stride] satisfies the two conditions above, else 0. */
int sslcr_resample_ksize(double in0, double in1, int outSize, int filter);
int sslcr_resample_coeffs(int inSize, double in0, double in1, int outSize, int filter, int32_t* k, int k_stride, int32_t* bounds);
int sslcr_resample_table_ok(const int32_t* k, int outSize, int k_stride);
/*      The launch.  src / dst: uint8 batches, each [N][H][W][C] (chw = 0) or [N][C][H][W] (chw = 1), C in {1, 3}, every
 *      combination; dst must not overlap src.  kx / bx: the horizontal tables, T sets of [OW][ksx] and [OW][2]; ky / by: the vertical
 *      ones, [OH][ksy] and [OH][2].  kx == bx == NULL: no horizontal pass (then OW == IW); likewise ky / by.  Both NULL: a copy
 *      between the layouts.  nearest = 1: bx / by are gather tables (k unused).  table_index: NULL (set 0 for every image) or a
 *      device int32 [N] naming the set of each image -- a batch in which every image has its own box in ONE launch.  bx_host /
 *      by_host: HOST copies of bx / by (all T sets), read by the plan only: the fused form sizes its LDS from the widest column
 *      and row range a tile reads; without them a two-pass descriptor takes the two-launch form.  workspace: the two-launch form's
 *      uint8 intermediate, sslcr_resample_plan_info.workspace_bytes of it (else unused).  form: 0 = the plan's choice, 1 / 2 force
 *      SSLCR_RESAMPLE_FUSED / _TWO_PASS for a descriptor that needs both passes (an error where the plan says fused does not fit,
 *      and for a descriptor that needs one pass or none).  N == 0 returns 0 and launches nothing.
 *      The device tables must be what sslcr_resample_coeffs wrote: the kernels clamp every range they read to the image and to
 *      their LDS tile, so a wrong table gives wrong bytes but no access outside the buffers.
 *
 *      Forms (sslcr_resample_plan_info.form):
 *        FUSED       one launch; a workgroup of 256 owns tile_h x tile_w output pixels of one image: it stages the source rows and
 *                    columns the tile reads into LDS with whole-dword loads, runs the horizontal pass from LDS into LDS as rounded
 *                    bytes (planar, four pixels per lane and dword), barrier, runs the vertical pass from LDS (one dword per tap
 *                    and lane, the coefficient uniform over a row of lanes) and stores whole dwords: 4 pixels of a plane (CHW) or 4
 *                    RGB pixels = 3 dwords (HWC).  The tile's slices of the four tables sit in LDS.  The intermediate never leaves the CU.
 *        TWO_PASS    a horizontal launch into `workspace` (planar [N][C][IH][OW]), then a vertical launch: every descriptor whose
 *                    fused tile would exceed SSLCR_RESAMPLE_LDS_CAP (large down-scales: ksize and the row range grow with the scale).
 *        HORIZONTAL / VERTICAL   the one launch of a descriptor that needs one pass.
 *        GATHER      NEAREST, and the copy.
 *      Every form is integer arithmetic only and returns the same bytes.  Work passes between workgroups at launch boundaries only. */
#define SSLCR_RESAMPLE_GATHER 0
#define SSLCR_RESAMPLE_FUSED 1
#define SSLCR_RESAMPLE_TWO_PASS 2
#define SSLCR_RESAMPLE_HORIZONTAL 3
#define SSLCR_RESAMPLE_VERTICAL 4
#define SSLCR_RESAMPLE_LDS_CAP 65536   /* dynamic LDS the fused kernel may ask of the launcher: two workgroups per CU at the least */
typedef struct sslcr_resample_desc {
  const uint8_t* src;
  uint8_t* dst;
  const int32_t* kx; const int32_t* bx; const int32_t* ky; const int32_t* by;
  const int32_t* table_index;
  const int32_t* bx_host; const int32_t* by_host;
  uint8_t* workspace;
  int N, C, IH, IW, OH, OW, ksx, ksy, T;
  int src_chw, dst_chw, nearest, form;
} sslcr_resample_desc;
typedef struct sslcr_resample_plan_info {
  int form;                 /* SSLCR_RESAMPLE_* the launch takes */
  int fused_ok;             /* 1: form = 1 (fused) is accepted for this descriptor */
  int tile_w, tile_h;       /* FUSED: output pixels of a workgroup's tile (else 0) */
  int rows, cols;           /* FUSED: the most source rows / columns a tile stages (else 0) */
  int grid[2];              /* workgroups of the (first, second) launch; 0 = no such launch */
  size_t lds_bytes;         /* dynamic LDS of the launch (FUSED only, <= SSLCR_RESAMPLE_LDS_CAP) */
  size_t workspace_bytes;   /* TWO_PASS only */
} sslcr_resample_plan_info;
/* HOST-ONLY: what sslcr_resample would launch for this descriptor (the device pointers are not read, only their NULL-ness).
 * -1 for a descriptor sslcr_resample refuses. */
int sslcr_resample_plan(const sslcr_resample_desc* d, sslcr_resample_plan_info* out);
int sslcr_resample(const sslcr_resample_desc* d, void* stream);

/* ---- k-nearest-neighbour feature probe on the device (csrc/knn.hip): a fused fp32 similarity and top-k, the vote over the
 *      neighbours, and the row normalisation cosine similarity needs.  The reference's train() functions return final_feats,
 *      final_targets for a t-SNE plot (pretrain_BreastPathQ.py:89-92, :322-340); the quantitative form of that plot is a k-NN probe
 *      of the embeddings.  Additive, again WITHOUT a new version number: a caller tests for sslcr_knn_plan, sslcr_knn_topk,
 *      sslcr_knn_vote and sslcr_l2_normalize by symbol.  Every entry is asynchronous; none synchronises with the host.
 *
 *      sslcr_knn_topk.  queries Q [nq][D] and bank B [nb][D], contiguous float32, D % 4 == 0, 4 <= D <= 2048, both 16-byte aligned.
 *      For every query i the k (1 <= k <= 64) admissible bank rows j with the greatest similarity s(i, j) = sum_d Q[i][d] B[j][d], best
 *      first, into scores [nq][k] and indices [nq][k].  The nq x nb similarities never reach memory.
 *        Arithmetic: v_mfma_f32_16x16x4_f32; every s(i, j) is accumulated over d = 0 .. D - 1 in RISING order from a +0 accumulator,
 *        one rounding per product-and-add: an fmaf chain in d order.  A ragged last chunk of D is padded with zeros for both operands.
 *        The value therefore does not depend on the tile, on the slice count or on the route: two plans return equal bits.
 *        Order: a TOTAL order on integers.  A candidate's 64-bit key is (score key << 32) | ~j: the score key is that of
 *        sslcr_rank_keys (b ^ 0x80000000 for b >= 0, ~b for b < 0, -0 tied to +0; csrc/score_key.hpp is the one definition), so a
 *        greater score is a greater key and of two equal scores the LOWER bank index is.  A NaN score gets the score key 1, below
 *        that of -inf (0x007FFFFF): it ranks below every number, NaNs among themselves by index, and is returned as the NaN
 *        0x7FC00000.  A score of -0 is returned as +0.  The key 0 is the empty slot.
 *        Admissible: j < nb_valid (0 <= nb_valid <= nb restricts the search to a prefix of the bank; bank tiles wholly past it are not
 *        walked, but the plan, and so the slices, are those of nb: a caller with nb_valid far below nb does better to state nb_valid as nb), and j != i + self_offset when
 *        self_offset >= 0 (-1: none): leave-one-out for queries that are rows self_offset .. of the bank.  With fewer than k admissible
 *        rows the trailing slots hold index -1 and score -inf.
 *        Launches: (1) grid = query tiles x S bank slices; a workgroup owns SSLCR_KNN_TILE queries and walks its slice in tiles of
 *        SSLCR_KNN_TILE bank rows: operands staged through LDS as whole rows, D in chunks of SSLCR_KNN_CHUNK, 2 x 2 accumulator tiles
 *        a wave; the tile's scores pass through LDS to the selection, one wave per 16 queries: a query's 64 candidates, one per lane,
 *        are tested against its current k-th key by ballot, and only where one passes are they sorted over the lanes (bitonic) and
 *        merged into the query's sorted list (one slot per lane).  Each (tile, slice) writes k keys per query to `workspace`.
 *        (2) one wave per query merges the S lists the same way and writes scores and indices.  Work passes between workgroups at
 *        the launch boundary only: no tickets, no look-back, no spinning, no floating-point atomics.
 *      sslcr_knn_plan: HOST-ONLY, usable without a device: the tile shape, S, the workspace bytes and the form of (nq, nb, D, k);
 *      slices_hint > 0 asks for that S (honoured up to the bank's tile count and SSLCR_KNN_MAX_SLICES; a trailing slice may then be
 *      empty), 0 lets the plan choose: the chip holds 512 of the first launch's workgroups at a time (two a CU), so the grid runs in
 *      rounds of 512, and the plan takes the smallest S whose rounds are at least 95 % full, else the fullest -- never fewer than 4
 *      bank tiles a slice, no empty slice.  For few queries that is as many slices as the bank allows; the second launch reads the
 *      (sorted) slice lists backwards, so a slice costs a query one 6-exchange merge.  The launch, the Python layer and the tests
 *      read this plan.  -1 for arguments sslcr_knn_topk refuses.
 *      Errors: NULL descriptor or pointers, nq < 0 (nq == 0: nothing is launched), nb < 1 or >= 2^31 - 64, D, k outside their ranges, ceil(nq / 64) * S >= 2^31,
 *      nb_valid outside [0, nb], self_offset < -1, slices < 0, queries / bank not 16-byte, workspace not 8-byte or scores / indices not
 *      4-byte aligned. */
#define SSLCR_KNN_TILE 64          /* queries of a workgroup = bank rows of a tile */
#define SSLCR_KNN_CHUNK 64         /* elements of D per LDS stage */
#define SSLCR_KNN_MAX_K 64
#define SSLCR_KNN_MAX_D 2048
#define SSLCR_KNN_MAX_SLICES 1024
#define SSLCR_KNN_DIRECT 0         /* form: one slice, the second launch only decodes */
#define SSLCR_KNN_SLICED 1         /* form: S > 1 slices, the second launch merges them */
typedef struct sslcr_knn_desc {
  const float* queries;     /* [nq][D] */
  const float* bank;        /* [nb][D] */
  float* scores;            /* [nq][k] */
  int32_t* indices;         /* [nq][k] */
  void* workspace;          /* sslcr_knn_plan_info.workspace_bytes */
  int nq, nb, D, k;
  int nb_valid;             /* rows [0, nb_valid) of the bank are searched */
  int self_offset;          /* >= 0: query i ignores bank row i + self_offset; -1: none */
  int slices;               /* the plan's slices_hint */
} sslcr_knn_desc;
typedef struct sslcr_knn_plan_info {
  int form;                 /* SSLCR_KNN_DIRECT | SSLCR_KNN_SLICED */
  int tile_q, tile_b, chunk;
  int slices;               /* S */
  int tiles_per_slice;      /* bank tiles a slice walks; slice s starts at bank row s * tiles_per_slice * tile_b */
  int grid[2];              /* workgroups of the (first, second) launch */
  size_t lds_bytes;         /* static LDS of the first launch's workgroup */
  size_t workspace_bytes;   /* S * nq * k keys of 8 bytes */
} sslcr_knn_plan_info;
int sslcr_knn_plan(int nq, int nb, int D, int k, int slices_hint, sslcr_knn_plan_info* out);
int sslcr_knn_topk(const sslcr_knn_desc* d, void* stream);

/*      sslcr_l2_normalize.  y[i][:] = x[i][:] / max(||x[i]||, eps), torch.nn.functional.normalize(x, dim = 1), one wave per row: the
 *      squares are summed in float64 in a fixed order (lane l takes elements l, l + 64, ...; then a butterfly over the lanes), the
 *      root is taken in float64 and rounded to float32 once, the maximum with eps is taken in float32, and every element is ONE
 *      correctly rounded float32 division.  y may alias x.
 *      Errors: NULL descriptor or pointers, n < 0 (n == 0: nothing is launched), D < 1, eps not >= 0, pointers not 4-byte aligned. */
int sslcr_l2_normalize(const float* x, float* y, int n, int D, float eps, void* stream);

/*      sslcr_knn_vote.  What a k-NN classifier or regressor makes of sslcr_knn_topk's output, one thread per query; a slot with index
 *      -1 (or outside [0, nb)) takes no part, nor does a neighbour whose label lies outside [0, C).
 *        UNIFORM  votes[i][c] = the number of neighbours with label c; pred[i] = the class with the most, a tie going to the LOWEST
 *                 class: sklearn's KNeighborsClassifier(weights = "uniform") (pinned to sklearn 1.7.2 by tests/test_knn_cpu.py).
 *        SOFTMAX  votes[i][c] = sum over the neighbours with label c, in rank order in float32, of expf((s - s_0) / temperature), s_0
 *                 the row's best score (slot 0): the weighted vote of DINO / InstDisc; the shift changes no ratio.  pred as above.
 *        REGRESS  pred_value[i] = (sum of the neighbours' targets, in rank order in float32) / their number; votes, pred unused.
 *      confusion (classification, optional): int64 [C][C], rows = query_labels; cell (query_labels[i], pred[i]) += 1 by integer
 *      atomics, counted per workgroup first as sslcr_predict does; it accumulates across calls.  A query without a neighbour
 *      predicts class 0 with all votes 0 (REGRESS: NaN).
 *      Errors: NULL descriptor, indices, or the mode's inputs / outputs, nq < 0 (0: nothing launched), k outside [1, 64], nb < 1, a
 *      classification C outside [1, 64], mode outside the three, SOFTMAX without scores or with temperature not > 0, confusion without
 *      query_labels, 8-byte tensors not 8-byte or 4-byte tensors not 4-byte aligned. */
#define SSLCR_KNN_VOTE_UNIFORM 0
#define SSLCR_KNN_VOTE_SOFTMAX 1
#define SSLCR_KNN_VOTE_REGRESS 2
typedef struct sslcr_knn_vote_desc {
  const int32_t* indices;   /* [nq][k] */
  const float* scores;      /* [nq][k]; SOFTMAX only (else may be NULL) */
  const int64_t* labels;    /* [nb] bank labels (classification) */
  const float* targets;     /* [nb] bank targets (REGRESS) */
  const int64_t* query_labels;  /* [nq] or NULL */
  int64_t* pred;            /* [nq] (classification) */
  float* pred_value;        /* [nq] (REGRESS) */
  float* votes;             /* [nq][C] (classification) */
  int64_t* confusion;       /* [C][C] or NULL */
  int nq, k, nb, C, mode;
  float temperature;
} sslcr_knn_vote_desc;
int sslcr_knn_vote(const sslcr_knn_vote_desc* d, void* stream);

/* ---- t-SNE embedding on the device (csrc/tsne.hip): what every main() of the reference does with final_feats after its best epoch,
 *      TSNE().fit_transform(final_feats) (pretrain_BreastPathQ.py:322-340), without the plot.  Two components, one degree of freedom,
 *      squared Euclidean distances, k <= 64 neighbours (sslcr_knn_topk's cap; sklearn takes 3 * perplexity + 1 = 91 at its default),
 *      an EXACT repulsive sum over all pairs.  tests/_tsne_ref.py is the float64 restatement, pinned to sklearn 1.7.2.  Additive,
 *      WITHOUT a new version number: a caller tests for sslcr_tsne_plan, sslcr_tsne_pair_dist2, sslcr_tsne_affinities,
 *      sslcr_tsne_repulsion, sslcr_tsne_update and sslcr_tsne_kl by symbol.  Every entry is asynchronous; none synchronises.
 *
 *      sslcr_tsne_pair_dist2.  dist2[i][r] = sum_d (x[i][d] - x[j][d])^2 for j = indices[i][r]: x float32 [n][D], every difference
 *      exact in float64, every square one float64 rounding, the sum one float64 rounding per term in RISING d, the result rounded to
 *      float32 once.  An index outside [0, n) gives +inf.  One thread per (i, r).
 *
 *      sslcr_tsne_affinities.  sklearn/manifold/_utils.pyx, _binary_search_perplexity, statement by statement: dist2 float32 [n][k]
 *      (1 <= k <= 64), P float32 [n][k] and beta float64 [n] out.  Per row: beta = 1, at most 100 steps of
 *      P_j = exp(-d_j beta), s = sum P (1e-8 if 0), P_j /= s, H = log(s) + beta sum d_j P_j, stop when |H - log(perplexity)| <= 1e-5,
 *      else double / halve / bisect beta as sklearn does.  float64 inside.  One wave per row, one neighbour per lane; both sums are
 *      xor-butterflies over the 64 lanes (lanes >= k hold 0): a fixed tree, every lane ends with the same bits.
 *
 *      sslcr_tsne_repulsion.  sklearn/manifold/_t_sne.py, _kl_divergence: q_ij = 1 / (1 + |y_i - y_j|^2), the self pair left out BY
 *      INDEX (coincident points count with q = 1).  Grid = row tiles (SSLCR_TSNE_TILE rows, one a thread) x S column slices; a
 *      workgroup stages SSLCR_TSNE_CHUNK points of y as float2 in LDS and every lane reads the same address.  Per lane, in float32 and
 *      RISING j: (sum q, sum q^2 dx, sum q^2 dy), q by v_rcp_f32; the three go to workspace[(i * S + s)] as one float4.  An empty
 *      slice writes zeros.  A second launch of ONE workgroup folds the n * S values of sum q into the float64 Z in a fixed order
 *      (thread t takes t, t + 1024, ...; then a tree).  No floating-point atomics, no tickets, no spins.
 *
 *      sslcr_tsne_update.  One wave per row i.  rep_i = the S partials folded in float64 in rising s; attr_i = sum over the row's CSR
 *      entries of p_ij q_ij (y_i - y_j) in float64 (lanes stride over the entries, then the butterfly); grad_i = 4 (exaggeration
 *      attr_i - rep_i / Z), written as float32.  kl_rows (optional): sum_j p_ij log(p_ij / max(q_ij / Z, DBL_EPSILON)) of the row.
 *      With y_out (sklearn/manifold/_t_sne.py, _gradient_descent, one iteration, float64 from the float32 state, each result
 *      rounded once): inc = update * grad < 0; gains = inc ? gains + 0.2 : gains * 0.8, floored at min_gain; update = momentum *
 *      update - lr * gains * grad; y_out = y + update.  y_out must not be y (other rows still read y).  y_out NULL: gradient only.
 *
 *      sslcr_tsne_kl.  One workgroup: log_row[0] = sum of kl_rows, [1] = |grad|_2, [2] = Z, [3] = iteration, float64, fixed order.
 *
 *      sslcr_tsne_plan: HOST-ONLY: tile, chunk, S, chunks per slice and workspace bytes of n points; slices_hint > 0 asks for that S
 *      (up to the chunk count and SSLCR_TSNE_MAX_SLICES), 0 lets the plan fill the chip (1024 workgroups).  2 <= n <= 2^20.
 *      Errors: NULL descriptor or tensors, n outside [2, 2^20], k outside [1, 64], D < 1, perplexity not > 0, slices < 0,
 *      y_out == y, float2 / float4 / float64 tensors not 8- / 16- / 8-byte aligned, others not 4-byte. */
#define SSLCR_TSNE_TILE 256        /* rows of a repulsion workgroup, one a thread */
#define SSLCR_TSNE_CHUNK 1024      /* points of y per LDS stage */
#define SSLCR_TSNE_MAX_SLICES 64
#define SSLCR_TSNE_MAX_N 1048576
#define SSLCR_TSNE_LOG_COLS 4
typedef struct sslcr_tsne_plan_info {
  int tile, chunk;
  int slices;               /* S */
  int chunks_per_slice;     /* slice s covers columns [s * chunks_per_slice * chunk, ...) */
  int grid[3];              /* workgroups of the repulsion launch (row tiles * S), of the Z fold (1) and of the update */
  size_t lds_bytes;
  size_t workspace_bytes;   /* n * S float4 */
} sslcr_tsne_plan_info;
typedef struct sslcr_tsne_grad_desc {
  const float* y;           /* [n][2] */
  float* y_out;             /* [n][2] or NULL (gradient only) */
  float* update;            /* [n][2] */
  float* gains;             /* [n][2] */
  float* grad;              /* [n][2] out */
  const int32_t* rowptr;    /* [n + 1] */
  const int32_t* col;
  const float* val;
  void* workspace;          /* sslcr_tsne_plan_info.workspace_bytes */
  double* Z;                /* [1] */
  double* kl_rows;          /* [n] or NULL */
  int n, slices;            /* slices: the plan's slices_hint */
  int nnz;                  /* entries col / val hold: rowptr is clamped to it */
  double exaggeration, momentum, lr, min_gain;   /* sklearn's are float64 */
} sslcr_tsne_grad_desc;
int sslcr_tsne_plan(int n, int slices_hint, sslcr_tsne_plan_info* out);
int sslcr_tsne_pair_dist2(const float* x, const int32_t* indices, float* dist2, int n, int D, int k, void* stream);
int sslcr_tsne_affinities(const float* dist2, float* P, double* beta, int n, int k, float perplexity, void* stream);
int sslcr_tsne_repulsion(const sslcr_tsne_grad_desc* d, void* stream);
int sslcr_tsne_update(const sslcr_tsne_grad_desc* d, void* stream);
int sslcr_tsne_kl(const double* kl_rows, const float* grad, const double* Z, double* log_row, int n, int iteration, void* stream);

/* ---- linear probe on the device (csrc/linprobe.hip): value and gradient of a linear classifier's loss over FIXED features, fused.
 *      The reference's `--modules 64` mode ("fine-tune only classifier", eval_Kather_SSL.py:229, :358-370) trains
 *      FinetuneResNet.classifier = nn.Linear(768, num_classes) on a frozen backbone: with the features fixed that is multinomial
 *      logistic regression (ridge regression for BreastPathQ's MSE), a convex problem whose cost is the repeated evaluation below.
 *      Additive, WITHOUT a new version number: a caller tests for sslcr_linprobe_plan, sslcr_linprobe_eval and sslcr_linprobe_logits
 *      by symbol.  Every entry is asynchronous; none synchronises with the host.
 *
 *      sslcr_linprobe_eval.  X [n][D] contiguous float32, D % 4 == 0, 4 <= D <= 2048, 16-byte aligned, 1 <= n < 2^31 - 64; W [C][D] and
 *      b [C] float32, 1 <= C <= 64; s_i = sample_weight[i] (float32 [n]; NULL: 1).  For the one point (W, b):
 *        value   one float64: sum_i s_i l_i / sum_i s_i;
 *        grad    float64 [C][D + 1]: the gradient of value in W (columns 0 .. D - 1) and in b (column D);
 *        logits  optionally float32 [n][C].
 *      The DATA term only: a penalty is the caller's host arithmetic.
 *        SSLCR_LINPROBE_SOFTMAX  labels int64 [n]; l_i = logsumexp(z_i) - z_{i, y_i}.  A row whose label lies OUTSIDE [0, C) contributes
 *                                nothing -- not to the value, not to the gradient -- and is LEFT OUT of sum_i s_i (its logits are
 *                                still written).  C = 1 is accepted (l_i = 0).
 *        SSLCR_LINPROBE_SQUARED  targets float32 [n][C]; l_i = 1/2 sum_c (z_ic - t_ic)^2.
 *      With sum_i s_i = 0 (every row left out or weighted 0) value and grad are 0 / 0 = NaN.
 *        Arithmetic.  Logit: v_mfma_f32_16x16x4_f32; z_ic is accumulated over d = 0 .. D - 1 in RISING order from a +0 accumulator, one
 *        rounding per product-and-add -- an fmaf chain in d order (D is padded to a multiple of 16 with zero products, which change no
 *        value) -- and then z_ic = chain + b[c], one float32 addition.  The value does not depend on the plan.  (tests/test_linprobe_gpu.py
 *        holds a logit to the BITS of that chain; the row order of the gradient's chains is held by bounds only, not by bits.)
 *        Softmax: in float32 with the accurate expf / logf: m = max_c z_ic; e_c = expf(z_ic - m); S = sum_c e_c (eight partial sums,
 *        classes c = j, j + 8, ... in rising c, then a 3-step butterfly); l_i = logf(S) + (m - z_{i, y_i}), the two summands added in
 *        float64; squared loss: differences, squares and their sum in float64 from the float32 z and t.  The row's term is
 *        s_i * l_i in float64.
 *        Residual: r_ic = s_i * (e_c / S - [c == y_i]) (softmax) or s_i * (z_ic - t_ic) (squared), formed in float64 from those float32
 *        values and rounded to float32 ONCE.
 *        Gradient: a workgroup owns a contiguous range of row tiles; every element sum_i r_ic x_id (and sum_i r_ic for column D) is ONE
 *        fp32 chain over the rows that workgroup owns in RISING row order (v_mfma_f32_16x16x4_f32 again; a plain float32 addition
 *        chain for column D), kept in accumulators across the workgroup's tiles.  The loss terms of a tile are summed in float64 by a
 *        fixed butterfly and added to the workgroup's float64 sums in rising tile order.
 *        Fold: the per-workgroup partials -- C (D + 1) floats, and the two float64 sums (s_i l_i and s_i) -- are folded by a SECOND
 *        launch in float64 in rising workgroup order, then divided by sum_i s_i (one float64 division each).
 *        Work passes between workgroups at the launch boundary only: no floating-point atomics, no tickets, no spinning, every loop
 *        states its bound.  Two calls with the same plan give equal bits.
 *        Launches: (0) W is repacked into `workspace`, rows padded to the MFMA block with zeros, in the operand order of the first
 *        product (C is padded to 16 / 32 / 64 in registers and in this scratch copy only, never in the caller's tensors); (1) grid =
 *        G workgroups x S column slices, 256 threads, tiles of SSLCR_LINPROBE_TILE rows; (2) the fold.
 *        Forms, chosen by the plan from D alone:
 *          SSLCR_LINPROBE_STAGED    the row tile [32][D] fits LDS (D <= 1024): it is fetched from memory ONCE, staged once, and serves both
 *                                   products -- X is read once per evaluation;
 *          SSLCR_LINPROBE_STREAMED  wider D: the tile passes through SSLCR_LINPROBE_CHUNK columns of LDS (two alternating stages of 256),
 *                                   once for the logits and once more for the gradient; the second read is of lines the workgroup
 *                                   has just fetched.
 *        In both forms the 256 columns of the next stage (or of the next tile's first) are in flight while a stage's MFMAs run.
 *        The gradient accumulators of a workgroup hold at most 32 blocks of 16 x 16 a wave; where ceil(C / 16) * ceil(D / 16) exceeds
 *        what four waves hold (C > 16 and D > 1024, C > 32 and D > 512) the columns are cut into S <= 4 slices, one workgroup each,
 *        and every slice repeats the first product; slice 0 alone writes logits, loss terms and column D.
 *      sslcr_linprobe_plan: HOST-ONLY, usable without a device: tile rows, G, tiles per workgroup, S, form, chunk, LDS bytes and
 *      workspace bytes of (n, D, C, loss).  groups_hint > 0 FORCES G (up to the tile count and SSLCR_LINPROBE_MAX_GROUPS; a trailing
 *      workgroup may then own no tile and writes zero partials); 0 lets the plan choose: as many workgroups as the chip holds at once
 *      (256 CUs x the 1 or 2 its LDS admits -- from LDS ALONE: whether the registers of the wider accumulator shapes also admit two
 *      a CU has not been measured, so where they do not the grid runs in two rounds), so that the dirty partials stay at a few hundred x C (D + 1) floats and never become
 *      one set per tile, rebalanced so that no workgroup is empty.  The launch, the Python layer and the tests read this plan.
 *      -1 for arguments sslcr_linprobe_eval refuses.
 *      sslcr_linprobe_logits: the first product alone, for queries: logits [n][C] = the SAME chain and addition, so its bits equal the
 *      `logits` output of sslcr_linprobe_eval.  Reads x, w, b, logits, workspace, n, D, C, groups of the descriptor.
 *      Errors: NULL descriptor or pointers (x, w, b, workspace; eval: value, grad, and labels / targets by loss; logits: logits), n, D,
 *      C outside their ranges, loss outside the two, groups < 0, x / workspace not 16-byte, labels / value / grad not 8-byte, the
 *      other tensors not 4-byte aligned. */
#define SSLCR_LINPROBE_SOFTMAX 0
#define SSLCR_LINPROBE_SQUARED 1
#define SSLCR_LINPROBE_STAGED 0    /* form: the whole row tile in LDS, X read once */
#define SSLCR_LINPROBE_STREAMED 1  /* form: chunks of columns, X read twice (the second time from cache) */
#define SSLCR_LINPROBE_TILE 32     /* rows of a tile */
#define SSLCR_LINPROBE_CHUNK 512   /* columns of LDS the streamed form passes a tile through */
#define SSLCR_LINPROBE_MAX_C 64
#define SSLCR_LINPROBE_MAX_D 2048
#define SSLCR_LINPROBE_MAX_GROUPS 1024
typedef struct sslcr_linprobe_desc {
  const float* x;               /* [n][D] */
  const float* w;               /* [C][D] */
  const float* b;               /* [C] */
  const int64_t* labels;        /* [n], SOFTMAX */
  const float* targets;         /* [n][C], SQUARED */
  const float* sample_weight;   /* [n] or NULL */
  double* value;                /* one float64 */
  double* grad;                 /* [C][D + 1] float64 */
  float* logits;                /* [n][C] or NULL (sslcr_linprobe_logits: required) */
  void* workspace;              /* sslcr_linprobe_plan_info.workspace_bytes */
  int n, D, C;
  int loss;                     /* SSLCR_LINPROBE_SOFTMAX | SSLCR_LINPROBE_SQUARED */
  int groups;                   /* the plan's groups_hint */
} sslcr_linprobe_desc;
typedef struct sslcr_linprobe_plan_info {
  int form;                     /* SSLCR_LINPROBE_STAGED | SSLCR_LINPROBE_STREAMED */
  int tile_rows;
  int groups;                   /* G */
  int tiles_per_group;          /* workgroup g owns tiles [g * tiles_per_group, ...) */
  int col_slices;               /* S */
  int chunk;                    /* columns of X resident in LDS (STAGED: D padded to 16) */
  int class_blocks;             /* ceil(C / 16) rounded to 1, 2 or 4: the padding, in registers only */
  int grid[3];                  /* workgroups of the (repack, evaluation, fold) launches */
  size_t lds_bytes;             /* dynamic LDS of the evaluation's workgroup */
  size_t workspace_bytes;
} sslcr_linprobe_plan_info;
int sslcr_linprobe_plan(int n, int D, int C, int loss, int groups_hint, sslcr_linprobe_plan_info* out);
int sslcr_linprobe_eval(const sslcr_linprobe_desc* d, void* stream);
int sslcr_linprobe_logits(const sslcr_linprobe_desc* d, void* stream);

/* ---- device-side strong augmentation, the colour ops of the reference's RandAugment pool ("next" row f4) on a uint8 batch in HBM.
 *      As with sslcr_weak_augment the random draws stay on the host, in the reference's order (ssl_cr_histo_amd/augment.py);
 *      the kernels are the deterministic per-pixel arithmetic.
 *
 *      sslcr_hed_colour_augment: models/randaugment.py:17-48 colour_augmentation() -- rgb2hed, per-image shift of the three stain
 *      channels, hed2rgb, (x * 255).astype(uint8) -- in float64, operation for operation as scikit-image 0.15.0 (requirements.txt:369)
 *      computes it (see csrc/augment.hip); replaces the reference's per-pixel Python loop (:35-38). */
typedef struct sslcr_colour_aug_desc {
  const uint8_t* src;       /* [N][3][H][W] (hwc=0, what the stem ingests) or [N][H][W][3] (hwc=1, the PIL/numpy layout) */
  uint8_t* dst;             /* same layout; may alias src */
  const double* shift;      /* [N][3] device doubles: (hmod, dmod, emod) of :30-32 */
  const uint8_t* apply;     /* [N] or NULL: 0 = the image is copied unchanged (RandAugment did not pick this op for it) */
  double hed_from_rgb[9];   /* row-major 3x3: skimage.color.hed_from_rgb = inv(rgb_from_hed) */
  double rgb_from_hed[9];
  int N, H, W, hwc;
} sslcr_colour_aug_desc;
int sslcr_hed_colour_augment(const sslcr_colour_aug_desc* d, void* stream);
/*      sslcr_brightness_contrast: models/randaugment.py:93-103 Brightness() / Contrast() = albumentations 0.1.8
 *      (requirements.txt:10) RandomBrightnessContrast: clip(float32(img) * alpha + beta * mean(img), 0, max(img)).astype(uint8),
 *      mean and max over the whole image. */
typedef struct sslcr_brightness_contrast_desc {
  const uint8_t* src; uint8_t* dst;      /* [N][3][H][W] or [N][H][W][3]: the map is layout-blind; dst may alias src */
  const double* alpha_beta; /* [N][2] device doubles: alpha = 1 + contrast draw, beta = brightness draw */
  const uint8_t* apply;     /* [N] or NULL */
  unsigned long long* stats;/* workspace [N][2] (sum, max), zeroed by the call */
  int N, H, W;
} sslcr_brightness_contrast_desc;
int sslcr_brightness_contrast(const sslcr_brightness_contrast_desc* d, void* stream);

/* ---- device-side RandAugment of the RSP v2 pipeline (library version >= 7): the Pillow ops of Pretraining_v2/models/randaugment.py
 *      (augment_pool(), :176-190) on a uint8 batch in HBM, replacing the per-tile PIL chain of RandAugment.__call__ (:203-213) that
 *      Pretraining_v2/dataset.py:85-95 runs on the host for the three tiles of every triplet.  One call serves ONE op slot of a whole
 *      batch: image n takes op[n] with its own parameters; SSLCR_AUGV2_COPY passes it through.  The random draws stay on the host, in
 *      the reference's order (ssl_cr_histo_amd/augment.py); the kernels are deterministic and equal Pillow byte for byte
 *      (csrc/augment_v2.hip spells out the arithmetic).  Reference lines per code: */
#define SSLCR_AUGV2_COPY 0            /* identity() :38-41 */
#define SSLCR_AUGV2_BRIGHTNESS 1      /* brightness() :52-57, ImageEnhance.Brightness(img).enhance(factor) */
#define SSLCR_AUGV2_CONTRAST 2        /* contrast() :44-49, ImageEnhance.Contrast */
#define SSLCR_AUGV2_COLOR 3           /* color() :160-165, ImageEnhance.Color */
#define SSLCR_AUGV2_AUTOCONTRAST 4    /* autocontrast() :147-157, ImageOps.autocontrast */
#define SSLCR_AUGV2_EQUALIZE 5        /* equalize() :168-172, ImageOps.equalize */
#define SSLCR_AUGV2_SHARPNESS 6       /* sharpness() :60-65, ImageEnhance.Sharpness (blend with ImageFilter.SMOOTH) */
#define SSLCR_AUGV2_NEAREST_FIXED 7   /* rotate() :68-74, Image.rotate: Pillow's 16.16 fixed-point nearest walk, fill 0 */
#define SSLCR_AUGV2_NEAREST_TABLE 8   /* translate_x() / translate_y() :77-94: Pillow's scale path (per-image index tables), fill 0 */
#define SSLCR_AUGV2_BICUBIC 9         /* shear_x() / shear_y() :97-122: Image.transform(AFFINE, BICUBIC) in float64, fill 0 */
typedef struct sslcr_augv2_desc {
  const uint8_t* src;       /* [N][3][H][W] (src_hwc=0) or [N][H][W][3] (src_hwc=1, what the v2 dataset holds) */
  uint8_t* dst;             /* [N][3][H][W] (dst_hwc=0, what the stem ingests) or [N][H][W][3]; must NOT alias src */
  const int32_t* op;        /* [N] device ints: SSLCR_AUGV2_* */
  const float* factor;      /* [N] device floats: the enhance() factor float32(val / 10 * 1.8 + 0.1) of the four ImageEnhance ops */
  const int32_t* fixed;     /* [N][6] device ints a0..a5 for NEAREST_FIXED: out(x, y) = in((a2 + a0 x + a1 y) >> 16, (a5 + a3 x + a4 y) >> 16);
                               NULL when ops_mask has no such op */
  const double* shift;      /* [N][2] device doubles (px, py) for NEAREST_TABLE: the a2 / a5 of the AFFINE tuple (1, 0, px, 0, 1, py); or NULL */
  const double* affine;     /* [N][6] device doubles a0..a5 for BICUBIC: xin = a0 (x + 0.5) + a1 (y + 0.5) + a2, yin likewise; or NULL */
  uint32_t* hist;           /* workspace [N][3][256], zeroed by the call; needed when ops_mask has CONTRAST / AUTOCONTRAST / EQUALIZE */
  unsigned long long* lsum; /* workspace [N], likewise */
  uint8_t* lut;             /* workspace [N][3][256]; needed when ops_mask has BRIGHTNESS or one of the three above */
  int32_t* tab;             /* workspace [N][W + H]; needed when ops_mask has NEAREST_TABLE: per image the source column of every output
                               column, then the source row of every output row, -1 = outside (built on the device from shift) */
  unsigned ops_mask;        /* bit (1 << code) set for every code that occurs in op[]: the host planned the slot and knows */
  int N, H, W, src_hwc, dst_hwc;
} sslcr_augv2_desc;
int sslcr_randaug_v2_slot(const sslcr_augv2_desc* d, void* stream);

/*      sslcr_randaug_v2_colour (library version >= 11): the two histopathology ops of the same pool, hed() :135-144 and hsv() :125-132,
 *      IN PLACE on a uint8 batch in HBM: image n takes op[n] with row n of param; SSLCR_AUGV2C_COPY leaves it untouched (its workgroups
 *      exit at once).  op[] lives on the device, so the entry cannot read it: it refuses an ops_mask with a bit outside the three codes
 *      ("unknown op"), and the kernels treat like COPY every op[n] outside the three codes and every op[n] whose bit ops_mask lacks
 *      (a HED image without the HED bit is NOT summed and NOT changed; bsum is then never read).  The class issues it on the output of the slot call, which passed
 *      these images through as SSLCR_AUGV2_COPY.  The host makes the draws of augmentor.randomize() (augment.py); the kernels are the
 *      deterministic arithmetic (csrc/augment_v2.hip spells it out).  With HED in ops_mask a byte-sum pass (integer atomics) runs first
 *      over the HED images, for the cutoff test of HedColorAugmenter.transform; then one apply pass.  Reference lines per code: */
#define SSLCR_AUGV2C_COPY 0           /* not picked for this image */
#define SSLCR_AUGV2C_HED 1            /* hed() :135-144 = HedColorAugmenter.transform (models/augmenters/color/hedcoloraugmenter.py:149-207) on
                                         models/augmenters/color/utils/custom_hed_transform.py:8-37, float32: x = float32(u8 * (1/255)) + 2,
                                         stains = -log(x) . hed_from_rgb, stain_j = stain_j * param[j] + param[3 + j], rgb = exp(-stains . rgb_from_hed) - 2,
                                         rescale_intensity(in_range=(-1, 1)), clip to [0, 1], * 255, truncate.  An image whose mean / 255 lies
                                         outside [cutoff_lo, cutoff_hi] is left as it is (:162-163) */
#define SSLCR_AUGV2C_HSV 2            /* hsv() :125-132 = HsbColorAugmenter.transform (models/augmenters/color/hsbcoloraugmenter.py:80-125), float64:
                                         scikit-image 0.15.0 rgb2hsv, h = (h + param[0]) % 1, s *= 1 + param[1] (param[1] < 0) or
                                         s *= 1 + (1 - s) param[1] (> 0), hsv2rgb, * 255, truncate */
typedef struct sslcr_augv2_colour_desc {
  uint8_t* img;             /* [N][3][H][W] (hwc=0) or [N][H][W][3] (hwc=1), modified in place */
  const int32_t* op;        /* [N] device ints: SSLCR_AUGV2C_* */
  const double* param;      /* [N][6] device doubles.  HED: float32(1 + sigma_j) for j = h, e, d, then float32(bias_j), each widened to double;
                               HSV: (sigma_hue % 1.0, sigma_saturation), the rest unused */
  unsigned long long* bsum; /* workspace [N], zeroed by the call; needed when ops_mask has HED */
  double cutoff_lo, cutoff_hi;   /* HED: the cutoff_range of :141, (0.15, 0.85) */
  float hed_from_rgb[9];    /* row-major 3x3 float32, as custom_hed_transform.py:8-11 builds them: inv(rgb_from_hed) and rgb_from_hed */
  float rgb_from_hed[9];
  unsigned ops_mask;        /* bit (1 << code) set for every code that occurs in op[] */
  int N, H, W, hwc;
} sslcr_augv2_colour_desc;
int sslcr_randaug_v2_colour(const sslcr_augv2_colour_desc* d, void* stream);

/* ---- device-side RandAugment of the consistency-training pipeline, the six OpenCV-style ops of models/randaugment.py:51-110 (HSV,
 *      Noise, Scale_Resize_Crop, Shift_Scale_Rotate, Blur_img, Rotate_Crop) on a uint8 RGB batch in HBM.  The library version stays
 *      16: the entries are told by their symbols.  One call serves ONE op slot of a whole batch: image n takes op[n] with row n of
 *      the parameter tables; SSLCR_AUGV1_COPY, or apply[n] == 0, passes it through (only the layout may change).  The random draws
 *      stay on the host, in the reference's order (ssl_cr_histo_amd/augment.py); the kernels are deterministic (no floating-point
 *      atomics, no spins, no host reads: two calls give equal bits).
 *
 *      The arithmetic below IS the definition.  It is written after OpenCV 3.4.2, albumentations 0.1.8 and imgaug 0.4.0, none of
 *      which can be run here: PARITY UNPINNED against all three.  tests/_cv_ref.py restates it in NumPy and is held to scipy,
 *      colorsys and torch; the kernels are held to the restatement, bit for bit except where stated.
 *
 *      REFLECT_101 of an index p into a length n: n == 1 -> 0; else m = p mod (2n - 2) (non-negative), m >= n -> 2n - 2 - m.  This
 *      is the repeated reflection of cv::borderInterpolate in closed form.
 *
 *      The cubic: A = -0.75, float32, every operation rounded on its own, for a fraction x:
 *        c0 = ((A (x + 1) - 5A) (x + 1) + 8A) (x + 1) - 4A;  c1 = ((A + 2) x - (A + 3)) x x + 1  (left to right);
 *        c2 = c1 at (1 - x);  c3 = 1 - c0 - c1 - c2  (left to right).
 *
 *      1. BLUR (Blur_img -> cv2.blur, k in {3, 5, 7}): per channel the integer sum over the k x k window centred on the pixel,
 *         indices through REFLECT_101; out = (2 sum + k k) / (2 k k) in integers (k k is odd: no tie).
 *      2. HSV (HSV -> shift_hsv): forward, OpenCV's 8-bit integer form with h in 0..179: v = max, diff = v - min,
 *         s = (diff sdiv[v] + 2048) >> 12, h = (g - b) if v == r, else (b - r + 2 diff) if v == g, else (r - g + 4 diff);
 *         h = (h hdiv[diff] + 2048) >> 12 (arithmetic shift), + 180 if negative; sdiv[i] = rint((255 << 12) / i),
 *         hdiv[i] = rint((180 << 12) / (6 i)) in float64, entry 0 of both = 0.  The shifts are the integers rint(draw):
 *         h += dh, then h = 255 - h where h < 0, then h -= 255 where h > 255 (the library's own wrap on the uint8 maximum, kept);
 *         s and v are clipped to 0..255.  Back, float32, + - x only: hf = float(h) (6.f / 180.f), - 6 while >= 6; sector = floor,
 *         f = hf - sector; s, v scaled by (1.f / 255.f); tab = {v, v (1 - s), v (1 - s f), v (1 - s (1 - f))}; the sector table
 *         {{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}} picks (b, g, r); each channel is rint(x 255.f) saturated.
 *      3. WARP (Rotate, ShiftScaleRotate -> cv2.warpAffine(INTER_CUBIC, BORDER_REFLECT_101)): dparam row = the six doubles M0..M5 of
 *         the INVERSE map (the host builds getRotationMatrix2D's matrix and inverts it in the library's order).  Per output pixel
 *         X = (sat32(rint((M1 y + M2) 1024)) + 16 + sat32(rint(M0 x 1024))) >> 5 in float64 with one rounding per operation, Y likewise
 *         from M4, M5, M3; sx = X >> 5, sy = Y >> 5, phase = (Y & 31) 32 + (X & 31); 16 taps at (sx - 1 + kx, sy - 1 + ky), each index
 *         through REFLECT_101 and then, where the flip pair (fx, fy) = iparam[0..1] is set, mirrored (W - 1 - x / H - 1 - y): the
 *         flip precedes the warp.  out = saturate((sum tap w[phase][4 ky + kx] + 16384) >> 15).  The host keeps
 *         |M0| (W - 1) + |M1| (H - 1) + |M2| and its Y counterpart below 32000 (OpenCV's maps are 16-bit), so X, Y fit 32 bits.
 *         The weight table w[1024][16] (sslcr_cv_warp_table): phase fy 32 + fx from the cubic at fy / 32 and fx / 32,
 *         entry = saturate_short(rint(float32(cy cx) 32768.f)); the residual r = sum - 32768 is subtracted from the largest (r < 0) or
 *         the smallest (r > 0) of the four CENTRE entries [1..2][1..2], scanned row-major, the first extreme winning, and the result
 *         is stored as the low 16 bits.  Entry 5 (the tap at (sx, sy); its weight is never negative) is READ AS UNSIGNED: at phase 0
 *         it holds 32768, the unit tap, which a signed read would turn into -32768.  Every other entry is read signed.
 *      4. RESIZE (RandomScale, Resize -> cv2.resize(INTER_CUBIC)): per axis f = float32((d + 0.5) (double(src) / double(dst)) - 0.5),
 *         s = floor(f), four taps at s - 1 .. s + 2 clamped to the image, coefficients saturate_short(rint(c 2048.f)) of the cubic at
 *         f - s (float32); horizontal pass in integers, vertical pass out = saturate((sum + (1 << 21)) >> 22); no antialiasing.
 *         Scale_Resize_Crop is resize S -> S', resize S' -> S + 20, crop S at (y1, x1): iparam row = (S', y1, x1) with
 *         1 <= S' <= work_smax and 0 <= y1, x1 <= 20; H == W is required.  Two launches: the first writes the S' x S' image into the
 *         uint8 workspace (planar), the second computes only the cropped window of the second resize.
 *      5. NOISE (Noise -> imgaug AdditiveGaussianNoise(per_channel=False)): one normal per pixel, shared by the three channels:
 *         out = clip(x + rint(double(sigma) double(z)), 0, 255), sigma = dparam[0].  The stream is this project's, NOT imgaug's:
 *         Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85), key = the image's 64-bit seed
 *         (iparam[0] the low, iparam[1] the high word), counter = (pixel_index >> 2, 0, 0, 0); from the words w0..w3,
 *         u1 = ((w >> 8) + 1) 2^-24 and u2 = (w >> 8) 2^-24; Box-Muller in float32, r = sqrt(-2 log u1), (r cos 2 pi u2, r sin 2 pi u2)
 *         from (w0, w1) for pixels 4q and 4q + 1 and from (w2, w3) for 4q + 2 and 4q + 3.  The integer stream is exact
 *         (sslcr_augv1_philox shows it); log, cos and sin are the device's float32 functions, so sigma z may differ from another
 *         float32 library's in the last bits and a pixel whose sigma z lies within 1e-3 of a half-integer may differ by one. */
#define SSLCR_AUGV1_COPY 0
#define SSLCR_AUGV1_BLUR 1            /* iparam[0] = k */
#define SSLCR_AUGV1_HSV 2             /* iparam[0..2] = (dh, ds, dv) */
#define SSLCR_AUGV1_WARP 3            /* dparam[0..5] = M0..M5 (inverse map), iparam[0..1] = (fx, fy) */
#define SSLCR_AUGV1_RESIZE 4          /* iparam[0..2] = (S', y1, x1) */
#define SSLCR_AUGV1_NOISE 5           /* dparam[0] = sigma, iparam[0..1] = the seed's low and high word */
typedef struct sslcr_augv1_desc {
  const uint8_t* src;       /* [N][3][H][W] (src_hwc=0) or [N][H][W][3] (src_hwc=1) */
  uint8_t* dst;             /* [N][3][H][W] (dst_hwc=0) or [N][H][W][3]; must NOT alias src */
  const int32_t* op;        /* [N] device ints: SSLCR_AUGV1_* */
  const uint8_t* apply;     /* [N] or NULL: 0 = the image is passed through like COPY */
  const int32_t* iparam;    /* [N][4] device ints, per code as above; NULL when ops_mask has only COPY */
  const double* dparam;     /* [N][6] device doubles (WARP, NOISE); or NULL */
  const int16_t* wtab;      /* [1024][16] device int16, what sslcr_cv_warp_table builds (WARP); or NULL */
  uint8_t* work;            /* workspace of sslcr_augv1_workspace_bytes(N, H, ...) bytes (RESIZE); or NULL */
  int work_smax;            /* the largest S' the workspace holds per image: 3 * work_smax^2 bytes, rounded up to 16 */
  unsigned ops_mask;        /* bit (1 << code) set for every code that occurs in op[]: the host planned the slot and knows.  An image
                               whose code is unknown, or whose tables are NULL, or whose S' / y1 / x1 / k leave their ranges, is
                               written BLACK instead of reading through a bad pointer */
  int N, H, W, src_hwc, dst_hwc;
} sslcr_augv1_desc;
int sslcr_randaug_v1_slot(const sslcr_augv1_desc* d, void* stream);
/* host only: the 1024 x 16 weight table of WARP into table (32 KiB of host memory) */
int sslcr_cv_warp_table(int16_t* table);
/* host only: bytes of the RESIZE workspace for N images of S x S whose scale draws stay <= max_scale (S' <= int(S max_scale));
   0 on bad arguments */
size_t sslcr_augv1_workspace_bytes(int N, int S, double max_scale);
/* the Philox words of NOISE: words[4 i + j] = word j at counter (first + i, 0, 0, 0) under key seed, i < count; words on the device */
int sslcr_augv1_philox(unsigned long long seed, uint32_t first, int count, uint32_t* words, void* stream);

/* ==================================================================================================
 * Engine: the whole ResNet18 TripletNet(_Finetune)+head graph, forward / backward / update, orchestrated
 * natively (one C call per step).  Replaces the step bodies of the reference's train()/validate():
 *   eval_BreastPathQ_SSL_CR.py:65-100, eval_Camelyon_SSL_CR.py:94-121, eval_Kather_SSL_CR.py:56-105,
 *   pretrain_BreastPathQ.py:42-61 and :110-128, eval_Camelyon_SSL.py:52-98, eval_BreastPathQ_SSL.py:52-84.
 * ================================================================================================== */
typedef struct sslcr_ctx sslcr_ctx;
typedef struct sslcr_net sslcr_net;

int sslcr_create(sslcr_ctx** out, int device, int dtype);
int sslcr_destroy(sslcr_ctx* ctx);
/* one process per GPU: rank 0 makes the 256-byte id pair, the host broadcasts it (torch.distributed), every rank inits.
 * With a communicator: gradients are all-reduced (bucketed, overlapped with backward) and train-mode BatchNorm uses
 * GLOBAL batch statistics (all-reduce of per-channel sums), which is what makes N ranks equal the single-device
 * reference (the reference's nn.DataParallel BN is per-replica, eval_BreastPathQ_SSL_CR.py:474-477). */
int sslcr_comm_unique_id(void* id256);       /* two 128-byte RCCL ids: [0] BatchNorm sums (compute stream), [1] gradient buckets (side stream) */
int sslcr_comm_init(sslcr_ctx* ctx, const void* id256, int rank, int world);
/* what the communicator itself reports (ncclCommUserRank / ncclCommCount when RCCL is in use): rank, world, transport
 * (0 none, 1 RCCL, 2 virtual ranks) -- bench.py prints it as ranks_seen. */
int sslcr_comm_info(sslcr_ctx* ctx, int* rank, int* world, int* transport);
/* in-place SUM of `n` floats over the ranks of ctx's communicator (RCCL or virtual) on `stream`; nothing happens without one.
 * The logging reduction of the step functions: per-rank loss shares -> global values, once per print_freq / epoch end (the
 * reference's meters, eval_BreastPathQ_SSL_CR.py:103-110, read .item() of losses nn.DataParallel had already gathered). */
int sslcr_comm_all_reduce_f32(sslcr_ctx* ctx, float* buf, size_t n, void* stream);
/* "Virtual ranks" (test infrastructure for single-GPU boxes; RCCL refuses two ranks on one device): `world` contexts of ONE
 * process on ONE device, one host thread and one stream each, exchange through a sslcr_vcomm instead of RCCL.  Every sharded
 * code path of the engine -- synced BatchNorm sums forward and backward, global-count loss scaling, bucketed gradient sums on
 * the side stream with their event joins -- runs exactly as with RCCL; only the transport differs (device-to-device copy +
 * rank-ordered sum kernel behind a host rendezvous, asynchronous on the callers' streams).  The nn.DataParallel seam this
 * replaces: eval_BreastPathQ_SSL_CR.py:474-477. */
typedef struct sslcr_vcomm sslcr_vcomm;
int sslcr_vcomm_create(sslcr_vcomm** out, int world);
int sslcr_vcomm_destroy(sslcr_vcomm* v);
int sslcr_comm_init_virtual(sslcr_ctx* ctx, sslcr_vcomm* v, int rank);
/* on (default): synced BatchNorm as described above.  off: every rank normalises with its own shard's statistics -- the
 * semantics of the reference's nn.DataParallel replicas -- and only the gradient buckets are exchanged. */
int sslcr_set_bn_sync(sslcr_ctx* ctx, int on);
/* on: sslcr_step_ssl_cr runs the (frozen, eval-mode) teacher forward on a second HIP stream next to the student forward --
 * the workgroups of one fill the tail rounds of the other's kernels (measured -0.4 ms of a 20.4 ms step in round 1; in round 6,
 * five boxes: together with sslcr_set_wgrad_stream every box runs the step in 15.5-15.6 ms where the serial step takes 15.2-15.75 ms
 * by box -- a gain on slow boxes, a loss on fast ones).  Off by default.
 * Forced off while sslcr_profile() is on: concurrent launches share the CUs, which makes per-kernel durations meaningless as a
 * statement about the kernel, and bench.py's roofline is built from those. */
int sslcr_set_aux_stream(sslcr_ctx* ctx, int on);
/* on: in backward the weight-gradient launches run on a second HIP stream behind an event -- they depend only on a
 * BatchNorm-backward output and feed only the gradient buffer, and they are MFMA-bound while the chain they leave behind
 * alternates MFMA-bound dgrads with HBM-bound BatchNorm passes.  Results are bit-identical.  OFF by default: measured
 * neutral on MI355X (18.84 vs 18.76 ms/step) -- the 4096-workgroup elementwise kernels fill every wave slot of the CUs, so
 * the 512-thread wgrad workgroups do not become co-resident and the two streams serialise.  Forced off while
 * sslcr_profile() is on. */
int sslcr_set_wgrad_stream(sslcr_ctx* ctx, int on);

/* measurement: bracket every conv launch of this ctx with HIP events on its own stream (bench.py roofline leg).
 * which = 0: conv_igemm (forward + dgrad), 1: wgrad.  out4 = {launches, total ms, algorithmic FLOPs, algorithmic bytes}.
 * sslcr_profile(ctx, 1) also clears the previous records. */
int sslcr_profile(sslcr_ctx* ctx, int enable);
int sslcr_profile_read(sslcr_ctx* ctx, int which, double* out4);
/* per kernel template instance: lines "name|launches|total_ms|algorithmic_flops|algorithmic_bytes" (names as rocprofv3 prints them) */
int sslcr_profile_dump(sslcr_ctx* ctx, char* buf, size_t n);

typedef struct sslcr_net_desc {
  float* const* params;                    /* [nparams] device pointers, named_parameters() order of models/net.py:
                                              0..59 resnet18 backbone, 60..63 fc.0/fc.2, then the classifier (2 or 4) */
  int nparams;
  float* const* bn_running_mean;           /* [20] in graph order */
  float* const* bn_running_var;
  int64_t* const* bn_num_batches_tracked;
  const uint8_t* requires_grad;            /* [nparams] host flags (freeze-by-index, eval_BreastPathQ_SSL_CR.py:408-441) */
  int head_kind;                           /* 0 FinetuneResNet 768->C (models/net.py:107-115); 1 Classifier 768->128->C (:8-20) */
  int num_classes;
  int triplet;                             /* 0 TripletNet_Finetune (models/net.py:70-103); 1 TripletNet (:25-66) */
} sslcr_net_desc;
int sslcr_net_create(sslcr_ctx* ctx, const sslcr_net_desc* d, sslcr_net** out);
int sslcr_net_destroy(sslcr_net* net);
int sslcr_net_set_requires_grad(sslcr_net* net, const uint8_t* flags);
/* re-derive the shadow weights from the bound fp32 parameters: mode bit0 = train packs (KRSC + dgrad CRSK),
 * bit1 = eval packs (BatchNorm running stats folded into KRSC weights + bias). Call after any parameter change.
 * SSLCR_FP8 contexts: mode 3 also drops the calibrated activation scales -- the first forward of the net in each mode (train,
 * eval) after sslcr_net_create or after a mode-3 pack runs the backbone TWICE (a calibration pass at scale 1 that only records
 * amax -- running statistics untouched, synced-BatchNorm all-reduces included -- then the real pass), so time steps after it. */
int sslcr_net_pack(sslcr_net* net, int mode, void* stream);

/* forward.  x2/x3 only for triplet nets.  train=0: eval-mode BN (folded), nothing saved.  train=1: batch-stat BN,
 * running stats updated (x3 for TripletNet_Finetune), activations kept for sslcr_net_backward. */
int sslcr_net_forward(sslcr_net* net, int train, const void* x1, const void* x2, const void* x3, int in_f32,
                      int N, int H, int W, float* feats, float* logits, void* stream);
/* backward of the last train forward from d(loss)/d(logits); zeroes then fills the engine's gradient buffer;
 * all-reduces it when a communicator is set. */
int sslcr_net_backward(sslcr_net* net, const float* dlogits, void* stream);
/* library version >= 9.  Gradient accumulation -- loss.backward() without a preceding optimizer.zero_grad(), i.e. autograd's
 * `.grad +=`: k micro-batches, one optimizer step.  Sticky: applies to every later backward of this net (sslcr_net_backward and the
 * backward leg of sslcr_step_ssl_cr / sslcr_step_supervised).
 *   off (0, the default): the behaviour and the launches described above, nothing added.
 *   on: after the backward the gradient buffer holds prev + new, elementwise in fp32 (sslcr_grad_accumulate), where prev is what the
 *       buffer held when the backward was entered -- also a gradient an optimizer step has already consumed: as in torch, nothing is
 *       cleared for the caller -- and new is what this backward alone would have left.  The backward writes `new` into a second flat
 *       buffer (allocated at the first accumulating backward); the sum is taken on `stream` after the bucket all-reduces and the
 *       side-stream weight gradients have been joined into it, so sharded ranks add identical buffers and need no further
 *       collective (every micro-step still all-reduces its own gradient: correct by linearity).  Only the range from the lowest
 *       trainable parameter to the end of the buffer is cleared, written and added: a frozen prefix costs nothing and stays zero.
 *       A net that has had no backward since sslcr_net_create has no prev: its first backward behaves as off.
 * The sum lives in the buffer sslcr_net_grad, sslcr_net_grad_norm and the optimizer entries read: they see it unchanged. */
int sslcr_net_set_grad_accumulate(sslcr_net* net, int on);
/* library version >= 10.  The options of the loss leg of sslcr_step_ssl_cr (the student's) and sslcr_step_supervised (train = 0: the
 * weighted validation loss).  Sticky, like sslcr_net_set_grad_accumulate; NULL sets the defaults, with which the steps issue the
 * launches they have always issued (sslcr_loss's kernel, which expects every target to be a class id: a row labelled -100 is left
 * out only once an option, or a stats / denominator pointer, is set).  The struct is copied; the device memory its pointers name stays the
 * caller's and must live until the last step that uses it has run.  A step of an MSE kind (0, 3) on a net with non-default options
 * is an error, as is an option sslcr_loss_ex refuses for the net's class count. */
int sslcr_net_set_loss_opts(sslcr_net* net, const sslcr_loss_opts* opts);
int sslcr_net_grad(sslcr_net* net, int param_index, float* out, void* stream);      /* -> PyTorch layout */
/* diagnostics for the layer-wise backward parity test (tests/test_backward_replay_gpu.py): autograd of one BasicBlock of
 * torchvision resnet18 (reached from models/net.py:32,77) checked kernel by kernel at the size the step really runs.  With the tap
 * on, sslcr_net_backward keeps a copy of every block's transient gradient tensors of every pass (the three TripletNet branches);
 * sslcr_net_debug_tensor copies one tensor of block 0..7 (layer1.0 .. layer4.1) into `out` (device memory, engine storage dtype,
 * NHWC) and reports its dims.  The pass rides in the high bits of `kind`: kind | pass << 8 (pass 0: the kinds as they always were;
 * a pass the last train-mode forward did not have is an error).  The weight packs (15..20) are the same for every pass.
 *   kind 0 G     = d(block output) * (output > 0)           1 dRaw2 = gradient at conv2's raw output (after bn2 backward)
 *        2 dAct1 = conv2's dgrad (flags bit 0: bn1's ReLU mask already applied)    3 dRaw1 = gradient at conv1's raw output
 *        4 dRawD = gradient at the projection conv's raw output                    5 dXin  = gradient at the block input
 *        6 raw1, 7 raw2, 8 rawd (saved raw conv outputs), 9 y (block output), 10 x (block input)
 *       11..14 bn1's saved scale, shift, mean, invstd (fp32 [C]; dims = {C,1,1,1})
 *       15..20 (library version >= 8) the train-mode shadow weights as the conv kernels read them, engine storage dtype: conv1's
 *              forward pack [K][R][S][C] (15) and dgrad pack [C][R][S][K] (16), conv2's (17, 18), the projection's (19, 20)
 *       21..24 bn2's saved scale, shift, mean, invstd; 25..28 the projection BatchNorm's (as 11..14)
 *       29 dOut = the gradient at the block output as bn2's backward reduce pass reads it (layer4.1's comes from the average pool)
 *       (21..29 and the pass bits came without a version bump: a library that lacks them refuses the kind.)
 * flags: which form each stage of this block took in the last step --
 *   bit 0 dAct1 carries bn1's ReLU mask            1 the BatchNorm backward passes ran the branches as segments of one launch
 *       2 conv2's masked dgrad ran them as segments     3 conv2's weight gradient ran them as one batched launch
 *       4 bn2 and the projection BatchNorm's backward ran as the paired kernels     5 the stride-2 dgrad ran its four parity classes
 *       in one launch (bits 0..5: the last backward)   6 the forward ran the branches as segments     7 conv1 and the projection
 *       ran as the paired stride-2 launch (6, 7: the last train-mode forward).
 *   The profiler cannot tell these apart (profiling switches the segment forms off).  The tap changes no routing decision and no output bit.
 * out == NULL: only dims4 / flags are filled. */
int sslcr_net_debug_tap(sslcr_net* net, int on);
/* 1 when the last train-mode forward of a TripletNet ran its three branches as segments of one launch per layer
 * (sslcr_conv_desc.seg_images; bf16, unsharded), 0 when it ran them pass by pass */
int sslcr_net_segments_used(const sslcr_net* net);
int sslcr_net_debug_tensor(sslcr_net* net, int block, int kind, void* out, size_t out_bytes, int* dims4, int* flags, void* stream);
/* fused multi-tensor update of every requires_grad parameter; state1/state2 = per-parameter optimizer state
 * (exp_avg/exp_avg_sq or momentum_buffer) owned by the caller, NULL entries for frozen parameters */
int sslcr_net_optimizer_step(sslcr_net* net, const sslcr_opt_desc* o, float* const* state1, float* const* state2, void* stream);
/* library version >= 8.  The same step for a torch optimizer with several param groups (e.g. backbone / head learning rates, no
 * weight decay on BatchNorm and bias), torch.optim.AdamW (kind 2) and torch.nn.utils.clip_grad_norm_ in front of optimizer.step():
 * groups[group_of_param[i]] is the row of parameter i (named_parameters() order; ignored for frozen parameters; NULL = all 0).  The
 * descriptor table is rebuilt when the state pointers, the trainable set or the group map changed.  clip: NULL = off (the launches
 * and the arithmetic of sslcr_net_optimizer_step); else the global 2-norm of the gradient buffer is taken on `stream` in front of
 * the update (sslcr_grad_norm) and every gradient is scaled by min(1, max_norm / (norm + 1e-6)).  The buffer is complete at that
 * point -- sslcr_net_backward returns with the bucket all-reduces and the side-stream weight gradients joined into its stream --
 * so sharded ranks reduce identical buffers in the same order and hold identical bits: no further collective. */
typedef struct sslcr_clip_desc {
  float max_norm;
  float* out2;            /* optional device [2]: receives {norm, coef} of this step */
} sslcr_clip_desc;
int sslcr_net_optimizer_step_groups(sslcr_net* net, const sslcr_opt_desc* groups, int ngroups, const int* group_of_param,
                                    float* const* state1, float* const* state2, const sslcr_clip_desc* clip, void* stream);
/* {norm, coef} (sslcr_grad_norm) of the gradients the last sslcr_net_backward left, over exactly the elements sslcr_net_grad exposes
 * for the requires_grad parameters: frozen parameters' ranges and the 64-element padding between parameters are zero in the flat
 * buffer (it is cleared before every backward and only trainable parameters' ranges are written). */
int sslcr_net_grad_norm(sslcr_net* net, float max_norm, float* out2_dev, void* stream);
int sslcr_net_lookahead(sslcr_net* net, float* const* cached, float alpha, void* stream);   /* lookahead.py:93-97 */
int sslcr_net_ema_from(sslcr_net* teacher, sslcr_net* student, float decay, void* stream);  /* decay 0 == deepcopy (:515-516) */

typedef struct sslcr_ssl_cr_desc {
  int kind;                 /* 0 mse+mse (BreastPathQ) ; 1 ce + hard-pseudo-label ce (Camelyon, Kather) */
  const void* x_student;    /* [nx+nu,3,H,W]: labeled then strong-augmented unlabeled (torch.cat at :82) */
  const void* x_teacher;    /* [nu,3,H,W]: weak-augmented unlabeled */
  int in_f32, nx, nu, H, W;
  const float* target_f; const int64_t* target_i;
  float lambda_u;
  int nx_global, nu_global; /* global batch counts (== nx, nu on one GPU) */
  float* feats;             /* [nx+nu,768] out */
  float* logits;            /* [nx+nu,C] out */
  float* logits_t;          /* [nu,C] out */
  float* losses;            /* [4] out: loss, loss_x, loss_u, #correct */
  int backward;
  const void* x_student2;   /* optional: then x_student holds only the nx labeled images and x_student2 the nu strong-augmented
                               unlabeled ones (the concatenation of :82 happens in the stem kernel's addressing) */
} sslcr_ssl_cr_desc;
int sslcr_step_ssl_cr(sslcr_net* teacher, sslcr_net* student, const sslcr_ssl_cr_desc* d, void* stream);

typedef struct sslcr_sup_desc {
  int kind;                 /* 2 cross-entropy ; 3 mse */
  const void* x1; const void* x2; const void* x3;   /* x2,x3: TripletNet (RSP) only */
  int in_f32, n, H, W;
  const float* target_f; const int64_t* target_i;
  int n_global;
  float* feats; float* logits; float* losses;
  int train;                /* 1: train-mode BN ; 0: validate() */
  int backward;
} sslcr_sup_desc;
int sslcr_step_supervised(sslcr_net* net, const sslcr_sup_desc* d, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* SSLCR_H_ */
