"""ctypes binding of libsslcr.so -- the C-ABI declared in include/sslcr.h.

There is NO fallback: if the HIP library is missing or a call fails, this raises.  ``import torch`` must
precede loading so that the process uses a single HIP runtime (torch's libamdhip64.so.7 soname).
"""
import ctypes as C
import os

import torch  # noqa: F401  (loads libamdhip64 / librccl first)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libsslcr.so")

vp, i32, f32, f64, sz = C.c_void_p, C.c_int, C.c_float, C.c_double, C.c_size_t


class SslcrError(RuntimeError):
    pass


MIRRORS = {}     # C struct name in include/sslcr.h -> its ctypes mirror: the one place a descriptor is registered (engine.py adds its three)


def _S(cname, pyname, fields):
    """the ctypes mirror of the header's struct cname, registered in MIRRORS under that name; tests/test_abi_cpu.py holds every entry
    to the header's size and field offsets, and MIRRORS' keys to the header's structs"""
    assert cname not in MIRRORS, cname
    MIRRORS[cname] = type(pyname, (C.Structure,), {"_fields_": fields})
    return MIRRORS[cname]


SwitchRow = _S("sslcr_switch_row", "SwitchRow", [(k, C.c_char_p) for k in ("name", "group", "rule", "when", "meaning")] +
               [("dflt", C.c_longlong), ("value", C.c_longlong), ("is_set", i32)])
ConvDesc = _S("sslcr_conv_desc", "ConvDesc", [("x", vp), ("w", vp), ("y", vp), ("in_scale", vp), ("in_shift", vp), ("bias", vp),
                           ("residual", vp), ("stats", vp)] +
              [(k, i32) for k in ("N", "H", "W", "C", "K", "R", "S", "stride", "pad", "PH", "PW", "OH", "OW", "osh",
                                  "transposed", "in_relu", "relu", "accumulate", "pix_mul", "pix_off_h", "pix_off_w")] +
              [("tap_mask", C.c_uint), ("mask_x", vp), ("mask_scale", vp), ("mask_shift", vp), ("mask_mean", vp),
               ("par4", i32), ("seg_images", i32), ("seg_stride", i32), ("out_scale", vp)])
WgradDesc = _S("sslcr_wgrad_desc", "WgradDesc", [("x", vp), ("dy", vp), ("dw", vp), ("in_scale", vp), ("in_shift", vp), ("in_relu", i32)] +
               [(k, i32) for k in ("N", "H", "W", "C", "K", "R", "S", "stride", "pad", "OH", "OW", "seg_images", "seg_stride")])
StemDesc = _S("sslcr_stem_desc", "StemDesc", [("x", vp), ("w", vp), ("y", vp), ("bias", vp), ("stats", vp)] +
              [(k, i32) for k in ("N", "H", "W", "OH", "OW", "in_f32", "relu")] + [("x2", vp), ("n_split", i32), ("out_scale", vp)])
StemWgradDesc = _S("sslcr_stem_wgrad_desc", "StemWgradDesc", [("x", vp), ("dy", vp), ("dw", vp)] +
                   [(k, i32) for k in ("N", "H", "W", "OH", "OW", "in_f32")] + [("x2", vp), ("n_split", i32)])
BnFinalizeDesc = _S("sslcr_bn_finalize_desc", "BnFinalizeDesc", [("partials", vp), ("rows", i32), ("C", i32), ("count", f64), ("gamma", vp),
                                       ("beta", vp), ("scale", vp), ("shift", vp), ("mean", vp), ("invstd", vp),
                                       ("running_mean", vp), ("running_var", vp), ("num_batches_tracked", vp),
                                       ("momentum", f32), ("eps", f32), ("replay", i32), ("sums_out", vp),
                                       ("sums_in", vp), ("stage", vp), ("nseg", i32), ("seg_stride", i32), ("tickets", vp)])
BnActDesc = _S("sslcr_bn_act_desc", "BnActDesc", [("x", vp), ("scale", vp), ("shift", vp), ("res", vp), ("rscale", vp), ("rshift", vp),
                             ("y", vp), ("pixels", sz), ("C", i32), ("relu", i32), ("nseg", i32), ("seg_stride", i32), ("ybits", vp)])
PoolFwdDesc = _S("sslcr_pool_fwd_desc", "PoolFwdDesc", [("x", vp), ("scale", vp), ("shift", vp), ("y", vp), ("argmax", vp)] +
                 [(k, i32) for k in ("N", "H", "W", "C", "OH", "OW")])
PoolBwdDesc = _S("sslcr_pool_bwd_desc", "PoolBwdDesc", [("dy", vp), ("argmax", vp), ("x", vp), ("scale", vp), ("shift", vp), ("dx", vp)] +
                 [(k, i32) for k in ("N", "H", "W", "C", "OH", "OW")])
BnBwdDesc = _S("sslcr_bn_bwd_desc", "BnBwdDesc", [("dy", vp), ("x", vp), ("yact", vp), ("scale", vp), ("shift", vp), ("mean", vp),
                             ("invstd", vp), ("sums", vp), ("dx", vp), ("gout", vp), ("pixels", sz), ("C", i32),
                             ("relu_from_x", i32), ("count", f64), ("pool_dy", vp), ("pool_argmax", vp), ("pH", i32),
                             ("pW", i32), ("pOH", i32), ("pOW", i32), ("pool_y", vp), ("g_in_reduce", i32), ("dgamma", vp), ("dbeta", vp),
                             ("pg_scale", f32), ("nseg", i32), ("seg_stride", i32), ("sums_stride", i32), ("yact_bits", vp)])
LossDesc = _S("sslcr_loss_desc", "LossDesc", [("kind", i32), ("logits", vp), ("logits_t", vp), ("target_f", vp), ("target_i", vp),
                           ("dlogits", vp), ("out", vp), ("nx", i32), ("nu", i32), ("C", i32), ("lambda_u", f32),
                           ("inv_nx_global", f32), ("inv_nu_global", f32)])
LossOpts = _S("sslcr_loss_opts", "LossOpts", [("class_weight", vp), ("label_smoothing", f32), ("ignore_index", i32), ("threshold", f32),
                           ("temperature", f32), ("denominator", vp), ("stats", vp)])
TensorDesc = _S("sslcr_tensor_desc", "TensorDesc", [("p", vp), ("g", vp), ("s1", vp), ("s2", vp), ("n", i32), ("K", i32), ("C", i32),
                               ("RS", i32), ("w_fwd", vp), ("w_dgrad", vp), ("pack_dtype", i32), ("dgrad_flip", i32),
                               ("group", i32)])
OptDesc = _S("sslcr_opt_desc", "OptDesc", [("kind", i32), ("lr", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("wd", f32),
                         ("momentum", f32), ("bc1", f32), ("bc2", f32), ("first_step", i32), ("grad_scale", f32)])
ClipDesc = _S("sslcr_clip_desc", "ClipDesc", [("max_norm", f32), ("out2", vp)])
MAX_OPT_GROUPS = 8
WeakAugDesc = _S("sslcr_weak_aug_desc", "WeakAugDesc", [("src", vp), ("dst", vp), ("params", vp)] +
                 [(k, i32) for k in ("N", "SH", "SW", "OH", "OW", "src_hwc")])
ColourAugDesc = _S("sslcr_colour_aug_desc", "ColourAugDesc", [("src", vp), ("dst", vp), ("shift", vp), ("apply", vp), ("hed_from_rgb", f64 * 9),
                                     ("rgb_from_hed", f64 * 9), ("N", i32), ("H", i32), ("W", i32), ("hwc", i32)])
BrightnessContrastDesc = _S("sslcr_brightness_contrast_desc", "BrightnessContrastDesc", [("src", vp), ("dst", vp), ("alpha_beta", vp), ("apply", vp), ("stats", vp),
                                                       ("N", i32), ("H", i32), ("W", i32)])
AugV2Desc = _S("sslcr_augv2_desc", "AugV2Desc", [(k, vp) for k in ("src", "dst", "op", "factor", "fixed", "shift", "affine", "hist", "lsum", "lut", "tab")] +
                [("ops_mask", C.c_uint)] + [(k, i32) for k in ("N", "H", "W", "src_hwc", "dst_hwc")])
AugV2ColourDesc = _S("sslcr_augv2_colour_desc", "AugV2ColourDesc", [("img", vp), ("op", vp), ("param", vp), ("bsum", vp), ("cutoff_lo", f64), ("cutoff_hi", f64),
                                         ("hed_from_rgb", f32 * 9), ("rgb_from_hed", f32 * 9), ("ops_mask", C.c_uint)] +
                      [(k, i32) for k in ("N", "H", "W", "hwc")])
AUGV1_OPS = ("copy", "blur", "hsv", "warp", "resize", "noise")      # SSLCR_AUGV1_*: the code is the index
AugV1Desc = _S("sslcr_augv1_desc", "AugV1Desc", [(k, vp) for k in ("src", "dst", "op", "apply", "iparam", "dparam", "wtab", "work")] +
               [("work_smax", i32), ("ops_mask", C.c_uint)] + [(k, i32) for k in ("N", "H", "W", "src_hwc", "dst_hwc")])
WsiGatherDesc = _S("sslcr_wsi_gather_desc", "WsiGatherDesc", [("src", vp), ("xy", vp), ("dst", vp)] +
                   [(k, i32) for k in ("origin_x", "origin_y", "N", "RH", "RW", "S", "fill")])
PredictDesc = _S("sslcr_predict_desc", "PredictDesc", [("logits", vp), ("n", i32), ("C", i32), ("target", vp), ("scores", vp), ("pred", vp), ("confusion", vp),
                                 ("col", i32), ("map", vp), ("map_index", vp), ("map_size", C.c_int64)])
D4Desc = _S("sslcr_d4_desc", "D4Desc", [("src", vp), ("dst", vp), ("orient", vp)] + [(k, i32) for k in ("N", "Cn", "H", "W", "elem_bytes")])
PredictTtaDesc = _S("sslcr_predict_tta_desc", "PredictTtaDesc", [("p", PredictDesc), ("G", i32), ("mode", i32)])
TISSUE_MODES = {"hsv_s": 0, "lab_a": 1}
TissueBitsDesc = _S("sslcr_tissue_bits_desc", "TissueBitsDesc", [("img", vp), ("bits", vp), ("lin", vp), ("thr_sum", vp), ("threshold", f64), ("factor", f64),
                                       ("count", f64)] + [(k, i32) for k in ("H", "W", "pitch", "mode")])
LAB_SUM_PARTIALS = 1024
LabASumDesc = _S("sslcr_lab_a_sum_desc", "LabASumDesc", [("img", vp), ("lin", vp), ("partials", vp), ("sum", vp), ("H", i32), ("W", i32)])
TilePopcountDesc = _S("sslcr_tile_popcount_desc", "TilePopcountDesc", [("bits", vp), ("count", vp), ("keep", vp), ("thresh", f64)] +
                      [(k, i32) for k in ("H", "W", "pitch", "ph", "pw", "sh", "sw", "ny", "nx")])
RspGatherDesc = _S("sslcr_rsp_gather_desc", "RspGatherDesc", [("src", vp * 3), ("xy", vp * 3), ("idx", vp), ("dst", vp * 3), ("label", vp), ("RH", i32 * 3),
                                     ("RW", i32 * 3)] + [(k, i32) for k in ("T", "N", "S", "fill")])
PIP_CHUNK = 256
PipDesc = _S("sslcr_pip_desc", "PipDesc", [("vertices", vp), ("offsets", vp), ("bounds", vp), ("points", vp), ("inside", vp), ("first", vp)] +
             [(k, C.c_int64) for k in ("x0", "y0", "step", "N")] + [(k, i32) for k in ("nx", "ny", "P", "V", "exact")])
MapConfusionDesc = _S("sslcr_map_confusion_desc", "MapConfusionDesc", [(k, vp) for k in ("map", "truth", "tissue", "thresholds", "confusion")] +
                      [(k, i32) for k in ("X", "Y", "T")])
SMOOTH_MAX_R = 64
LABEL_RUN_CELLS = 1024        # cells per run of the labeller's numbering: one int32 of its scratch per run
LabelDesc = _S("sslcr_label_desc", "LabelDesc", [(k, vp) for k in ("mask", "labels", "count", "work")] + [(k, i32) for k in ("X", "Y", "connectivity")])
SmoothDesc = _S("sslcr_smooth_desc", "SmoothDesc", [(k, vp) for k in ("src", "tmp", "dst", "weights")] + [(k, i32) for k in ("X", "Y", "R")])
NmsDesc = _S("sslcr_nms_desc", "NmsDesc", [(k, vp) for k in ("map", "state", "cand", "stage", "counters", "det_xy", "det_prob")] + [("threshold", f32)] +
             [(k, i32) for k in ("X", "Y", "radius", "max_detections", "ncand")])
HitsDesc = _S("sslcr_hits_desc", "HitsDesc", [(k, vp) for k in ("labels", "det_xy", "det_prob", "n_det", "ignore", "hit", "tp_prob", "areas")] +
              [(k, i32) for k in ("X", "Y", "L", "max_detections", "n_ignore")])
EDT_ROW_CELLS = 1024
EdtDesc = _S("sslcr_edt_desc", "EdtDesc", [(k, vp) for k in ("mask", "out", "below", "work")] + [(k, i32) for k in ("X", "Y", "limit", "invert")])
FillDesc = _S("sslcr_fill_desc", "FillDesc", [(k, vp) for k in ("mask", "out", "labels", "count", "work")] + [(k, i32) for k in ("X", "Y")])
MomentsDesc = _S("sslcr_moments_desc", "MomentsDesc", [(k, vp) for k in ("labels", "moments")] + [(k, i32) for k in ("X", "Y", "L")])
SORT_TILE = 4096
RANK_SCAN_TRIP = 64
SortDesc = _S("sslcr_sort_desc", "SortDesc", [("keys", vp * 2), ("values", vp * 2), ("workspace", vp)] + [(k, i32) for k in ("B", "n", "lo", "hi")])
RankKeysDesc = _S("sslcr_rank_keys_desc", "RankKeysDesc", [(k, vp) for k in ("scores", "target", "valid", "positive", "keys", "values", "nan")] +
                  [("n", i32), ("C", i32)])
AucDesc = _S("sslcr_auc_desc", "AucDesc", [(k, vp) for k in ("keys", "values", "nan", "counts", "work")] + [("n", i32), ("C", i32)])
RESAMPLE_FILTERS = {"nearest": 0, "lanczos": 1, "bilinear": 2, "bicubic": 3, "box": 4, "hamming": 5}     # Pillow's codes
RESAMPLE_FORMS = ("gather", "fused", "two_pass", "horizontal", "vertical")
RESAMPLE_LDS_CAP = 65536
ResampleDesc = _S("sslcr_resample_desc", "ResampleDesc", [(k, vp) for k in ("src", "dst", "kx", "bx", "ky", "by", "table_index", "bx_host", "by_host", "workspace")] +
                  [(k, i32) for k in ("N", "C", "IH", "IW", "OH", "OW", "ksx", "ksy", "T", "src_chw", "dst_chw", "nearest", "form")])
ResamplePlan = _S("sslcr_resample_plan_info", "ResamplePlan", [(k, i32) for k in ("form", "fused_ok", "tile_w", "tile_h", "rows", "cols")] + [("grid", i32 * 2),
                                                                                                                ("lds_bytes", sz), ("workspace_bytes", sz)])
KNN_TILE, KNN_CHUNK, KNN_MAX_K, KNN_MAX_D, KNN_MAX_SLICES = 64, 64, 64, 2048, 1024
KNN_FORMS = ("direct", "sliced")
KNN_VOTES = {"uniform": 0, "softmax": 1, "regress": 2}
KnnDesc = _S("sslcr_knn_desc", "KnnDesc", [(k, vp) for k in ("queries", "bank", "scores", "indices", "workspace")] +
             [(k, i32) for k in ("nq", "nb", "D", "k", "nb_valid", "self_offset", "slices")])
KnnPlan = _S("sslcr_knn_plan_info", "KnnPlan", [(k, i32) for k in ("form", "tile_q", "tile_b", "chunk", "slices", "tiles_per_slice")] +
             [("grid", i32 * 2), ("lds_bytes", sz), ("workspace_bytes", sz)])
KnnVoteDesc = _S("sslcr_knn_vote_desc", "KnnVoteDesc", [(k, vp) for k in ("indices", "scores", "labels", "targets", "query_labels", "pred", "pred_value",
                                                                          "votes", "confusion")] +
                 [(k, i32) for k in ("nq", "k", "nb", "C", "mode")] + [("temperature", f32)])
TSNE_TILE, TSNE_CHUNK, TSNE_MAX_SLICES, TSNE_MAX_N, TSNE_LOG_COLS = 256, 1024, 64, 1 << 20, 4
TsnePlan = _S("sslcr_tsne_plan_info", "TsnePlan", [(k, i32) for k in ("tile", "chunk", "slices", "chunks_per_slice")] +
              [("grid", i32 * 3), ("lds_bytes", sz), ("workspace_bytes", sz)])
TsneGradDesc = _S("sslcr_tsne_grad_desc", "TsneGradDesc", [(k, vp) for k in ("y", "y_out", "update", "gains", "grad", "rowptr", "col", "val", "workspace",
                                                                             "Z", "kl_rows")] +
                  [(k, i32) for k in ("n", "slices", "nnz")] + [(k, f64) for k in ("exaggeration", "momentum", "lr", "min_gain")])
LINPROBE_LOSSES = {"softmax": 0, "squared": 1}
LINPROBE_FORMS = ("staged", "streamed")
LINPROBE_TILE, LINPROBE_CHUNK, LINPROBE_MAX_C, LINPROBE_MAX_D, LINPROBE_MAX_GROUPS = 32, 512, 64, 2048, 1024
LinprobeDesc = _S("sslcr_linprobe_desc", "LinprobeDesc", [(k, vp) for k in ("x", "w", "b", "labels", "targets", "sample_weight", "value", "grad",
                                                                             "logits", "workspace")] +
                  [(k, i32) for k in ("n", "D", "C", "loss", "groups")])
LinprobePlan = _S("sslcr_linprobe_plan_info", "LinprobePlan", [(k, i32) for k in ("form", "tile_rows", "groups", "tiles_per_group", "col_slices", "chunk",
                                                                                  "class_blocks")] +
                  [("grid", i32 * 3), ("lds_bytes", sz), ("workspace_bytes", sz)])
PackDesc = _S("sslcr_pack_desc", "PackDesc", [("w", vp), ("w_fwd", vp), ("w_dgrad", vp), ("gamma", vp), ("beta", vp), ("rmean", vp),
                           ("rvar", vp), ("eps", f32), ("bias_out", vp)] + [(k, i32) for k in ("K", "C", "R", "S", "dgrad_flip")] + [("scale_out", vp)])

Fp8Desc = _S("sslcr_fp8_desc", "Fp8Desc", [("w8", vp), ("w_dequant", vp), ("x_scale", f32), ("x_scale_dev", vp), ("amax_out", vp)])
PackFp8Desc = _S("sslcr_pack_fp8_desc", "PackFp8Desc", [("w", vp), ("w8", vp), ("w_dequant", vp), ("gamma", vp), ("beta", vp), ("rmean", vp), ("rvar", vp),
                                 ("eps", f32), ("bias_out", vp), ("K", i32), ("C", i32)])

# SSLCR_* macro of include/sslcr.h -> its value on this side: the one place a mirrored #define is registered (tests/test_abi_cpu.py
# holds every entry to the header)
CONSTANTS = {"SSLCR_MAX_OPT_GROUPS": MAX_OPT_GROUPS, "SSLCR_LAB_SUM_PARTIALS": LAB_SUM_PARTIALS, "SSLCR_PIP_CHUNK": PIP_CHUNK,
             "SSLCR_SMOOTH_MAX_R": SMOOTH_MAX_R, "SSLCR_LABEL_RUN_CELLS": LABEL_RUN_CELLS, "SSLCR_EDT_ROW_CELLS": EDT_ROW_CELLS,
             "SSLCR_SORT_TILE": SORT_TILE, "SSLCR_RANK_SCAN_TRIP": RANK_SCAN_TRIP, "SSLCR_RESAMPLE_LDS_CAP": RESAMPLE_LDS_CAP}
CONSTANTS.update({"SSLCR_TISSUE_" + k.upper(): v for k, v in TISSUE_MODES.items()})
CONSTANTS.update({"SSLCR_RESAMPLE_" + k.upper(): v for k, v in RESAMPLE_FILTERS.items()})
CONSTANTS.update({"SSLCR_RESAMPLE_" + k.upper(): v for v, k in enumerate(RESAMPLE_FORMS)})
CONSTANTS.update({"SSLCR_KNN_TILE": KNN_TILE, "SSLCR_KNN_CHUNK": KNN_CHUNK, "SSLCR_KNN_MAX_K": KNN_MAX_K, "SSLCR_KNN_MAX_D": KNN_MAX_D,
                  "SSLCR_KNN_MAX_SLICES": KNN_MAX_SLICES})
CONSTANTS.update({"SSLCR_KNN_" + k.upper(): v for v, k in enumerate(KNN_FORMS)})
CONSTANTS.update({"SSLCR_TSNE_TILE": TSNE_TILE, "SSLCR_TSNE_CHUNK": TSNE_CHUNK, "SSLCR_TSNE_MAX_SLICES": TSNE_MAX_SLICES,
                  "SSLCR_TSNE_MAX_N": TSNE_MAX_N, "SSLCR_TSNE_LOG_COLS": TSNE_LOG_COLS})
CONSTANTS.update({"SSLCR_KNN_VOTE_" + k.upper(): v for k, v in KNN_VOTES.items()})
CONSTANTS.update({"SSLCR_LINPROBE_" + k.upper(): v for k, v in LINPROBE_LOSSES.items()})
CONSTANTS.update({"SSLCR_LINPROBE_" + k.upper(): v for v, k in enumerate(LINPROBE_FORMS)})
CONSTANTS.update({"SSLCR_LINPROBE_TILE": LINPROBE_TILE, "SSLCR_LINPROBE_CHUNK": LINPROBE_CHUNK, "SSLCR_LINPROBE_MAX_C": LINPROBE_MAX_C,
                  "SSLCR_LINPROBE_MAX_D": LINPROBE_MAX_D, "SSLCR_LINPROBE_MAX_GROUPS": LINPROBE_MAX_GROUPS})
CONSTANTS.update({"SSLCR_AUGV1_" + k.upper(): v for v, k in enumerate(AUGV1_OPS)})

# symbol -> (restype, argtypes); every symbol include/sslcr.h declares
P = C.POINTER
SIGNATURES = {
    "sslcr_version": (i32, []),
    "sslcr_last_error": (C.c_char_p, []),
    "sslcr_switch_count": (i32, []),
    "sslcr_switch_info": (i32, [i32, P(SwitchRow)]),
    "sslcr_conv2d": (i32, [i32, P(ConvDesc), vp]),
    "sslcr_conv2d_partial_rows": (i32, [P(ConvDesc)]),
    "sslcr_conv2d_segments_ok": (i32, [i32, P(ConvDesc)]),
    "sslcr_conv2d_kernel_name": (C.c_char_p, [i32, P(ConvDesc)]),
    "sslcr_conv2d_s2_pair": (i32, [i32, P(ConvDesc), P(ConvDesc), vp]),
    "sslcr_conv2d_s2_pair_ok": (i32, [i32, P(ConvDesc), P(ConvDesc)]),
    "sslcr_conv2d_fp8": (i32, [P(ConvDesc), P(Fp8Desc), vp]),
    "sslcr_conv2d_fp8_partial_rows": (i32, [P(ConvDesc)]),
    "sslcr_conv2d_fp8_kernel_name": (C.c_char_p, [P(ConvDesc)]),
    "sslcr_fp8_scale_update": (i32, [vp, i32, vp]),
    "sslcr_pack_conv_fp8": (i32, [P(PackFp8Desc), vp]),
    "sslcr_conv2d_wgrad": (i32, [i32, P(WgradDesc), vp]),
    "sslcr_conv2d_wgrad_kernel_name": (C.c_char_p, [i32, P(WgradDesc)]),
    "sslcr_probe_tr16": (i32, [vp, vp, vp, vp]),
    "sslcr_stem_conv": (i32, [i32, P(StemDesc), vp]),
    "sslcr_stem_partial_rows": (i32, [P(StemDesc)]),
    "sslcr_stem_conv_pool": (i32, [i32, P(StemDesc), i32, i32, vp]),
    "sslcr_stem_wgrad": (i32, [i32, P(StemWgradDesc), vp]),
    "sslcr_stem_wgrad_pool": (i32, [i32, P(StemWgradDesc), P(BnBwdDesc), vp]),
    "sslcr_stem_wgrad_pool_kernel_name": (C.c_char_p, [i32, P(StemWgradDesc)]),
    "sslcr_bn_finalize": (i32, [P(BnFinalizeDesc), vp]),
    "sslcr_bn_act": (i32, [i32, P(BnActDesc), vp]),
    "sslcr_bn_relu_maxpool": (i32, [i32, P(PoolFwdDesc), vp]),
    "sslcr_maxpool_relu_bwd": (i32, [i32, P(PoolBwdDesc), vp]),
    "sslcr_avgpool_fwd": (i32, [i32, vp, vp, i32, i32, i32, vp]),
    "sslcr_avgpool_bwd": (i32, [i32, vp, vp, i32, i32, i32, vp]),
    "sslcr_bn_bwd_reduce": (i32, [i32, P(BnBwdDesc), vp]),
    "sslcr_bn_bwd_apply": (i32, [i32, P(BnBwdDesc), vp]),
    "sslcr_bn_param_grads": (i32, [vp, vp, vp, vp, i32, vp]),
    "sslcr_linear_fwd": (i32, [vp, vp, vp, vp, i32, i32, i32, i32, vp]),
    "sslcr_linear_bwd": (i32, [vp, vp, vp, vp, vp, vp, vp, i32, i32, i32, i32, vp, vp]),
    "sslcr_loss": (i32, [P(LossDesc), vp]),
    "sslcr_loss_ex": (i32, [P(LossDesc), P(LossOpts), vp]),
    "sslcr_ce_denominator": (i32, [vp, i32, i32, vp, i32, vp, vp]),
    "sslcr_softmax_col": (i32, [vp, vp, i32, i32, i32, vp]),
    "sslcr_predict": (i32, [P(PredictDesc), vp]),
    "sslcr_wsi_gather": (i32, [P(WsiGatherDesc), vp]),
    "sslcr_wsi_gather_d4": (i32, [P(WsiGatherDesc), vp, vp]),
    "sslcr_d4_transform": (i32, [P(D4Desc), vp]),
    "sslcr_predict_tta": (i32, [P(PredictTtaDesc), vp]),
    "sslcr_tissue_bits": (i32, [P(TissueBitsDesc), vp]),
    "sslcr_lab_a_sum": (i32, [P(LabASumDesc), vp]),
    "sslcr_tile_popcount": (i32, [P(TilePopcountDesc), vp]),
    "sslcr_rsp_gather": (i32, [P(RspGatherDesc), vp]),
    "sslcr_points_in_polygons": (i32, [P(PipDesc), vp]),
    "sslcr_map_confusion": (i32, [P(MapConfusionDesc), vp]),
    "sslcr_label_components": (i32, [P(LabelDesc), vp]),
    "sslcr_gaussian_smooth": (i32, [P(SmoothDesc), vp]),
    "sslcr_nms_candidates": (i32, [P(NmsDesc), vp]),
    "sslcr_nms_rounds": (i32, [P(NmsDesc), i32, vp]),
    "sslcr_nms_collect": (i32, [P(NmsDesc), vp]),
    "sslcr_lesion_hits": (i32, [P(HitsDesc), vp]),
    "sslcr_edt_squared": (i32, [P(EdtDesc), vp]),
    "sslcr_fill_holes": (i32, [P(FillDesc), vp]),
    "sslcr_region_moments": (i32, [P(MomentsDesc), vp]),
    "sslcr_sort_workspace_bytes": (sz, [i32, i32]),
    "sslcr_sort_pairs": (i32, [P(SortDesc), vp]),
    "sslcr_rank_keys": (i32, [P(RankKeysDesc), vp]),
    "sslcr_auc_workspace_bytes": (sz, [i32, i32]),
    "sslcr_auc_counts": (i32, [P(AucDesc), vp]),
    "sslcr_resample_ksize": (i32, [f64, f64, i32, i32]),
    "sslcr_resample_coeffs": (i32, [i32, f64, f64, i32, i32, vp, i32, vp]),
    "sslcr_resample_table_ok": (i32, [vp, i32, i32]),
    "sslcr_resample_plan": (i32, [P(ResampleDesc), P(ResamplePlan)]),
    "sslcr_resample": (i32, [P(ResampleDesc), vp]),
    "sslcr_knn_plan": (i32, [i32, i32, i32, i32, i32, P(KnnPlan)]),
    "sslcr_knn_topk": (i32, [P(KnnDesc), vp]),
    "sslcr_l2_normalize": (i32, [vp, vp, i32, i32, f32, vp]),
    "sslcr_knn_vote": (i32, [P(KnnVoteDesc), vp]),
    "sslcr_tsne_plan": (i32, [i32, i32, P(TsnePlan)]),
    "sslcr_tsne_pair_dist2": (i32, [vp, vp, vp, i32, i32, i32, vp]),
    "sslcr_tsne_affinities": (i32, [vp, vp, vp, i32, i32, f32, vp]),
    "sslcr_tsne_repulsion": (i32, [P(TsneGradDesc), vp]),
    "sslcr_tsne_update": (i32, [P(TsneGradDesc), vp]),
    "sslcr_tsne_kl": (i32, [vp, vp, vp, vp, i32, i32, vp]),
    "sslcr_linprobe_plan": (i32, [i32, i32, i32, i32, i32, P(LinprobePlan)]),
    "sslcr_linprobe_eval": (i32, [P(LinprobeDesc), vp]),
    "sslcr_linprobe_logits": (i32, [P(LinprobeDesc), vp]),
    "sslcr_optimizer_step": (i32, [vp, i32, i32, P(OptDesc), vp]),
    "sslcr_optimizer_step_groups": (i32, [vp, i32, i32, P(OptDesc), i32, vp, vp]),
    "sslcr_grad_norm": (i32, [vp, sz, f32, vp, vp, vp]),
    "sslcr_grad_norm_partials": (i32, []),
    "sslcr_grad_accumulate": (i32, [vp, vp, sz, vp]),
    "sslcr_axpby": (i32, [vp, vp, sz, f32, i32, vp]),
    "sslcr_fill": (i32, [vp, sz, f32, vp]),
    "sslcr_pack_conv": (i32, [i32, P(PackDesc), vp]),
    "sslcr_pack_stem": (i32, [i32, P(PackDesc), vp]),
    "sslcr_weak_augment": (i32, [P(WeakAugDesc), vp]),
    "sslcr_hed_colour_augment": (i32, [P(ColourAugDesc), vp]),
    "sslcr_brightness_contrast": (i32, [P(BrightnessContrastDesc), vp]),
    "sslcr_randaug_v2_slot": (i32, [P(AugV2Desc), vp]),
    "sslcr_randaug_v2_colour": (i32, [P(AugV2ColourDesc), vp]),
    "sslcr_randaug_v1_slot": (i32, [P(AugV1Desc), vp]),
    "sslcr_cv_warp_table": (i32, [vp]),
    "sslcr_augv1_workspace_bytes": (sz, [i32, i32, f64]),
    "sslcr_augv1_philox": (i32, [C.c_ulonglong, C.c_uint32, i32, vp, vp]),
}

_lib = None


def lib():
    """Load libsslcr.so (once).  Raises SslcrError if it was not built -- never falls back."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise SslcrError(f"{LIB_PATH} not built: run `python -m ssl_cr_histo_amd.build` "
                             "(or __graft_entry__.build()); there is no CPU/PyTorch fallback")
        L = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)          # AttributeError => header/library mismatch, fail loudly
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc):
    if rc != 0:
        raise SslcrError(lib().sslcr_last_error().decode())


def stream_ptr():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def ptr_at(t, byte_offset):
    """the address ``byte_offset`` bytes past a tensor's first element"""
    return C.c_void_p(t.data_ptr() + byte_offset)
