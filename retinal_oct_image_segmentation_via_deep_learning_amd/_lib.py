"""ctypes binding of liboct_hip.so (C ABI declared in include/oct_hip.h).

The product path has NO CPU fallback: if the shared library is missing or a call fails this
module raises.  Build it with `python __graft_entry__.py` (or `make -C .../csrc`).
"""
from __future__ import annotations

import ctypes as C
import os
import subprocess
import threading

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("OCT_HIP_LIB") or os.path.join(PKG_DIR, "liboct_hip.so")  # override: ablation builds
CSRC_DIR = os.path.join(PKG_DIR, "csrc")

DT_BF16, DT_F32 = 0, 1
XF_NONE, XF_AFFINE_RELU, XF_AFFINE = 0, 1, 2
IN_PLAIN, IN_S2D = 0, 1
IMG_SHIFT_ALL = 2   # OctWgradDesc.in_img_shift: all depth taps in one launch (OCT_IMG_SHIFT_ALL)
ACT_NONE, ACT_RELU, ACT_SIGMOID = 0, 1, 2
ACT_PRELU = 3   # host-side tag only: PReLU has its own entry points (oct_affine_prelu_fwd / _bwd)
OUT_PLAIN, OUT_D2S = 0, 1
PACK_CONV_FPROP, PACK_CONV_DGRAD, PACK_DECONV_FPROP, PACK_DECONV_DGRAD, PACK_1X1_DGRAD, PACK_1X1_FPROP = range(6)
PACK_CONV3D_FPROP, PACK_CONV3D_DGRAD, PACK_DECONV3D_FPROP, PACK_DECONV3D_DGRAD = 6, 7, 8, 9
MAX_CLASSES = 16
HEAD_LOSS_SLOTS = 2 + 3 * MAX_CLASSES
SEG_NHWC, SEG_NCHW = 0, 1   # oct_seg_loss_* logits layouts (OCT_SEG_NHWC / OCT_SEG_NCHW)

c_void_p, c_int, c_size_t, c_float, c_double = C.c_void_p, C.c_int, C.c_size_t, C.c_float, C.c_double


class PackJob(C.Structure):          # struct OctPackJob
    _fields_ = [("mode", c_int), ("cout", c_int), ("cin", c_int), ("reserved", c_int), ("w", c_void_p),
                ("wpacked", c_void_p)]


class UnpackJob(C.Structure):        # struct OctUnpackJob
    _fields_ = [("mode", c_int), ("cout", c_int), ("cin", c_int), ("accumulate", c_int), ("nparts", c_int),
                ("reserved", c_int), ("dwp", c_void_p), ("grad", c_void_p)]


PACK_BATCH_MAX = 96


class ConvDesc(C.Structure):
    _fields_ = [(k, c_int) for k in (
        "dtype", "n", "h", "w", "c0", "c1", "cout", "taps", "xform0", "xform1", "in_mode", "out_mode",
        "split", "want_stats", "kh", "kw", "depth", "out_img_mul", "out_img_add")]


class ConvArgs(C.Structure):
    _fields_ = [(k, c_void_p) for k in (
        "x0", "x1", "scale0", "shift0", "scale1", "shift1", "wpacked", "bias", "y0", "y1", "stat_partials")]


class WgradDesc(C.Structure):
    _fields_ = [(k, c_int) for k in (
        "dtype", "n", "h", "w", "c0", "c1", "cout", "taps", "xform0", "xform1", "dy_mode", "kh", "kw", "depth",
        "in_img_shift", "dy_img_mul", "dy_img_add", "partials")]


class WgradArgs(C.Structure):
    _fields_ = [(k, c_void_p) for k in ("x0", "x1", "scale0", "shift0", "scale1", "shift1", "dy", "dwp", "dbias",
                                                "dy_y", "dy_coef", "dy_scale", "dy_shift", "dbias_partials", "dy_out")]


class ConvBwdFusedArgs(C.Structure):   # struct OctConvBwdFusedArgs
    _fields_ = [(k, c_void_p) for k in ("x", "scale", "shift", "mean", "invstd", "dy", "wpacked", "dx", "dwp", "partials")]


class HeadDesc(C.Structure):
    _fields_ = [(k, c_int) for k in ("dtype", "n", "h", "w", "feat", "classes")]


class SegEvalDesc(C.Structure):      # struct OctSegEvalDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "classes", "target_elem", "pred_kind", "has_ignore")] + \
               [("ignore_index", C.c_int64)]


class ContourDesc(C.Structure):      # struct OctContourDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "classes", "target_elem", "pred_elem", "has_ignore")] + \
               [("ignore_index", C.c_int64)]


class ScoreEvalDesc(C.Structure):    # struct OctScoreEvalDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "channels", "score_elem", "has_ignore", "ignore_value")]


class AugmentDesc(C.Structure):      # struct OctAugmentDesc
    _fields_ = [(k, c_int) for k in ("batch", "cin", "hs", "ws", "ho", "wo", "src_elem", "out_elem", "label_kind", "label_planes",
                                     "flags", "grid_pitch")] + \
               [(k, C.c_uint32) for k in ("seed_lo", "seed_hi", "step", "sample_base")] + \
               [("fill", c_float), ("reserved", c_int), ("label_fill", C.c_int64)]


class CcDesc(C.Structure):           # struct OctCcDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "classes", "map_elem", "pred_elem", "connectivity", "op", "has_ignore",
                                     "overlap_num", "overlap_den", "reserved")] + \
               [("ignore_index", C.c_int64)]


class CcRules(C.Structure):          # struct OctCcRules
    _fields_ = [("min_area", c_int * 16), ("keep_largest", c_int * 16), ("drop_enclosed", c_int * 16), ("replace", C.c_int64 * 16)]


class DtDesc(C.Structure):           # struct OctDtDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "classes", "map_elem", "has_ignore", "planes", "op")] + \
               [("ignore_index", C.c_int64)]


class SurfDesc(C.Structure):         # struct OctSurfDesc
    _fields_ = [(k, c_int) for k in ("images", "h", "w", "classes", "elem", "k", "max_step", "has_ignore", "nkeep", "qmax")] + \
               [("scale", c_float), ("reserved", c_int), ("ignore_index", C.c_int64)]


CC_OP_LABEL, CC_OP_FILTER, CC_OP_LESION = range(3)   # OCT_CC_OP_*
DT_FAR = 1 << 30       # OCT_DT_FAR: the squared distance where an image has no site of the plane
DT_MAX_PLANES = 64     # OCT_DT_MAX_PLANES; oct_dt_signed takes half as many classes
DT_MAX_DIM = 16384     # h, w of the distance-map entry points
DT_BOUNDARY, DT_CLASS, DT_OTHER = range(3)   # OCT_DT_* plane kinds
DT_OP_SQUARED, DT_OP_WEIGHT, DT_OP_SIGNED = range(3)   # OCT_DT_OP_*
SURF_MAX_K, SURF_MAX_H, SURF_MAX_STEP = 16, 4095, 32   # OCT_SURF_MAX_*
SURF_F32, SURF_BF16 = 3, 4   # OctSurfDesc.elem of scores (class maps: 0 uint8, 2 int64)
SURF_STATE_FIELDS = 5  # count, sum |e|, sum e, sum e^2, max |e| per surface
CC_BORDER_BIT = 30     # info of a root: area | touches_border << 30
CC_MAX_DIM = 16384     # h, w of the connected-component entry points
LESION_STATE_EXTRA = 4   # images, ignored, invalid, updates behind [classes][4]
SCORE_F32, SCORE_BF16, SCORE_U8 = 0, 1, 2   # OCT_SCORE_*
AUG_U8, AUG_BF16, AUG_F32 = 0, 1, 2   # OCT_AUG_* element kinds
AUG_LABEL_NONE, AUG_LABEL_CLASS_U8, AUG_LABEL_CLASS_I64, AUG_LABEL_MASK_U8 = range(4)   # OCT_AUG_LABEL_*
AUG_GAMMA, AUG_NOISE, AUG_ELASTIC = 1, 2, 4   # OCT_AUG_* flags
AUG_PARAM_WORDS = 16   # 32-bit words per sample of oct_augment_pair's params
AUG_MAX_DIM = 8192
SCORE_KEYS = 65536   # hist[C][2][SCORE_KEYS] | nan[C] | ignored[C] | invalid[C] | updates
CONTOUR_MAX_DIM = 16384   # h, w of oct_contour_update: keeps every squared distance below 2^31
EVAL_PRED_U8, EVAL_PRED_I64, EVAL_PRED_NHWC_BF16, EVAL_PRED_NHWC_F32, EVAL_PRED_NCHW_F32 = range(5)   # OCT_EVAL_PRED_*
EVAL_STATE_EXTRA = 4   # columns, ignored, invalid, updates behind cm [C*C] and thick_abs [C]


# name -> (restype, argtypes).  Every symbol of include/oct_hip.h is listed here;
# tests/test_abi.py checks the two stay in sync.
SIGNATURES = {
    "oct_version_string": (C.c_char_p, []),
    "oct_version": (c_int, []),
    "oct_get_last_error": (c_int, [C.c_char_p, c_size_t]),
    "oct_device_count": (c_int, []),
    "oct_conv_stat_blocks": (c_int, [C.POINTER(ConvDesc)]),
    "oct_packed_weight_elems": (c_size_t, [c_int, c_int, c_int]),
    "oct_pack_weights": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_void_p]),
    "oct_pack_weights3d": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "oct_unpack_wgrad3d": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_depth_pool_fwd": (c_int, [c_int, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "oct_depth_pool_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "oct_pack_weights_kk": (c_int, [c_int, c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_unpack_wgrad_kk": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_affine_prelu_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "oct_affine_prelu_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t,
                                     c_int, c_void_p]),
    "oct_maxpool_idx_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_index_scatter": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_int, c_void_p]),
    "oct_index_gather": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_size_t, c_size_t, c_int, c_void_p]),
    "oct_prelu_bn_fused_ok": (c_int, [c_int, c_int]),
    "oct_dact_bn_reduce_prelu": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                         c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bn_bwd_apply_prelu_to": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int,
                                          c_void_p]),
    "oct_maxpool_code_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_window_scatter": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_window_gather": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_pack_weights_batch": (c_int, [c_int, c_int, C.POINTER(PackJob), c_void_p]),
    "oct_conv_forward": (c_int, [C.POINTER(ConvDesc), C.POINTER(ConvArgs), c_void_p]),
    "oct_conv_wgrad": (c_int, [C.POINTER(WgradDesc), C.POINTER(WgradArgs), c_void_p]),
    "oct_conv_wgrad_fused_apply_ok": (c_int, [C.POINTER(WgradDesc)]),
    "oct_conv_wgrad_apply_store_ok": (c_int, [C.POINTER(WgradDesc)]),
    "oct_conv_wgrad_all_depth_taps_ok": (c_int, [C.POINTER(WgradDesc)]),
    "oct_conv_backward_fused_ok": (c_int, [C.POINTER(WgradDesc)]),
    "oct_conv_backward_fused_blocks": (c_int, [C.POINTER(WgradDesc)]),
    "oct_conv_backward_fused": (c_int, [C.POINTER(WgradDesc), C.POINTER(ConvBwdFusedArgs), c_void_p]),
    "oct_conv_wgrad_partials": (c_int, [C.POINTER(WgradDesc)]),
    "oct_reduce_bias_partials": (c_int, [c_void_p, c_int, c_int, c_int, c_void_p, c_int, c_void_p]),
    "oct_unpack_wgrad": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p]),
    "oct_unpack_wgrad_batch": (c_int, [c_int, C.POINTER(UnpackJob), c_void_p]),
    "oct_bn_finalize": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p, c_float, c_float,
                                c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_bn_eval_coeffs": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "oct_bn_relu_pool_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                     c_void_p]),
    "oct_bn_relu_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "oct_dact_bn_reduce": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_dact_bn_reduce_blocks": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "oct_bn_bwd_apply_pool_ok": (c_int, [c_int, c_int, c_int, c_int, c_int]),
    "oct_bn_bwd_apply_pool": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                      c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bn_bwd_finalize": (c_int, [c_void_p, c_int, c_int, c_double, c_void_p, c_void_p, c_void_p, c_void_p,
                                    c_void_p, c_void_p, c_int, c_void_p]),
    "oct_bn_bwd_apply": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int,
                                 c_void_p]),
    "oct_bn_bwd_apply_to": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int,
                                    c_void_p]),
    "oct_channel_sum": (c_int, [c_int, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "oct_rowdot_ok": (c_int, [c_int, c_int]),
    "oct_rowdot_blocks": (c_int, [c_size_t, c_int]),
    "oct_rowdot_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "oct_rowdot_bwd_data": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_void_p]),
    "oct_rowdot_bwd_weight": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int, c_void_p]),
    "oct_rowdot_bwd_weight_bias": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_int, c_int,
                                           c_void_p]),
    "oct_head_blocks": (c_int, [C.POINTER(HeadDesc)]),
    "oct_head_forward": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_head_loss_finalize": (c_int, [C.POINTER(HeadDesc), c_void_p, c_int, c_float, c_float, c_float, c_void_p,
                                       c_void_p, c_void_p]),
    "oct_head_dlogits": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_float, c_void_p, c_void_p, c_void_p]),
    "oct_head_backward_fused": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                        c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_head_backward_dl_ok": (c_int, [C.POINTER(HeadDesc)]),
    "oct_head_backward_dl": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p,
                                     c_void_p, c_void_p]),
    "oct_head_bwd_apply": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                   c_void_p, c_void_p]),
    "oct_seg_loss_blocks": (c_int, [c_size_t, c_int]),
    "oct_seg_loss_forward": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_seg_loss_backward": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p,
                                      c_void_p, c_void_p]),
    "oct_seg_loss_weight_sum": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_void_p, c_int, C.c_int64, c_void_p, c_void_p,
                                        c_void_p]),
    "oct_seg_loss_forward_weighted": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                              C.c_int64, c_void_p, c_void_p]),
    "oct_seg_loss_backward_weighted": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int,
                                               C.c_int64, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_seg_loss_finalize_weighted": (c_int, [C.POINTER(HeadDesc), c_void_p, c_int, c_float, c_float, c_float, c_void_p,
                                               c_void_p, c_void_p, c_void_p]),
    "oct_bce_loss_weight_sum": (c_int, [C.POINTER(HeadDesc), c_void_p, c_void_p, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "oct_bce_loss_forward": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                     c_float, c_void_p, c_void_p, c_void_p]),
    "oct_bce_loss_backward": (c_int, [C.POINTER(HeadDesc), c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                      c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_nchw_to_nhwc": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_nhwc_to_nchw": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_sgd_step": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_int,
                             c_void_p]),
    "oct_adam_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_float,
                              c_int, c_float, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "oct_sgd_step_scaled": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_float, c_float, c_float, c_float, c_int,
                                    c_void_p, c_void_p, c_void_p]),
    "oct_grad_norm_blocks": (c_int, [c_size_t]),
    "oct_grad_norm": (c_int, [c_void_p, c_size_t, c_float, c_float, c_void_p, c_void_p, c_void_p]),
    "oct_affine_act_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_int,
                                   c_void_p]),
    "oct_affine_res_act_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_size_t,
                                       c_int, c_void_p]),
    "oct_act_bwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_void_p, c_size_t, c_void_p]),
    "oct_maxpool_fwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_maxpool_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bilinear_up_fwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bilinear_up_bwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bilinear_resize_fwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_bilinear_resize_bwd": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_depth_to_space": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_space_to_depth": (c_int, [c_int, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p]),
    "oct_gate_fwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "oct_gate_bwd": (c_int, [c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_size_t, c_int, c_void_p]),
    "oct_confusion_counts": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p, c_void_p]),
    "oct_class_confusion_counts": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_int, c_void_p, c_void_p, c_void_p]),
    "oct_sqdiff_sum": (c_int, [c_void_p, c_void_p, c_int, c_size_t, c_void_p, c_void_p]),
    "oct_column_absdiff_sum": (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, c_size_t, c_void_p, c_void_p]),
    "oct_seg_eval_update": (c_int, [C.POINTER(SegEvalDesc), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_contour_workspace_bytes": (c_size_t, [C.POINTER(ContourDesc)]),
    "oct_contour_update": (c_int, [C.POINTER(ContourDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_score_eval_state_elems": (c_size_t, [c_int]),
    "oct_score_eval_update": (c_int, [C.POINTER(ScoreEvalDesc), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_augment_pair": (c_int, [C.POINTER(AugmentDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_void_p, c_void_p]),
    "oct_augment_philox_words": (c_int, [c_void_p, c_size_t, C.c_uint32, C.c_uint32, c_void_p, c_void_p]),
    "oct_cc_workspace_bytes": (c_size_t, [C.POINTER(CcDesc)]),
    "oct_cc_tile": (c_int, [C.POINTER(c_int), C.POINTER(c_int)]),
    "oct_cc_label": (c_int, [C.POINTER(CcDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_cc_filter": (c_int, [C.POINTER(CcDesc), C.POINTER(CcRules), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_lesion_eval_update": (c_int, [C.POINTER(CcDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_dt_workspace_bytes": (c_size_t, [C.POINTER(DtDesc)]),
    "oct_dt_block": (c_int, [C.POINTER(c_int), C.POINTER(c_int)]),
    "oct_dt_squared": (c_int, [C.POINTER(DtDesc), C.POINTER(C.c_int32), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_dt_weight_map": (c_int, [C.POINTER(DtDesc), C.POINTER(C.c_int32), c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p]),
    "oct_dt_signed": (c_int, [C.POINTER(DtDesc), C.POINTER(C.c_int32), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_surf_workspace_bytes": (c_size_t, [C.POINTER(SurfDesc)]),
    "oct_surf_extract": (c_int, [C.POINTER(SurfDesc), C.POINTER(C.c_int32), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_surf_paint": (c_int, [C.POINTER(SurfDesc), C.POINTER(C.c_int32), C.POINTER(C.c_int32), c_void_p, c_void_p, c_void_p, c_void_p]),
    "oct_surf_error_update": (c_int, [C.POINTER(SurfDesc), c_void_p, c_void_p, c_void_p, c_void_p, c_void_p]),
}

_lib = None
_lock = threading.Lock()
# bumped whenever parameter memory is modified behind torch's back (FusedSGD / FusedAdam, DDP broadcast)
param_generation = [0]


class OctError(RuntimeError):
    pass


def build(verbose: bool = False) -> str:
    """Compile liboct_hip.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    cmd = ["make", "-C", CSRC_DIR, "-j8"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    if verbose or res.returncode != 0:
        print(res.stdout[-4000:])
        print(res.stderr[-4000:])
    if res.returncode != 0:
        raise OctError("building liboct_hip.so failed (see output above)")
    return LIB_PATH


def lib():
    """The loaded library.  Raises OctError when it has not been built -- never falls back."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise OctError(
                    f"{LIB_PATH} is missing: the HIP extension has not been built "
                    "(run `python __graft_entry__.py` or `make -C .../csrc`). There is no CPU fallback.")
            handle = C.CDLL(LIB_PATH)
            for name, (res, args) in SIGNATURES.items():
                fn = getattr(handle, name)  # AttributeError if the .so lacks a declared symbol
                fn.restype = res
                fn.argtypes = args
            _lib = handle
    return _lib


def last_error() -> str:
    buf = C.create_string_buffer(512)
    lib().oct_get_last_error(buf, 512)
    return buf.value.decode("utf-8", "replace")


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        raise OctError(f"{what or 'liboct_hip'} failed with code {rc}: {last_error()}")


def ptr(t) -> int | None:
    """data_ptr of a torch tensor (None stays NULL)."""
    return None if t is None else t.data_ptr()
