"""ctypes binding of libunetr_hip.so (declared in include/unetr_hip.h).

There is NO fallback: if the shared library is missing or a kernel returns non-zero this raises.  The
library is built in-tree by ``__graft_entry__.build()`` / ``make -C csrc``.
"""
import ctypes
import os
from ctypes import c_double, c_float, c_int, c_long, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
# UNETR_AMD_LIB: an alternative build of the same ABI (diagnostic builds such as `make x3droplo`); the product loads libunetr_hip.so
LIB_PATH = os.environ.get("UNETR_AMD_LIB") or os.path.join(_HERE, "libunetr_hip.so")

PREC_F32 = 0
PREC_BF16 = 1
PREC_BF16X3 = 2      # fp32 storage, operands split into bf16 (hi, lo) pairs inside the kernels (csrc/common.hpp: PrecBF16x3)
ABI_VERSION = 21       # = UNETR_ABI_VERSION of include/unetr_hip.h this table of signatures was written against

_ERR = {1: "invalid argument", 2: "kernel launch failed", 3: "unsupported shape/configuration",
        4: "workspace too small"}


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ("M", c_int), ("N", c_int), ("K", c_int), ("batch", c_int),
        ("a_trans", c_int), ("b_trans", c_int),
        ("lda", c_long), ("ldb", c_long), ("ldc", c_long),
        ("strideA", c_long), ("strideB", c_long), ("strideC", c_long),
        ("bias", c_void_p), ("res", c_void_p),
        ("ldr", c_long), ("strideR", c_long), ("res_mod", c_int),
        ("pre", c_void_p), ("aux", c_void_p), ("ldaux", c_long),
        ("act", c_int), ("accumulate", c_int), ("alpha", c_float), ("prec", c_int), ("b_x3words", c_int),
    ]


class GemmBf16Desc(ctypes.Structure):
    _fields_ = [
        ("M", c_int), ("N", c_int), ("K", c_int), ("b_kn", c_int),
        ("lda", c_long), ("ldb", c_long), ("ldc", c_long), ("ldcb", c_long),
        ("bias", c_void_p), ("res", c_void_p), ("ldr", c_long), ("res_mod", c_int),
        ("pre", c_void_p), ("aux", c_void_p), ("ldaux", c_long),
        ("act", c_int), ("accumulate", c_int), ("alpha", c_float),
        ("tc_d", c_int), ("tc_h", c_int), ("tc_w", c_int), ("tc_cout", c_int), ("x3", c_int),
    ]


class GroupedProblem(ctypes.Structure):
    _fields_ = [("dy", c_void_p), ("x", c_void_p), ("dw", c_void_p), ("M", c_int), ("N", c_int), ("K", c_int)]


class AdamWArena(ctypes.Structure):
    _fields_ = [("param", c_void_p), ("grad", c_void_p), ("m", c_void_p), ("v", c_void_p), ("shadow_bf16", c_void_p), ("steps", c_void_p),
                ("total", c_long), ("lr", c_float), ("beta1", c_float), ("beta2", c_float), ("eps", c_float), ("weight_decay", c_float),
                ("shadow_x3", c_void_p), ("hyper", c_void_p)]


class LrSchedule(ctypes.Structure):
    _fields_ = [("kind", c_int), ("base_lr", c_float), ("min_lr", c_float), ("warmup", c_float), ("total", c_float), ("power", c_float)]


class TransposeProblem(ctypes.Structure):
    _fields_ = [("offset", c_long), ("N", c_int), ("K", c_int)]


class PackProblem(ctypes.Structure):
    _fields_ = [("w", c_void_p), ("out", c_void_p), ("Cin", c_int), ("Cout", c_int), ("kind", c_int)]


class ReduceProblem(ctypes.Structure):
    _fields_ = [("part", c_void_p), ("dst", c_void_p), ("n", c_long), ("rows", c_int)]


class SplitProblem(ctypes.Structure):
    _fields_ = [("src", c_void_p), ("dst", c_void_p), ("rows", c_long), ("cols", c_long), ("second", c_int)]


class Prefetch(ctypes.Structure):
    _fields_ = [("ptr", c_void_p * 2), ("bytes", c_size_t * 2)]


class ColsumProblem(ctypes.Structure):
    _fields_ = [("x", c_void_p), ("out", c_void_p), ("ld", c_long), ("M", c_int), ("N", c_int), ("x_bf16", c_int)]


class AugDesc(ctypes.Structure):
    _fields_ = [("B", c_int), ("num_samples", c_int), ("C", c_int), ("L", c_int), ("S0", c_int), ("S1", c_int), ("S2", c_int),
                ("sampling", c_int), ("ax0", c_int), ("ax1", c_int), ("max_k", c_int), ("normalize", c_int),
                ("pos_ratio", c_double), ("flip_prob", c_double * 3), ("rot90_prob", c_double), ("shift_prob", c_double),
                ("shift_lo", c_double), ("shift_hi", c_double), ("seed", ctypes.c_uint64)]


class AugAffineDesc(ctypes.Structure):
    _fields_ = [("prob", c_double), ("rotate", c_double * 3), ("zoom_lo", c_double), ("zoom_hi", c_double), ("zoom_per_axis", c_int)]


class AugIntensityDesc(ctypes.Structure):      # index: noise std, blur sigma, brightness, contrast, gamma
    _fields_ = [("prob", c_double * 5), ("lo", c_double * 5), ("hi", c_double * 5)]


class SwVolume(ctypes.Structure):
    _fields_ = [("in_", c_void_p), ("out", c_void_p), ("count", c_void_p), ("table", c_void_p),
                ("B", c_int), ("Cin", c_int), ("C", c_int), ("Di", c_int), ("Hi", c_int), ("Wi", c_int),
                ("D", c_int), ("H", c_int), ("W", c_int), ("pz", c_int), ("py", c_int), ("px", c_int),
                ("cval", c_float), ("rows", c_int), ("cursor", c_int), ("activation", c_int)]


class RestoreGeom(ctypes.Structure):      # unetr_restore_geom, passed by value
    _fields_ = [("m", c_double * 12), ("full", c_int * 3), ("origin", c_int * 3), ("crop", c_int * 3)]


class SegLossDesc(ctypes.Structure):      # unetr_segloss_desc
    _fields_ = [("B", c_int), ("C", c_int), ("V", c_long), ("multilabel", c_int), ("region", c_int), ("voxel", c_int),
                ("include_background", c_int), ("squared_pred", c_int), ("batch", c_int), ("w_type", c_int),
                ("has_ignore", c_int), ("ignore_index", c_int),
                ("smooth_nr", c_float), ("smooth_dr", c_float), ("alpha", c_float), ("beta", c_float), ("gamma", c_float),
                ("lambda_region", c_float), ("lambda_voxel", c_float), ("class_weight", c_void_p)]


class EdtDesc(ctypes.Structure):      # unetr_edt_desc
    _fields_ = [("B", c_int), ("C", c_int), ("D", c_int), ("H", c_int), ("W", c_int),
                ("form", c_int), ("field", c_int), ("squared", c_int), ("accumulate", c_int), ("has_spacing", c_int),
                ("spacing", c_float * 3), ("alpha", c_float)]


class DistLossDesc(ctypes.Structure):      # unetr_distloss_desc
    _fields_ = [("B", c_int), ("C", c_int), ("V", c_long), ("multilabel", c_int), ("kind", c_int), ("include_background", c_int)]


class TopKCEDesc(ctypes.Structure):      # unetr_topkce_desc
    _fields_ = [("B", c_int), ("C", c_int), ("V", c_long), ("multilabel", c_int), ("has_ignore", c_int), ("ignore_index", c_int),
                ("class_weight", c_void_p)]


class SelectResult(ctypes.Structure):      # unetr_select_result
    _fields_ = [("value", c_float), ("n_beyond", ctypes.c_uint), ("n_equal", ctypes.c_uint)]


SELECT_LARGEST, SELECT_PLAIN_HIST = 1, 2      # = UNETR_SELECT_*

SW_MAX_BATCH = 16                     # = UNETR_SW_MAX_BATCH
SW_ROW_INTS = 4 + 4 * SW_MAX_BATCH     # = UNETR_SW_ROW_INTS

P = c_void_p
_SIGNATURES = {
    "unetr_abi_version": [],
    "unetr_gemm": [ctypes.POINTER(GemmDesc), P, P, P, P, c_size_t, P],
    "unetr_gemm_bf16": [ctypes.POINTER(GemmBf16Desc), P, P, P, P, P, c_size_t, P],
    "unetr_gemm_bf16_ln_bwd": [ctypes.POINTER(GemmBf16Desc), P, P, P, P, P, P, P, P, P, P, P, P, P, c_size_t, P, c_size_t, P],
    "unetr_gemm_bf16_ln_bwd_pf": [ctypes.POINTER(GemmBf16Desc), P, P, P, P, P, P, P, P, P, P, P, P, P, c_size_t, P, c_size_t, P, ctypes.POINTER(Prefetch)],
    "unetr_gemm_bf16_ln_fwd": [ctypes.POINTER(GemmBf16Desc), P, P, P, P, P, c_float, P, P, P, P, P, c_size_t, P],
    "unetr_gemm_bf16_ln_fwd_pf": [ctypes.POINTER(GemmBf16Desc), P, P, P, P, P, c_float, P, P, P, P, P, c_size_t, P, ctypes.POINTER(Prefetch)],
    "unetr_cast_bf16": [P, P, c_long, P],
    "unetr_split_words": [P, P, c_long, P],
    "unetr_split_stack_bf16": [P, P, c_long, c_long, c_int, P],
    "unetr_split_stack_bf16_grouped": [ctypes.POINTER(SplitProblem), c_int, P],
    "unetr_attention_bf16_fwd": [P, P, P, P, c_int, c_int, c_int, c_int, c_float, P],
    "unetr_attention_bf16_fwd_pf": [P, P, P, P, c_int, c_int, c_int, c_int, c_float, P, ctypes.POINTER(Prefetch)],
    "unetr_attention_bf16_bwd": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P],
    "unetr_attention_bf16_bwd_pf": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, P, ctypes.POINTER(Prefetch)],
    "unetr_gemm_grouped_wgrad": [ctypes.POINTER(GroupedProblem), c_int, c_int, P],
    "unetr_gemm_bf16_grouped_wgrad": [ctypes.POINTER(GroupedProblem), c_int, P],
    "unetr_gemm_bf16_grouped_wgrad_adamw": [ctypes.POINTER(GroupedProblem), c_int, ctypes.POINTER(AdamWArena), ctypes.POINTER(c_int), P],
    "unetr_gemm_bf16_grouped_wgrad_adamw_t": [ctypes.POINTER(GroupedProblem), c_int, ctypes.POINTER(AdamWArena), ctypes.POINTER(c_int), P, P],
    "unetr_transpose_bf16_grouped": [P, P, ctypes.POINTER(TransposeProblem), c_int, P],
    "unetr_adamw_ranges": [ctypes.POINTER(AdamWArena), P, c_int, c_long, P],
    "unetr_gemm_bf16_grouped_wgrad_bf16out": [ctypes.POINTER(GroupedProblem), c_int, P, P, c_long, P],
    "unetr_cast_bf16_ranges": [P, P, P, c_int, c_long, P],
    "unetr_colsum_grouped": [ctypes.POINTER(ColsumProblem), c_int, P],
    "unetr_tconv_fwd": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv_dgrad": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv_wgrad": [P, c_long, P, c_long, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv2_fwd": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv2_wgrad": [P, c_long, P, c_long, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv2_dgrad": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_tconv2_fwd_supported": [c_long, c_int, c_int, c_long, c_long],
    "unetr_tconv2_wgrad_supported": [c_long, c_int, c_int, c_long, c_long],
    "unetr_pixel_shuffle2": [P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_pixel_unshuffle2_bf16": [P, c_long, P, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_colsum": [P, c_long, c_int, c_int, P, c_int, P, c_size_t, P],
    "unetr_layernorm_fwd": [P, P, P, P, P, P, P, c_int, c_int, c_float, P],
    "unetr_layernorm_fwd_pf": [P, P, P, P, P, P, P, c_int, c_int, c_float, P, ctypes.POINTER(Prefetch)],
    "unetr_layernorm_bwd": [P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, c_size_t, P],
    "unetr_layernorm_bwd_pf": [P, P, P, P, P, P, P, P, P, P, c_int, c_int, P, c_size_t, P, ctypes.POINTER(Prefetch)],
    "unetr_attention_fwd": [P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_int, P],
    "unetr_attention_bwd": [P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_float, c_int, P],
    "unetr_conv_pack_weight": [P, P, c_int, c_int, c_int, c_int, P],
    "unetr_conv_gemm_fwd": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_conv_gemm_wgrad": [P, c_long, P, c_long, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_conv3_pack_weight": [P, P, c_int, c_int, c_int, c_int, P],
    "unetr_conv3_fwd": [P, c_long, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_conv3_fwd_fused": [P, c_long, P, P, c_long, P, P, P, c_long, P, c_float, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_conv3_fwd_parts": [P, c_long, P, P, c_long, P, P, P, c_long, P, ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_conv3_slab_dispatch": [c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_int)],
    "unetr_conv3_dgrad_stats": [P, c_long, P, P, c_long, P, c_long, P, P, ctypes.POINTER(c_int), c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_instnorm_apply_fin": [P, c_long, P, c_int, P, c_long, P, c_int, P, P, c_float, P, c_long, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_instnorm_apply_fin_img": [P, c_long, P, c_int, P, c_int, P, P, c_int, P, P, c_float, P, c_long, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_instnorm_bwd_img": [P, c_long, P, c_long, P, P, c_int, P, P, P, c_long, P, ctypes.POINTER(c_int), c_int, c_long, c_int, c_int, P, c_size_t, c_int, P],
    "unetr_instnorm_bwd_apply_fin": [P, c_long, P, c_long, P, P, c_long, P, P, c_int, c_int, P, c_long, P, c_long, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_conv3_wgrad_parts": [P, c_long, P, c_long, P, c_long, P, c_size_t, ctypes.POINTER(c_long), c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_tconv2_wgrad_parts": [P, c_long, P, c_long, P, c_size_t, ctypes.POINTER(c_long), c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_reduce_rows_grouped": [ctypes.POINTER(ReduceProblem), c_int, P],
    "unetr_conv3_dgrad_fused": [P, c_long, P, P, c_long, P, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_conv3_pack_grouped": [ctypes.POINTER(PackProblem), c_int, c_int, P],
    "unetr_conv3_pack_1x1": [P, P, c_int, c_int, c_int, P],
    "unetr_instnorm_stats_finalize": [P, c_int, c_int, c_long, c_int, c_float, P, P],
    "unetr_conv3_wgrad": [P, c_long, P, c_long, P, P, c_long, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_debug_tr16": [P, P, P],
    "unetr_instnorm_stats": [P, c_long, c_int, c_long, c_int, c_float, P, P, c_size_t, c_int, P],
    "unetr_instnorm_apply": [P, c_long, P, P, c_long, P, P, c_long, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_instnorm_bwd": [P, c_long, P, c_long, P, P, c_long, P, P, c_long, P, c_long, c_int, c_long, c_int, c_int, P, c_size_t, c_int, P],
    "unetr_nchw_to_nhwc": [P, P, c_long, c_int, c_int, c_long, c_int, P],
    "unetr_nhwc_to_nchw": [P, c_long, P, c_int, c_int, c_long, c_int, c_int, P],
    "unetr_patch_gather": [P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_counter_add": [P, P, c_int, P],
    "unetr_counter_add_lr": [P, P, c_int, P, ctypes.POINTER(LrSchedule), P],
    "unetr_adamw_hyper_set": [P, c_int, c_float, c_float, c_float, P],
    "unetr_add_cast_bf16": [P, P, P, P, c_long, P],
    "unetr_copy_rows": [P, c_long, P, c_long, c_long, c_int, c_int, c_int, P],
    "unetr_outconv_fwd": [P, c_long, P, P, P, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_outconv_bwd": [P, P, c_long, P, P, c_long, P, P, c_int, c_long, c_int, c_int, P, c_size_t, c_int, P],
    "unetr_outconv_in_fwd": [P, c_long, P, c_int, P, c_long, P, c_int, P, P, c_float, P, P, P, c_int, c_long, c_int, c_int, c_int, P],
    "unetr_outconv_in_bwd": [P, P, c_long, P, P, c_long, P, P, P, c_long, P, P, P, c_int, c_long, c_int, c_int, P, c_size_t, c_int, P],
    "unetr_dicece_fwd": [P, P, c_int, c_int, c_long, c_int, c_float, c_float, P, P, P, c_size_t, P],
    "unetr_dicece_bwd": [P, P, P, P, P, c_int, c_int, c_long, c_int, P],
    "unetr_segloss_fwd": [ctypes.POINTER(SegLossDesc), P, P, P, P, P, c_size_t, P],
    "unetr_segloss_bwd": [ctypes.POINTER(SegLossDesc), P, P, P, P, P, P],
    "unetr_edt": [ctypes.POINTER(EdtDesc), P, P, P, c_size_t, P],
    "unetr_distloss_fwd": [ctypes.POINTER(DistLossDesc), P, P, P, P, P, P, c_size_t, P],
    "unetr_distloss_bwd": [ctypes.POINTER(DistLossDesc), P, P, P, P, P, P, P],
    "unetr_select_kth": [P, c_long, P, c_int, c_int, P, P, c_size_t, P],
    "unetr_topkce_fwd": [ctypes.POINTER(TopKCEDesc), P, P, P, P, P, P, P, c_size_t, P],
    "unetr_topkce_bwd": [ctypes.POINTER(TopKCEDesc), P, P, P, P, P, P, P],
    "unetr_sw_accumulate": [P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_sw_finalize": [P, P, c_int, c_int, c_long, P],
    "unetr_dice_counts": [P, P, c_int, c_int, c_long, c_int, P, P, c_size_t, P],
    "unetr_sw_advance": [P, P],
    "unetr_sw_gather_batch": [P, P, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_sw_accumulate_batch": [P, P, P, c_int, c_int, c_int, c_int, c_int, P],
    "unetr_sw_finalize_post": [P, P, P, c_int, c_int, c_long, c_int, P],
    "unetr_sw_rewind": [P, P],
    "unetr_sw_finalize_post_thr": [P, P, P, c_int, c_int, c_long, c_int, c_float, P],
    "unetr_hausdorff": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_double, c_int, P, P, c_size_t, c_int, P],
    "unetr_surface_metrics": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_double), ctypes.POINTER(c_double), c_int,
                              ctypes.POINTER(c_double), P, P, c_size_t, c_int, P],
    "unetr_aug_prep": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_int, P, P, P],
    "unetr_aug_crop": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P],
    "unetr_aug_index_count": [P, P, c_int, c_int, c_long, c_float, P, c_size_t, P],
    "unetr_aug_index_scatter": [P, P, c_int, c_int, c_long, c_float, P, c_size_t, P, P, P],
    "unetr_aug_sample": [ctypes.POINTER(AugDesc), P, c_int, P, P, P, P],
    "unetr_aug_gather": [ctypes.POINTER(AugDesc), P, c_int, P, P, P, P, c_size_t, P],
    "unetr_aug_sample_affine": [ctypes.POINTER(AugDesc), ctypes.POINTER(AugAffineDesc), P, c_int, P, P, P, P, P],
    "unetr_aug_gather_affine": [ctypes.POINTER(AugDesc), P, c_int, P, P, P, P, P, c_size_t, P],
    "unetr_aug_intensity_sample": [ctypes.POINTER(AugDesc), ctypes.POINTER(AugIntensityDesc), P, P, P],
    "unetr_aug_intensity_apply": [ctypes.POINTER(AugDesc), P, P, P, c_size_t, P],
    "unetr_aug_class_count": [P, P, c_int, c_int, c_int, c_long, c_int, c_float, P, c_size_t, P, P],
    "unetr_aug_class_scatter": [P, P, c_int, c_int, c_int, c_long, c_int, c_float, P, c_size_t, P, P, P],
    "unetr_aug_sample_classes": [ctypes.POINTER(AugDesc), ctypes.POINTER(AugAffineDesc), P, c_int, P, c_int, P, P, P, P, P, P, P],
    "unetr_resample_orient": [P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_double), c_int, c_int, c_int, P, P, P],
    "unetr_restore_native": [P, c_int, c_int, RestoreGeom, c_int, c_int, c_int, c_int, c_int, c_int, P, P],
    "unetr_ccl": [P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint, c_int, c_int, c_int, c_int, P, c_size_t, c_int, P],
    "unetr_morph": [P, P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, P, c_size_t, P],
    "unetr_fill_holes": [P, P, c_int, P, c_int, c_int, c_int, c_int, c_int, c_int, ctypes.c_uint, c_int, P, c_size_t, P],
    "unetr_label_overlaps": [P, P, P, c_long, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, c_size_t, c_int, P],
    "unetr_ranking_loss_fwd": [P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, P, P, P, c_size_t, P],
    "unetr_ranking_loss_bwd": [P, c_int, c_int, c_int, c_int, c_int, c_int, P, P, P, P],
    "unetr_adamw": [P, P, P, P, c_long, c_float, c_float, c_float, c_float, c_float, P, P, P],
    "unetr_adamw_reduced": [P, P, c_int, c_float, P, P, c_long, c_float, c_float, c_float, c_float, c_float, P, P, P, P],
    "unetr_adamw_hyper": [P, P, c_int, c_float, P, P, c_long, P, c_float, c_float, c_float, P, P, P, P],
    "unetr_adamw_hyper_clip": [P, P, c_int, c_float, P, P, c_long, P, c_float, c_float, c_float, P, P, P, P, P],
    "unetr_grad_sumsq_ranges": [P, c_int, P, c_int, c_long, P, c_size_t, P],
    "unetr_grad_sumsq": [P, c_int, c_long, P, c_size_t, P],
    "unetr_grad_clip_finalize": [P, c_long, c_float, P, P],
    "unetr_grad_clip_set": [P, c_float, P],
    "unetr_grad_scale_ranges": [P, P, c_int, c_long, P, P],
    "unetr_grad_scale": [P, c_long, P, P],
}

EXPORTED_SYMBOLS = tuple(_SIGNATURES) + ("unetr_conv3_packed_bytes", "unetr_conv3_packed_1x1_bytes", "unetr_ranking_workspace_floats",
                                            "unetr_conv3_wgrad_rows", "unetr_tconv2_wgrad_rows", "unetr_outconv_in_bwd_rows", "unetr_hausdorff_workspace_bytes",
                                            "unetr_aug_index_ws_ints", "unetr_aug_gather_ws_bytes", "unetr_aug_gather_affine_ws_bytes", "unetr_ccl_workspace_bytes",
                                            "unetr_surface_metrics_workspace_bytes", "unetr_aug_intensity_ws_bytes", "unetr_segloss_workspace_bytes",
                                            "unetr_aug_class_ws_ints", "unetr_edt_workspace_bytes", "unetr_distloss_workspace_bytes",
                                            "unetr_select_workspace_bytes", "unetr_topkce_workspace_bytes", "unetr_morph_workspace_bytes",
                                            "unetr_fill_holes_workspace_bytes", "unetr_label_overlaps_workspace_bytes")

_lib = None


def load():
    """Load libunetr_hip.so once; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} is missing: the HIP extension is not built. Run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` or `make -C {os.path.join(_HERE, 'csrc')}`. There is no CPU/PyTorch fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    lib.unetr_abi_version.restype = c_int
    got = lib.unetr_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"{LIB_PATH} reports C-ABI version {got}, this binding was written against {ABI_VERSION}: the "
                           f"library is stale -- rebuild the extension (`make -C {os.path.join(_HERE, 'csrc')}`).")
    for name, argtypes in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.argtypes = argtypes
        fn.restype = c_int
    lib.unetr_conv3_packed_bytes.argtypes = [c_int, c_int, c_int, c_int]
    lib.unetr_conv3_packed_bytes.restype = c_size_t
    lib.unetr_conv3_packed_1x1_bytes.argtypes = [c_int, c_int, c_int]
    lib.unetr_conv3_packed_1x1_bytes.restype = c_size_t
    lib.unetr_conv3_wgrad_rows.argtypes = [c_int] * 9
    lib.unetr_conv3_wgrad_rows.restype = c_long
    lib.unetr_tconv2_wgrad_rows.argtypes = [c_int] * 6
    lib.unetr_tconv2_wgrad_rows.restype = c_long
    lib.unetr_outconv_in_bwd_rows.argtypes = [c_int, c_long, c_int, c_int]
    lib.unetr_outconv_in_bwd_rows.restype = c_long
    lib.unetr_ranking_workspace_floats.argtypes = [c_int, c_int, c_int, c_int, c_int]
    lib.unetr_ranking_workspace_floats.restype = c_size_t
    lib.unetr_hausdorff_workspace_bytes.argtypes = [c_int] * 7
    lib.unetr_hausdorff_workspace_bytes.restype = c_size_t
    lib.unetr_surface_metrics_workspace_bytes.argtypes = [c_int] * 7
    lib.unetr_surface_metrics_workspace_bytes.restype = c_size_t
    lib.unetr_ccl_workspace_bytes.argtypes = [c_int] * 4
    lib.unetr_ccl_workspace_bytes.restype = c_size_t
    lib.unetr_aug_index_ws_ints.argtypes = [c_long]
    lib.unetr_aug_index_ws_ints.restype = c_long
    lib.unetr_aug_gather_ws_bytes.argtypes = [ctypes.POINTER(AugDesc)]
    lib.unetr_aug_gather_ws_bytes.restype = c_size_t
    lib.unetr_aug_gather_affine_ws_bytes.argtypes = [ctypes.POINTER(AugDesc)]
    lib.unetr_aug_gather_affine_ws_bytes.restype = c_size_t
    lib.unetr_aug_intensity_ws_bytes.argtypes = [ctypes.POINTER(AugDesc)]
    lib.unetr_aug_intensity_ws_bytes.restype = c_size_t
    lib.unetr_aug_class_ws_ints.argtypes = [c_long, c_int]
    lib.unetr_aug_class_ws_ints.restype = c_long
    lib.unetr_segloss_workspace_bytes.argtypes = [ctypes.POINTER(SegLossDesc)]
    lib.unetr_segloss_workspace_bytes.restype = c_size_t
    lib.unetr_edt_workspace_bytes.argtypes = [ctypes.POINTER(EdtDesc)]
    lib.unetr_edt_workspace_bytes.restype = c_size_t
    lib.unetr_distloss_workspace_bytes.argtypes = [ctypes.POINTER(DistLossDesc)]
    lib.unetr_distloss_workspace_bytes.restype = c_size_t
    lib.unetr_select_workspace_bytes.argtypes = [c_long]
    lib.unetr_select_workspace_bytes.restype = c_size_t
    lib.unetr_topkce_workspace_bytes.argtypes = [ctypes.POINTER(TopKCEDesc)]
    lib.unetr_topkce_workspace_bytes.restype = c_size_t
    lib.unetr_morph_workspace_bytes.argtypes = [c_int] * 4
    lib.unetr_morph_workspace_bytes.restype = c_size_t
    lib.unetr_fill_holes_workspace_bytes.argtypes = [c_int] * 5
    lib.unetr_fill_holes_workspace_bytes.restype = c_size_t
    lib.unetr_label_overlaps_workspace_bytes.argtypes = [c_int] * 5
    lib.unetr_label_overlaps_workspace_bytes.restype = c_size_t
    _lib = lib
    return lib


def call_rc(name, *args):
    """like call(), but hands 'unsupported shape' (3) back to the caller, which then takes the unfused route"""
    rc = getattr(load(), name)(*args)
    if rc not in (0, 3):
        raise RuntimeError(f"{name} failed: {_ERR.get(rc, rc)}")
    return rc


def call(name, *args):
    rc = getattr(load(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed: {_ERR.get(rc, rc)}")
