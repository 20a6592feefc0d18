"""ctypes binding of ``libloco_hip.so`` (C ABI: ``include/loco_hip.h``).

PyTorch is used only as the owner of device memory and the current HIP stream;
every numerical operation below is a call into the hand-written gfx950 kernels.
There is NO fallback: a missing library or a missing GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, Optional

import numpy as np
import torch

from .config import UNetConfig

# LOCO_HIP_LIB: alternative build of the same library (A/B timing of kernel variants); default = the in-tree build
_LIB_PATH = os.environ.get("LOCO_HIP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "libloco_hip.so")
_lib = None

# diagnostics of include/loco_hip_diag.h: only in a -DLOCO_DIAG build (make -C loco-edit_amd/csrc diag)
DIAG_SYMBOLS = ["loco_bench_conv", "loco_debug_conv", "loco_debug_attn", "loco_debug_norm", "loco_debug_gemm", "loco_debug_pointwise",
                "loco_debug_enc_attn", "loco_debug_tensor"]

# every symbol include/loco_hip.h declares
SYMBOLS = [
    "loco_version", "loco_device_count", "loco_create", "loco_fork", "loco_destroy", "loco_last_error",
    "loco_load_param", "loco_params_missing", "loco_unet_forward", "loco_ddim_step", "loco_sched_step",
    "loco_pmp_primal", "loco_pmp_set_second_mask", "loco_pmp_jvp", "loco_pmp_vjp", "loco_pmp_vjp_context", "loco_orthonormalize", "loco_qr_rows",
    "loco_convergence", "loco_convergence_rows", "loco_krylov_extend", "loco_krylov_ritz", "loco_krylov_left", "loco_null_project", "loco_edit_axpy", "loco_mask_gather", "loco_mask_count",
    "loco_unet_flops", "loco_workspace_bytes", "loco_clock_stamp", "loco_set_side_stream", "loco_timer_start", "loco_timer_stop",
    "loco_profile_enable", "loco_profile_report", "loco_set_precision", "loco_get_precision", "loco_set_streams", "loco_set_chip_share",
    "loco_set_cond", "loco_set_context", "loco_lincomb", "loco_masked_axpby", "loco_latent_sample",
    "loco_text_create", "loco_text_load_param", "loco_text_params_missing", "loco_text_encode", "loco_text_last_error",
    "loco_text_destroy", "loco_t5_create", "loco_text_encode_masked",
    "loco_diffedit_mask", "loco_cfg_masked_step", "loco_set_time_cond", "loco_lcm_step",
    "loco_h_dims", "loco_unet_get_h", "loco_unet_forward_dh", "loco_pmp_primal_tap", "loco_pmp_primal_eps", "loco_pmp_primal_tap_dh", "loco_sched_step_asym",
    "loco_sam_create", "loco_sam_load_param", "loco_sam_params_missing", "loco_sam_encode", "loco_sam_profile",
    "loco_sam_profile_read", "loco_sam_last_error", "loco_sam_destroy",
    "loco_samdec_create", "loco_samdec_load_param", "loco_samdec_params_missing", "loco_samdec_set_image", "loco_samdec_predict",
    "loco_samdec_score", "loco_samdec_binarize", "loco_samdec_last_error", "loco_samdec_destroy",
    "loco_clipvis_create", "loco_clipvis_load_param", "loco_clipvis_params_missing", "loco_clipvis_preprocess",
    "loco_clipvis_encode", "loco_clipvis_last_error", "loco_clipvis_destroy",
    "loco_clipvis_enable_grad", "loco_clipvis_grad_bytes", "loco_clipvis_encode_vjp", "loco_clipvis_preprocess_f32",
    "loco_clipvis_preprocess_f32_vjp", "loco_clipvis_encode_taps",
    "loco_clipseg_create", "loco_clipseg_load_param", "loco_clipseg_params_missing", "loco_clipseg_logit_size", "loco_clipseg_decode",
    "loco_clipseg_preprocess", "loco_clipseg_masks", "loco_clipseg_last_error", "loco_clipseg_destroy",
    "loco_quality_create", "loco_quality_load_param", "loco_quality_params_missing", "loco_quality_lpips", "loco_quality_ssim",
    "loco_quality_masked_mse", "loco_quality_last_error", "loco_quality_destroy",
    "loco_pca_create", "loco_pca_reset", "loco_pca_rows", "loco_pca_add_rows", "loco_pca_fit", "loco_pca_center", "loco_pca_gram",
    "loco_pca_project", "loco_pca_set_route", "loco_pca_routes", "loco_pca_last_error", "loco_pca_destroy",
    "loco_asyrp_create", "loco_asyrp_load_param", "loco_asyrp_params_missing", "loco_asyrp_read_param", "loco_asyrp_read_grad",
    "loco_asyrp_forward", "loco_asyrp_backward", "loco_asyrp_zero_grad", "loco_asyrp_adam_step", "loco_asyrp_reset_moments",
    "loco_asyrp_last_error", "loco_asyrp_destroy",
]

# operators of loco_pmp_primal_tap (include/loco_hip.h): None x_t -> x0 / eps, "enc" x_t -> h, "dec" h -> eps
TAPS = {None: 0, "enc": 1, "dec": 2}

# threshold rules of loco_diffedit_mask (include/loco_hip.h)
DIFFEDIT_RULES = {"reference": 0, "intended": 1}


class LocoCfg(C.Structure):
    _fields_ = [
        ("struct_size", C.c_int32), ("resolution", C.c_int32), ("in_channels", C.c_int32), ("out_ch", C.c_int32), ("ch", C.c_int32),
        ("num_levels", C.c_int32), ("ch_mult", C.c_int32 * 8), ("num_res_blocks", C.c_int32),
        ("num_attn_res", C.c_int32), ("attn_resolutions", C.c_int32 * 8), ("gn_groups", C.c_int32),
        ("gn_eps", C.c_float), ("max_batch", C.c_int32),
        ("arch", C.c_int32), ("num_head_channels", C.c_int32), ("learn_sigma", C.c_int32),
        ("context_dim", C.c_int32), ("context_len", C.c_int32),
        ("scale_shift_norm", C.c_int32), ("resblock_updown", C.c_int32), ("num_heads", C.c_int32),
        ("transformer_depth", C.c_int32),
        ("act", C.c_int32), ("res_scale", C.c_float), ("added_kv", C.c_int32),
        ("time_cond_proj_dim", C.c_int32),
    ]


class LocoConvDesc(C.Structure):
    """loco_conv_desc of include/loco_hip_diag.h (loco_debug_conv): one conv launch on caller-supplied operands."""
    _PTRS = ("weight", "bias", "in", "bias2", "res", "prim", "sc", "sh", "mr", "gamma", "tst", "tc", "in2", "w2", "bias2nd",
             "cot_d", "cot_prim", "cot_sc", "cot_sh", "cot_mr", "cot_tc", "out", "st_prim", "st_mr", "st_out")
    _ST_PTRS = ("st_gamma", "st_beta", "st_ss_scale", "st_ss_shift", "st_sc", "st_sh", "st_o_mr", "st_o_sc", "st_o_sh", "st_o_tst",
                "st_o_tc", "st_keep_out")
    _HOST = ("weight", "bias", "w2", "bias2nd")
    _fields_ = ([("struct_size", C.c_int32)] +
                [(k, C.c_int32) for k in ("Cin", "Cout", "Hin", "Win", "B", "taps", "stride", "upsample", "zins", "mode", "cpg",
                                          "transposed", "accumulate", "in_arena", "pad", "Cin2", "cot_cpg")] +
                [("res_scale", C.c_float), ("st_cpg", C.c_int32)] + [(k, C.c_void_p) for k in _PTRS] + [("pool2", C.c_int32)] +
                [("st_kind", C.c_int32), ("st_keep", C.c_int32), ("st_eps", C.c_float), ("st_keep_cap", C.c_int32)] +
                [(k, C.c_void_p) for k in _ST_PTRS])
    _PTRS = _PTRS + _ST_PTRS


class LocoNormDesc(C.Structure):
    """loco_norm_desc of include/loco_hip_diag.h (loco_debug_norm): one launch of one standalone GroupNorm launcher."""
    OPS = {"gn_stats": 0, "gn_tstats": 1, "gn_apply": 2, "gn_cache": 3, "gn_fused_finalize": 4, "gn_fused_finalize_cat": 5,
           "gn_lin_fused_finalize": 6, "ctx_groupnorm": 7}
    _PTRS = ("x", "d", "base", "gamma", "beta", "ss_scale", "ss_shift", "sc", "sh", "mr", "tst", "partA", "partB",
             "o_mr", "o_sc", "o_sh", "o_tst", "o_tc", "out")
    _fields_ = ([("struct_size", C.c_int32)] +
                [(k, C.c_int32) for k in ("op", "kind", "act", "B", "C", "HW", "G", "C1", "ntA", "ntB", "accumulate")] +
                [("eps", C.c_float), ("base_scale", C.c_float)] +
                [(k, C.c_int64) for k in ("x_bs", "d_bs", "base_bs", "out_bs", "pbs_c", "pbs_g", "o_bs", "t_bs")] +
                [(k, C.c_void_p) for k in _PTRS])


class LocoPointwiseDesc(C.Structure):
    """loco_pointwise_desc of include/loco_hip_diag.h (loco_debug_pointwise): one launch of one token-wise / pointwise launcher."""
    OPS = {"ln_fwd": 0, "ln_tan": 1, "ln_cot": 2, "geglu": 3, "temb": 4, "temb_proj": 5, "pool2x2_sum": 6, "upsample2x": 7, "copy": 8,
           "masked_axpby": 9, "cot_seed": 10, "ddim_step": 11, "latent_sample": 12, "lincomb": 13, "add": 14}
    _PTRS = ("x", "y", "stats", "gamma", "beta", "base", "freq", "w0", "b0", "w1", "b1", "add", "add_in")
    _MASKS = ("mask", "mask2")
    _OUTS = ("out", "out2", "t_dev")
    _fields_ = ([("struct_size", C.c_int32)] +
                [(k, C.c_int32) for k in ("op", "kind", "act", "B", "C", "T", "H", "W", "n", "k", "accumulate", "cos_first")] +
                [(k, C.c_float) for k in ("eps", "scale", "t", "cv", "ce")] + [("f", C.c_float * 5), ("pad_", C.c_int32)] +
                [(k, C.c_int64) for k in ("count", "split", "in_bs", "out_bs", "aux_bs", "st_bs")] +
                [(k, C.c_void_p) for k in _PTRS] + [("src", C.c_void_p * 4)] + [(k, C.c_void_p) for k in _MASKS + _OUTS])


class LocoAttnDesc(C.Structure):
    """loco_attn_desc of include/loco_hip_diag.h (loco_debug_attn): one pass of one attention stage on caller-supplied tensors."""
    _PTRS = ("q", "k", "v", "kt", "vt", "P", "o", "dq", "dk", "dv", "out", "go", "gq", "gk", "gv")
    _fields_ = ([("struct_size", C.c_int32)] +
                [(k, C.c_int32) for k in ("kind", "pass_", "T", "NH", "CH", "B", "Lt", "L", "pair", "no_workspace")] +
                [(k, C.c_void_p) for k in _PTRS])


class LocoEncAttnDesc(C.Structure):
    """loco_enc_attn_desc of include/loco_hip_diag.h (loco_debug_enc_attn): one launch of one attention kernel of the encoders."""
    OPS = {"enc_attn": 0, "enc_attn_keep": 1, "enc_attn_bias": 2, "prompt_attn_causal": 3, "prompt_attn_bias": 4,
           "clipvis_attn_cot_q": 5, "clipvis_attn_cot_kv": 6, "seg_attn": 7, "sd_t2i": 8, "sd_i2t": 9}
    _PTRS = ("qkv", "relh", "relw", "bias_tab", "o", "go", "q", "k", "v", "lens", "out", "ml", "gqkv", "delta")
    _fields_ = ([("struct_size", C.c_int32)] +
                [(k, C.c_int32) for k in ("op", "D", "hd", "heads", "nk", "groups", "size", "NQ", "Tp")] +
                [(k, C.c_int64) for k in ("ld", "Tall", "kbs", "qbs")] + [("scale", C.c_float), ("pad2_", C.c_int32)] +
                [(k, C.c_void_p) for k in _PTRS])


class LocoGemmProb(C.Structure):
    """loco_gemm_prob of include/loco_hip_diag.h: one problem slot of loco_debug_gemm, GemmArgs field by field."""
    _PTRS = ("A", "B", "A2", "B2", "bias", "colbias", "R", "C")
    _STRIDES = ("sam", "sak", "sab", "sah", "sbk", "sbn", "sbb", "sbh", "scm", "scn", "scb", "sch", "srb", "sab2", "sbb2")
    _fields_ = ([(k, C.c_void_p) for k in _PTRS] + [(k, C.c_int64) for k in _STRIDES] +
                [("n_" + k, C.c_int64) for k in ("A", "B", "A2", "B2", "bias", "colbias", "R", "C")] +
                [(k, C.c_int32) for k in ("M", "N", "K", "batch", "batch2")] + [("alpha", C.c_float), ("beta", C.c_float), ("pad_", C.c_int32)])


class LocoGemmDesc(C.Structure):
    """loco_gemm_desc of include/loco_hip_diag.h (loco_debug_gemm): one call of one GEMM launcher on caller-supplied tensors."""
    OPS = {"gemm": 0, "gemm_fixed": 1, "gemm_bf16x3": 2, "gemm_rec": 3, "gemm_pair": 4}
    ACTS = {"none": 0, "quick_gelu": 1, "gelu": 2}
    _fields_ = [("struct_size", C.c_int32), ("op", C.c_int32), ("act", C.c_int32), ("pad_", C.c_int32), ("p", LocoGemmProb * 2)]


class LocoTextCfg(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("width", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32), ("ffn", C.c_int32),
                ("positions", C.c_int32), ("act", C.c_int32), ("ln_eps", C.c_float)]


class LocoT5Cfg(C.Structure):
    _fields_ = [("vocab", C.c_int32), ("d_model", C.c_int32), ("d_kv", C.c_int32), ("heads", C.c_int32), ("d_ff", C.c_int32),
                ("layers", C.c_int32), ("positions", C.c_int32), ("buckets", C.c_int32), ("max_distance", C.c_int32),
                ("act", C.c_int32), ("ln_eps", C.c_float)]


SAM_MAX_GLOBAL = 16


class LocoSamCfg(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("width", C.c_int32), ("depth", C.c_int32),
                ("heads", C.c_int32), ("mlp_dim", C.c_int32), ("window_size", C.c_int32), ("num_global", C.c_int32),
                ("global_attn", C.c_int32 * SAM_MAX_GLOBAL), ("out_channels", C.c_int32), ("ln_eps", C.c_float)]


class LocoSamDecCfg(C.Structure):
    _fields_ = [("grid", C.c_int32), ("image_size", C.c_int32), ("hidden", C.c_int32), ("layers", C.c_int32), ("heads", C.c_int32),
                ("mlp_dim", C.c_int32), ("attention_downsample_rate", C.c_int32), ("num_multimask_outputs", C.c_int32),
                ("iou_head_depth", C.c_int32), ("iou_head_hidden_dim", C.c_int32), ("layer_norm_eps", C.c_float),
                ("hidden_act", C.c_int32), ("max_prompts", C.c_int32)]


class LocoClipVisCfg(C.Structure):
    _fields_ = [("image_size", C.c_int32), ("patch_size", C.c_int32), ("width", C.c_int32), ("layers", C.c_int32),
                ("heads", C.c_int32), ("mlp_dim", C.c_int32), ("projection_dim", C.c_int32), ("act", C.c_int32),
                ("ln_eps", C.c_float), ("image_mean", C.c_float * 3), ("image_std", C.c_float * 3)]


class LocoClipSegCfg(C.Structure):
    _fields_ = [("width", C.c_int32), ("grid", C.c_int32), ("patch_size", C.c_int32), ("reduce_dim", C.c_int32), ("heads", C.c_int32),
                ("ffn", C.c_int32), ("n_taps", C.c_int32), ("conditional_layer", C.c_int32), ("projection_dim", C.c_int32),
                ("complex_head", C.c_int32), ("ln_eps", C.c_float), ("max_masks", C.c_int32)]


class LocoQualityCfg(C.Structure):
    _fields_ = [("max_h", C.c_int32), ("max_w", C.c_int32), ("ssim_window", C.c_double * 11)]


def library_path() -> str:
    return _LIB_PATH


def load_library():
    """dlopen the engine and declare prototypes.  Raises if it was not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise RuntimeError(
            f"{_LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(_LIB_PATH)
    vp, i32, i64, f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float
    lib.loco_version.restype = C.c_char_p
    lib.loco_device_count.restype = C.c_int
    lib.loco_create.argtypes = [C.POINTER(LocoCfg), C.POINTER(vp)]
    if hasattr(lib, "loco_fork"):      # (a library of an earlier round, loaded by LOCO_HIP_LIB for an A/B: everything but fork works)
        lib.loco_fork.argtypes = [vp, C.c_int32, C.POINTER(vp)]
    lib.loco_destroy.argtypes = [vp]
    lib.loco_destroy.restype = None
    lib.loco_last_error.argtypes = [vp]
    lib.loco_last_error.restype = C.c_char_p
    lib.loco_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32, i32]
    lib.loco_params_missing.argtypes = [vp]
    lib.loco_unet_forward.argtypes = [vp, vp, f32, i32, vp, vp]
    lib.loco_ddim_step.argtypes = [vp, vp, f32, f32, f32, f32, vp, i32, vp, vp]
    lib.loco_sched_step.argtypes = [vp, vp, vp, f32, f32, f32, vp, i64, vp, vp, vp]
    if hasattr(lib, "loco_sched_step_asym"):
        lib.loco_sched_step_asym.argtypes = [vp, vp, vp, vp, f32, f32, i64, vp, vp, vp]
    lib.loco_pmp_primal.argtypes = [vp, vp, f32, f32, vp, i32, vp]
    lib.loco_pmp_set_second_mask.argtypes = [vp, vp, i32, vp]
    lib.loco_h_dims.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i32)]
    lib.loco_unet_get_h.argtypes = [vp, vp, f32, i32, vp, vp]
    lib.loco_unet_forward_dh.argtypes = [vp, vp, f32, i32, vp, vp, vp]
    lib.loco_pmp_primal_tap.argtypes = [vp, vp, f32, f32, vp, i32, i32, vp]
    if hasattr(lib, "loco_pmp_primal_tap_dh"):
        lib.loco_pmp_primal_tap_dh.argtypes = [vp, vp, f32, f32, vp, i32, vp, vp]
    if hasattr(lib, "loco_pmp_primal_eps"):
        lib.loco_pmp_primal_eps.argtypes = [vp, vp, vp]
    lib.loco_pmp_jvp.argtypes = [vp, vp, i32, vp, vp]
    lib.loco_pmp_vjp.argtypes = [vp, vp, i32, vp, vp]
    if hasattr(lib, "loco_pmp_vjp_context"):      # (absent from a library of an earlier round loaded by LOCO_HIP_LIB for an A/B)
        lib.loco_pmp_vjp_context.argtypes = [vp, vp, i32, vp, vp, vp]
    lib.loco_orthonormalize.argtypes = [vp, vp, i32, i64, vp, vp]
    lib.loco_qr_rows.argtypes = [vp, vp, i32, i64, vp]
    lib.loco_convergence.argtypes = [vp, vp, vp, i64, f32, vp, vp]
    lib.loco_convergence_rows.argtypes = [vp, vp, vp, i32, i64, f32, vp, vp]
    lib.loco_krylov_extend.argtypes = [vp, vp, i32, vp, i32, i64, vp, vp, i32, vp]
    lib.loco_krylov_ritz.argtypes = [vp, vp, i32, i64, i32, vp, vp, f32, vp, vp, i32, vp]
    lib.loco_krylov_left.argtypes = [vp, vp, i32, i64, i32, vp, vp, i32, vp]
    lib.loco_null_project.argtypes = [vp, vp, i32, vp, i32, i64, vp, vp]
    lib.loco_edit_axpy.argtypes = [vp, vp, vp, C.POINTER(f32), i32, i64, vp, vp]
    lib.loco_mask_gather.argtypes = [vp, vp, i32, vp, vp]
    lib.loco_mask_count.argtypes = [vp]
    lib.loco_mask_count.restype = i64
    lib.loco_clock_stamp.argtypes = [vp, vp, vp]
    lib.loco_set_side_stream.argtypes = [vp, vp]
    lib.loco_unet_flops.argtypes = [vp]
    lib.loco_unet_flops.restype = C.c_double
    lib.loco_workspace_bytes.argtypes = [vp]
    lib.loco_workspace_bytes.restype = i64
    lib.loco_timer_start.argtypes = [vp, vp]
    lib.loco_timer_stop.argtypes = [vp, vp, C.POINTER(f32)]
    lib.loco_set_precision.argtypes = [vp, i32]
    lib.loco_get_precision.argtypes = [vp]
    lib.loco_set_streams.argtypes = [vp, i32]
    lib.loco_set_chip_share.argtypes = [vp, i32]
    lib.loco_set_cond.argtypes = [vp, vp, vp]
    lib.loco_set_context.argtypes = [vp, vp, vp]
    lib.loco_masked_axpby.argtypes = [vp, vp, vp, f32, f32, i32, vp, vp]
    lib.loco_latent_sample.argtypes = [vp, vp, vp, f32, i32, vp, vp]
    lib.loco_lincomb.argtypes = [vp, C.POINTER(vp), C.POINTER(f32), i32, vp, i64, vp]
    lib.loco_diffedit_mask.argtypes = [vp, vp, vp, f32, i32, i32, i64, i32, vp, vp, vp]
    lib.loco_cfg_masked_step.argtypes = [vp, vp, vp, vp, vp, f32, f32, f32, vp, i32, i64, vp, vp]
    lib.loco_set_time_cond.argtypes = [vp, vp, vp]
    lib.loco_lcm_step.argtypes = [vp, vp, vp, f32, f32, f32, f32, vp, i64, vp, vp, vp]
    lib.loco_profile_enable.argtypes = [vp, i32]
    lib.loco_profile_report.argtypes = [vp, C.c_char_p, i64]
    if hasattr(lib, "loco_text_create"):
        lib.loco_text_create.argtypes = [C.POINTER(LocoTextCfg), i32, i32, C.POINTER(vp)]
        lib.loco_text_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_text_params_missing.argtypes = [vp]
        lib.loco_text_encode.argtypes = [vp, vp, i32, vp, vp]
        lib.loco_text_last_error.argtypes = [vp]
        lib.loco_text_last_error.restype = C.c_char_p
        lib.loco_text_destroy.argtypes = [vp]
        lib.loco_text_destroy.restype = None
    if hasattr(lib, "loco_t5_create"):
        lib.loco_t5_create.argtypes = [C.POINTER(LocoT5Cfg), i32, i32, C.POINTER(vp)]
        lib.loco_text_encode_masked.argtypes = [vp, vp, C.POINTER(i32), i32, vp, vp]
    if hasattr(lib, "loco_sam_create"):
        lib.loco_sam_create.argtypes = [C.POINTER(LocoSamCfg), i32, C.POINTER(vp)]
        lib.loco_sam_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_sam_params_missing.argtypes = [vp]
        lib.loco_sam_encode.argtypes = [vp, vp, vp, vp]
        lib.loco_sam_profile.argtypes = [vp, i32]
        lib.loco_sam_profile_read.argtypes = [vp, C.POINTER(f32)]
        lib.loco_sam_last_error.argtypes = [vp]
        lib.loco_sam_last_error.restype = C.c_char_p
        lib.loco_sam_destroy.argtypes = [vp]
        lib.loco_sam_destroy.restype = None
    if hasattr(lib, "loco_samdec_create"):
        lib.loco_samdec_create.argtypes = [C.POINTER(LocoSamDecCfg), i32, C.POINTER(vp)]
        lib.loco_samdec_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_samdec_params_missing.argtypes = [vp]
        lib.loco_samdec_set_image.argtypes = [vp, vp, vp]
        lib.loco_samdec_predict.argtypes = [vp, vp, i32, vp, vp, vp]
        lib.loco_samdec_score.argtypes = [vp, vp] + [i32] * 8 + [f32, f32, vp, vp, vp]
        lib.loco_samdec_binarize.argtypes = [vp, vp, i32, vp] + [i32] * 8 + [f32, vp, vp]
        lib.loco_samdec_last_error.argtypes = [vp]
        lib.loco_samdec_last_error.restype = C.c_char_p
        lib.loco_samdec_destroy.argtypes = [vp]
        lib.loco_samdec_destroy.restype = None
    if hasattr(lib, "loco_clipvis_create"):
        lib.loco_clipvis_create.argtypes = [C.POINTER(LocoClipVisCfg), i32, i32, C.POINTER(vp)]
        lib.loco_clipvis_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_clipvis_params_missing.argtypes = [vp]
        lib.loco_clipvis_preprocess.argtypes = [vp, vp, i32, i32, i32, vp, vp]
        lib.loco_clipvis_encode.argtypes = [vp, vp, i32, vp, vp, vp, vp]
        lib.loco_clipvis_last_error.argtypes = [vp]
        lib.loco_clipvis_last_error.restype = C.c_char_p
        lib.loco_clipvis_destroy.argtypes = [vp]
        lib.loco_clipvis_destroy.restype = None
    if hasattr(lib, "loco_clipvis_encode_vjp"):
        lib.loco_clipvis_enable_grad.argtypes = [vp, i32]
        lib.loco_clipvis_grad_bytes.argtypes = [vp]
        lib.loco_clipvis_grad_bytes.restype = i64
        lib.loco_clipvis_encode_vjp.argtypes = [vp, vp, i32, vp, vp]
        lib.loco_clipvis_preprocess_f32.argtypes = [vp, vp, i32, vp, i32, i32, i32, vp, vp]
        lib.loco_clipvis_preprocess_f32_vjp.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp]
    if hasattr(lib, "loco_clipseg_create"):
        lib.loco_clipvis_encode_taps.argtypes = [vp, vp, i32, C.POINTER(i32), i32, vp, vp]
        lib.loco_clipseg_create.argtypes = [C.POINTER(LocoClipSegCfg), i32, C.POINTER(vp)]
        lib.loco_clipseg_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_clipseg_params_missing.argtypes = [vp]
        lib.loco_clipseg_logit_size.argtypes = [vp]
        lib.loco_clipseg_logit_size.restype = i32
        lib.loco_clipseg_decode.argtypes = [vp, vp, i32, vp, C.POINTER(i32), i32, vp, vp]
        lib.loco_clipseg_preprocess.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, C.POINTER(C.c_float), C.POINTER(C.c_float), vp, vp]
        lib.loco_clipseg_masks.argtypes = [vp, vp, i32, i32, i32, C.c_double, vp, vp, vp]
        lib.loco_clipseg_last_error.argtypes = [vp]
        lib.loco_clipseg_last_error.restype = C.c_char_p
        lib.loco_clipseg_destroy.argtypes = [vp]
        lib.loco_clipseg_destroy.restype = None
    if hasattr(lib, "loco_quality_create"):
        lib.loco_quality_create.argtypes = [C.POINTER(LocoQualityCfg), i32, i32, C.POINTER(vp)]
        lib.loco_quality_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_quality_params_missing.argtypes = [vp]
        lib.loco_quality_lpips.argtypes = [vp, vp, vp, i32, i32, i32, i32, vp, vp, vp]
        lib.loco_quality_ssim.argtypes = [vp, vp, vp, i32, i32, i32, i32, C.c_double, vp, vp]
        lib.loco_quality_masked_mse.argtypes = [vp, vp, vp, vp, i32, i64, vp, vp, vp]
        lib.loco_quality_last_error.argtypes = [vp]
        lib.loco_quality_last_error.restype = C.c_char_p
        lib.loco_quality_destroy.argtypes = [vp]
        lib.loco_quality_destroy.restype = None
    if hasattr(lib, "loco_pca_create"):
        lib.loco_pca_create.argtypes = [i32, i64, i64, i32, C.POINTER(vp)]
        lib.loco_pca_reset.argtypes = [vp]
        lib.loco_pca_rows.argtypes = [vp]
        lib.loco_pca_rows.restype = i64
        lib.loco_pca_add_rows.argtypes = [vp, vp, i64, i64, vp]
        lib.loco_pca_fit.argtypes = [vp, i32, i32, vp, i32, vp, vp, vp, vp]
        lib.loco_pca_center.argtypes = [vp, i32, vp, vp, vp]
        lib.loco_pca_gram.argtypes = [vp, vp, i64, i32, vp, vp]
        lib.loco_pca_project.argtypes = [vp, vp, i32, i32, i32, vp, vp]
        lib.loco_pca_set_route.argtypes = [vp, i32]
        lib.loco_pca_routes.argtypes = [vp]
        lib.loco_pca_routes.restype = C.c_char_p
        lib.loco_pca_last_error.argtypes = [vp]
        lib.loco_pca_last_error.restype = C.c_char_p
        lib.loco_pca_destroy.argtypes = [vp]
        lib.loco_pca_destroy.restype = None
    if hasattr(lib, "loco_asyrp_create"):
        lib.loco_asyrp_create.argtypes = [i32, i32, i32, i32, i32, i32, f32, C.POINTER(vp)]
        lib.loco_asyrp_load_param.argtypes = [vp, C.c_char_p, vp, C.POINTER(i64), i32]
        lib.loco_asyrp_params_missing.argtypes = [vp]
        lib.loco_asyrp_read_param.argtypes = [vp, C.c_char_p, vp, i64]
        lib.loco_asyrp_read_grad.argtypes = [vp, C.c_char_p, vp, i64]
        lib.loco_asyrp_forward.argtypes = [vp, vp, vp, i32, f32, vp, i32, vp]
        lib.loco_asyrp_backward.argtypes = [vp, vp, i32, vp, vp]
        lib.loco_asyrp_zero_grad.argtypes = [vp, vp]
        lib.loco_asyrp_adam_step.argtypes = [vp, f32, f32, f32, f32, i32, vp]
        lib.loco_asyrp_reset_moments.argtypes = [vp, vp]
        lib.loco_asyrp_last_error.argtypes = [vp]
        lib.loco_asyrp_last_error.restype = C.c_char_p
        lib.loco_asyrp_destroy.argtypes = [vp]
        lib.loco_asyrp_destroy.restype = None
    if hasattr(lib, "loco_bench_conv"):          # diag build only
        lib.loco_bench_conv.argtypes = [vp, i32, i32, i32, i32, i32, i32, i32, i32, i32, C.POINTER(f32), vp]
        lib.loco_debug_tensor.argtypes = [vp, C.c_char_p, vp, i64, vp]
        lib.loco_debug_tensor.restype = i64
    if hasattr(lib, "loco_debug_conv"):
        lib.loco_debug_conv.argtypes = [vp, C.POINTER(LocoConvDesc), C.c_char_p, i64, vp]
    if hasattr(lib, "loco_debug_attn"):
        lib.loco_debug_attn.argtypes = [vp, C.POINTER(LocoAttnDesc), C.c_char_p, i64, vp]
    if hasattr(lib, "loco_debug_norm"):
        lib.loco_debug_norm.argtypes = [vp, C.POINTER(LocoNormDesc), vp]
    if hasattr(lib, "loco_debug_pointwise"):
        lib.loco_debug_pointwise.argtypes = [vp, C.POINTER(LocoPointwiseDesc), vp]
    if hasattr(lib, "loco_debug_gemm"):
        lib.loco_debug_gemm.argtypes = [vp, C.POINTER(LocoGemmDesc), C.c_char_p, i64, vp]
    if hasattr(lib, "loco_debug_enc_attn"):
        lib.loco_debug_enc_attn.argtypes = [C.POINTER(LocoEncAttnDesc), C.c_char_p, i64, C.c_char_p, i64, vp]
    _lib = lib
    return lib


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _chk_dev(t: torch.Tensor, dtype=torch.float32):
    if not t.is_cuda:
        raise ValueError("loco_hip operates on device tensors only")
    if t.dtype != dtype:
        raise ValueError(f"expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError("tensor must be contiguous")


def debug_enc_attn(**desc):
    """One launch of one attention kernel of the encoders on caller-supplied tensors through the product's launcher
    (loco_debug_enc_attn, include/loco_hip_diag.h; no engine).  `desc`: the fields of loco_enc_attn_desc, `op` a number or a name of
    LocoEncAttnDesc.OPS; every tensor a contiguous device tensor, float32 but for `lens` (int32).  Returns the route: one dict
    per launch.  A refusal or a HIP error raises RuntimeError with the entry point's message."""
    lib = load_library()
    if not hasattr(lib, "loco_debug_enc_attn"):
        raise RuntimeError("loco_debug_enc_attn is a diagnostic of include/loco_hip_diag.h: build `make -C loco-edit_amd/csrc diag` "
                           "and set LOCO_HIP_LIB=<repo>/loco-edit_amd/libloco_hip_diag.so")
    d = LocoEncAttnDesc()
    d.struct_size = C.sizeof(LocoEncAttnDesc)
    keep = []
    for k, v in desc.items():
        if k == "op":
            d.op = LocoEncAttnDesc.OPS[v] if isinstance(v, str) else int(v)
        elif k not in LocoEncAttnDesc._PTRS:
            if not hasattr(d, k) or k == "struct_size":
                raise TypeError(f"debug_enc_attn: no descriptor field {k!r}")
            setattr(d, k, v)
        elif v is not None:
            _chk_dev(v, torch.int32 if k == "lens" else torch.float32)
            keep.append(v)
            setattr(d, k, v.data_ptr())
    buf, err = C.create_string_buffer(256), C.create_string_buffer(512)
    rc = lib.loco_debug_enc_attn(C.byref(d), buf, len(buf), err, len(err), _stream())
    if rc != 0:
        raise RuntimeError(f"loco_debug_enc_attn failed ({rc}): {err.value.decode()}")
    route = []
    for line in buf.value.decode().splitlines():
        rec = dict(f.split("=", 1) for f in line.split(" "))
        route.append({k: (v if k == "kernel" else int(v)) for k, v in rec.items()})
    return route


def c_cfg(cfg: UNetConfig, max_batch: int) -> LocoCfg:
    """The loco_unet_cfg that loco_create receives for `cfg` (also what the host-side program check is fed)."""
    c = LocoCfg()
    c.struct_size = C.sizeof(LocoCfg)
    c.resolution, c.in_channels, c.out_ch, c.ch = cfg.resolution, cfg.in_channels, cfg.out_ch, cfg.ch
    c.num_levels = len(cfg.ch_mult)
    for i, m in enumerate(cfg.ch_mult):
        c.ch_mult[i] = m
    c.num_res_blocks = cfg.num_res_blocks
    c.num_attn_res = len(cfg.attn_resolutions)
    for i, r in enumerate(cfg.attn_resolutions):
        c.attn_resolutions[i] = r
    c.gn_groups, c.gn_eps, c.max_batch = cfg.gn_groups, cfg.gn_eps, int(max_batch)
    c.arch = {"ddpm": 0, "adm": 1, "dec": 2, "enc": 3}[cfg.arch]
    c.num_head_channels, c.learn_sigma = cfg.num_head_channels, int(cfg.learn_sigma)
    c.context_dim, c.context_len = cfg.context_dim, cfg.context_len
    c.scale_shift_norm, c.resblock_updown = int(cfg.scale_shift_norm), int(cfg.resblock_updown)
    c.num_heads, c.transformer_depth = cfg.num_heads, cfg.transformer_depth
    c.act, c.res_scale, c.added_kv = {"silu": 0, "gelu": 1}[cfg.act], float(cfg.res_scale), int(cfg.added_kv)
    c.time_cond_proj_dim = int(cfg.time_cond_proj_dim)
    return c


class LocoEngine:
    """One engine (= loco_ctx) per process and GPU."""

    def __init__(self, cfg: UNetConfig, max_batch: int = 8, device: Optional[torch.device] = None):
        self.lib = load_library()
        if not torch.cuda.is_available() or self.lib.loco_device_count() < 1:
            raise RuntimeError("loco_hip: no HIP device visible; the hot path has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:0")
        torch.cuda.set_device(self.device)
        self.cfg = cfg
        self.max_batch = int(max_batch)
        c = c_cfg(cfg, self.max_batch)
        self._ctx = C.c_void_p()
        rc = self.lib.loco_create(C.byref(c), C.byref(self._ctx))
        if rc != 0:
            msg = self.lib.loco_last_error(self._ctx).decode() if self._ctx else "?"
            raise RuntimeError(f"loco_create failed ({rc}): {msg}")
        self.n = cfg.n              # elements of the network input (image / latent)
        self.n_out = cfg.n_out      # elements of its output (= n for the denoisers; the decoded image for arch "dec")
        self._tap = None            # operator of the cached primal (pmp_primal(tap=...)): the row widths of pmp_jvp / pmp_vjp

    def fork(self, max_batch: Optional[int] = None) -> "LocoEngine":
        """A second engine context on THIS engine's parameters (loco_fork): shares the device copies of the weights in every
        layout, owns its arenas / statistics / scratch / per-prompt constants.  What the reference does with one U-Net object
        for all classifier-free-guidance branches (edit.py:1319-1322, :655-667); bit-identical to an independent engine."""
        child = object.__new__(LocoEngine)
        child.lib, child.cfg, child.device = self.lib, self.cfg, self.device
        child.max_batch = int(max_batch or self.max_batch)
        child.n, child.n_out = self.n, self.n_out
        child._tap = None
        for k, v in self.__dict__.items():      # host-side settings (stream mode ...) that __init__ derives from the arguments
            if k not in child.__dict__ and k != "_ctx":
                child.__dict__[k] = v
        child._ctx = C.c_void_p()
        torch.cuda.set_device(self.device)
        rc = self.lib.loco_fork(self._ctx, child.max_batch, C.byref(child._ctx))
        if rc != 0:
            msg = self.lib.loco_last_error(child._ctx).decode() if child._ctx else self.lib.loco_last_error(self._ctx).decode()
            raise RuntimeError(f"loco_fork failed ({rc}): {msg}")
        return child

    def __del__(self):
        try:
            if getattr(self, "_ctx", None):
                self.lib.loco_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self.lib.loco_last_error(self._ctx).decode()}")

    # ---- parameters (model.load_state_dict, reference utils.py:102-105)
    def load_state_dict(self, sd: Dict[str, "np.ndarray | torch.Tensor"]):
        for name, v in sd.items():
            if self.cfg.encoder_dim > 0 and name.startswith(("encoder_proj.", "encoder_pooling.")):
                continue        # the image-independent text conditioning of the IF U-Net lives on the host (tloco.IFTextConditioner)
            a = v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)
            a = np.ascontiguousarray(a, dtype=np.float32)
            shape = (C.c_int64 * a.ndim)(*a.shape)
            rc = self.lib.loco_load_param(self._ctx, name.encode(), a.ctypes.data_as(C.c_void_p), shape, a.ndim, 0)
            self._check(rc, f"loco_load_param({name})")
        miss = self.lib.loco_params_missing(self._ctx)
        if miss != 0:
            raise RuntimeError(f"{miss} parameters missing: {self.lib.loco_last_error(self._ctx).decode()}")

    # ---- denoiser
    def _chk_input(self, x: torch.Tensor):
        """[B, in_channels, R, R] of this network (the C ABI takes a pointer and a count: a wrong shape would be read
        as garbage, not refused; the batch bound is checked there)."""
        want = (self.cfg.in_channels, self.cfg.resolution, self.cfg.resolution)
        if x.dim() != 4 or tuple(x.shape[1:]) != want:
            raise ValueError(f"input must be [B, {want[0]}, {want[1]}, {want[2]}], got {tuple(x.shape)}")

    # ---- h-space tap (loco_hip.h "h-space tap"): the U-Net bottleneck of a denoiser
    @property
    def h_shape(self):
        """(C, H, W) of the bottleneck tensor h = get_h(x, t, 'mid', 0); the latent decoder / encoder have none (RuntimeError)."""
        d = [C.c_int32(), C.c_int32(), C.c_int32()]
        self._check(self.lib.loco_h_dims(self._ctx, *[C.byref(v) for v in d]), "loco_h_dims")
        return tuple(int(v.value) for v in d)

    @property
    def n_h(self) -> int:
        c, h, w = self.h_shape
        return c * h * w

    def get_h(self, x: torch.Tensor, t: float) -> torch.Tensor:
        """h [B, C, H, W] of ``x`` [B, in_channels, R, R]: the ops up to the tap only."""
        _chk_dev(x)
        self._chk_input(x)
        h = torch.empty(x.shape[0], *self.h_shape, device=x.device, dtype=torch.float32)
        self._check(self.lib.loco_unet_get_h(self._ctx, _ptr(x), float(t), x.shape[0], _ptr(h), _stream()), "loco_unet_get_h")
        return h

    def _rows(self, side: str) -> int:
        """Row width of the operator of the cached primal: ``in`` of pmp_jvp's V and pmp_vjp's A, ``out`` of the other two."""
        if self._tap == "enc":
            return self.n if side == "in" else self.n_h
        if self._tap == "dec":
            return self.n_h if side == "in" else self.n_out
        return self.n if side == "in" else self.n_out

    def unet_forward(self, x: torch.Tensor, t: float, out: Optional[torch.Tensor] = None,
                     dh: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``dh`` [B, n_h] (any shape with B * n_h elements): added to the bottleneck tensor of each sample, the reference's
        ``forward(x, t, u=dh, op='mid', block_idx=0)``."""
        _chk_dev(x)
        self._chk_input(x)
        if dh is not None:
            _chk_dev(dh)
            if dh.numel() != x.shape[0] * self.n_h:
                raise ValueError(f"dh must hold {x.shape[0]} x {self.n_h} elements, got {tuple(dh.shape)}")
        if out is not None:
            _chk_dev(out)
            if out.numel() != x.shape[0] * self.n_out:
                raise ValueError(f"out must hold {x.shape[0]} x {self.n_out} elements, got {tuple(out.shape)}")
            eps = out
        elif self.cfg.arch in ("dec", "enc"):      # decoder / encoder: [B, C_in, R, R] -> [B, out_ch, R_out, R_out]
            eps = torch.empty(x.shape[0], self.cfg.out_ch, self.cfg.out_resolution, self.cfg.out_resolution,
                              device=x.device, dtype=torch.float32)
        else:
            eps = torch.empty_like(x)
        if dh is not None:
            self._check(self.lib.loco_unet_forward_dh(self._ctx, _ptr(x), float(t), x.shape[0], _ptr(dh), _ptr(eps), _stream()),
                        "loco_unet_forward_dh")
            return eps
        self._check(self.lib.loco_unet_forward(self._ctx, _ptr(x), float(t), x.shape[0], _ptr(eps), _stream()),
                    "loco_unet_forward")
        return eps

    def ddim_step(self, x, t, at, at_next, eta=0.0, noise=None, out=None):
        _chk_dev(x)
        self._chk_input(x)
        if noise is not None:
            _chk_dev(noise)
        out = torch.empty_like(x) if out is None else out
        self._check(self.lib.loco_ddim_step(self._ctx, _ptr(x), float(t), float(at), float(at_next), float(eta),
                                            _ptr(noise), x.shape[0], _ptr(out), _stream()), "loco_ddim_step")
        return out

    def sched_step(self, x, et, at, at_next, eta=0.0, noise=None, want_x0=False):
        _chk_dev(x)
        _chk_dev(et)
        out = torch.empty_like(x)
        x0 = torch.empty_like(x) if want_x0 else None
        self._check(self.lib.loco_sched_step(self._ctx, _ptr(x), _ptr(et), float(at), float(at_next), float(eta),
                                             _ptr(noise), x.numel(), _ptr(out), _ptr(x0), _stream()),
                    "loco_sched_step")
        return out, x0

    def sched_step_asym(self, x, et_edit, et_src, at, at_next, want_x0=False):
        """The eta = 0 step with the x0 estimate from ``et_edit`` and the direction term from ``et_src`` (Asyrp's asymmetric step):
        ``(x_next, x0 or None)``."""
        for t_ in (x, et_edit, et_src):
            _chk_dev(t_)
        if et_edit.numel() != x.numel() or et_src.numel() != x.numel():
            raise ValueError("sched_step_asym: x, et_edit and et_src must have the same number of elements")
        out = torch.empty_like(x)
        x0 = torch.empty_like(x) if want_x0 else None
        self._check(self.lib.loco_sched_step_asym(self._ctx, _ptr(x), _ptr(et_edit), _ptr(et_src), float(at), float(at_next), x.numel(),
                                                  _ptr(out), _ptr(x0), _stream()), "loco_sched_step_asym")
        return out, x0

    # ---- PMP-Jacobian operator
    def pmp_primal(self, x, t, at, mask: Optional[torch.Tensor] = None, use_et: bool = False, tap: Optional[str] = None,
                   dh: Optional[torch.Tensor] = None):
        """``tap``: None (J = d x0_hat[mask] / d x_t), ``"enc"`` (J = d h / d x_t, no mask) or ``"dec"`` (J = mask . c . d eps / d h);
        pmp_jvp / pmp_vjp take and return rows of that operator's widths until the next pmp_primal.  ``dh`` (``tap="dec"`` only):
        the decoder tap is linearised at the shifted bottleneck ``h(x_t) + dh`` and ``pmp_primal_eps`` is the network output there."""
        if tap not in TAPS:
            raise ValueError(f"tap must be None, 'enc' or 'dec', got {tap!r}")
        if dh is not None:
            if tap != "dec":
                raise ValueError("dh shifts the bottleneck of the decoder tap: it needs tap='dec'")
            _chk_dev(dh)
            if dh.numel() != self.n_h:
                raise ValueError(f"dh must have the {self.n_h} elements of h, got {tuple(dh.shape)}")
        _chk_dev(x)
        if x.numel() != self.n:
            raise ValueError(f"the linearisation point is one sample of {self.n} elements, got {tuple(x.shape)}")
        m8 = None
        if mask is not None:
            m8 = mask.to(device=x.device, dtype=torch.uint8).contiguous().view(-1)
            if m8.numel() != self.n_out:
                raise ValueError("mask must have C*H*W elements (of the network output)")
        self._mask_keepalive = m8
        if dh is not None:
            self._check(self.lib.loco_pmp_primal_tap_dh(self._ctx, _ptr(x), float(t), float(at), _ptr(m8), int(use_et), _ptr(dh), _stream()),
                        "loco_pmp_primal_tap_dh")
            self._tap = tap
            return
        if tap is not None:
            self._check(self.lib.loco_pmp_primal_tap(self._ctx, _ptr(x), float(t), float(at), _ptr(m8), int(use_et), TAPS[tap],
                                                     _stream()), "loco_pmp_primal_tap")
            self._tap = tap
            return
        self._tap = None
        self._check(self.lib.loco_pmp_primal(self._ctx, _ptr(x), float(t), float(at), _ptr(m8), int(use_et),
                                             _stream()), "loco_pmp_primal")

    def pmp_primal_eps(self) -> torch.Tensor:
        """The network output [n_out] the last ``pmp_primal`` evaluated at its linearisation point (no second evaluation)."""
        eps = torch.empty(self.n_out, device=self.device, dtype=torch.float32)
        self._check(self.lib.loco_pmp_primal_eps(self._ctx, _ptr(eps), _stream()), "loco_pmp_primal_eps")
        return eps

    def pmp_set_second_mask(self, mask2: Optional[torch.Tensor], from_row: int = 0):
        """Rows >= from_row of later pmp_jvp / pmp_vjp calls use ``mask2`` (None: off)."""
        m8 = None
        if mask2 is not None:
            m8 = mask2.to(device=self.device, dtype=torch.uint8).contiguous().view(-1)
            if m8.numel() != self.n_out:
                raise ValueError("mask must have C*H*W elements (of the network output)")
        self._mask2_keepalive = m8                   # the copy is enqueued on the stream: keep the source alive, no host sync
        self._check(self.lib.loco_pmp_set_second_mask(self._ctx, _ptr(m8), int(from_row), _stream()), "loco_pmp_set_second_mask")

    def pmp_jvp(self, V: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """``out``: a [k, n_out] tensor to write into (callers that launch on a side stream allocate it on their own
        stream first, so no allocation happens under the side stream)."""
        _chk_dev(V)
        k = V.shape[0]
        n_out = self._rows("out")
        if self._tap is not None and (V.dim() != 2 or V.shape[1] != self._rows("in")):
            raise ValueError(f"V must be [k, {self._rows('in')}] for the '{self._tap}' tap, got {tuple(V.shape)}")
        U = torch.empty(k, n_out, device=V.device, dtype=torch.float32) if out is None else out
        if out is not None:
            _chk_dev(out)
            if tuple(out.shape) != (k, n_out):
                raise ValueError(f"out must be {(k, n_out)}, got {tuple(out.shape)}")
        self._check(self.lib.loco_pmp_jvp(self._ctx, _ptr(V), k, _ptr(U), _stream()), "loco_pmp_jvp")
        return U

    def pmp_vjp(self, U: torch.Tensor, out: Optional[torch.Tensor] = None, context_grad: bool = False):
        """``context_grad``: also return G [k, context_len, context_dim], the gradient of the same rows with respect to the
        states of the last ``set_context`` -- ``(A, G)``; A is what the call without the flag returns, to the bit.  A row of G
        does not depend on k or its position: the rows come from single-probe passes (k = 1: one pass for A and G)."""
        _chk_dev(U)
        k = U.shape[0]
        n_in = self._rows("in")
        if self._tap is not None and (U.dim() != 2 or U.shape[1] != self._rows("out")):
            raise ValueError(f"U must be [k, {self._rows('out')}] for the '{self._tap}' tap, got {tuple(U.shape)}")
        A = torch.empty(k, n_in, device=U.device, dtype=torch.float32) if out is None else out
        if out is not None:
            _chk_dev(out)
            if tuple(out.shape) != (k, n_in):
                raise ValueError(f"out must be {(k, n_in)}, got {tuple(out.shape)}")
        if context_grad:
            G = torch.empty(k, self.cfg.context_len, self.cfg.context_dim, device=U.device, dtype=torch.float32)
            self._check(self.lib.loco_pmp_vjp_context(self._ctx, _ptr(U), k, _ptr(A), _ptr(G), _stream()), "loco_pmp_vjp_context")
            return A, G
        self._check(self.lib.loco_pmp_vjp(self._ctx, _ptr(U), k, _ptr(A), _stream()), "loco_pmp_vjp")
        return A

    # ---- solver algebra
    def orthonormalize_(self, A: torch.Tensor) -> torch.Tensor:
        _chk_dev(A)
        k, n = A.shape
        s = torch.empty(k, device=A.device, dtype=torch.float32)
        self._check(self.lib.loco_orthonormalize(self._ctx, _ptr(A), k, n, _ptr(s), _stream()), "loco_orthonormalize")
        return s

    def qr_rows_(self, A: torch.Tensor):
        _chk_dev(A)
        k, n = A.shape
        self._check(self.lib.loco_qr_rows(self._ctx, _ptr(A), k, n, _stream()), "loco_qr_rows")
        return A

    def convergence(self, Vprev, V, atol) -> torch.Tensor:
        _chk_dev(Vprev)
        _chk_dev(V)
        out = torch.empty(2, device=V.device, dtype=torch.float32)
        self._check(self.lib.loco_convergence(self._ctx, _ptr(Vprev), _ptr(V), V.numel(), float(atol), _ptr(out),
                                              _stream()), "loco_convergence")
        return out

    def convergence_rows(self, Vprev, V, atol) -> torch.Tensor:
        """[distance, allclose flag] of the rows of V against +-the rows of Vprev (loco_convergence_rows)."""
        _chk_dev(Vprev)
        _chk_dev(V)
        k, n = V.shape
        out = torch.empty(2, device=V.device, dtype=torch.float32)
        self._check(self.lib.loco_convergence_rows(self._ctx, _ptr(Vprev), _ptr(V), k, n, float(atol), _ptr(out),
                                                   _stream()), "loco_convergence_rows")
        return out

    # ---- block Krylov solver (solver.krylov_iteration drives these; include/loco_hip.h states the contract)
    def krylov_extend(self, A, Q, m: int, nxt, stat, slot: int = 0):
        """One step's n-wide algebra on A [k, n] = J^T J Q[m-k:m] against the first ``m`` rows of Q; ``nxt`` [k, n] (or None)
        receives the next block; stat[3] is set."""
        for t in (A, Q, stat) + ((nxt,) if nxt is not None else ()):
            _chk_dev(t)
        k, n = A.shape
        if Q.shape[1] != n or Q.shape[0] < m or stat.numel() < 4 or (nxt is not None and tuple(nxt.shape) != (k, n)):
            raise ValueError("krylov_extend: Q must hold m rows of A's width, nxt must have A's shape, stat 4 floats")
        self._check(self.lib.loco_krylov_extend(self._ctx, _ptr(A), k, _ptr(Q), int(m), n, _ptr(nxt), _ptr(stat), int(slot),
                                                _stream()), "loco_krylov_extend")

    def krylov_ritz(self, Q, m: int, Y, Yprev, atol, resid, stat, slot: int = 0):
        """Y [k, n] = top-k Ritz vectors over Q[:m]; resid [k]; stat[0..2] (loco_krylov_ritz)."""
        for t in (Q, Y, resid, stat) + ((Yprev,) if Yprev is not None else ()):
            _chk_dev(t)
        k, n = Y.shape
        if Q.shape[1] != n or Q.shape[0] < m or resid.numel() < k or stat.numel() < 4 or \
                (Yprev is not None and tuple(Yprev.shape) != (k, n)):
            raise ValueError("krylov_ritz: Q must hold m rows of Y's width, Yprev must have Y's shape, resid k and stat 4 floats")
        self._check(self.lib.loco_krylov_ritz(self._ctx, _ptr(Q), int(m), n, k, _ptr(Y), _ptr(Yprev), float(atol), _ptr(resid),
                                              _ptr(stat), int(slot), _stream()), "loco_krylov_ritz")

    def krylov_left(self, Ustore, m: int, UY, s, slot: int = 0):
        """UY [k, n_out] = the Ritz combination (and signs) of Ustore[:m]; s [k] = ||UY_i||^2 (loco_krylov_left)."""
        for t in (Ustore, UY, s):
            _chk_dev(t)
        k, n_out = UY.shape
        if Ustore.shape[1] != n_out or Ustore.shape[0] < m or s.numel() < k:
            raise ValueError("krylov_left: Ustore must hold m rows of UY's width, s k floats")
        self._check(self.lib.loco_krylov_left(self._ctx, _ptr(Ustore), int(m), n_out, k, _ptr(UY), _ptr(s), int(slot),
                                              _stream()), "loco_krylov_left")

    def null_project(self, Vm, Vn=None) -> torch.Tensor:
        _chk_dev(Vm)
        k, n = Vm.shape
        k0 = 0
        if Vn is not None:
            _chk_dev(Vn)
            k0 = Vn.shape[0]
        out = torch.empty_like(Vm)
        self._check(self.lib.loco_null_project(self._ctx, _ptr(Vm), k, _ptr(Vn), k0, n, _ptr(out), _stream()),
                    "loco_null_project")
        return out

    def edit_axpy(self, x, v, alphas) -> torch.Tensor:
        _chk_dev(x)
        _chk_dev(v)
        B = len(alphas)
        n = x.numel()
        out = torch.empty((B,) + tuple(x.shape[1:]), device=x.device, dtype=torch.float32)
        arr = (C.c_float * B)(*[float(a) for a in alphas])
        self._check(self.lib.loco_edit_axpy(self._ctx, _ptr(x), _ptr(v), arr, B, n, _ptr(out), _stream()),
                    "loco_edit_axpy")
        torch.cuda.current_stream().synchronize()   # `arr` is host memory read asynchronously
        return out

    def mask_gather(self, U) -> torch.Tensor:
        _chk_dev(U)
        k = U.shape[0]
        L = int(self.lib.loco_mask_count(self._ctx))
        out = torch.empty(k, L, device=U.device, dtype=torch.float32)
        self._check(self.lib.loco_mask_gather(self._ctx, _ptr(U), k, _ptr(out), _stream()), "loco_mask_gather")
        return out

    def mask_count(self) -> int:
        """L = number of selected elements of the mask given to the last ``pmp_primal`` (n when unmasked)."""
        return int(self.lib.loco_mask_count(self._ctx))

    # ---- conditioning / CFG combination (T-LOCO)
    def set_cond(self, emb_add: Optional[torch.Tensor]):
        """Conditioning embedding [4*ch] added to the time embedding before its SiLU (None clears it)."""
        if emb_add is not None:
            _chk_dev(emb_add)
            if emb_add.numel() != 4 * self.cfg.ch:
                raise ValueError("conditioning embedding must have 4*ch elements")
        self._check(self.lib.loco_set_cond(self._ctx, _ptr(emb_add), _stream()), "loco_set_cond")

    def set_time_cond(self, w_emb: Optional[torch.Tensor]):
        """Guidance-scale embedding [time_cond_proj_dim] of a latent-consistency denoiser (``timestep_cond`` of
        ``self.unet(...)``, edit.py:126-132): cond_proj(w_emb) is added to the sinusoid of every later time embedding of THIS
        context (forks keep their own).  None clears it."""
        if w_emb is not None:
            _chk_dev(w_emb)
            if self.cfg.time_cond_proj_dim > 0 and w_emb.numel() != self.cfg.time_cond_proj_dim:      # (0: the engine refuses)
                raise ValueError(f"guidance-scale embedding must have time_cond_proj_dim = {self.cfg.time_cond_proj_dim} "
                                 f"elements, got {tuple(w_emb.shape)}")
        self._check(self.lib.loco_set_time_cond(self._ctx, _ptr(w_emb), _stream()), "loco_set_time_cond")
        if w_emb is not None:
            torch.cuda.current_stream().synchronize()     # `w_emb` may be a temporary

    def set_context(self, tokens: torch.Tensor):
        """Encoder states of the prompt [context_len, context_dim] for the cross-attention stages (the
        ``encoder_hidden_states`` of ``self.unet(...)``, edit.py:664-667); projected to keys / values once."""
        _chk_dev(tokens)
        if tuple(tokens.shape) != (self.cfg.context_len, self.cfg.context_dim):
            raise ValueError(f"context must be [{self.cfg.context_len}, {self.cfg.context_dim}], got {tuple(tokens.shape)}")
        self._check(self.lib.loco_set_context(self._ctx, _ptr(tokens), _stream()), "loco_set_context")
        torch.cuda.current_stream().synchronize()     # `tokens` may be a temporary

    def masked_axpby(self, V: torch.Tensor, E: torch.Tensor, cv: float, ce: float) -> torch.Tensor:
        """mask * (cv*V + ce*E) with the mask of the last pmp_primal; V, E: [k, n]."""
        _chk_dev(V)
        _chk_dev(E)
        out = torch.empty_like(V)
        self._check(self.lib.loco_masked_axpby(self._ctx, _ptr(V), _ptr(E), float(cv), float(ce), V.shape[0], _ptr(out),
                                               _stream()), "loco_masked_axpby")
        return out

    def latent_sample(self, moments: torch.Tensor, noise: Optional[torch.Tensor], scale: float) -> torch.Tensor:
        """Encoder contexts: scale * (mean + std * noise) from the moments [B, 2Z, h, w] (noise None: the mean)."""
        _chk_dev(moments)
        B, C2, h, w = moments.shape
        if C2 * h * w != self.n_out:
            raise ValueError(f"moments must be [B, {self.cfg.out_ch}, ...] of this encoder, got {tuple(moments.shape)}")
        if noise is not None:
            _chk_dev(noise)
            if tuple(noise.shape) != (B, C2 // 2, h, w):
                raise ValueError(f"noise must be {(B, C2 // 2, h, w)}, got {tuple(noise.shape)}")
        z = torch.empty(B, C2 // 2, h, w, device=moments.device, dtype=torch.float32)
        self._check(self.lib.loco_latent_sample(self._ctx, _ptr(moments), _ptr(noise) if noise is not None else None,
                                                float(scale), B, _ptr(z), _stream()), "loco_latent_sample")
        return z

    def lincomb(self, terms, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """sum_i coef_i * tensor_i for [(coef, tensor), ...] (<= 4 terms, same shape, fp32, contiguous)."""
        for _, t in terms:
            _chk_dev(t)
        out = torch.empty_like(terms[0][1]) if out is None else out
        n = len(terms)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() for _, t in terms])
        coef = (C.c_float * n)(*[float(c) for c, _ in terms])
        self._check(self.lib.loco_lincomb(self._ctx, ptrs, coef, n, _ptr(out), out.numel(), _stream()), "loco_lincomb")
        return out

    # ---- DiffEdit (edit.py:1395-1407, :1486-1563)
    def diffedit_mask(self, eps_a: torch.Tensor, eps_b: torch.Tensor, scale: float, rule: str = "reference",
                      want_map: bool = False):
        """uint8 mask [HW] from the two guided noise predictions [B, C, H, W] (or [B, C, HW]): the map
        m = mean_c mean_b scale (eps_a - eps_b), thresholded by `rule` ("reference": |m - min/(max-min)| > 0.5, edit.py:1402
        as written; "intended": (m - min)/(max - min) > 0.5).  A constant map raises ValueError (the reference divides by
        zero there).  want_map: returns (mask, m)."""
        _chk_dev(eps_a)
        _chk_dev(eps_b)
        if eps_a.shape != eps_b.shape or eps_a.dim() < 3:
            raise ValueError(f"two [B, C, ...] tensors of one shape, got {tuple(eps_a.shape)} and {tuple(eps_b.shape)}")
        if rule not in DIFFEDIT_RULES:
            raise ValueError(f"rule must be one of {sorted(DIFFEDIT_RULES)}, got {rule!r}")
        B, Cc = eps_a.shape[0], eps_a.shape[1]
        HW = eps_a.numel() // (B * Cc)
        mask = torch.empty(HW, device=eps_a.device, dtype=torch.uint8)
        m = torch.empty(HW, device=eps_a.device, dtype=torch.float32) if want_map else None
        rc = self.lib.loco_diffedit_mask(self._ctx, _ptr(eps_a), _ptr(eps_b), float(scale), B, Cc, HW, DIFFEDIT_RULES[rule],
                                         _ptr(m), _ptr(mask), _stream())
        if rc in (-4, -5):
            raise ValueError(self.lib.loco_last_error(self._ctx).decode())
        self._check(rc, "loco_diffedit_mask")
        return (mask, m) if want_map else mask

    def cfg_masked_step(self, x, ef, ee, en, g: float, at: float, at_next: float, mask: torch.Tensor,
                        out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One masked-sampler step: mask ? ddim(x, en + g (ee - en)) : ddim(x, en + g (ef - en)), eta = 0.  x, ef, ee, en:
        [B, ...] of one shape; mask: uint8 with the elements of one frame, broadcast over B; out may be x."""
        for t_ in (x, ef, ee, en):
            _chk_dev(t_)
            if t_.shape != x.shape:
                raise ValueError(f"x and the three noise predictions must share a shape, got {tuple(t_.shape)} vs {tuple(x.shape)}")
        _chk_dev(mask, torch.uint8)
        B = x.shape[0]
        n = x.numel() // B
        if mask.numel() != n:
            raise ValueError(f"mask must hold the {n} elements of one frame, got {tuple(mask.shape)}")
        if out is None:
            out = torch.empty_like(x)
        else:
            _chk_dev(out)
            if out.shape != x.shape:
                raise ValueError(f"out must be {tuple(x.shape)}, got {tuple(out.shape)}")
        self._check(self.lib.loco_cfg_masked_step(self._ctx, _ptr(x), _ptr(ef), _ptr(ee), _ptr(en), float(g), float(at),
                                                  float(at_next), _ptr(mask), B, n, _ptr(out), _stream()),
                    "loco_cfg_masked_step")
        return out

    # ---- latent-consistency scheduler (edit.py:135, 194, 235)
    def lcm_step(self, x, eps, at: float, at_prev: float, c_skip: float, c_out: float, noise: Optional[torch.Tensor] = None,
                 want_prev: bool = True, want_denoised: bool = True, out: Optional[torch.Tensor] = None):
        """One LCMScheduler step after the denoiser call, one launch: denoised = c_out (x - sqrt(1-at) eps) / sqrt(at) +
        c_skip x, prev = sqrt(at_prev) denoised + sqrt(1-at_prev) noise (noise None: prev = denoised).  -> (prev, denoised),
        None for the one not asked for; ``out``: the tensor prev is written into (may be x)."""
        _chk_dev(x)
        _chk_dev(eps)
        if eps.shape != x.shape:
            raise ValueError(f"x and eps must share a shape, got {tuple(x.shape)} and {tuple(eps.shape)}")
        if noise is not None:
            _chk_dev(noise)
            if noise.shape != x.shape:
                raise ValueError(f"noise must be {tuple(x.shape)}, got {tuple(noise.shape)}")
        if not (want_prev or want_denoised):
            raise ValueError("lcm_step: ask for prev, denoised or both")
        prev = None
        if want_prev:
            prev = torch.empty_like(x) if out is None else out
            if out is not None:
                _chk_dev(out)
                if out.shape != x.shape:
                    raise ValueError(f"out must be {tuple(x.shape)}, got {tuple(out.shape)}")
        den = torch.empty_like(x) if want_denoised else None
        self._check(self.lib.loco_lcm_step(self._ctx, _ptr(x), _ptr(eps), float(at), float(at_prev), float(c_skip), float(c_out),
                                           _ptr(noise), x.numel(), _ptr(prev), _ptr(den), _stream()), "loco_lcm_step")
        return prev, den

    # ---- introspection
    def version(self) -> str:
        return self.lib.loco_version().decode()

    def clock_stamp(self) -> torch.Tensor:
        """Enqueue a {s_memtime, s_memrealtime} stamp on the current stream; returns the device int64[2] it lands in."""
        out = torch.zeros(2, device=self.device, dtype=torch.int64)
        self._check(self.lib.loco_clock_stamp(self._ctx, _ptr(out), _stream()), "loco_clock_stamp")
        return out

    @staticmethod
    def sclk_mhz(stamp0: torch.Tensor, stamp1: torch.Tensor) -> float:
        """Average shader clock between two stamps (after a synchronize)."""
        d = (stamp1 - stamp0).tolist()
        return 100.0 * d[0] / max(d[1], 1)

    def unet_flops(self) -> float:
        return float(self.lib.loco_unet_flops(self._ctx))

    def workspace_bytes(self) -> int:
        return int(self.lib.loco_workspace_bytes(self._ctx))

    def timer_start(self):
        self._check(self.lib.loco_timer_start(self._ctx, _stream()), "loco_timer_start")

    def timer_stop(self) -> float:
        ms = C.c_float()
        self._check(self.lib.loco_timer_stop(self._ctx, _stream(), C.byref(ms)), "loco_timer_stop")
        return float(ms.value)

    PRECISIONS = {"f32": 0, "bf16x3": 1, "f16": 2}

    def set_precision(self, mode: str):
        """'f32' = exact fp32 MFMA (parity anchor); 'bf16x3' = split-bf16 MFMA (fp32-faithful to ~2^-16);
        'f16' = one f16 MFMA per product (11-bit operands, fp32 accumulate)."""
        self._check(self.lib.loco_set_precision(self._ctx, self.PRECISIONS[mode]), "loco_set_precision")

    def set_streams(self, n: int):
        """Probe groups of a tangent / cotangent pass on 1 (default) or 2 HIP streams (identical results)."""
        self._check(self.lib.loco_set_streams(self._ctx, int(n)), "loco_set_streams")

    def set_chip_share(self, n: int):
        """n engine contexts run their passes side by side on different streams (T-LOCO's guidance branches): split-K then aims
        at 256 / n workgroups per launch (include/loco_hip.h `loco_set_chip_share`)."""
        self._check(self.lib.loco_set_chip_share(self._ctx, int(n)), "loco_set_chip_share")

    def set_side_stream(self, stream: "Optional[torch.cuda.Stream]"):
        """The second stream of `set_streams(2)`: a stream the caller measured to run BESIDE its current stream (HIP hands
        hardware queues out round-robin; `tloco.BranchStreams._pick` does the measurement).  None: the context's own."""
        self._side_stream = stream            # keep the torch object alive while the context may enqueue on it
        ptr = C.c_void_p(stream.cuda_stream) if stream is not None else None
        self._check(self.lib.loco_set_side_stream(self._ctx, ptr), "loco_set_side_stream")

    def set_streams_measured(self, n: int):
        """`set_streams(n)`; for n = 2 the side stream is chosen by measurement (falls back to one stream when no stream of
        this process runs beside the current one)."""
        if n == 2:
            from .tloco import BranchStreams
            side = BranchStreams._pick(1, self.device)
            if not side:
                self.set_streams(1)
                return 1
            self.set_side_stream(side[0])
        self.set_streams(n)
        return n

    def get_precision(self) -> str:
        m = self.lib.loco_get_precision(self._ctx)
        return {v: k for k, v in self.PRECISIONS.items()}[m]

    def _need_diag(self, sym):
        if not hasattr(self.lib, sym):
            raise RuntimeError(f"{sym} is a diagnostic of include/loco_hip_diag.h: build `make -C loco-edit_amd/csrc diag` "
                               "and set LOCO_HIP_LIB=<repo>/loco-edit_amd/libloco_hip_diag.so")

    def bench_conv(self, cin, cout, H, W, B, mode, taps=9, tile=-1, iters=20) -> float:
        self._need_diag("loco_bench_conv")
        ms = C.c_float()
        self._check(self.lib.loco_bench_conv(self._ctx, cin, cout, H, W, B, mode, taps, tile, iters, C.byref(ms),
                                             _stream()), "loco_bench_conv")
        return float(ms.value)

    def debug_conv(self, out: torch.Tensor, with_closing: bool = False, **desc):
        """One conv launch on caller-supplied operands through run_conv -> plan_conv (loco_debug_conv, include/loco_hip_diag.h).
        `desc`: the fields of loco_conv_desc; weight / bias / w2 / bias2nd are CPU float32 tensors, every other operand a
        contiguous float32 device tensor.  Writes `out` and returns (plan, cot_rode): the plan as a list of dicts, one per
        launch and part, and whether a requested norm-cotangent term rode in the epilogue.  with_closing: a third value, the closing
        line of the (main operator's) plan as a dict (stats_all, keep_ntile)."""
        self._need_diag("loco_debug_conv")
        d = LocoConvDesc()
        d.struct_size = C.sizeof(LocoConvDesc)
        d.stride, d.in_arena, d.pad, d.res_scale = 1, 1, -1, 1.0
        keep = []
        _chk_dev(out)
        d.out = out.data_ptr()
        for k, v in desc.items():
            if k not in LocoConvDesc._PTRS:
                if not hasattr(d, k) or k == "struct_size":
                    raise TypeError(f"debug_conv: no descriptor field {k!r}")
                setattr(d, k, v)
            elif v is not None:
                if k in LocoConvDesc._HOST:
                    v = v.detach().to("cpu", torch.float32).contiguous()
                else:
                    _chk_dev(v)
                keep.append(v)
                setattr(d, k, v.data_ptr())
        buf = C.create_string_buffer(1 << 12)
        rc = self.lib.loco_debug_conv(self._ctx, C.byref(d), buf, len(buf), _stream())
        if rc not in (0, 1):
            self._check(rc, "loco_debug_conv")
        plan = []
        closing = None
        for line in buf.value.decode().splitlines():
            rec = dict(f.split("=", 1) for f in line.split(" "))
            rec = {k: (v if k in ("kernel", "stats") else int(v)) for k, v in rec.items()}
            if "launch" in rec:
                plan.append(rec)
            else:
                closing = rec
        return (plan, rc == 0, closing) if with_closing else (plan, rc == 0)

    def debug_norm(self, op: str, **desc):
        """One launch of one standalone GroupNorm launcher (loco_debug_norm, include/loco_hip_diag.h).  `desc`: the fields of
        loco_norm_desc; a tensor operand is a contiguous float32 device tensor (or a view into one: strides are the caller's)."""
        self._need_diag("loco_debug_norm")
        d = LocoNormDesc()
        d.struct_size = C.sizeof(LocoNormDesc)
        d.op, d.base_scale, d.B = LocoNormDesc.OPS[op], 1.0, 1
        keep = []
        for k, v in desc.items():
            if k not in LocoNormDesc._PTRS:
                if not hasattr(d, k) or k in ("struct_size", "op"):
                    raise TypeError(f"debug_norm: no descriptor field {k!r}")
                setattr(d, k, v)
            elif v is not None:
                if not (v.is_cuda and v.dtype == torch.float32):
                    raise TypeError(f"debug_norm: {k} must be a float32 device tensor")
                keep.append(v)
                setattr(d, k, v.data_ptr())
        self._check(self.lib.loco_debug_norm(self._ctx, C.byref(d), _stream()), "loco_debug_norm")

    def debug_pointwise(self, op: str, **desc):
        """One launch of one token-wise / pointwise launcher (loco_debug_pointwise, include/loco_hip_diag.h).  `desc`: the fields of
        loco_pointwise_desc; a tensor operand is a float32 device tensor (uint8 for mask / mask2) or a view into one: strides are
        the caller's.  `f` and `src` are sequences of up to 5 floats / 4 tensors."""
        self._need_diag("loco_debug_pointwise")
        P = LocoPointwiseDesc
        d = P()
        d.struct_size = C.sizeof(P)
        d.op, d.B, d.scale = (P.OPS[op] if isinstance(op, str) else int(op)), 1, 1.0
        keep = []

        def addr(k, v, dtype):
            if not (torch.is_tensor(v) and v.is_cuda and v.dtype == dtype):
                raise TypeError(f"debug_pointwise: {k} must be a {dtype} device tensor")
            keep.append(v)
            return v.data_ptr()
        for k, v in desc.items():
            if k == "f":
                for i, fv in enumerate(v):
                    d.f[i] = fv
            elif k == "src":
                for i, sv in enumerate(v):
                    d.src[i] = None if sv is None else addr(k, sv, torch.float32)
            elif k in P._PTRS or k in P._OUTS or k in P._MASKS:
                if v is not None:
                    setattr(d, k, addr(k, v, torch.uint8 if k in P._MASKS else torch.float32))
            elif not hasattr(d, k) or k in ("struct_size", "op", "pad_"):
                raise TypeError(f"debug_pointwise: no descriptor field {k!r}")
            else:
                setattr(d, k, v)
        self._check(self.lib.loco_debug_pointwise(self._ctx, C.byref(d), _stream()), "loco_debug_pointwise")

    def debug_attn(self, **desc):
        """One pass of one attention stage on caller-supplied tensors through the engine's own attn_* / xa_* functions
        (loco_debug_attn, include/loco_hip_diag.h).  `desc`: the fields of loco_attn_desc (`pass_` for the pass); every tensor a
        contiguous float32 device tensor.  Returns the route: one dict per launch (kernel, and M, N, K, batch, heads, kcat of a GEMM)."""
        self._need_diag("loco_debug_attn")
        d = LocoAttnDesc()
        d.struct_size = C.sizeof(LocoAttnDesc)
        keep = []
        for k, v in desc.items():
            if k not in LocoAttnDesc._PTRS:
                if not hasattr(d, k) or k == "struct_size":
                    raise TypeError(f"debug_attn: no descriptor field {k!r}")
                setattr(d, k, v)
            elif v is not None:
                _chk_dev(v)
                keep.append(v)
                setattr(d, k, v.data_ptr())
        buf = C.create_string_buffer(1 << 12)
        self._check(self.lib.loco_debug_attn(self._ctx, C.byref(d), buf, len(buf), _stream()), "loco_debug_attn")
        route = []
        for line in buf.value.decode().splitlines():
            rec = dict(f.split("=", 1) for f in line.split(" "))
            route.append({k: (v if k == "kernel" else int(v)) for k, v in rec.items()})
        return route

    def debug_gemm(self, op: str, problems, act: str = "none"):
        """One call of one GEMM launcher (loco_debug_gemm, include/loco_hip_diag.h).  `problems`: one dict per problem slot (two for
        "gemm_pair") with the fields of loco_gemm_prob; an operand is a (tensor, offset) pair: a flat float32 device tensor and the
        float offset of the operand's base inside it -- the pointer is the tensor's plus the offset, n_* what is left of the tensor
        from there.  Returns the route: one dict per launch line (kernel, and the numbers of that line)."""
        self._need_diag("loco_debug_gemm")
        d = LocoGemmDesc()
        d.struct_size = C.sizeof(LocoGemmDesc)
        d.op, d.act = LocoGemmDesc.OPS[op], LocoGemmDesc.ACTS[act]
        keep = []
        for slot, prob in enumerate(problems):
            p = d.p[slot]
            p.alpha, p.batch, p.batch2 = 1.0, 1, 1
            for k, v in prob.items():
                if k not in LocoGemmProb._PTRS:
                    if not hasattr(p, k) or k.startswith("n_"):
                        raise TypeError(f"debug_gemm: no descriptor field {k!r}")
                    setattr(p, k, v)
                elif v is not None:
                    t, off = v
                    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.dim() == 1 and 0 <= off < t.numel()):
                        raise TypeError(f"debug_gemm: {k} must be (flat float32 device tensor, offset inside it)")
                    keep.append(t)
                    setattr(p, k, t.data_ptr() + 4 * off)
                    setattr(p, "n_" + k, t.numel() - off)
        buf = C.create_string_buffer(1 << 12)
        self._check(self.lib.loco_debug_gemm(self._ctx, C.byref(d), buf, len(buf), _stream()), "loco_debug_gemm")
        route = []
        for line in buf.value.decode().splitlines():
            rec = dict(f.split("=", 1) for f in line.split(" "))
            route.append({k: (v if k == "kernel" else int(v)) for k, v in rec.items()})
        return route

    def profile_enable(self, on):
        """True/1: per kernel variant; 2: per layer shape; False: off."""
        self._check(self.lib.loco_profile_enable(self._ctx, int(on)), "loco_profile_enable")

    def profile_report(self):
        """-> {kernel variant: dict(launches, ms, flops)} for the conv launches since profile_enable(True)."""
        buf = C.create_string_buffer(1 << 18)
        self._check(self.lib.loco_profile_report(self._ctx, buf, len(buf)), "loco_profile_report")
        out = {}
        for line in buf.value.decode().splitlines():
            name, n, ms, fl = line.rsplit(" ", 3)
            out[name] = dict(launches=int(float(n)), ms=float(ms), flops=float(fl))
        return out

    def debug_tensor(self, name: str, numel: int) -> torch.Tensor:
        self._need_diag("loco_debug_tensor")
        dst = torch.empty(numel, device=self.device, dtype=torch.float32)
        got = self.lib.loco_debug_tensor(self._ctx, name.encode(), _ptr(dst), numel, _stream())
        if got < 0:
            raise RuntimeError(f"loco_debug_tensor({name}) failed: {self.lib.loco_last_error(self._ctx).decode()}")
        return dst[:got]


class _EncoderEngine:
    """What the encoder handles of include/loco_hip.h share on this side: `_prefix` is the symbol prefix of the handle's
    functions (``{prefix}_load_param``, ``_params_missing``, ``_last_error``, ``_destroy``), `_label` names the encoder in
    messages.  A subclass creates the handle with ``_create``."""
    _prefix = ""
    _label = ""

    def _open(self, device: Optional[torch.device]):
        self.lib = load_library()
        if not torch.cuda.is_available() or self.lib.loco_device_count() < 1:
            raise RuntimeError(f"loco_hip: no HIP device visible; the {self._label} has no CPU fallback")
        self.device = torch.device(device if device is not None else "cuda:0")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._t = C.c_void_p()

    def _fn(self, name):
        return getattr(self.lib, f"{self._prefix}_{name}")

    def _create(self, what, c_cfg, *args):
        rc = getattr(self.lib, what)(C.byref(c_cfg), self.device.index, *args, C.byref(self._t))
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self._fn('last_error')(None).decode()}")

    def __del__(self):
        try:
            if getattr(self, "_t", None):
                self._fn("destroy")(self._t)
                self._t = None
        except Exception:
            pass

    def _check(self, rc, what):
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc}): {self._fn('last_error')(self._t).decode()}")

    def load_params(self, sd: Dict[str, "np.ndarray | torch.Tensor"]):
        """Loads the entries of `sd` (a part of the state_dict: a shard, a layer) without asking for completeness."""
        if any(isinstance(v, torch.Tensor) and v.is_cuda for v in sd.values()):
            torch.cuda.synchronize()        # the copies below read device values written on torch's streams
        for name, v in sd.items():
            t = torch.as_tensor(np.asarray(v) if not isinstance(v, torch.Tensor) else v).detach().to(torch.float32).contiguous()
            if not t.is_cuda:
                t = t.cpu()
            shape = (C.c_int64 * max(t.dim(), 1))(*t.shape)
            self._check(self._fn("load_param")(self._t, name.encode(), C.c_void_p(t.data_ptr()), shape, t.dim()),
                        f"{self._prefix}_load_param({name})")

    def check_complete(self):
        missing = self._fn("params_missing")(self._t)
        if missing:
            raise RuntimeError(f"{self._label}: {missing} parameters missing ({self._fn('last_error')(self._t).decode()})")

    def load_state_dict(self, sd: Dict[str, "np.ndarray | torch.Tensor"]):
        """The state_dict of the encoder under the names of its *_load_param (include/loco_hip.h), all of it."""
        self.load_params(sd)
        self.check_complete()


class LocoTextEngine(_EncoderEngine):
    """A text encoder (= loco_text, include/loco_hip.h): parameters on the device, one batched encode per call.
    `cfg` is a ``text_encoder.TextConfig`` (CLIP, loco_text_create) or a ``text_encoder.T5Config`` (the T5 encoder of
    DeepFloyd IF, loco_t5_create); token ids in, last_hidden_state [n, positions, width] out, exact fp32.
    ``load_state_dict`` takes the names of CLIPTextTransformer without a prefix (text_encoder.normalize_text_state_dict
    produces them), or of T5EncoderModel (text_encoder.normalize_t5_state_dict)."""
    _prefix, _label = "loco_text", "text encoder"

    def __init__(self, cfg, max_prompts: int = 8, device: Optional[torch.device] = None):
        self._open(device)
        self.cfg, self.max_prompts = cfg, int(max_prompts)
        self.is_t5 = hasattr(cfg, "d_kv")
        if self.is_t5:
            if cfg.act != "gated-gelu":
                raise ValueError(f"feed_forward_proj {cfg.act!r}: the T5 encoder builds gated-gelu only")
            c = LocoT5Cfg(vocab=cfg.vocab, d_model=cfg.d_model, d_kv=cfg.d_kv, heads=cfg.heads, d_ff=cfg.d_ff, layers=cfg.layers,
                          positions=cfg.positions, buckets=cfg.buckets, max_distance=cfg.max_distance, act=0, ln_eps=cfg.ln_eps)
            self._create("loco_t5_create", c, self.max_prompts)
        else:
            c = LocoTextCfg(vocab=cfg.vocab, width=cfg.width, layers=cfg.layers, heads=cfg.heads, ffn=cfg.ffn,
                            positions=cfg.positions, act={"quick_gelu": 0, "gelu": 1}[cfg.act], ln_eps=cfg.ln_eps)
            self._create("loco_text_create", c, self.max_prompts)

    @property
    def width(self) -> int:
        return self.cfg.d_model if self.is_t5 else self.cfg.width

    def encode_ids(self, ids: torch.Tensor, out: Optional[torch.Tensor] = None, lens=None) -> torch.Tensor:
        """ids [n, positions] (any integer dtype, host or device) -> [n, positions, width] fp32 on the device.
        lens (T5 only): the count of real tokens of every prompt, keys beyond it are masked; None = all `positions`."""
        ids = torch.as_tensor(ids)
        if ids.dim() != 2 or ids.shape[1] != self.cfg.positions:
            raise ValueError(f"ids must be [n, {self.cfg.positions}], got {tuple(ids.shape)}")
        n = ids.shape[0]
        ids = ids.to(device=self.device, dtype=torch.int32).contiguous()
        if out is None:
            out = torch.empty(n, self.cfg.positions, self.width, device=self.device, dtype=torch.float32)
        _chk_dev(out)
        if tuple(out.shape) != (n, self.cfg.positions, self.width):
            raise ValueError(f"out must be [{n}, {self.cfg.positions}, {self.width}], got {tuple(out.shape)}")
        with torch.cuda.device(self.device):
            if lens is None and not self.is_t5:
                self._check(self.lib.loco_text_encode(self._t, _ptr(ids), n, _ptr(out), _stream()), "loco_text_encode")
            else:
                larr = None
                if lens is not None:
                    lens = [int(v) for v in (lens.tolist() if isinstance(lens, torch.Tensor) else lens)]
                    if len(lens) != n:
                        raise ValueError(f"lens must hold {n} lengths, got {len(lens)}")
                    larr = (C.c_int32 * n)(*lens)
                self._check(self.lib.loco_text_encode_masked(self._t, _ptr(ids), larr, n, _ptr(out), _stream()),
                            "loco_text_encode_masked")
        return out


class LocoSamEngine(_EncoderEngine):
    """The image encoder of Segment Anything (= loco_sam, include/loco_hip.h): parameters and the workspace of one image on
    the device.  `cfg` is a ``mask_segmentation.SamVisionConfig``; preprocessed pixel_values [3, S, S] in, image embeddings
    [1, C_out, G, G] out, exact fp32.  ``load_state_dict`` takes the names of SamVisionEncoder without a prefix
    (mask_segmentation.vision_state_dict produces them)."""
    _prefix, _label = "loco_sam", "SAM image encoder"

    def __init__(self, cfg, device: Optional[torch.device] = None):
        self._open(device)
        self.cfg = cfg
        glob = [int(i) for i in cfg.global_attn_indexes]
        if len(glob) > SAM_MAX_GLOBAL:
            raise ValueError(f"at most {SAM_MAX_GLOBAL} global attention layers, got {len(glob)}")
        c = LocoSamCfg(image_size=cfg.image_size, patch_size=cfg.patch_size, width=cfg.hidden_size, depth=cfg.num_hidden_layers,
                       heads=cfg.num_attention_heads, mlp_dim=cfg.mlp_dim, window_size=cfg.window_size, num_global=len(glob),
                       out_channels=cfg.output_channels, ln_eps=cfg.layer_norm_eps)
        for i, g in enumerate(glob):
            c.global_attn[i] = g
        self.grid = cfg.image_size // cfg.patch_size
        self._create("loco_sam_create", c)

    def encode(self, pixel_values: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """pixel_values [3, S, S] or [1, 3, S, S] (fp32, host or device) -> [1, C_out, G, G] fp32 on the device."""
        S, G, Co = self.cfg.image_size, self.grid, self.cfg.output_channels
        pv = torch.as_tensor(pixel_values)
        if tuple(pv.shape) == (1, 3, S, S):
            pv = pv[0]
        if tuple(pv.shape) != (3, S, S):
            raise ValueError(f"pixel_values must be [3, {S}, {S}] (one image per call), got {tuple(pv.shape)}")
        pv = pv.to(device=self.device, dtype=torch.float32).contiguous()
        if out is None:
            out = torch.empty(1, Co, G, G, device=self.device, dtype=torch.float32)
        _chk_dev(out)
        if tuple(out.shape) != (1, Co, G, G):
            raise ValueError(f"out must be [1, {Co}, {G}, {G}], got {tuple(out.shape)}")
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_sam_encode(self._t, _ptr(pv), _ptr(out), _stream()), "loco_sam_encode")
        return out

    def profile(self, on: bool):
        self._check(self.lib.loco_sam_profile(self._t, int(bool(on))), "loco_sam_profile")

    def profile_read(self) -> Dict[str, float]:
        """Milliseconds of the last profiled encode by kind of launch (waits for it)."""
        ms = (C.c_float * 4)()
        self._check(self.lib.loco_sam_profile_read(self._t, ms), "loco_sam_profile_read")
        return dict(zip(("gemm", "window_attn", "global_attn", "other"), [float(v) for v in ms]))


class LocoSamHeadEngine(_EncoderEngine):
    """The prompt encoder, mask decoder and mask scoring of Segment Anything (= loco_samdec, include/loco_hip.h): parameters
    and the workspace of `max_prompts` point prompts on the device.  `cfg` is a ``mask_segmentation.SamConfig``;
    ``load_state_dict`` takes the names of SamModel (mask_segmentation.head_state_dict produces them).  ``set_image`` once per
    image embedding, then ``predict`` per batch of prompts; ``score`` / ``binarize`` are the automatic mask generator's view of
    low-resolution logits at the original size.  Exact fp32."""
    _prefix, _label = "loco_samdec", "SAM prompt encoder / mask decoder"

    def __init__(self, cfg, max_prompts: int = 64, device: Optional[torch.device] = None):
        self._open(device)
        self.cfg, self.max_prompts = cfg, int(max_prompts)
        d, v = cfg.decoder, cfg.vision
        if d.hidden_act not in ("relu", "gelu"):
            raise ValueError(f"mask_decoder hidden_act {d.hidden_act!r}: the head builds relu and the erf gelu")
        self.grid, self.hidden, self.num_masks = v.grid, d.hidden_size, d.num_multimask_outputs
        c = LocoSamDecCfg(grid=v.grid, image_size=v.image_size, hidden=d.hidden_size, layers=d.num_hidden_layers,
                          heads=d.num_attention_heads, mlp_dim=d.mlp_dim, attention_downsample_rate=d.attention_downsample_rate,
                          num_multimask_outputs=d.num_multimask_outputs, iou_head_depth=d.iou_head_depth,
                          iou_head_hidden_dim=d.iou_head_hidden_dim, layer_norm_eps=d.layer_norm_eps,
                          hidden_act={"relu": 0, "gelu": 1}[d.hidden_act], max_prompts=self.max_prompts)
        self._create("loco_samdec_create", c)

    def set_image(self, image_embeddings: torch.Tensor):
        """image_embeddings [1, C, G, G] or [C, G, G] (fp32): everything that does not depend on the prompts."""
        C_, G = self.hidden, self.grid
        emb = torch.as_tensor(image_embeddings)
        if tuple(emb.shape) == (1, C_, G, G):
            emb = emb[0]
        if tuple(emb.shape) != (C_, G, G):
            raise ValueError(f"image_embeddings must be [1, {C_}, {G}, {G}] (the grid of this head), got {tuple(image_embeddings.shape)}")
        emb = emb.to(device=self.device, dtype=torch.float32).contiguous()
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_samdec_set_image(self._t, _ptr(emb), _stream()), "loco_samdec_set_image")

    def predict(self, coords: torch.Tensor):
        """coords [P, 2] fp32: (x, y) as 2 (p + 0.5) / S - 1 -> (low-resolution logits [P, n, 4G, 4G], predicted IoU [P, n])."""
        coords = torch.as_tensor(coords)
        if coords.dim() != 2 or coords.shape[1] != 2:
            raise ValueError(f"coords must be [P, 2], got {tuple(coords.shape)}")
        P, n, side = coords.shape[0], self.num_masks, 4 * self.grid
        if not 1 <= P <= self.max_prompts:
            raise ValueError(f"{P} prompts: one predict call carries 1 ... max_prompts = {self.max_prompts}")
        coords = coords.to(device=self.device, dtype=torch.float32).contiguous()
        masks = torch.empty(P, n, side, side, device=self.device, dtype=torch.float32)
        iou = torch.empty(P, n, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_samdec_predict(self._t, _ptr(coords), P, _ptr(masks), _ptr(iou), _stream()), "loco_samdec_predict")
        return masks, iou

    def _low(self, low_res):
        low = torch.as_tensor(low_res)
        if low.dim() != 3:
            raise ValueError(f"low_res must be [N, h, w], got {tuple(low.shape)}")
        return low.to(device=self.device, dtype=torch.float32).contiguous()

    def score(self, low_res, original_size, reshaped_size, image_size: int, mask_threshold: float, offset: float):
        """low_res [N, h, w] -> (counts [N, 2] int32: pixels above threshold + offset / - offset; boxes [N, 4] int32: inclusive
        XYXY of logit > threshold), all at `original_size` through the two bilinear stages of MaskGenerator.upsample."""
        low = self._low(low_res)
        N, h, w = low.shape
        counts = torch.empty(N, 2, device=self.device, dtype=torch.int32)
        boxes = torch.empty(N, 4, device=self.device, dtype=torch.int32)
        (oh, ow), (rh, rw) = original_size, reshaped_size
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_samdec_score(self._t, _ptr(low), N, h, w, int(oh), int(ow), int(rh), int(rw), int(image_size),
                                                   float(mask_threshold), float(offset), _ptr(counts), _ptr(boxes), _stream()),
                        "loco_samdec_score")
        return counts, boxes

    def binarize(self, low_res, rows, original_size, reshaped_size, image_size: int, mask_threshold: float) -> torch.Tensor:
        """bool [K, H, W]: logit > threshold at `original_size` for the rows `rows` [K] of low_res [N, h, w]."""
        low = self._low(low_res)
        N, h, w = low.shape
        rows = torch.as_tensor(rows).to(device=self.device, dtype=torch.int32).contiguous()
        (oh, ow), (rh, rw) = original_size, reshaped_size
        K = int(rows.numel())
        out = torch.empty(K, int(oh), int(ow), device=self.device, dtype=torch.uint8)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_samdec_binarize(self._t, _ptr(low), N, _ptr(rows), K, h, w, int(oh), int(ow), int(rh), int(rw),
                                                      int(image_size), float(mask_threshold), _ptr(out), _stream()),
                        "loco_samdec_binarize")
        return out.bool()


class LocoClipVisionEngine(_EncoderEngine):
    """The CLIP image encoder (= loco_clipvis, include/loco_hip.h): parameters and the workspace of `max_images` images on
    the device.  `cfg` is a ``clip_score.ClipVisionConfig``; ``preprocess`` turns uint8 frames [n, H, W, 3] into the
    pixel_values [n, 3, S, S] of CLIPImageProcessor in float arithmetic, ``encode`` turns pixel_values into the
    un-normalised image_embeds [n, P], exact fp32.  ``load_state_dict`` takes the names of CLIPVisionModelWithProjection
    without the ``vision_model.`` prefix (clip_score.split_clip_state_dict produces them)."""
    _prefix, _label = "loco_clipvis", "CLIP image encoder"

    def __init__(self, cfg, max_images: int = 8, device: Optional[torch.device] = None, grad: bool = False):
        self._open(device)
        self.cfg, self.max_images = cfg, int(max_images)
        c = LocoClipVisCfg(image_size=cfg.image_size, patch_size=cfg.patch_size, width=cfg.width, layers=cfg.layers, heads=cfg.heads,
                           mlp_dim=cfg.mlp_dim, projection_dim=cfg.projection_dim, act={"quick_gelu": 0, "gelu": 1}[cfg.act],
                           ln_eps=cfg.ln_eps)
        for i in range(3):
            c.image_mean[i], c.image_std[i] = cfg.image_mean[i], cfg.image_std[i]
        self._create("loco_clipvis_create", c, self.max_images)
        self.grad = bool(grad)
        if self.grad:
            with torch.cuda.device(self.device):
                self._check(self.lib.loco_clipvis_enable_grad(self._t, 1), "loco_clipvis_enable_grad")

    @property
    def grad_bytes(self) -> int:
        """Bytes of the per-layer records and the gradient workspace (0 without ``grad``)."""
        return int(self.lib.loco_clipvis_grad_bytes(self._t))

    def _boxes(self, boxes, n_default):
        """-> (int32 [n, 4] on the device or None, n)"""
        if boxes is None:
            return None, n_default
        b = torch.as_tensor(boxes)
        if b.dim() != 2 or b.shape[1] != 4 or b.shape[0] < 1 or b.is_floating_point():
            raise ValueError(f"boxes must be integer [n, 4] = (top, left, h, w), got {b.dtype} {tuple(b.shape)}")
        return b.to(device=self.device, dtype=torch.int32).contiguous(), int(b.shape[0])

    def preprocess_float(self, frames: torch.Tensor, boxes=None) -> torch.Tensor:
        """frames [nf, 3, H, W] or [3, H, W] (fp32 in [-1, 1], host or device), boxes integer [n, 4] = (top, left, h, w) or None
        (the centred largest square of every frame) -> pixel_values [n, 3, S, S] on the device; nf is 1 or n."""
        fr = torch.as_tensor(frames)
        if fr.dim() == 3:
            fr = fr[None]
        if fr.dim() != 4 or fr.shape[1] != 3 or not fr.is_floating_point() or 0 in fr.shape:
            raise ValueError(f"frames must be floating point [nf, 3, H, W], got {fr.dtype} {tuple(fr.shape)}")
        fr = fr.to(device=self.device, dtype=torch.float32).contiguous()
        nf, H, W, S = fr.shape[0], fr.shape[2], fr.shape[3], self.cfg.image_size
        bx, n = self._boxes(boxes, nf)
        out = torch.empty(n, 3, S, S, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_preprocess_f32(self._t, _ptr(fr), nf, _ptr(bx), n, H, W, _ptr(out), _stream()),
                        "loco_clipvis_preprocess_f32")
        return out

    def preprocess_float_vjp(self, g_pixel_values: torch.Tensor, boxes, nf: int, H: int, W: int) -> torch.Tensor:
        """The transpose of ``preprocess_float``: g_pixel_values [n, 3, S, S] -> the cotangent of the frames [nf, 3, H, W]."""
        S = self.cfg.image_size
        g = torch.as_tensor(g_pixel_values)
        if g.dim() != 4 or tuple(g.shape[1:]) != (3, S, S) or g.shape[0] < 1:
            raise ValueError(f"g_pixel_values must be [n, 3, {S}, {S}], got {tuple(g.shape)}")
        g = g.to(device=self.device, dtype=torch.float32).contiguous()
        bx, n = self._boxes(boxes, g.shape[0])
        if n != g.shape[0]:
            raise ValueError(f"{n} boxes for {g.shape[0]} gradients")
        nf, H, W = int(nf), int(H), int(W)
        if nf < 1 or H < 1 or W < 1:
            raise ValueError("nf, H and W must be positive")
        out = torch.empty(nf, 3, H, W, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_preprocess_f32_vjp(self._t, _ptr(g), _ptr(bx), n, nf, H, W, _ptr(out), _stream()),
                        "loco_clipvis_preprocess_f32_vjp")
        return out

    def encode_vjp(self, g_embeds: torch.Tensor) -> torch.Tensor:
        """g_embeds [n, P] -> the cotangent of image_embeds with respect to the pixel_values [n, 3, S, S] of the last
        ``encode`` (a ``grad=True`` engine keeps its records)."""
        S, P = self.cfg.image_size, self.cfg.projection_dim
        g = torch.as_tensor(g_embeds)
        if g.dim() != 2 or g.shape[1] != P or g.shape[0] < 1:
            raise ValueError(f"g_embeds must be [n, {P}], got {tuple(g.shape)}")
        n = g.shape[0]
        g = g.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(n, 3, S, S, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_encode_vjp(self._t, _ptr(g), n, _ptr(out), _stream()), "loco_clipvis_encode_vjp")
        return out

    @property
    def tokens(self) -> int:
        return 1 + (self.cfg.image_size // self.cfg.patch_size) ** 2

    def preprocess(self, frames_uint8: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """frames [n, H, W, 3] or [H, W, 3] (uint8, host or device) -> pixel_values [n, 3, S, S] fp32 on the device."""
        fr = torch.as_tensor(frames_uint8)
        if fr.dim() == 3:
            fr = fr[None]
        if fr.dim() != 4 or fr.shape[-1] != 3 or fr.dtype != torch.uint8 or 0 in fr.shape:
            raise ValueError(f"frames must be uint8 [n, H, W, 3], got {fr.dtype} {tuple(fr.shape)}")
        fr = fr.to(self.device).contiguous()
        n, H, W, S = fr.shape[0], fr.shape[1], fr.shape[2], self.cfg.image_size
        if out is None:
            out = torch.empty(n, 3, S, S, device=self.device, dtype=torch.float32)
        _chk_dev(out)
        if tuple(out.shape) != (n, 3, S, S):
            raise ValueError(f"out must be [{n}, 3, {S}, {S}], got {tuple(out.shape)}")
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_preprocess(self._t, _ptr(fr), n, H, W, _ptr(out), _stream()), "loco_clipvis_preprocess")
        return out

    def encode(self, pixel_values: torch.Tensor, want_hidden: bool = False):
        """pixel_values [n, 3, S, S] (fp32, host or device), n <= max_images -> image_embeds [n, P] on the device;
        ``want_hidden``: (image_embeds, last_hidden_state [n, T, D], pooler_output [n, D])."""
        S, D, P = self.cfg.image_size, self.cfg.width, self.cfg.projection_dim
        pv = torch.as_tensor(pixel_values)
        if pv.dim() != 4 or tuple(pv.shape[1:]) != (3, S, S) or pv.shape[0] < 1:
            raise ValueError(f"pixel_values must be [n, 3, {S}, {S}], got {tuple(pv.shape)}")
        n = pv.shape[0]
        pv = pv.to(device=self.device, dtype=torch.float32).contiguous()
        emb = torch.empty(n, P, device=self.device, dtype=torch.float32)
        hid = torch.empty(n, self.tokens, D, device=self.device, dtype=torch.float32) if want_hidden else None
        pool = torch.empty(n, D, device=self.device, dtype=torch.float32) if want_hidden else None
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_encode(self._t, _ptr(pv), n, _ptr(emb), _ptr(hid), _ptr(pool), _stream()),
                        "loco_clipvis_encode")
        return (emb, hid, pool) if want_hidden else emb

    def encode_taps(self, pixel_values: torch.Tensor, layers) -> torch.Tensor:
        """pixel_values [n, 3, S, S], n <= max_images; layers: strictly increasing 0-based layer indices -> the residual stream
        after each of them [n_taps, n, T, D] (slot j = ``hidden_states[layers[j] + 1]`` of transformers).  The tower stops
        after the last tapped layer."""
        S, D = self.cfg.image_size, self.cfg.width
        pv = torch.as_tensor(pixel_values)
        if pv.dim() != 4 or tuple(pv.shape[1:]) != (3, S, S) or pv.shape[0] < 1:
            raise ValueError(f"pixel_values must be [n, 3, {S}, {S}], got {tuple(pv.shape)}")
        layers = [int(v) for v in layers]
        n = pv.shape[0]
        pv = pv.to(device=self.device, dtype=torch.float32).contiguous()
        out = torch.empty(max(len(layers), 1), n, self.tokens, D, device=self.device, dtype=torch.float32)
        arr = (C.c_int32 * max(len(layers), 1))(*layers)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipvis_encode_taps(self._t, _ptr(pv), n, arr, len(layers), _ptr(out), _stream()),
                        "loco_clipvis_encode_taps")
        return out


class LocoClipSegDecoder(_EncoderEngine):
    """The CLIPSeg decoder (= loco_clipseg, include/loco_hip.h, csrc/clipseg.hip): parameters and the workspace of `max_masks`
    masks on the device.  `cfg` is a ``prompt_mask.ClipSegDecoderConfig``.  ``decode`` turns the taps of
    ``LocoClipVisionEngine.encode_taps`` and one conditional embedding per mask into logits, ``preprocess`` resizes frames the
    way ViTImageProcessor does for CLIPSeg, ``masks`` resizes logits bilinearly and thresholds them.  ``load_state_dict``
    takes the names of transformers' ``decoder.*`` without the prefix."""
    _prefix, _label = "loco_clipseg", "CLIPSeg decoder"

    def __init__(self, cfg, device: Optional[torch.device] = None):
        self._open(device)
        self.cfg = cfg
        c = LocoClipSegCfg(width=cfg.width, grid=cfg.grid, patch_size=cfg.patch_size, reduce_dim=cfg.reduce_dim, heads=cfg.heads,
                           ffn=cfg.ffn, n_taps=cfg.n_taps, conditional_layer=cfg.conditional_layer, projection_dim=cfg.projection_dim,
                           complex_head=int(bool(cfg.complex_head)), ln_eps=cfg.ln_eps, max_masks=cfg.max_masks)
        self._create("loco_clipseg_create", c)
        self.logit_size = int(self.lib.loco_clipseg_logit_size(self._t))

    def decode(self, taps: torch.Tensor, cond: torch.Tensor, image_of_mask=None) -> torch.Tensor:
        """taps [n_taps, n, T, D] (device), cond [M, P], image_of_mask: M image indices (None: mask m looks at image m) ->
        logits [M, s, s] on the device."""
        cfg, T = self.cfg, 1 + self.cfg.grid ** 2
        taps = torch.as_tensor(taps)
        if taps.dim() != 4 or taps.shape[0] != cfg.n_taps or tuple(taps.shape[2:]) != (T, cfg.width) or taps.shape[1] < 1:
            raise ValueError(f"taps must be [{cfg.n_taps}, n, {T}, {cfg.width}], got {tuple(taps.shape)}")
        cond = torch.as_tensor(cond)
        if cond.dim() != 2 or cond.shape[1] != cfg.projection_dim:
            raise ValueError(f"cond must be [M, {cfg.projection_dim}], got {tuple(cond.shape)}")
        M, n = cond.shape[0], taps.shape[1]
        iom = list(range(M)) if image_of_mask is None else [int(v) for v in image_of_mask]
        if len(iom) != M:
            raise ValueError(f"image_of_mask must hold {M} indices, got {len(iom)}")
        taps = taps.to(device=self.device, dtype=torch.float32).contiguous()
        cond = cond.to(device=self.device, dtype=torch.float32).contiguous()
        s = self.logit_size
        out = torch.empty(M, s, s, device=self.device, dtype=torch.float32)
        arr = (C.c_int32 * max(M, 1))(*iom)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipseg_decode(self._t, _ptr(taps), n, _ptr(cond), arr, M, _ptr(out), _stream()),
                        "loco_clipseg_decode")
        return out

    def preprocess(self, frames: torch.Tensor, size: int, resample: int, mean, std) -> torch.Tensor:
        """frames fp32 [n, 3, H, W] in [-1, 1] or uint8 [n, H, W, 3] -> pixel_values [n, 3, size, size] on the device."""
        fr = torch.as_tensor(frames)
        if fr.dtype == torch.uint8:
            if fr.dim() != 4 or fr.shape[-1] != 3 or 0 in fr.shape:
                raise ValueError(f"uint8 frames must be [n, H, W, 3], got {tuple(fr.shape)}")
            n, H, W, u8 = fr.shape[0], fr.shape[1], fr.shape[2], 1
            fr = fr.to(self.device).contiguous()
        else:
            if fr.dim() != 4 or fr.shape[1] != 3 or not fr.is_floating_point() or 0 in fr.shape:
                raise ValueError(f"frames must be uint8 [n, H, W, 3] or floating point [n, 3, H, W], got {fr.dtype} {tuple(fr.shape)}")
            n, H, W, u8 = fr.shape[0], fr.shape[2], fr.shape[3], 0
            fr = fr.to(device=self.device, dtype=torch.float32).contiguous()
        size = int(size)
        out = torch.empty(n, 3, max(size, 1), max(size, 1), device=self.device, dtype=torch.float32)
        m3, s3 = (C.c_float * 3)(*[float(v) for v in mean]), (C.c_float * 3)(*[float(v) for v in std])
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipseg_preprocess(self._t, _ptr(fr), u8, n, H, W, size, int(resample), m3, s3, _ptr(out), _stream()),
                        "loco_clipseg_preprocess")
        return out

    def masks(self, logits: torch.Tensor, resolution: int, threshold_logit: float):
        """logits [M, s, s] -> (mask uint8 [M, res, res], area int32 [M]) on the device."""
        lg = torch.as_tensor(logits)
        if lg.dim() != 3 or lg.shape[1] != lg.shape[2] or 0 in lg.shape:
            raise ValueError(f"logits must be [M, s, s], got {tuple(lg.shape)}")
        lg = lg.to(device=self.device, dtype=torch.float32).contiguous()
        M, s, res = lg.shape[0], lg.shape[1], int(resolution)
        mask = torch.empty(M, max(res, 1), max(res, 1), device=self.device, dtype=torch.uint8)
        area = torch.empty(M, device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_clipseg_masks(self._t, _ptr(lg), M, s, res, float(threshold_logit), _ptr(mask), _ptr(area), _stream()),
                        "loco_clipseg_masks")
        return mask, area


class LocoQualityEngine(_EncoderEngine):
    """The edit-quality scorer (= loco_quality, include/loco_hip.h): LPIPS (AlexNet), SSIM and mask-restricted MSE between
    the images of two batches, pair by pair, as ``eval.lpips`` / ``eval.ssim`` / ``eval.masked_mse`` define them.  The
    workspace holds `max_pairs` pairs of `max_hw` = (H, W) images.  ``load_state_dict`` takes the names of
    ``eval.lpips_weight_names()``; ``ssim`` and ``masked_mse`` need no parameters.  Every method returns one value per pair
    on the device."""
    _prefix, _label = "loco_quality", "quality scorer"

    def __init__(self, max_hw=(256, 256), max_pairs: int = 32, device: Optional[torch.device] = None):
        self._open(device)
        self.max_hw, self.max_pairs = (int(max_hw[0]), int(max_hw[1])), int(max_pairs)
        c = LocoQualityCfg(max_h=self.max_hw[0], max_w=self.max_hw[1])
        x = torch.arange(11, dtype=torch.float64) - 5.0                # the 1-D factor of eval._gaussian_window, in float64
        g = torch.exp(-(x / 1.5) ** 2 / 2)
        g = g / g.sum()
        for i in range(11):
            c.ssim_window[i] = float(g[i])
        self._create("loco_quality_create", c, self.max_pairs)

    def _pair(self, a, b, channels=None):
        a, b = torch.as_tensor(a), torch.as_tensor(b)
        if a.shape != b.shape or a.dim() != 4 or a.shape[0] < 1 or (channels is not None and a.shape[1] != channels):
            raise ValueError(f"expected a and b of the same shape [n,{channels or 'C'},H,W], got {tuple(a.shape)} and {tuple(b.shape)}")
        return (a.to(device=self.device, dtype=torch.float32).contiguous(), b.to(device=self.device, dtype=torch.float32).contiguous())

    def lpips(self, a: torch.Tensor, b: torch.Tensor, normalize: bool = False, want_taps: bool = False):
        """a, b [n,3,H,W] in [-1, 1] (``normalize``: in [0, 1]), n <= max_pairs -> LPIPS [n] fp32; ``want_taps``: (LPIPS, the five
        terms [n,5])."""
        a, b = self._pair(a, b, 3)
        n, _, H, W = a.shape
        out = torch.empty(n, device=self.device, dtype=torch.float32)
        taps = torch.empty(n, 5, device=self.device, dtype=torch.float32) if want_taps else None
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_quality_lpips(self._t, _ptr(a), _ptr(b), n, H, W, int(bool(normalize)), _ptr(out), _ptr(taps),
                                                    _stream()), "loco_quality_lpips")
        return (out, taps) if want_taps else out

    def ssim(self, a: torch.Tensor, b: torch.Tensor, data_range=None) -> torch.Tensor:
        """a, b [n,C,H,W] -> mean SSIM of every pair [n] float64.  ``data_range=None``: the larger of the two dynamic ranges over
        the batch, as in ``eval.ssim`` (read back from the device before the call)."""
        a, b = self._pair(a, b)
        n, ch, H, W = a.shape
        if data_range is None:
            lo_a, hi_a = torch.aminmax(a)
            lo_b, hi_b = torch.aminmax(b)
            data_range = max(float(hi_a.double() - lo_a.double()), float(hi_b.double() - lo_b.double()))
        out = torch.empty(n, device=self.device, dtype=torch.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_quality_ssim(self._t, _ptr(a), _ptr(b), n, ch, H, W, float(data_range), _ptr(out), _stream()),
                        "loco_quality_ssim")
        return out

    def masked_mse(self, a: torch.Tensor, b: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        """MSE of every pair over ``mask`` only (boolean, broadcastable to the images) [n] float64; ``ValueError("empty mask")``
        when a pair has no masked element, as ``eval.masked_mse``."""
        a, b = self._pair(a, b)
        n = a.shape[0]
        m = torch.as_tensor(mask).to(self.device).to(torch.bool).expand_as(a).to(torch.uint8).contiguous()
        s = torch.empty(n, device=self.device, dtype=torch.float64)
        cnt = torch.empty(n, device=self.device, dtype=torch.int64)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_quality_masked_mse(self._t, _ptr(a), _ptr(b), _ptr(m), n, a[0].numel(), _ptr(s), _ptr(cnt),
                                                         _stream()), "loco_quality_masked_mse")
        if bool((cnt == 0).any()):
            raise ValueError("empty mask")
        return s / cnt.double()


class LocoPca(_EncoderEngine):
    """Randomized, centred low-rank PCA of a sample matrix that stays on the device (= loco_pca, include/loco_hip.h): the
    sample store ``[n_max, d]`` (fp32) and every workspace live in the handle.  ``add_rows`` appends, ``fit`` returns
    ``(s [q], V [d, q], mean [d])`` as a deterministic function of the store and ``omega``.  ``ValueError`` for arguments
    that are refused here (dtype, device, shapes), ``RuntimeError`` with the library's message for what it refuses
    (capacity, q, numerical rank)."""
    _prefix, _label = "loco_pca", "device PCA"
    ROUTES = {"auto": 0, "gemm": 1, "split": 2}
    Q_LIMIT = 512

    def __init__(self, n_max: int, d: int, q_max: int, device: Optional[torch.device] = None):
        self._open(device)
        self.n_max, self.d, self.q_max = int(n_max), int(d), int(q_max)
        if self.q_max > self.Q_LIMIT:
            raise ValueError(f"q_max = {self.q_max} is above the unit's limit of {self.Q_LIMIT}")
        with torch.cuda.device(self.device):
            rc = self.lib.loco_pca_create(self.device.index, self.n_max, self.d, self.q_max, C.byref(self._t))
        if rc != 0:
            raise RuntimeError(f"loco_pca_create failed ({rc}): {self.lib.loco_pca_last_error(None).decode()}")

    def _chk(self, t: torch.Tensor, what: str, shape=None, dtype=torch.float32) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: expected a tensor")
        if t.dtype != dtype:
            raise ValueError(f"{what}: expected {dtype}, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{what}: expected a tensor on {self.device}, got one on {t.device}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    @property
    def rows(self) -> int:
        return int(self.lib.loco_pca_rows(self._t))

    def reset(self):
        self._check(self.lib.loco_pca_reset(self._t), "loco_pca_reset")

    def set_route(self, route: str):
        """'auto' (launch_gemm where the output grid fills the chip, else the split-contraction kernel), 'gemm', 'split'."""
        if route not in self.ROUTES:
            raise ValueError(f"route must be one of {sorted(self.ROUTES)}, got {route!r}")
        self._check(self.lib.loco_pca_set_route(self._t, self.ROUTES[route]), "loco_pca_set_route")

    def routes(self) -> str:
        return self.lib.loco_pca_routes(self._t).decode()

    def add_rows(self, rows: torch.Tensor):
        """Appends ``rows [b, d]`` (fp32, on the handle's device)."""
        if not isinstance(rows, torch.Tensor) or rows.dim() != 2:
            raise ValueError("add_rows: expected rows [b, d]")
        rows = self._chk(rows, "add_rows")
        if rows.shape[0] == 0:
            return
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_add_rows(self._t, _ptr(rows), rows.shape[0], rows.shape[1], _stream()), "loco_pca_add_rows")
            torch.cuda.current_stream().synchronize()       # `rows` may be a temporary of the caller

    def fit(self, q: int, niter: int, omega: torch.Tensor, center: bool = True):
        """``(s [q], V [d, q], mean [d])`` of the rows held; ``omega [d, q]`` is the caller's random test matrix."""
        q, niter = int(q), int(niter)
        if q < 1:
            raise ValueError(f"fit: q = {q} must be positive")
        omega = self._chk(omega, "fit: omega", (self.d, q))
        s = torch.zeros(q, device=self.device, dtype=torch.float32)
        V = torch.zeros(self.d, q, device=self.device, dtype=torch.float32)
        mean = torch.zeros(self.d, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_fit(self._t, q, niter, _ptr(omega), int(bool(center)), _ptr(s), _ptr(V), _ptr(mean), _stream()),
                        "loco_pca_fit")
        return s, V, mean

    def center(self, center: bool = True):
        """Forms the centred store inside the handle (what ``fit`` does first), without copying it out."""
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_center(self._t, int(bool(center)), None, None, _stream()), "loco_pca_center")

    def centered(self, center: bool = True):
        """``(Hc [N, d], mean [d])``: the centred store as ``fit`` reads it."""
        Hc = torch.empty(self.rows, self.d, device=self.device, dtype=torch.float32)
        mean = torch.empty(self.d, device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_center(self._t, int(bool(center)), _ptr(Hc), _ptr(mean), _stream()), "loco_pca_center")
        return Hc, mean

    def gram(self, Y: torch.Tensor) -> torch.Tensor:
        """``Y^T Y [q, q]`` in float64 for ``Y [rows, q]`` (fp32), summed as ``fit`` sums its Gram matrices."""
        if not isinstance(Y, torch.Tensor) or Y.dim() != 2:
            raise ValueError("gram: expected Y [rows, q]")
        Y = self._chk(Y, "gram: Y")
        G = torch.empty(Y.shape[1], Y.shape[1], device=self.device, dtype=torch.float64)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_gram(self._t, _ptr(Y), Y.shape[0], Y.shape[1], _ptr(G), _stream()), "loco_pca_gram")
        return G

    def project(self, W: torch.Tensor, transpose: bool = False, center: bool = True) -> torch.Tensor:
        """``Hc W [N, q]`` for ``W [d, q]``, or with ``transpose`` ``Hc^T W [d, q]`` for ``W [N, q]``."""
        if not isinstance(W, torch.Tensor) or W.dim() != 2:
            raise ValueError("project: expected W [rows, q]")
        n = self.rows
        W = self._chk(W, "project: W", (n if transpose else self.d, W.shape[1]))
        out = torch.empty(self.d if transpose else n, W.shape[1], device=self.device, dtype=torch.float32)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_pca_project(self._t, _ptr(W), W.shape[1], int(bool(transpose)), int(bool(center)), _ptr(out), _stream()),
                        "loco_pca_project")
        return out


class LocoAsyrpBlock(_EncoderEngine):
    """The trainable h-space block f_t of the Asyrp baseline (= loco_asyrp, include/loco_hip.h):
    ``dh = s (W2 swish(GN(W1 swish(GN(h)) + c1 + Wt swish(e) + ct)) + c2)`` for ``h [B, C, H, W]`` and a time vector ``e [E]``.
    The parameters, their gradient store and Adam's moments live in the handle.  ``forward`` keeps the records ``backward``
    reads; ``backward`` ADDS the parameter gradients to the store.  ``ValueError`` for arguments refused here (dtype, device,
    shapes), ``RuntimeError`` with the library's message for what it refuses (geometry, missing records)."""
    _prefix, _label = "loco_asyrp", "Asyrp block"
    PARAMS = ("g1", "b1", "W1", "c1", "Wt", "ct", "g2", "b2", "W2", "c2")
    GROUPS = 32

    @staticmethod
    def param_shapes(C_: int, E: int) -> Dict[str, tuple]:
        return {"g1": (C_,), "b1": (C_,), "W1": (C_, C_), "c1": (C_,), "Wt": (C_, E), "ct": (C_,), "g2": (C_,), "b2": (C_,),
                "W2": (C_, C_), "c2": (C_,)}

    @staticmethod
    def init_params(C_: int, E: int, seed: int = 0) -> Dict[str, torch.Tensor]:
        """The seeded initial state (fp32, CPU): unit gains, zero offsets and biases, W1 / Wt uniform in +-1 / sqrt(fan_in),
        W2 = c2 = 0 -- an untrained block is the identity edit (dh = 0)."""
        gen = torch.Generator().manual_seed(int(seed))
        sd = {k: torch.zeros(s, dtype=torch.float32) for k, s in LocoAsyrpBlock.param_shapes(C_, E).items()}
        sd["g1"].fill_(1.0)
        sd["g2"].fill_(1.0)
        sd["W1"] = (torch.rand(C_, C_, generator=gen, dtype=torch.float64) * 2 - 1).div(C_ ** 0.5).to(torch.float32)
        sd["Wt"] = (torch.rand(C_, E, generator=gen, dtype=torch.float64) * 2 - 1).div(E ** 0.5).to(torch.float32)
        return sd

    def __init__(self, C_: int, H: int, W: int, E: int, max_batch: int = 1, gn_eps: float = 1e-6, seed: Optional[int] = 0,
                 device: Optional[torch.device] = None):
        self._open(device)
        self.C, self.H, self.W, self.E, self.max_batch, self.gn_eps = int(C_), int(H), int(W), int(E), int(max_batch), float(gn_eps)
        with torch.cuda.device(self.device):
            rc = self.lib.loco_asyrp_create(self.device.index, self.C, self.H, self.W, self.E, self.max_batch, self.gn_eps, C.byref(self._t))
        if rc != 0:
            raise RuntimeError(f"loco_asyrp_create failed ({rc}): {self.lib.loco_asyrp_last_error(None).decode()}")
        if seed is not None:
            self.load_state_dict(self.init_params(self.C, self.E, seed))

    def _chk(self, t: torch.Tensor, what: str, shape) -> torch.Tensor:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{what}: expected a tensor")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: expected torch.float32, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"{what}: expected a tensor on {self.device}, got one on {t.device}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t.contiguous()

    def _read(self, fn: str) -> Dict[str, torch.Tensor]:
        out = {}
        with torch.cuda.device(self.device):
            for name, shape in self.param_shapes(self.C, self.E).items():
                t = torch.empty(shape, dtype=torch.float32)
                self._check(self._fn(fn)(self._t, name.encode(), C.c_void_p(t.data_ptr()), t.numel()), f"loco_asyrp_{fn}({name})")
                out[name] = t
        return out

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The ten parameters (fp32, CPU)."""
        return self._read("read_param")

    def grads(self) -> Dict[str, torch.Tensor]:
        """The accumulated gradients of the ten parameters (fp32, CPU)."""
        return self._read("read_grad")

    def forward(self, h: torch.Tensor, e: torch.Tensor, s: float = 1.0, keep_records: bool = True) -> torch.Tensor:
        """``dh [B, C, H, W]`` for ``h [B, C, H, W]`` and the time vector ``e [E]``."""
        if not isinstance(h, torch.Tensor) or h.dim() != 4:
            raise ValueError("forward: expected h [B, C, H, W]")
        h = self._chk(h, "forward: h", (h.shape[0], self.C, self.H, self.W))
        e = self._chk(e, "forward: e", (self.E,))
        dh = torch.empty_like(h)
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_asyrp_forward(self._t, _ptr(h), _ptr(e), h.shape[0], float(s), _ptr(dh), int(bool(keep_records)), _stream()),
                        "loco_asyrp_forward")
        return dh

    def backward(self, g_dh: torch.Tensor, need_g_h: bool = False) -> Optional[torch.Tensor]:
        """Adds the parameter gradients for the cotangent ``g_dh [B, C, H, W]`` of the last forward's output to the store;
        with ``need_g_h`` returns the cotangent of h."""
        if not isinstance(g_dh, torch.Tensor) or g_dh.dim() != 4:
            raise ValueError("backward: expected g_dh [B, C, H, W]")
        g_dh = self._chk(g_dh, "backward: g_dh", (g_dh.shape[0], self.C, self.H, self.W))
        g_h = torch.empty_like(g_dh) if need_g_h else None
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_asyrp_backward(self._t, _ptr(g_dh), g_dh.shape[0], _ptr(g_h), _stream()), "loco_asyrp_backward")
        return g_h

    def zero_grad(self):
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_asyrp_zero_grad(self._t, _stream()), "loco_asyrp_zero_grad")

    def adam_step(self, step: int, lr: float, beta1: float = 0.9, beta2: float = 0.999, eps: float = 1e-8):
        """One Adam step of all ten parameters from the gradient store; ``step`` counts from 1."""
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_asyrp_adam_step(self._t, float(lr), float(beta1), float(beta2), float(eps), int(step), _stream()),
                        "loco_asyrp_adam_step")

    def reset_moments(self):
        with torch.cuda.device(self.device):
            self._check(self.lib.loco_asyrp_reset_moments(self._t, _stream()), "loco_asyrp_reset_moments")
