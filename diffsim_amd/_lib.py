"""ctypes binding of libdiffsim_amd.so (the C ABI declared in include/diffsim_amd.h).

There is NO fallback: if the shared library is missing or a call fails, an exception is raised.
"""
from __future__ import annotations

import ctypes as C
import os

# PyTorch-ROCm owns the device memory and streams this library works on, and its wheel bundles its
# own HIP runtime.  Import it BEFORE dlopen()ing libdiffsim_amd.so so the library's libamdhip64
# dependency binds to the runtime torch already loaded; loaded the other way round the process
# ends up with two HIP runtimes and the second one sees no device.
import torch  # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libdiffsim_amd.so")

DSIM_F32, DSIM_BF16, DSIM_F16 = 0, 1, 2
TAP = {"down_blocks": 0, "mid_blocks": 1, "up_blocks": 2}
MAX_LEVELS = 4
FUSE_FF, FUSE_LNPROJ, FUSE_TAPQKV, FUSE_ALL = 1, 2, 4, 7        # dsim_unet_set_fusion bits


class DsimError(RuntimeError):
    pass


class UNetCfgC(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("n_levels", C.c_int32),
        ("block_out_channels", C.c_int32 * MAX_LEVELS),
        ("down_has_attn", C.c_int32 * MAX_LEVELS), ("up_has_attn", C.c_int32 * MAX_LEVELS),
        ("layers_per_block", C.c_int32), ("num_heads", C.c_int32),
        ("cross_attention_dim", C.c_int32), ("norm_num_groups", C.c_int32),
        ("norm_eps", C.c_float), ("sample_size", C.c_int32), ("ctx_len", C.c_int32),
        ("compute_dtype", C.c_int32), ("tap_block", C.c_int32), ("tap_layer", C.c_int32),
        ("tap_attn", C.c_int32), ("tap_tfm", C.c_int32),
        ("heads_per_level", C.c_int32 * MAX_LEVELS), ("depth_per_level", C.c_int32 * MAX_LEVELS),
        ("addition_embed", C.c_int32), ("addition_time_embed_dim", C.c_int32), ("pooled_dim", C.c_int32),
    ]


class VAECfgC(C.Structure):
    _fields_ = [
        ("in_channels", C.c_int32), ("latent_channels", C.c_int32), ("n_levels", C.c_int32),
        ("block_out_channels", C.c_int32 * MAX_LEVELS), ("layers_per_block", C.c_int32),
        ("norm_num_groups", C.c_int32), ("compute_dtype", C.c_int32),
    ]


class GemmOpC(C.Structure):
    """dsim_gemm_op (include/diffsim_amd.h)"""
    _fields_ = [
        ("mode", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("stride", C.c_int32), ("ups", C.c_int32), ("pad", C.c_int32),
        ("A0", C.c_void_p), ("C0", C.c_int32), ("A1", C.c_void_p), ("C1", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
        ("w", C.c_void_p), ("wb_rows", C.c_int32), ("wb_stride", C.c_uint32),
        ("bias", C.c_void_p), ("bias2", C.c_void_p), ("rows_per_batch", C.c_int32),
        ("act", C.c_int32), ("gate", C.c_void_p), ("gate2", C.c_void_p),
        ("epi", C.c_int32),
        ("residual", C.c_void_p), ("out", C.c_void_p), ("ldo", C.c_int32),
        ("out_split", C.c_int32), ("out_split_stride", C.c_int64),
        ("force_big", C.c_int32),
        ("gn_part", C.c_void_p), ("gn_hw", C.c_int32),
        ("dtype", C.c_int32),
    ]


class GemmLaunchC(C.Structure):
    """dsim_gemm_launch (include/diffsim_amd.h)"""
    _fields_ = [(n, C.c_int32) for n in ("bm", "bn", "kind", "geglu", "ek", "small")] + [("family", C.c_char * 128)]


class AttnLaunchC(C.Structure):
    """dsim_attn_launch (include/diffsim_amd.h)"""
    _fields_ = [(n, C.c_int32) for n in ("kind", "D", "dtype", "k80", "qit", "grid")] + [("family", C.c_char * 64)]


class GnPlanC(C.Structure):
    """dsim_gn_plan (include/diffsim_amd.h)"""
    _fields_ = [(n, C.c_int32) for n in ("form", "NS", "UNR", "CS", "tpr", "R", "chunks", "rb")]


class LnPlanC(C.Structure):
    """dsim_ln_plan (include/diffsim_amd.h)"""
    _fields_ = [(n, C.c_int32) for n in ("form", "LPR", "CPL", "passes", "MAXS", "RPW", "blocks")]


GN_FORMS = ("onepass", "twopass", "pre")     # dsim_gn_plan.form, by index
LN_FORMS = ("rows", "wave")                  # dsim_ln_plan.form, by index

# dsim_attn_kind, by index
ATTN_KINDS = ("P160", "Short", "ShortK80", "Long", "Q2", "Q2Fast", "Fast", "Exact", "FP8")


class TapC(C.Structure):
    """dsim_tap (include/diffsim_amd.h): one tap of a sweep, the dsim_unet_cfg fields of the same names"""
    _fields_ = [(n, C.c_int32) for n in ("block", "layer", "attn", "tfm")]


class DiTCfgC(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("input_size", "patch_size", "in_channels", "hidden_size", "depth", "num_heads",
                                          "mlp_ratio", "num_classes", "freq_dim", "compute_dtype", "tap_layer")]


class ViTCfgC(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("image_size", "patch_size", "hidden_size", "depth", "num_heads", "mlp_dim", "act", "pre_norm",
                                           "patch_bias", "layer_scale", "tap_input")] +
                [("ln_eps", C.c_float), ("compute_dtype", C.c_int32), ("tap_layer", C.c_int32)])


VGG_MAX_PLAN = 32        # DSIM_VGG_MAX_PLAN


class VGGCfgC(C.Structure):
    _fields_ = [("in_channels", C.c_int32), ("plan", C.c_int32 * VGG_MAX_PLAN), ("compute_dtype", C.c_int32)]


class ResizeImageC(C.Structure):
    """dsim_resize_image (include/diffsim_amd.h)"""
    _fields_ = [("src_offset", C.c_int64), ("w", C.c_int32), ("h", C.c_int32), ("h_table", C.c_int32), ("v_table", C.c_int32),
                ("y_first", C.c_int32), ("rows", C.c_int32), ("temp_offset", C.c_int64)]


class ResizeTableC(C.Structure):
    """dsim_resize_table (include/diffsim_amd.h)"""
    _fields_ = [("offset", C.c_int64), ("in_size", C.c_int32), ("out_size", C.c_int32), ("ksize", C.c_int32), ("reserved", C.c_int32)]


VIT_ACT = {"gelu": 0, "quick_gelu": 1}          # DSIM_VIT_ACT_*
VIT_TAP_INPUT = {"norm1": 0, "block": 1}        # dsim_vit_cfg.tap_input

# every symbol include/diffsim_amd.h declares: (restype, argtypes)
_vp, _i, _f, _sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
ABI_VERSION = 7          # include/diffsim_amd.h DSIM_ABI_VERSION (tests/test_host.py checks the header against it)
SYMBOLS = {
    "dsim_version": (_i, []),
    "dsim_strerror": (C.c_char_p, [_i]),
    "dsim_device_count": (_i, []),
    "dsim_unet_create": (_i, [C.POINTER(UNetCfgC), C.POINTER(_vp)]),
    "dsim_unet_destroy": (None, [_vp]),
    "dsim_unet_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i]),
    "dsim_unet_finalize": (_i, [_vp, _vp]),
    "dsim_unet_set_timestep": (_i, [_vp, _i, _vp]),
    "dsim_unet_set_conditioning": (_i, [_vp, _i, _vp, _vp, _vp]),
    "dsim_unet_workspace_bytes": (_sz, [_vp, _i]),
    "dsim_unet_qkv": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_unet_tap_shape": (_i, [_vp, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dsim_unet_set_tap": (_i, [_vp, _i, _i, _i, _i]),
    "dsim_unet_tap_shape_at": (_i, [_vp, C.POINTER(TapC), C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dsim_unet_taps_workspace_bytes": (_sz, [_vp, _i, _i, C.POINTER(TapC)]),
    "dsim_unet_qkv_taps": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i, _i, C.POINTER(TapC), C.POINTER(_vp), C.POINTER(_vp),
                                C.POINTER(_vp), _vp, _sz, _vp]),
    "dsim_unet_ctx_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dsim_unet_taps_ctx_workspace_bytes": (_sz, [_vp, _i, _i, _i, C.POINTER(TapC)]),
    "dsim_unet_qkv_ctx": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_unet_qkv_taps_ctx": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i, _vp, _i, _i, C.POINTER(TapC), C.POINTER(_vp), C.POINTER(_vp),
                                    C.POINTER(_vp), _vp, _sz, _vp]),
    "dsim_unet_set_sample_size": (_i, [_vp, _i]),
    "dsim_unet_set_cfg_dedup": (_i, [_vp, _i]),
    "dsim_unet_set_fusion": (_i, [_vp, _i]),
    "dsim_unet_profile": (_i, [_vp, _i]),
    "dsim_unet_profile_count": (_i, [_vp]),
    "dsim_unet_profile_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                   C.POINTER(C.c_double)]),
    "dsim_vae_create": (_i, [C.POINTER(VAECfgC), C.POINTER(_vp)]),
    "dsim_vae_destroy": (None, [_vp]),
    "dsim_vae_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i]),
    "dsim_vae_finalize": (_i, [_vp, _vp]),
    "dsim_vae_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dsim_vae_encode": (_i, [_vp, _vp, _i, _i, _vp, _vp, _sz, _vp]),
    "dsim_vae_profile": (_i, [_vp, _i]),
    "dsim_vae_profile_count": (_i, [_vp]),
    "dsim_vae_profile_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsim_image_preprocess": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
    "dsim_latent_sample": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _f, _i, _vp]),
    "dsim_resize_u8_workspace_bytes": (_sz, [C.POINTER(ResizeImageC), _i, C.POINTER(ResizeTableC), _i, _sz, _i, _i, _i, _i, _i, _i, _sz]),
    "dsim_resize_u8": (_i, [_vp, _sz, C.POINTER(ResizeImageC), _i, _vp, _sz, C.POINTER(ResizeTableC), _i, _i, _i, _i, _i, _i, _i, _vp,
                            _vp, _sz, _vp]),
    "dsim_dit_create": (_i, [C.POINTER(DiTCfgC), C.POINTER(_vp)]),
    "dsim_dit_destroy": (None, [_vp]),
    "dsim_dit_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i]),
    "dsim_dit_finalize": (_i, [_vp, _vp]),
    "dsim_dit_set_conditioning": (_i, [_vp, _i, _i, _i, _vp]),
    "dsim_dit_set_attention": (_i, [_vp, _i]),
    "dsim_dit_set_tap": (_i, [_vp, _i]),
    "dsim_dit_profile": (_i, [_vp, _i]),
    "dsim_dit_profile_count": (_i, [_vp]),
    "dsim_dit_profile_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsim_dit_workspace_bytes": (_sz, [_vp, _i]),
    "dsim_dit_qkv": (_i, [_vp, _vp, _vp, _f, _f, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_dit_taps_workspace_bytes": (_sz, [_vp, _i, _i, C.POINTER(_i)]),
    "dsim_dit_qkv_taps": (_i, [_vp, _vp, _vp, _f, _f, _i, _i, C.POINTER(_i), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp,
                               _sz, _vp]),
    "dsim_vit_create": (_i, [C.POINTER(ViTCfgC), C.POINTER(_vp)]),
    "dsim_vit_destroy": (None, [_vp]),
    "dsim_vit_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i]),
    "dsim_vit_finalize": (_i, [_vp, _vp]),
    "dsim_vit_set_tap": (_i, [_vp, _i]),
    "dsim_vit_profile": (_i, [_vp, _i]),
    "dsim_vit_profile_count": (_i, [_vp]),
    "dsim_vit_profile_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsim_vit_workspace_bytes": (_sz, [_vp, _i]),
    "dsim_vit_qkv": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_vit_taps_workspace_bytes": (_sz, [_vp, _i, _i, C.POINTER(_i)]),
    "dsim_vit_qkv_taps": (_i, [_vp, _vp, _i, _i, C.POINTER(_i), C.POINTER(_vp), C.POINTER(_vp), C.POINTER(_vp), _vp, _sz, _vp]),
    "dsim_vgg_create": (_i, [C.POINTER(VGGCfgC), C.POINTER(_vp)]),
    "dsim_vgg_destroy": (None, [_vp]),
    "dsim_vgg_load_weight": (_i, [_vp, C.c_char_p, _vp, _i, C.POINTER(C.c_int64), _i]),
    "dsim_vgg_finalize": (_i, [_vp, _vp]),
    "dsim_vgg_profile": (_i, [_vp, _i]),
    "dsim_vgg_profile_count": (_i, [_vp]),
    "dsim_vgg_profile_get": (_i, [_vp, _i, C.c_char_p, _i, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "dsim_vgg_out_shape": (_i, [_vp, _i, _i, C.POINTER(_i), C.POINTER(_i), C.POINTER(_i)]),
    "dsim_vgg_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "dsim_vgg_features": (_i, [_vp, _vp, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "dsim_op_relu": (_i, [_vp, _sz, _i, _vp]),
    "dsim_op_relu_pool2": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dsim_gram_rows_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_gram_rows": (_i, [_vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_proj_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_score_proj": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_attn_features_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i, _i]),
    "dsim_attn_features": (_i, [_vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_feature_pair_score_workspace_bytes": (_sz, [_i, _i, _i]),
    "dsim_feature_pair_score": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_feature_matrix_workspace_bytes": (_sz, [_i, _i, _i, _i]),
    "dsim_feature_matrix": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_feature_matrix_chunked_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dsim_feature_matrix_chunked": (_i, [_vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dsim_pair_score": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_status": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_score_matrix_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_score_matrix": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_maps_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dsim_pair_score_maps": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_align_workspace_bytes": (_sz, [_i, _i, _i, _i, _i]),
    "dsim_pair_align": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_unet_text_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dsim_unet_qkv_text": (_i, [_vp, _vp, _vp, _f, _f, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_text_attention_workspace_bytes": (_sz, [_i, _i, _i]),
    "dsim_text_attention": (_i, [_vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp, _i, _f, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_regions_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_score_regions": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_weights_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_score_weights": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_maps_regions_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_score_maps_regions": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_align_regions_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_align_regions": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_score_matrix_regions_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_score_matrix_regions": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_score_maps_weights_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_score_maps_weights": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_align_weights_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_align_weights": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_pair_region_transfer_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i]),
    "dsim_pair_region_transfer": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_score_matrix_weights_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_score_matrix_weights": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_region_transfer_matrix_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_region_transfer_matrix": (_i, [_vp, _vp, _vp, _i, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _sz, _vp]),
    "dsim_score_matrix_cell_regions_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_score_matrix_cell_regions": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_score_matrix_cell_weights_workspace_bytes": (_sz, [_i, _i, _i, _i, _i, _i, _i]),
    "dsim_score_matrix_cell_weights": (_i, [_vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _sz, _vp]),
    "dsim_op_linear": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_conv3x3": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_groupnorm": (_i, [_vp, _i, _vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _vp]),
    "dsim_op_layernorm": (_i, [_vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp]),
    "dsim_op_layernorm_mod": (_i, [_vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "dsim_groupnorm_plan": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(GnPlanC)]),
    "dsim_layernorm_plan": (_i, [_i, _i, _i, _i, C.POINTER(LnPlanC)]),
    "dsim_op_attention": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_attention_fp8": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_ff_fused": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _vp]),
    "dsim_op_ln_linear": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _vp]),
    "dsim_op_ff_fused_dt": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _f, _i, _vp]),
    "dsim_op_ln_linear_dt": (_i, [_vp, _vp, _vp, _vp, _vp, _i, _i, _i, _f, _i, _vp]),
    "dsim_op_gn_linear_dt": (_i, [_vp, _vp, _vp, _i, _f, _vp, _vp, _vp, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_gemm": (_i, [C.POINTER(GemmOpC), C.POINTER(GemmLaunchC), _vp]),
    "dsim_op_groupnorm_pre": (_i, [_vp, _i, _vp, _vp, _vp, _i, _i, _i, _f, _i, _i, _vp, _i, _vp]),
    "dsim_op_attention_ex": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(AttnLaunchC), _vp]),
    "dsim_attention_plan": (_i, [_vp, _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(_i)]),
    "dsim_op_softmax_rows": (_i, [_vp, _vp, _i, _i, _f, _i, _vp]),
    "dsim_op_conv_in": (_i, [_vp, _vp, _f, _f, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp, _i, C.POINTER(_i), _vp]),
    "dsim_op_timestep_sincos": (_i, [_vp, _i, _i, _vp]),
    "dsim_op_sincos_values": (_i, [_vp, _i, _vp, _i, _vp]),
    "dsim_op_gemv_f32": (_i, [_vp, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp]),
    "dsim_op_pack": (_i, [_i, _vp, _i, _vp, _i, _i, _i, _i, _vp]),
    "dsim_op_dup_batch": (_i, [_vp, _vp, _i, _sz, _vp]),
    "dsim_op_resize_nearest": (_i, [_vp, _vp, _i, _i, _i, _i, _i, _sz, _vp]),
    "dsim_op_gather_ctx": (_i, [_vp, _i, _vp, _vp, _i, _i, _sz, _vp]),
    "dsim_op_patch_embed": (_i, [_vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _i, _i, _i, _i, _i, _i, _vp]),
    "dsim_op_fold_quant": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "dsim_op_to_nchw_f32": (_i, [_vp, _vp, _i, _i, _i, _i, _vp]),
}

CONV_IN_KERNELS = (None, "generic", "eight", "rows")      # dsim_conv_in_kernel, by value (0: the executors' choice, as `force`)
PACK_KINDS = ("linear", "conv3", "conv_in", "vector")    # dsim_pack_kind, by value

_lib = None


def lib() -> C.CDLL:
    """Load the HIP extension; raise loudly if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise DsimError(
                f"{LIB_PATH} not found: the HIP extension is not built "
                "(run `python -m diffsim_amd.build`); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            fn = getattr(L, name)          # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if L.dsim_version() != ABI_VERSION:
            raise DsimError(f"ABI version mismatch: library {L.dsim_version()}, bindings {ABI_VERSION}")
        _lib = L
    return _lib


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = lib().dsim_strerror(status).decode()
        raise DsimError(f"{what}: {msg} (status {status})")
