"""ctypes binding of libxpretrain_hip.so (the C ABI in include/xpretrain_hip.h).

The library is built in-tree by ``__graft_entry__.build()`` / ``make -C xpretrain_amd/csrc``.
Loading fails loudly if it is missing -- there is no fallback path.
"""
import ctypes as C
import os
import sys

# PyTorch must be imported BEFORE the library is dlopen'ed: torch bundles its own HIP runtime
# (torch/lib/libamdhip64.so, SONAME libamdhip64.so.7).  Loaded first, it satisfies our DT_NEEDED by soname and
# the process has ONE runtime / one set of streams; loaded second, torch would bring a second runtime whose
# streams are not ordered with ours.
import torch  # noqa: F401

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libxpretrain_hip.so")

XP_BF16, XP_F32 = 0, 1
(EPI_NONE, EPI_BIAS, EPI_BIAS_QSCALE, EPI_BIAS_GELU, EPI_BIAS_RESID, EPI_GELU_BWD, EPI_PATCH, EPI_SCALE,
 EPI_BIAS_GELU_ERF, EPI_GELU_ERF_BWD) = range(10)
# XpLayerDims.act (XP_ACT_*) by config.hidden_act, and the fc1 / dpre epilogue kinds of each
ACT_QUICK_GELU, ACT_GELU = 0, 1
ACTS = {"quick_gelu": ACT_QUICK_GELU, "gelu": ACT_GELU}
EPI_ACT_FWD = (EPI_BIAS_GELU, EPI_BIAS_GELU_ERF)
EPI_ACT_BWD = (EPI_GELU_BWD, EPI_GELU_ERF_BWD)
ATTN_PROXY, ATTN_CAUSAL = 0, 1
# XpLossKind, in the header's order
(XP_LOSS_NCE, XP_LOSS_VSC_FC, XP_LOSS_DSL, XP_LOSS_VS_VC, XP_LOSS_VS_VC_FC, XP_LOSS_VSC, XP_LOSS_VIDIMG,
 XP_LOSS_VIDIMG_DIVIDE) = range(8)
# XpPairLossKind, in the header's order
XP_PAIR_NCE, XP_PAIR_TRIPLET, XP_PAIR_HARDNEG, XP_PAIR_MILNCE = range(4)
# XpOptKind, in the header's order
XP_OPT_ADAM, XP_OPT_ADAMAX = range(2)

i32, i64, f32, vp, sz = C.c_int32, C.c_int64, C.c_float, C.c_void_p, C.c_size_t


class XpGemmDesc(C.Structure):
    _fields_ = [
        ("A", vp), ("B", vp), ("C", vp),
        ("M", i64), ("N", i64), ("K", i64),
        ("lda", i64), ("ldb", i64), ("ldc", i64),
        ("a_kstrided", i32), ("b_kstrided", i32),
        ("in_dtype", i32), ("out_dtype", i32),
        ("epilogue", i32), ("split_k", i32),
        ("a_grp", i64), ("a_grp_stride", i64), ("a_off", i64),
        ("c_grp", i64), ("c_grp_stride", i64), ("c_off", i64),
        ("bias", vp),
        ("scale", f32), ("scale_cols", i64),
        ("resid", vp), ("ldr", i64),
        ("aux", vp), ("ldaux", i64),
        ("tab1", vp), ("tab2", vp), ("tab_L", i64),
        ("colsum_partials", vp),
        ("reserved0", i32), ("side_M", i32),
        ("resid_side", vp), ("out_side", vp), ("side_S", i64),
        ("a_frames", vp), ("a_frames_u8", i32), ("fr_H", i32), ("fr_W", i32), ("fr_P", i32),
        ("fr_mean", f32 * 3), ("fr_std", f32 * 3),
    ]


class XpGemmPlanInfo(C.Structure):
    _fields_ = [("family", i32), ("tile_rows", i32), ("split", i32), ("flat_split", i32), ("k_per_split", i64),
                ("tiles_m", i32), ("tiles_n", i32), ("group_n", i32), ("epi_impl", i32), ("grid", i32 * 3), ("reserved", i32),
                ("colsum_rows", i64)]


GEMM_FAMILY_256, GEMM_FAMILY_DIRECT, GEMM_FAMILY_STAGED, GEMM_FAMILY_FRAMES = range(4)
GEMM_EPI_FAST, GEMM_EPI_ROW8, GEMM_EPI_ROW4 = range(3)


class XpAttnPlanInfo(C.Structure):
    _fields_ = [("kernel", i32), ("grid", i32), ("lds_bytes", i32), ("reduce_grid", i32), ("uses_counter", i32), ("reserved", i32),
                ("part", i64 * 2), ("delta", i64 * 2), ("dq", i64 * 2), ("dkv", i64 * 2), ("counter", i64 * 2),
                ("workspace_bytes", i64), ("colsum_rows", i64)]


# XP_ATTN_KERNEL_* by value, lower case
ATTN_KERNELS = ("fwd", "fwd3", "fwd4", "bwd_pair", "bwd5", "f32")
# XP_ATTN_OPTIN_* by value: kernels only an opt-in switch plans (xp_set_attn_bwd_wide)
ATTN_OPTIN_KERNELS = {6: "bwd6"}


class XpReduceSeg(C.Structure):
    _fields_ = [("in_", vp), ("out", vp), ("stride", i64), ("nrows", i32), ("width", i32), ("accumulate", i32),
                ("reserved", i32)]


XP_REDUCE_MAX_SEGS = 16


class XpLayerDims(C.Structure):
    _fields_ = [("rows", i64), ("D", i64), ("Dff", i64), ("B", i64), ("S", i64), ("heads", i64),
                ("M", i64), ("N", i64), ("L", i64), ("attn_mode", i32), ("dtype", i32), ("q_scale", f32), ("ln_eps", f32), ("act", i32)]


class XpLayerFwd(C.Structure):
    _fields_ = ([("dims", XpLayerDims)]
                + [(n, vp) for n in ("x", "Wqkv", "Wo", "W1", "W2", "ln1_w", "ln1_b", "bqkv", "bo", "ln2_w", "ln2_b", "b1", "b2",
                                     "pad_mask", "h1", "qkv", "attn_o", "x2", "h2", "pre", "act", "x3", "mean1", "rstd1",
                                     "mean2", "rstd2", "stats", "workspace")]
                + [("workspace_bytes", sz), ("side_in", vp), ("side_out", vp), ("side_S", i64), ("side_M", i32), ("reserved", i32),
                   ("side_x2", vp)])


class XpLayerBwd(C.Structure):
    _fields_ = ([("dims", XpLayerDims)]
                + [(n, vp) for n in ("x", "h1", "qkv", "attn_o", "x2", "h2", "pre", "act", "Wqkv", "Wo", "W1", "W2", "ln1_w",
                                     "ln2_w", "mean1", "rstd1", "mean2", "rstd2", "stats", "pad_mask", "dx3", "dx",
                                     "dln1_w", "dln1_b", "dwqkv", "dbqkv", "dwo", "dbo", "dln2_w", "dln2_b", "dw1", "db1",
                                     "dw2", "db2", "workspace")]
                + [("workspace_bytes", sz), ("side_in", vp), ("side_x2", vp), ("side_S", i64), ("side_M", i32), ("reserved", i32)])


class XpLayerPooledFwd(C.Structure):
    _fields_ = ([("dims", XpLayerDims)]
                + [(n, vp) for n in ("x", "Wqkv", "Wo", "W1", "W2", "ln1_w", "ln1_b", "bqkv", "bo", "ln2_w", "ln2_b", "b1", "b2",
                                     "h1", "kv", "mean1", "rstd1", "h1p", "q", "attn_o", "x2", "h2", "pre", "act", "x3",
                                     "mean1p", "rstd1p", "mean2", "rstd2", "stats", "workspace")]
                + [("workspace_bytes", sz), ("side_in", vp), ("side_out", vp), ("side_x2", vp)])


class XpLayerPooledBwd(C.Structure):
    _fields_ = ([("dims", XpLayerDims)]
                + [(n, vp) for n in ("x", "h1", "kv", "h1p", "q", "attn_o", "x2", "h2", "pre", "act", "Wqkv", "Wo", "W1", "W2",
                                     "ln1_w", "ln2_w", "mean1", "rstd1", "mean1p", "rstd1p", "mean2", "rstd2", "stats", "dx3", "dx",
                                     "dln1_w", "dln1_b", "dwqkv", "dbqkv", "dwo", "dbo", "dln2_w", "dln2_b", "dw1", "db1",
                                     "dw2", "db2", "workspace")]
                + [("workspace_bytes", sz), ("side_in", vp), ("side_x2", vp)])


class XpAttnPooledPlanInfo(C.Structure):
    _fields_ = [("chunks", i32), ("chunk_keys", i32), ("grid", i32), ("combine_grid", i32), ("part_ml", i64 * 2),
                ("part_acc", i64 * 2), ("part_dq", i64 * 2), ("workspace_bytes", i64), ("colsum_rows", i64)]


class XpAdamTensor(C.Structure):
    _fields_ = [("p", vp), ("m", vp), ("v", vp), ("shadow", vp), ("numel", i64), ("shadow_dtype", i32), ("reserved", i32)]


class XpAdamGroup(C.Structure):
    _fields_ = [("lr", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("weight_decay", f32), ("step_size", f32)]


class XpOptGroup(C.Structure):
    _fields_ = [("lr", f32), ("beta1", f32), ("beta2", f32), ("eps", f32), ("weight_decay", f32), ("step_size", f32),
                ("bias2_sqrt", f32), ("one_minus_beta1", f32)]


class XpPairLossParams(C.Structure):
    _fields_ = [("temp", f32), ("margin", f32), ("max_violation", i32), ("order_measure", i32), ("hard_negative_num", i32),
                ("bag", i32)]


XP_OPT_CHUNK, XP_OPT_MAX_TENSORS, XP_OPT_MAX_GROUPS = 65536, 256, 16


class XpFrameSrc(C.Structure):
    _fields_ = [("src", vp), ("src_bytes", i64), ("stride_t", i64), ("stride_y", i64), ("stride_x", i64), ("stride_c", i64),
                ("T", i32), ("H", i32), ("W", i32), ("box_y", i32), ("box_x", i32), ("box_h", i32), ("box_w", i32),
                ("rh", i32), ("rw", i32), ("top", i32), ("left", i32), ("flip", i32)]


XP_FRAMES_MAX_VIDEOS, XP_FRAMES_MAX_SIZE = 32, 16384


class XpFrameTransform(C.Structure):
    _fields_ = [("src", XpFrameSrc), ("filter", i32), ("mid_h", i32), ("mid_w", i32), ("crop_y", i32), ("crop_x", i32),
                ("crop_h", i32), ("crop_w", i32), ("n_color", i32), ("color_op", i32 * 3), ("color_factor", f32 * 3)]


XP_FRAMES_TRANSFORM_MAX_VIDEOS = 24
XP_FRAMES_FILTER_BICUBIC, XP_FRAMES_FILTER_BILINEAR2 = 0, 1
# torchvision's ColorJitter op indices (1 would be contrast: not provided)
XP_FRAMES_COLOR_BRIGHTNESS, XP_FRAMES_COLOR_SATURATION, XP_FRAMES_COLOR_HUE = 0, 2, 3
XP_FRAMES_AA_MAX_TAPS = 128

# name -> (restype, argtypes); mirrors include/xpretrain_hip.h one-to-one
SIGNATURES = {
    "xp_abi_version": (i32, []),
    "xp_last_error": (C.c_char_p, []),
    "xp_gemm": (i32, [C.POINTER(XpGemmDesc), vp]),
    "xp_gemm_auto_split": (i32, [C.POINTER(XpGemmDesc)]),
    "xp_gemm_auto_split_slack": (i32, [C.POINTER(XpGemmDesc)]),
    "xp_set_cu_budget": (i32, [i32]),
    "xp_get_cu_budget": (i32, []),
    "xp_gemm_colsum_rows": (i64, [C.POINTER(XpGemmDesc)]),
    "xp_gemm_tile_rows": (i32, [C.POINTER(XpGemmDesc)]),
    "xp_colsum_partial_rows": (i64, [i64, i64]),
    "xp_colsum_partials": (i32, [vp, i64, i64, i64, i32, vp, sz, vp]),
    "xp_reduce_rows_batch_workspace_bytes": (sz, [C.POINTER(XpReduceSeg), i32]),
    "xp_reduce_rows_batch": (i32, [C.POINTER(XpReduceSeg), i32, vp, sz, vp]),
    "xp_layernorm_bwd_partial_rows": (i64, [i64]),
    "xp_layernorm_bwd_partials": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64, i32, i64, i64, i32, vp, sz, vp]),
    "xp_grad_sqnorm_partials": (i32, [vp, vp, i32, C.POINTER(vp), i32, vp, vp]),
    "xp_adamw_step": (i32, [vp, vp, i32, C.POINTER(vp), C.POINTER(C.c_uint8), i32, C.POINTER(XpAdamGroup), i32, vp, i32, f32,
                            vp, vp]),
    "xp_optim_step": (i32, [i32, vp, vp, i32, C.POINTER(vp), C.POINTER(C.c_uint8), i32, C.POINTER(XpOptGroup), i32, vp, i32, f32,
                            vp, vp]),
    "xp_splitk_reduce": (i32, [vp, vp, i64, i32, i32, vp]),
    "xp_colsum_workspace_bytes": (sz, [i64, i64]),
    "xp_colsum": (i32, [vp, i64, i64, i64, i32, vp, i32, vp, sz, vp]),
    "xp_layernorm_fwd": (i32, [vp, i64, vp, vp, vp, i64, vp, vp, i64, i64, f32, i32, vp]),
    "xp_layernorm_fwd_side": (i32, [vp, i64, vp, vp, vp, i64, vp, vp, i64, i64, f32, i32, vp, vp, i64, i32, i32, vp]),
    "xp_layernorm_bwd_workspace_bytes": (sz, [i64, i64]),
    "xp_layernorm_bwd_partials_side": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64, i32, i64, i64, i32, vp, i64, i32, i32,
                                             vp, sz, vp]),
    "xp_layernorm_bwd_side": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, vp, i32, i64, i64, i32, vp, i64, i32, i32,
                                    vp, sz, vp]),
    "xp_layernorm_bwd": (i32, [vp, i64, vp, i64, vp, vp, vp, vp, i64, vp, i64, vp, vp, i32, i64, i64, i32, vp, sz, vp]),
    "xp_attn_workspace_bytes": (sz, [i32, i64, i64, i64, i64, i64]),
    "xp_attn_fwd": (i32, [vp, i64, vp, i64, vp, vp, i32, i64, i64, i64, i64, i64, i64, i32, vp, sz, vp]),
    "xp_attn_bwd": (i32, [vp, i64, vp, vp, i64, vp, vp, vp, f32, i32, i64, i64, i64, i64, i64, i64, i32, vp, sz, vp]),
    "xp_attn_bwd2": (i32, [vp, i64, vp, vp, i64, vp, vp, vp, f32, i32, i64, i64, i64, i64, i64, i64, i32, vp, sz, vp, vp]),
    "xp_attn_bwd_colsum_rows": (i64, [i32, i64, i64, i64, i64, i64, i64, i32]),
    "xp_attn_probs": (i32, [vp, i64, vp, vp, vp, vp, i32, i64, i64, i64, i64, i64, i64, i32, vp]),
    "xp_set_attn_bwd_wide": (i32, [i32]),
    "xp_get_attn_bwd_wide": (i32, []),
    "xp_attn_pooled_workspace_bytes": (sz, [i64, i64, i64, i32]),
    "xp_attn_pooled_fwd": (i32, [vp, vp, i64, vp, vp, i64, i64, i64, i32, vp, sz, vp]),
    "xp_attn_pooled_colsum_rows": (i64, [i64, i64, i64, i32]),
    "xp_attn_pooled_colsum_rows_max": (i64, [i64, i64]),
    "xp_attn_pooled_bwd": (i32, [vp, vp, i64, vp, vp, vp, vp, i64, vp, i64, f32, i64, i64, i64, i32, vp, sz, vp, vp]),
    "xp_im2col": (i32, [vp, vp, i64, i64, i64, i64, i32, vp]),
    "xp_im2col_u8": (i32, [vp, C.POINTER(f32), C.POINTER(f32), vp, i64, i64, i64, i64, i32, vp]),
    "xp_frames_resize_norm": (i32, [C.POINTER(XpFrameSrc), i32, C.POINTER(f32), C.POINTER(f32), vp, i32, i32, vp]),
    "xp_frames_transform": (i32, [C.POINTER(XpFrameTransform), i32, C.POINTER(f32), C.POINTER(f32), vp, i32, i32, vp]),
    "xp_frames_transform_aa_workspace_bytes": (sz, [C.POINTER(XpFrameTransform), i32, i32, i32]),
    "xp_frames_transform_aa": (i32, [C.POINTER(XpFrameTransform), i32, C.POINTER(f32), C.POINTER(f32), vp, i32, i32, vp, sz, vp]),
    "xp_vip_proxy_rows": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, i32, vp]),
    "xp_vip_embed_bwd_workspace_bytes": (sz, [i64, i64, i64, i64]),
    "xp_vip_embed_bwd": (i32, [vp, vp, vp, vp, vp, i64, i64, i64, i64, i64, i32, i32, vp, sz, vp]),
    "xp_pos_resample_fwd": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "xp_pos_resample_bwd": (i32, [vp, vp, i32, i32, i32, i32, vp]),
    "xp_text_embed_fwd": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, i32, vp]),
    "xp_text_embed_bwd": (i32, [vp, vp, vp, vp, i64, i64, i64, i64, i32, i32, vp]),
    "xp_argmax_rows": (i32, [vp, vp, i64, i64, vp]),
    "xp_gather_rows": (i32, [vp, vp, vp, i64, i64, i64, i32, vp]),
    "xp_scatter_rows": (i32, [vp, vp, vp, i64, i64, i64, i32, vp]),
    "xp_l2norm_fwd": (i32, [vp, vp, vp, i64, i64, i32, vp]),
    "xp_l2norm_bwd": (i32, [vp, vp, vp, vp, i64, i64, i32, vp]),
    "xp_cast": (i32, [vp, vp, i64, i32, vp]),
    "xp_cast_back": (i32, [vp, vp, i64, i32, i32, vp]),
    "xp_nce_loss_workspace_bytes": (sz, [i64, i64]),
    "xp_nce_loss": (i32, [vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, sz, vp]),
    "xp_sim_matrix": (i32, [vp, vp, vp, i64, i64, i64, vp]),
    "xp_dsl_rerank": (i32, [vp, i64, i64, f32, i32, vp]),
    "xp_retrieval_ranks": (i32, [vp, vp, i64, i64, i32, vp, vp, vp]),
    "xp_vsc_fc_loss_workspace_bytes": (sz, [i64, i64]),
    "xp_vsc_fc_loss": (i32, [vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, vp, sz, vp]),
    "xp_contrastive_loss_workspace_bytes": (sz, [i32, i64, i64, i64]),
    "xp_contrastive_loss": (i32, [i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, i64, i64, i64, vp, sz, vp]),
    "xp_pair_loss_workspace_bytes": (sz, [i32, C.POINTER(XpPairLossParams), i64, i64]),
    "xp_pair_loss": (i32, [i32, C.POINTER(XpPairLossParams), vp, vp, vp, vp, vp, i64, i64, vp, sz, vp]),
    "xp_encoder_layer_fwd_workspace_bytes": (sz, [C.POINTER(XpLayerDims)]),
    "xp_encoder_layer_fwd": (i32, [C.POINTER(XpLayerFwd), vp]),
    "xp_encoder_layer_bwd_workspace_bytes": (sz, [C.POINTER(XpLayerDims)]),
    "xp_encoder_layer_bwd": (i32, [C.POINTER(XpLayerBwd), vp]),
    "xp_encoder_layer_pooled_fwd_workspace_bytes": (sz, [C.POINTER(XpLayerDims)]),
    "xp_encoder_layer_pooled_fwd": (i32, [C.POINTER(XpLayerPooledFwd), vp]),
    "xp_encoder_layer_pooled_bwd_workspace_bytes": (sz, [C.POINTER(XpLayerDims)]),
    "xp_encoder_layer_pooled_bwd": (i32, [C.POINTER(XpLayerPooledBwd), vp]),
    "xp_side_stream": (vp, []),
    "xp_debug_set_gemm_trace": (i32, [vp]),
    "xp_debug_gemm_timer_arm": (i32, [i64, i64, i64, i32, i32, i32, i32, i32]),
    "xp_debug_gemm_timer_read": (i32, [C.POINTER(C.c_float), i32]),
    "xp_debug_set_attn_trace": (i32, [vp]),
    "xp_debug_gemm_occupancy": (i32, [i32]),
    "xp_debug_gemm_plan": (i32, [C.POINTER(XpGemmDesc), C.POINTER(XpGemmPlanInfo)]),
    "xp_debug_attn_plan": (i32, [i32, i64, i64, i64, i64, i64, i64, i32, i32, i32, i32, C.POINTER(XpAttnPlanInfo)]),
    "xp_debug_attn_pooled_plan": (i32, [i64, i64, i64, i32, i32, i32, C.POINTER(XpAttnPooledPlanInfo)]),
    "xp_probe_mfma_bf16": (i32, [vp, vp, vp, vp]),
    "xp_probe_mfma_f32": (i32, [vp, vp, vp, vp]),
    "xp_probe_tr16": (i32, [vp, vp, vp, vp]),
    "xp_probe_stream_copy": (i32, [vp, vp, i64, i32, i32, vp]),
    "xp_probe_stream_copy_fat": (i32, [vp, vp, i64, i32, i32, vp]),
    "xp_probe_pk_f32": (i32, [vp, i32, i32, C.c_uint32, vp]),
}

_lib = None


def lib():
    """The loaded library (raises RuntimeError if it has not been built)."""
    global _lib
    if _lib is None:
        if not os.path.isfile(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `make -C xpretrain_amd/csrc`.  xpretrain_amd has no CPU / eager fallback.")
        l = C.CDLL(LIB_PATH)
        missing = [n for n in SIGNATURES if not hasattr(l, n)]
        if missing:
            raise RuntimeError(f"{LIB_PATH} is missing C-ABI symbols: {missing}")
        for n, (res, args) in SIGNATURES.items():
            fn = getattr(l, n)
            fn.restype, fn.argtypes = res, args
        if l.xp_abi_version() != 1:
            raise RuntimeError(f"ABI version mismatch: library {l.xp_abi_version()} != binding 1")
        _lib = l
    return _lib


# XPRETRAIN_DEBUG=flag[,flag...]: the debug / test facilities (csrc/common.cpp lists the library's flags).  Python side:
#   sync      synchronise and check the device after every library call (errors then surface at the call that caused them)
#   op_by_op  encoder layers as separate operator calls instead of one C-ABI call per pass (the fingerprinting / calibration tools)
#   no_comm   GradBucketReducer packs and tracks its buckets but skips the all-reduce calls (cost attribution on one GPU)
DEBUG = frozenset(f for f in os.environ.get("XPRETRAIN_DEBUG", "").split(",") if f)
DEBUG_SYNC = "sync" in DEBUG


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed (rc={rc}): {lib().xp_last_error().decode()}")
    if DEBUG_SYNC:      # debugging aid: localise an asynchronous fault to the call that caused it
        sys.stderr.write(f"[xp] {what} ... "); sys.stderr.flush()
        torch.cuda.synchronize()
        sys.stderr.write("ok\n"); sys.stderr.flush()
