"""ctypes binding of libctdet_hip.so (the C ABI in include/ctdet_hip.h).

The product path has no CPU fallback: if the shared library is missing or a call fails, a
RuntimeError is raised (the reference raises RuntimeError from TORCH_CHECK/AT_ERROR the same way,
detectron2/layers/csrc/deformable/deform_conv.h:282-311).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libctdet_hip.so")

F16, F32, U8, F16X3 = 0, 1, 2, 3
ACT_NONE, ACT_RELU, ACT_SIGMOID_CLAMP = 0, 1, 2
# mask mode of the DCN entry points (enum ctdet_dcn_mask; the argument named mask_is_prob): mask logits, probabilities, no mask
DCN_MASK_LOGIT, DCN_MASK_PROB, DCN_MASK_NONE = 0, 1, 2
# enum ctdet_sgd_clip / ctdet_grad_norm
CLIP_NONE, CLIP_VALUE, CLIP_NORM = 0, 1, 2
NORM_L1, NORM_L2, NORM_INF = 1, 2, 3


class ConvDesc(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "B", "H", "W", "Cin", "in_stride", "Cout", "Ho", "Wo", "out_stride",
        "R", "S", "stride", "pad", "dil", "Kpad", "Cout_pad",
        "compute_dtype", "out_dtype", "act", "res_stride")] + [("clamp_lo", C.c_float), ("clamp_hi", C.c_float), ("korder", C.c_int32), ("in_dil", C.c_int32)]


_vp, _i32, _i64, _f32, _f64, _sz = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t
# name -> (restype, argtypes); must list every symbol declared in include/ctdet_hip.h
SIGNATURES = {
    "ctdet_last_error": (C.c_char_p, []),
    "ctdet_abi_version": (_i32, []),
    "ctdet_conv_cout_tile": (_i32, [_i32]),
    "ctdet_set_label_mode": (_i32, [_i32]),
    "ctdet_last_kernel_label": (C.c_char_p, []),
    "ctdet_conv_pair_supported": (_i32, [C.POINTER(ConvDesc), _vp]),
    "ctdet_head_fused_supported": (_i32, [_i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_conv2d_fwd": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_conv1x1_cat_fwd": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_dcnv2_fwd": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_dcnv2_offset_supported": (_i32, [C.POINTER(ConvDesc)]),
    "ctdet_dcnv2_cols_supported": (_i32, [C.POINTER(ConvDesc), _vp, _vp]),
    "ctdet_dcnv2_fwd_cols": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_dcnv2_offset_fwd": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_dcnv2_offset_finite_fwd": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_preprocess": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _vp]),
    "ctdet_preprocess_mirror": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i64, _vp, _vp, _i32, _i32, _i32, _vp]),
    "ctdet_head_fused_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp]),
    "ctdet_head_fused_x3_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_head_sparse_x3_fwd": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _vp, _vp, _vp]),
    "ctdet_dla_base_fwd": (_i32, [_vp] * 14),
    "ctdet_dla_base_x3_fwd": (_i32, [_vp] * 14),
    "ctdet_dla_base_mirror_fwd": (_i32, [_vp, _i32] + [_vp] * 13),
    "ctdet_dla_base_x3_mirror_fwd": (_i32, [_vp, _i32] + [_vp] * 13),
    "ctdet_maxpool2x2": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_maxpool3x3s2": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_maxpool3x3s2_ceil": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_global_avgpool": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ctdet_ese_scale": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_pack_weights": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_pack_weights_batch": (_i32, [_vp, _i32, _i32, _vp]),
    "ctdet_split_weights": (_i32, [_vp, _vp, _i64, _vp]),
    "ctdet_pack_weights_x3": (_i32, [_vp, _vp, _vp] + [_i32] * 10 + [_vp]),
    "ctdet_pack_weights_x3_batch": (_i32, [_vp, _i32, _i32, _vp]),
    "ctdet_dwconvT_add": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dwconv3x3_fwd": (_i32, [_vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dwconv3x3_wgrad_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ctdet_dwconv3x3_wgrad": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_decode_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "ctdet_decode": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_decode_flip": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_postprocess": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_postprocess_affine": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_decode_status": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_gaussian_targets": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_gaussian_radius": (_i32, [_vp, _i32, _vp, _vp, _vp]),
    "ctdet_focal_loss_workspace_bytes": (_sz, [_i64]),
    "ctdet_focal_loss": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_reg_l1_loss": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _i32, _vp]),
    "ctdet_chan_workspace_bytes": (_sz, [_i32]),
    "ctdet_bn_train_fwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _vp,
                                   _vp, _vp, _vp, _i32, _i32, _vp]),
    "ctdet_bn_train_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _i32,
                                   _vp, _vp, _f32, _vp, _i32, _vp]),
    "ctdet_bn_local_stats": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "ctdet_bn_sync_fwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _f32, _f32, _vp, _vp, _vp,
                                  _vp, _vp, _vp, _i32, _i32, _vp]),
    "ctdet_bn_local_grad_sums": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                         _f32, _vp, _i32, _vp]),
    "ctdet_bn_sync_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _i32,
                                  _vp, _i32, _i32, _vp]),
    "ctdet_conv_wgrad": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _f32, _vp]),
    "ctdet_conv_wgrad_oihw": (_i32, [C.POINTER(ConvDesc), _vp, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_grad_scatter_oihw": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _vp]),
    "ctdet_depth_to_space2": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_maxpool3x3s2_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_finite_flag": (_i32, [_vp, _i64, _i32, _i32, _vp, _vp]),
    "ctdet_ese_dot": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "ctdet_ese_bwd": (_i32, [_vp, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_maxpool2x2_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dwconvT_bwd": (_i32, [_vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dcn_cols": (_i32, [_vp, _i32, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dcn_col2im_coord": (_i32, [_vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_dcn_col2im_fused": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "ctdet_sgd_momentum": (_i32, [_vp, _vp, _vp, _i64, _vp, _f32, _f32, _i32, _vp]),
    "ctdet_sgd_momentum_runs": (_i32, [_vp, _vp, _vp, C.c_int64, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _vp]),
    "ctdet_grad_chunk_norms": (_i32, [_vp, _i64, _vp, _vp, _i32, _i32, _vp, _vp]),
    "ctdet_grad_clip_coefs": (_i32, [_vp, _vp, _i32, _i32, _i32, _f32, _vp, _vp, _vp]),
    "ctdet_sgd_momentum_runs_clip": (_i32, [_vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _f32, _i32, _i32, _i32, _f32, _vp,
                                             _vp]),
    "ctdet_adam_advance": (_i32, [_vp, _vp, _f64, _f64, _vp]),
    "ctdet_adam_runs": (_i32, [_vp, _vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _vp, _f64, _f64, _f64, _i32, _i32, _i32,
                               _f32, _vp, _vp]),
    "ctdet_ema_advance": (_i32, [_vp, _vp, _f64, _i32, _vp]),
    "ctdet_ema_lerp_segments": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp, _vp]),
    "ctdet_ema_swap_segments": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp]),
    "ctdet_precise_bn_merge_segments": (_i32, [_vp, _vp, _vp, _vp, _i32, _i64, _vp, _i64, _vp]),
    "ctdet_precise_bn_finish_segments": (_i32, [_vp, _vp, _vp, _i32, _i64, _vp, _i32, _i64, _vp]),
    "ctdet_cocoeval_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "ctdet_cocoeval_iou": (_i32, [_vp, _i32, _vp, _vp, _i32, _vp, _vp]),
    "ctdet_cocoeval_match": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _i32, _i32,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_cocoeval_accumulate": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp,
                                         _vp, _vp, _vp, _vp]),
    "ctdet_resize_bilinear_u8": (_i32, [_vp, _vp, _vp]),
    "ctdet_resize_bilinear_u8_batch": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "ctdet_warp_affine_u8_batch": (_i32, [_vp, _i32, _i32, _vp, _vp]),
    "ctdet_byte_sum_u8_batch": (_i32, [_vp, _i32, _vp, _i32, _vp]),
    "ctdet_colour_jitter_u8_batch": (_i32, [_vp, _i32, _i32, _vp, _i32, _vp]),
    "ctdet_soft_nms_merge": (_i32, [_vp, _i32, _i32, _i32, C.c_float, C.c_float, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_set_tuning_flags": (_i32, [C.c_uint32]),
    "ctdet_get_tuning_flags": (C.c_uint32, []),
    "ctdet_comm_unique_id": (_i32, [_vp]),
    "ctdet_comm_init": (_i32, [_vp, _i32, _i32, C.POINTER(C.c_void_p)]),
    "ctdet_allreduce_bucket": (_i32, [_vp, _vp, _i64, _vp]),
    "ctdet_bcast": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "ctdet_comm_destroy": (_i32, [_vp]),
}

_loaded = {}   # id(signature table) -> CDLL: one library per table, loaded once


def _load(path, signatures, after_main):
    """CDLL of `path` with every signature bound, loaded once; raises if it has not been built (no fallback).  after_main:
    a library that links against libctdet_hip.so, which is loaded first; the main library itself takes CTDET_TUNE_FLAGS"""
    l = _loaded.get(id(signatures))
    if l is None:
        if after_main:
            lib()
        if not os.path.exists(path):
            raise RuntimeError(
                f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (or `make -C "
                f"detectron2-centernet_amd/csrc`). There is no CPU fallback{'' if after_main else ' for the HIP path'}.")
        l = C.CDLL(path)
        for name, (res, args) in signatures.items():
            fn = getattr(l, name)  # AttributeError if the .so is stale
            fn.restype = res
            fn.argtypes = args
        _loaded[id(signatures)] = l
        if not after_main and os.environ.get("CTDET_TUNE_FLAGS"):      # kernel-selection bits for a whole process (A/B runs of bench.py's ranks)
            l.ctdet_set_tuning_flags(int(os.environ["CTDET_TUNE_FLAGS"], 0))
    return l


def lib():
    """Loads libctdet_hip.so once; raises if it has not been built (no fallback)."""
    return _load(LIB_PATH, SIGNATURES, False)


# libctdet_metrics.so (include/ctdet_metrics.h): the training loop's metric push, loaded when a metric ring is first built
METRICS_LIB_PATH = os.path.join(_HERE, "lib", "libctdet_metrics.so")
METRICS_SIGNATURES = {
    "ctdet_metric_push": (_i32, [_vp, _i32, _f32, _vp, _i32, _i32, _vp, _i64, _vp]),
}


def metrics_lib():
    """Loads libctdet_metrics.so once (after libctdet_hip.so, which it links against); raises if it has not been built"""
    return _load(METRICS_LIB_PATH, METRICS_SIGNATURES, True)


# libctdet_voceval.so (include/ctdet_voceval.h): the Pascal VOC scorer, loaded when VOCevalHIP first scores
VOCEVAL_LIB_PATH = os.path.join(_HERE, "lib", "libctdet_voceval.so")
VOCEVAL_SIGNATURES = {
    "ctdet_voceval_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32]),
    "ctdet_voceval_match": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp, _vp,
                                   _vp, _vp]),
    "ctdet_voceval_ap": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
}


def voceval_lib():
    """Loads libctdet_voceval.so once (after libctdet_hip.so, which it links against); raises if it has not been built"""
    return _load(VOCEVAL_LIB_PATH, VOCEVAL_SIGNATURES, True)


# libctdet_lviseval.so (include/ctdet_lviseval.h): the LVIS scorer, loaded when LVISevalHIP first scores
LVISEVAL_LIB_PATH = os.path.join(_HERE, "lib", "libctdet_lviseval.so")
LVISEVAL_SIGNATURES = {
    "ctdet_lviseval_workspace_bytes": (_sz, [_i64, _i64, _i32, _i32, _i32, _i32]),
    "ctdet_lviseval_match": (_i32, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ctdet_lviseval_accumulate": (_i32, [_vp, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
}


def lviseval_lib():
    """Loads libctdet_lviseval.so once (after libctdet_hip.so, which it links against); raises if it has not been built"""
    return _load(LVISEVAL_LIB_PATH, LVISEVAL_SIGNATURES, True)


def check(rc, what):
    if rc != 0:
        msg = lib().ctdet_last_error()
        raise RuntimeError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")


class SoftNmsPass(C.Structure):
    """mirrors ctdet_softnms_pass"""
    _fields_ = [("boxes", C.c_void_p), ("scores", C.c_void_p), ("classes", C.c_void_p), ("counts", C.c_void_p),
                ("K", C.c_int32), ("pad_", C.c_int32)]


class PackDesc(C.Structure):
    """mirrors ctdet_pack_desc"""
    _fields_ = [("w", C.c_void_p), ("packed", C.c_void_p)] + [(n, C.c_int32) for n in (
        "O", "I", "R", "S", "chans_pad", "rows_pad", "Kpad", "korder", "transposed", "blk0")]


class Pack3Desc(C.Structure):
    """mirrors ctdet_pack3_desc"""
    _fields_ = [("w", C.c_void_p), ("packed", C.c_void_p), ("scale_out", C.c_void_p)] + [(n, C.c_int32) for n in (
        "O", "I", "R", "S", "chans_pad", "rows_pad", "Kpad", "layout", "transposed", "scale_n", "blk0", "pad_")]


class DlaBaseDesc(C.Structure):
    """mirrors ctdet_dla_base_desc"""
    _fields_ = [("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Hp", C.c_int32), ("Wp", C.c_int32),
                ("img_dtype", C.c_int32), ("img_batch_stride", C.c_int64), ("mean", C.c_float * 3), ("std", C.c_float * 3),
                ("out_stride", C.c_int32), ("pool_stride", C.c_int32)]


class ResizeDesc(C.Structure):
    """mirrors ctdet_resize_desc (ops.RESIZE_DESC_DTYPE is the same layout as a numpy record)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(n, C.c_int64) for n in (
        "src_row", "src_pix", "src_chan", "dst_row", "dst_pix", "dst_chan")] + [(n, C.c_int32) for n in (
        "H", "W", "new_h", "new_w", "hb", "hc", "vb", "vc", "kh", "kv", "blk0", "pad_")]


class WarpDesc(C.Structure):
    """mirrors ctdet_warp_desc (ops.WARP_DESC_DTYPE is the same layout as a numpy record)"""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p)] + [(n, C.c_int64) for n in (
        "src_row", "src_pix", "src_chan", "dst_row", "dst_pix", "dst_chan")] + [(n, C.c_int32) for n in (
        "H", "W", "out_h", "out_w", "ax", "bx", "x0", "y0", "blk0", "pad_")]


class JitterDesc(C.Structure):
    """mirrors ctdet_jitter_desc (ops.JITTER_DESC_DTYPE is the same layout as a numpy record)"""
    _fields_ = [("img", C.c_void_p)] + [(n, C.c_int64) for n in ("row", "pix", "chan")] + [(n, C.c_int32) for n in (
        "h", "w", "blk0", "sum_slot")] + [("on", C.c_int32 * 4)] + [(n, C.c_double * 2) for n in (
        "contrast", "brightness", "saturation")] + [("lighting", C.c_double * 3)]


class HeadDesc(C.Structure):
    """mirrors ctdet_head_desc"""
    _fields_ = [("nheads", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32),
                ("in_stride", C.c_int32), ("w2", C.c_void_p * 4), ("b2", C.c_void_p * 4), ("y", C.c_void_p * 4),
                ("y_stride", C.c_int32 * 4), ("cout", C.c_int32 * 4), ("act", C.c_int32 * 4),
                ("clamp_lo", C.c_float), ("clamp_hi", C.c_float)]


TUNE_NO_HALO, TUNE_NO_WIN, TUNE_DCN_MIXED, TUNE_NO_WGRAD_WINDOW, TUNE_NO_COL2IM_WINDOW, TUNE_NO_F32_DCN_WINDOW, TUNE_DCN_WINDOW_V1, TUNE_NO_SMALL_GRID_TILES = 1, 2, 4, 8, 16, 32, 64, 128
TUNE_DCN_SPLIT_4W = 256
TUNE_NO_HALO_TAP2 = 512
TUNE_TARGETS_MEMSET = 4096     # 1024 and 2048: two variants that lost their A/B and are gone


class tuning:
    """`with _lib.tuning(_lib.TUNE_DCN_MIXED): ...` -- kernel-selection switches of the library for the block (tests, tools)"""

    def __init__(self, flags):
        self.flags = flags

    def __enter__(self):
        self.prev = lib().ctdet_get_tuning_flags()
        lib().ctdet_set_tuning_flags(self.prev | self.flags)
        return self

    def __exit__(self, *exc):
        lib().ctdet_set_tuning_flags(self.prev)
        return False
