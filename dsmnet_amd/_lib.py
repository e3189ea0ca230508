"""ctypes binding of libdsmnet_hip.so (the C ABI of include/dsmnet_hip.h).

This is the whole reference-side binding: the reference is Python, so a
maintainer who wants the MI355X path adds exactly this stub.
There is no CPU fallback: if the library is missing the import of any op raises.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# DSM_LIB_PATH: another build of the same ABI (same-box A/B runs of kernel variants: scripts/ab_builds.sh)
LIB_PATH = os.environ.get("DSM_LIB_PATH") or os.path.join(_HERE, "csrc", "libdsmnet_hip.so")

c_int, c_void_p, c_size_t = ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t

DSM_OK = 0
DSM_F32 = 0
DSM_NCDHW, DSM_NDHWC = 0, 1
DSM_CONV_FP32_MFMA, DSM_CONV_COUT1_CHUNKED, DSM_CONV_TM_SHIFT, DSM_CONV_BLOCKS_SHIFT = 1, 2, 4, 16
DSM_CONV_NO_NSPLIT = 4
DSM_CONV_NO_ONCE = 8
DSM_CONV_KSPLIT_SHIFT = 8
DSM_PREC_F32, DSM_PREC_F16, DSM_PREC_F16X2 = 0, 1, 2
DSM_SIM_DOT, DSM_SIM_COSINE = 0, 1
DSM_CORR_BWD_NAIVE = 1


class Bn3dArgs(ctypes.Structure):
    """struct dsm_bn3d_args (include/dsmnet_hip.h)."""
    _fields_ = [("y", c_void_p), ("residual", c_void_p), ("out", c_void_p), ("gamma", c_void_p),
                ("beta", c_void_p), ("running_mean", c_void_p), ("running_var", c_void_p),
                ("affine", c_void_p), ("workspace", c_void_p), ("gout", c_void_p), ("dy", c_void_p),
                ("dresidual", c_void_p), ("B", c_int), ("C", c_int),
                ("Dy", c_int), ("Hy", c_int), ("Wy", c_int), ("Dr", c_int), ("Hr", c_int), ("Wr", c_int),
                ("relu", c_int), ("momentum", ctypes.c_float), ("eps", ctypes.c_float),
                ("out_amax", c_void_p), ("dy_amax", c_void_p), ("dres_amax", c_void_p)]


class Conv3dArgs(ctypes.Structure):
    """struct dsm_conv3d_args (include/dsmnet_hip.h)."""
    _fields_ = [("x", c_void_p), ("w_packed", c_void_p), ("scale", c_void_p),
                ("shift", c_void_p), ("residual", c_void_p), ("y", c_void_p),
                ("B", c_int), ("Cin", c_int), ("Cout", c_int),
                ("Di", c_int), ("Hi", c_int), ("Wi", c_int),
                ("Do", c_int), ("Ho", c_int), ("Wo", c_int),
                ("Dr", c_int), ("Hr", c_int), ("Wr", c_int),
                ("stride", c_int), ("transposed", c_int), ("relu", c_int),
                ("kd", c_int), ("k", c_int), ("dil", c_int),
                ("flags", c_int), ("precision", c_int), ("x_amax", c_void_p), ("y_amax", c_void_p),
                ("vol_virtual", c_int), ("vol_mask_left", c_int),
                ("workspace", c_void_p), ("workspace_bytes", c_size_t)]


class BasicBlock2dArgs(ctypes.Structure):
    """struct dsm_basicblock2d_args (include/dsmnet_hip.h)."""
    _fields_ = [("x", c_void_p), ("y", c_void_p), ("w1_packed", c_void_p), ("w2_packed", c_void_p),
                ("scale1", c_void_p), ("shift1", c_void_p), ("scale2", c_void_p), ("shift2", c_void_p),
                ("x_amax", c_void_p), ("y_amax", c_void_p),
                ("B", c_int), ("H", c_int), ("W", c_int), ("C", c_int), ("precision", c_int), ("relu", c_int), ("no_skip", c_int)]


class SelfsupItem(ctypes.Structure):
    """struct dsm_selfsup_item (include/dsmnet_hip.h)."""
    _fields_ = [("im", c_void_p), ("src", c_void_p), ("disp", c_void_p), ("disp_other", c_void_p),
                ("grad_disp", c_void_p), ("grad_other", c_void_p),
                ("im_stride", c_int * 4), ("src_stride", c_int * 4),
                ("B", c_int), ("h", c_int), ("w", c_int), ("H0", c_int), ("W0", c_int),
                ("left", c_int), ("top", c_int), ("scale_factor", c_int),
                ("delt_im", ctypes.c_float), ("delt_disp", ctypes.c_float), ("weight", ctypes.c_float),
                ("ds_divisor", c_int)]


# the flags word of dsm_selfsup_fwd / dsm_selfsup_bwd (include/dsmnet_hip.h)
DSM_SELFSUP_MASK, DSM_SELFSUP_CAP, DSM_SELFSUP_DS, DSM_SELFSUP_LR = 1, 2, 4, 8
DSM_SELFSUP_COMMON, DSM_SELFSUP_SSSMNET = 16, 32        # dsm_selfsup_ext_* only


class SelfsupExt(ctypes.Structure):
    """struct dsm_selfsup_ext (include/dsmnet_hip.h): the side array of SsSMnet, one per item."""
    _fields_ = [("warp", c_void_p), ("grad_warp", c_void_p), ("delt_im1", ctypes.c_float), ("reserved", c_int)]


class SuplossItem(ctypes.Structure):
    """struct dsm_suploss_item (include/dsmnet_hip.h), 48 bytes."""
    _fields_ = [("pred", c_void_p), ("grad", c_void_p), ("B", c_int), ("hc", c_int), ("wc", c_int),
                ("level", c_int), ("weight", ctypes.c_float), ("pad_", c_int * 3)]


DSM_SUPLOSS_MAX_ITEMS = 16


class MetricsArgs(ctypes.Structure):
    """struct dsm_metrics_args (include/dsmnet_hip.h), 72 bytes."""
    _fields_ = [("pred", c_void_p), ("gt", c_void_p), ("imL", c_void_p), ("imR", c_void_p),
                ("workspace", c_void_p), ("out", c_void_p), ("B", c_int), ("C", c_int), ("H", c_int),
                ("W", c_int), ("delt", ctypes.c_float), ("flags", c_int)]


DSM_METRICS_SLOTS = 16
DSM_METRICS_NEGATE_WARP = 1


class LrcheckArgs(ctypes.Structure):
    """struct dsm_lrcheck_args (include/dsmnet_hip.h), 80 bytes."""
    _fields_ = [("disp", c_void_p), ("other", c_void_p), ("wrap", c_void_p), ("weight", c_void_p),
                ("mask", c_void_p), ("masked", c_void_p), ("B", c_int), ("H", c_int), ("W", c_int),
                ("delt", ctypes.c_float), ("factor", ctypes.c_float), ("threshold", ctypes.c_float),
                ("flags", c_int), ("reserved", c_int)]


DSM_LRCHECK_OTHER_RIGHT_FRAME = 1


class SpeckleArgs(ctypes.Structure):
    """struct dsm_speckle_args (include/dsmnet_hip.h), 80 bytes."""
    _fields_ = [("disp", c_void_p), ("valid", c_void_p), ("out", c_void_p), ("keep", c_void_p),
                ("size", c_void_p), ("workspace", c_void_p), ("B", c_int), ("H", c_int), ("W", c_int),
                ("max_size", c_int), ("max_diff", ctypes.c_float), ("new_val", ctypes.c_float), ("flags", c_int)]


class EncodeArgs(ctypes.Structure):
    """struct dsm_encode_args (include/dsmnet_hip.h), 104 bytes."""
    _fields_ = [("disp", c_void_p), ("gt", c_void_p), ("mask", c_void_p), ("u16", c_void_p), ("u8", c_void_p),
                ("rgb", c_void_p), ("err", c_void_p), ("workspace", c_void_p), ("B", c_int), ("Hs", c_int),
                ("Ws", c_int), ("y0", c_int), ("x0", c_int), ("h", c_int), ("w", c_int),
                ("vmin", ctypes.c_float), ("vmax", ctypes.c_float), ("flags", c_int)]


DSM_ENCODE_FLIP, DSM_ENCODE_AUTO_RANGE = 1, 2


class ColorRecord(ctypes.Structure):
    """struct dsm_color_record (include/dsmnet_hip.h)."""
    _fields_ = [("order", c_int * 4), ("jitter", ctypes.c_float * 4), ("flags", c_int), ("alpha_row", c_int)]


DSM_COLOR_JITTER, DSM_COLOR_LIGHTING, DSM_COLOR_NORMALIZE = 1, 2, 4
DSM_COLOR_MAX_RECORDS = 64


class SpatialRecord(ctypes.Structure):
    """struct dsm_spatial_record (include/dsmnet_hip.h), 48 bytes."""
    _fields_ = [("shift", c_int), ("ws", c_int), ("hs", c_int), ("w", c_int), ("h", c_int),
                ("resize", c_int), ("scale_rand", ctypes.c_float), ("pad_", c_int),
                ("scale_x", ctypes.c_double), ("scale_y", ctypes.c_double)]


DSM_SPATIAL_MAX_RECORDS = 48


class FrameSource(ctypes.Structure):
    """struct dsm_frame_source (include/dsmnet_hip.h), 64 bytes."""
    _fields_ = [("imL", ctypes.c_longlong), ("imR", ctypes.c_longlong),
                ("dispL", ctypes.c_longlong), ("dispR", ctypes.c_longlong),
                ("Hs", c_int), ("Ws", c_int), ("y0", c_int), ("x0", c_int),
                ("flip", c_int), ("disp_format", c_int), ("pad_", c_int * 2)]


DSM_DISP_F32 = 0
DSM_DISP_U16_256 = 1
DSM_DISP_U16 = 2
DSM_DISP_U8 = 3
DSM_FRAMES_MAX_RECORDS = 32


# name -> (restype, argtypes); must list every symbol declared in dsmnet_hip.h
SIGNATURES = {
    "dsm_abi_version": (c_int, []),
    "dsm_strerror": (ctypes.c_char_p, [c_int]),
    "dsm_corr1d_fwd": (c_int, [c_void_p] * 4 + [c_int] * 8 + [c_void_p]),
    "dsm_corr1d_bwd": (c_int, [c_void_p] * 6 + [c_int] * 8 + [c_void_p]),
    "dsm_concat_volume_fwd": (c_int, [c_void_p] * 3 + [c_int] * 8 + [c_void_p]),
    "dsm_concat_volume_bwd": (c_int, [c_void_p] * 3 + [c_int] * 8 + [c_void_p]),
    "dsm_soft_argmin_fwd": (c_int, [c_void_p] * 3 + [c_int] * 10 + [c_void_p]),
    "dsm_soft_argmin_bwd": (c_int, [c_void_p] * 5 + [c_int] * 10 + [c_void_p]),
    "dsm_corr1d_plan": (c_int, [c_void_p] * 4 + [c_int] * 8 + [ctypes.c_char_p, c_int]),
    "dsm_corr1d_sim_fwd": (c_int, [c_void_p] * 5 + [c_int] * 8 + [ctypes.c_float, c_int, c_void_p]),
    "dsm_corr1d_sim_fwd_plan": (c_int, [c_void_p] * 5 + [c_int] * 8 + [ctypes.c_float, c_int, ctypes.c_char_p, c_int]),
    "dsm_corr1d_sim_bwd": (c_int, [c_void_p] * 8 + [c_int] * 8 + [ctypes.c_float, c_int, c_int, c_void_p]),
    "dsm_corr1d_sim_bwd_plan": (c_int, [c_void_p] * 8 + [c_int] * 8 + [ctypes.c_float, c_int, c_int, ctypes.c_char_p, c_int]),
    "dsm_corr1d_sim_workspace_bytes": (c_size_t, [c_int] * 7),
    "dsm_concat_volume_fwd_plan": (c_int, [c_void_p] * 3 + [c_int] * 8 + [ctypes.c_char_p, c_int]),
    "dsm_concat_volume_bwd_plan": (c_int, [c_void_p] * 3 + [c_int] * 8 + [ctypes.c_char_p, c_int]),
    "dsm_soft_argmin_fwd_plan": (c_int, [c_void_p] * 3 + [c_int] * 10 + [ctypes.c_char_p, c_int]),
    "dsm_soft_argmin_bwd_plan": (c_int, [c_void_p] * 5 + [c_int] * 10 + [ctypes.c_char_p, c_int]),
    "dsm_disp_confidence_fwd": (c_int, [c_void_p] * 6 + [c_int] * 11 + [c_void_p]),
    "dsm_disp_confidence_fwd_plan": (c_int, [c_void_p] * 6 + [c_int] * 11 + [ctypes.c_char_p, c_int]),
    "dsm_conv3d_packed_weight_bytes": (c_size_t, [c_int] * 3),
    "dsm_conv3d_pack_weights": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_void_p]),
    "dsm_conv_pack_weights": (c_int, [c_void_p] * 2 + [c_int] * 5 + [c_void_p]),
    "dsm_absmax": (c_int, [c_void_p, c_size_t, c_void_p, c_void_p]),
    "dsm_conv3d_fwd": (c_int, [ctypes.POINTER(Conv3dArgs), c_void_p]),
    "dsm_basicblock2d_fwd": (c_int, [ctypes.POINTER(BasicBlock2dArgs), c_void_p]),
    "dsm_conv3d_plan": (c_int, [ctypes.POINTER(Conv3dArgs), ctypes.c_char_p, c_int]),
    "dsm_conv3d_workspace_bytes": (c_size_t, [ctypes.POINTER(Conv3dArgs)]),
    "dsm_conv3d_wgrad": (c_int, [c_void_p] * 4 + [c_int] * 12 + [c_void_p] * 3),
    "dsm_conv2d_wgrad": (c_int, [c_void_p] * 4 + [c_int] * 11 + [c_void_p] * 3),
    "dsm_bias_relu_bwd": (c_int, [c_void_p] * 6 + [ctypes.c_long, c_int, c_void_p]),
    "dsm_conv3d_cout1_bwd": (c_int, [c_void_p] * 5 + [c_int] * 5 + [c_void_p]),
    "dsm_deconv3d_cout1_bwd": (c_int, [c_void_p] * 5 + [c_int] * 8 + [c_void_p]),
    "dsm_bn3d_train_fwd": (c_int, [ctypes.POINTER(Bn3dArgs), c_void_p]),
    "dsm_bn3d_train_bwd": (c_int, [ctypes.POINTER(Bn3dArgs), c_void_p]),
    "dsm_decoder_cat": (c_int, [c_void_p] * 5 + [c_int] * 11 + [c_void_p]),
    "dsm_stage_images_nhwc16": (c_int, [c_void_p] * 3 + [c_int] * 4 + [c_void_p]),
    "dsm_volume_relayout": (c_int, [c_void_p] * 2 + [c_int] * 6 + [c_void_p]),
    "dsm_conv_packed_weight_bytes": (ctypes.c_size_t, [c_int] * 4),
    "dsm_spp_branch_floats": (ctypes.c_size_t, [c_int] * 3),
    "dsm_spp_pool8": (c_int, [c_void_p] * 2 + [c_int] * 3 + [c_void_p]),
    "dsm_spp_branches": (c_int, [c_void_p] * 5 + [c_int] * 3 + [c_void_p]),
    "dsm_spp_concat": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p] * 2),
    "dsm_warp_abs_error": (c_int, [c_void_p] * 4 + [c_int] * 6 + [ctypes.c_float, c_void_p]),
    "dsm_warp_abs_error_bwd": (c_int, [c_void_p] * 7 + [c_int] * 6 + [ctypes.c_float, c_void_p]),
    "dsm_decoder_cat_bwd": (c_int, [c_void_p] * 6 + [c_int] * 11 + [c_void_p]),
    "dsm_selfsup_workspace_floats": (c_size_t, [ctypes.POINTER(SelfsupItem), c_int]),
    "dsm_selfsup_fwd": (c_int, [ctypes.POINTER(SelfsupItem), c_int, c_int] + [c_void_p] * 4),
    "dsm_selfsup_bwd": (c_int, [ctypes.POINTER(SelfsupItem), c_int, c_int] + [c_void_p] * 4),
    "dsm_selfsup_ext_workspace_floats": (c_size_t, [ctypes.POINTER(SelfsupItem), c_int, c_int]),
    "dsm_selfsup_ext_fwd": (c_int, [ctypes.POINTER(SelfsupItem), ctypes.POINTER(SelfsupExt), c_int, c_int] + [c_void_p] * 4),
    "dsm_selfsup_ext_bwd": (c_int, [ctypes.POINTER(SelfsupItem), ctypes.POINTER(SelfsupExt), c_int, c_int] + [c_void_p] * 4),
    "dsm_selfsup_dyn_fwd": (c_int, [ctypes.POINTER(SelfsupItem), ctypes.POINTER(SelfsupExt), c_int, c_int] + [c_void_p] * 5),
    "dsm_selfsup_dyn_bwd": (c_int, [ctypes.POINTER(SelfsupItem), ctypes.POINTER(SelfsupExt), c_int, c_int] + [c_void_p] * 5),
    "dsm_suploss_workspace_floats": (c_size_t, [c_int] * 5),
    "dsm_suploss_fwd": (c_int, [ctypes.POINTER(SuplossItem), c_int, c_void_p, c_int, c_int, c_int, c_int] + [c_void_p] * 4),
    "dsm_suploss_bwd": (c_int, [ctypes.POINTER(SuplossItem), c_int, c_void_p, c_int, c_int, c_int] + [c_void_p] * 4),
    "dsm_stereo_metrics_workspace_bytes": (c_size_t, [c_int] * 3),
    "dsm_stereo_metrics": (c_int, [ctypes.POINTER(MetricsArgs), c_void_p]),
    "dsm_lr_check": (c_int, [ctypes.POINTER(LrcheckArgs), c_void_p]),
    "dsm_fill_background_workspace_bytes": (c_size_t, [c_int] * 3),
    "dsm_fill_background": (c_int, [c_void_p] * 4 + [c_int] * 3 + [c_void_p]),
    "dsm_speckle_workspace_bytes": (c_size_t, [c_int] * 3),
    "dsm_speckle_filter": (c_int, [ctypes.POINTER(SpeckleArgs), c_void_p]),
    "dsm_disp_encode_workspace_bytes": (c_size_t, [c_int] * 3),
    "dsm_disp_encode": (c_int, [ctypes.POINTER(EncodeArgs), c_void_p]),
    "dsm_stereo_color": (c_int, [c_void_p, c_void_p, ctypes.POINTER(ColorRecord)] + [c_int] * 6 + [c_void_p]),
    "dsm_stereo_spatial": (c_int, [c_void_p, c_void_p, ctypes.POINTER(SpatialRecord)] + [c_int] * 8 + [c_void_p]),
    "dsm_stereo_spatial_raw": (c_int, [c_void_p, c_size_t, ctypes.POINTER(FrameSource), c_void_p,
                                       ctypes.POINTER(SpatialRecord)] + [c_int] * 8 + [c_void_p]),
    "dsm_stereo_spatial_raw_plan": (c_int, [c_void_p, c_size_t, ctypes.POINTER(FrameSource), c_void_p,
                                            ctypes.POINTER(SpatialRecord)] + [c_int] * 8),
    "dsm_concat_conv_fwd": (c_int, [c_void_p] * 5 + [c_size_t] + [c_void_p] * 2 + [c_int] * 9 + [c_void_p]),
}

_lib = None


class DsmnetHipError(RuntimeError):
    pass


def _bind_torch_hip_runtime():
    """One HIP runtime per process.  PyTorch ships its own libamdhip64.so.7 and this
    library is linked against the same soname, so the dynamic loader gives both whichever
    copy was loaded FIRST.  Loading ours before torch would bring in /opt/rocm's runtime,
    torch would then run on a runtime it was not built with, and launches on torch's
    streams fail (observed: hipErrorLaunchFailure on the first kernel).  Import torch and
    map its copy globally before ours."""
    import torch
    hip = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    if os.path.exists(hip):
        ctypes.CDLL(hip, mode=ctypes.RTLD_GLOBAL)


def load():
    """Load the HIP library (once).  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DsmnetHipError(
            "libdsmnet_hip.so not found at %s -- build it with "
            "`python -m dsmnet_amd.csrc.build` (there is no CPU fallback)" % LIB_PATH)
    _bind_torch_hip_runtime()
    lib = ctypes.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the symbol is missing
        fn.restype = res
        fn.argtypes = args
    if lib.dsm_abi_version() != 7:
        raise DsmnetHipError("libdsmnet_hip.so ABI version mismatch")
    _lib = lib
    return lib


def check(code, what):
    if code != DSM_OK:
        msg = load().dsm_strerror(code).decode()
        raise DsmnetHipError("%s failed: %s (code %d)" % (what, msg, code))
