"""ctypes binding of libvti.so (include/vti.h).  This is the stub INTEGRATION.md shows a
maintainer of the reference adding next to measurement.py.  There is no CPU fallback: if the
HIP library is missing the import fails loudly."""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# VTI_LIB_VARIANT=stamps selects the diagnostic build (tools/ only); the product always loads libvti.so
_VARIANT = os.environ.get("VTI_LIB_VARIANT", "")       # developer builds: "stamps" (in-kernel timing), experiment variants (csrc/Makefile: variant)
LIB_PATH = os.path.join(_HERE, f"libvti_{_VARIANT}.so" if _VARIANT else "libvti.so")

VTI_F16, VTI_F32, VTI_H2 = 0, 1, 2
VTI_MASK_LOGIT, VTI_MASK_SIGMOID = 0, 1
VTI_PACK_U8, VTI_PACK_BITS = 0, 1
VTI_MASK_NATIVE = 0x10       # vti_predict mask_mode flag: frame-resolution masks (vti_masks_native)


class VtiDesc(C.Structure):
    _fields_ = [("scale", C.c_char), ("nc", C.c_int32), ("nm", C.c_int32), ("reg_max", C.c_int32),
                ("H", C.c_int32), ("W", C.c_int32), ("max_batch", C.c_int32), ("dtype", C.c_int32)]


class VtiConvInfo(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("c1", C.c_int32), ("c2", C.c_int32), ("k", C.c_int32),
                ("s", C.c_int32), ("kind", C.c_int32), ("h_in", C.c_int32), ("w_in", C.c_int32),
                ("h_out", C.c_int32), ("w_out", C.c_int32), ("macs", C.c_int64),
                ("tile_h", C.c_int32), ("tile_w", C.c_int32), ("waves_n", C.c_int32), ("nrep", C.c_int32),
                ("lds_bytes", C.c_int32), ("fused", C.c_int32), ("persistent", C.c_int32)]


class VtiMeasureParams(C.Structure):
    """include/vti.h vti_measure_params."""
    _fields_ = [("K", C.c_double * 9), ("dist", C.c_double * 5), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("max_px_distance", C.c_double), ("two_row_threshold_px", C.c_double),
                ("stitch_id", C.c_int32), ("fabric_id", C.c_int32), ("roi_enabled", C.c_int32), ("roi", C.c_int32 * 4),
                ("min_stitches", C.c_int32), ("envelope_neighborhood", C.c_int32), ("skip_cluster", C.c_int32),
                ("kmeans_iters", C.c_int32), ("drop_empty", C.c_int32), ("frame_buffer", C.c_int32)]


class VtiCheckerParams(C.Structure):
    """include/vti.h vti_checker_params."""
    _fields_ = [("K", C.c_double * 9), ("dist", C.c_double * 5), ("R", C.c_double * 9), ("t", C.c_double * 3),
                ("max_px_distance", C.c_double),
                ("stitch_id", C.c_int32), ("fabric_id", C.c_int32), ("min_stitches", C.c_int32), ("envelope_neighborhood", C.c_int32),
                ("skip_cluster", C.c_int32), ("kmeans_iters", C.c_int32), ("drop_empty", C.c_int32), ("frame_buffer", C.c_int32)]


class VtiStampDesc(C.Structure):
    """include/vti.h vti_stamp_desc."""
    _fields_ = [("picture", C.c_int32), ("x", C.c_int32), ("y", C.c_int32), ("w", C.c_int32), ("h", C.c_int32), ("pitch", C.c_int32),
                ("bgr", C.c_uint8 * 4), ("reserved", C.c_int32), ("word_offset", C.c_int64)]


class VtiNmsParams(C.Structure):
    """include/vti.h vti_nms_params."""
    _fields_ = [("conf", C.c_float), ("max_det", C.c_int32), ("iou", C.c_double), ("agnostic", C.c_int32), ("n_classes", C.c_int32),
                ("classes", C.POINTER(C.c_int32))]


VTI_NMS_TABLE_MAX_ROWS, VTI_NMS_TABLE_MAX_CLASSES = 65536, 1024
VTI_MEASURE_OK, VTI_MEASURE_NO_FABRIC, VTI_MEASURE_NO_STITCHES, VTI_MEASURE_BAD_CAMERA = 0, 1, 2, 3
VTI_STITCH_KEPT, VTI_STITCH_MASK, VTI_STITCH_SELECTED, VTI_STITCH_NEAR, VTI_STITCH_DIST, VTI_STITCH_WIDTH = 1, 2, 4, 8, 16, 32
VTI_MEASURE_MAX_DET = 1000

VTI_POLY_LARGEST, VTI_POLY_CONCAT = 0, 1
VTI_POLY_OK, VTI_POLY_ERR_BOUND, VTI_POLY_ERR_RANGE = 0, 1, 2
VTI_ANNOTATE_OUTLINE_SKIPPED = 1
VTI_OVERLAY_DRAW, VTI_OVERLAY_BLEND, VTI_OVERLAY_BOTH = 1, 2, 3
VTI_OVERLAY_OUTLINE_SKIPPED = 1
VTI_JPEG_CORRUPT = 1
VTI_RAW_YUYV, VTI_RAW_UYVY, VTI_RAW_NV12, VTI_RAW_NV21, VTI_RAW_I420, VTI_RAW_YV12 = range(6)
VTI_STAMP_MAX_PICTURES, VTI_STAMP_MAX_PER_PICTURE, VTI_STAMP_MAX_TOTAL, VTI_STAMP_MAX_PITCH = 4096, 65536, 1 << 24, 65536
VTI_ERR_ARG, VTI_ERR_UNSUPPORTED = -1, -6


class VtiError(RuntimeError):
    """Raised for any non-zero vti_status (the reference catches every predict exception,
    measurement.py:207-216)."""

    def __init__(self, code, msg):
        super().__init__(f"libvti error {code}: {msg}")
        self.code = code


_P, _I32, _I64, _F, _D, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_double, C.c_size_t

# name -> (restype, argtypes); every symbol include/vti.h declares
SIGNATURES = {
    "vti_create": (_I32, [C.POINTER(VtiDesc), C.POINTER(_P)]),
    "vti_destroy": (None, [_P]),
    "vti_last_error": (C.c_char_p, [_P]),
    "vti_num_convs": (_I32, [_P]),
    "vti_conv_at": (_I32, [_P, _I32, C.POINTER(VtiConvInfo)]),
    "vti_num_anchors": (_I32, [_P]),
    "vti_fused_params": (_I64, [_P]),
    "vti_macs_per_frame": (_I64, [_P]),
    "vti_workspace_bytes": (_I64, [_P]),
    "vti_num_launches": (_I32, [_P]),
    "vti_load_weights": (_I32, [_P, _P, _SZ, _I32]),
    "vti_set_workspace": (_I32, [_P, _P, _SZ]),
    "vti_letterbox": (_I32, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "vti_forward": (_I32, [_P, _P, _I32, _I32, _P, _P, _P]),
    "vti_nms": (_I32, [_P, _P, _I32, _F, _D, _I32, _I32, _P, _P, _P]),
    "vti_forward_scored": (_I32, [_P, _P, _I32, _I32, _P, _P, _P, _P]),
    "vti_nms_scored": (_I32, [_P, _P, _P, _I32, _F, _D, _I32, _I32, _P, _P, _P]),
    "vti_masks": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "vti_masks_native": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _I32, _P, _P]),
    "vti_mask_native_layout": (_I32, [_P, _I32, _I32, _I32, C.POINTER(_I32)]),
    "vti_scale_boxes": (_I32, [_P, _P, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "vti_predict": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _F, _D, _I32, _I32, _I32, _I32,
                           _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P]),
    "vti_mask_to_frame": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P, _P]),
    "vti_union_envelope": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "vti_mask_stats": (_I32, [_P, _P, _I32, _I32, _I32, _P, _P]),
    "vti_mask_stats_bits": (_I32, [_P, _P, _I32, _P, _I32, _I32, _I32, _I32, _P, _P]),
    "vti_envelope_bits": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "vti_pixels_to_world": (_I32, [_P, _P, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "vti_kmeans1d2": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _P, _P]),
    "vti_measure_scratch_bytes": (_I64, [_P, _I32, _I32, _I32]),
    "vti_measure": (_I32, [_P, C.POINTER(VtiMeasureParams), _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ,
                           _P, _P, _P, _P, _P]),
    "vti_measure_checker": (_I32, [_P, C.POINTER(VtiCheckerParams), _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ,
                                   _P, _P, _P, _P, _P]),
    "vti_measure_cameras_bytes": (_I64, [_I32]),
    "vti_measure_pack_cameras": (_I32, [_P, C.POINTER(VtiMeasureParams), _I32, _P, _SZ]),
    "vti_measure_cameras": (_I32, [_P, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ,
                                   _P, _P, _P, _P, _P]),
    "vti_frame_table_bytes": (_I64, [_I32]),
    "vti_pack_frames": (_I32, [_P, _I32, _I32, _P, _P, _P, _I32, _I64, _P, _SZ]),
    "vti_frame_table_info": (_I32, [_P, _I32, _P, _P]),
    "vti_letterbox_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _P]),
    "vti_scale_boxes_frames": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "vti_predict_frames": (_I32, [_P, _P, _P, _P, _I32, _I32, _F, _D, _I32, _I32, _I32, _I32,
                                  _P, _P, _P, _P, _P, _P, _I32, _P, _P, _P]),
    "vti_measure_frames": (_I32, [_P, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _SZ,
                                  _P, _P, _P, _P, _P]),
    "vti_mask_native_frames_bytes": (_I64, [_P, _P, _I32]),
    "vti_masks_native_frames": (_I32, [_P, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _P]),
    "vti_predict_frames_native": (_I32, [_P, _P, _P, _P, _I32, _I32, _F, _D, _I32, _I32, _I32, _I32,
                                         _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P]),
    "vti_measure_frames_native": (_I32, [_P, _P, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _SZ,
                                         _P, _P, _P, _P, _P]),
    "vti_mask_polygons_scratch_bytes": (_I64, [_P, _I32, _I32, _I32]),
    "vti_mask_polygons": (_I32, [_P, _P, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _SZ, _P, _P, _I64, _P]),
    "vti_mask_polygons_frames_scratch_bytes": (_I64, [_P, _P, _I32]),
    "vti_mask_polygons_frames": (_I32, [_P, _P, _I32, _P, _I64, _P, _P, _P, _I32, _I32, _I32, _P, _SZ, _P, _P, _I64, _P]),
    "vti_annotate_scratch_bytes": (_I64, [_P, _I32, _I32, _I32, _I32, _I32]),
    "vti_annotate": (_I32, [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _I32,
                            _I32, _P, _P, _P, _SZ, _P]),
    "vti_annotate_frames_scratch_bytes": (_I64, [_P, _P, _I32, _I32]),
    "vti_annotate_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _I32,
                                   _I32, _P, _P, _P, _P, _P, _SZ, _P]),
    "vti_annotate_checker": (_I32, [_P, _P, _I32, _I32, _I32, C.POINTER(VtiCheckerParams), _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P,
                                    _P, _P, _I32, _I32, _P, _P, _P, _SZ, _P]),
    "vti_checker_pack_cameras": (_I32, [_P, C.POINTER(VtiCheckerParams), _I32, _P, _SZ]),
    "vti_measure_checker_cameras": (_I32, [_P, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ,
                                           _P, _P, _P, _P, _P]),
    "vti_measure_checker_frames": (_I32, [_P, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _SZ,
                                          _P, _P, _P, _P, _P]),
    "vti_measure_checker_frames_native": (_I32, [_P, _P, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _SZ,
                                                 _P, _P, _P, _P, _P]),
    "vti_annotate_checker_cameras": (_I32, [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P,
                                            _P, _P, _I32, _I32, _P, _P, _P, _SZ, _P]),
    "vti_annotate_checker_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P,
                                           _I32, _I32, _P, _P, _P, _P, _P, _SZ, _P]),
    "vti_annotate_frames_native": (_I32, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _I32, _P, _P, _P, _P, _P,
                                          _I32, _I32, _P, _P, _P, _P, _P, _SZ, _P]),
    "vti_annotate_checker_frames_native": (_I32, [_P, _P, _P, _P, _I32, _P, _I32, _P, _P, _P, _I64, _P, _P, _P, _P, _I32, _I32, _P, _P, _P,
                                                  _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _SZ, _P]),
    "vti_overlay_scratch_bytes": (_I64, [_P, _I32, _I32, _I32, _I32, _I32]),
    "vti_overlay": (_I32, [_P, _P, _I32, _I32, _I32, _P, _I32, _P, _P, _P, _P, _I32, _I32, _P, _P, _I32, _F, _F, _P, _P, _I32, _I32, _P,
                           _I32, _P, _P, _P, _SZ, _P]),
    "vti_overlay_frames_scratch_bytes": (_I64, [_P, _P, _I32, _I32]),
    "vti_overlay_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _I32, _P, _I64, _P, _P, _P, _P, _I32, _I32, _P, _P, _I32, _F, _F, _P, _P, _I32,
                                  _I32, _P, _I32, _P, _P, _P, _P, _P, _SZ, _P]),
    "vti_encode_jpeg_scratch_bytes": (_I64, [_P, _I32, _I32, _I32]),
    "vti_encode_jpeg_max_bytes": (_I64, [_I32, _I32, _I32]),
    "vti_encode_jpeg": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _SZ, _P, _P, _I64, _P]),
    "vti_encode_jpeg_frames_scratch_bytes": (_I64, [_P, _P]),
    "vti_encode_jpeg_frames_max_bytes": (_I64, [_P]),
    "vti_encode_jpeg_frames": (_I32, [_P, _P, _P, _P, _I32, _I32, _I32, _P, _SZ, _P, _P, _I64, _P]),
    "vti_stamp_table_bytes": (_I64, [_I32, _I32]),
    "vti_pack_stamps": (_I32, [_P, _P, _P, _I32, _P, _I32, _I64, _P, _SZ]),
    "vti_stamp": (_I32, [_P, _P, _I32, _I32, _I32, _P, _P, _P, _I64, _P]),
    "vti_stamp_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _P, _P, _I64, _P]),
    "vti_nms_table_bytes": (_I64, [_I32]),
    "vti_pack_nms_table": (_I32, [_P, C.POINTER(VtiNmsParams), _I32, _P, _SZ]),
    "vti_set_nms_table": (_I32, [_P, _P, _P, _I32, _P]),
    "vti_window_table_bytes": (_I64, [_I32]),
    "vti_pack_windows": (_I32, [_P, _I32, _I32, _P, _P, _P, _P, _I32, _I64, _P, _SZ]),
    "vti_window_table_info": (_I32, [_P, _I32, _P, _P]),
    "vti_letterbox_windows": (_I32, [_P, _P, _P, _P, _I32, _P, _P]),
    "vti_scale_boxes_windows": (_I32, [_P, _P, _P, _P, _P, _I32, _I32, _P, _P]),
    "vti_mask_native_windows_bytes": (_I64, [_P, _P, _I32]),
    "vti_masks_native_windows": (_I32, [_P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _I32, _P, _I64, _P, _P, _P]),
    "vti_predict_windows": (_I32, [_P, _P, _P, _P, _I32, _I32, _F, _D, _I32, _I32, _I32, _I32,
                                   _P, _P, _P, _P, _P, _P, _I64, _P, _P, _P, _P]),
    "vti_decode_jpeg_table_bytes": (_I64, [_I32]),
    "vti_decode_jpeg_plan": (_I32, [_P, _P, _P, _I32, _I32, _I32, _P, _SZ, _P, _P, _P, _P]),
    "vti_decode_jpeg": (_I32, [_P, _P, _P, _P, _I32, _I32, _P, _I64, _P, _P, _SZ, _P]),
    "vti_raw_frame_bytes": (_I64, [_I32, _I32, _I32]),
    "vti_convert_raw": (_I32, [_P, _P, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "vti_raw_table_bytes": (_I64, [_I32]),
    "vti_pack_raw_frames": (_I32, [_P, _P, _P, _P, _I32, _P, _SZ, _P]),
    "vti_convert_raw_frames": (_I32, [_P, _P, _I64, _P, _P, _P, _P, _I32, _I32, _P, _I64, _P]),
    "vti_debug_conv_output": (_I32, [_P, _I32, _I32, _P, _P]),
    "vti_debug_conv2d": (_I32, [_I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P, _I32, _I32, _I32, _I32,
                                _P, _I32, _I32, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32,
                                _P, _P, _P]),
    "vti_debug_sppf_pool": (_I32, [_I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P, _P]),
    "vti_debug_upsample2x": (_I32, [_I32, _P, _P, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _I32, _P]),
    "vti_debug_decode": (_I32, [_I32, _P, _P, _P, _P, _P, _P, _I32, _I32, _I32, _P, _P]),
    "vti_debug_set_conv_output": (_I32, [_P, _I32, _I32, _P, _P]),
    "vti_debug_run_op": (_I32, [_P, _I32, _P, _I32, _I32, _P, _P, _P, _P, _P]),
}

_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                              f"g.build()'` (hipcc --offload-arch=gfx950); there is no CPU fallback")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        _lib = L
    return _lib


def check(ctx, rc):
    if rc != 0:
        msg = lib().vti_last_error(ctx)
        raise VtiError(rc, msg.decode() if msg else "")
