"""ctypes binding of ``libideepcolor_hip.so`` (the C ABI in ``include/ideepcolor.h``).

There is NO fallback: if the shared library has not been built, importing the
binding raises, and if no gfx950 device is visible ``idc_create`` fails with
``IDC_ERR_NO_DEVICE``.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C interactive_deep_colorization_amd/csrc``).
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libideepcolor_hip.so")

IDC_FP32, IDC_BF16, IDC_BF16X3, IDC_BF16X6, IDC_FP16X3, IDC_FP16 = 0, 1, 2, 3, 4, 5
IDC_FLAG_DIST_HEAD, IDC_FLAG_GLOBAL_HINTS, IDC_FLAG_DIST313, IDC_FLAG_THROUGHPUT_BLOB = 0x1, 0x4, 0x8, 0x10
IDC_OK = 0
STATUS_NAMES = {0: "IDC_OK", -1: "IDC_ERR_INVALID_ARG", -2: "IDC_ERR_NO_DEVICE", -3: "IDC_ERR_HIP",
                -4: "IDC_ERR_NO_WEIGHTS", -5: "IDC_ERR_MISSING_KEY", -6: "IDC_ERR_BATCH",
                -7: "IDC_ERR_UNSUPPORTED", -8: "IDC_ERR_INTERNAL"}

# every symbol include/ideepcolor.h declares (tests check the .so exports all of them)
EXPORTED_SYMBOLS = [
    "idc_version", "idc_set_tile_policy", "idc_set_option", "idc_set_splitk_policy", "idc_device_count", "idc_last_error", "idc_create", "idc_destroy", "idc_set_io_scales",
    "idc_weights_blob_bytes", "idc_pack_weights", "idc_set_weights_host", "idc_set_weights_device",
    "idc_load_weights", "idc_weights_device_ptr", "idc_forward", "idc_forward_device", "idc_forward_dist",
    "idc_lab2rgb", "idc_forward_rgb", "idc_forward_rgb_lazy", "idc_fetch_outputs", "idc_global_histogram", "idc_forward_dist313", "idc_set_dist_temperature", "idc_set_global_hints", "idc_clear_global_hints", "idc_sync", "idc_stream", "idc_num_layers", "idc_layer_info_get", "idc_set_profiling",
    "idc_layer_times_ms", "idc_layer_times_stats", "idc_get_activation", "idc_op_conv2d", "idc_op_deconv4x4s2", "idc_op_deconv_shortcut", "idc_op_last_kernel",
    "idc_grid_last", "idc_grid_tag",
    "idc_set_image_l", "idc_set_hints", "idc_get_hint_planes", "idc_forward_resident",
    "idc_dist_bins", "idc_keep_dist", "idc_dist_at", "idc_get_dist", "idc_suggest_colors",
    "idc_dist_entropy", "idc_dist_decode",
    "idc_stream_wait", "idc_stream_signal", "idc_alloc_host", "idc_free_host", "idc_forward_async", "idc_wait", "idc_pipeline_times",
    "idc_comm_unique_id", "idc_broadcast_weights", "idc_upsample_lab2rgb", "idc_set_image_rgb", "idc_fullres_rgb",
    "idc_forward_async_rgb",
    "idc_global_stats_rgb", "idc_set_global_refs", "idc_forward_async_rgb_ref",
    "idc_forward_async_images",
    "idc_reveal_hints", "idc_forward_async_eval",
    "idc_dist_peaks", "idc_suggest_colors_batch", "idc_forward_async_dist",
    "idc_dist_score", "idc_forward_async_dist_score",
    "idc_gamut_map", "idc_snap_colors",
    "idc_set_joint_upsample", "idc_fullres_ab", "idc_set_batch_upsample",
    "idc_set_image_gray", "idc_fullres_rgb16", "idc_forward_async_gray",
    "idc_set_ingest_filter",
    "idc_set_hints_layer", "idc_forward_async_layers",
    "idc_ycc420_bytes", "idc_set_batch_output", "idc_fullres_ycc", "idc_rgb_to_ycc420",
    "idc_set_temporal_filter", "idc_temporal_reset", "idc_temporal_info", "idc_temporal_apply", "idc_temporal_state",
    "idc_set_temporal_motion", "idc_temporal_vectors",
    "idc_set_hint_tracking", "idc_tracked_hints", "idc_track_hints_apply",
    "idc_set_range_audit", "idc_range_reset", "idc_range_report", "idc_pack_weights_ex", "idc_load_weights_ex",
]
IDC_STORE_NONE, IDC_STORE_F32, IDC_STORE_BF16, IDC_STORE_F16 = 0, 1, 2, 3
IDC_INTERP_CUBIC, IDC_INTERP_LINEAR, IDC_INTERP_NEAREST = 0, 1, 2
IDC_INTERP_JOINT, IDC_JOINT_EPS = 3, 1e-6       # idc_fullres_rgb, idc_fullres_ab, idc_set_batch_upsample
IDC_FILTER_BILINEAR, IDC_FILTER_ANTIALIAS = 0, 1    # idc_set_ingest_filter
IDC_SRC_OUTPUT_AB, IDC_SRC_OUTPUT_AB_RAW, IDC_SRC_INPUT_AB, IDC_SRC_NO_AB = 0, 1, 2, 3
IDC_INGEST_KEEP_SOURCE = 1
IDC_L_IMAGE, IDC_L_MASK50 = 0, 1
IDC_BATCH_OUT_SOURCE = 1
IDC_OUT_RGB, IDC_OUT_I420, IDC_OUT_NV12 = 0, 1, 2   # idc_set_batch_output / idc_fullres_ycc / idc_rgb_to_ycc420
IDC_YCC_JFIF, IDC_YCC_BT709_VIDEO = 0, 1
IDC_BATCH_OUT_RGB16 = 2         # idc_forward_async_gray only, 16-bit samples only
IDC_BATCH_MAX_SOURCE_BYTES, IDC_BATCH_MAX_HINTS = 1 << 30, 1 << 20
IDC_REF_SATURATION, IDC_REF_MAX = 1, 4096
IDC_GAMUT_MAX_MAPS, IDC_GAMUT_MAX_SIZE, IDC_SNAP_MAX_COLORS = 64, 512, 65536
IDC_UNIQUE_ID_BYTES = 128
IDC_HINT_AB, IDC_HINT_RGB = 0, 1
IDC_HINT_REVEAL = 2         # idc_reveal_hints / idc_forward_async_eval only
IDC_DECODE_MODE, IDC_DECODE_MEAN = 0, 1
IDC_PEAKS_SKIP_HINTS, IDC_TAPS_SUGGEST_AT_PEAKS = 1, 2
IDC_PEAKS_MAX, IDC_SUGGEST_MAX_QUERIES = 256, 4096
IDC_SCORE_MAX_NN, IDC_SCORE_MAX_RANKS = 16, 8


class IdcError(RuntimeError):
    def __init__(self, status, message):
        RuntimeError.__init__(self, "%s (%d): %s" % (STATUS_NAMES.get(status, "IDC_ERR"), status, message))
        self.status = status


class TensorDesc(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char_p), ("data", ctypes.POINTER(ctypes.c_float)),
                ("ndim", ctypes.c_int), ("dims", ctypes.c_int64 * 4)]


class Hint(ctypes.Structure):
    """idc_hint: inclusive rectangle + (a, b) or (r, g, b)."""
    _fields_ = [("y0", ctypes.c_int32), ("x0", ctypes.c_int32), ("y1", ctypes.c_int32), ("x1", ctypes.c_int32),
                ("c0", ctypes.c_float), ("c1", ctypes.c_float), ("c2", ctypes.c_float)]


class RefImage(ctypes.Structure):
    """idc_ref_image: one host reference photograph, [h,w,3] uint8."""
    _fields_ = [("rgb", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class HintLayer(ctypes.Structure):
    """idc_hint_layer: one host RGBA layer, [h,w,4] uint8, straight alpha; rgba NULL = the image has no layer."""
    _fields_ = [("rgba", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class BatchLayers(ctypes.Structure):
    """idc_batch_layers: the layer table [n], the rule's two parameters, and where the cell counts int32[n] go (or NULL)."""
    _fields_ = [("layers", ctypes.POINTER(HintLayer)), ("alpha_min", ctypes.c_int32), ("cover", ctypes.c_int32), ("cells", ctypes.c_void_p)]


class GrayImage(ctypes.Structure):
    """idc_gray_image: one host greyscale plane, [h,w] uint8 or uint16."""
    _fields_ = [("pix", ctypes.c_void_p), ("h", ctypes.c_int32), ("w", ctypes.c_int32)]


class BatchRefs(ctypes.Structure):
    """idc_batch_refs: the six reference arguments of idc_forward_async_rgb_ref, for idc_forward_async_images."""
    _fields_ = [("m", ctypes.c_int32), ("refs", ctypes.POINTER(RefImage)), ("ref_index", ctypes.c_void_p), ("centres", ctypes.c_void_p),
                ("hist_flag", ctypes.c_float), ("flags", ctypes.c_uint32)]


class DistQuery(ctypes.Structure):
    """idc_dist_query: one suggestion query; (y, x) = (-1, -1) is the empty query."""
    _fields_ = [("img", ctypes.c_int32), ("y", ctypes.c_int32), ("x", ctypes.c_int32), ("seed", ctypes.c_uint32)]


class DistTaps(ctypes.Structure):
    """idc_dist_taps: what idc_forward_async_dist reads off the distribution behind the network."""
    _fields_ = [("n_peaks", ctypes.c_int32), ("radius", ctypes.c_int32), ("flags", ctypes.c_uint32),
                ("peaks", ctypes.c_void_p), ("peak_ent", ctypes.c_void_p), ("entropy", ctypes.c_void_p),
                ("n_queries", ctypes.c_int32), ("queries", ctypes.POINTER(DistQuery)),
                ("K", ctypes.c_int32), ("N", ctypes.c_int32), ("seed", ctypes.c_uint32), ("centres", ctypes.c_void_p),
                ("sugg_centres", ctypes.c_void_p), ("sugg_conf", ctypes.c_void_p)]


class DistScoreSpec(ctypes.Structure):
    """idc_dist_score_spec: neighbours and sigma of the soft encoding, and up to 8 top-k thresholds."""
    _fields_ = [("nn", ctypes.c_int32), ("sigma", ctypes.c_float), ("n_ranks", ctypes.c_int32), ("ranks", ctypes.c_int32 * 8)]


class DistScoreOut(ctypes.Structure):
    """idc_dist_score_out: where the score's results go; every pointer but xent may be NULL."""
    _fields_ = [("xent", ctypes.c_void_p), ("hits", ctypes.c_void_p), ("xent_map", ctypes.c_void_p), ("rank_map", ctypes.c_void_p),
                ("target", ctypes.c_void_p), ("truth_ab", ctypes.c_void_p)]


class LayerInfo(ctypes.Structure):
    _fields_ = [("name", ctypes.c_char * 32), ("kernel", ctypes.c_char * 48), ("flops", ctypes.c_double),
                ("min_bytes", ctypes.c_double), ("launches", ctypes.c_int)]


class RangeInfo(ctypes.Structure):
    """idc_range_info: one layer's sticky range-audit record."""
    _fields_ = [("name", ctypes.c_char * 32), ("storage", ctypes.c_int), ("parts", ctypes.c_int), ("act_exp", ctypes.c_int),
                ("max_abs", ctypes.c_float), ("n_values", ctypes.c_uint64), ("n_saturated", ctypes.c_uint64),
                ("n_tiny", ctypes.c_uint64), ("n_nonfinite", ctypes.c_uint64)]


_lib = None


def load():
    """Load the shared library once; raise loudly if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libideepcolor_hip.so not found at %s -- the HIP extension is not built and there is "
            "no CPU fallback.  Run `python -c \"import __graft_entry__ as g; g.build()\"` "
            "(needs hipcc, cross-compiles for gfx950 without a GPU)." % LIB_PATH)
    lib = ctypes.CDLL(LIB_PATH)
    c_float_p = ctypes.POINTER(ctypes.c_float)
    vp, ci, cf, csz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_size_t

    def proto(name, restype, argtypes):
        fn = getattr(lib, name)
        fn.restype = restype
        fn.argtypes = argtypes

    proto("idc_version", ci, [])
    proto("idc_set_tile_policy", ci, [ci])
    proto("idc_set_option", ci, [ctypes.c_char_p, ci])
    proto("idc_set_splitk_policy", ci, [ci])
    proto("idc_device_count", ci, [])
    proto("idc_last_error", ctypes.c_char_p, [vp])
    proto("idc_create", ci, [ci, ci, ci, ci, ci, ctypes.c_uint, ctypes.POINTER(vp)])
    proto("idc_destroy", ci, [vp])
    proto("idc_set_io_scales", ci, [vp, cf, cf, cf, cf])
    proto("idc_weights_blob_bytes", csz, [ci, ctypes.c_uint])
    proto("idc_pack_weights", ci, [ci, ctypes.c_uint, ctypes.POINTER(TensorDesc), ci, vp, csz])
    proto("idc_set_weights_host", ci, [vp, vp, csz])
    proto("idc_set_weights_device", ci, [vp, vp, csz, ci])
    proto("idc_load_weights", ci, [vp, ctypes.POINTER(TensorDesc), ci])
    proto("idc_weights_device_ptr", vp, [vp])
    proto("idc_forward", ci, [vp, ci, c_float_p, c_float_p, c_float_p, cf, c_float_p])
    proto("idc_forward_device", ci, [vp, ci, vp, vp, vp, cf, vp, ci])
    proto("idc_forward_dist", ci, [vp, ci, c_float_p, c_float_p, c_float_p, cf, c_float_p, c_float_p])
    proto("idc_global_histogram", ci, [vp, ci, vp, c_float_p, c_float_p, c_float_p])
    proto("idc_lab2rgb", ci, [vp, ci, c_float_p, c_float_p, vp, vp])
    proto("idc_forward_rgb", ci, [vp, ci, c_float_p, c_float_p, c_float_p, cf, cf, c_float_p, vp, vp])
    proto("idc_forward_rgb_lazy", ci, [vp, ci, c_float_p, c_float_p, c_float_p, cf, cf, vp])
    proto("idc_fetch_outputs", ci, [vp, ci, c_float_p, vp])
    proto("idc_forward_dist313", ci, [vp, ci, c_float_p, c_float_p, c_float_p, cf, c_float_p, c_float_p, c_float_p])
    proto("idc_set_dist_temperature", ci, [vp, cf])
    proto("idc_set_global_hints", ci, [vp, ci, c_float_p, c_float_p])
    proto("idc_clear_global_hints", ci, [vp])
    proto("idc_sync", ci, [vp])
    proto("idc_stream", vp, [vp])
    proto("idc_num_layers", ci, [vp])
    proto("idc_layer_info_get", ci, [vp, ci, ctypes.POINTER(LayerInfo)])
    proto("idc_set_profiling", ci, [vp, ci])
    proto("idc_layer_times_ms", ci, [vp, c_float_p, ci])
    proto("idc_layer_times_stats", ci, [vp, c_float_p, c_float_p, c_float_p, ci])
    proto("idc_get_activation", ci, [vp, ctypes.c_char_p, ci, c_float_p, csz,
                                     ctypes.POINTER(ci), ctypes.POINTER(ci), ctypes.POINTER(ci)])
    proto("idc_op_conv2d", ci, [ci, ci, ci, ci, ci, ci, c_float_p, ci, ci, ci, ci, c_float_p, c_float_p, ci,
                                c_float_p, c_float_p, c_float_p, c_float_p])
    proto("idc_op_deconv4x4s2", ci, [ci, ci, ci, ci, ci, ci, c_float_p, ci, c_float_p, c_float_p, ci,
                                     c_float_p, c_float_p])
    proto("idc_op_deconv_shortcut", ci, [ci, ci, ci, ci, ci, ci, c_float_p, ci, c_float_p, c_float_p, ci, c_float_p,
                                         c_float_p, c_float_p, ci, c_float_p])
    proto("idc_op_last_kernel", ci, [ctypes.c_char_p, ci])
    proto("idc_grid_last", ci, [ctypes.c_char_p, ctypes.POINTER(ctypes.c_longlong), ctypes.POINTER(ci)])
    proto("idc_grid_tag", ctypes.c_char_p, [ci])
    proto("idc_set_image_l", ci, [vp, ci, c_float_p])
    proto("idc_set_hints", ci, [vp, ci, ci, ctypes.POINTER(Hint), ci, cf])
    proto("idc_get_hint_planes", ci, [vp, ci, c_float_p, c_float_p])
    proto("idc_forward_resident", ci, [vp, ci, cf, cf, c_float_p, vp, vp])
    proto("idc_dist_bins", ci, [vp])
    proto("idc_keep_dist", ci, [vp, ci])
    proto("idc_dist_at", ci, [vp, ci, ci, ci, c_float_p])
    proto("idc_get_dist", ci, [vp, ci, c_float_p])
    proto("idc_suggest_colors", ci, [vp, ci, ci, ci, ci, ci, ctypes.c_uint, c_float_p, vp, vp, vp])
    proto("idc_dist_entropy", ci, [vp, ci, c_float_p])
    proto("idc_dist_decode", ci, [vp, ci, ci, cf, c_float_p, c_float_p, c_float_p])
    proto("idc_stream_wait", ci, [vp, vp])
    proto("idc_stream_signal", ci, [vp, vp])
    proto("idc_alloc_host", vp, [csz])
    proto("idc_free_host", ci, [vp])
    proto("idc_forward_async", ci, [vp, ci, ci, c_float_p, c_float_p, c_float_p, cf, c_float_p])
    proto("idc_wait", ci, [vp, ci])
    proto("idc_pipeline_times", ci, [vp, ci, c_float_p])
    proto("idc_comm_unique_id", ci, [vp])
    proto("idc_broadcast_weights", ci, [vp, vp, ci, ci, ci])
    proto("idc_upsample_lab2rgb", ci, [vp, ci, ci, ci, ci, ci, vp, vp])
    proto("idc_set_image_rgb", ci, [vp, ci, ci, ci, ci, vp, cf, ctypes.c_uint, vp, vp])
    proto("idc_fullres_rgb", ci, [vp, ci, ci, ci, ci, vp])
    proto("idc_forward_async_rgb", ci, [vp, ci, ci, ci, ci, vp, vp, vp, ci, cf, cf, cf, ctypes.c_uint, vp, vp])
    proto("idc_global_stats_rgb", ci, [vp, ci, ctypes.POINTER(RefImage), c_float_p, c_float_p, c_float_p])
    proto("idc_set_global_refs", ci, [vp, ci, ci, ci, ctypes.POINTER(RefImage), vp, c_float_p, cf, ctypes.c_uint])
    proto("idc_forward_async_rgb_ref", ci, [vp, ci, ci, ci, ci, vp, vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                            ci, ctypes.POINTER(RefImage), vp, c_float_p, cf, ctypes.c_uint, vp, vp])
    proto("idc_forward_async_images", ci, [vp, ci, ci, ctypes.POINTER(RefImage), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                           ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp])
    proto("idc_reveal_hints", ci, [vp, ci, ci, ctypes.POINTER(Hint), cf, c_float_p])
    proto("idc_forward_async_eval", ci, [vp, ci, ci, ctypes.POINTER(RefImage), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                         ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp, vp, vp])
    proto("idc_dist_peaks", ci, [vp, ci, ci, ci, ctypes.c_uint, vp, vp])
    proto("idc_suggest_colors_batch", ci, [vp, ci, ctypes.POINTER(DistQuery), ci, ci, c_float_p, vp, vp])
    proto("idc_forward_async_dist", ci, [vp, ci, ci, ctypes.POINTER(RefImage), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                         ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp, vp, vp, ctypes.POINTER(DistTaps)])
    proto("idc_dist_score", ci, [vp, ci, ctypes.POINTER(DistScoreSpec), c_float_p, ctypes.POINTER(DistScoreOut)])
    proto("idc_forward_async_dist_score", ci, [vp, ci, ci, ctypes.POINTER(RefImage), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                               ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp, vp, vp, ctypes.POINTER(DistTaps),
                                               ctypes.POINTER(DistScoreSpec), c_float_p, ctypes.POINTER(DistScoreOut)])
    proto("idc_gamut_map", ci, [vp, ci, vp, ci, ci, vp, vp, vp])
    proto("idc_snap_colors", ci, [vp, ci, vp, vp, vp, vp, vp])
    proto("idc_set_joint_upsample", ci, [vp, ci, ctypes.c_double, ctypes.c_double])
    proto("idc_fullres_ab", ci, [vp, ci, ci, ci, vp])
    proto("idc_set_image_gray", ci, [vp, ci, ci, ci, ci, ci, vp, cf, ctypes.c_uint, vp, vp])
    proto("idc_fullres_rgb16", ci, [vp, ci, ci, ci, vp])
    proto("idc_forward_async_gray", ci, [vp, ci, ci, ci, ctypes.POINTER(GrayImage), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                         ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp, ctypes.POINTER(DistTaps)])
    proto("idc_set_hints_layer", ci, [vp, ci, ci, vp, ci, cf, ctypes.POINTER(HintLayer), ci, ci, vp])
    proto("idc_forward_async_layers", ci, [vp, ci, ci, ci, vp, ctypes.POINTER(BatchLayers), vp, vp, ci, cf, cf, cf, ctypes.c_uint,
                                           ctypes.POINTER(BatchRefs), ctypes.POINTER(vp), vp])
    proto("idc_ycc420_bytes", csz, [ci, ci])
    proto("idc_set_batch_output", ci, [vp, ci, ci])
    proto("idc_fullres_ycc", ci, [vp, ci, ci, ci, ci, ci, ci, vp])
    proto("idc_rgb_to_ycc420", ci, [vp, ci, ctypes.POINTER(RefImage), ci, ci, ctypes.POINTER(vp)])
    proto("idc_set_temporal_filter", ci, [vp, ci, ctypes.c_double, ctypes.c_double, ci, ctypes.c_double])
    proto("idc_temporal_reset", ci, [vp])
    proto("idc_temporal_info", ci, [vp, ci, vp, vp])
    proto("idc_temporal_apply", ci, [vp, ci, vp, vp, vp, vp, vp])
    proto("idc_temporal_state", ci, [vp, vp, vp, vp])
    proto("idc_set_temporal_motion", ci, [vp, ci, ci, ctypes.c_double])
    proto("idc_temporal_vectors", ci, [vp, ci, vp])
    proto("idc_set_hint_tracking", ci, [vp, ci, ci, ctypes.c_double])
    proto("idc_tracked_hints", ci, [vp, ci, vp, vp, vp])
    proto("idc_track_hints_apply", ci, [vp, ci, vp, vp, vp, vp, vp, vp, vp])
    proto("idc_set_batch_upsample", ci, [vp, ci])
    proto("idc_set_ingest_filter", ci, [vp, ci])
    proto("idc_set_range_audit", ci, [vp, ci])
    proto("idc_range_reset", ci, [vp])
    proto("idc_range_report", ci, [vp, ci, ctypes.POINTER(RangeInfo)])
    proto("idc_pack_weights_ex", ci, [ci, ctypes.c_uint, ctypes.POINTER(TensorDesc), ci, ctypes.POINTER(ci), ci, vp, csz])
    proto("idc_load_weights_ex", ci, [vp, ctypes.POINTER(TensorDesc), ci, ctypes.POINTER(ci), ci])
    _lib = lib
    return lib


def check(status, handle=None):
    if status != IDC_OK:
        msg = load().idc_last_error(handle)
        raise IdcError(status, msg.decode("utf-8", "replace") if msg else "")
    return status
