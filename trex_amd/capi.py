"""ctypes binding of libtrexhip.so (include/trexhip.h) for the Python-side callers in this repo
(tests, bench.py).  The C ABI is the product boundary; this module is only plumbing.

There is NO CPU fallback: if the HIP library is missing or a call fails, this raises.
"""
import collections
import ctypes as C
import os
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("TREXHIP_LIB_PATH") or os.path.join(_HERE, "libtrexhip.so")      # (the override: another build of the library, for A/B runs)
_LIB = None

RUN_DTYPE = np.dtype([("x0", "<u2"), ("x1", "<u2"), ("y", "<u2"), ("pad", "<u2")])
BLOB_DTYPE = np.dtype([
    ("run_begin", "<u4"), ("n_runs", "<u4"), ("pix_begin", "<u4"), ("n_pixels", "<u4"),
    ("x0", "<u2"), ("y0", "<u2"), ("x1", "<u2"), ("y1", "<u2"),
    ("bid", "<u4"), ("px_min_max", "<u4"), ("parent", "<u4"), ("flags", "<u4"),
    ("m10", "<u8"), ("m01", "<u8"), ("m20", "<u8"), ("m11", "<u8"), ("m02", "<u8"),
    ("sp", "<u8"), ("spx", "<u8"), ("spy", "<u8"),
])
INFO_DTYPE = np.dtype([
    ("n_blobs", "<u4"), ("n_runs", "<u4"), ("n_pixels", "<u4"),
    ("blob_begin", "<u4"), ("run_begin", "<u4"), ("pix_begin", "<u4"),
    ("n_raw_runs", "<u4"), ("n_raw_blobs", "<u4"), ("flags", "<u4"), ("reserved", "<u4", (3,)),
])
assert BLOB_DTYPE.itemsize == 104 and RUN_DTYPE.itemsize == 8 and INFO_DTYPE.itemsize == 48

CNN_FP32, CNN_BF16X6, CNN_BF16X3, CNN_FP16X3 = 0, 1, 2, 3
STAGE_ROWS, STAGE_SEGMENT_ALL, STAGE_CONV2, STAGE_CONV3, STAGE_CNN_ALL, STAGE_CROPS, STAGE_POSTURE = 0, 1, 2, 3, 4, 5, 6
STAGE_UPLOAD_COPY, STAGE_UPLOAD_DMA = 8, 9       # host-input legs (per frame): pageable -> pinned copy (host ms), DMA (event ms)
STAGE_PREPARE = 10                               # the launches of identify_prepare_device (outside CONV2 / CONV3 where a call was prepared)


class Params(C.Structure):
    _fields_ = [
        ("device", C.c_int32), ("width", C.c_int32), ("height", C.c_int32),
        ("max_batch", C.c_int32), ("max_runs", C.c_int32), ("max_blobs", C.c_int32), ("max_pixels", C.c_int32),
        ("threshold", C.c_int32), ("threshold_maximum", C.c_int32),
        ("enable_difference", C.c_int32), ("absolute_difference", C.c_int32),
        ("image_invert", C.c_int32), ("inclusive", C.c_int32), ("zero_is_background", C.c_int32),
        ("connectivity", C.c_int32), ("dilation_size", C.c_int32), ("use_closing", C.c_int32),
        ("closing_size", C.c_int32), ("n_ranges", C.c_int32),
        ("cm_per_pixel", C.c_double), ("ranges", C.c_double * 16),
        ("pixel_encoding", C.c_int32),
        # not implemented: any non-zero value makes trexhip_create return TREXHIP_E_UNSUPPORTED
        ("image_adjust", C.c_int32), ("blur_difference", C.c_int32), ("equalize_histogram", C.c_int32), ("correct_luminance", C.c_int32),
        ("use_adaptive_threshold", C.c_int32), ("device_color_reduce", C.c_int32), ("reserved_", C.c_int32 * 1),
    ]


class LiveParams(C.Structure):
    _fields_ = [("threshold", C.c_int32), ("threshold_maximum", C.c_int32), ("inclusive", C.c_int32),
                ("enable_difference", C.c_int32), ("absolute_difference", C.c_int32), ("image_invert", C.c_int32), ("zero_is_background", C.c_int32),
                ("n_ranges", C.c_int32), ("cm_per_pixel", C.c_double), ("ranges", C.c_double * 16)]


class PostureParams(C.Structure):
    _fields_ = [("outline_resample", C.c_float), ("outline_smooth_samples", C.c_int32), ("outline_smooth_step", C.c_int32),
                ("outline_approximate", C.c_int32), ("outline_curvature_range_ratio", C.c_float),
                ("midline_walk_offset", C.c_float), ("max_points", C.c_int32),
                ("posture_closing_steps", C.c_int32), ("peak_mode", C.c_int32), ("posture_direction_smoothing", C.c_int32)]


class MidlineParams(C.Structure):
    _fields_ = [("midline_resolution", C.c_int32), ("midline_stiff_percentage", C.c_float), ("midline_invert", C.c_int32),
                ("midline_start_with_head", C.c_int32)]


class SplitParams(C.Structure):
    _fields_ = [("track_threshold", C.c_int32), ("track_posture_threshold", C.c_int32), ("calculate_posture", C.c_int32), ("algorithm", C.c_int32),
                ("blob_split_max_shrink", C.c_float), ("blob_split_global_shrink_limit", C.c_float), ("n_ranges", C.c_int32), ("reserved_", C.c_int32),
                ("size_ranges", C.c_double * 16)]


class PrefilterParams(C.Structure):
    _fields_ = [("track_threshold", C.c_int32), ("method", C.c_int32), ("track_threshold_2", C.c_int32), ("n_ranges", C.c_int32),
                ("threshold_ratio_range", C.c_float * 2), ("size_ranges", C.c_double * 16)]


class PrefilterTables(C.Structure):
    _fields_ = [("d_include_points", C.c_void_p), ("d_include_offsets", C.c_void_p), ("n_include_shapes", C.c_int32), ("n_include_points", C.c_int32),
                ("d_ignore_points", C.c_void_p), ("d_ignore_offsets", C.c_void_p), ("n_ignore_shapes", C.c_int32), ("n_ignore_points", C.c_int32),
                ("d_ignore_bdx", C.c_void_p), ("d_ignore_bdx_offsets", C.c_void_p), ("n_ignore_bdx", C.c_int32), ("reserved_", C.c_int32),
                ("d_second_count", C.c_void_p)]


# trexhip_prefilter_device: d_decision values and the library's numbering of pv::FilterReason
DECISION_COMMITTED, DECISION_BIG, DECISION_FILTERED, DECISION_NONE = 0, 1, 16, 255
FILTER_OUTSIDE_INCLUDE, FILTER_INSIDE_IGNORE, FILTER_BDX_IGNORED, FILTER_OUTSIDE_RANGE, FILTER_SECOND_THRESHOLD = 0, 1, 2, 3, 4

class VfParams(C.Structure):
    _fields_ = [("max_d", C.c_double), ("max_distance", C.c_double), ("max_points", C.c_int32), ("max_tess_points", C.c_int32)]


# trexhip_visual_field_device: one individual of one frame, one VisualField object; outputs are [n_observers][2 eyes][VF_LAYERS][VF_RESOLUTION]
VF_ENTRY_DTYPE = np.dtype([("id", "<i4"), ("posture_row", "<i4"), ("pos_x", "<f4"), ("pos_y", "<f4"), ("flags", "<i4"), ("reserved", "<i4")])
VF_OBSERVER_DTYPE = np.dtype([("frame", "<i4"), ("entry", "<i4"), ("eye_x", "<f8", (2,)), ("eye_y", "<f8", (2,)), ("eye_angle", "<f8", (2,))])
assert VF_ENTRY_DTYPE.itemsize == 24 and VF_OBSERVER_DTYPE.itemsize == 56
VF_RESOLUTION, VF_LAYERS = 512, 2
VF_CHUNK_RECORDS, VF_LDS_RECORDS = 512, 1024      # TREXHIP_VF_CHUNK_RECORDS / TREXHIP_VF_LDS_RECORDS: records per compute step of a workgroup, records waiting in LDS
VF_OUTPUTS = ("depth", "ids", "points", "fov", "head_distance", "status")

SPLIT_INFO_DTYPE = np.dtype([("threshold", "<i4"), ("effective_threshold", "<i4"), ("status", "<i4"), ("initial_action", "<i4"), ("n_result", "<i4"),
                             ("n_evaluated", "<i4"), ("min_pixel", "<i4"), ("max_pixel", "<i4"), ("first_size", "<f4"), ("reserved_", "<f4"),
                             ("min_size_bound", "<f8")])
MIDLINE_INFO_DTYPE = np.dtype([("status", "<i4"), ("n", "<i4"), ("len", "<f4"), ("angle", "<f4"), ("offx", "<f4"), ("offy", "<f4"),
                               ("reserved", "<i4", (2,))])
POSTURE_INFO_DTYPE = np.dtype([("status", "<i4"), ("n_outline", "<i4"), ("n_segments", "<i4"), ("tail_index", "<i4"),
                               ("head_index", "<i4"), ("n_traced", "<i4"), ("reserved", "<i4", (2,))])


class BatchResult(C.Structure):
    _fields_ = [
        ("n_frames", C.c_int32), ("total_blobs", C.c_uint32), ("total_runs", C.c_uint32), ("total_pixels", C.c_uint32),
        ("frames", C.c_void_p), ("blobs", C.c_void_p), ("runs", C.c_void_p), ("pixels", C.c_void_p),
        ("pixel_channels", C.c_uint32), ("reserved_", C.c_uint32),
    ]


ENC_GRAY, ENC_R3G3B2, ENC_RGB8 = 0, 1, 2        # pixel_encoding, order of cmn::meta_encoding_t
FRAME_OVERFLOW_RUNS, FRAME_OVERFLOW_OUTPUT, FRAME_MALFORMED = 1, 2, 4       # trexhip_frame_info.flags


class DeviceView(C.Structure):
    _fields_ = [("frames", C.c_void_p), ("blobs", C.c_void_p), ("runs", C.c_void_p), ("pixels", C.c_void_p),
                ("totals", C.c_void_p), ("blob_frame", C.c_void_p)]


class TrexHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libtrexhip error {code}: {msg}")
        self.code = code
        self.frames = None            # Segmenter.fetch on a loaded batch with a malformed frame: the per-frame results all the same


# every symbol include/trexhip.h declares (tests check the library exports all of them)
class TrainParams(C.Structure):
    _fields_ = [("max_batch", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("bn_momentum", C.c_float), ("dropout", C.c_float), ("precision", C.c_int32), ("seed", C.c_uint64)]


class AugmentParams(C.Structure):
    _fields_ = [("degrees", C.c_float), ("translate_x", C.c_float), ("translate_y", C.c_float), ("brightness_lo", C.c_float), ("brightness_hi", C.c_float),
                ("contrast_lo", C.c_float), ("contrast_hi", C.c_float), ("saturation_lo", C.c_float), ("saturation_hi", C.c_float),
                ("hue_lo", C.c_float), ("hue_hi", C.c_float), ("seed", C.c_uint64)]


# trexhip_augment_draw: one sample's augmentation; order = 2 bits per position, first operation lowest (0 brightness, 1 contrast, 2 saturation, 3 hue)
AUGMENT_DRAW_DTYPE = np.dtype([("angle", "<f4"), ("tx", "<i4"), ("ty", "<i4"), ("brightness", "<f4"), ("contrast", "<f4"), ("saturation", "<f4"),
                               ("hue", "<f4"), ("order", "<i4")])
assert AUGMENT_DRAW_DTYPE.itemsize == 32
AUGMENT_IDENTITY_ORDER = 0xE4


class UniquenessResult(C.Structure):
    _fields_ = [("good_frames", C.c_uint32), ("bad_frames", C.c_uint32), ("good_ratio", C.c_float), ("mean_unique", C.c_float), ("mean_unique_raw", C.c_float)]


class ValidationMetrics:
    """What Segmenter.validation_metrics returns.  With targets: confusion (uint32 [classes][classes], row = target, column = np.argmax) and
    per_class_accuracy (float64 [classes]: diagonal / row sum, plot_comparison_raw's column 3; a class without samples is left out of the
    division and stays 0, as the reference's `continue` leaves it, visual_recognition_torch.py:409-416 -- never NaN).  With frame ranges: good_frames, bad_frames, good_ratio,
    mean_unique, mean_unique_raw, unique_percent / unique_percent_raw (float32 [n_frames]) and uniqueness_per_class (float32 [classes]) of
    Accumulation::calculate_uniqueness.  What was not asked for is None."""
    __slots__ = ("confusion", "per_class_accuracy", "good_frames", "bad_frames", "good_ratio", "mean_unique", "mean_unique_raw",
                 "unique_percent", "unique_percent_raw", "uniqueness_per_class")

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


class ClassAverages:
    """What Segmenter.class_averages returns, per dense key 0..n_ids-1: samples (float32 [n_ids], the row count as VINetwork::paverages counts
    it), values (float32 [n_ids][classes], the averaged rows; all zero for a key without rows), and the arg-max scan of
    Accumulation::check_additional_range over every averaged row: max_index (int32 [n_ids], -1 = nothing above 0) and max_p (float32 [n_ids])."""
    __slots__ = ("samples", "values", "max_index", "max_p")

    def __init__(self, samples, values, max_index, max_p):
        self.samples, self.values, self.max_index, self.max_p = samples, values, max_index, max_p


class VisualFieldResult:
    """What Segmenter.visual_field returns: depth (float64), ids (int32), points (float32 [..., 2]), fov (uint8), head_distance (float64), each
    [n_observers][2 eyes][2 layers][512] -- per eye the members _depth, _visible_ids, _visible_points, _fov, _visible_head_distance of
    VisualField::eye -- and status (int32 [n_observers]: 0 ok, 1 the observer has no usable posture, 2 an entry of its frame exceeded
    max_tess_points).  What was not asked for is None."""
    __slots__ = VF_OUTPUTS

    def __init__(self):
        for k in self.__slots__:
            setattr(self, k, None)


TrackletLabels = collections.namedtuple("TrackletLabels", "counts rows label share skipped")


SYMBOLS = [
    "trexhip_abi_version", "trexhip_network_channels", "trexhip_network_image_size", "trexhip_network_version", "trexhip_network_blob_bytes", "trexhip_identify_chunk_crops", "trexhip_comm_unique_id", "trexhip_comm_create", "trexhip_comm_destroy", "trexhip_comm_rank", "trexhip_comm_world", "trexhip_comm_gather_device", "trexhip_comm_gather_device_on", "trexhip_comm_count_ranks", "trexhip_last_error", "trexhip_default_params", "trexhip_create", "trexhip_destroy",
    "trexhip_set_stream", "trexhip_get_live_params", "trexhip_update_params", "trexhip_set_background", "trexhip_set_background_device", "trexhip_set_background_color", "trexhip_set_background_color_device", "trexhip_generate_average_device", "trexhip_get_background", "trexhip_segment_device",
    "trexhip_segment", "trexhip_segment_color", "trexhip_segment_color_device", "trexhip_rethreshold_device", "trexhip_rethreshold_per_blob_device", "trexhip_fetch_rethreshold", "trexhip_fetch", "trexhip_device_view_get", "trexhip_synchronize",
    "trexhip_profile_enable", "trexhip_profile_read", "trexhip_profile_reset",
    "trexhip_default_posture_params", "trexhip_posture_device", "trexhip_posture_auto_device", "trexhip_pack_frames_v6_device", "trexhip_crops_device", "trexhip_pixel_channels", "trexhip_device_alloc", "trexhip_device_free", "trexhip_copy_to_host", "trexhip_copy_to_device", "trexhip_crops_transformed_device", "trexhip_crops_posture_device", "trexhip_default_midline_params", "trexhip_midline_device", "trexhip_midline_movement_device", "trexhip_default_split_params", "trexhip_split_search_device", "trexhip_export_id_table_device", "trexhip_export_id_table_ex_device", "trexhip_load_weights", "trexhip_set_identity_precision", "trexhip_num_classes", "trexhip_identify_device", "trexhip_identify", "trexhip_identify_guard_stats", "trexhip_identify_skip_stats", "trexhip_identify_skip3_stats", "trexhip_identify_skip3x_stats", "trexhip_identify_skip3_ran", "trexhip_identify_skipx_stats", "trexhip_identify_bgrow_stats", "trexhip_identify_fc1_stats",
    "trexhip_weight_blob_bytes", "trexhip_trainer_create", "trexhip_trainer_destroy", "trexhip_trainer_set_lr", "trexhip_trainer_steps", "trexhip_trainer_image_size", "trexhip_trainer_version", "trexhip_trainer_keep_mask_bytes", "trexhip_train_step_device", "trexhip_train_step", "trexhip_train_eval_device", "trexhip_train_eval", "trexhip_trainer_read", "trexhip_trainer_export",
    "trexhip_default_augment_params", "trexhip_augment_device",
    "trexhip_train_predict_device", "trexhip_validation_metrics_device", "trexhip_class_averages_device",
    "trexhip_lzo1x_bound", "trexhip_lzo1x_compress", "trexhip_pv_write_frames",
    "trexhip_load_frames_v6_device", "trexhip_lzo1x_decompress", "trexhip_pv_read_frames",
    "trexhip_default_prefilter_params", "trexhip_prefilter_device",
    "trexhip_default_vf_params", "trexhip_visual_field_device",
    "trexhip_categorize_load_weights", "trexhip_categorize_info", "trexhip_categorize_blob_bytes", "trexhip_categorize_device", "trexhip_categorize",
    "trexhip_tracklet_labels_device", "trexhip_tracklet_medians_device",
    "trexhip_identify_prepare_device", "trexhip_fetch_begin", "trexhip_fetch_wait", "trexhip_identify_prepare_stats",
]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise TrexHipError(-1, f"{LIB_PATH} is missing: run __graft_entry__.build() (make -C trex_amd/csrc)")
        L = C.CDLL(LIB_PATH)
        L.trexhip_last_error.restype = C.c_char_p
        L.trexhip_default_params.argtypes = [C.POINTER(Params), C.c_int32, C.c_int32]
        L.trexhip_default_params.restype = None
        L.trexhip_create.argtypes = [C.POINTER(Params), C.POINTER(C.c_void_p)]
        L.trexhip_destroy.argtypes = [C.c_void_p]
        L.trexhip_destroy.restype = None
        L.trexhip_set_stream.argtypes = [C.c_void_p, C.c_void_p]
        L.trexhip_get_live_params.argtypes = [C.c_void_p, C.POINTER(LiveParams)]
        L.trexhip_update_params.argtypes = [C.c_void_p, C.POINTER(LiveParams)]
        L.trexhip_set_background.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.trexhip_set_background_device.argtypes = [C.c_void_p, C.c_void_p]
        L.trexhip_set_background_color.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.trexhip_set_background_color_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.trexhip_generate_average_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
        L.trexhip_get_background.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.trexhip_segment_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.trexhip_segment.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32]
        L.trexhip_segment_color.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.trexhip_segment_color_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
        L.trexhip_rethreshold_device.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]
        L.trexhip_rethreshold_per_blob_device.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.trexhip_fetch_rethreshold.argtypes = [C.c_void_p, C.POINTER(BatchResult)]
        L.trexhip_fetch.argtypes = [C.c_void_p, C.POINTER(BatchResult)]
        L.trexhip_fetch_begin.argtypes = [C.c_void_p, C.POINTER(BatchResult)]
        L.trexhip_fetch_wait.argtypes = [C.c_void_p]
        L.trexhip_device_view_get.argtypes = [C.c_void_p, C.POINTER(DeviceView)]
        L.trexhip_synchronize.argtypes = [C.c_void_p]
        L.trexhip_profile_enable.argtypes = [C.c_void_p, C.c_int32]
        L.trexhip_profile_read.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_double), C.POINTER(C.c_int64)]
        L.trexhip_profile_reset.argtypes = [C.c_void_p]
        L.trexhip_default_midline_params.argtypes = [C.POINTER(MidlineParams)]
        L.trexhip_default_midline_params.restype = None
        L.trexhip_midline_device.argtypes = [C.c_void_p, C.POINTER(MidlineParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_midline_movement_device.argtypes = [C.c_void_p, C.POINTER(MidlineParams), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_default_split_params.argtypes = [C.POINTER(SplitParams)]
        L.trexhip_default_split_params.restype = None
        L.trexhip_split_search_device.argtypes = [C.c_void_p, C.POINTER(SplitParams), C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.trexhip_crops_posture_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32]
        L.trexhip_default_posture_params.argtypes = [C.POINTER(PostureParams)]
        L.trexhip_default_posture_params.restype = None
        L.trexhip_posture_device.argtypes = [C.c_void_p, C.c_int32, C.POINTER(PostureParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_posture_auto_device.argtypes = [C.c_void_p, C.POINTER(PostureParams), C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_crops_transformed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_float, C.c_int32]
        L.trexhip_crops_device.argtypes = [C.c_void_p, C.c_void_p] + [C.c_int32] * 5
        L.trexhip_export_id_table_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_int32]
        L.trexhip_export_id_table_ex_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        L.trexhip_load_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.trexhip_num_classes.argtypes = [C.c_void_p]
        L.trexhip_network_channels.argtypes = [C.c_void_p]
        L.trexhip_network_image_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.trexhip_network_version.argtypes = [C.c_void_p]
        L.trexhip_network_blob_bytes.argtypes = [C.c_int32] * 5; L.trexhip_network_blob_bytes.restype = C.c_size_t
        L.trexhip_identify_chunk_crops.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.trexhip_pack_frames_v6_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.trexhip_lzo1x_bound.argtypes = [C.c_size_t]; L.trexhip_lzo1x_bound.restype = C.c_size_t
        L.trexhip_lzo1x_compress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.trexhip_pv_write_frames.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
        L.trexhip_load_frames_v6_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.trexhip_lzo1x_decompress.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.trexhip_pv_read_frames.argtypes = [C.c_void_p, C.c_size_t, C.c_uint64, C.c_void_p, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_size_t)]
        L.trexhip_comm_unique_id.argtypes = [C.c_void_p]
        L.trexhip_comm_create.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
        L.trexhip_comm_destroy.argtypes = [C.c_void_p]
        L.trexhip_comm_destroy.restype = None
        L.trexhip_comm_rank.argtypes = [C.c_void_p]
        L.trexhip_comm_world.argtypes = [C.c_void_p]
        L.trexhip_comm_gather_device.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.trexhip_comm_gather_device_on.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        L.trexhip_comm_count_ranks.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.trexhip_set_identity_precision.argtypes = [C.c_void_p, C.c_int32]
        L.trexhip_identify_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        L.trexhip_identify_prepare_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32]
        L.trexhip_identify_prepare_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.trexhip_identify_guard_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify_skip_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.trexhip_identify_skipx_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify_bgrow_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify_skip3x_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify_skip3_ran.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_identify_skip3_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]
        L.trexhip_identify_fc1_stats.argtypes = [C.c_void_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
        L.trexhip_weight_blob_bytes.argtypes = [C.c_int32, C.c_int32]
        L.trexhip_weight_blob_bytes.restype = C.c_size_t
        L.trexhip_trainer_create.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(TrainParams), C.POINTER(C.c_void_p)]
        L.trexhip_trainer_destroy.argtypes = [C.c_void_p]
        L.trexhip_trainer_destroy.restype = None
        L.trexhip_trainer_set_lr.argtypes = [C.c_void_p, C.c_float]
        L.trexhip_trainer_steps.argtypes = [C.c_void_p]
        L.trexhip_trainer_steps.restype = C.c_int64
        L.trexhip_trainer_image_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.trexhip_trainer_version.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        L.trexhip_trainer_keep_mask_bytes.argtypes = [C.c_void_p, C.c_int32]
        L.trexhip_trainer_keep_mask_bytes.restype = C.c_size_t
        L.trexhip_train_step_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        L.trexhip_train_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        L.trexhip_train_eval_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        L.trexhip_train_eval.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.POINTER(C.c_float), C.POINTER(C.c_int32)]
        L.trexhip_trainer_read.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t]
        L.trexhip_trainer_export.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.trexhip_default_augment_params.argtypes = [C.POINTER(AugmentParams), C.c_int32, C.c_int32]
        L.trexhip_default_augment_params.restype = None
        L.trexhip_augment_device.argtypes = [C.c_void_p, C.POINTER(AugmentParams), C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_int32, C.c_void_p, C.c_int32, C.c_uint64, C.c_void_p, C.c_void_p]
        L.trexhip_train_predict_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.trexhip_validation_metrics_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                                        C.POINTER(UniquenessResult), C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_class_averages_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_device_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]
        L.trexhip_device_free.argtypes = [C.c_void_p, C.c_void_p]
        L.trexhip_copy_to_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.trexhip_copy_to_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
        L.trexhip_default_prefilter_params.argtypes = [C.POINTER(PrefilterParams)]
        L.trexhip_default_prefilter_params.restype = None
        L.trexhip_prefilter_device.argtypes = [C.c_void_p, C.POINTER(PrefilterParams), C.POINTER(PrefilterTables), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_default_vf_params.argtypes = [C.c_void_p, C.POINTER(VfParams)]
        L.trexhip_default_vf_params.restype = None
        L.trexhip_visual_field_device.argtypes = [C.c_void_p, C.POINTER(VfParams), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                                                  C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_categorize_load_weights.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
        L.trexhip_categorize_info.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        L.trexhip_categorize_blob_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
        L.trexhip_categorize_blob_bytes.restype = C.c_size_t
        L.trexhip_categorize_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        L.trexhip_categorize.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
        L.trexhip_tracklet_labels_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                     C.c_void_p, C.POINTER(C.c_uint32)]
        L.trexhip_tracklet_medians_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p]
        _LIB = L
    return _LIB


def _check(rc):
    if rc != 0:
        raise TrexHipError(rc, lib().trexhip_last_error().decode())


def default_params(width, height, **kw):
    p = Params()
    lib().trexhip_default_params(C.byref(p), width, height)
    ranges = kw.pop("size_ranges", None)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    if ranges is not None:
        p.n_ranges = len(ranges)
        for i, (a, b) in enumerate(ranges):
            p.ranges[2 * i], p.ranges[2 * i + 1] = a, b
    return p


def default_augment_params(width, height, **kw):
    """The reference's training transform for width x height crops (visual_recognition_torch.py:1301, :1325-1331): RandomAffine(5, move_range) +
    ColorJitter(0.85..1.15 x 3, hue +-0.05); keywords override single fields (seed among them)."""
    p = AugmentParams()
    lib().trexhip_default_augment_params(C.byref(p), width, height)
    for k, v in kw.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _from_addr(addr, count, dtype):
    if count == 0 or not addr:
        return np.zeros(0, dtype)
    buf = (C.c_uint8 * (count * dtype.itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype, count=count)


class FrameResult:
    """Blobs of one frame: structured arrays with frame-relative run/pixel offsets."""
    __slots__ = ("info", "blobs", "runs", "pixels")

    def __init__(self, info, blobs, runs, pixels):
        self.info, self.blobs, self.runs, self.pixels = info, blobs, runs, pixels


HIP_STREAM_LEGACY = 1        # hipStreamLegacy: the explicit handle of the legacy default stream (hip_runtime_api.h)


class Segmenter:
    """Host-side handle mirroring TRex's BackgroundSubtraction (set_background / apply / fps / deinit)."""

    def __init__(self, params, stream="torch"):
        """stream: "torch" = enqueue on torch's current stream of the device when torch is loaded (callers hand torch tensors to
        the context, so torch's own fills / copies and the context's kernels must be ordered); None = the context's own
        non-blocking stream (the library default); or a hipStream_t value."""
        self.params = params
        self._h = C.c_void_p()
        _check(lib().trexhip_create(C.byref(params), C.byref(self._h)))
        if stream == "torch":
            import sys
            torch = sys.modules.get("torch")
            if torch is not None and torch.cuda.is_available():
                s = torch.cuda.current_stream(params.device).cuda_stream
                self.set_stream(s if s else HIP_STREAM_LEGACY)     # torch's default stream is the legacy null stream
        elif stream:
            self.set_stream(stream)

    def close(self):
        if self._h:
            lib().trexhip_destroy(self._h)
            self._h = C.c_void_p()

    deinit = close

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    def update_params(self, size_ranges=None, **kw):
        """the settings TRex re-reads on every apply(): threshold, threshold_maximum, inclusive, enable_difference, absolute_difference,
        image_invert, zero_is_background, cm_per_pixel, size_ranges -- effective from the next segment call (trexhip_update_params)"""
        lp = LiveParams()
        _check(lib().trexhip_get_live_params(self._h, C.byref(lp)))
        for k, v in kw.items():
            if k not in dict(LiveParams._fields_):
                raise KeyError(k)
            setattr(lp, k, v)
        if size_ranges is not None:
            if len(size_ranges) > 8:
                lp.n_ranges = len(size_ranges)       # the library refuses it
            else:
                lp.n_ranges = len(size_ranges)
                for i, (a, b) in enumerate(size_ranges):
                    lp.ranges[2 * i], lp.ranges[2 * i + 1] = a, b
        _check(lib().trexhip_update_params(self._h, C.byref(lp)))
        for k, _ in LiveParams._fields_:
            if k != "ranges":
                setattr(self.params, k, getattr(lp, k))
        for i in range(16):
            self.params.ranges[i] = lp.ranges[i]

    def set_stream(self, hip_stream_ptr):
        _check(lib().trexhip_set_stream(self._h, C.c_void_p(hip_stream_ptr)))

    def set_background(self, bg):
        """bg: numpy uint8 [H,W] (host) or a torch CUDA uint8 tensor (device)."""
        if isinstance(bg, np.ndarray):
            bg = np.ascontiguousarray(bg, np.uint8)
            assert bg.shape == (self.params.height, self.params.width)
            _check(lib().trexhip_set_background(self._h, bg.ctypes.data_as(C.c_void_p), bg.shape[1]))
        else:
            assert bg.is_cuda and bg.is_contiguous() and bg.numel() == self.params.height * self.params.width
            _check(lib().trexhip_set_background_device(self._h, C.c_void_p(bg.data_ptr())))

    def generate_average(self, d_frames_ptr, n, method=0):
        """Background = per-pixel mean (0) / max (1) / min (2) of n HBM-resident gray frames; returns it as numpy."""
        _check(lib().trexhip_generate_average_device(self._h, C.c_void_p(d_frames_ptr), n, method))
        out = np.empty((self.params.height, self.params.width), np.uint8)
        _check(lib().trexhip_get_background(self._h, out.ctypes.data_as(C.c_void_p), out.shape[1]))
        return out

    def get_background(self):
        """The context's gray background as numpy uint8 [H,W]."""
        out = np.empty((self.params.height, self.params.width), np.uint8)
        _check(lib().trexhip_get_background(self._h, out.ctypes.data_as(C.c_void_p), out.shape[1]))
        return out

    def segment_device(self, d_ptr, n):
        """Enqueue the detect stage for n HBM-resident gray frames at device address d_ptr."""
        _check(lib().trexhip_segment_device(self._h, C.c_void_p(d_ptr), n))

    def segment_host(self, frames):
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        stride = frames[0].shape[1] if frames else self.params.width
        _check(lib().trexhip_segment(self._h, ptrs, stride, len(frames)))

    def set_background_color(self, bgc, color_channel=-1):
        """bgc: numpy uint8 [H,W,3|4] BGR / BGRA background (Background(image, rgb8)); also installs its gray image."""
        bgc = np.ascontiguousarray(bgc, np.uint8)
        assert bgc.shape[:2] == (self.params.height, self.params.width)
        _check(lib().trexhip_set_background_color(self._h, bgc.ctypes.data_as(C.c_void_p), bgc.shape[1] * bgc.shape[2], bgc.shape[2], color_channel))

    def segment_color_host(self, frames, color_channel=-1):
        """frames: list of uint8 [H,W,3|4] BGR/BGRA host images (what TRex's TileImage holds)."""
        frames = [np.ascontiguousarray(f, np.uint8) for f in frames]
        ch = frames[0].shape[2]
        ptrs = (C.c_void_p * len(frames))(*[f.ctypes.data for f in frames])
        _check(lib().trexhip_segment_color(self._h, ptrs, frames[0].shape[1] * ch, len(frames), ch, color_channel))

    def segment_color_device(self, d_color_ptr, n, channels, color_channel=-1):
        """n contiguous colour frames [n,H,W,channels] already in HBM."""
        _check(lib().trexhip_segment_color_device(self._h, C.c_void_p(d_color_ptr), n, channels, color_channel))

    def synchronize(self):
        _check(lib().trexhip_synchronize(self._h))

    def fetch_raw(self, rethreshold=False):
        """trexhip_fetch without building per-frame views: the BatchResult struct (counts + pointers into the context's pinned tables)."""
        r = BatchResult()
        rc = (lib().trexhip_fetch_rethreshold if rethreshold else lib().trexhip_fetch)(self._h, C.byref(r))
        if rc != 0 and rc != -3:
            _check(rc)
        if rc == -3:
            self.last_capacity_error = lib().trexhip_last_error().decode()
        return r

    def fetch_begin_raw(self):
        """trexhip_fetch_begin: the BatchResult with the counts and the frame table; the blob / run / pixel tables behind its pointers are on
        their way and valid once fetch_wait() has returned.  The return code (0, or -3 for a batch over capacity) is kept in last_fetch_rc."""
        r = BatchResult()
        rc = self.last_fetch_rc = lib().trexhip_fetch_begin(self._h, C.byref(r))
        if rc != 0 and rc != -3:
            _check(rc)
        if rc == -3:
            self.last_capacity_error = lib().trexhip_last_error().decode()
        return r

    def fetch_wait(self):
        _check(lib().trexhip_fetch_wait(self._h))

    def fetch(self, copy=True, rethreshold=False):
        r = BatchResult()
        rc = (lib().trexhip_fetch_rethreshold if rethreshold else lib().trexhip_fetch)(self._h, C.byref(r))
        malformed = rc == -1 and r.n_frames > 0 and bool((_from_addr(r.frames, r.n_frames, INFO_DTYPE)["flags"] & FRAME_MALFORMED).any())
        if rc != 0 and rc != -3 and not malformed:
            _check(rc)
        info = _from_addr(r.frames, r.n_frames, INFO_DTYPE)
        blobs = _from_addr(r.blobs, r.total_blobs, BLOB_DTYPE)
        runs = _from_addr(r.runs, r.total_runs, RUN_DTYPE)
        pc = int(r.pixel_channels) or 1                       # bytes per pixel: 3 for the rgb8 pixel encoding
        pixels = _from_addr(r.pixels, r.total_pixels * pc, np.dtype(np.uint8))
        out = []
        for i in range(r.n_frames):
            fi = info[i]
            if fi["flags"]:
                out.append(FrameResult(fi.copy(), np.zeros(0, BLOB_DTYPE), np.zeros(0, RUN_DTYPE), np.zeros(0, np.uint8)))
                continue
            b = blobs[fi["blob_begin"]:fi["blob_begin"] + fi["n_blobs"]]
            ru = runs[fi["run_begin"]:fi["run_begin"] + fi["n_runs"]]
            px = pixels[int(fi["pix_begin"]) * pc:(int(fi["pix_begin"]) + int(fi["n_pixels"])) * pc]
            if copy:
                b, ru, px = b.copy(), ru.copy(), px.copy()
            out.append(FrameResult(fi.copy(), b, ru, px))
        if malformed:                                        # a stored frame broke the V_6 layout: raised, with the other frames' tables attached
            e = TrexHipError(rc, lib().trexhip_last_error().decode())
            e.frames = out
            raise e
        if rc == -3:
            self.last_capacity_error = lib().trexhip_last_error().decode()
        return out

    def posture_device(self, n_blobs, d_outline_ptr, d_segments_ptr, d_info_ptr, table=0, **kw):
        """posture::calculate_posture for every blob of the detect (0) or re-threshold (1) table; see include/trexhip.h."""
        pp = PostureParams()
        lib().trexhip_default_posture_params(C.byref(pp))
        for k, v in kw.items():
            setattr(pp, k, v)
        _check(lib().trexhip_posture_device(self._h, table, C.byref(pp), n_blobs, C.c_void_p(d_outline_ptr),
                                            C.c_void_p(d_segments_ptr), C.c_void_p(d_info_ptr)))
        return pp

    def posture_auto_device(self, n_blobs, d_outline_ptr, d_segments_ptr, d_info_ptr, method=0, track_posture_threshold=15, d_threshold_ptr=0, d_iterations_ptr=0, **kw):
        """posture::calculate_posture with its threshold retry loop for every detect blob; see include/trexhip.h."""
        pp = PostureParams()
        lib().trexhip_default_posture_params(C.byref(pp))
        for k, v in kw.items():
            setattr(pp, k, v)
        _check(lib().trexhip_posture_auto_device(self._h, C.byref(pp), method, track_posture_threshold, n_blobs, C.c_void_p(d_outline_ptr),
                                                 C.c_void_p(d_segments_ptr), C.c_void_p(d_info_ptr), C.c_void_p(d_threshold_ptr or 0), C.c_void_p(d_iterations_ptr or 0)))

    def pack_frames_v6_device(self, d_out_ptr, capacity, d_offsets_ptr, timestamps=None):
        """pv::Frame::serialize bodies (file version V_6 layout) of the last fetched batch; see include/trexhip.h."""
        ts = np.ascontiguousarray(timestamps, np.uint64) if timestamps is not None else None
        _check(lib().trexhip_pack_frames_v6_device(self._h, ts.ctypes.data if ts is not None else None, C.c_void_p(d_out_ptr), capacity, C.c_void_p(d_offsets_ptr)))

    def load_frames_v6_device(self, d_bodies_ptr, d_offsets_ptr, n, d_timestamps_ptr=0):
        """pv::Frame::read_from for n stored V_6 frame bodies in HBM (what pack_frames_v6_device wrote): afterwards fetch() and every
        track-stage call work as behind segment_device; d_timestamps_ptr: device uint64 [n] or 0; see include/trexhip.h."""
        _check(lib().trexhip_load_frames_v6_device(self._h, C.c_void_p(d_bodies_ptr or 0), C.c_void_p(d_offsets_ptr or 0), n, C.c_void_p(d_timestamps_ptr or 0)))

    def crops_device(self, d_crops_ptr, n_blobs, out_w=80, out_h=80, normalization=0, difference=0):
        """constraints::diff_image for every blob of the last batch -> uint8 [n_blobs][out_h][out_w] at d_crops_ptr."""
        _check(lib().trexhip_crops_device(self._h, C.c_void_p(d_crops_ptr), n_blobs, out_w, out_h, normalization, difference))

    def midline_device(self, n_blobs, max_points, d_posture_info_ptr, d_segments_ptr, d_midline_ptr, d_midline_info_ptr, d_movement_ptr=None, **kw):
        """Midline::post_process + normalize for every blob of a posture call; d_movement_ptr: [n_blobs][2] float MovementInformation::direction
        (trexhip_midline_movement_device); see include/trexhip.h."""
        mp = MidlineParams()
        lib().trexhip_default_midline_params(C.byref(mp))
        for k, v in kw.items():
            setattr(mp, k, v)
        if d_movement_ptr is None:
            _check(lib().trexhip_midline_device(self._h, C.byref(mp), n_blobs, max_points, C.c_void_p(d_posture_info_ptr), C.c_void_p(d_segments_ptr),
                                                C.c_void_p(d_midline_ptr), C.c_void_p(d_midline_info_ptr)))
        else:
            _check(lib().trexhip_midline_movement_device(self._h, C.byref(mp), n_blobs, max_points, C.c_void_p(d_posture_info_ptr), C.c_void_p(d_segments_ptr),
                                                         C.c_void_p(d_midline_ptr), C.c_void_p(d_midline_info_ptr), C.c_void_p(d_movement_ptr)))

    def split_search_device(self, d_presumed_ptr, n_blobs, d_thresholds_ptr, d_info_ptr, method=1, size_ranges=(), **kw):
        """SplitBlob's threshold search for the detect blobs with presumed_nr > 0; see include/trexhip.h."""
        sp = SplitParams()
        lib().trexhip_default_split_params(C.byref(sp))
        for k, v in kw.items():
            setattr(sp, k, v)
        sp.n_ranges = len(size_ranges)
        for i, (a, b) in enumerate(size_ranges):
            sp.size_ranges[2 * i], sp.size_ranges[2 * i + 1] = a, b
        _check(lib().trexhip_split_search_device(self._h, C.byref(sp), method, C.c_void_p(d_presumed_ptr), n_blobs, C.c_void_p(d_thresholds_ptr),
                                                 C.c_void_p(d_info_ptr)))

    def crops_posture_device(self, d_crops_ptr, n_blobs, d_midline_info_ptr, midline_lengths=None, out_w=80, out_h=80, legacy=False, scale=1.0, difference=0):
        ln = None if midline_lengths is None else np.ascontiguousarray(midline_lengths, np.float32)
        _check(lib().trexhip_crops_posture_device(self._h, C.c_void_p(d_crops_ptr), n_blobs, out_w, out_h, C.c_void_p(d_midline_info_ptr),
                                                  None if ln is None else ln.ctypes.data_as(C.c_void_p), 1 if legacy else 0, scale, difference))

    def crops_transformed_device(self, d_crops_ptr, transforms, midline_lengths, out_w=80, out_h=80, legacy=False, scale=1.0, difference=0):
        """posture / legacy normalisation with caller-supplied Midline::transform matrices (host float32 [n,6]) and lengths [n]."""
        tr = np.ascontiguousarray(transforms, np.float32)
        ln = np.ascontiguousarray(midline_lengths, np.float32)
        _check(lib().trexhip_crops_transformed_device(self._h, C.c_void_p(d_crops_ptr), len(tr), out_w, out_h, tr.ctypes.data_as(C.c_void_p),
                                                      ln.ctypes.data_as(C.c_void_p), 1 if legacy else 0, scale, difference))

    def export_id_table_ex(self, d_probs_ptr, n_blobs, classes, frame_base, d_table_ptr, max_rows, d_midline_ptr=0, d_midline_info_ptr=0, midline_resolution=0):
        """Full per-blob record (16 header words + classes floats + 3 * midline_resolution floats per row); see include/trexhip.h."""
        _check(lib().trexhip_export_id_table_ex_device(self._h, C.c_void_p(d_probs_ptr) if d_probs_ptr else None, n_blobs, classes, frame_base,
                                                       C.c_void_p(d_midline_ptr) if d_midline_ptr else None,
                                                       C.c_void_p(d_midline_info_ptr) if d_midline_info_ptr else None, midline_resolution,
                                                       C.c_void_p(d_table_ptr), max_rows))

    def export_id_table(self, d_probs_ptr, n_blobs, classes, frame_base, d_table_ptr, max_rows):
        """Fixed-size per-blob identity table (8 header words + classes floats per row) into caller memory."""
        _check(lib().trexhip_export_id_table_device(self._h, C.c_void_p(d_probs_ptr) if d_probs_ptr else None, n_blobs,
                                                    classes, frame_base, C.c_void_p(d_table_ptr), max_rows))

    # ---- identity network (mirrors VINetwork: load_weights / probabilities) ----
    def load_weights(self, blob: bytes):
        buf = (C.c_uint8 * len(blob)).from_buffer_copy(blob)
        _check(lib().trexhip_load_weights(self._h, buf, len(blob)))

    def set_identity_precision(self, mode):
        """TREXHIP_CNN_*: 0 = exact fp32 MFMA, 1 = bf16x6 split (fp32-equivalent), 2 = bf16x3 (experiments), 3 = fp16x3 split (default:
        fp32-class on the fp16 matrix cores, range-guarded)."""
        _check(lib().trexhip_set_identity_precision(self._h, mode))

    def num_classes(self):
        return lib().trexhip_num_classes(self._h)

    def network_image_size(self):
        """(width, height) of the crops the loaded network expects; (0, 0) without weights."""
        w, h = C.c_int32(0), C.c_int32(0)
        _check(lib().trexhip_network_image_size(self._h, C.byref(w), C.byref(h)))
        return int(w.value), int(h.value)

    def network_version(self):
        """TREXHIP_NET_* of the loaded network (trex_amd.weights.ARCH_IDS: 0 v118_3, 1 v100, 2 v110, 3 v119, 4 v200); 0 without weights."""
        return int(lib().trexhip_network_version(self._h))

    def identify_chunk_crops(self):
        """crops per chunk of an identify call on the loaded network; 0 for v118_3 (not chunked) and without weights."""
        c = C.c_int32(0)
        _check(lib().trexhip_identify_chunk_crops(self._h, C.byref(c)))
        return int(c.value)

    def probabilities(self, crops):
        """crops: uint8 ndarray (n,H,W,C) on the host, the loaded network's size and channels -> float32 (n,classes) softmax rows."""
        crops = np.ascontiguousarray(crops, np.uint8)
        w, h = self.network_image_size()
        if w:                                   # (without weights the library reports that itself)
            want = (h, w, lib().trexhip_network_channels(self._h))
            if crops.ndim != 4 or tuple(crops.shape[1:]) != want:
                raise ValueError(f"crops must have shape (n, {want[0]}, {want[1]}, {want[2]}) for the loaded network, got {crops.shape}")
        n = crops.shape[0]
        out = np.empty((n, self.num_classes()), np.float32)
        _check(lib().trexhip_identify(self._h, crops.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def guard_stats(self):
        """(crops re-run by the fp16 range guard in the last identify call, whole batch re-run?)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_guard_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), bool(b.value)

    def skip_stats(self):
        """(passes of the batch, passes the role-split conv1+conv2 kernel computed, bytes of V3 rows filled instead) of the last call that skipped"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _check(lib().trexhip_identify_skip_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def skipx_stats(self):
        """(crops that took windowed conv1+conv2 passes, those passes, the aligned full-width passes the other crops took) of the last call;
        (0, 0, 0) where the windowed form did not run"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_skipx_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def bgrow_stats(self):
        """(rows of conv1's pooled output the windowed passes of the last call read, a crop's passes counted as one run; those of them the
        kernel made -- the others are background rows); (0, 0) where every row is made"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_bgrow_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def skip3_stats(self):
        """(row pairs of the batch, row pairs conv3 had to compute, passes its listed form walked -- 0: the dense kernel ran --, bytes of act3 filled
        instead) of the last call that listed; the passes are counted by the row rule alone, six pairs each: skip3x_stats says what ran"""
        a, b, c, d = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        _check(lib().trexhip_identify_skip3_stats(self._h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return int(a.value), int(b.value), int(c.value), int(d.value)

    def skip3x_stats(self):
        """(crops whose listed conv3 row pairs went into windowed passes of 3 tiles, those passes, the full-width listed passes the other crops
        took) of the last call that listed; (0, 0, 0) where the dense kernel ran"""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_skip3x_stats(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return int(a.value), int(b.value), int(c.value)

    def skip3_ran(self):
        """(windowed passes, full-width passes) that the listed instances of conv3 walked in the last call that listed: passes of up to 64
        consecutive tiles, or -- TREXHIP_CONV_GEOM bit 20 -- the passes of whole pairs that skip3x_stats counts either way; (0, 0): the dense
        kernel ran"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_skip3_ran(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def fc1_stats(self):
        """(crop-plane rows of the last identify call -- 10 per crop --, rows its listed fc1 computed); (0, 0) where fc1 was not the listed form"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_fc1_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    def identify_device(self, d_crops_ptr, n, d_probs_ptr, d_logits_ptr=None):
        _check(lib().trexhip_identify_device(self._h, C.c_void_p(d_crops_ptr), n, C.c_void_p(d_probs_ptr),
                                             C.c_void_p(d_logits_ptr) if d_logits_ptr else None))

    def identify_prepare_device(self, d_crops_ptr, n):
        """queues the part of the next identify_device(d_crops_ptr, n, ...) that reads only the crops and the loaded network (the role-split
        chain's lists and background fills); that call skips it if its arguments match, and runs everything otherwise.  Same bits either way."""
        _check(lib().trexhip_identify_prepare_device(self._h, C.c_void_p(d_crops_ptr), n))

    def prepare_stats(self):
        """(records prepare calls made on this context, records an identify call found and used)"""
        a, b = C.c_uint32(0), C.c_uint32(0)
        _check(lib().trexhip_identify_prepare_stats(self._h, C.byref(a), C.byref(b)))
        return int(a.value), int(b.value)

    # ---- the training loader on the device ----
    def device_alloc(self, nbytes):
        """-> device address of nbytes of HBM on the context's device (trexhip_device_alloc)"""
        out = C.c_void_p()
        _check(lib().trexhip_device_alloc(self._h, nbytes, C.byref(out)))
        return int(out.value)

    def device_free(self, d_ptr):
        _check(lib().trexhip_device_free(self._h, C.c_void_p(d_ptr or 0)))

    def copy_to_device(self, d_ptr, array):
        a = np.ascontiguousarray(array)
        _check(lib().trexhip_copy_to_device(self._h, C.c_void_p(d_ptr), a.ctypes.data_as(C.c_void_p), a.nbytes))

    def copy_to_host(self, d_ptr, shape, dtype):
        out = np.empty(shape, dtype)
        _check(lib().trexhip_copy_to_host(self._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d_ptr), out.nbytes))
        return out

    def augment_device(self, d_pool_ptr, pool_size, n, width, height, channels, d_out_ptr, ap=None, indices=None, d_pool_targets_ptr=0,
                       d_targets_out_ptr=0, d_draws_ptr=0, draws_given=False, counter=0):
        """uint8 pool [pool_size][H][W][C] + indices (host, None = 0..n-1) -> float32 batch [n][H][W][C] at d_out_ptr, augmented like the reference's
        training transform (ap: AugmentParams; None = the validation loader, float(byte)); one kernel launch, no synchronisation; see include/trexhip.h."""
        idx = None
        if indices is not None:
            idx = np.ascontiguousarray(indices, np.int32)
            if idx.shape != (n,):
                raise ValueError(f"indices must hold n = {n} entries, got shape {idx.shape}")
        _check(lib().trexhip_augment_device(self._h, C.byref(ap) if ap is not None else None, C.c_void_p(d_pool_ptr), C.c_void_p(d_pool_targets_ptr or 0), pool_size,
                                            idx.ctypes.data_as(C.c_void_p) if idx is not None else None, n, width, height, channels,
                                            C.c_void_p(d_draws_ptr or 0), 1 if draws_given else 0, counter, C.c_void_p(d_out_ptr), C.c_void_p(d_targets_out_ptr or 0)))

    def validation_metrics(self, d_probs_ptr, n, classes, d_targets_ptr=0, frame_ranges=None):
        """Confusion matrix / per-class accuracy (with d_targets_ptr: int32 [n] on the device) and the uniqueness of
        Accumulation::calculate_uniqueness (with frame_ranges: host integers [n_frames][2] = (start, end) rows) of float32 probabilities
        [n][classes] in HBM, reduced on the device (trexhip_validation_metrics_device; synchronises) -> ValidationMetrics."""
        out = ValidationMetrics()
        conf = np.zeros((classes, classes), np.uint32) if d_targets_ptr else None
        fr = None
        res = UniquenessResult()
        up = upr = upc = None
        if frame_ranges is not None:
            fr = np.ascontiguousarray(frame_ranges, np.int32).reshape(-1, 2)
            up, upr, upc = np.zeros(len(fr), np.float32), np.zeros(len(fr), np.float32), np.zeros(classes, np.float32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        _check(lib().trexhip_validation_metrics_device(self._h, C.c_void_p(d_probs_ptr or 0), n, classes, C.c_void_p(d_targets_ptr or 0), ptr(fr),
                                                       len(fr) if fr is not None else 0, ptr(conf), C.byref(res) if fr is not None else None,
                                                       ptr(up), ptr(upr), ptr(upc)))
        if conf is not None:
            rows = conf.sum(axis=1, dtype=np.int64)
            out.confusion = conf
            out.per_class_accuracy = np.zeros(classes, np.float64)
            np.divide(np.diagonal(conf), rows, out=out.per_class_accuracy, where=rows > 0)
        if fr is not None:
            out.good_frames, out.bad_frames = int(res.good_frames), int(res.bad_frames)
            out.good_ratio, out.mean_unique, out.mean_unique_raw = float(res.good_ratio), float(res.mean_unique), float(res.mean_unique_raw)
            out.unique_percent, out.unique_percent_raw, out.uniqueness_per_class = up, upr, upc
        return out

    def class_averages(self, d_probs_ptr, n, classes, d_ids_ptr, n_ids):
        """VINetwork::paverages of float32 probabilities [n][classes] in HBM with one dense key 0..n_ids-1 per row (int32 [n] on the device):
        per key the float32 sum of its rows in row order over their number, bit for bit what the host loop gives, and the arg-max of every
        averaged row (trexhip_class_averages_device; synchronises) -> ClassAverages."""
        samples, values = np.zeros(max(n_ids, 0), np.float32), np.zeros((max(n_ids, 0), max(classes, 0)), np.float32)
        max_index, max_p = np.zeros(max(n_ids, 0), np.int32), np.zeros(max(n_ids, 0), np.float32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _check(lib().trexhip_class_averages_device(self._h, C.c_void_p(d_probs_ptr or 0), n, classes, C.c_void_p(d_ids_ptr or 0), n_ids,
                                                   ptr(samples), ptr(values), ptr(max_index), ptr(max_p)))
        return ClassAverages(samples, values, max_index, max_p)

    # ---- categorisation: the category network beside the identity network, and the tracklet vote ----
    def load_category_weights(self, blob):
        """a category blob (weights.pack_category_blob) into the context's second slot; the identity network is not touched"""
        _check(lib().trexhip_categorize_load_weights(self._h, blob, len(blob)))

    def category_info(self):
        """(categories, channels, width, height) of the loaded category network; zeros without one"""
        v = [C.c_int32(0) for _ in range(4)]
        _check(lib().trexhip_categorize_info(self._h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def categorize_device(self, d_crops_ptr, n, d_labels_ptr, d_probs_ptr=None, d_logits_ptr=None):
        """uint8 crops [n][H][W][C] in HBM -> int32 labels [n] (and, where asked, float32 softmax rows / logits [n][categories]); no synchronisation"""
        _check(lib().trexhip_categorize_device(self._h, C.c_void_p(d_crops_ptr or 0), n, C.c_void_p(d_labels_ptr or 0),
                                               C.c_void_p(d_probs_ptr) if d_probs_ptr else None, C.c_void_p(d_logits_ptr) if d_logits_ptr else None))

    def categorize(self, crops):
        """crops: uint8 ndarray (n,H,W,C) on the host, the category network's size and channels -> int32 (n,) labels (host route)"""
        crops = np.ascontiguousarray(crops, np.uint8)
        cats, ch, w, h = self.category_info()
        if cats and (crops.ndim != 4 or tuple(crops.shape[1:]) != (h, w, ch)):      # (without weights the library reports that itself)
            raise ValueError(f"crops must have shape (n, {h}, {w}, {ch}) for the loaded category network, got {crops.shape}")
        n = crops.shape[0]
        out = np.empty(n, np.int32)
        _check(lib().trexhip_categorize(self._h, crops.ctypes.data_as(C.c_void_p), n, out.ctypes.data_as(C.c_void_p)))
        return out

    def tracklet_labels_device(self, d_labels_ptr, d_tracklet_ptr, n, n_tracklets, categories, d_counts_ptr, d_rows_ptr, d_label_ptr, d_share_ptr=None):
        """DataStore::label_averaged for every tracklet on rows in HBM (trexhip_tracklet_labels_device; synchronises) -> rows skipped for a label >= categories"""
        skipped = C.c_uint32(0)
        _check(lib().trexhip_tracklet_labels_device(self._h, C.c_void_p(d_labels_ptr or 0), C.c_void_p(d_tracklet_ptr or 0), n, n_tracklets, categories,
                                                    C.c_void_p(d_counts_ptr or 0), C.c_void_p(d_rows_ptr or 0), C.c_void_p(d_label_ptr or 0),
                                                    C.c_void_p(d_share_ptr) if d_share_ptr else None, C.byref(skipped)))
        return int(skipped.value)

    def tracklet_labels(self, labels, tracklet, n_tracklets, categories, share=True):
        """the same on host arrays (int32 labels and tracklet ids per row): uploads, votes, fetches -> TrackletLabels(counts, rows, label, share, skipped)"""
        lb, tr = np.ascontiguousarray(labels, np.int32).reshape(-1), np.ascontiguousarray(tracklet, np.int32).reshape(-1)
        if lb.shape != tr.shape:
            raise ValueError(f"labels and tracklet must have one entry per row, got {lb.shape} and {tr.shape}")
        n, T, Cn = len(lb), int(n_tracklets), int(categories)
        sizes = [max(n, 1) * 4, max(n, 1) * 4, max(T * Cn, 1) * 4, max(T, 1) * 4, max(T, 1) * 4, max(T * Cn, 1) * 4]
        ptrs = []
        try:
            for b in sizes:
                ptrs.append(self.device_alloc(b))
            if n:
                self.copy_to_device(ptrs[0], lb)
                self.copy_to_device(ptrs[1], tr)
            skipped = self.tracklet_labels_device(ptrs[0], ptrs[1], n, T, Cn, ptrs[2], ptrs[3], ptrs[4], ptrs[5] if share else None)
            if n == 0:
                return TrackletLabels(np.zeros((T, Cn), np.uint32), np.zeros(T, np.uint32), np.full(T, -1, np.int32),
                                      np.zeros((T, Cn), np.float32) if share else None, 0)
            return TrackletLabels(self.copy_to_host(ptrs[2], (T, Cn), np.uint32), self.copy_to_host(ptrs[3], (T,), np.uint32),
                                  self.copy_to_host(ptrs[4], (T,), np.int32), self.copy_to_host(ptrs[5], (T, Cn), np.float32) if share else None, skipped)
        finally:
            for d in ptrs:
                self.device_free(d)

    def tracklet_medians_device(self, d_crops_ptr, n, width, height, channels, d_tracklet_ptr, n_tracklets, d_median_ptr, d_rows_ptr):
        """hist_utils::addImage's final image for every tracklet of a crop pool in HBM (trexhip_tracklet_medians_device): uint8 medians
        [n_tracklets][height][width] at d_median_ptr, uint32 row counts [n_tracklets] at d_rows_ptr; synchronises only for the checked pass"""
        _check(lib().trexhip_tracklet_medians_device(self._h, C.c_void_p(d_crops_ptr or 0), n, width, height, channels, C.c_void_p(d_tracklet_ptr or 0),
                                                     n_tracklets, C.c_void_p(d_median_ptr or 0), C.c_void_p(d_rows_ptr or 0)))

    def tracklet_medians(self, d_crops_ptr, n, width, height, channels, d_tracklet_ptr, n_tracklets):
        """the same with the results fetched: crops uint8 [n][height][width][channels] and int32 tracklet ids [n] (-1 = none) on the device ->
        (medians uint8 (n_tracklets, height, width), rows uint32 (n_tracklets,)) on the host.  The reference keeps a median where rows > 1."""
        T = int(n_tracklets)
        if not 1 <= T <= 1 << 24 or not (8 <= width <= 256 and 8 <= height <= 256):
            self.tracklet_medians_device(d_crops_ptr, n, width, height, channels, d_tracklet_ptr, T, 0, 0)      # the library says what is wrong
            raise ValueError("trexhip_tracklet_medians_device accepted arguments outside its ranges")
        ptrs = []
        try:
            for b in (T * width * height, T * 4):
                ptrs.append(self.device_alloc(b))
            self.tracklet_medians_device(d_crops_ptr, n, width, height, channels, d_tracklet_ptr, T, ptrs[0], ptrs[1])
            return self.copy_to_host(ptrs[0], (T, height, width), np.uint8), self.copy_to_host(ptrs[1], (T,), np.uint32)
        finally:
            for d in ptrs:
                self.device_free(d)

    def default_vf_params(self, **kw):
        """trexhip_default_vf_params: max_d from the context's frame size, max_distance 5; keywords override single fields"""
        vp = VfParams()
        lib().trexhip_default_vf_params(self._h, C.byref(vp))
        for k, v in kw.items():
            if not hasattr(vp, k):
                raise KeyError(k)
            setattr(vp, k, v)
        return vp

    def visual_field(self, outline, posture_info, frame_entries, entries, observers, max_points, max_tess_points=1024, max_d=None, max_distance=5.0,
                     outputs=VF_OUTPUTS):
        """track::VisualField for every observer of a batch of frames (trexhip_visual_field_device; see include/trexhip.h).
        outline / posture_info: device addresses of what the posture call wrote (float2 [rows][max_points], trexhip_posture_info [rows]), or
        host arrays (float32 [rows][max_points][2], POSTURE_INFO_DTYPE [rows]) that are uploaded first.  frame_entries int32 [n_frames + 1],
        entries VF_ENTRY_DTYPE, observers VF_OBSERVER_DTYPE: host arrays.  outputs: which of VF_OUTPUTS to compute and copy back.
        -> VisualFieldResult."""
        unknown = set(outputs) - set(VF_OUTPUTS)
        if unknown:
            raise KeyError(sorted(unknown))
        fe = np.ascontiguousarray(frame_entries, np.int32).reshape(-1)
        en = np.ascontiguousarray(entries, VF_ENTRY_DTYPE).reshape(-1)
        ob = np.ascontiguousarray(observers, VF_OBSERVER_DTYPE).reshape(-1)
        n_frames, n_entries, n_obs = len(fe) - 1, len(en), len(ob)
        kw = dict(max_points=max_points, max_tess_points=max_tess_points, max_distance=max_distance)
        if max_d is not None:
            kw["max_d"] = max_d
        vp = self.default_vf_params(**kw)
        owned = []

        def up(a):
            d = self.device_alloc(max(a.nbytes, 16))
            owned.append(d)
            if a.nbytes:
                self.copy_to_device(d, a)
            return d

        try:
            if isinstance(outline, np.ndarray):
                o = np.ascontiguousarray(outline, np.float32)
                if o.ndim != 3 or o.shape[1:] != (max_points, 2):
                    raise ValueError(f"outline must be [rows][{max_points}][2], got {o.shape}")
                outline = up(o)
            if isinstance(posture_info, np.ndarray):
                posture_info = up(np.ascontiguousarray(posture_info, POSTURE_INFO_DTYPE))
            d_fe, d_en, d_ob = up(fe), up(en), up(ob)
            cells = n_obs * 2 * VF_LAYERS * VF_RESOLUTION
            spec = {"depth": ((n_obs, 2, VF_LAYERS, VF_RESOLUTION), np.float64), "ids": ((n_obs, 2, VF_LAYERS, VF_RESOLUTION), np.int32),
                    "points": ((n_obs, 2, VF_LAYERS, VF_RESOLUTION, 2), np.float32), "fov": ((n_obs, 2, VF_LAYERS, VF_RESOLUTION), np.uint8),
                    "head_distance": ((n_obs, 2, VF_LAYERS, VF_RESOLUTION), np.float64), "status": ((n_obs,), np.int32)}
            dev = {}
            for k in VF_OUTPUTS:
                if k in outputs:
                    shape, dt = spec[k]
                    dev[k] = self.device_alloc(max(int(np.prod(shape)) * np.dtype(dt).itemsize, 16))
                    owned.append(dev[k])
            _check(lib().trexhip_visual_field_device(self._h, C.byref(vp), C.c_void_p(outline or 0), C.c_void_p(posture_info or 0), C.c_void_p(d_fe),
                                                     n_frames, C.c_void_p(d_en), n_entries, C.c_void_p(d_ob), n_obs,
                                                     *[C.c_void_p(dev.get(k, 0)) for k in VF_OUTPUTS]))
            res = VisualFieldResult()
            for k, d in dev.items():
                shape, dt = spec[k]
                setattr(res, k, self.copy_to_host(d, shape, dt) if cells else np.zeros(shape, dt))
            return res
        finally:
            for d in owned:
                self.device_free(d)

    def rethreshold_per_blob(self, d_thresholds_ptr, method=0, size_ranges=(), threshold=0):
        """SplitBlob::apply_threshold building block: one threshold per detect blob (int32 device array, pooled order; <0 skips)."""
        rng = np.ascontiguousarray(np.array(size_ranges, np.float64).reshape(-1))
        _check(lib().trexhip_rethreshold_per_blob_device(self._h, threshold, C.c_void_p(d_thresholds_ptr), method,
                                                         rng.ctypes.data_as(C.c_void_p) if len(rng) else None, len(rng) // 2))

    def rethreshold(self, threshold, method=0, size_ranges=()):
        """Tracker::prefilter's threshold_blob for every blob of the last batch; fetch(rethreshold=True) reads it."""
        rng = np.ascontiguousarray(np.array(size_ranges, np.float64).reshape(-1))
        _check(lib().trexhip_rethreshold_device(self._h, threshold, method, rng.ctypes.data_as(C.c_void_p) if len(rng) else None,
                                                len(rng) // 2))

    def device_view(self):
        v = DeviceView()
        _check(lib().trexhip_device_view_get(self._h, C.byref(v)))
        return v

    def profile_enable(self, on=True):
        _check(lib().trexhip_profile_enable(self._h, 1 if on else 0))

    def profile_read(self, stage):
        ms, n = C.c_double(), C.c_int64()
        _check(lib().trexhip_profile_read(self._h, stage, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def profile_reset(self):
        _check(lib().trexhip_profile_reset(self._h))


class Trainer:
    """Training step of the identity network (include/trexhip.h: trexhip_trainer_*, trexhip_train_step_device): V118_3, v100 or v110, as the
    blob's header says -- or of the category network, when the blob is a 'TRXC' one (version NET_CATEGORY).  `dropout` is V118_3's rate: the other
    networks use their architecture's own and do not read it."""
    NET_CATEGORY = 100                                    # TREXHIP_NET_CATEGORY

    def __init__(self, seg, weight_blob, max_batch, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, bn_momentum=0.1, dropout=0.05, seed=0, precision=0):
        self._h = C.c_void_p()
        p = TrainParams(max_batch=max_batch, lr=lr, beta1=beta1, beta2=beta2, eps=eps, bn_momentum=bn_momentum, dropout=dropout, seed=seed, precision=precision)
        buf = (C.c_char * len(weight_blob)).from_buffer_copy(weight_blob)
        _check(lib().trexhip_trainer_create(seg.handle, buf, len(weight_blob), C.byref(p), C.byref(self._h)))
        hdr = np.frombuffer(weight_blob[:32], np.int32)
        self.classes, self.channels = int(hdr[2]), int(hdr[5])
        w, h = C.c_int32(), C.c_int32()
        _check(lib().trexhip_trainer_image_size(self._h, C.byref(w), C.byref(h)))
        self.width, self.height = w.value, h.value        # individual_image_size: every batch and crop of this trainer is [n][height][width][channels]
        self._blob_bytes = len(weight_blob)
        v = C.c_int32()
        _check(lib().trexhip_trainer_version(self._h, C.byref(v)))
        self.version = v.value                            # TREXHIP_NET_*: 0 V118_3, 1 v100, 2 v110 (trex_amd.weights.ARCH_IDS); NET_CATEGORY
        # injected keep masks of one sample: Dropout2d behind block 1, 2, 3 and the Dropout behind fc1; conv3 has 128 channels in V118_3, 100 in v100 / v110.
        # The category network's dropout is element-wise: one byte per pooled element, NHWC, (h_i, w_i) by successive floors
        if self.version == self.NET_CATEGORY:
            h1, w1 = self.height // 2, self.width // 2
            self.mask_planes = (h1 * w1 * 16, (h1 // 2) * (w1 // 2) * 64, (h1 // 4) * (w1 // 4) * 100, 100)
        else:
            self.mask_planes = (16, 64, 128, 100) if self.version == 0 else (16, 64, 100, 100)
        self.mask_row = self.keep_mask_bytes(1)           # the library's own statement of the layout
        assert self.mask_row == sum(self.mask_planes)

    def keep_mask_bytes(self, n):
        """bytes of the keep masks of a step of n samples (trexhip_trainer_keep_mask_bytes): the planes lie back to back, each [n][...]"""
        return int(lib().trexhip_trainer_keep_mask_bytes(self._h, n))

    def step_device(self, d_inputs_ptr, d_targets_ptr, n, d_keep_ptr=0, want_loss=True):
        """-> (mean loss, correct count) when want_loss (synchronises), else None"""
        loss, correct = C.c_float(), C.c_int32()
        _check(lib().trexhip_train_step_device(self._h, C.c_void_p(d_inputs_ptr), C.c_void_p(d_targets_ptr), n, C.c_void_p(d_keep_ptr or 0),
                                               C.byref(loss) if want_loss else None, C.byref(correct) if want_loss else None))
        return (loss.value, correct.value) if want_loss else None

    def _check_batch(self, inputs, targets):
        """the reference asserts image size, channel count and integer class labels per batch (visual_recognition_torch.py:1109-1110); the ABI
        takes raw pointers, so a wrong shape would be an out-of-bounds read, not an error"""
        x = np.asarray(inputs)
        if x.ndim != 4 or tuple(x.shape[1:]) != (self.height, self.width, self.channels):
            raise ValueError(f"inputs must be (n, {self.height}, {self.width}, {self.channels}), got {tuple(x.shape)}")
        t = np.asarray(targets)
        if t.dtype.kind not in "iu":
            raise ValueError(f"targets must be integer class indices, got dtype {t.dtype}")
        if t.shape != (x.shape[0],):
            raise ValueError(f"targets must be ({x.shape[0]},), got {tuple(t.shape)}")
        return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(t, np.int32)

    def step(self, inputs, targets, keep_masks=None):
        """host arrays: inputs float32 (n,height,width,C) in [0,255], targets int (n,), keep_masks uint8 (n*mask_row,) or None -> (loss, correct);
        mask_row is 308 for V118_3, 280 for v100 / v110 and keep_mask_bytes(1) for the category network (element-wise masks: it follows the size)"""
        x, y = self._check_batch(inputs, targets)
        k = np.ascontiguousarray(keep_masks, np.uint8) if keep_masks is not None else None
        if k is not None and k.size != x.shape[0] * self.mask_row:
            raise ValueError(f"keep_masks holds {k.size} entries, a batch of {x.shape[0]} needs {x.shape[0]} x {self.mask_row} ({' + '.join(map(str, self.mask_planes))} per sample)")
        loss, correct = C.c_float(), C.c_int32()
        _check(lib().trexhip_train_step(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.shape[0],
                                        k.ctypes.data_as(C.c_void_p) if k is not None else None, C.byref(loss), C.byref(correct)))
        return loss.value, correct.value

    def evaluate(self, inputs, targets):
        """model.eval() forward of one validation batch (host arrays) -> (mean cross entropy, correct count); the trainer is unchanged"""
        x, y = self._check_batch(inputs, targets)
        loss, correct = C.c_float(), C.c_int32()
        _check(lib().trexhip_train_eval(self._h, x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p), x.shape[0], C.byref(loss), C.byref(correct)))
        return loss.value, correct.value

    def evaluate_device(self, d_inputs_ptr, d_targets_ptr, n):
        """the same from device memory (trexhip_train_eval_device; synchronises) -> (mean cross entropy, correct count)"""
        loss, correct = C.c_float(), C.c_int32()
        _check(lib().trexhip_train_eval_device(self._h, C.c_void_p(d_inputs_ptr), C.c_void_p(d_targets_ptr), n, C.byref(loss), C.byref(correct)))
        return loss.value, correct.value

    def predict_device(self, d_crops_ptr, n, d_probs_ptr):
        """uint8 crops [n][height][width][C] in HBM -> float32 softmax rows [n][classes] at d_probs_ptr from the weights as they stand (eval mode; any
        n, chunked by max_batch inside; no synchronisation; the trainer is unchanged): trexhip_train_predict_device"""
        _check(lib().trexhip_train_predict_device(self._h, C.c_void_p(d_crops_ptr), n, C.c_void_p(d_probs_ptr)))

    def set_lr(self, lr):
        _check(lib().trexhip_trainer_set_lr(self._h, lr))

    @property
    def steps(self):
        return int(lib().trexhip_trainer_steps(self._h))

    def read(self, tensor, kind, shape):
        """tensor: index in the version's state_dict order (trex_amd.weights.shapes(arch=version)); kind 0 parameter, 1 gradient, 2 / 3 Adam moments; torch layout"""
        out = np.empty(int(np.prod(shape)), np.float32)
        _check(lib().trexhip_trainer_read(self._h, tensor, kind, out.ctypes.data_as(C.c_void_p), out.size))
        return out.reshape(shape)

    def export(self):
        need = self._blob_bytes                            # the blob it was created from: same classes, channels and size
        buf = (C.c_char * need)()
        got = C.c_size_t()
        _check(lib().trexhip_trainer_export(self._h, buf, need, C.byref(got)))
        return bytes(buf)

    def close(self):
        if self._h:
            lib().trexhip_trainer_destroy(self._h)
            self._h = C.c_void_p()


class Comm:
    """The library's communicator (include/trexhip.h: trexhip_comm_*): gather of every rank's table to rank 0 over RCCL."""

    def __init__(self, seg, rank=0, world=1, unique_id=None):
        self._h = C.c_void_p()
        self.rank, self.world = rank, world
        buf = (C.c_char * 128).from_buffer_copy(unique_id) if unique_id is not None else None
        _check(lib().trexhip_comm_create(seg.handle, buf, rank, world, C.byref(self._h)))

    @staticmethod
    def unique_id():
        buf = (C.c_char * 128)()
        _check(lib().trexhip_comm_unique_id(buf))
        return bytes(buf)

    def gather_device(self, d_send_ptr, nbytes, d_recv_rank0_ptr, seg=None):
        """seg: enqueue on that context's stream instead of the communicator's own (contexts of one device sharing the communicator)"""
        if seg is None:
            _check(lib().trexhip_comm_gather_device(self._h, C.c_void_p(d_send_ptr), nbytes, C.c_void_p(d_recv_rank0_ptr or 0)))
        else:
            _check(lib().trexhip_comm_gather_device_on(self._h, seg.handle, C.c_void_p(d_send_ptr), nbytes, C.c_void_p(d_recv_rank0_ptr or 0)))

    def count_ranks(self):
        """all-reduce of 1 over the communicator: the number of ranks that took part"""
        n = C.c_int32()
        _check(lib().trexhip_comm_count_ranks(self._h, C.byref(n)))
        return n.value

    def close(self):
        if self._h:
            lib().trexhip_comm_destroy(self._h)
            self._h = C.c_void_p()


def lzo1x_compress(data):
    """this library's LZO1X encoder (host code: no GPU needed) -> compressed bytes; see include/trexhip.h"""
    src = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    cap = int(lib().trexhip_lzo1x_bound(len(src)))
    out = np.empty(cap, np.uint8)
    n = C.c_size_t()
    _check(lib().trexhip_lzo1x_compress(src.ctypes.data_as(C.c_void_p) if len(src) else None, len(src), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)))
    return out[:n.value].copy()


def pv_write_frames(bodies, offsets, always_compress=False, file_offset=0):
    """.pv data section of the frames trexhip_pack_frames_v6_device packed (host arrays): -> (bytes, index table [n] u64); see include/trexhip.h"""
    b = np.ascontiguousarray(bodies, np.uint8)
    o = np.ascontiguousarray(offsets, np.uint64)
    n = len(o) - 1
    out = np.empty(int(o[n]) + 16, np.uint8)
    idx = np.zeros(n, np.uint64)
    used = C.c_size_t()
    _check(lib().trexhip_pv_write_frames(b.ctypes.data_as(C.c_void_p), o.ctypes.data_as(C.c_void_p), n, 1 if always_compress else 0, file_offset,
                                         out.ctypes.data_as(C.c_void_p), len(out), idx.ctypes.data_as(C.c_void_p), C.byref(used)))
    return out[:used.value].copy(), idx


def lzo1x_decompress(data, out_len):
    """this library's bounds-checked LZO1X decoder (host code): the stream -> out_len bytes; raises on a truncated / overlong stream or when the
    output does not fit out_len; see include/trexhip.h"""
    src = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8))
    out = np.empty(max(1, out_len), np.uint8)
    n = C.c_size_t()
    _check(lib().trexhip_lzo1x_decompress(src.ctypes.data_as(C.c_void_p), len(src), out.ctypes.data_as(C.c_void_p), out_len, C.byref(n)))
    return out[:n.value].copy()


def pv_read_frames(data, index_table, file_offset=0):
    """inverse of pv_write_frames: .pv data section + index table -> (bodies, offsets [n + 1] u64), every body uncompressed with its flag byte 0:
    what Segmenter.load_frames_v6_device takes once uploaded; see include/trexhip.h"""
    d = np.ascontiguousarray(data, np.uint8)
    idx = np.ascontiguousarray(index_table, np.uint64)
    n = len(idx)
    off = np.zeros(n + 1, np.uint64)
    used = C.c_size_t()
    args = (d.ctypes.data_as(C.c_void_p), len(d), file_offset, idx.ctypes.data_as(C.c_void_p), n)
    _check(lib().trexhip_pv_read_frames(*args, None, 0, off.ctypes.data_as(C.c_void_p), C.byref(used)))      # sizes first
    out = np.empty(max(1, used.value), np.uint8)
    _check(lib().trexhip_pv_read_frames(*args, out.ctypes.data_as(C.c_void_p), used.value, off.ctypes.data_as(C.c_void_p), C.byref(used)))
    return out[:used.value].copy(), off


class PrefilterResult:
    """Host copies of what trexhip_prefilter_device wrote: decision (uint8 [2 * cap]), order (int32 [n_frames][2 * max_blobs]), counts (int32
    [n_frames][4]), presumed_nr (int32 [total detect blobs]) and, when asked for, second_count (int32 [2 * cap]); cap = max_batch * max_blobs.  Entry f * max_blobs + k is sub-blob k of frame f,
    entry cap + f * max_blobs + k its detect blob k; presumed_nr alone is in pooled order of the detect table."""
    __slots__ = ("decision", "order", "counts", "presumed_nr", "second_count", "cap")

    def __init__(self, decision, order, counts, presumed_nr, second_count, cap):
        self.decision, self.order, self.counts, self.presumed_nr, self.second_count, self.cap = decision, order, counts, presumed_nr, second_count, cap


class Prefilter:
    """Tracker::prefilter's blob policy on the last fetched batch of a Segmenter (trexhip_prefilter_device).  Packs track_include /
    track_ignore (lists of shapes, a shape = list of (x, y) points: 2 = rectangle, more = polygon) and track_ignore_bdx (per frame of the
    batch an iterable of pv::bid words, or None) into the device tables, owns the output buffers (device memory of the context) and keeps
    them until close().  d_presumed_nr is what Segmenter.split_search_device takes."""

    def __init__(self, seg, n_frames, total_blobs):
        self.seg, self.n_frames, self.total_blobs = seg, int(n_frames), int(total_blobs)
        self.cap = int(seg.params.max_batch) * int(seg.params.max_blobs)
        self.per_frame = 2 * int(seg.params.max_blobs)
        self._bufs = []
        self.d_decision = self._alloc(2 * self.cap)
        self.d_order = self._alloc(4 * self.n_frames * self.per_frame)
        self.d_counts = self._alloc(16 * self.n_frames)
        self.d_presumed_nr = self._alloc(4 * max(self.total_blobs, 1))
        self.d_second_count = None
        self._tables = []                                      # device tables of the last run(): freed by the next run() and by close()
        self._want_second = False

    def _alloc(self, nbytes):
        p = C.c_void_p()
        _check(lib().trexhip_device_alloc(self.seg._h, max(int(nbytes), 4), C.byref(p)))
        self._bufs.append(p)
        return p.value

    def _free_tables(self):
        if self._tables:
            self.seg.synchronize()                             # the last run may still read them
        for p in self._tables:
            lib().trexhip_device_free(self.seg._h, p)
            self._bufs.remove(p)
        self._tables = []

    def _upload(self, arr):
        arr = np.ascontiguousarray(arr)
        d = self._alloc(arr.nbytes)
        self._tables.append(self._bufs[-1])
        if arr.nbytes:
            _check(lib().trexhip_copy_to_device(self.seg._h, C.c_void_p(d), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return d

    @staticmethod
    def pack_shapes(shapes):
        """-> (float32 [n_points][2], int32 [n_shapes + 1])"""
        pts = [np.asarray(s, np.float32).reshape(-1, 2) for s in shapes]
        off = np.zeros(len(pts) + 1, np.int32)
        if pts:
            off[1:] = np.cumsum([len(q) for q in pts])
        flat = np.concatenate(pts) if pts else np.zeros((0, 2), np.float32)
        return np.ascontiguousarray(flat, np.float32), off

    @staticmethod
    def pack_bdx(per_frame, n_frames):
        """-> (uint32 sorted per frame, int32 [n_frames + 1])"""
        lists = [np.unique(np.asarray(list(per_frame[f]) if per_frame[f] is not None else [], np.uint32)) for f in range(n_frames)]
        off = np.zeros(n_frames + 1, np.int32)
        off[1:] = np.cumsum([len(q) for q in lists])
        return (np.concatenate(lists) if lists else np.zeros(0, np.uint32)).astype(np.uint32), off

    def run(self, track_threshold, method=0, size_ranges=(), track_threshold_2=0, threshold_ratio_range=(0.5, 1.0), include=(), ignore=(),
            ignore_bdx=None, second_count=False):
        """Enqueue the call; fetch() reads the results."""
        pp = PrefilterParams()
        lib().trexhip_default_prefilter_params(C.byref(pp))
        pp.track_threshold, pp.method, pp.track_threshold_2 = int(track_threshold), int(method), int(track_threshold_2)
        pp.threshold_ratio_range[0], pp.threshold_ratio_range[1] = threshold_ratio_range
        pp.n_ranges = len(size_ranges)
        for i, (a, b) in enumerate(list(size_ranges)[:8]):
            pp.size_ranges[2 * i], pp.size_ranges[2 * i + 1] = a, b
        self._free_tables()
        tb = PrefilterTables()
        ipts, ioff = self.pack_shapes(include)
        gpts, goff = self.pack_shapes(ignore)
        tb.n_include_shapes, tb.n_include_points = len(ioff) - 1, len(ipts)
        tb.n_ignore_shapes, tb.n_ignore_points = len(goff) - 1, len(gpts)
        if len(ioff) > 1:
            tb.d_include_points, tb.d_include_offsets = self._upload(ipts), self._upload(ioff)
        if len(goff) > 1:
            tb.d_ignore_points, tb.d_ignore_offsets = self._upload(gpts), self._upload(goff)
        if ignore_bdx is not None:
            words, boff = self.pack_bdx(ignore_bdx, self.n_frames)
            tb.d_ignore_bdx, tb.d_ignore_bdx_offsets, tb.n_ignore_bdx = self._upload(words), self._upload(boff), len(words)
        if second_count:
            if self.d_second_count is None:
                self.d_second_count = self._alloc(8 * self.cap)
            tb.d_second_count = self.d_second_count
        self._want_second = bool(second_count)
        _check(lib().trexhip_prefilter_device(self.seg._h, C.byref(pp), C.byref(tb), C.c_void_p(self.d_decision), C.c_void_p(self.d_order),
                                              C.c_void_p(self.d_counts), C.c_void_p(self.d_presumed_nr)))

    def _download(self, d, count, dtype):
        out = np.empty(count, dtype)
        if out.nbytes:
            _check(lib().trexhip_copy_to_host(self.seg._h, out.ctypes.data_as(C.c_void_p), C.c_void_p(d), out.nbytes))
        return out

    def fetch(self):
        return PrefilterResult(self._download(self.d_decision, 2 * self.cap, np.uint8),
                               self._download(self.d_order, self.n_frames * self.per_frame, np.int32).reshape(self.n_frames, self.per_frame),
                               self._download(self.d_counts, 4 * self.n_frames, np.int32).reshape(self.n_frames, 4),
                               self._download(self.d_presumed_nr, self.total_blobs, np.int32),
                               self._download(self.d_second_count, 2 * self.cap, np.int32) if self._want_second else None, self.cap)

    def close(self):
        for p in self._bufs:
            lib().trexhip_device_free(self.seg._h, p)
        self._bufs, self._tables = [], []
