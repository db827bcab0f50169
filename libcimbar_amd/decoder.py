"""ctypes binding of the C ABI in include/cimbar_hip.h (plumbing for tests / bench.py / the multi-GPU driver).

Mirrors the reference's Decoder surface for the hot path (src/lib/encoder/Decoder.h:16-38):
`HipDecoder.decode_fountain(img, sink, should_preprocess, color_correction)` writes the good chunks to `sink.write` in chunk
order and returns the good byte count, exactly what `Decoder::decode_fountain` does through aligned_stream.

There is deliberately no CPU fallback: if the shared library or a gfx950 device is missing, loading/creating raises.
"""
import ctypes
import os

import numpy as np

from . import geometry

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libcimbar_hip.so")

MEM_HOST, MEM_DEVICE = 0, 1
TAP_BITPLANE, TAP_SYMBOLS, TAP_COLORS, TAP_DRIFT, TAP_RS_OK, TAP_FLOOD, TAP_CCM, TAP_FLOOD_PATH, TAP_FLOOD_INFO, TAP_FLOOD_VERIFY = range(10)
TAP_GROUP_CELLS, TAP_GROUP_MARGIN, TAP_GROUPS = 10, 11, 12
GROUP_OPEN = -2   # CIMBAR_HIP_GROUP_OPEN: the capture's group is still open at the end of a stream call
TAP_COLOUR_MARGIN = 13
TAP_SCAN_PATH = 14
TAP_GROUP_COLOUR_MARGIN, TAP_GROUP_COLOUR_WEIGHTS = 15, 16   # the colour vote of the last combined batch (set_group_colour_vote / set_stream_colour_vote)
TAP_STREAM_CARRY_WEIGHTS = 17   # the carried weights of the open group's members after a stream call with set_stream_colour_vote on
TAP_STITCH_CELLS, TAP_STITCH_LINES = 18, 19   # the stitching of the last stitched batch (decode_batch_stitched): n = its captures
TAP_STITCH_STRIPS, TAP_STITCH_STRIP_LINES = 22, 23   # the strips of the last stitched batch (set_stitch_strips above 1): tap_stitch_strips
TAP_STITCH_DISTANCE, TAP_STITCH_COLOUR_MARGIN = 36, 37   # the erasure retry of the last plain stitched batch (set_stitch_erasure): tap_stitch_distance / tap_stitch_colour_margin
TAP_STITCH_CARRY = 20   # the capture the stitched-stream calls carry (decode_batch_stitched_stream): tap_stitch_carry
TAP_CELL_MEANS = 21   # the threshold kernel's undrifted cell means, r | g << 8 | b << 16 by grid slot (row * DIM_X + column)
TAP_SCAN_GRAY, TAP_SCAN_HIST, TAP_SCAN_THRESHOLD = 24, 25, 26   # what the stage in front of the last anchor search produced: tap_scan
# CIMBAR_HIP_COLOUR_MARGIN_SUGGESTED (include/cimbar_hip.h): the colour erasure threshold chosen on rendered frames (DESIGN_WIDENING.md)
COLOUR_MARGIN_SUGGESTED = 32512
TAP_FLOOD_ROUNDS = 27   # the relaxed flood of the last batch (set_relaxed_flood): rounds | cells decoded << 16 per frame flooded in rounds
# CIMBAR_HIP_RELAXED_FLOOD_SUGGESTED (include/cimbar_hip.h): the threshold of the table in DESIGN_WIDENING.md "Relaxed flood"
RELAXED_FLOOD_SUGGESTED = 12
TAP_REPEAT_SIG, TAP_REPEAT_AGREE = 28, 29   # the grouping of the last once-call (decode_batch_once): tap_repeat_sig / tap_repeat_agree
TAP_REPEAT_CARRY = 30   # what the once-stream calls carry (decode_batch_once_stream): tap_repeat_carry
TAP_ONCE_RESCUE, TAP_ONCE_RESCUE_CELLS = 31, 32   # the run rescue of the last plain once-call (set_once_rescue): tap_once_rescue / tap_once_rescue_cells
# CIMBAR_HIP_ONCE_*: a capture's role in a once-call
ONCE_UNUSABLE, ONCE_SKIPPED, ONCE_REPRESENTATIVE, ONCE_FALLBACK = -1, 0, 1, 2
ONCE_TORN = 3           # ... with set_once_tear_skip on: a torn boundary capture that was left undecoded
TAP_ONCE_TEAR = 33      # tear skipping in the last plain once-call (set_once_tear_skip): tap_once_tear
TAP_ONCE_SALVAGE = 35   # tear salvage in the last plain once-call (set_once_tear_salvage): tap_once_salvage
TAP_FLOOD_LAUNCH = 34   # the exact-replay launches the last batch made (host bookkeeping, no device wait): tap_flood_launches
FLOOD_LAUNCH_FIELDS = ("instance", "grid", "frames", "first_frame", "area0", "counter", "flags")
FLOOD_LAUNCH_MAX = 16

# every symbol include/cimbar_hip.h declares (tests/test_capi_symbols.py checks the header against this list and the .so)
EXPORTS = (
    "cimbar_hip_create", "cimbar_hip_destroy", "cimbar_hip_bufsize", "cimbar_hip_last_error", "cimbar_hip_decode_frame",
    "cimbar_hip_decode_frame_async", "cimbar_hip_decode_frame_wait",
    "cimbar_hip_decode_batch", "cimbar_hip_reset_ccm", "cimbar_hip_get_ccm", "cimbar_hip_tap", "cimbar_hip_enable_timing",
    "cimbar_hip_stage_times", "cimbar_hip_set_template", "cimbar_hip_encode_batch", "cimbar_hip_decode_plain_batch",
    "cimbar_hip_decode_batch_pipelined", "cimbar_hip_pipeline_wait", "cimbar_hip_pipeline_depth",
    "cimbar_hip_scan_preprocess", "cimbar_hip_deskew_batch", "cimbar_hip_tile_hashes",
    "cimbar_hip_extract_batch", "cimbar_hip_scan_extract_decode_batch", "cimbar_hip_comm_init_all", "cimbar_hip_comm_unique_id",
    "cimbar_hip_comm_init_rank", "cimbar_hip_comm_info", "cimbar_hip_comm_destroy", "cimbar_hip_gather_chunks", "cimbar_hip_pipeline_gather", "cimbar_hip_device", "cimbar_hip_geometry",
    "cimbar_hip_png_scratch_bytes", "cimbar_hip_png_decode_batch", "cimbar_hip_png_decode_batch_v",
    "cimbar_hip_ctx_bufsize", "cimbar_hip_mode_bufsize", "cimbar_hip_set_ccm",
    "cimbar_hip_capture_bytes", "cimbar_hip_scan_preprocess_fmt", "cimbar_hip_deskew_batch_fmt", "cimbar_hip_extract_batch_fmt",
    "cimbar_hip_scan_extract_decode_batch_fmt",
    "cimbar_hip_undistort_calibrate_fmt", "cimbar_hip_undistort_batch_fmt", "cimbar_hip_scan_undistort_extract_decode_batch_fmt",
    "cimbar_hip_rs_decode_erasures", "cimbar_hip_set_erasure_decode", "cimbar_hip_get_erasure_decode",
    "cimbar_hip_set_colour_erasure_decode", "cimbar_hip_get_colour_erasure_decode",
    "cimbar_hip_set_group_colour_vote", "cimbar_hip_get_group_colour_vote",
    "cimbar_hip_set_stream_colour_vote", "cimbar_hip_get_stream_colour_vote",
    "cimbar_hip_decode_batch_combined", "cimbar_hip_scan_extract_decode_batch_combined_fmt",
    "cimbar_hip_decode_batch_combined_stream", "cimbar_hip_scan_extract_decode_batch_combined_stream_fmt", "cimbar_hip_combine_stream_reset",
    "cimbar_hip_auto_create", "cimbar_hip_auto_destroy", "cimbar_hip_auto_bufsize", "cimbar_hip_auto_last_error", "cimbar_hip_auto_reset_ccm",
    "cimbar_hip_auto_get_ccm", "cimbar_hip_auto_set_ccm", "cimbar_hip_auto_scan_extract_decode_batch_fmt",
    "cimbar_hip_deliver_chunks", "cimbar_hip_delivery_reset", "cimbar_hip_delivery_stats",
    "cimbar_hip_decode_batch_stitched", "cimbar_hip_scan_extract_decode_batch_stitched_fmt",
    "cimbar_hip_decode_batch_stitched_stream", "cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt", "cimbar_hip_stitch_stream_reset",
    "cimbar_hip_set_stitch_strips", "cimbar_hip_get_stitch_strips",
    "cimbar_hip_set_stitch_erasure", "cimbar_hip_get_stitch_erasure",
    "cimbar_hip_set_relaxed_flood", "cimbar_hip_get_relaxed_flood", "cimbar_hip_relaxed_flood_stats",
    "cimbar_hip_decode_batch_once", "cimbar_hip_scan_extract_decode_batch_once_fmt",
    "cimbar_hip_decode_batch_once_stream", "cimbar_hip_scan_extract_decode_batch_once_stream_fmt", "cimbar_hip_once_stream_reset",
    "cimbar_hip_set_once_rescue", "cimbar_hip_get_once_rescue",
    "cimbar_hip_set_once_tear_skip", "cimbar_hip_get_once_tear_skip",
    "cimbar_hip_set_once_tear_salvage", "cimbar_hip_get_once_tear_salvage",
)
# cimbar_hip_deliver_chunks' flags
DELIVER_DEDUP, DELIVER_REMEMBER, DELIVER_DROP_EMPTY = 1, 2, 4
PNG_EHEADER, PNG_ESTREAM, PNG_ECODES, PNG_ESIZE, PNG_ECHECK = -30, -31, -32, -33, -34


class PngDesc(ctypes.Structure):
    """cimbar_hip_png_desc"""
    _fields_ = [("zoff", ctypes.c_uint64), ("zlen", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("color_type", ctypes.c_uint32), ("pal_off", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


class CimbarHipError(RuntimeError):
    pass


_lib = None


def load_library(path=None):
    """dlopen libcimbar_hip.so and declare the prototypes. Raises if the library has not been built."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("CIMBAR_HIP_LIB") or LIB_PATH   # CIMBAR_HIP_LIB: A/B-test another build of the same ABI
    if not os.path.exists(p):
        raise CimbarHipError(f"{p} not found: build it with `python -m libcimbar_amd.build` (hipcc, gfx950). "
                             "There is no CPU fallback for the decode path.")
    lib = ctypes.CDLL(p)
    vp, i32, u32, i64, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_int64, ctypes.c_size_t
    lib.cimbar_hip_create.argtypes = [i32, i32, ctypes.POINTER(vp)]
    lib.cimbar_hip_create.restype = i32
    lib.cimbar_hip_destroy.argtypes = [vp]
    lib.cimbar_hip_destroy.restype = None
    lib.cimbar_hip_bufsize.argtypes = []
    lib.cimbar_hip_bufsize.restype = i32
    lib.cimbar_hip_geometry.argtypes = [vp, vp]
    lib.cimbar_hip_geometry.restype = i32
    lib.cimbar_hip_tile_hashes.argtypes = [vp]
    lib.cimbar_hip_tile_hashes.restype = i32
    lib.cimbar_hip_last_error.argtypes = [vp]
    lib.cimbar_hip_last_error.restype = ctypes.c_char_p
    lib.cimbar_hip_decode_frame.argtypes = [vp, vp, u32, u32, sz, i32, i32, vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.cimbar_hip_decode_frame.restype = i32
    lib.cimbar_hip_decode_frame_async.argtypes = [vp, vp, u32, u32, sz, i32, i32, vp, ctypes.POINTER(ctypes.c_uint32)]
    lib.cimbar_hip_decode_frame_async.restype = ctypes.c_longlong
    lib.cimbar_hip_decode_frame_wait.argtypes = [vp, ctypes.c_longlong]
    lib.cimbar_hip_decode_frame_wait.restype = i32
    lib.cimbar_hip_decode_batch.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_decode_batch.restype = i64
    lib.cimbar_hip_decode_plain_batch.argtypes = [vp, vp, i32, i32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_decode_plain_batch.restype = i64
    lib.cimbar_hip_decode_batch_pipelined.argtypes = [vp, vp, i32, i32, i32, vp, vp, vp]
    lib.cimbar_hip_decode_batch_pipelined.restype = i32
    lib.cimbar_hip_pipeline_wait.argtypes = [vp, vp, i32]
    lib.cimbar_hip_pipeline_wait.restype = i32
    lib.cimbar_hip_pipeline_depth.argtypes = [vp]
    lib.cimbar_hip_pipeline_depth.restype = i32
    lib.cimbar_hip_scan_preprocess.argtypes = [vp, vp, u32, u32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_scan_preprocess.restype = i32
    lib.cimbar_hip_deskew_batch.argtypes = [vp, vp, u32, u32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_deskew_batch.restype = i32
    lib.cimbar_hip_extract_batch.argtypes = [vp, vp, u32, u32, i32, i32, vp, vp, vp, i32, vp]
    lib.cimbar_hip_extract_batch.restype = i32
    lib.cimbar_hip_scan_extract_decode_batch.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.cimbar_hip_scan_extract_decode_batch.restype = i64
    lib.cimbar_hip_capture_bytes.argtypes = [u32, u32, i32]
    lib.cimbar_hip_capture_bytes.restype = sz
    lib.cimbar_hip_scan_preprocess_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_scan_preprocess_fmt.restype = i32
    lib.cimbar_hip_deskew_batch_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, vp, vp, i32, vp]
    lib.cimbar_hip_deskew_batch_fmt.restype = i32
    lib.cimbar_hip_extract_batch_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.cimbar_hip_extract_batch_fmt.restype = i32
    lib.cimbar_hip_scan_extract_decode_batch_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, vp, vp, vp, i32, vp]
    lib.cimbar_hip_scan_extract_decode_batch_fmt.restype = i64
    lib.cimbar_hip_undistort_calibrate_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, vp, vp, vp]
    lib.cimbar_hip_undistort_calibrate_fmt.restype = i32
    lib.cimbar_hip_undistort_batch_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, vp, vp, i32, vp, vp, vp]
    lib.cimbar_hip_undistort_batch_fmt.restype = i32
    lib.cimbar_hip_scan_undistort_extract_decode_batch_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.cimbar_hip_scan_undistort_extract_decode_batch_fmt.restype = i64
    lib.cimbar_hip_comm_init_all.argtypes = [i32, vp, ctypes.POINTER(vp)]
    lib.cimbar_hip_comm_init_all.restype = i32
    lib.cimbar_hip_comm_unique_id.argtypes = [vp]
    lib.cimbar_hip_comm_unique_id.restype = i32
    lib.cimbar_hip_comm_init_rank.argtypes = [vp, i32, i32, i32, ctypes.POINTER(vp)]
    lib.cimbar_hip_comm_init_rank.restype = i32
    lib.cimbar_hip_comm_info.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.cimbar_hip_comm_info.restype = i32
    lib.cimbar_hip_comm_destroy.argtypes = [vp]
    lib.cimbar_hip_comm_destroy.restype = None
    lib.cimbar_hip_gather_chunks.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.cimbar_hip_gather_chunks.restype = i32
    lib.cimbar_hip_pipeline_gather.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp]
    lib.cimbar_hip_pipeline_gather.restype = i32
    lib.cimbar_hip_device.argtypes = [vp]
    lib.cimbar_hip_device.restype = i32
    lib.cimbar_hip_reset_ccm.argtypes = [vp]
    lib.cimbar_hip_reset_ccm.restype = i32
    lib.cimbar_hip_get_ccm.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.cimbar_hip_get_ccm.restype = i32
    lib.cimbar_hip_set_ccm.argtypes = [vp, ctypes.POINTER(ctypes.c_float)]
    lib.cimbar_hip_set_ccm.restype = i32
    lib.cimbar_hip_rs_decode_erasures.argtypes = [vp, vp, i32, vp, vp, i32, vp, vp, vp]
    lib.cimbar_hip_rs_decode_erasures.restype = i32
    lib.cimbar_hip_decode_batch_combined.argtypes = [vp, vp, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.cimbar_hip_decode_batch_combined.restype = i64
    lib.cimbar_hip_scan_extract_decode_batch_combined_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp, vp,
                                                                      vp, i32, vp]
    lib.cimbar_hip_scan_extract_decode_batch_combined_fmt.restype = i64
    lib.cimbar_hip_decode_batch_combined_stream.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
    lib.cimbar_hip_decode_batch_combined_stream.restype = i64
    lib.cimbar_hip_scan_extract_decode_batch_combined_stream_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp,
                                                                             vp, vp, vp, i32, vp]
    lib.cimbar_hip_scan_extract_decode_batch_combined_stream_fmt.restype = i64
    lib.cimbar_hip_decode_batch_stitched.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.cimbar_hip_decode_batch_stitched.restype = i64
    lib.cimbar_hip_scan_extract_decode_batch_stitched_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp,
                                                                      i32, vp]
    lib.cimbar_hip_scan_extract_decode_batch_stitched_fmt.restype = i64
    lib.cimbar_hip_decode_batch_stitched_stream.argtypes = lib.cimbar_hip_decode_batch_stitched.argtypes
    lib.cimbar_hip_decode_batch_stitched_stream.restype = i64
    lib.cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt.argtypes = lib.cimbar_hip_scan_extract_decode_batch_stitched_fmt.argtypes
    lib.cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt.restype = i64
    lib.cimbar_hip_stitch_stream_reset.argtypes = [vp]
    lib.cimbar_hip_stitch_stream_reset.restype = i32
    if hasattr(lib, "cimbar_hip_set_stitch_strips"):   # (CIMBAR_HIP_LIB may name an older build for an A/B run)
        lib.cimbar_hip_set_stitch_strips.argtypes = [vp, i32]
        lib.cimbar_hip_set_stitch_strips.restype = i32
        lib.cimbar_hip_get_stitch_strips.argtypes = [vp, ctypes.POINTER(i32)]
        lib.cimbar_hip_get_stitch_strips.restype = i32
    if hasattr(lib, "cimbar_hip_set_stitch_erasure"):   # (likewise)
        lib.cimbar_hip_set_stitch_erasure.argtypes = [vp, i32]
        lib.cimbar_hip_set_stitch_erasure.restype = i32
        lib.cimbar_hip_get_stitch_erasure.argtypes = [vp, ctypes.POINTER(i32)]
        lib.cimbar_hip_get_stitch_erasure.restype = i32
    if hasattr(lib, "cimbar_hip_decode_batch_once"):   # (CIMBAR_HIP_LIB may name an older build for an A/B run)
        lib.cimbar_hip_decode_batch_once.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        lib.cimbar_hip_decode_batch_once.restype = i64
        lib.cimbar_hip_scan_extract_decode_batch_once_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp,
                                                                      i32, vp]
        lib.cimbar_hip_scan_extract_decode_batch_once_fmt.restype = i64
    if hasattr(lib, "cimbar_hip_decode_batch_once_stream"):   # (likewise)
        lib.cimbar_hip_decode_batch_once_stream.argtypes = [vp, vp, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, i32, vp]
        lib.cimbar_hip_decode_batch_once_stream.restype = i64
        lib.cimbar_hip_scan_extract_decode_batch_once_stream_fmt.argtypes = [vp, vp, u32, u32, i32, i32, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp,
                                                                             vp, vp, vp, i32, vp]
        lib.cimbar_hip_scan_extract_decode_batch_once_stream_fmt.restype = i64
        lib.cimbar_hip_once_stream_reset.argtypes = [vp]
        lib.cimbar_hip_once_stream_reset.restype = i32
    lib.cimbar_hip_combine_stream_reset.argtypes = [vp]
    lib.cimbar_hip_combine_stream_reset.restype = i32
    lib.cimbar_hip_auto_create.argtypes = [i32, vp, i32, ctypes.POINTER(vp)]
    lib.cimbar_hip_auto_create.restype = i32
    lib.cimbar_hip_auto_destroy.argtypes = [vp]
    lib.cimbar_hip_auto_destroy.restype = None
    lib.cimbar_hip_auto_bufsize.argtypes = [vp]
    lib.cimbar_hip_auto_bufsize.restype = i32
    lib.cimbar_hip_auto_last_error.argtypes = [vp]
    lib.cimbar_hip_auto_last_error.restype = ctypes.c_char_p
    lib.cimbar_hip_auto_reset_ccm.argtypes = [vp]
    lib.cimbar_hip_auto_reset_ccm.restype = i32
    lib.cimbar_hip_auto_get_ccm.argtypes = [vp, vp]
    lib.cimbar_hip_auto_get_ccm.restype = i32
    lib.cimbar_hip_auto_set_ccm.argtypes = [vp, vp]
    lib.cimbar_hip_auto_set_ccm.restype = i32
    lib.cimbar_hip_auto_scan_extract_decode_batch_fmt.argtypes = [vp, vp, i32, vp, u32, u32, i32, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp]
    lib.cimbar_hip_auto_scan_extract_decode_batch_fmt.restype = i64
    lib.cimbar_hip_deliver_chunks.argtypes = [vp, vp, vp, i32, i32, u32, vp, vp, vp, i32, vp]
    lib.cimbar_hip_deliver_chunks.restype = i64
    lib.cimbar_hip_delivery_reset.argtypes = [vp, i32]
    lib.cimbar_hip_delivery_reset.restype = i32
    lib.cimbar_hip_delivery_stats.argtypes = [vp, ctypes.POINTER(i64), ctypes.POINTER(i64), ctypes.POINTER(i32)]
    lib.cimbar_hip_delivery_stats.restype = i32
    lib.cimbar_hip_set_erasure_decode.argtypes = [vp, i32, i32, i32]
    lib.cimbar_hip_set_erasure_decode.restype = i32
    lib.cimbar_hip_get_erasure_decode.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.cimbar_hip_get_erasure_decode.restype = i32
    lib.cimbar_hip_set_relaxed_flood.argtypes = [vp, i32, i32]
    lib.cimbar_hip_set_relaxed_flood.restype = i32
    lib.cimbar_hip_get_relaxed_flood.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.cimbar_hip_get_relaxed_flood.restype = i32
    lib.cimbar_hip_relaxed_flood_stats.argtypes = [vp, ctypes.POINTER(i64)]
    lib.cimbar_hip_relaxed_flood_stats.restype = i32
    lib.cimbar_hip_set_colour_erasure_decode.argtypes = [vp, i32, i32]
    lib.cimbar_hip_set_colour_erasure_decode.restype = i32
    lib.cimbar_hip_get_colour_erasure_decode.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
    lib.cimbar_hip_get_colour_erasure_decode.restype = i32
    if hasattr(lib, "cimbar_hip_set_group_colour_vote"):   # (CIMBAR_HIP_LIB may name an older build for an A/B run: tools/group_colour_bench.py --lib)
        lib.cimbar_hip_set_group_colour_vote.argtypes = [vp, i32]
        lib.cimbar_hip_set_group_colour_vote.restype = i32
        lib.cimbar_hip_get_group_colour_vote.argtypes = [vp, ctypes.POINTER(i32)]
        lib.cimbar_hip_get_group_colour_vote.restype = i32
    if hasattr(lib, "cimbar_hip_set_stream_colour_vote"):   # (the same: tools/stream_colour_bench.py --lib)
        lib.cimbar_hip_set_stream_colour_vote.argtypes = [vp, i32]
        lib.cimbar_hip_set_stream_colour_vote.restype = i32
        lib.cimbar_hip_get_stream_colour_vote.argtypes = [vp, ctypes.POINTER(i32)]
        lib.cimbar_hip_get_stream_colour_vote.restype = i32
    if hasattr(lib, "cimbar_hip_set_once_rescue"):   # (the same: tools/once_rescue_bench.py --parent-lib)
        lib.cimbar_hip_set_once_rescue.argtypes = [vp, i32]
        lib.cimbar_hip_set_once_rescue.restype = i32
        lib.cimbar_hip_get_once_rescue.argtypes = [vp, ctypes.POINTER(i32)]
        lib.cimbar_hip_get_once_rescue.restype = i32
    if hasattr(lib, "cimbar_hip_set_once_tear_skip"):   # (the same: tools/once_tear_bench.py --parent-lib)
        lib.cimbar_hip_set_once_tear_skip.argtypes = [vp, i32, i32, i32]
        lib.cimbar_hip_set_once_tear_skip.restype = i32
        lib.cimbar_hip_get_once_tear_skip.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32), ctypes.POINTER(i32)]
        lib.cimbar_hip_get_once_tear_skip.restype = i32
    if hasattr(lib, "cimbar_hip_set_once_tear_salvage"):   # (the same: tools/once_salvage_bench.py --parent-lib)
        lib.cimbar_hip_set_once_tear_salvage.argtypes = [vp, i32, i32]
        lib.cimbar_hip_set_once_tear_salvage.restype = i32
        lib.cimbar_hip_get_once_tear_salvage.argtypes = [vp, ctypes.POINTER(i32), ctypes.POINTER(i32)]
        lib.cimbar_hip_get_once_tear_salvage.restype = i32
    lib.cimbar_hip_mode_bufsize.argtypes = [i32]
    lib.cimbar_hip_mode_bufsize.restype = i32
    lib.cimbar_hip_ctx_bufsize.argtypes = [vp]
    lib.cimbar_hip_ctx_bufsize.restype = i32
    lib.cimbar_hip_tap.argtypes = [vp, i32, vp, sz]
    lib.cimbar_hip_tap.restype = i64
    lib.cimbar_hip_enable_timing.argtypes = [vp, i32]
    lib.cimbar_hip_enable_timing.restype = i32
    lib.cimbar_hip_stage_times.argtypes = [vp, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_float), i32]
    lib.cimbar_hip_stage_times.restype = i32
    lib.cimbar_hip_set_template.argtypes = [vp, vp, i32]
    lib.cimbar_hip_set_template.restype = i32
    lib.cimbar_hip_encode_batch.argtypes = [vp, vp, i32, i32, vp, i32, vp]
    lib.cimbar_hip_encode_batch.restype = i32
    lib.cimbar_hip_png_scratch_bytes.argtypes = [ctypes.c_uint, ctypes.c_uint, ctypes.c_uint]
    lib.cimbar_hip_png_scratch_bytes.restype = sz
    lib.cimbar_hip_png_decode_batch.argtypes = [i32, vp, sz, vp, i32, vp, sz, vp, sz, vp, vp]
    lib.cimbar_hip_png_decode_batch.restype = i32
    lib.cimbar_hip_png_decode_batch_v.argtypes = [i32, vp, sz, vp, i32, vp, sz, vp, sz, vp, i32, vp]
    lib.cimbar_hip_png_decode_batch_v.restype = i32
    if path is None:
        _lib = lib
    return lib


def png_split(png):
    """PNG bytes -> (width, height, colour type, bit depth, interlace, zlib stream = the concatenated IDAT payloads, palette bytes or None):
    the chunk walk the ingest library's device mode does on the host"""
    import struct
    if png[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError("not a PNG")
    pos, z, pal, hdr = 8, [], None, None
    while pos + 12 <= len(png):
        n, tag = struct.unpack(">I4s", png[pos:pos + 8])
        body = png[pos + 8:pos + 8 + n]
        if tag == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif tag == b"PLTE":
            pal = bytes(body)
        elif tag == b"IDAT":
            z.append(body)
        elif tag == b"IEND":
            break
        pos += 12 + n
    w, h, depth, ctype, _c, _f, interlace = hdr
    return w, h, ctype, depth, interlace, b"".join(z), pal


def png_decode_batch_device(pngs, device=0, variant=0):
    """PNG files (bytes) -> (list of (h, w, 3) uint8 arrays or None, status array): cimbar_hip_png_decode_batch on torch device buffers.
    Test / bench plumbing: packs the streams the way libcimbar_ingest.so's device mode does."""
    import torch
    lib = load_library()
    n = len(pngs)
    desc = (PngDesc * n)()
    blob = bytearray()
    dims = []
    for i, png in enumerate(pngs):
        w, h, ctype, depth, interlace, z, pal = png_split(png)
        if depth != 8 or interlace:
            raise ValueError("the device decoder takes 8-bit non-interlaced PNGs")
        while len(blob) % 16:
            blob.append(0)
        desc[i].zoff, desc[i].zlen, desc[i].width, desc[i].height, desc[i].color_type = len(blob), len(z), w, h, ctype
        blob += z
        if ctype == 3:
            while len(blob) % 16:
                blob.append(0)
            desc[i].pal_off = len(blob)
            blob += (pal or b"") + bytes(768 - len(pal or b""))
        dims.append((w, h, ctype))
    while len(blob) % 16:
        blob.append(0)
    dev = torch.device("cuda", device)
    d_z = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).to(dev)
    d_desc = torch.from_numpy(np.frombuffer(bytes(desc), np.uint8).copy()).to(dev)
    sstride = max(int(lib.cimbar_hip_png_scratch_bytes(w, h, ct)) for w, h, ct in dims)
    rstride = (max(w * h * 3 for w, h, _ in dims) + 15) & ~15
    d_scratch = torch.empty(n * sstride, dtype=torch.uint8, device=dev)
    d_rgb = torch.zeros(n * rstride, dtype=torch.uint8, device=dev)
    d_status = torch.full((n,), 12345, dtype=torch.int32, device=dev)
    # variant: cimbar_hip_png_decode_batch_v's (0 = chosen by n, 1 = one stream per wavefront, 4 = "many in flight": the device chooses the kernel)
    lib.cimbar_hip_png_decode_batch_v.restype = ctypes.c_int
    rc = lib.cimbar_hip_png_decode_batch_v(device, ctypes.c_void_p(d_z.data_ptr()), ctypes.c_size_t(d_z.numel()), ctypes.c_void_p(d_desc.data_ptr()), n,
                                           ctypes.c_void_p(d_scratch.data_ptr()), ctypes.c_size_t(sstride), ctypes.c_void_p(d_rgb.data_ptr()), ctypes.c_size_t(rstride),
                                           ctypes.c_void_p(d_status.data_ptr()), int(variant), ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise CimbarHipError(f"cimbar_hip_png_decode_batch: {rc}")
    torch.cuda.synchronize(dev)
    status = d_status.cpu().numpy()
    rgb = d_rgb.cpu().numpy()
    out = [rgb[i * rstride:i * rstride + w * h * 3].reshape(h, w, 3).copy() if status[i] == 0 else None for i, (w, h, _) in enumerate(dims)]
    return out, status


def tile_hashes():
    """the 16 tile hashes the library computes at create time (host arithmetic, no device needed)"""
    out = np.zeros(16, dtype=np.uint64)
    load_library().cimbar_hip_tile_hashes(out.ctypes.data)
    return out


def comm_unique_id():
    """128 bytes naming a new RCCL communicator (rank 0 makes it, every rank passes it to HipDecoder.comm_init_rank)"""
    buf = (ctypes.c_uint8 * 128)()
    rc = load_library().cimbar_hip_comm_unique_id(buf)
    if rc != 0:
        raise CimbarHipError(f"cimbar_hip_comm_unique_id failed: {rc} (RCCL not available?)")
    return bytes(buf)


def comm_info(comm):
    """(nranks, rank) of a communicator as RCCL itself reports them (ncclCommCount / ncclCommUserRank)"""
    n, r = ctypes.c_int32(0), ctypes.c_int32(-1)
    rc = load_library().cimbar_hip_comm_info(comm, ctypes.byref(n), ctypes.byref(r))
    if rc != 0:
        raise CimbarHipError(f"cimbar_hip_comm_info failed: {rc}")
    return int(n.value), int(r.value)


def comm_destroy(comm):
    load_library().cimbar_hip_comm_destroy(comm)


_ERR = {-1: "EINVAL", -2: "EDIM", -3: "ENODEVICE", -4: "EHIP", -5: "ENOMEM"}


# the C ABI's `format` values (include/cimbar_hip.h, enum cimbar_hip_format): the reference's four, and the formats of native receivers
FMT_RGB, FMT_RGBA, FMT_NV12, FMT_I420 = 3, 4, 12, 420
FMT_NV21, FMT_YUYV, FMT_UYVY, FMT_BGR, FMT_BGRA = 21, 422, 4221, 30, 40
_SHAPED = {FMT_RGB: 3, FMT_BGR: 3, FMT_RGBA: 4, FMT_BGRA: 4}     # formats an (n, h, w, channels) array describes by itself


def _captures(lib, captures, size, fmt):
    """RGB8 captures as an (n,h,w,3) array (BGR8 with fmt=30; RGBA8 / BGRA8 as (n,h,w,4) with fmt=4 / 40), or -- with size=(w,h) and the C ABI's
    `fmt` (FMT_*: 3 RGB, 4 RGBA, 12 NV12, 420, 21 NV21, 422 YUYV, 4221 UYVY, 30 BGR, 40 BGRA) -- n captures of
    cimbar_hip_capture_bytes(w, h, fmt) bytes each as an (n, bytes) array. Returns (array, n, w, h, fmt)."""
    captures = np.ascontiguousarray(captures, dtype=np.uint8)
    if size is None:
        fmt = int(fmt) if int(fmt) > 0 else 3          # (<= 0 means RGB to the C ABI as well, cimbar_recv_js.cpp:150-151)
        if _SHAPED.get(fmt) == 4 and captures.ndim == 4 and captures.shape[3] == 4:
            n, h, w = captures.shape[:3]
            return captures, n, w, h, fmt
        if _SHAPED.get(fmt) != 3:
            raise CimbarHipError(f"captures in format {fmt} need size=(w, h): the array's shape does not say what the frame is")
        if captures.ndim != 4 or captures.shape[3] != 3:
            raise CimbarHipError(f"{'BGR' if fmt == FMT_BGR else 'RGB'} captures are an (n, h, w, 3) array, got {captures.shape}")
        n, h, w = captures.shape[:3]
        return captures, n, w, h, fmt
    w, h = size
    per = int(lib.cimbar_hip_capture_bytes(w, h, int(fmt)))
    if per == 0 or captures.size % per:
        raise CimbarHipError(f"captures of {w}x{h} in format {fmt}: {captures.size} bytes is no multiple of {per}")
    return captures, captures.size // per, w, h, int(fmt)


class HipDecoder:
    """One decode context on one GPU (== one reference `Decoder` + its thread_local colour-correction state)."""

    def __init__(self, device=0, mode=68, lib_path=None):
        self._lib = load_library(lib_path)   # lib_path: another build of the same ABI (tests: the spill-path variant)
        self._ctx = ctypes.c_void_p()
        rc = self._lib.cimbar_hip_create(int(device), int(mode), ctypes.byref(self._ctx))
        if rc != 0:
            self._ctx = ctypes.c_void_p()
            raise CimbarHipError(f"cimbar_hip_create(device={device}, mode={mode}) failed: {_ERR.get(rc, rc)} "
                                 "(a gfx950 GPU is required; there is no CPU fallback)")
        self.device = device
        g = (ctypes.c_int32 * 12)()
        self._check(self._lib.cimbar_hip_geometry(self._ctx, g), "cimbar_hip_geometry")
        self.geo = geometry.for_mode(g[0])
        if (self.geo.IMG_W, self.geo.IMG_H, self.geo.NCELLS, self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK, self.geo.BLOCKS, self.geo.RS_BLOCK,
                self.geo.RS_PARITY, self.geo.DIM_X, self.geo.DIM_Y, self.geo.OFFSET) != tuple(g[1:12]):
            raise CimbarHipError(f"library geometry {list(g)} does not match libcimbar_amd.geometry for mode {g[0]}")

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.cimbar_hip_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            msg = self._lib.cimbar_hip_last_error(self._ctx).decode("utf-8", "replace")
            raise CimbarHipError(f"{what}: {_ERR.get(int(rc), rc)} {msg}")
        return rc

    # ------------------------------------------------------------------ host-memory entry points
    def decode_frame(self, rgb, should_preprocess=False, color_correction=2):
        """rgb: (1024,1024,3) uint8 numpy array. Returns (good_bytes, chunks (12,625) uint8, mask int)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise CimbarHipError("decode_frame: expected an HxWx3 uint8 image")
        chunks = np.zeros((self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), dtype=np.uint8)
        mask = ctypes.c_uint32(0)
        rc = self._lib.cimbar_hip_decode_frame(self._ctx, rgb.ctypes.data, rgb.shape[1], rgb.shape[0], rgb.strides[0],
                                               int(bool(should_preprocess)), int(color_correction), chunks.ctypes.data,
                                               ctypes.byref(mask))
        self._check(rc, "cimbar_hip_decode_frame")
        return rc, chunks, mask.value

    def decode_frame_async(self, rgb, should_preprocess=False, color_correction=2):
        """Starts one frame (cimbar_hip_decode_frame_async) and returns a ticket for decode_frame_wait; up to pipeline_depth frames in flight, the
        next frame's host-to-device copy running beside this one's kernels. `rgb` must stay alive and untouched until the wait when it is
        page-locked memory (the array is kept referenced here either way)."""
        rgb = np.ascontiguousarray(rgb, dtype=np.uint8)
        if rgb.ndim != 3 or rgb.shape[2] != 3:
            raise CimbarHipError("decode_frame_async: expected an HxWx3 uint8 image")
        chunks = np.zeros((self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), dtype=np.uint8)
        mask = ctypes.c_uint32(0)
        t = self._lib.cimbar_hip_decode_frame_async(self._ctx, rgb.ctypes.data, rgb.shape[1], rgb.shape[0], rgb.strides[0],
                                                    int(bool(should_preprocess)), int(color_correction), chunks.ctypes.data, ctypes.byref(mask))
        self._check(t, "cimbar_hip_decode_frame_async")
        if not hasattr(self, "_frames_in_flight"):
            self._frames_in_flight = {}
        self._frames_in_flight[int(t)] = (rgb, chunks, mask)
        for old in [k for k in self._frames_in_flight if k < int(t) - 16]:      # (tickets nobody waited for)
            del self._frames_in_flight[old]
        return int(t)

    def decode_frame_wait(self, ticket):
        """Blocks until the frame is complete. Returns (good_bytes, chunks (12,625) uint8, mask int) like decode_frame."""
        rc = self._lib.cimbar_hip_decode_frame_wait(self._ctx, int(ticket))
        self._check(rc, "cimbar_hip_decode_frame_wait")
        _rgb, chunks, mask = self._frames_in_flight.pop(int(ticket))
        return rc, chunks, mask.value

    def decode_batch(self, frames, should_preprocess=False, color_correction=2):
        """frames: (n,1024,1024,3) uint8 numpy. Returns (total_good_bytes, chunks (n,12,625), masks (n,) uint32)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError("decode_batch: frames must be (n,1024,1024,3) uint8")
        chunks = np.zeros((n, self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), dtype=np.uint8)
        masks = np.zeros(n, dtype=np.uint32)
        rc = self._lib.cimbar_hip_decode_batch(self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)),
                                               int(color_correction), chunks.ctypes.data, masks.ctypes.data, MEM_HOST, None)
        self._check(rc, "cimbar_hip_decode_batch")
        return int(rc), chunks, masks

    def _groups_in(self, groups, n):
        if groups is None:
            return None, None
        g = np.ascontiguousarray(groups, dtype=np.int32).reshape(-1)
        if len(g) != n:
            raise CimbarHipError(f"groups: one entry per capture ({n}), got {len(g)}")
        return g, g.ctypes.data

    def _group_outputs(self, n):
        geo = self.geo
        return (np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32),
                np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32))

    def decode_batch_combined(self, frames, groups=None, min_agree_permille=0, max_group=0, should_preprocess=False, color_correction=2):
        """Multi-capture decoding (cimbar_hip_decode_batch_combined): frames as for decode_batch; groups = None (the device groups runs of
        captures of one frame) or n ids (-1 / 0, 1, ... contiguous). Returns (n_groups, chunks, masks, groups, gchunks, gmasks): the
        per-capture results of decode_batch, the group of every capture, and n slots of group chunks / masks (zero from n_groups on)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_combined: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        _keep, gin = self._groups_in(groups, n)
        chunks, masks, gout, gchunks, gmasks = self._group_outputs(n)
        ng = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_decode_batch_combined(self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)),
                                                                    int(color_correction), gin, int(min_agree_permille), int(max_group),
                                                                    chunks.ctypes.data, masks.ctypes.data, gout.ctypes.data, gchunks.ctypes.data,
                                                                    gmasks.ctypes.data, ctypes.byref(ng), MEM_HOST, None),
                         "cimbar_hip_decode_batch_combined")
        assert rc == ng.value
        return int(rc), chunks, masks, gout, gchunks, gmasks

    def decode_batch_combined_device(self, frames_ptr, n, chunks_ptr, masks_ptr, groups_out_ptr, gchunks_ptr, gmasks_ptr, n_groups_ptr,
                                     groups=None, min_agree_permille=0, max_group=0, should_preprocess=False, color_correction=2, stream=None):
        """Device pointers in and out (layouts as in include/cimbar_hip.h; groups_out_ptr / n_groups_ptr may be 0); enqueues on `stream`
        (None / 0 = the null stream) and returns at once -- the group count is written to n_groups_ptr (one int32) on the device."""
        _keep, gin = self._groups_in(groups, n)
        vp = ctypes.c_void_p
        self._check(self._lib.cimbar_hip_decode_batch_combined(self._ctx, vp(frames_ptr), int(n), MEM_DEVICE, int(bool(should_preprocess)),
                                                               int(color_correction), gin, int(min_agree_permille), int(max_group), vp(chunks_ptr),
                                                               vp(masks_ptr), vp(groups_out_ptr or None), vp(gchunks_ptr), vp(gmasks_ptr),
                                                               vp(n_groups_ptr or None), MEM_DEVICE, vp(stream) if stream else None),
                    "cimbar_hip_decode_batch_combined(device)")

    def scan_extract_decode_batch_combined(self, captures, groups=None, min_agree_permille=0, max_group=0, preprocess=-1, color_correction=2,
                                           size=None, fmt=3):
        """The capture path with multi-capture decoding (cimbar_hip_scan_extract_decode_batch_combined_fmt). Returns
        (n_groups, chunks, masks, status, groups, gchunks, gmasks); a capture whose extraction failed is in no group."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        _keep, gin = self._groups_in(groups, n)
        chunks, masks, gout, gchunks, gmasks = self._group_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        ng = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_combined_fmt(
            self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess), int(color_correction), gin, int(min_agree_permille),
            int(max_group), chunks.ctypes.data, masks.ctypes.data, status.ctypes.data, gout.ctypes.data, gchunks.ctypes.data, gmasks.ctypes.data,
            ctypes.byref(ng), MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_combined_fmt")
        return int(rc), chunks, masks, status, gout, gchunks, gmasks

    def _stream_outputs(self, n):
        geo = self.geo
        return (np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32),
                np.zeros((n + 1, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n + 1, dtype=np.uint32), np.zeros(n + 1, dtype=np.int32))

    def decode_batch_combined_stream(self, frames, flush=False, min_agree_permille=0, max_group=0, should_preprocess=False, color_correction=2):
        """Multi-capture decoding across calls (cimbar_hip_decode_batch_combined_stream): the group still open at the end of a call is carried
        into the next stream call; flush closes it. frames as for decode_batch, or None / empty with flush. Returns (n_closed, chunks,
        masks, groups, gchunks, gmasks, gsizes): groups has the call-local id of a capture's group if it closed in this call, GROUP_OPEN if
        it stays open; the group outputs have n + 1 slots (zero from n_closed on)."""
        if frames is None:
            frames = np.zeros((0,) + tuple(self.geo.FRAME_SHAPE), dtype=np.uint8)
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_combined_stream: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        chunks, masks, gout, gchunks, gmasks, gsizes = self._stream_outputs(n)
        ng = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_decode_batch_combined_stream(
            self._ctx, frames.ctypes.data if n else None, n, MEM_HOST, int(bool(should_preprocess)), int(color_correction), int(min_agree_permille),
            int(max_group), int(bool(flush)), chunks.ctypes.data if n else None, masks.ctypes.data if n else None, gout.ctypes.data if n else None,
            gchunks.ctypes.data, gmasks.ctypes.data, gsizes.ctypes.data, ctypes.byref(ng), MEM_HOST, None), "cimbar_hip_decode_batch_combined_stream")
        assert rc == ng.value
        return int(rc), chunks, masks, gout, gchunks, gmasks, gsizes

    def decode_batch_combined_stream_device(self, frames_ptr, n, chunks_ptr, masks_ptr, groups_out_ptr, gchunks_ptr, gmasks_ptr, gsizes_ptr, n_groups_ptr,
                                            flush=False, min_agree_permille=0, max_group=0, should_preprocess=False, color_correction=2, stream=None):
        """Device pointers in and out (gchunks / gmasks / gsizes: n + 1 slots; groups_out_ptr / gsizes_ptr / n_groups_ptr may be 0); enqueues on
        `stream` (None / 0 = the null stream) and returns at once -- nothing about the open group is read back."""
        vp = ctypes.c_void_p
        self._check(self._lib.cimbar_hip_decode_batch_combined_stream(
            self._ctx, vp(frames_ptr or None), int(n), MEM_DEVICE, int(bool(should_preprocess)), int(color_correction), int(min_agree_permille),
            int(max_group), int(bool(flush)), vp(chunks_ptr or None), vp(masks_ptr or None), vp(groups_out_ptr or None), vp(gchunks_ptr), vp(gmasks_ptr),
            vp(gsizes_ptr or None), vp(n_groups_ptr or None), MEM_DEVICE, vp(stream) if stream else None), "cimbar_hip_decode_batch_combined_stream(device)")

    def scan_extract_decode_batch_combined_stream(self, captures, flush=False, min_agree_permille=0, max_group=0, preprocess=-1, color_correction=2,
                                                  size=None, fmt=3):
        """The capture path across calls (cimbar_hip_scan_extract_decode_batch_combined_stream_fmt); captures = None with flush closes the open
        group. Returns (n_closed, chunks, masks, status, groups, gchunks, gmasks, gsizes); an unusable capture is in no group and closes
        the group in front of it."""
        if captures is None:
            n, w, h, ptr = 0, 0, 0, None
        else:
            captures, n, w, h, fmt = self._captures(captures, size, fmt)
            ptr = captures.ctypes.data
        chunks, masks, gout, gchunks, gmasks, gsizes = self._stream_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        ng = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_combined_stream_fmt(
            self._ctx, ptr, w, h, int(fmt), n, MEM_HOST, int(preprocess), int(color_correction), int(min_agree_permille), int(max_group),
            int(bool(flush)), chunks.ctypes.data if n else None, masks.ctypes.data if n else None, status.ctypes.data if n else None,
            gout.ctypes.data if n else None, gchunks.ctypes.data, gmasks.ctypes.data, gsizes.ctypes.data, ctypes.byref(ng), MEM_HOST, None),
            "cimbar_hip_scan_extract_decode_batch_combined_stream_fmt")
        return int(rc), chunks, masks, status, gout, gchunks, gmasks, gsizes

    def _stitch_outputs(self, n):
        geo = self.geo
        p = max(n - 1, 0)
        return (np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32),
                np.zeros((2 * p, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(2 * p, dtype=np.uint32), np.zeros((p, 4), dtype=np.int32))

    def decode_batch_stitched(self, frames, axis=0, min_agree_permille=0, min_band=0, should_preprocess=False, color_correction=2):
        """Torn-capture stitching (cimbar_hip_decode_batch_stitched): frames as for decode_batch; axis 0 = a tear along a grid row, 1 = along
        a grid column. Returns (candidate pairs, chunks, masks, schunks, smasks, tears): the per-capture results of decode_batch, 2 (n - 1)
        slots of stitched chunks / masks (pair k, direction d at slot 2k + d) and the (n - 1, 4) tear records {a, b, s, f}."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_stitched: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        chunks, masks, schunks, smasks, tears = self._stitch_outputs(n)
        rc = self._check(self._lib.cimbar_hip_decode_batch_stitched(self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)),
                                                                    int(color_correction), int(axis), int(min_agree_permille), int(min_band),
                                                                    chunks.ctypes.data, masks.ctypes.data, schunks.ctypes.data, smasks.ctypes.data,
                                                                    tears.ctypes.data, MEM_HOST, None), "cimbar_hip_decode_batch_stitched")
        return int(rc), chunks, masks, schunks, smasks, tears

    def decode_batch_stitched_device(self, frames_ptr, n, chunks_ptr, masks_ptr, schunks_ptr, smasks_ptr, tears_ptr=None, axis=0,
                                     min_agree_permille=0, min_band=0, should_preprocess=False, color_correction=2, stream=None):
        """Device pointers in and out (layouts as in include/cimbar_hip.h; tears_ptr may be 0); enqueues on `stream` (None / 0 = the null
        stream) and returns at once."""
        vp = ctypes.c_void_p
        return int(self._check(self._lib.cimbar_hip_decode_batch_stitched(self._ctx, vp(frames_ptr), int(n), MEM_DEVICE, int(bool(should_preprocess)),
                                                                          int(color_correction), int(axis), int(min_agree_permille), int(min_band),
                                                                          vp(chunks_ptr), vp(masks_ptr), vp(schunks_ptr or None), vp(smasks_ptr or None),
                                                                          vp(tears_ptr or None), MEM_DEVICE, vp(stream) if stream else None),
                               "cimbar_hip_decode_batch_stitched(device)"))

    def scan_extract_decode_batch_stitched(self, captures, axis=0, min_agree_permille=0, min_band=0, preprocess=-1, color_correction=2,
                                           size=None, fmt=3):
        """The capture path with torn-capture stitching (cimbar_hip_scan_extract_decode_batch_stitched_fmt). Returns
        (candidate pairs, chunks, masks, status, schunks, smasks, tears); a capture whose extraction failed is in no pair."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks, masks, schunks, smasks, tears = self._stitch_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_stitched_fmt(
            self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess), int(color_correction), int(axis), int(min_agree_permille),
            int(min_band), chunks.ctypes.data, masks.ctypes.data, status.ctypes.data, schunks.ctypes.data, smasks.ctypes.data, tears.ctypes.data,
            MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_stitched_fmt")
        return int(rc), chunks, masks, status, schunks, smasks, tears

    def _once_outputs(self, n):
        geo = self.geo
        return (np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int32),
                np.zeros(n, dtype=np.int32), np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32))

    def decode_batch_once(self, frames, min_agree_permille=0, max_run=0, should_preprocess=False, color_correction=2):
        """Repeat-capture skipping (cimbar_hip_decode_batch_once): frames as for decode_batch. Runs of captures of one displayed frame are found
        from an ink-colour signature in front of the decode; one member of each run is decoded, the others only if that one is incomplete.
        Returns (n_runs, chunks, masks, runs, roles, rchunks, rmasks): per capture its chunks / mask (zero for a skipped one), its run and its
        role (ONCE_*), and n slots of run chunks / masks (zero from n_runs on)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_once: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        chunks, masks, runs, roles, rchunks, rmasks = self._once_outputs(n)
        n_runs = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_decode_batch_once(self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)),
                                                                int(color_correction), int(min_agree_permille), int(max_run), chunks.ctypes.data,
                                                                masks.ctypes.data, runs.ctypes.data, roles.ctypes.data, rchunks.ctypes.data,
                                                                rmasks.ctypes.data, ctypes.addressof(n_runs), MEM_HOST, None),
                         "cimbar_hip_decode_batch_once")
        assert rc == n_runs.value
        return int(rc), chunks, masks, runs, roles, rchunks, rmasks

    def decode_batch_once_device(self, frames_ptr, n, chunks_ptr, masks_ptr, runs_ptr=None, roles_ptr=None, rchunks_ptr=None, rmasks_ptr=None,
                                 n_runs_ptr=None, min_agree_permille=0, max_run=0, should_preprocess=False, color_correction=2, stream=None):
        """Device pointers in and out (layouts as in include/cimbar_hip.h; the five run outputs may each be 0). Synchronises `stream` (None / 0 =
        the null stream) at most twice to size its decode passes, enqueues the rest and returns 0."""
        vp = ctypes.c_void_p
        return int(self._check(self._lib.cimbar_hip_decode_batch_once(self._ctx, vp(frames_ptr), int(n), MEM_DEVICE, int(bool(should_preprocess)),
                                                                      int(color_correction), int(min_agree_permille), int(max_run), vp(chunks_ptr),
                                                                      vp(masks_ptr), vp(runs_ptr or None), vp(roles_ptr or None),
                                                                      vp(rchunks_ptr or None), vp(rmasks_ptr or None), vp(n_runs_ptr or None),
                                                                      MEM_DEVICE, vp(stream) if stream else None),
                               "cimbar_hip_decode_batch_once(device)"))

    def scan_extract_decode_batch_once(self, captures, min_agree_permille=0, max_run=0, preprocess=-1, color_correction=2, size=None, fmt=3):
        """The capture path with repeat-capture skipping (cimbar_hip_scan_extract_decode_batch_once_fmt). Returns
        (n_runs, chunks, masks, status, runs, roles, rchunks, rmasks); a capture whose extraction failed is in no run (run and role -1)."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks, masks, runs, roles, rchunks, rmasks = self._once_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        n_runs = ctypes.c_int(0)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_once_fmt(
            self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess), int(color_correction), int(min_agree_permille), int(max_run),
            chunks.ctypes.data, masks.ctypes.data, status.ctypes.data, runs.ctypes.data, roles.ctypes.data, rchunks.ctypes.data, rmasks.ctypes.data,
            ctypes.addressof(n_runs), MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_once_fmt")
        assert rc == n_runs.value
        return int(rc), chunks, masks, status, runs, roles, rchunks, rmasks

    def decode_batch_once_stream(self, frames, min_agree_permille=0, max_run=0, should_preprocess=False, color_correction=2):
        """Repeat-capture skipping across calls (cimbar_hip_decode_batch_once_stream): as decode_batch_once, but run 0 may continue the run
        the last frame of the once-stream call before belongs to, and a run whose earlier calls already delivered every chunk decodes
        nothing. Returns (n_runs, continued, chunks, masks, runs, roles, rchunks, rmasks); rchunks / rmasks of a continued run are cumulative
        over its calls."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_once_stream: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        chunks, masks, runs, roles, rchunks, rmasks = self._once_outputs(n)
        n_runs, continued = ctypes.c_int(0), ctypes.c_int(-1)
        rc = self._check(self._lib.cimbar_hip_decode_batch_once_stream(
            self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)), int(color_correction), int(min_agree_permille), int(max_run),
            chunks.ctypes.data, masks.ctypes.data, runs.ctypes.data, roles.ctypes.data, rchunks.ctypes.data, rmasks.ctypes.data,
            ctypes.addressof(n_runs), ctypes.addressof(continued), MEM_HOST, None), "cimbar_hip_decode_batch_once_stream")
        assert rc == n_runs.value
        return int(rc), int(continued.value), chunks, masks, runs, roles, rchunks, rmasks

    def decode_batch_once_stream_device(self, frames_ptr, n, chunks_ptr, masks_ptr, runs_ptr=None, roles_ptr=None, rchunks_ptr=None, rmasks_ptr=None,
                                        n_runs_ptr=None, continued_ptr=None, min_agree_permille=0, max_run=0, should_preprocess=False,
                                        color_correction=2, stream=None):
        """Device pointers in and out (the six run outputs may each be 0). Behind the once-stream call before, whatever its stream;
        synchronises `stream` (None / 0 = the null stream) at most twice to size its decode passes, enqueues the rest and returns 0."""
        vp = ctypes.c_void_p
        return int(self._check(self._lib.cimbar_hip_decode_batch_once_stream(
            self._ctx, vp(frames_ptr), int(n), MEM_DEVICE, int(bool(should_preprocess)), int(color_correction), int(min_agree_permille), int(max_run),
            vp(chunks_ptr), vp(masks_ptr), vp(runs_ptr or None), vp(roles_ptr or None), vp(rchunks_ptr or None), vp(rmasks_ptr or None),
            vp(n_runs_ptr or None), vp(continued_ptr or None), MEM_DEVICE, vp(stream) if stream else None),
            "cimbar_hip_decode_batch_once_stream(device)"))

    def scan_extract_decode_batch_once_stream(self, captures, min_agree_permille=0, max_run=0, preprocess=-1, color_correction=2, size=None, fmt=3):
        """The capture path of decode_batch_once_stream (cimbar_hip_scan_extract_decode_batch_once_stream_fmt). Returns
        (n_runs, continued, chunks, masks, status, runs, roles, rchunks, rmasks); a capture whose extraction failed is in no run, carried or
        not."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks, masks, runs, roles, rchunks, rmasks = self._once_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        n_runs, continued = ctypes.c_int(0), ctypes.c_int(-1)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_once_stream_fmt(
            self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess), int(color_correction), int(min_agree_permille), int(max_run),
            chunks.ctypes.data, masks.ctypes.data, status.ctypes.data, runs.ctypes.data, roles.ctypes.data, rchunks.ctypes.data, rmasks.ctypes.data,
            ctypes.addressof(n_runs), ctypes.addressof(continued), MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_once_stream_fmt")
        assert rc == n_runs.value
        return int(rc), int(continued.value), chunks, masks, status, runs, roles, rchunks, rmasks

    def once_stream_reset(self):
        """forget what the once-stream calls carry: the next one's first capture starts a run"""
        self._check(self._lib.cimbar_hip_once_stream_reset(self._ctx), "cimbar_hip_once_stream_reset")

    def tap_repeat_carry(self):
        """TAP_REPEAT_CARRY: (sig (NCELLS,) uint8, usable, len, P) of the capture the once-stream calls carry; raises while nothing is carried"""
        out = np.zeros(self.geo.NCELLS + 12, dtype=np.uint8)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_REPEAT_CARRY, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        usable, length, p = (int(v) for v in out[self.geo.NCELLS:].copy().view(np.uint32))
        return out[:self.geo.NCELLS].copy(), usable, length, p

    def _stitch_stream_outputs(self, n):
        geo = self.geo
        return (np.zeros((n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(n, dtype=np.uint32),
                np.zeros((2 * n, geo.CHUNKS_PER_FRAME, geo.CHUNK), dtype=np.uint8), np.zeros(2 * n, dtype=np.uint32), np.zeros((n, 4), dtype=np.int32))

    def decode_batch_stitched_stream(self, frames, axis=0, min_agree_permille=0, min_band=0, should_preprocess=False, color_correction=2):
        """Torn-capture stitching across calls (cimbar_hip_decode_batch_stitched_stream): as decode_batch_stitched, but a call of n frames
        reports n pair rows -- row 0 is (the last frame of the stream call before, frame 0), row r is (frame r - 1, frame r). Returns
        (candidate rows, chunks, masks, schunks, smasks, tears) with n / n / 2n / 2n / n rows; row r, direction d is slot 2r + d. Row 0 of
        the first call after create or stitch_stream_reset is {-1, -1, -1, 0} with zero slots."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError(f"decode_batch_stitched_stream: frames must be (n,{self.geo.IMG_H},{self.geo.IMG_W},3) uint8")
        chunks, masks, schunks, smasks, tears = self._stitch_stream_outputs(n)
        rc = self._check(self._lib.cimbar_hip_decode_batch_stitched_stream(
            self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)), int(color_correction), int(axis), int(min_agree_permille),
            int(min_band), chunks.ctypes.data, masks.ctypes.data, schunks.ctypes.data, smasks.ctypes.data, tears.ctypes.data, MEM_HOST, None),
            "cimbar_hip_decode_batch_stitched_stream")
        return int(rc), chunks, masks, schunks, smasks, tears

    def decode_batch_stitched_stream_device(self, frames_ptr, n, chunks_ptr, masks_ptr, schunks_ptr, smasks_ptr, tears_ptr=None, axis=0,
                                            min_agree_permille=0, min_band=0, should_preprocess=False, color_correction=2, stream=None):
        """Device pointers in and out (2n stitched slots, n tear records; tears_ptr may be 0); enqueues on `stream` (None / 0 = the null
        stream), behind the stitched-stream call before, and returns at once."""
        vp = ctypes.c_void_p
        return int(self._check(self._lib.cimbar_hip_decode_batch_stitched_stream(
            self._ctx, vp(frames_ptr), int(n), MEM_DEVICE, int(bool(should_preprocess)), int(color_correction), int(axis), int(min_agree_permille),
            int(min_band), vp(chunks_ptr), vp(masks_ptr), vp(schunks_ptr or None), vp(smasks_ptr or None), vp(tears_ptr or None), MEM_DEVICE,
            vp(stream) if stream else None), "cimbar_hip_decode_batch_stitched_stream(device)"))

    def scan_extract_decode_batch_stitched_stream(self, captures, axis=0, min_agree_permille=0, min_band=0, preprocess=-1, color_correction=2,
                                                  size=None, fmt=3):
        """The capture path of decode_batch_stitched_stream (cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt). Returns
        (candidate rows, chunks, masks, status, schunks, smasks, tears); a capture whose extraction failed is in no pair, carried or not."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks, masks, schunks, smasks, tears = self._stitch_stream_outputs(n)
        status = np.zeros(n, dtype=np.int32)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt(
            self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess), int(color_correction), int(axis), int(min_agree_permille),
            int(min_band), chunks.ctypes.data, masks.ctypes.data, status.ctypes.data, schunks.ctypes.data, smasks.ctypes.data, tears.ctypes.data,
            MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_stitched_stream_fmt")
        return int(rc), chunks, masks, status, schunks, smasks, tears

    def stitch_stream_reset(self):
        """forget the capture the stitched-stream calls carry: the next one's row 0 has no partner"""
        self._check(self._lib.cimbar_hip_stitch_stream_reset(self._ctx), "cimbar_hip_stitch_stream_reset")

    def set_stitch_strips(self, strips):
        """cimbar_hip_set_stitch_strips: the stitched calls find the shared band in `strips` strips across the lines (1 .. 8; 1, the
        setting after create, is whole lines). Read by every stitched call when it is made."""
        self._check(self._lib.cimbar_hip_set_stitch_strips(self._ctx, int(strips)), "cimbar_hip_set_stitch_strips")

    def get_stitch_strips(self):
        a = ctypes.c_int32(0)
        self._check(self._lib.cimbar_hip_get_stitch_strips(self._ctx, ctypes.byref(a)), "cimbar_hip_get_stitch_strips")
        return int(a.value)

    def tap_stitch_strips(self, n, strips, stream=False):
        """TAP_STITCH_STRIPS of the last stitched batch of n captures, which ran with `strips` above 1: (n - 1, strips, 4) int32
        {a_j, b_j, s_j, f_j}; stream=True: (n, strips, 4)"""
        out = np.zeros((n if stream else max(n - 1, 0), int(strips), 4), np.int32)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_STRIPS, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_stitch_strip_lines(self, n, strips, axis=0, stream=False):
        """TAP_STITCH_STRIP_LINES of that batch on `axis`: (n - 1, strips, L) uint16, the agreeing cells of every line in every strip;
        stream=True: (n, strips, L)"""
        out = np.zeros((n if stream else max(n - 1, 0), int(strips), self.geo.DIM_Y if axis == 0 else self.geo.DIM_X), np.uint16)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_STRIP_LINES, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def set_stitch_erasure(self, on):
        """cimbar_hip_set_stitch_erasure: the plain stitched calls retry the chunks a stitched slot lacks with low-confidence cells erased,
        each cell's confidence taken in the capture it came from (the symbol retry where set_erasure_decode is on, the colour retry where
        set_colour_erasure_decode is on). Off after create; the stitched-stream calls are not affected; modes 4 and 8 refuse it."""
        self._check(self._lib.cimbar_hip_set_stitch_erasure(self._ctx, int(bool(on))), "cimbar_hip_set_stitch_erasure")

    def get_stitch_erasure(self):
        a = ctypes.c_int32(0)
        self._check(self._lib.cimbar_hip_get_stitch_erasure(self._ctx, ctypes.byref(a)), "cimbar_hip_get_stitch_erasure")
        return int(a.value)

    def tap_stitch_distance(self, n):
        """TAP_STITCH_DISTANCE of the last plain stitched batch of n captures, which ran the symbol retry: (2 (n - 1), NCELLS) uint8 d_sym of
        every stitched cell, 0xFF for the slots the retry skipped; raises when that retry did not run"""
        out = np.zeros((2 * max(n - 1, 0), self.geo.NCELLS), np.uint8)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_DISTANCE, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_stitch_colour_margin(self, n):
        """TAP_STITCH_COLOUR_MARGIN of that batch, which ran the colour retry: (2 (n - 1), NCELLS) uint32, 0xFFFFFFFF for the slots the
        retry skipped; raises when that retry did not run"""
        out = np.zeros((2 * max(n - 1, 0), self.geo.NCELLS), np.uint32)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_COLOUR_MARGIN, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_stitch_carry(self):
        """TAP_STITCH_CARRY: (symbols (NCELLS,), colours (NCELLS,)) uint8 of the carried capture; raises while nothing is carried"""
        out = np.zeros((2, self.geo.NCELLS), dtype=np.uint8)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_CARRY, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out[0], out[1]

    def tap_scan(self, n, w, h):
        """TAP_SCAN_GRAY / _HIST / _THRESHOLD of the last anchor search, which ran on n captures of w x h: (gray (n, h, w) uint8, the blurred
        gray planes; hist (n, 256) uint32; thr (n,) int32). Raises before any search"""
        gray, hist, thr = np.zeros((n, h, w), np.uint8), np.zeros((n, 256), np.uint32), np.zeros((n,), np.int32)
        for what, out in ((TAP_SCAN_GRAY, gray), (TAP_SCAN_HIST, hist), (TAP_SCAN_THRESHOLD, thr)):
            got = self._check(self._lib.cimbar_hip_tap(self._ctx, what, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
            if got != out.nbytes:
                raise ValueError(f"tap_scan: the last search ran on captures of another size or count ({got} bytes, not {out.nbytes})")
        return gray, hist, thr

    def combine_stream_reset(self):
        """drop the open group and the stream's fixed min_agree_permille / max_group"""
        self._check(self._lib.cimbar_hip_combine_stream_reset(self._ctx), "cimbar_hip_combine_stream_reset")

    def decode_plain_batch(self, frames, should_preprocess=False, color_correction=2):
        """Decoder::decode (the --no-fountain path) for frames (n,1024,1024,3) uint8 numpy. Returns (bytes_written,
        data (n,7500) uint8 with failed RS blocks zeroed, block_ok (n,60) uint8)."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        if frames.shape[1:] != self.geo.FRAME_SHAPE:
            raise CimbarHipError("decode_plain_batch: frames must be (n,1024,1024,3) uint8")
        data = np.zeros((n, self.geo.FRAME_BYTES), dtype=np.uint8)
        ok = np.zeros((n, self.geo.BLOCKS), dtype=np.uint8)
        rc = self._lib.cimbar_hip_decode_plain_batch(self._ctx, frames.ctypes.data, n, MEM_HOST, int(bool(should_preprocess)),
                                                     int(color_correction), data.ctypes.data, ok.ctypes.data, MEM_HOST, None)
        self._check(rc, "cimbar_hip_decode_plain_batch")
        return int(rc), data, ok

    # ------------------------------------------------------------------ device-memory entry point (torch tensors as raw memory)
    def decode_batch_device(self, frames_ptr, n, chunks_ptr, masks_ptr, should_preprocess=False, color_correction=2, stream=None):
        """Enqueue a batch whose input and outputs are device pointers (ints) on HIP stream handle `stream` (None / 0 = the null
        stream, i.e. torch's default stream). Asynchronous: the caller synchronises that stream."""
        rc = self._lib.cimbar_hip_decode_batch(self._ctx, ctypes.c_void_p(frames_ptr), int(n), MEM_DEVICE,
                                               int(bool(should_preprocess)), int(color_correction), ctypes.c_void_p(chunks_ptr),
                                               ctypes.c_void_p(masks_ptr), MEM_DEVICE,
                                               ctypes.c_void_p(stream) if stream else None)
        self._check(rc, "cimbar_hip_decode_batch(device)")
        return int(rc)

    def decode_batch_pipelined(self, frames_ptr, n, chunks_ptr, masks_ptr, should_preprocess=False, color_correction=2, stream=None):
        """Like decode_batch_device, but only the threshold pass runs on `stream`: the rest of the batch overlaps the next batch's
        threshold pass. Outputs are valid once a later pipeline_wait() on a stream has been reached; at most pipeline_depth batches in
        flight."""
        rc = self._lib.cimbar_hip_decode_batch_pipelined(self._ctx, ctypes.c_void_p(frames_ptr), int(n), int(bool(should_preprocess)),
                                                         int(color_correction), ctypes.c_void_p(chunks_ptr), ctypes.c_void_p(masks_ptr),
                                                         ctypes.c_void_p(stream) if stream else None)
        self._check(rc, "cimbar_hip_decode_batch_pipelined")

    def pipeline_wait(self, stream=None, keep_newest=0):
        """`stream` waits for the pipelined batches issued so far except the `keep_newest` most recent ones."""
        self._check(self._lib.cimbar_hip_pipeline_wait(self._ctx, ctypes.c_void_p(stream) if stream else None, int(keep_newest)),
                    "cimbar_hip_pipeline_wait")

    @property
    def pipeline_depth(self):
        return int(self._lib.cimbar_hip_pipeline_depth(self._ctx))

    # ------------------------------------------------------------------ the stage in front: Scanner's image preparation, Deskewer
    def _captures(self, captures, size, fmt):
        return _captures(getattr(self, "_lib", None), captures, size, fmt)

    def scan_preprocess(self, captures, size=None, fmt=3):
        """captures -> (binary (n,h,w) uint8 of 0/255, thresholds (n,) int32): Scanner::preprocess_image."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        out = np.zeros((n, h, w), dtype=np.uint8)
        thr = np.zeros(n, dtype=np.int32)
        self._check(self._lib.cimbar_hip_scan_preprocess_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, out.ctypes.data, thr.ctypes.data,
                                                             MEM_HOST, None), "cimbar_hip_scan_preprocess_fmt")
        return out, thr

    def deskew_batch(self, captures, corners, size=None, fmt=3):
        """captures, corners (n,8) float32 (tl, tr, bl, br as x,y) -> frames (n,1024,1024,3): Deskewer::deskew."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        out = np.zeros((n, *self.geo.FRAME_SHAPE), dtype=np.uint8)
        self._check(self._lib.cimbar_hip_deskew_batch_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, corners.ctypes.data, out.ctypes.data,
                                                          MEM_HOST, None), "cimbar_hip_deskew_batch_fmt")
        return out

    def deskew_batch_device(self, captures_ptr, w, h, n, corners, frames_ptr, stream=None, fmt=3):
        """device captures -> device frames (what cimbar_hip_decode_batch takes next); corners stay a host array."""
        corners = np.ascontiguousarray(corners, dtype=np.float32).reshape(-1, 8)
        self._check(self._lib.cimbar_hip_deskew_batch_fmt(self._ctx, ctypes.c_void_p(captures_ptr), int(w), int(h), int(fmt), int(n), MEM_DEVICE,
                                                          corners.ctypes.data, ctypes.c_void_p(frames_ptr), MEM_DEVICE,
                                                          ctypes.c_void_p(stream) if stream else None), "cimbar_hip_deskew_batch_fmt(device)")

    def extract_batch(self, captures, size=None, fmt=3):
        """Extractor::extract for captures -> (status (n,) int32, corners (n,8) float32, frames (n,1024,1024,3))"""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        frames = np.zeros((n, *self.geo.FRAME_SHAPE), dtype=np.uint8)
        status = np.zeros(n, dtype=np.int32)
        corners = np.zeros((n, 8), dtype=np.float32)
        self._check(self._lib.cimbar_hip_extract_batch_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, frames.ctypes.data, status.ctypes.data,
                                                           corners.ctypes.data, MEM_HOST, None), "cimbar_hip_extract_batch_fmt")
        return status, corners, frames

    def scan_extract_decode_batch(self, captures, preprocess=-1, color_correction=2, size=None, fmt=3):
        """cimbard_scan_extract_decode for n captures -> (good_bytes, chunks (n,12,625), masks (n,), status (n,))"""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks = np.zeros((n, self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), dtype=np.uint8)
        masks = np.zeros(n, dtype=np.uint32)
        status = np.zeros(n, dtype=np.int32)
        rc = self._check(self._lib.cimbar_hip_scan_extract_decode_batch_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess),
                                                                             int(color_correction), chunks.ctypes.data, masks.ctypes.data,
                                                                             status.ctypes.data, MEM_HOST, None), "cimbar_hip_scan_extract_decode_batch_fmt")
        return int(rc), chunks, masks, status

    # ------------------------------------------------------------------ lens undistortion (`cimbar --undistort`, Undistort<SimpleCameraCalibration>)
    def undistort_calibrate(self, captures, size=None, fmt=3):
        """SimpleCameraCalibration::scan per capture -> (ok (n,) int32, k1 (n,) float64); camera = [w/4, 0, w/2; 0, h/4, h/2; 0, 0, 1]"""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        ok = np.zeros(n, dtype=np.int32)
        k1 = np.zeros(n, dtype=np.float64)
        self._check(self._lib.cimbar_hip_undistort_calibrate_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, ok.ctypes.data, k1.ctypes.data,
                                                                 None), "cimbar_hip_undistort_calibrate_fmt")
        return ok, k1

    def undistort_batch(self, captures, params=None, size=None, fmt=3):
        """Undistort::undistort per capture -> (images (n,h,w,3) uint8, ok (n,) int32, k1 (n,) float64). params: None (calibrate each capture) or
        14 floats, camera[9] + distortion[5] (k1 k2 p1 p2 k3), for all of them (set_distortion_params)."""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        out = np.zeros((n, h, w, 3), dtype=np.uint8)
        ok = np.zeros(n, dtype=np.int32)
        k1 = np.zeros(n, dtype=np.float64)
        p = None
        if params is not None:
            p = np.ascontiguousarray(params, dtype=np.float64).reshape(-1)
            if p.size != 14:
                raise CimbarHipError(f"params: camera[9] + distortion[5], got {p.size} values")
        self._check(self._lib.cimbar_hip_undistort_batch_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, p.ctypes.data if p is not None else None,
                                                             out.ctypes.data, MEM_HOST, ok.ctypes.data, k1.ctypes.data, None), "cimbar_hip_undistort_batch_fmt")
        return out, ok, k1

    def scan_undistort_extract_decode_batch(self, captures, preprocess=-1, color_correction=2, size=None, fmt=3):
        """the decode loop of `cimbar --undistort` for n captures -> (good_bytes, chunks (n,12,625), masks (n,), status (n,), undistort_ok (n,))"""
        captures, n, w, h, fmt = self._captures(captures, size, fmt)
        chunks = np.zeros((n, self.geo.CHUNKS_PER_FRAME, self.geo.CHUNK), dtype=np.uint8)
        masks = np.zeros(n, dtype=np.uint32)
        status = np.zeros(n, dtype=np.int32)
        ok = np.zeros(n, dtype=np.int32)
        rc = self._check(self._lib.cimbar_hip_scan_undistort_extract_decode_batch_fmt(self._ctx, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess),
                                                                                       int(color_correction), chunks.ctypes.data, masks.ctypes.data,
                                                                                       status.ctypes.data, ok.ctypes.data, MEM_HOST, None),
                         "cimbar_hip_scan_undistort_extract_decode_batch_fmt")
        return int(rc), chunks, masks, status, ok

    def scan_extract_decode_device(self, captures_ptr, w, h, n, chunks_ptr, masks_ptr, status_ptr=None, preprocess=-1, color_correction=2, stream=None, fmt=3):
        """device captures in, device chunks / masks / status out; asynchronous on `stream`"""
        self._check(self._lib.cimbar_hip_scan_extract_decode_batch_fmt(self._ctx, ctypes.c_void_p(captures_ptr), int(w), int(h), int(fmt), int(n), MEM_DEVICE,
                                                                        int(preprocess), int(color_correction), ctypes.c_void_p(chunks_ptr),
                                                                        ctypes.c_void_p(masks_ptr), ctypes.c_void_p(status_ptr) if status_ptr else None,
                                                                        MEM_DEVICE, ctypes.c_void_p(stream) if stream else None),
                    "cimbar_hip_scan_extract_decode_batch_fmt(device)")

    # ------------------------------------------------------------------ the reference's operator surface
    def decode_fountain(self, img, ostream, should_preprocess=False, color_correction=2):
        """Decoder::decode_fountain (Decoder.h:171-189): good chunks go to ostream.write(bytes) in chunk order; returns good bytes.
        Like the reference, a sink whose chunk_size() is not 625 gets nothing written but the byte count is still returned."""
        good, chunks, mask = self.decode_frame(img, should_preprocess, color_correction)
        feed = True
        if hasattr(ostream, "chunk_size") and ostream.chunk_size() != self.geo.CHUNK:
            feed = False
        if feed:
            for j in range(self.geo.CHUNKS_PER_FRAME):
                if mask & (1 << j):
                    ostream.write(chunks[j].tobytes())
        return good

    # ------------------------------------------------------------------ encode half (frame synthesiser)
    def _ensure_template(self):
        if getattr(self, "_have_template", False):
            return
        path = os.path.join(_HERE, "data", self.geo.TEMPLATE)
        z = np.load(path)
        t = np.zeros(self.geo.FRAME_RGB_BYTES, dtype=np.uint8)
        t[z["idx"]] = z["val"]
        self._check(self._lib.cimbar_hip_set_template(self._ctx, t.ctypes.data, MEM_HOST), "cimbar_hip_set_template")
        self._have_template = True

    def encode_batch(self, payload):
        """payload (n,7500) uint8 numpy -> frames (n,1024,1024,3) uint8 numpy (Encoder::encode_next for n frames)."""
        self._ensure_template()
        payload = np.ascontiguousarray(payload, dtype=np.uint8).reshape(-1, self.geo.FRAME_BYTES)
        n = payload.shape[0]
        out = np.empty((n, *self.geo.FRAME_SHAPE), dtype=np.uint8)
        self._check(self._lib.cimbar_hip_encode_batch(self._ctx, payload.ctypes.data, n, MEM_HOST, out.ctypes.data, MEM_HOST, None),
                    "cimbar_hip_encode_batch")
        return out

    def encode_batch_device(self, payload_ptr, n, rgb_ptr, stream=None):
        """Device pointers in and out; asynchronous on `stream` (None / 0 = the null stream)."""
        self._ensure_template()
        self._check(self._lib.cimbar_hip_encode_batch(self._ctx, ctypes.c_void_p(payload_ptr), int(n), MEM_DEVICE, ctypes.c_void_p(rgb_ptr),
                                                      MEM_DEVICE, ctypes.c_void_p(stream) if stream else None),
                    "cimbar_hip_encode_batch(device)")

    # ------------------------------------------------------------------ multi-GPU exchange through the library's own RCCL binding
    def comm_init_rank(self, uid, nranks, rank):
        """join the communicator named by the 128-byte `uid` (bytes from comm_unique_id() on rank 0); returns an opaque handle"""
        comm = ctypes.c_void_p()
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(uid))
        self._check(self._lib.cimbar_hip_comm_init_rank(buf, int(nranks), int(rank), int(self.device), ctypes.byref(comm)), "cimbar_hip_comm_init_rank")
        return comm

    def pipeline_gather(self, comm, root, chunks_ptr, masks_ptr, n, all_chunks_ptr, all_masks_ptr):
        """cimbar_hip_pipeline_gather: the exchange of the pipelined batch issued last, on that batch's own stream (pipeline_wait then covers it)."""
        self._check(self._lib.cimbar_hip_pipeline_gather(self._ctx, comm, int(root), ctypes.c_void_p(chunks_ptr), ctypes.c_void_p(masks_ptr), int(n),
                                                         ctypes.c_void_p(all_chunks_ptr) if all_chunks_ptr else None,
                                                         ctypes.c_void_p(all_masks_ptr) if all_masks_ptr else None), "cimbar_hip_pipeline_gather")

    def gather_chunks(self, comm, root, chunks_ptr, masks_ptr, n, all_chunks_ptr, all_masks_ptr, stream=None):
        self._check(self._lib.cimbar_hip_gather_chunks(self._ctx, comm, int(root), ctypes.c_void_p(chunks_ptr), ctypes.c_void_p(masks_ptr), int(n),
                                                       ctypes.c_void_p(all_chunks_ptr) if all_chunks_ptr else None,
                                                       ctypes.c_void_p(all_masks_ptr) if all_masks_ptr else None,
                                                       ctypes.c_void_p(stream) if stream else None), "cimbar_hip_gather_chunks")

    # ------------------------------------------------------------------ state / taps / timing
    def reset_ccm(self):
        self._check(self._lib.cimbar_hip_reset_ccm(self._ctx), "cimbar_hip_reset_ccm")

    def get_ccm(self):
        out = (ctypes.c_float * 9)()
        rc = self._check(self._lib.cimbar_hip_get_ccm(self._ctx, out), "cimbar_hip_get_ccm")
        return bool(rc), np.array(list(out), dtype=np.float32).reshape(3, 3)

    def set_ccm(self, m):
        """CimbDecoder::update_color_correction: the carried matrix becomes `m` (3x3) and is active from the next frame on"""
        arr = (ctypes.c_float * 9)(*[float(x) for x in np.asarray(m, dtype=np.float32).reshape(-1)])
        self._check(self._lib.cimbar_hip_set_ccm(self._ctx, arr), "cimbar_hip_set_ccm")

    def set_erasure_decode(self, sym_distance, colour_margin=-1, max_erasures=-1):
        """cimbar_hip_set_erasure_decode: sym_distance <= 0 turns erasure decoding off; max_erasures < 0 = parity - 8"""
        self._check(self._lib.cimbar_hip_set_erasure_decode(self._ctx, int(sym_distance), int(colour_margin), int(max_erasures)),
                    "cimbar_hip_set_erasure_decode")

    def get_erasure_decode(self):
        """(on, sym_distance, colour_margin, max_erasures)"""
        a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        rc = self._check(self._lib.cimbar_hip_get_erasure_decode(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)),
                         "cimbar_hip_get_erasure_decode")
        return bool(rc), a.value, b.value, c.value

    def set_colour_erasure_decode(self, colour_margin, max_erasures=-1):
        """cimbar_hip_set_colour_erasure_decode: colour_margin <= 0 turns the colour retry off; max_erasures < 0 = parity - 8"""
        self._check(self._lib.cimbar_hip_set_colour_erasure_decode(self._ctx, int(colour_margin), int(max_erasures)),
                    "cimbar_hip_set_colour_erasure_decode")

    def get_colour_erasure_decode(self):
        """(on, colour_margin, max_erasures)"""
        a, b = ctypes.c_int(), ctypes.c_int()
        rc = self._check(self._lib.cimbar_hip_get_colour_erasure_decode(self._ctx, ctypes.byref(a), ctypes.byref(b)),
                         "cimbar_hip_get_colour_erasure_decode")
        return bool(rc), a.value, b.value

    def set_relaxed_flood(self, threshold, fallback=True):
        """cimbar_hip_set_relaxed_flood: threshold -1 = off (the default), 0 .. 32 = flagged frames are flooded in threshold rounds and kept
        where every symbol RS block decodes; fallback: every other frame takes the exact replay inside the same call. Modes 4 / 8 refuse it."""
        self._check(self._lib.cimbar_hip_set_relaxed_flood(self._ctx, int(threshold), int(bool(fallback))), "cimbar_hip_set_relaxed_flood")

    def get_relaxed_flood(self):
        """(on, threshold, fallback)"""
        a, b = ctypes.c_int(), ctypes.c_int()
        rc = self._check(self._lib.cimbar_hip_get_relaxed_flood(self._ctx, ctypes.byref(a), ctypes.byref(b)), "cimbar_hip_get_relaxed_flood")
        return bool(rc), a.value, bool(b.value)

    def relaxed_flood_stats(self):
        """(frames flooded in rounds, accepted, handed to the exact replay, rounds in total) since the last set_relaxed_flood"""
        out = (ctypes.c_int64 * 4)()
        self._check(self._lib.cimbar_hip_relaxed_flood_stats(self._ctx, out), "cimbar_hip_relaxed_flood_stats")
        return tuple(int(x) for x in out)

    def set_group_colour_vote(self, on=True):
        """cimbar_hip_set_group_colour_vote: the combined calls settle a disputed colour by the members' classifier margins instead of by
        plurality; with set_colour_erasure_decode on as well, the group's missing colour chunks are retried. Modes 4 / 8 refuse it."""
        self._check(self._lib.cimbar_hip_set_group_colour_vote(self._ctx, int(bool(on))), "cimbar_hip_set_group_colour_vote")

    def get_group_colour_vote(self):
        a = ctypes.c_int()
        self._check(self._lib.cimbar_hip_get_group_colour_vote(self._ctx, ctypes.byref(a)), "cimbar_hip_get_group_colour_vote")
        return bool(a.value)

    def set_once_rescue(self, on=True):
        """cimbar_hip_set_once_rescue: decode_batch_once / scan_extract_decode_batch_once decode a run that stays incomplete after pass 2
        once more from all its members' cells, as decode_batch_combined decodes a group (off after create; the once-stream calls ignore it)"""
        self._check(self._lib.cimbar_hip_set_once_rescue(self._ctx, int(bool(on))), "cimbar_hip_set_once_rescue")

    def get_once_rescue(self):
        a = ctypes.c_int(0)
        self._check(self._lib.cimbar_hip_get_once_rescue(self._ctx, ctypes.byref(a)), "cimbar_hip_get_once_rescue")
        return bool(a.value)

    def set_once_tear_skip(self, axis, line_permille=0, min_side=0):
        """cimbar_hip_set_once_tear_skip: decode_batch_once / scan_extract_decode_batch_once leave a torn capture between two complete runs
        undecoded (role ONCE_TORN). axis -1 = off (the state after create), 0 = the tear runs along grid rows, 1 = along grid columns, 2 =
        either; line_permille <= 0: 750, min_side <= 0: 2. The once-stream calls ignore it; modes 4 / 8 refuse anything but -1."""
        self._check(self._lib.cimbar_hip_set_once_tear_skip(self._ctx, int(axis), int(line_permille), int(min_side)), "cimbar_hip_set_once_tear_skip")

    def get_once_tear_skip(self):
        """(axis, line_permille, min_side) as resolved"""
        a, b, c = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.cimbar_hip_get_once_tear_skip(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "cimbar_hip_get_once_tear_skip")
        return a.value, b.value, c.value

    def set_once_tear_salvage(self, on=True, guard_lines=-1):
        """cimbar_hip_set_once_tear_salvage: with set_once_rescue and set_once_tear_skip both on, a torn capture decoded in pass 2 joins the
        rescue's vote of its neighbour runs on its good side, guard_lines lines away from the tear (-1: 1; 0 .. 16). Off after create; the
        once-stream calls ignore it; modes 4 / 8 refuse on."""
        self._check(self._lib.cimbar_hip_set_once_tear_salvage(self._ctx, int(bool(on)), int(guard_lines)), "cimbar_hip_set_once_tear_salvage")

    def get_once_tear_salvage(self):
        """(on, guard_lines) as resolved"""
        a, b = ctypes.c_int(0), ctypes.c_int(0)
        self._check(self._lib.cimbar_hip_get_once_tear_salvage(self._ctx, ctypes.byref(a), ctypes.byref(b)), "cimbar_hip_get_once_tear_salvage")
        return bool(a.value), b.value

    def set_stream_colour_vote(self, on=True):
        """cimbar_hip_set_stream_colour_vote: the colour vote (and, with set_colour_erasure_decode on, the group colour retry) in the stream
        calls; set_group_colour_vote governs the plain combined calls only. A stream samples it in its first call after create /
        combine_stream_reset; a call that finds it changed in mid-stream is refused. Modes 4 / 8 refuse it."""
        self._check(self._lib.cimbar_hip_set_stream_colour_vote(self._ctx, int(bool(on))), "cimbar_hip_set_stream_colour_vote")

    def get_stream_colour_vote(self):
        a = ctypes.c_int()
        self._check(self._lib.cimbar_hip_get_stream_colour_vote(self._ctx, ctypes.byref(a)), "cimbar_hip_get_stream_colour_vote")
        return bool(a.value)

    def rs_decode_erasures(self, blocks, erasures):
        """Errors-and-erasures Reed-Solomon decode of caller-given blocks of this mode's code (cimbar_hip_rs_decode_erasures).
        blocks: (n, RS_BLOCK) uint8; erasures: a list of n sequences of byte positions (at most RS_BLOCK each, any count: more than
        RS_PARITY fails the block). Returns (msgs (n, RS_DATA) uint8, status (n,) int8: -1 libcorrect fails, 0 rejected, 1 accepted)."""
        g = self.geo
        blocks = np.ascontiguousarray(blocks, dtype=np.uint8).reshape(-1, g.RS_BLOCK)
        n = blocks.shape[0]
        if len(erasures) != n:
            raise ValueError("one erasure list per block")
        er = np.zeros((n, g.RS_BLOCK), np.uint8)
        counts = np.zeros(n, np.uint8)
        for b, pos in enumerate(erasures):
            pos = np.asarray(pos, dtype=np.int64).reshape(-1)
            if len(pos) > g.RS_BLOCK or (len(pos) and (pos.min() < 0 or pos.max() >= g.RS_BLOCK)):
                raise ValueError(f"block {b}: at most {g.RS_BLOCK} erasure positions, each < {g.RS_BLOCK}")
            er[b, :len(pos)] = pos
            counts[b] = len(pos)
        msgs = np.zeros((n, g.RS_DATA), np.uint8)
        status = np.zeros(n, np.int8)
        self._check(self._lib.cimbar_hip_rs_decode_erasures(self._ctx, blocks.ctypes.data, n, er.ctypes.data, counts.ctypes.data, MEM_HOST,
                                                            msgs.ctypes.data, status.ctypes.data, None), "cimbar_hip_rs_decode_erasures")
        return msgs, status

    def rs_decode_erasures_device(self, blocks_ptr, n, erasures_ptr, counts_ptr, msgs_ptr, status_ptr, stream=None):
        """Device pointers in and out (layouts as in include/cimbar_hip.h); asynchronous on `stream` (None / 0 = the null stream)."""
        self._check(self._lib.cimbar_hip_rs_decode_erasures(self._ctx, ctypes.c_void_p(blocks_ptr), int(n), ctypes.c_void_p(erasures_ptr),
                                                            ctypes.c_void_p(counts_ptr), MEM_DEVICE, ctypes.c_void_p(msgs_ptr),
                                                            ctypes.c_void_p(status_ptr), ctypes.c_void_p(stream) if stream else None),
                    "cimbar_hip_rs_decode_erasures(device)")

    # ------------------------------------------------------------------ chunk delivery (cimbar_hip_deliver_chunks)
    @staticmethod
    def delivery_flags(dedup=True, remember=False, drop_empty=True):
        return (DELIVER_DEDUP if dedup else 0) | (DELIVER_REMEMBER if remember else 0) | (DELIVER_DROP_EMPTY if drop_empty else 0)

    def deliver_chunks(self, chunks, masks, dedup=True, remember=False, drop_empty=True):
        """chunks (n, chunks per frame, chunk size) uint8 and masks (n,) uint32 as a batch call returns them (or the gchunks / gmasks of a
        combined one). Returns (packed (count, chunk size) uint8, src (count,) int32): the delivered chunks front to back in frame and slot
        order -- packed.tobytes() is what cimbard_fountain_decode walks -- and the linear slot index frame * chunks per frame + slot of each.
        drop_empty leaves out chunks whose header says file size 0, dedup every chunk whose six header bytes an earlier kept chunk of the call
        has, remember (implies dedup) also those an earlier remember call on this decoder delivered."""
        g = self.geo
        masks = np.ascontiguousarray(masks, dtype=np.uint32).reshape(-1)
        n = masks.shape[0]
        chunks = np.ascontiguousarray(chunks, dtype=np.uint8)
        if chunks.size != n * g.CHUNKS_PER_FRAME * g.CHUNK:
            raise CimbarHipError(f"deliver_chunks: chunks must hold {n} x {g.CHUNKS_PER_FRAME} x {g.CHUNK} bytes")
        packed = np.zeros((n * g.CHUNKS_PER_FRAME, g.CHUNK), np.uint8)
        src = np.zeros(n * g.CHUNKS_PER_FRAME, np.int32)
        count = ctypes.c_int32(0)
        rc = self._lib.cimbar_hip_deliver_chunks(self._ctx, chunks.ctypes.data, masks.ctypes.data, n, MEM_HOST,
                                                 self.delivery_flags(dedup, remember, drop_empty), packed.ctypes.data, src.ctypes.data,
                                                 ctypes.addressof(count), MEM_HOST, None)
        self._check(rc, "cimbar_hip_deliver_chunks")
        return packed[:int(rc)], src[:int(rc)]

    def deliver_chunks_device(self, chunks_ptr, masks_ptr, n, packed_ptr, src_ptr, count_ptr, dedup=True, remember=False, drop_empty=True,
                              stream=None, flags=None):
        """Device pointers in and out (src_ptr may be None / 0); asynchronous on `stream` (None / 0 = the null stream). `flags`, when given,
        is passed as it is instead of the three switches."""
        fl = self.delivery_flags(dedup, remember, drop_empty) if flags is None else int(flags)
        rc = self._lib.cimbar_hip_deliver_chunks(self._ctx, ctypes.c_void_p(chunks_ptr), ctypes.c_void_p(masks_ptr), int(n), MEM_DEVICE, fl,
                                                 ctypes.c_void_p(packed_ptr), ctypes.c_void_p(src_ptr) if src_ptr else None,
                                                 ctypes.c_void_p(count_ptr), MEM_DEVICE, ctypes.c_void_p(stream) if stream else None)
        self._check(rc, "cimbar_hip_deliver_chunks(device)")

    def delivery_reset(self, capacity_log2=0):
        """forget every remembered header; capacity_log2 0 = the default table (2^20 entries), else 4 .. 24"""
        self._check(self._lib.cimbar_hip_delivery_reset(self._ctx, int(capacity_log2)), "cimbar_hip_delivery_reset")

    def delivery_stats(self):
        """(remembered headers, table entries, overflowed)"""
        a, b, c = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
        self._check(self._lib.cimbar_hip_delivery_stats(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)), "cimbar_hip_delivery_stats")
        return a.value, b.value, bool(c.value)

    def bufsize(self):
        """cimbard_get_bufsize() of this context's configuration"""
        return self._check(self._lib.cimbar_hip_ctx_bufsize(self._ctx), "cimbar_hip_ctx_bufsize")

    def tap(self, what, n):
        shapes = {
            TAP_BITPLANE: ((n, self.geo.IMG_W * self.geo.IMG_H // 8), np.uint8), TAP_SYMBOLS: ((n, self.geo.NCELLS), np.uint8),
            TAP_COLORS: ((n, self.geo.NCELLS), np.uint8), TAP_DRIFT: ((n, self.geo.NCELLS, 2), np.int8),
            TAP_RS_OK: ((n, self.geo.BLOCKS), np.uint8), TAP_FLOOD: ((n,), np.uint8), TAP_CCM: ((n, 10), np.float32), TAP_FLOOD_PATH: ((n,), np.uint8), TAP_FLOOD_INFO: ((n,), np.uint32), TAP_FLOOD_VERIFY: ((n,), np.uint32), TAP_FLOOD_ROUNDS: ((n,), np.uint32),
            TAP_GROUP_CELLS: ((n, self.geo.NCELLS), np.uint8), TAP_GROUP_MARGIN: ((n, self.geo.NCELLS), np.uint16), TAP_GROUPS: ((n,), np.int32),
            TAP_COLOUR_MARGIN: ((n, self.geo.NCELLS), np.uint32), TAP_SCAN_PATH: ((n,), np.int32),
            TAP_GROUP_COLOUR_MARGIN: ((n, self.geo.NCELLS), np.uint32), TAP_GROUP_COLOUR_WEIGHTS: ((n, self.geo.NCELLS), np.uint32),
            TAP_STREAM_CARRY_WEIGHTS: ((n, self.geo.NCELLS), np.uint32),
            # (n = the captures of the stitched batch; the lines tap has DIM_Y entries per pair on axis 0 and DIM_X on axis 1: tap_stitch_lines)
            TAP_STITCH_CELLS: ((2 * max(n - 1, 0), self.geo.NCELLS), np.uint8),
            TAP_CELL_MEANS: ((n, self.geo.DIM_Y, self.geo.DIM_X), np.uint32),
            # (does not depend on n: a header record and up to FLOOD_LAUNCH_MAX launches; tap_flood_launches reads it as dicts)
            TAP_FLOOD_LAUNCH: ((1 + FLOOD_LAUNCH_MAX, len(FLOOD_LAUNCH_FIELDS)), np.int32),
        }
        shape, dt = shapes[what]
        out = np.zeros(shape, dtype=dt)
        self._check(self._lib.cimbar_hip_tap(self._ctx, what, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_stitch_cells(self, n, stream=False):
        """TAP_STITCH_CELLS of the last stitched batch of n captures: (2 (n - 1), NCELLS) uint8, colour << 4 | symbol; stream=True: (2n, NCELLS)"""
        out = np.zeros((2 * (n if stream else max(n - 1, 0)), self.geo.NCELLS), dtype=np.uint8)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_CELLS, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_stitch_lines(self, n, axis=0, stream=False):
        """TAP_STITCH_LINES of the last stitched batch of n captures on `axis`: (n - 1, L) uint16, the agreeing cells per line; stream=True:
        that batch was a stitched-stream call, (n, L)"""
        out = np.zeros((n if stream else max(n - 1, 0), self.geo.DIM_Y if axis == 0 else self.geo.DIM_X), dtype=np.uint16)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_STITCH_LINES, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_repeat_sig(self, n):
        """TAP_REPEAT_SIG of the last once-call of n captures: (n, NCELLS) uint8, the ink signature 0..3 of every cell"""
        out = np.zeros((n, self.geo.NCELLS), dtype=np.uint8)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_REPEAT_SIG, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_repeat_agree(self, n, stream=False):
        """TAP_REPEAT_AGREE of the last once-call of n captures: (n - 1,) uint32, the cells of equal signature in captures k and k + 1;
        stream=True, after a once-stream call: (n,), entry 0 against the carried capture (0 when the carry is unusable)"""
        out = np.zeros(n if stream else max(n - 1, 0), dtype=np.uint32)
        if out.size:
            self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_REPEAT_AGREE, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_once_rescue(self, n):
        """TAP_ONCE_RESCUE of the last plain once-call of n captures with set_once_rescue on: (n,) int32 per run slot, -1 = not tried, else
        the chunk bits the rescue added to the OR of the members' masks"""
        out = np.zeros(n, dtype=np.int32)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_ONCE_RESCUE, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_once_tear(self, n):
        """TAP_ONCE_TEAR of the last plain once-call of n captures with set_once_tear_skip on: (n, 4) int32 {axis * 2 + o, s, first, last},
        {-1, -1, 0, 0} for a capture that is no candidate"""
        out = np.zeros((n, 4), dtype=np.int32)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_ONCE_TEAR, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_once_salvage(self, n):
        """TAP_ONCE_SALVAGE of the last plain once-call of n captures in which set_once_tear_salvage was effective: (n, 8) int32 per run slot
        {kp, axis_p, lo_p, hi_p, kf, axis_f, lo_f, hi_f}; {-1, -1, 0, 0} for a partial the run lacks and for a run that was not tried"""
        out = np.zeros((n, 8), dtype=np.int32)
        self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_ONCE_SALVAGE, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        return out

    def tap_flood_launches(self):
        """TAP_FLOOD_LAUNCH of the batch issued last: (launches, areas_reserved) -- one dict per exact-replay launch (k_flood3) in issue order
        with the keys FLOOD_LAUNCH_FIELDS (instance 3 / 4 / 8 = frames per CU; workgroup b of `grid` spills into area area0 + b; frames from `grid`
        on are handed out through counter pair `counter`; flags 0 = the batch's own, 1 = the verify replay, 2 = the relaxed flood's fallback), and
        the spill areas the batch asked the context to hold. Host bookkeeping: answered at once, also while pipelined batches are in flight."""
        out = np.zeros((1 + FLOOD_LAUNCH_MAX, len(FLOOD_LAUNCH_FIELDS)), dtype=np.int32)
        got = self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_FLOOD_LAUNCH, out.ctypes.data, out.nbytes), "cimbar_hip_tap")
        asked, held, count = (int(v) for v in out[0, :3])
        assert got == (1 + count) * out.shape[1] * 4 and held >= asked, (got, asked, held, count)
        return [dict(zip(FLOOD_LAUNCH_FIELDS, (int(v) for v in row))) for row in out[1:1 + count]], asked

    def tap_once_rescue_cells(self, n_tried):
        """TAP_ONCE_RESCUE_CELLS of that call: (n_tried, NCELLS) uint8, the combined cells of the tried runs in run order, colour << 4 | symbol"""
        out = np.zeros((max(n_tried, 1), self.geo.NCELLS), dtype=np.uint8)   # (never a null pointer; a call that tried nothing writes nothing)
        got = self._check(self._lib.cimbar_hip_tap(self._ctx, TAP_ONCE_RESCUE_CELLS, out.ctypes.data, n_tried * self.geo.NCELLS), "cimbar_hip_tap")
        assert got == n_tried * self.geo.NCELLS, (got, n_tried)
        return out[:n_tried]

    def enable_timing(self, on=True):
        self._lib.cimbar_hip_enable_timing(self._ctx, int(bool(on)))

    def stage_times(self):
        names = (ctypes.c_char_p * 16)()
        ms = (ctypes.c_float * 16)()
        k = self._check(self._lib.cimbar_hip_stage_times(self._ctx, names, ms, 16), "cimbar_hip_stage_times")
        return {names[i].decode(): float(ms[i]) for i in range(k)}


class AutoDecoder:
    """Mode auto-detection (cimbar_hip_auto_*): one decoder per candidate mode and ONE carried colour-correction matrix, shared by all of
    them -- the reference's receiver in auto mode (web/recv.js), batched. See include/cimbar_hip.h."""

    def __init__(self, device=0, modes=(66, 68, 67, 4), lib_path=None):
        self._lib = load_library(lib_path)
        self._a = ctypes.c_void_p()
        self.modes = tuple(int(m) for m in modes)
        arr = (ctypes.c_int32 * len(self.modes))(*self.modes)
        rc = self._lib.cimbar_hip_auto_create(int(device), arr, len(self.modes), ctypes.byref(self._a))
        if rc != 0:
            self._a = ctypes.c_void_p()
            raise CimbarHipError(f"cimbar_hip_auto_create(device={device}, modes={self.modes}) failed: {_ERR.get(rc, rc)} "
                                 "(a gfx950 GPU is required; there is no CPU fallback)")
        self.device = device
        self.slot = self._lib.cimbar_hip_auto_bufsize(self._a)

    def close(self):
        if getattr(self, "_a", None) and self._a.value:
            self._lib.cimbar_hip_auto_destroy(self._a)
            self._a = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc, what):
        if rc < 0:
            msg = self._lib.cimbar_hip_auto_last_error(self._a).decode("utf-8", "replace")
            raise CimbarHipError(f"{what}: {_ERR.get(int(rc), rc)} {msg}")
        return rc

    def bufsize(self):
        return self._check(self._lib.cimbar_hip_auto_bufsize(self._a), "cimbar_hip_auto_bufsize")

    def reset_ccm(self):
        self._check(self._lib.cimbar_hip_auto_reset_ccm(self._a), "cimbar_hip_auto_reset_ccm")

    def get_ccm(self):
        out = (ctypes.c_float * 9)()
        rc = self._check(self._lib.cimbar_hip_auto_get_ccm(self._a, out), "cimbar_hip_auto_get_ccm")
        return bool(rc), np.array(list(out), dtype=np.float32).reshape(3, 3)

    def set_ccm(self, m):
        arr = (ctypes.c_float * 9)(*[float(x) for x in np.asarray(m, dtype=np.float32).reshape(-1)])
        self._check(self._lib.cimbar_hip_auto_set_ccm(self._a, arr), "cimbar_hip_auto_set_ccm")

    def _order(self, order):
        if order is None:
            return None, 0
        o = np.ascontiguousarray(order, dtype=np.int32)
        return o, o.size

    def scan_extract_decode_batch_raw(self, captures, preprocess=-1, color_correction=2, size=None, fmt=3, order=None):
        """-> (good_bytes, slots (n, bufsize) uint8, masks (n,), modes (n,), status (n,)): the C ABI's outputs as they are"""
        captures, n, w, h, fmt = _captures(self._lib, captures, size, fmt)
        slots = np.zeros((n, self.slot), dtype=np.uint8)
        masks = np.zeros(n, dtype=np.uint32)
        modes = np.zeros(n, dtype=np.int32)
        status = np.zeros(n, dtype=np.int32)
        o, no = self._order(order)
        rc = self._check(self._lib.cimbar_hip_auto_scan_extract_decode_batch_fmt(
            self._a, o.ctypes.data if o is not None else None, no, captures.ctypes.data, w, h, fmt, n, MEM_HOST, int(preprocess),
            int(color_correction), slots.ctypes.data, masks.ctypes.data, modes.ctypes.data, status.ctypes.data, MEM_HOST, None),
            "cimbar_hip_auto_scan_extract_decode_batch_fmt")
        return int(rc), slots, masks, modes, status

    def scan_extract_decode_batch(self, captures, preprocess=-1, color_correction=2, size=None, fmt=3, order=None):
        """-> (good_bytes, chunks, masks (n,), modes (n,), status (n,)); chunks[f] = (chunks per frame, chunk size) of the accepted mode,
        an empty (0, 0) array for a capture no candidate delivered for"""
        total, slots, masks, modes, status = self.scan_extract_decode_batch_raw(captures, preprocess, color_correction, size, fmt, order)
        chunks = []
        for f in range(len(modes)):
            if modes[f] == 0:
                chunks.append(np.zeros((0, 0), np.uint8))
                continue
            g = geometry.for_mode(int(modes[f]))
            chunks.append(slots[f, : g.CHUNKS_PER_FRAME * g.CHUNK].reshape(g.CHUNKS_PER_FRAME, g.CHUNK))
        return total, chunks, masks, modes, status

    def scan_extract_decode_device(self, d_captures, w, h, n, d_slots, d_masks, d_modes, d_status, preprocess=-1, color_correction=2, fmt=3,
                                   order=None, stream=None):
        """device-memory captures and outputs (raw pointers) on `stream` (a HIP stream handle, or None)"""
        o, no = self._order(order)
        return self._check(self._lib.cimbar_hip_auto_scan_extract_decode_batch_fmt(
            self._a, o.ctypes.data if o is not None else None, no, ctypes.c_void_p(d_captures), w, h, int(fmt), n, MEM_DEVICE, int(preprocess),
            int(color_correction), ctypes.c_void_p(d_slots), ctypes.c_void_p(d_masks), ctypes.c_void_p(d_modes), ctypes.c_void_p(d_status),
            MEM_DEVICE, ctypes.c_void_p(stream) if stream else None), "cimbar_hip_auto_scan_extract_decode_batch_fmt(device)")
