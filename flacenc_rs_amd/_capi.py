"""ctypes binding of the C ABI in ``include/flacenc_hip.h`` (libflacenc_hip.so).

This is plumbing for the Python test/bench drivers: every compute call goes
through the same ``extern "C"`` entry points a Rust/C host would bind.  There is
no CPU fallback -- if the HIP library is missing or no GPU is present the calls
raise.
"""
from __future__ import annotations

import ctypes as C
import os
import sys

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# FLACENC_HIP_LIB: development aid for A/B timing of two builds on one GPU box; never a fallback
LIB_PATH = os.environ.get("FLACENC_HIP_LIB") or os.path.join(_HERE, "libflacenc_hip.so")
# The same objects + the test / profiling hooks of csrc/flacenc_hip_debug.h (the product library has none of them):
# what Handle(dev, hooks=True) loads.  An A/B library named by FLACENC_HIP_LIB (tools/variant_*.sh build them with the
# hooks) serves both.
HOOKS_LIB_PATH = os.environ.get("FLACENC_HIP_LIB") or os.path.join(_HERE, "libflacenc_hip_hooks.so")

OK = 0
ERR_BAD_CONFIG = -1
ERR_BAD_ARGUMENT = -2
ERR_DEVICE = -3
ERR_UNSUPPORTED = -4
ERR_NO_DEVICE = -5
_ERR_NAMES = {
    ERR_BAD_CONFIG: "BAD_CONFIG",
    ERR_BAD_ARGUMENT: "BAD_ARGUMENT",
    ERR_DEVICE: "DEVICE",
    ERR_UNSUPPORTED: "UNSUPPORTED",
    ERR_NO_DEVICE: "NO_DEVICE",
}

WINDOW_RECTANGLE = 0
WINDOW_TUKEY = 1
WINDOW_PARTIAL_TUKEY = 2  # FLAG_WINDOW_SEARCH's extra windows only: T(e - s) on [s, e)
WINDOW_PUNCHOUT_TUKEY = 3  # T(s) on [0, s), zero on [s, e), T(n - e) on [e, n)
MAX_LPC_WINDOWS = 8  # FLACENC_HIP_MAX_LPC_WINDOWS: the config's window + at most 7 extra windows
WINDOW_UNIT = 65536  # FLACENC_HIP_WINDOW_UNIT: start / end of an extra window in 1/65536 of the block
# the extra windows of a fresh handle, (type, alpha, start, end) -- include/flacenc_hip.h, FLACENC_HIP_FLAG_WINDOW_SEARCH
DEFAULT_LPC_WINDOWS = (
    (WINDOW_PARTIAL_TUKEY, 0.2, 0, 36044),
    (WINDOW_PARTIAL_TUKEY, 0.2, 29492, 65536),
    (WINDOW_PUNCHOUT_TUKEY, 0.2, 0, 21845),
    (WINDOW_PUNCHOUT_TUKEY, 0.2, 21845, 43690),
    (WINDOW_PUNCHOUT_TUKEY, 0.2, 43690, 65536),
)
FLAG_ALLOW_ORDER_32 = 1
MEM_HOST = 0
MEM_DEVICE = 1
COMM_ID_BYTES = 128  # FLACENC_HIP_COMM_ID_BYTES
# FLACENC_HIP_DECODE_* status bits of the frame decoder, FLACENC_HIP_INDEX_ERROR
DECODE_BAD_HEADER, DECODE_HEADER_CRC, DECODE_FRAME_CRC, DECODE_PARSE = 1, 2, 4, 8
DECODE_LENGTH, DECODE_STREAM_MISMATCH, DECODE_UNSUPPORTED, DECODE_MISMATCH = 16, 32, 64, 128
DECODE_NO_ROOM, DECODE_CHAIN = 256, 512  # totals[3] of flacenc_hip_decode_pcm: why the call stopped
DECODE_RANGE_END = 1024  # totals[r][1] of flacenc_hip_decode_ranges: the chain ended at the span's end before the range
SAMPLE_I32, SAMPLE_F32 = 0, 1  # FLACENC_HIP_SAMPLE_*: sample_format of flacenc_hip_decode_ranges_planar
ENCODE_NO_ROOM = 256  # FLACENC_HIP_ENCODE_NO_ROOM: totals[s][3] of flacenc_hip_encode_streams
INDEX_ERROR = 1 << 63
VARIABLE_OVERFLOW = 1 << 63  # FLACENC_HIP_VARIABLE_OVERFLOW: totals[0] of flacenc_hip_encode_variable*

# every symbol include/flacenc_hip.h declares
ABI_VERSION = 6  # FLACENC_HIP_ABI_VERSION of include/flacenc_hip.h
DEBUG_SYMBOLS = ("flacenc_hip_debug_set_stamps", "flacenc_hip_debug_set_fixed_keys", "flacenc_hip_debug_set_cert_stats",
                 "flacenc_hip_debug_set_adaptive_order", "flacenc_hip_debug_adaptive_state",
                 "flacenc_hip_debug_set_order_guess_trace", "flacenc_hip_debug_set_stream_chunk",
                 "flacenc_hip_debug_last_stream_plan", "flacenc_hip_debug_last_stream_buffers",
                 "flacenc_hip_debug_set_decode_plan", "flacenc_hip_debug_last_decode_plan",
                 "flacenc_hip_debug_last_decode_streams_plan", "flacenc_hip_debug_last_decode_ranges_plan",
                 "flacenc_hip_debug_last_recover_plan",
                 "flacenc_hip_debug_set_encode_streams_chunk",
                 "flacenc_hip_debug_last_encode_streams_plan", "flacenc_hip_debug_streams_fill",
                 "flacenc_hip_debug_set_planar_fill_form", "flacenc_hip_debug_segmax_scan",
                 "flacenc_hip_debug_scratch_bytes", "flacenc_hip_debug_last_search_slices")
EXPORTED_SYMBOLS = (
    "flacenc_hip_abi_version",
    "flacenc_hip_device_count",
    "flacenc_hip_create",
    "flacenc_hip_destroy",
    "flacenc_hip_last_error",
    "flacenc_hip_verify_config",
    "flacenc_hip_window_weights",
    "flacenc_hip_set_lpc_windows",
    "flacenc_hip_set_order_guesses",
    "flacenc_hip_set_precision_floor",
    "flacenc_hip_set_max_bits_per_sample",
    "flacenc_hip_set_max_encode_bits_per_sample",
    "flacenc_hip_lpc_window_weights",
    "flacenc_hip_qlpc_batch",
    "flacenc_hip_qlpc_batch_async",
    "flacenc_hip_stereo_qlpc_batch",
    "flacenc_hip_stereo_qlpc_batch_async",
    "flacenc_hip_encode_stereo_frames",
    "flacenc_hip_encode_stereo_frames_async",
    "flacenc_hip_fixed_lpc_batch",
    "flacenc_hip_fixed_lpc_batch_async",
    "flacenc_hip_stereo_frame_bytes_bound",
    "flacenc_hip_pack_stereo_frames",
    "flacenc_hip_pack_stereo_frames_async",
    "flacenc_hip_stereo_frame_lengths_async",
    "flacenc_hip_place_frames_async",
    "flacenc_hip_frame_wire_bytes",
    "flacenc_hip_stereo_frame_wire_async",
    "flacenc_hip_stream_offsets_async",
    "flacenc_hip_encode_pcm_stereo",
    "flacenc_hip_encode_pcm",
    "flacenc_hip_host_alloc",
    "flacenc_hip_host_free",
    "flacenc_hip_set_host_threads",
    "flacenc_hip_encode_frames",
    "flacenc_hip_encode_frames_async",
    "flacenc_hip_frame_bytes_bound",
    "flacenc_hip_pack_frames",
    "flacenc_hip_pack_frames_async",
    "flacenc_hip_fill_le_bytes",
    "flacenc_hip_fill_le_bytes_async",
    "flacenc_hip_encode_pack_stereo_frames_async",
    "flacenc_hip_encode_pack_frames_async",
    "flacenc_hip_encode_pack_frames_wide",
    "flacenc_hip_comm_unique_id",
    "flacenc_hip_comm_create",
    "flacenc_hip_comm_destroy",
    "flacenc_hip_comm_info",
    "flacenc_hip_allgather_async",
    "flacenc_hip_allgather_records_async",
    "flacenc_hip_decode_frames_async",
    "flacenc_hip_decode_frames",
    "flacenc_hip_verify_frames_async",
    "flacenc_hip_index_frames_async",
    "flacenc_hip_pack_le_bytes",
    "flacenc_hip_decode_pcm",
    "flacenc_hip_decode_streams",
    "flacenc_hip_md5_spans",
    "flacenc_hip_decode_streams_md5",
    "flacenc_hip_recover_streams",
    "flacenc_hip_decode_ranges",
    "flacenc_hip_decode_ranges_planar",
    "flacenc_hip_encode_streams_frames",
    "flacenc_hip_encode_streams",
    "flacenc_hip_encode_streams_planar",
    "flacenc_hip_variable_bytes_bound",
    "flacenc_hip_variable_max_frames",
    "flacenc_hip_encode_variable_async",
    "flacenc_hip_encode_variable",
    "flacenc_hip_synchronize",
    "flacenc_sigen_fill_frames",
    "flacenc_sigen_fill_frames_strided",
)


class QlpcConfig(C.Structure):
    """flacenc_hip_qlpc_config == the path's fields of config::Qlpc / config::Prc."""

    _fields_ = [
        ("lpc_order", C.c_uint32),
        ("quant_precision", C.c_uint32),
        ("window_type", C.c_uint32),
        ("tukey_alpha", C.c_float),
        ("max_rice_parameter", C.c_uint32),
        ("flags", C.c_uint32),
        ("use_direct_mse", C.c_uint32),
        ("mae_optimization_steps", C.c_uint32),
    ]


# flacenc_hip_subframe_params (352 bytes)
PARAMS_DTYPE = np.dtype(
    [
        ("coefs", np.int16, (32,)),
        ("order", np.uint8),
        ("shift", np.int8),
        ("precision", np.uint8),
        ("rice_order", np.uint8),
        ("status", np.int32),
        ("code_bits", np.uint64),
        ("subframe_bits", np.uint64),
        ("sum_quotients", np.uint64),
        ("rice_params", np.uint8, (256,)),
    ],
    align=True,
)
assert PARAMS_DTYPE.itemsize == 352


# flacenc_hip_stream_desc (48 bytes): one stream of flacenc_hip_decode_streams
STREAM_DESC_DTYPE = np.dtype([("offset", "<u8"), ("n_bytes", "<u8"), ("out_offset", "<u8"), ("out_capacity", "<u8"),
                              ("channels", "<u4"), ("bits_per_sample", "<u4"), ("max_block_size", "<u4"),
                              ("bytes_per_sample", "<u4")])
assert STREAM_DESC_DTYPE.itemsize == 48


# flacenc_hip_range_desc (32 bytes): one range of flacenc_hip_decode_ranges
RANGE_DESC_DTYPE = np.dtype([("first_sample", "<u8"), ("n_samples", "<u8"), ("out_offset", "<u8"), ("stream", "<u4"),
                             ("reserved", "<u4")])
assert RANGE_DESC_DTYPE.itemsize == 32

# flacenc_hip_pcm_stream_desc (48 bytes): one stream of flacenc_hip_encode_streams
PCM_STREAM_DESC_DTYPE = np.dtype([("offset", "<u8"), ("total_samples", "<u8"), ("out_offset", "<u8"),
                                  ("out_capacity", "<u8"), ("channels", "<u4"), ("bits_per_sample", "<u4"),
                                  ("bytes_per_sample", "<u4"), ("sample_rate", "<u4")])
assert PCM_STREAM_DESC_DTYPE.itemsize == 48


class FrameConfig(C.Structure):
    """flacenc_hip_frame_config: the config::Encoder fields that steer encode_frame."""

    _fields_ = [
        ("qlpc", QlpcConfig),
        ("use_constant", C.c_uint32),
        ("use_fixed", C.c_uint32),
        ("use_lpc", C.c_uint32),
        ("use_leftside", C.c_uint32),
        ("use_rightside", C.c_uint32),
        ("use_midside", C.c_uint32),
        ("fixed_max_order", C.c_uint32),
        ("fixed_order_sel", C.c_uint32),
        ("fixed_partitions", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


LAYOUT_SUBFRAMES = 0
LAYOUT_STEREO_FRAMES = 1
ORDERSEL_BITCOUNT = 0
ORDERSEL_APPROXENT = 1
KIND_CONSTANT, KIND_VERBATIM, KIND_FIXED, KIND_LPC = 0, 1, 2, 3


def make_frame_config(qlpc: QlpcConfig | None = None, use_constant=True, use_fixed=False, use_lpc=True,
                      use_leftside=True, use_rightside=True, use_midside=True, fixed_max_order=4,
                      fixed_order_sel=ORDERSEL_APPROXENT, fixed_partitions=16) -> FrameConfig:
    """config::SubFrameCoding / config::Fixed / StereoCoding (src/config.rs:167-183, 236-244, 137-144).
    The reference's default has use_fixed = True; here it is opt-in so that the QLPC-only analysis
    the north-star metric is quoted on stays the default of the bench."""
    return FrameConfig(qlpc or make_config(), int(use_constant), int(use_fixed), int(use_lpc),
                       int(use_leftside), int(use_rightside), int(use_midside), int(fixed_max_order),
                       int(fixed_order_sel), int(fixed_partitions), 0)


# flacenc_hip_channel_result (368 bytes): one channel of an Independent(n) frame
# the record of flacenc_hip_debug_set_order_guess_trace (csrc/flacenc_hip_debug.h), 264 bytes: orders 1..eligible are
# eligible, bit o - 1 of mask says order o is a guess, cost[o - 1] for o <= eligible and +0.0 above
ORDER_GUESS_TRACE_DTYPE = np.dtype([("eligible", "<u4"), ("mask", "<u4"), ("cost", "<f8", 32)])
assert ORDER_GUESS_TRACE_DTYPE.itemsize == 264

CHANNEL_RESULT_DTYPE = np.dtype(
    [("kind", np.uint8), ("analysis_status", np.uint8), ("pad", np.uint8, (2,)), ("dc_offset", np.int32), ("bits", np.uint64),
     ("params", PARAMS_DTYPE)], align=False)
assert CHANNEL_RESULT_DTYPE.itemsize == 368

# flacenc_hip_stereo_frame_result (752 bytes)
FRAME_RESULT_DTYPE = np.dtype(
    [
        ("channel_assignment", np.uint8),
        ("kind", np.uint8, (2,)),
        ("role", np.uint8, (2,)),
        ("analysis_status", np.uint8),
        ("pad", np.uint8, (2,)),
        ("dc_offset", np.int32, (2,)),
        ("bits", np.uint64, (4,)),
        ("lpc", PARAMS_DTYPE, (2,)),
    ],
    align=True,
)
assert FRAME_RESULT_DTYPE.itemsize == 752


def stream_descs(streams) -> np.ndarray:
    """A STREAM_DESC_DTYPE array from one, or from rows (offset, n_bytes, out_offset, out_capacity, channels,
    bits_per_sample, max_block_size, bytes_per_sample); never empty memory, so that its address is not NULL."""
    if isinstance(streams, np.ndarray) and streams.dtype == STREAM_DESC_DTYPE:
        table = np.ascontiguousarray(streams)
    else:
        table = np.array([tuple(int(v) for v in row) for row in streams], STREAM_DESC_DTYPE)
    if table.size == 0:
        return np.zeros(1, STREAM_DESC_DTYPE)[:0]
    return table


def range_descs(ranges) -> np.ndarray:
    """A RANGE_DESC_DTYPE array from one, or from rows (first_sample, n_samples, out_offset, stream[, reserved])."""
    if isinstance(ranges, np.ndarray) and ranges.dtype == RANGE_DESC_DTYPE:
        table = np.ascontiguousarray(ranges)
    else:
        table = np.array([tuple(int(v) for v in (tuple(row) + (0,))[:5]) for row in ranges], RANGE_DESC_DTYPE)
    if len(table) == 0:  # never empty memory, so that its address is not NULL
        return np.zeros(1, RANGE_DESC_DTYPE)[:0]
    return table


def pcm_stream_descs(streams) -> np.ndarray:
    """A PCM_STREAM_DESC_DTYPE array from one, or from rows (offset, total_samples, out_offset, out_capacity, channels,
    bits_per_sample, bytes_per_sample, sample_rate); never empty memory, so that its address is not NULL."""
    if isinstance(streams, np.ndarray) and streams.dtype == PCM_STREAM_DESC_DTYPE:
        table = np.ascontiguousarray(streams)
    else:
        table = np.array([tuple(int(v) for v in row) for row in streams], PCM_STREAM_DESC_DTYPE)
    if table.size == 0:
        return np.zeros(1, PCM_STREAM_DESC_DTYPE)[:0]
    return table


def encode_streams_frames(streams, block_size: int) -> int:
    """flacenc_hip_encode_streams_frames: the sum of ceil(total_samples / block_size) over the table."""
    table = pcm_stream_descs(streams)
    return int(load().flacenc_hip_encode_streams_frames(table.ctypes.data, len(table), block_size))


class FlacencHipError(RuntimeError):
    def __init__(self, code, message=""):
        self.code = code
        super().__init__(f"flacenc_hip error {_ERR_NAMES.get(code, code)}: {message}")


_libs = {}


def load() -> C.CDLL:
    """Load libflacenc_hip.so (the product library); raises if it has not been built (no fallback)."""
    return _load_path(LIB_PATH)


def load_hooks() -> C.CDLL:
    """Load libflacenc_hip_hooks.so: the product's objects + flacenc_hip_debug_* (tests and tools only)."""
    return _load_path(HOOKS_LIB_PATH)


def _load_path(LIB_PATH: str) -> C.CDLL:
    if LIB_PATH in _libs:
        return _libs[LIB_PATH]
    if not os.path.exists(LIB_PATH):
        raise FileNotFoundError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`"
            " or `make -C flacenc_rs_amd/csrc`")
    # One HIP runtime per process: PyTorch ships its own libamdhip64 and the library links the
    # system one under the same SONAME, so whichever is loaded first serves both.  PyTorch cannot
    # work on the system copy ("No HIP GPUs are available"), the library is fine on PyTorch's --
    # so in a process that will use both (tests, bench) PyTorch has to come first.
    if "torch" not in sys.modules:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    L = C.CDLL(LIB_PATH)
    vp, i32p, u8p, f64p = C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p
    L.flacenc_hip_abi_version.restype = C.c_int
    # (the config structs are passed by value inside others: a library of another ABI revision reads them shifted)
    if L.flacenc_hip_abi_version() != ABI_VERSION:
        raise RuntimeError("%s has ABI %d, this binding is written for %d" % (LIB_PATH, L.flacenc_hip_abi_version(), ABI_VERSION))
    L.flacenc_hip_device_count.restype = C.c_int
    L.flacenc_hip_create.argtypes = [C.POINTER(vp), C.c_int]
    L.flacenc_hip_create.restype = C.c_int
    L.flacenc_hip_destroy.argtypes = [vp]
    L.flacenc_hip_destroy.restype = None
    L.flacenc_hip_last_error.argtypes = [vp]
    L.flacenc_hip_last_error.restype = C.c_char_p
    L.flacenc_hip_verify_config.argtypes = [C.POINTER(QlpcConfig)]
    L.flacenc_hip_verify_config.restype = C.c_int
    L.flacenc_hip_window_weights.argtypes = [C.POINTER(QlpcConfig), C.c_uint32, vp]
    L.flacenc_hip_window_weights.restype = C.c_int
    L.flacenc_hip_set_lpc_windows.argtypes = [vp, vp, vp, vp, vp, C.c_uint32]
    L.flacenc_hip_set_lpc_windows.restype = C.c_int
    L.flacenc_hip_set_order_guesses.argtypes = [vp, C.c_uint32]
    L.flacenc_hip_set_order_guesses.restype = C.c_int
    L.flacenc_hip_set_precision_floor.argtypes = [vp, C.c_uint32]
    L.flacenc_hip_set_precision_floor.restype = C.c_int
    L.flacenc_hip_set_max_bits_per_sample.argtypes = [vp, C.c_uint32]
    L.flacenc_hip_set_max_bits_per_sample.restype = C.c_int
    L.flacenc_hip_set_max_encode_bits_per_sample.argtypes = [vp, C.c_uint32]
    L.flacenc_hip_set_max_encode_bits_per_sample.restype = C.c_int
    L.flacenc_hip_lpc_window_weights.argtypes = [C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_uint32, vp]
    L.flacenc_hip_lpc_window_weights.restype = C.c_int
    L.flacenc_hip_synchronize.argtypes = [vp]
    L.flacenc_hip_synchronize.restype = C.c_int
    # test / profiling hooks (csrc/flacenc_hip_debug.h): present in builds with -DFLACENC_HIP_DEBUG_HOOKS only
    for name in DEBUG_SYMBOLS:
        if hasattr(L, name):
            getattr(L, name).argtypes = [vp, vp]
            getattr(L, name).restype = C.c_int
    if hasattr(L, "flacenc_hip_debug_set_adaptive_order"):
        L.flacenc_hip_debug_set_adaptive_order.argtypes = [vp, C.c_int]
        L.flacenc_hip_debug_adaptive_state.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "flacenc_hip_debug_set_stream_chunk"):
        L.flacenc_hip_debug_set_stream_chunk.argtypes = [vp, C.c_size_t]
        L.flacenc_hip_debug_last_stream_plan.argtypes = [vp, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
        L.flacenc_hip_debug_last_stream_buffers.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    if hasattr(L, "flacenc_hip_debug_set_encode_streams_chunk"):
        L.flacenc_hip_debug_set_encode_streams_chunk.argtypes = [vp, C.c_size_t]
        L.flacenc_hip_debug_set_planar_fill_form.argtypes = [vp, C.c_int]
        L.flacenc_hip_debug_streams_fill.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32,
                                                     vp, C.c_size_t]
    if hasattr(L, "flacenc_hip_debug_segmax_scan"):
        L.flacenc_hip_debug_segmax_scan.argtypes = [vp, vp, vp, C.c_size_t, C.c_size_t, vp]
    if hasattr(L, "flacenc_hip_debug_scratch_bytes"):
        L.flacenc_hip_debug_scratch_bytes.argtypes = [vp, vp]
        L.flacenc_hip_debug_last_search_slices.argtypes = [vp, C.POINTER(C.c_uint32)]
    if hasattr(L, "flacenc_hip_debug_set_decode_plan"):
        L.flacenc_hip_debug_set_decode_plan.argtypes = [vp, C.c_size_t, C.c_size_t]
        L.flacenc_hip_debug_last_decode_plan.argtypes = [vp] + [C.POINTER(C.c_size_t)] * 4
    batch_args = [vp, C.POINTER(QlpcConfig), i32p, C.c_size_t, C.c_uint32, C.c_size_t, u8p, vp, i32p,
                  C.c_size_t, f64p, f64p]
    L.flacenc_hip_qlpc_batch.argtypes = batch_args + [C.c_int]
    L.flacenc_hip_qlpc_batch.restype = C.c_int
    L.flacenc_hip_qlpc_batch_async.argtypes = batch_args + [vp]
    L.flacenc_hip_qlpc_batch_async.restype = C.c_int
    stereo_args = [vp, C.POINTER(QlpcConfig), i32p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32,
                   vp, i32p, C.c_size_t]
    L.flacenc_hip_stereo_qlpc_batch.argtypes = stereo_args + [C.c_int]
    L.flacenc_hip_stereo_qlpc_batch.restype = C.c_int
    L.flacenc_hip_stereo_qlpc_batch_async.argtypes = stereo_args + [vp]
    L.flacenc_hip_stereo_qlpc_batch_async.restype = C.c_int
    fixed_args = [vp, C.POINTER(FrameConfig), i32p, C.c_size_t, C.c_uint32, C.c_size_t, vp, C.c_uint32,
                  C.c_int, vp, i32p, C.c_size_t, vp]
    L.flacenc_hip_fixed_lpc_batch.argtypes = fixed_args + [C.c_int]
    L.flacenc_hip_fixed_lpc_batch.restype = C.c_int
    L.flacenc_hip_fixed_lpc_batch_async.argtypes = fixed_args + [vp]
    L.flacenc_hip_fixed_lpc_batch_async.restype = C.c_int
    pack_args = [vp, i32p, C.c_size_t, C.c_uint32, C.c_size_t, vp, i32p, C.c_size_t, C.c_uint32, C.c_uint32,
                 C.c_uint32, C.c_uint32, vp, C.c_size_t, vp]
    L.flacenc_hip_pack_stereo_frames.argtypes = pack_args + [C.c_int]
    L.flacenc_hip_pack_stereo_frames.restype = C.c_int
    L.flacenc_hip_pack_stereo_frames_async.argtypes = pack_args + [vp]
    L.flacenc_hip_pack_stereo_frames_async.restype = C.c_int
    L.flacenc_hip_stereo_frame_lengths_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                          C.c_uint32, C.c_uint32, vp, vp]
    L.flacenc_hip_stereo_frame_lengths_async.restype = C.c_int
    L.flacenc_hip_place_frames_async.argtypes = [vp, vp, vp, vp, C.c_size_t, vp, vp, vp]
    L.flacenc_hip_place_frames_async.restype = C.c_int
    L.flacenc_hip_frame_wire_bytes.argtypes = [C.c_uint32]
    L.flacenc_hip_frame_wire_bytes.restype = C.c_size_t
    L.flacenc_hip_stereo_frame_wire_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                       C.c_uint32, C.c_uint32, vp, C.c_size_t, vp, vp]
    L.flacenc_hip_stereo_frame_wire_async.restype = C.c_int
    L.flacenc_hip_stream_offsets_async.argtypes = [vp, vp, C.c_size_t, C.c_uint32, C.c_uint64, vp, vp, vp, vp]
    L.flacenc_hip_stream_offsets_async.restype = C.c_int
    L.flacenc_hip_encode_pcm_stereo.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_uint64, C.c_uint32, C.c_uint32,
                                                C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp,
                                                C.POINTER(C.c_uint64)]
    L.flacenc_hip_encode_pcm_stereo.restype = C.c_int
    L.flacenc_hip_encode_pcm.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32,
                                         C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t, vp,
                                         C.POINTER(C.c_uint64)]
    L.flacenc_hip_encode_pcm.restype = C.c_int
    L.flacenc_hip_host_alloc.argtypes = [C.c_size_t]
    L.flacenc_hip_host_alloc.restype = C.c_void_p
    L.flacenc_hip_host_free.argtypes = [C.c_void_p]
    L.flacenc_hip_host_free.restype = None
    L.flacenc_hip_set_host_threads.argtypes = [C.c_void_p, C.c_int]
    L.flacenc_hip_set_host_threads.restype = C.c_int
    L.flacenc_hip_fill_le_bytes.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32, i32p,
                                            C.c_size_t, C.c_int]
    L.flacenc_hip_fill_le_bytes.restype = C.c_int
    L.flacenc_hip_fill_le_bytes_async.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, C.c_uint32,
                                                  vp, C.c_size_t, vp]
    L.flacenc_hip_fill_le_bytes_async.restype = C.c_int
    L.flacenc_hip_encode_pack_stereo_frames_async.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_size_t, C.c_uint32,
                                                               C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                               C.c_uint32, vp, vp, C.c_size_t, vp, vp]
    L.flacenc_hip_encode_pack_stereo_frames_async.restype = C.c_int
    L.flacenc_hip_encode_pack_frames_async.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_size_t, C.c_uint32,
                                                        C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                        C.c_uint32, vp, vp, C.c_size_t, vp, vp]
    L.flacenc_hip_encode_pack_frames_async.restype = C.c_int
    L.flacenc_hip_encode_pack_frames_wide.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_size_t, C.c_uint32,
                                                      C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                                      C.c_uint32, vp, C.c_size_t, vp]
    L.flacenc_hip_encode_pack_frames_wide.restype = C.c_int
    L.flacenc_hip_stereo_frame_bytes_bound.argtypes = [C.c_uint32, C.c_uint32]
    L.flacenc_hip_stereo_frame_bytes_bound.restype = C.c_size_t
    L.flacenc_hip_encode_frames.argtypes = [vp, C.POINTER(FrameConfig), i32p, C.c_size_t, C.c_uint32, C.c_uint32,
                                            C.c_size_t, C.c_uint32, vp, i32p, C.c_size_t, C.c_int]
    L.flacenc_hip_encode_frames.restype = C.c_int
    L.flacenc_hip_encode_frames_async.argtypes = L.flacenc_hip_encode_frames.argtypes[:-1] + [vp]
    L.flacenc_hip_encode_frames_async.restype = C.c_int
    L.flacenc_hip_frame_bytes_bound.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.flacenc_hip_frame_bytes_bound.restype = C.c_size_t
    L.flacenc_hip_pack_frames.argtypes = [vp, i32p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t, vp, i32p,
                                          C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_size_t,
                                          vp, C.c_int]
    L.flacenc_hip_pack_frames.restype = C.c_int
    L.flacenc_hip_pack_frames_async.argtypes = L.flacenc_hip_pack_frames.argtypes[:-1] + [vp]
    L.flacenc_hip_pack_frames_async.restype = C.c_int
    frame_args = [vp, C.POINTER(FrameConfig), i32p, C.c_size_t, C.c_uint32, C.c_size_t, C.c_uint32,
                  vp, i32p, C.c_size_t]
    L.flacenc_hip_encode_stereo_frames.argtypes = frame_args + [C.c_int]
    L.flacenc_hip_encode_stereo_frames.restype = C.c_int
    L.flacenc_hip_encode_stereo_frames_async.argtypes = frame_args + [vp]
    L.flacenc_hip_encode_stereo_frames_async.restype = C.c_int
    L.flacenc_hip_decode_frames_async.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                                  C.c_size_t, vp, vp, vp, vp]
    L.flacenc_hip_decode_frames_async.restype = C.c_int
    L.flacenc_hip_decode_frames.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32,
                                            vp, C.c_size_t, vp, vp, vp, C.c_int]
    L.flacenc_hip_decode_frames.restype = C.c_int
    L.flacenc_hip_verify_frames_async.argtypes = [vp, vp, vp, vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                                  C.c_size_t, vp, vp]
    L.flacenc_hip_verify_frames_async.restype = C.c_int
    L.flacenc_hip_index_frames_async.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_size_t, vp, vp, vp,
                                                 vp]
    L.flacenc_hip_index_frames_async.restype = C.c_int
    pack_le_args = [vp, vp, C.c_size_t, vp, C.c_size_t, C.c_uint32, C.c_uint32, vp, C.c_uint64, vp, vp]
    L.flacenc_hip_pack_le_bytes.argtypes = pack_le_args + [C.c_int]
    L.flacenc_hip_pack_le_bytes.restype = C.c_int
    L.flacenc_hip_decode_pcm.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, vp,
                                         C.c_uint64, vp]
    L.flacenc_hip_decode_pcm.restype = C.c_int
    L.flacenc_hip_decode_streams.argtypes = [vp, vp, C.c_uint64, vp, C.c_size_t, C.c_size_t, vp, C.c_uint64, vp, vp,
                                             C.c_int]
    L.flacenc_hip_decode_streams.restype = C.c_int
    L.flacenc_hip_md5_spans.argtypes = [vp, vp, C.c_uint64, vp, vp, C.c_size_t, vp, C.c_int]
    L.flacenc_hip_md5_spans.restype = C.c_int
    L.flacenc_hip_decode_streams_md5.argtypes = L.flacenc_hip_decode_streams.argtypes + [vp]
    L.flacenc_hip_decode_streams_md5.restype = C.c_int
    L.flacenc_hip_recover_streams.argtypes = [vp, vp, C.c_uint64, vp, C.c_size_t, vp, C.c_size_t, vp, C.c_uint64, vp, vp,
                                              C.c_size_t, vp, C.c_int]
    L.flacenc_hip_recover_streams.restype = C.c_int
    L.flacenc_hip_decode_ranges.argtypes = [vp, vp, C.c_uint64, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp,
                                            C.c_uint64, vp, vp, C.c_int]
    L.flacenc_hip_decode_ranges.restype = C.c_int
    L.flacenc_hip_decode_ranges_planar.argtypes = [vp, vp, C.c_uint64, vp, C.c_size_t, vp, C.c_size_t, C.c_size_t, vp,
                                                   C.c_uint64, C.c_uint32, vp, vp, C.c_int]
    L.flacenc_hip_decode_ranges_planar.restype = C.c_int
    L.flacenc_hip_encode_streams_frames.argtypes = [vp, C.c_size_t, C.c_uint32]
    L.flacenc_hip_encode_streams_frames.restype = C.c_size_t
    L.flacenc_hip_encode_streams.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_uint64, vp, C.c_size_t, C.c_uint32, vp,
                                             C.c_uint64, vp, C.c_size_t, vp, vp, C.c_int]
    L.flacenc_hip_encode_streams.restype = C.c_int
    L.flacenc_hip_encode_streams_planar.argtypes = [vp, C.POINTER(FrameConfig), vp, C.c_uint64, C.c_uint32, C.c_uint64, vp,
                                                    C.c_size_t, C.c_uint32, vp, C.c_uint64, vp, C.c_size_t, vp, vp, vp, vp,
                                                    C.c_int]
    L.flacenc_hip_encode_streams_planar.restype = C.c_int
    L.flacenc_hip_variable_bytes_bound.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64]
    L.flacenc_hip_variable_bytes_bound.restype = C.c_size_t
    L.flacenc_hip_variable_max_frames.argtypes = [C.c_uint32, C.c_uint32, C.c_uint64]
    L.flacenc_hip_variable_max_frames.restype = C.c_size_t
    variable_args = [vp, C.POINTER(FrameConfig), vp, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t,
                     C.c_uint32, C.c_uint32, C.c_uint64, vp, C.c_size_t, vp, vp, vp, C.c_size_t, vp, vp]
    L.flacenc_hip_encode_variable_async.argtypes = variable_args + [vp]
    L.flacenc_hip_encode_variable_async.restype = C.c_int
    L.flacenc_hip_encode_variable.argtypes = variable_args + [C.c_int]
    L.flacenc_hip_encode_variable.restype = C.c_int
    L.flacenc_hip_comm_unique_id.argtypes = [vp]
    L.flacenc_hip_comm_unique_id.restype = C.c_int
    L.flacenc_hip_comm_create.argtypes = [vp, vp, C.c_int, C.c_int]
    L.flacenc_hip_comm_create.restype = C.c_int
    L.flacenc_hip_comm_destroy.argtypes = [vp]
    L.flacenc_hip_comm_destroy.restype = C.c_int
    L.flacenc_hip_comm_info.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.flacenc_hip_comm_info.restype = C.c_int
    L.flacenc_hip_allgather_async.argtypes = [vp, vp, vp, C.c_size_t, vp]
    L.flacenc_hip_allgather_async.restype = C.c_int
    L.flacenc_hip_allgather_records_async.argtypes = [vp, vp, C.c_size_t, C.c_size_t, C.c_size_t, vp, vp]
    L.flacenc_hip_allgather_records_async.restype = C.c_int
    L.flacenc_sigen_fill_frames.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t,
                                            C.c_uint32, C.c_float, C.c_float, C.c_float,
                                            C.c_uint64, C.c_uint64, C.c_int]
    L.flacenc_sigen_fill_frames.restype = C.c_int
    L.flacenc_sigen_fill_frames_strided.argtypes = [vp, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t,
                                                    C.c_uint32, C.c_float, C.c_float, C.c_float,
                                                    C.c_uint64, C.c_uint64, C.c_uint64, C.c_int]
    L.flacenc_sigen_fill_frames_strided.restype = C.c_int
    _libs[LIB_PATH] = L
    return L


FLAG_FINEST_RICE_ORDER = 2
FLAG_GENERIC_KERNEL = 4
FLAG_FUSED_PACK = 8
FLAG_TWO_STAGE_PACK = 16
FLAG_REFERENCE_SUM_ORDER = 32
FLAG_NIGHTLY_SUM_ORDER = 64
FLAG_CANONICAL_SUM_ORDER = 128  # the kernels' own order without the order certificate
FLAG_INTEGER_PARITY_ONLY = 256  # with FLAG_REFERENCE_SUM_ORDER: certified shapes keep their own order (integers only)
FLAG_WASTED_BITS = 512  # frame-level calls code subframes whose low bits are all zero as x >> k at w - k bits
FLAG_ORDER_SEARCH = 1024  # every LPC candidate's order chosen by an exhaustive search over 1..lpc_order
FLAG_WINDOW_SEARCH = 2048  # every LPC candidate analysed under the config's window and the handle's extra windows
FLAG_ORDER_GUESS = 4096  # the LPC order guessed from the Levinson error: (0, P) and K guesses per window are coded
FLAG_PRECISION_SEARCH = 8192  # every LPC candidate coded at each precision quant_precision .. the handle's floor
FLAG_RICE_ESCAPE = 16384  # Rice partitions may be stored escaped (raw, rice_params[q] = 0x80 | width): the general path
DEFAULT_PRECISION_FLOOR = 5  # a fresh handle's floor (flacenc_hip_set_precision_floor)


def wasted_bits(results) -> np.ndarray:
    """Wasted bits k per output channel (FLAG_WASTED_BITS): the `pad` field of the result records, [n, 2] for
    FRAME_RESULT_DTYPE (output channel c) and [n] for CHANNEL_RESULT_DTYPE (pad[0]); 0 wherever the flag found none."""
    pad = np.asarray(results)["pad"]
    return pad.copy() if results.dtype == FRAME_RESULT_DTYPE else pad[..., 0].copy()


def make_config(lpc_order=10, quant_precision=15, window=("tukey", 0.4), max_rice_parameter=30,
                flags=0, rice_finest_only=False, use_direct_mse=False, mae_optimization_steps=0) -> QlpcConfig:
    """Defaults of config::Qlpc / config::Prc (src/constant.rs:109-115, src/config.rs:216-221)."""
    if window == "rectangle" or window[0] == "rectangle":
        wt, alpha = WINDOW_RECTANGLE, 0.0
    else:
        wt, alpha = WINDOW_TUKEY, float(window[1])
    if lpc_order > 24:
        flags |= FLAG_ALLOW_ORDER_32
    if rice_finest_only:  # build extension: BASELINE config 2's "fixed Rice partition order"
        flags |= FLAG_FINEST_RICE_ORDER
    return QlpcConfig(lpc_order, quant_precision, wt, alpha, max_rice_parameter, flags, 1 if use_direct_mse else 0,
                      int(mae_optimization_steps))


def verify_config(cfg: QlpcConfig) -> int:
    return int(load().flacenc_hip_verify_config(C.byref(cfg)))


def window_weights(cfg: QlpcConfig, block_size: int) -> np.ndarray:
    out = np.empty(block_size, np.float32)
    rc = load().flacenc_hip_window_weights(C.byref(cfg), block_size, out.ctypes.data)
    if rc != OK:
        raise FlacencHipError(rc)
    return out


def lpc_window_weights(window_type: int, alpha: float, start: int, end: int, block_size: int) -> np.ndarray:
    """flacenc_hip_lpc_window_weights: one extra-window entry's weights over a block (host only, no GPU)."""
    out = np.empty(max(block_size, 1), np.float32)
    rc = load().flacenc_hip_lpc_window_weights(window_type, alpha, start, end, block_size, out.ctypes.data)
    if rc != OK:
        raise FlacencHipError(rc, "flacenc_hip_lpc_window_weights")
    return out[:block_size]


def _window_arrays(entries):
    """(type, alpha, start, end) entries -> the four parallel arrays flacenc_hip_set_lpc_windows takes."""
    entries = list(entries)
    return (np.array([e[0] for e in entries], np.uint32), np.array([e[1] for e in entries], np.float32),
            np.array([e[2] for e in entries], np.uint32), np.array([e[3] for e in entries], np.uint32))


def sigen_frames(n_frames: int, channels: int, block_size: int, bits_per_sample: int,
                 sine_period: float, sine_amplitude: float, noise_amplitude: float, seed: int,
                 first_frame: int = 0, nthreads: int | None = None, frame_step: int = 1) -> np.ndarray:
    """flacenc_sigen_fill_frames[_strided] -> int32 [n_frames, channels, block_size] (FrameBuf layout).

    Local frame f is stream frame first_frame + f*frame_step."""
    out = np.empty((n_frames, channels, block_size), np.int32)
    if nthreads is None:
        nthreads = min(16, os.cpu_count() or 1)
    rc = load().flacenc_sigen_fill_frames_strided(out.ctypes.data, n_frames, channels, block_size,
                                                  block_size, bits_per_sample, sine_period,
                                                  sine_amplitude, noise_amplitude, seed, first_frame,
                                                  frame_step, nthreads)
    if rc != 0:
        raise FlacencHipError(rc, "flacenc_sigen_fill_frames")
    return out


def pinned_array(nbytes: int) -> np.ndarray:
    """uint8 array in page-locked host memory (flacenc_hip_host_alloc).  The allocation lives exactly as long
    as the array and its views: the ctypes buffer the array is built on is their common base object, and a
    finalizer on that buffer hands the memory back (flacenc_hip_host_free)."""
    import weakref
    lib = load()
    p = lib.flacenc_hip_host_alloc(nbytes)
    if not p:
        raise MemoryError("flacenc_hip_host_alloc")
    buf = (C.c_uint8 * nbytes).from_address(p)
    weakref.finalize(buf, lib.flacenc_hip_host_free, p)
    arr = np.frombuffer(buf, dtype=np.uint8)
    arr.flags.writeable = True
    return arr


def variable_bytes_bound(channels: int, block_size: int, levels: int, bits_per_sample: int, total_samples: int) -> int:
    """flacenc_hip_variable_bytes_bound: room for the frames of flacenc_hip_encode_variable (0: arguments rejected)."""
    return int(load().flacenc_hip_variable_bytes_bound(channels, block_size, levels, bits_per_sample, total_samples))


def variable_max_frames(block_size: int, levels: int, total_samples: int) -> int:
    """flacenc_hip_variable_max_frames: the most frames flacenc_hip_encode_variable can choose (0: rejected)."""
    return int(load().flacenc_hip_variable_max_frames(block_size, levels, total_samples))


class Handle:
    """RAII wrapper of flacenc_hip_handle (one per host thread / GPU)."""

    def __init__(self, device_id: int = 0, hooks: bool = False):
        """hooks=True: a handle of libflacenc_hip_hooks.so, the only one the debug_* methods below work on."""
        self._lib = load_hooks() if hooks else load()
        self._h = C.c_void_p()
        rc = self._lib.flacenc_hip_create(C.byref(self._h), device_id)
        if rc != OK:
            raise FlacencHipError(rc, "flacenc_hip_create failed (is a GPU visible?)")

    def close(self):
        if self._h:
            self._lib.flacenc_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _check(self, rc):
        if rc != OK:
            raise FlacencHipError(rc, self._lib.flacenc_hip_last_error(self._h).decode())

    def set_lpc_windows(self, entries):
        """flacenc_hip_set_lpc_windows: the extra analysis windows of FLAG_WINDOW_SEARCH, (type, alpha, start, end)
        each (DEFAULT_LPC_WINDOWS on a fresh handle; [] leaves the config's window only)."""
        t, a, s, e = _window_arrays(entries)
        n = len(t)
        ptr = (lambda x: x.ctypes.data) if n else (lambda x: None)
        self._check(self._lib.flacenc_hip_set_lpc_windows(self._h, ptr(t), ptr(a), ptr(s), ptr(e), n))

    def set_order_guesses(self, k: int):
        """flacenc_hip_set_order_guesses: K of FLAG_ORDER_GUESS, the guessed orders coded per window, 1..32 (a fresh
        handle holds 1); applies to the calls made after it."""
        self._check(self._lib.flacenc_hip_set_order_guesses(self._h, int(k)))

    def set_precision_floor(self, floor: int):
        """flacenc_hip_set_precision_floor: F of FLAG_PRECISION_SEARCH, the lowest coefficient precision searched,
        1..15 (a fresh handle holds 5); applies to the calls made after it."""
        self._check(self._lib.flacenc_hip_set_precision_floor(self._h, int(floor)))

    def set_max_bits_per_sample(self, bits: int):
        """flacenc_hip_set_max_bits_per_sample: the deepest FLAC stream the decode calls take, 24 (a fresh handle) or
        32; applies to the calls made after it.  The encode calls do not read it: set_max_encode_bits_per_sample is
        theirs."""
        self._check(self._lib.flacenc_hip_set_max_bits_per_sample(self._h, int(bits)))

    def set_max_encode_bits_per_sample(self, bits: int):
        """flacenc_hip_set_max_encode_bits_per_sample: the deepest PCM encode_pcm*, encode_streams and
        encode_streams_planar (SAMPLE_I32) take, 24 (a fresh handle) or 32; applies to the calls made after it.  More
        than 24 bits come in 4-byte samples and run the wide path (encode_pack_frames_wide_device)."""
        self._check(self._lib.flacenc_hip_set_max_encode_bits_per_sample(self._h, int(bits)))

    def _hook(self, name):
        if not hasattr(self._lib, name):
            raise RuntimeError(name + " is not in the product library: make the handle with Handle(dev, hooks=True)")
        return getattr(self._lib, name)

    def debug_scratch_bytes(self):
        """(total, largest) capacity in bytes of the device buffers the handle holds (flacenc_hip_debug.h)."""
        out = np.zeros(2, np.uint64)
        self._check(self._hook("flacenc_hip_debug_scratch_bytes")(self._h, out.ctypes.data))
        return int(out[0]), int(out[1])

    def debug_last_search_slices(self) -> int:
        """Slices of the last search-flag launch on the handle (flacenc_hip_debug.h); 0 before the first."""
        n = C.c_uint32(0)
        self._check(self._hook("flacenc_hip_debug_last_search_slices")(self._h, C.byref(n)))
        return n.value

    def debug_set_fixed_keys(self, device_ptr: int):
        self._check(self._hook("flacenc_hip_debug_set_fixed_keys")(self._h, device_ptr or None))

    def debug_set_order_guess_trace(self, device_ptr: int):
        """Calls under FLAG_ORDER_GUESS store every (subframe, window)'s guess as one ORDER_GUESS_TRACE_DTYPE record at
        [subframe of the call * W + window] of this device buffer, which the caller sizes (flacenc_hip_debug.h); 0
        switches it off."""
        self._check(self._hook("flacenc_hip_debug_set_order_guess_trace")(self._h, device_ptr or None))

    def debug_set_stamps(self, device_ptr: int):
        self._check(self._hook("flacenc_hip_debug_set_stamps")(self._h, device_ptr or None))

    def debug_set_cert_stats(self, device_ptr: int):
        """3 x uint32 on the device: subframes certified launches analysed, certificates that needed the rows of T^-1,
        subframes recomputed from the reference's chains (flacenc_hip_debug.h)."""
        self._check(self._hook("flacenc_hip_debug_set_cert_stats")(self._h, device_ptr or None))

    def debug_set_adaptive_order(self, on: bool):
        """Launches of the certified shapes that return integers only switch to the two-pass form on hard material
        (flacenc_hip_debug.h); off pins the fused kernel's certificate."""
        self._check(self._hook("flacenc_hip_debug_set_adaptive_order")(self._h, 1 if on else 0))

    def debug_adaptive_state(self):
        """(span, left) of the adaptive order mode: span 0 = the material last seen was easy."""
        span, left = C.c_int(0), C.c_int(0)
        self._check(self._hook("flacenc_hip_debug_adaptive_state")(self._h, C.byref(span), C.byref(left)))
        return span.value, left.value

    def debug_set_stream_chunk(self, frames: int):
        """encode_pcm* cuts its full blocks into chunks of `frames` frames in place of its rule (flacenc_hip_debug.h);
        0: the rule again.  More than 8192 is refused."""
        self._check(self._hook("flacenc_hip_debug_set_stream_chunk")(self._h, int(frames)))

    def debug_last_stream_plan(self):
        """(frames per chunk, chunks -- the short last block's included) of the last encode_pcm* call on this handle;
        (0, 0) when it ran none."""
        chunk, n = C.c_size_t(0), C.c_size_t(0)
        self._check(self._hook("flacenc_hip_debug_last_stream_plan")(self._h, C.byref(chunk), C.byref(n)))
        return chunk.value, n.value

    def debug_last_stream_buffers(self):
        """(pcm, out) of the last encode_pcm* call that reached its plan: True where the call found the buffer page-locked
        and transferred it directly, False where it staged it through the handle's pinned slots."""
        a, b = C.c_int(0), C.c_int(0)
        self._check(self._hook("flacenc_hip_debug_last_stream_buffers")(self._h, C.byref(a), C.byref(b)))
        return bool(a.value), bool(b.value)

    def debug_set_decode_plan(self, window_bytes: int = 0, group_frames: int = 0):
        """decode_pcm cuts its input into windows of `window_bytes` (raised to 2B by the call) and decodes groups of
        `group_frames` frames in place of its rules (flacenc_hip_debug.h); 0: the rule again."""
        self._check(self._hook("flacenc_hip_debug_set_decode_plan")(self._h, int(window_bytes), int(group_frames)))

    def debug_last_decode_plan(self):
        """(window bytes, windows indexed, frames per group, groups decoded) of the last decode_pcm call on this handle;
        zeros when it ran none."""
        v = [C.c_size_t(0) for _ in range(4)]
        self._check(self._hook("flacenc_hip_debug_last_decode_plan")(self._h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def debug_last_decode_streams_plan(self):
        """(kernel launches, host synchronisations, host-device transfers, channel counts present) of the last
        decode_streams call on this handle."""
        plan = np.zeros(4, np.uint64)
        self._check(self._hook("flacenc_hip_debug_last_decode_streams_plan")(self._h, plan.ctypes.data))
        return tuple(int(x) for x in plan)

    def debug_last_recover_plan(self):
        """(kernel launches, host synchronisations, host-device transfers, channel counts present) of the last
        recover_streams call on this handle."""
        plan = np.zeros(4, np.uint64)
        self._check(self._hook("flacenc_hip_debug_last_recover_plan")(self._h, plan.ctypes.data))
        return tuple(int(x) for x in plan)

    def debug_set_encode_streams_chunk(self, frames: int):
        """encode_streams cuts every run of a class into frame-level calls of at most `frames` frames in place of its
        rule (flacenc_hip_debug.h); 0: the rule again.  More than 8192 is refused."""
        self._check(self._hook("flacenc_hip_debug_set_encode_streams_chunk")(self._h, int(frames)))

    def debug_last_decode_ranges_plan(self):
        """[launches, synchronisations, transfers, channel counts among the ranges' streams] of the last decode_ranges
        call on this handle."""
        plan = np.zeros(4, np.uint64)
        self._check(self._hook("flacenc_hip_debug_last_decode_ranges_plan")(self._h, plan.ctypes.data))
        return [int(v) for v in plan]

    def debug_last_encode_streams_plan(self):
        """dict(launches, syncs, transfers, classes, full_runs, tail_runs, calls) of the last encode_streams call on
        this handle: launches are the call's own kernels, calls the frame-level calls (= full_runs + tail_runs)."""
        plan = np.zeros(8, np.uint64)
        self._check(self._hook("flacenc_hip_debug_last_encode_streams_plan")(self._h, plan.ctypes.data))
        names = ("launches", "syncs", "transfers", "classes", "full_runs", "tail_runs", "calls")
        return {k: int(v) for k, v in zip(names, plan)}

    def debug_last_encode_streams_planar_plan(self):
        """debug_last_encode_streams_plan after an encode_streams_planar call, with `digest_launches`: how many of
        `launches` the digests cost."""
        plan = np.zeros(8, np.uint64)
        self._check(self._hook("flacenc_hip_debug_last_encode_streams_plan")(self._h, plan.ctypes.data))
        names = ("launches", "syncs", "transfers", "classes", "full_runs", "tail_runs", "calls", "digest_launches")
        return {k: int(v) for k, v in zip(names, plan)}

    def debug_set_planar_fill_form(self, form: int):
        """How encode_streams_planar's fill kernel loads in the calls that follow: 1 aligned 16-byte loads brought into
        place (the product's form), 0 dword loads (flacenc_hip_debug.h).  The bytes do not depend on it."""
        self._check(self._hook("flacenc_hip_debug_set_planar_fill_form")(self._h, int(form)))

    def debug_streams_fill(self, bytes_ptr: int, total_samples: int, channels: int, bytes_per_sample: int, n_frames: int,
                           block_size: int, frames_ptr: int, stride: int, check: bool = True) -> int:
        """The fill kernel of encode_streams alone, on device pointers, with the arguments of fill_le_bytes
        (flacenc_hip_debug.h): rows 16-byte aligned, stride a multiple of 4, rows written up to the stride; blocks."""
        rc = self._hook("flacenc_hip_debug_streams_fill")(self._h, bytes_ptr or None, total_samples, channels,
                                                          bytes_per_sample, n_frames, block_size, frames_ptr or None,
                                                          stride)
        if check:
            self._check(rc)
        return rc

    def debug_segmax_scan(self, values, heads, room: int = None, check: bool = True):
        """The segmented max-scan of recover_streams alone (flacenc_hip_debug.h): values uint64 [n], heads [n] (non-zero:
        the element starts a segment; element 0 must), the launches sized by room >= n (default n).  -> uint64 [n], each
        element's maximum from its segment's head on; blocks.  check=False: -> (return code, the array)."""
        v = np.ascontiguousarray(values, np.uint64)
        hd = np.ascontiguousarray(np.asarray(heads) != 0, np.uint8)
        assert v.ndim == 1 and hd.shape == v.shape
        out = np.zeros(len(v), np.uint64)
        ptr = (lambda x: x.ctypes.data) if len(v) else (lambda x: None)
        rc = self._hook("flacenc_hip_debug_segmax_scan")(self._h, ptr(v), ptr(hd), len(v),
                                                         len(v) if room is None else int(room), ptr(out))
        if not check:
            return rc, out
        self._check(rc)
        return out

    def synchronize(self):
        self._check(self._lib.flacenc_hip_synchronize(self._h))

    def set_host_threads(self, threads: int):
        """Host threads sharing the staging copies of encode_pcm* for pageable buffers (default 4)."""
        self._check(self._lib.flacenc_hip_set_host_threads(self._h, threads))

    # -- host-memory path (what the reference's FFI would hand over) ----------
    def qlpc_batch(self, samples, bps, cfg: QlpcConfig, want_fp: bool = False):
        """estimated_qlpc over a [n_subframes, block_size] int32 host array.

        Returns (params record array, residual [n_subframes, block_size], R, a).
        """
        x = np.ascontiguousarray(samples, np.int32)
        ns, n = x.shape
        params = np.zeros(ns, PARAMS_DTYPE)
        residual = np.zeros((ns, n), np.int32)
        bps_a = np.ascontiguousarray(np.broadcast_to(np.asarray(bps, np.uint8), (ns,)))
        R = np.zeros((ns, 33), np.float64) if want_fp else None
        A = np.zeros((ns, 32), np.float64) if want_fp else None
        rc = self._lib.flacenc_hip_qlpc_batch(
            self._h, C.byref(cfg), x.ctypes.data, ns, n, n, bps_a.ctypes.data, params.ctypes.data,
            residual.ctypes.data, n, R.ctypes.data if want_fp else None,
            A.ctypes.data if want_fp else None, MEM_HOST)
        self._check(rc)
        return params, residual, R, A

    def stereo_qlpc_batch(self, frames, bits_per_sample: int, cfg: QlpcConfig):
        """The four estimated_qlpc calls of encode_frame per 2-channel frame (L, R, M, S).

        `frames` is int32 [n_frames, 2, block_size]; returns (params [n_frames, 4],
        residual [n_frames, 4, block_size]).
        """
        x = np.ascontiguousarray(frames, np.int32)
        nf, ch, n = x.shape
        assert ch == 2
        params = np.zeros((nf, 4), PARAMS_DTYPE)
        residual = np.zeros((nf, 4, n), np.int32)
        rc = self._lib.flacenc_hip_stereo_qlpc_batch(
            self._h, C.byref(cfg), x.ctypes.data, nf, n, n, bits_per_sample, params.ctypes.data,
            residual.ctypes.data, n, MEM_HOST)
        self._check(rc)
        return params, residual

    def stereo_qlpc_batch_device(self, cfg: QlpcConfig, frames_ptr: int, n_frames: int,
                                 block_size: int, stride: int, bits_per_sample: int, params_ptr: int,
                                 residual_ptr: int, residual_stride: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_stereo_qlpc_batch_async(
            self._h, C.byref(cfg), frames_ptr, n_frames, block_size, stride, bits_per_sample,
            params_ptr, residual_ptr, residual_stride, stream or None)
        self._check(rc)

    def fixed_lpc_batch(self, samples, bps, cfg: FrameConfig, stereo: bool = False):
        """fixed_lpc (src/coding.rs:298-331) for a batch of any block size.

        plain:  `samples` int32 [n_subframes, n], `bps` array or int -> params [n_subframes], residual
                [n_subframes, n], selector keys [n_subframes];
        stereo: `samples` int32 [n_frames, 2, n], `bps` int -> the same for L, R, M, S: [n_frames, 4, ...]."""
        x = np.ascontiguousarray(samples, np.int32)
        if stereo:
            nf, ch, n = x.shape
            assert ch == 2
            n_units, n_sub, shape = nf, nf * 4, (nf, 4)
            bps_arr, bps_uni = None, int(bps)
        else:
            n_units, n = x.shape
            n_sub, shape = n_units, (n_units,)
            if np.ndim(bps) == 0:
                bps_arr, bps_uni = None, int(bps)
            else:
                bps_arr, bps_uni = np.ascontiguousarray(bps, np.uint8), 16
        params = np.zeros(shape, PARAMS_DTYPE)
        residual = np.zeros(shape + (n,), np.int32)
        keys = np.zeros(shape, np.uint64)
        rc = self._lib.flacenc_hip_fixed_lpc_batch(
            self._h, C.byref(cfg), x.ctypes.data, n_units, n, n,
            bps_arr.ctypes.data if bps_arr is not None else None, bps_uni,
            LAYOUT_STEREO_FRAMES if stereo else LAYOUT_SUBFRAMES, params.ctypes.data, residual.ctypes.data, n,
            keys.ctypes.data, MEM_HOST)
        self._check(rc)
        return params, residual, keys

    def fixed_lpc_batch_device(self, cfg: FrameConfig, samples_ptr: int, n_units: int, block_size: int, stride: int,
                               bps_ptr: int | None, bits_per_sample: int, layout: int, params_ptr: int,
                               residual_ptr: int, residual_stride: int, selector_keys_ptr: int | None,
                               stream: int | None = None):
        """flacenc_hip_fixed_lpc_batch_async: device pointers (bps_ptr None: bits_per_sample for every subframe)."""
        rc = self._lib.flacenc_hip_fixed_lpc_batch_async(
            self._h, C.byref(cfg), samples_ptr, n_units, block_size, stride, bps_ptr or None, bits_per_sample, layout,
            params_ptr, residual_ptr, residual_stride, selector_keys_ptr or None, stream or None)
        self._check(rc)

    def pack_stereo_frames(self, frames, results, residual, bits_per_sample: int, sample_rate: int,
                           first_frame_number: int = 0, frame_number_step: int = 1):
        """Frame::write (src/component/bitrepr.rs:289-319) for the frames encode_stereo_frames decided:
        -> list of `bytes`, one FLAC frame each."""
        x = np.ascontiguousarray(frames, np.int32)
        nf, ch, n = x.shape
        res = np.ascontiguousarray(results)
        rs = np.ascontiguousarray(residual, np.int32)
        stride = int(self._lib.flacenc_hip_stereo_frame_bytes_bound(n, bits_per_sample))
        out = np.zeros((nf, stride), np.uint8)
        lens = np.zeros(nf, np.uint32)
        rc = self._lib.flacenc_hip_pack_stereo_frames(
            self._h, x.ctypes.data, nf, n, n, res.ctypes.data, rs.ctypes.data, n, bits_per_sample, sample_rate,
            first_frame_number, frame_number_step, out.ctypes.data, stride, lens.ctypes.data, MEM_HOST)
        self._check(rc)
        return [bytes(out[f, :lens[f]]) for f in range(nf)]

    def pack_stereo_frames_device(self, frames_ptr: int, n_frames: int, block_size: int, stride: int,
                                  results_ptr: int, residual_ptr: int, residual_stride: int, bits_per_sample: int,
                                  sample_rate: int, first_frame_number: int, frame_number_step: int, out_ptr: int,
                                  out_stride: int, out_len_ptr: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_pack_stereo_frames_async(
            self._h, frames_ptr, n_frames, block_size, stride, results_ptr, residual_ptr, residual_stride,
            bits_per_sample, sample_rate, first_frame_number, frame_number_step, out_ptr, out_stride, out_len_ptr,
            stream or None)
        self._check(rc)

    def stereo_frame_lengths_device(self, results_ptr: int, n_frames: int, block_size: int, bits_per_sample: int,
                                    sample_rate: int, first_frame_number: int, frame_number_step: int,
                                    out_len_ptr: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_stereo_frame_lengths_async(
            self._h, results_ptr, n_frames, block_size, bits_per_sample, sample_rate, first_frame_number,
            frame_number_step, out_len_ptr, stream or None)
        self._check(rc)

    def frame_wire_bytes(self, block_size: int) -> int:
        return int(self._lib.flacenc_hip_frame_wire_bytes(block_size))

    def stereo_frame_wire_device(self, results_ptr: int, n_frames: int, block_size: int, bits_per_sample: int,
                                 sample_rate: int, first_frame_number: int, frame_number_step: int, wire_ptr: int,
                                 wire_stride: int, out_len_ptr: int | None, stream: int | None = None):
        """Decision records -> wire records (+ the frames' byte lengths when out_len_ptr is given), one kernel."""
        rc = self._lib.flacenc_hip_stereo_frame_wire_async(
            self._h, results_ptr, n_frames, block_size, bits_per_sample, sample_rate, first_frame_number,
            frame_number_step, wire_ptr, wire_stride, out_len_ptr or None, stream or None)
        self._check(rc)

    def stream_offsets_device(self, gathered_lengths_ptr: int, n_frames_total: int, world: int, header_bytes: int,
                              lengths_stream_ptr: int | None, offsets_ptr: int, total_ptr: int,
                              stream: int | None = None):
        """All-gathered lengths (rank-major, uint32) -> stream-order lengths (uint32, optional), offsets and total
        (uint64), one kernel."""
        rc = self._lib.flacenc_hip_stream_offsets_async(self._h, gathered_lengths_ptr, n_frames_total, world,
                                                        header_bytes, lengths_stream_ptr or None, offsets_ptr,
                                                        total_ptr, stream or None)
        self._check(rc)

    def place_frames_device(self, src_ptr: int, src_offsets_ptr: int, lengths_ptr: int, n_frames: int, dst_ptr: int,
                            dst_offsets_ptr: int, stream: int | None = None):
        """ParSink's reordering on the GPU: frame i = lengths[i] bytes, src + src_offsets[i] -> dst + dst_offsets[i]
        (uint64 offsets, uint32 lengths, all device pointers)."""
        rc = self._lib.flacenc_hip_place_frames_async(self._h, src_ptr, src_offsets_ptr, lengths_ptr, n_frames,
                                                      dst_ptr, dst_offsets_ptr, stream or None)
        self._check(rc)

    def encode_pcm(self, pcm: np.ndarray, channels: int, cfg: FrameConfig, bytes_per_sample: int, bits_per_sample: int,
                   block_size: int, sample_rate: int, first_frame_number: int = 0, frame_number_step: int = 1,
                   out: np.ndarray | None = None, out_len: np.ndarray | None = None):
        """flacenc_hip_encode_pcm: interleaved LE PCM of 1..8 channels -> (frame bytes, lengths).  `pcm` / `out` may be
        pinned_array()s or views into one; `out` (uint8, its size is the capacity the call is told) and `out_len`
        (uint32, one entry per frame or more) are the caller's own buffers, and what comes back are views of them."""
        assert pcm.dtype == np.uint8 and pcm.flags["C_CONTIGUOUS"]
        total = pcm.size // (channels * bytes_per_sample)
        n_frames = (total + block_size - 1) // block_size
        if out is None:
            bound = int(self._lib.flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample))
            out = np.empty(n_frames * (bound + 16), np.uint8)
        lens = self._own_lengths(out_len, n_frames)
        written = C.c_uint64(0)
        rc = self._lib.flacenc_hip_encode_pcm(self._h, C.byref(cfg), pcm.ctypes.data, total, channels, bytes_per_sample,
                                              bits_per_sample, block_size, sample_rate, first_frame_number,
                                              frame_number_step, out.ctypes.data, out.size, lens.ctypes.data,
                                              C.byref(written))
        self._check(rc)
        return out[: written.value], lens[:n_frames]

    @staticmethod
    def _own_lengths(out_len, n_frames):
        """The lengths' buffer of encode_pcm*: the caller's, checked, or a fresh one."""
        if out_len is None:
            return np.zeros(n_frames, np.uint32)
        assert out_len.dtype == np.uint32 and out_len.ndim == 1 and out_len.flags["C_CONTIGUOUS"]
        assert out_len.flags["WRITEABLE"] and out_len.size >= n_frames
        return out_len

    def encode_pcm_stereo(self, pcm: np.ndarray, cfg: FrameConfig, bytes_per_sample: int, bits_per_sample: int,
                          block_size: int, sample_rate: int, out: np.ndarray | None = None,
                          first_frame_number: int = 0, frame_number_step: int = 1, out_len: np.ndarray | None = None):
        """Packed interleaved LE stereo PCM (uint8 array) -> (frame bytes uint8 [total], lengths uint32 [n_frames]),
        the streaming host path (flacenc_hip_encode_pcm_stereo).  `pcm` / `out` may be pinned_array()s; `out_len` as
        in encode_pcm."""
        assert pcm.dtype == np.uint8 and pcm.flags["C_CONTIGUOUS"]
        total = pcm.size // (2 * bytes_per_sample)
        n_frames = (total + block_size - 1) // block_size
        if out is None:
            out = np.empty(n_frames * (self.frame_bytes_bound(block_size, bits_per_sample) + 16), np.uint8)
        lens = self._own_lengths(out_len, n_frames)
        written = C.c_uint64(0)
        rc = self._lib.flacenc_hip_encode_pcm_stereo(self._h, C.byref(cfg), pcm.ctypes.data, total, bytes_per_sample,
                                                     bits_per_sample, block_size, sample_rate, first_frame_number,
                                                     frame_number_step, out.ctypes.data, out.size, lens.ctypes.data,
                                                     C.byref(written))
        self._check(rc)
        return out[: written.value], lens[:n_frames]

    def fill_le_bytes(self, data: bytes, channels: int, bytes_per_sample: int, block_size: int):
        """FrameBuf::fill_le_bytes for a whole stream: packed interleaved PCM -> int32 [n_frames, channels, n]."""
        b = np.frombuffer(bytes(data), np.uint8).copy()
        total = len(b) // (channels * bytes_per_sample)
        nf = (total + block_size - 1) // block_size
        out = np.full((nf, channels, block_size), -1, np.int32)
        rc = self._lib.flacenc_hip_fill_le_bytes(self._h, b.ctypes.data, total, channels, bytes_per_sample, nf,
                                                 block_size, out.ctypes.data, block_size, MEM_HOST)
        self._check(rc)
        return out

    def fill_le_bytes_device(self, bytes_ptr: int, total_samples: int, channels: int, bytes_per_sample: int,
                             n_frames: int, block_size: int, frames_ptr: int, stride: int, stream: int | None = None):
        """flacenc_hip_fill_le_bytes_async: packed interleaved PCM in HBM -> FrameBuf rows in HBM."""
        rc = self._lib.flacenc_hip_fill_le_bytes_async(self._h, bytes_ptr, total_samples, channels, bytes_per_sample,
                                                       n_frames, block_size, frames_ptr, stride, stream or None)
        self._check(rc)

    def encode_pack_stereo_frames_device(self, cfg: FrameConfig, frames_ptr: int, n_frames: int, block_size: int,
                                         stride: int, bits_per_sample: int, sample_rate: int,
                                         first_frame_number: int, frame_number_step: int, results_ptr: int,
                                         out_ptr: int, out_stride: int, out_len_ptr: int, stream: int | None = None):
        """PCM frames -> FLAC frame bytes on the device (one fused kernel for 4096-sample blocks)."""
        rc = self._lib.flacenc_hip_encode_pack_stereo_frames_async(
            self._h, C.byref(cfg), frames_ptr, n_frames, block_size, stride, bits_per_sample, sample_rate,
            first_frame_number, frame_number_step, results_ptr, out_ptr, out_stride, out_len_ptr, stream or None)
        self._check(rc)

    def encode_pack_frames_device(self, cfg: FrameConfig, frames_ptr: int, n_frames: int, channels: int,
                                  block_size: int, stride: int, bits_per_sample: int, sample_rate: int,
                                  first_frame_number: int, frame_number_step: int, results_ptr: int, out_ptr: int,
                                  out_stride: int, out_len_ptr: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_encode_pack_frames_async(
            self._h, C.byref(cfg), frames_ptr, n_frames, channels, block_size, stride, bits_per_sample, sample_rate,
            first_frame_number, frame_number_step, results_ptr, out_ptr, out_stride, out_len_ptr, stream or None)
        self._check(rc)

    def encode_pack_frames_wide_device(self, cfg: FrameConfig, frames_ptr: int, n_frames: int, channels: int,
                                       block_size: int, stride: int, bits_per_sample: int, sample_rate: int,
                                       first_frame_number: int, frame_number_step: int, out_ptr: int, out_stride: int,
                                       out_len_ptr: int):
        """flacenc_hip_encode_pack_frames_wide: rows of 8..32-bit samples -> FLAC frame bytes on the device, the wide
        path (Constant, Verbatim, fixed predictors; 2 channels take the stereo decision); blocks on the handle's
        stream."""
        rc = self._lib.flacenc_hip_encode_pack_frames_wide(
            self._h, C.byref(cfg), frames_ptr, n_frames, channels, block_size, stride, bits_per_sample, sample_rate,
            first_frame_number, frame_number_step, out_ptr, out_stride, out_len_ptr)
        self._check(rc)

    def encode_frames_wide(self, frames, bits_per_sample: int, cfg: FrameConfig, sample_rate: int = 44100,
                           first_frame_number: int = 0, frame_number_step: int = 1):
        """The wide path on a host array int32 [n_frames, channels, block_size] (staged through device tensors) ->
        the frames' bytes, one bytes object each."""
        import torch
        x = np.ascontiguousarray(frames, np.int32)
        n_frames, channels, n = x.shape
        bound = int(self._lib.flacenc_hip_stereo_frame_bytes_bound(n, bits_per_sample) if channels == 2 else
                    self._lib.flacenc_hip_frame_bytes_bound(channels, n, bits_per_sample))
        rows = self._device_copy(x)
        out = torch.full((n_frames, bound), 0xA5, dtype=torch.uint8, device="cuda")
        lens = torch.zeros(n_frames, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()  # the inputs are in place before the handle's stream reads them
        self.encode_pack_frames_wide_device(cfg, rows.data_ptr(), n_frames, channels, n, n, bits_per_sample, sample_rate,
                                            first_frame_number, frame_number_step, out.data_ptr(), bound, lens.data_ptr())
        got, lengths = out.cpu().numpy(), lens.cpu().numpy()
        return [got[f, : int(lengths[f])].tobytes() for f in range(n_frames)]

    def frame_bytes_bound(self, block_size: int, bits_per_sample: int) -> int:
        return int(self._lib.flacenc_hip_stereo_frame_bytes_bound(block_size, bits_per_sample))

    # -- the way back: decode, verify and index frames --------------------------------------------------------
    def decode_frames(self, data, offsets, lengths, channels: int, bits_per_sample: int, max_block_size: int):
        """flacenc_hip_decode_frames on host arrays: frame f = lengths[f] bytes at data[offsets[f]:] ->
        (samples int32 [n, channels, max_block_size], block_sizes uint32, numbers uint64, status uint32)."""
        buf = np.ascontiguousarray(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data,
                                   np.uint8)
        off = np.ascontiguousarray(offsets, np.uint64)
        ln = np.ascontiguousarray(lengths, np.uint32)
        n = len(off)
        out = np.empty((n, channels, max_block_size), np.int32)
        bs = np.zeros(n, np.uint32)
        num = np.zeros(n, np.uint64)
        st = np.zeros(n, np.uint32)
        rc = self._lib.flacenc_hip_decode_frames(self._h, buf.ctypes.data, buf.size, off.ctypes.data, ln.ctypes.data,
                                                 n, channels, bits_per_sample, max_block_size, out.ctypes.data,
                                                 max_block_size, bs.ctypes.data, num.ctypes.data, st.ctypes.data,
                                                 MEM_HOST)
        self._check(rc)
        return out, bs, num, st

    @staticmethod
    def _device_copy(arr):
        import torch
        return torch.from_numpy(np.array(arr, copy=True)).to("cuda")

    def verify_frames(self, data, offsets, lengths, channels: int, bits_per_sample: int, max_block_size: int,
                      expected):
        """flacenc_hip_verify_frames_async on host arrays (staged through device tensors): -> status uint32 [n]."""
        import torch
        buf = self._device_copy(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
        off = self._device_copy(np.asarray(offsets, np.uint64).view(np.int64))
        ln = self._device_copy(np.asarray(lengths, np.uint32).view(np.int32))
        exp = self._device_copy(np.asarray(expected, np.int32))
        n = len(offsets)
        st = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.verify_frames_device(buf.data_ptr(), off.data_ptr(), ln.data_ptr(), n, channels, bits_per_sample,
                                  max_block_size, exp.data_ptr(), exp.shape[-1], st.data_ptr(),
                                  torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return st.cpu().numpy().view(np.uint32)

    def index_frames(self, data, channels: int, bits_per_sample: int, max_frames: int):
        """flacenc_hip_index_frames_async on a host buffer of frames -> (offsets uint64, lengths uint32, ok).
        ok is False (FLACENC_HIP_INDEX_ERROR) when the chain from byte 0 does not end at the buffer's end, holds more than
        max_frames frames, or when the buffer holds more candidate headers than max_frames + max_frames // 4 + 4096 (a
        larger max_frames clears that); the frames returned are then a verified prefix of the chain."""
        import torch
        buf = self._device_copy(np.frombuffer(bytes(data), np.uint8) if not isinstance(data, np.ndarray) else data)
        off = torch.zeros(max(1, max_frames), dtype=torch.int64, device="cuda")
        ln = torch.zeros(max(1, max_frames), dtype=torch.int32, device="cuda")
        nf = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.index_frames_device(buf.data_ptr() if buf.numel() else 0, buf.numel(), channels, bits_per_sample,
                                 max_frames, off.data_ptr(), ln.data_ptr(), nf.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        raw = int(nf.cpu().numpy().view(np.uint64)[0])
        n = raw & (INDEX_ERROR - 1)
        return (off.cpu().numpy().view(np.uint64)[:n], ln.cpu().numpy().view(np.uint32)[:n],
                not (raw & INDEX_ERROR))

    def decode_frames_device(self, bytes_ptr: int, offsets_ptr: int, lengths_ptr: int, n_frames: int, channels: int,
                             bits_per_sample: int, max_block_size: int, out_ptr: int, stride: int,
                             block_sizes_ptr: int, numbers_ptr: int | None, status_ptr: int,
                             stream: int | None = None):
        rc = self._lib.flacenc_hip_decode_frames_async(self._h, bytes_ptr, offsets_ptr, lengths_ptr, n_frames, channels,
                                                       bits_per_sample, max_block_size, out_ptr, stride,
                                                       block_sizes_ptr, numbers_ptr or None, status_ptr,
                                                       stream or None)
        self._check(rc)

    def verify_frames_device(self, bytes_ptr: int, offsets_ptr: int, lengths_ptr: int, n_frames: int, channels: int,
                             bits_per_sample: int, max_block_size: int, expected_ptr: int, stride: int,
                             status_ptr: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_verify_frames_async(self._h, bytes_ptr, offsets_ptr, lengths_ptr, n_frames, channels,
                                                       bits_per_sample, max_block_size, expected_ptr, stride,
                                                       status_ptr, stream or None)
        self._check(rc)

    def index_frames_device(self, bytes_ptr: int, n_bytes: int, channels: int, bits_per_sample: int, max_frames: int,
                            offsets_ptr: int, lengths_ptr: int, n_frames_ptr: int, stream: int | None = None):
        rc = self._lib.flacenc_hip_index_frames_async(self._h, bytes_ptr or None, n_bytes, channels, bits_per_sample,
                                                      max_frames, offsets_ptr, lengths_ptr, n_frames_ptr,
                                                      stream or None)
        self._check(rc)

    def pack_le_bytes(self, frames, block_sizes, bytes_per_sample: int, out_capacity: int | None = None,
                      out: np.ndarray | None = None):
        """flacenc_hip_pack_le_bytes on host arrays: rows int32 [n_frames, channels, stride] + one block size per frame ->
        (packed interleaved little-endian PCM uint8, sample offsets uint64 [n_frames + 1], total samples, fits).  `out`
        (uint8; its size is the capacity unless out_capacity says less) defaults to exactly the room the block sizes need;
        fits is False (FLACENC_HIP_ERR_BAD_ARGUMENT from the call: nothing was written) when the output needs more."""
        x = np.ascontiguousarray(frames, np.int32)
        n, channels, stride = x.shape
        bs = np.ascontiguousarray(block_sizes, np.uint32)
        assert bs.shape == (n,)
        need = int(np.minimum(bs.astype(np.uint64), stride).sum()) * channels * bytes_per_sample
        if out is None:
            out = np.zeros(max(1, need if out_capacity is None else out_capacity), np.uint8)
        cap = (need if out.size >= need else out.size) if out_capacity is None else out_capacity
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and cap <= out.size
        off = np.zeros(n + 1, np.uint64)
        total = np.zeros(1, np.uint64)
        rc = self._lib.flacenc_hip_pack_le_bytes(self._h, x.ctypes.data if n else None, stride,
                                                 bs.ctypes.data if n else None, n, channels, bytes_per_sample,
                                                 out.ctypes.data, cap, off.ctypes.data, total.ctypes.data, MEM_HOST)
        fits = int(total[0]) * channels * bytes_per_sample <= cap
        if not (rc == ERR_BAD_ARGUMENT and not fits):
            self._check(rc)
        return out[: int(total[0]) * channels * bytes_per_sample if fits else 0], off, int(total[0]), fits

    def pack_le_bytes_device(self, frames_ptr: int, stride: int, block_sizes_ptr: int, n_frames: int, channels: int,
                             bytes_per_sample: int, out_ptr: int, out_capacity: int, sample_offsets_ptr: int | None,
                             total_ptr: int, check: bool = True) -> int:
        """flacenc_hip_pack_le_bytes on device pointers: decoded rows in HBM -> packed interleaved PCM in HBM, on the
        handle's stream; returns when the launches have run (work the caller queued on other streams must be complete).
        -> the call's code; with check=False a failure is returned instead of raised (ERR_BAD_ARGUMENT is also what an
        output that needs more than out_capacity gives: `total` and the offsets are then written, `out` is not)."""
        rc = self._lib.flacenc_hip_pack_le_bytes(self._h, frames_ptr or None, stride, block_sizes_ptr or None, n_frames,
                                                 channels, bytes_per_sample, out_ptr or None, out_capacity,
                                                 sample_offsets_ptr or None, total_ptr, MEM_DEVICE)
        if check:
            self._check(rc)
        return rc

    def decode_pcm(self, data, channels: int, bits_per_sample: int, max_block_size: int,
                   bytes_per_sample: int | None = None, out: np.ndarray | None = None, out_capacity: int | None = None):
        """flacenc_hip_decode_pcm: a buffer of frames (bytes, or a uint8 array -- a pinned_array() or a view into one is
        transferred directly) -> (packed interleaved little-endian PCM, a view of `out`; totals = [frames, samples, bytes
        consumed, stop reason]).  `out` (uint8; pinned or not) is the caller's buffer, its size the capacity unless
        out_capacity says less; without one the call gets room for len(data) // 9 + 1 frames of max_block_size, which
        always suffices but is only sensible for small inputs."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        width = bytes_per_sample or (bits_per_sample + 7) // 8
        if out is None:
            room = (buf.size // 9 + 1) * max_block_size * channels * width if out_capacity is None else out_capacity
            out = np.zeros(max(1, room), np.uint8)
        cap = out.size if out_capacity is None else out_capacity
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"] and cap <= out.size
        totals = np.zeros(4, np.uint64)
        rc = self._lib.flacenc_hip_decode_pcm(self._h, buf.ctypes.data if buf.size else None, buf.size, channels,
                                              bits_per_sample, max_block_size, width, out.ctypes.data, cap,
                                              totals.ctypes.data)
        self._check(rc)
        return out[: int(totals[1]) * channels * width], [int(t) for t in totals]

    def decode_streams(self, data, streams, max_frames: int, out: np.ndarray, totals: np.ndarray | None = None,
                       check: bool = True):
        """flacenc_hip_decode_streams on host arrays: `data` (bytes, or a uint8 array -- pinned or not) holds every
        stream's frames, `streams` is a STREAM_DESC_DTYPE array (or rows of its eight fields), `out` the caller's uint8
        buffer that holds every slot (written in place).  -> (totals uint64 [n_streams, 4], call totals [frames |
        INDEX_ERROR, samples], the call's code); with check=False a failure is returned instead of raised."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table = stream_descs(streams)
        if totals is None:
            totals = np.zeros((len(table), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(table)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_streams(self._h, buf.ctypes.data, buf.size, table.ctypes.data, len(table),
                                                  max_frames, out.ctypes.data, out.size, totals.ctypes.data,
                                                  call.ctypes.data, MEM_HOST)
        if check:
            self._check(rc)
        return totals, [int(call[0]), int(call[1])], rc

    def decode_streams_device(self, bytes_ptr: int, n_bytes: int, streams, max_frames: int, out_ptr: int,
                              out_bytes: int, totals_ptr: int, check: bool = True):
        """flacenc_hip_decode_streams on device pointers (the table stays host memory); blocks on the handle's stream.
        -> (call totals, the call's code)."""
        table = stream_descs(streams)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_streams(self._h, bytes_ptr or None, n_bytes, table.ctypes.data, len(table),
                                                  max_frames, out_ptr or None, out_bytes, totals_ptr or None,
                                                  call.ctypes.data, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    def recover_streams(self, data, streams, max_frames: int, out: np.ndarray, origins=None, max_gaps: int = 0,
                        gaps: np.ndarray | None = None, check: bool = True):
        """flacenc_hip_recover_streams on host arrays: decode_streams' `data`, `streams` and `out` (written in place),
        `origins` one sample number per stream (None: all zero), `gaps` a uint64 [max_gaps, 3] array (None: one is made
        when max_gaps > 0).  -> (out, totals uint64 [n_streams, 8], gaps -- the records written: min(call totals[2],
        max_gaps) rows of (stream, first sample, samples) --, call totals [frames | INDEX_ERROR, samples, gaps, frames
        dropped]); with check=False a failure's code is appended instead of raised."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table = stream_descs(streams)
        totals = np.zeros((len(table), 8), np.uint64)
        org = None if origins is None else np.ascontiguousarray(origins, np.uint64)
        assert org is None or org.size == len(table)
        if gaps is None and max_gaps:
            gaps = np.zeros((max_gaps, 3), np.uint64)
        assert gaps is None or (gaps.dtype == np.uint64 and gaps.flags["C_CONTIGUOUS"] and gaps.size >= 3 * max_gaps)
        call = np.zeros(4, np.uint64)
        rc = self._lib.flacenc_hip_recover_streams(self._h, buf.ctypes.data, buf.size, table.ctypes.data, len(table),
                                                   None if org is None else org.ctypes.data, max_frames,
                                                   out.ctypes.data, out.size, totals.ctypes.data,
                                                   None if gaps is None else gaps.ctypes.data, max_gaps,
                                                   call.ctypes.data, MEM_HOST)
        if check:
            self._check(rc)
        n = min(int(call[2]), max_gaps) if rc == 0 else 0
        written = np.zeros((0, 3), np.uint64) if gaps is None else gaps.reshape(-1, 3)[:n]
        result = (out, totals, written, [int(v) for v in call])
        return result if check else result + (rc,)

    def recover_streams_device(self, bytes_ptr: int, n_bytes: int, streams, max_frames: int, out_ptr: int,
                               out_bytes: int, totals_ptr: int, origins=None, gaps_ptr: int = 0, max_gaps: int = 0,
                               check: bool = True):
        """flacenc_hip_recover_streams on device pointers (the table and the origins stay host memory); blocks on the
        handle's stream.  -> (call totals, the call's code)."""
        table = stream_descs(streams)
        org = None if origins is None else np.ascontiguousarray(origins, np.uint64)
        call = np.zeros(4, np.uint64)
        rc = self._lib.flacenc_hip_recover_streams(self._h, bytes_ptr or None, n_bytes, table.ctypes.data, len(table),
                                                   None if org is None else org.ctypes.data, max_frames,
                                                   out_ptr or None, out_bytes, totals_ptr or None, gaps_ptr or None,
                                                   max_gaps, call.ctypes.data, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(v) for v in call], rc

    def decode_ranges(self, data, streams, ranges, max_frames: int, out: np.ndarray, totals: np.ndarray | None = None,
                      check: bool = True):
        """flacenc_hip_decode_ranges on host arrays: `data` and `streams` as for decode_streams (out_offset and
        out_capacity are ignored), `ranges` a RANGE_DESC_DTYPE array (or rows first_sample, n_samples, out_offset,
        stream), `out` the caller's uint8 buffer that holds every range's slot (written in place).  -> (totals uint64
        [n_ranges, 4] = samples written, stop reason, seek offset, seek position; call totals [frame decodes |
        INDEX_ERROR, samples]; the call's code); with check=False a failure is returned instead of raised."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table, rtable = stream_descs(streams), range_descs(ranges)
        if totals is None:
            totals = np.zeros((len(rtable), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(rtable)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_ranges(self._h, buf.ctypes.data, buf.size, table.ctypes.data, len(table),
                                                 rtable.ctypes.data, len(rtable), max_frames, out.ctypes.data, out.size,
                                                 totals.ctypes.data, call.ctypes.data, MEM_HOST)
        if check:
            self._check(rc)
        return totals, [int(call[0]), int(call[1])], rc

    def decode_ranges_device(self, bytes_ptr: int, n_bytes: int, streams, ranges, max_frames: int, out_ptr: int,
                             out_bytes: int, totals_ptr: int, check: bool = True):
        """flacenc_hip_decode_ranges on device pointers (both tables stay host memory); blocks on the handle's stream.
        -> (call totals, the call's code)."""
        table, rtable = stream_descs(streams), range_descs(ranges)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_ranges(self._h, bytes_ptr or None, n_bytes, table.ctypes.data, len(table),
                                                 rtable.ctypes.data, len(rtable), max_frames, out_ptr or None, out_bytes,
                                                 totals_ptr or None, call.ctypes.data, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    def decode_ranges_planar(self, data, streams, ranges, max_frames: int, out: np.ndarray, sample_format: int,
                             totals: np.ndarray | None = None, check: bool = True):
        """flacenc_hip_decode_ranges_planar on host arrays: the arguments of decode_ranges, `out` the caller's
        C-contiguous buffer of any dtype (uint8, int32, float32 ...) that holds every range's slot -- `channels` rows of
        n_samples 4-byte elements from out_offset (in bytes, a multiple of 4), samples behind the written ones zero --
        and `sample_format` SAMPLE_I32 or SAMPLE_F32.  -> (totals, call totals, the call's code) as for decode_ranges."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table, rtable = stream_descs(streams), range_descs(ranges)
        if totals is None:
            totals = np.zeros((len(rtable), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(rtable)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_ranges_planar(self._h, buf.ctypes.data, buf.size, table.ctypes.data, len(table),
                                                        rtable.ctypes.data, len(rtable), max_frames, out.ctypes.data,
                                                        out.nbytes, sample_format, totals.ctypes.data, call.ctypes.data,
                                                        MEM_HOST)
        if check:
            self._check(rc)
        return totals, [int(call[0]), int(call[1])], rc

    def decode_ranges_planar_device(self, bytes_ptr: int, n_bytes: int, streams, ranges, max_frames: int, out_ptr: int,
                                    out_bytes: int, sample_format: int, totals_ptr: int, check: bool = True):
        """flacenc_hip_decode_ranges_planar on device pointers (both tables stay host memory); blocks on the handle's
        stream.  -> (call totals, the call's code)."""
        table, rtable = stream_descs(streams), range_descs(ranges)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_ranges_planar(self._h, bytes_ptr or None, n_bytes, table.ctypes.data,
                                                        len(table), rtable.ctypes.data, len(rtable), max_frames,
                                                        out_ptr or None, out_bytes, sample_format, totals_ptr or None,
                                                        call.ctypes.data, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    @staticmethod
    def _span_table(offsets, lengths):
        """(offsets, lengths) as uint64 arrays of one size; never empty memory, so that their addresses are not NULL."""
        off = np.ascontiguousarray(offsets, np.uint64).reshape(-1)
        ln = np.ascontiguousarray(lengths, np.uint64).reshape(-1)
        assert off.shape == ln.shape
        if off.size == 0:
            return np.zeros(1, np.uint64)[:0], np.zeros(1, np.uint64)[:0]
        return off, ln

    def md5_spans(self, data, offsets, lengths, check: bool = True):
        """flacenc_hip_md5_spans on host arrays: `data` (bytes, or a uint8 array -- pinned or not), span i =
        data[offsets[i] : offsets[i] + lengths[i]] -> the digests, uint8 [n, 16] (hashlib.md5(span).digest() each); with
        check=False -> (digests, the call's code)."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        off, ln = self._span_table(offsets, lengths)
        digests = np.zeros((off.size, 16), np.uint8)
        base = buf if buf.size else np.zeros(1, np.uint8)
        rc = self._lib.flacenc_hip_md5_spans(self._h, base.ctypes.data, buf.size, off.ctypes.data, ln.ctypes.data,
                                             off.size, np.zeros(16, np.uint8).ctypes.data if off.size == 0
                                             else digests.ctypes.data, MEM_HOST)
        if check:
            self._check(rc)
            return digests
        return digests, rc

    def md5_spans_device(self, bytes_ptr: int, n_bytes: int, offsets, lengths, digests_ptr: int,
                         check: bool = True) -> int:
        """flacenc_hip_md5_spans on device pointers (the span table stays host memory): 16 bytes per span to
        digests_ptr; blocks on the handle's stream.  -> the call's code."""
        off, ln = self._span_table(offsets, lengths)
        rc = self._lib.flacenc_hip_md5_spans(self._h, bytes_ptr or None, n_bytes, off.ctypes.data, ln.ctypes.data,
                                             off.size, digests_ptr or None, MEM_DEVICE)
        if check:
            self._check(rc)
        return rc

    def decode_streams_md5(self, data, streams, max_frames: int, out: np.ndarray, totals: np.ndarray | None = None,
                           check: bool = True):
        """flacenc_hip_decode_streams_md5 on host arrays: decode_streams plus, per stream, the MD5 of the bytes the call
        wrote to its slot.  -> (totals, call totals, the call's code, digests uint8 [n_streams, 16])."""
        buf = data if isinstance(data, np.ndarray) else np.frombuffer(bytes(data), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table = stream_descs(streams)
        if totals is None:
            totals = np.zeros((len(table), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(table)
        call = np.zeros(2, np.uint64)
        digests = np.zeros((max(1, len(table)), 16), np.uint8)
        rc = self._lib.flacenc_hip_decode_streams_md5(self._h, buf.ctypes.data, buf.size, table.ctypes.data, len(table),
                                                      max_frames, out.ctypes.data, out.size, totals.ctypes.data,
                                                      call.ctypes.data, MEM_HOST, digests.ctypes.data)
        if check:
            self._check(rc)
        return totals, [int(call[0]), int(call[1])], rc, digests[:len(table)]

    def decode_streams_md5_device(self, bytes_ptr: int, n_bytes: int, streams, max_frames: int, out_ptr: int,
                                  out_bytes: int, totals_ptr: int, digests_ptr: int, check: bool = True):
        """flacenc_hip_decode_streams_md5 on device pointers (the table stays host memory): 16 digest bytes per stream to
        digests_ptr; blocks on the handle's stream.  -> (call totals, the call's code)."""
        table = stream_descs(streams)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_decode_streams_md5(self._h, bytes_ptr or None, n_bytes, table.ctypes.data, len(table),
                                                      max_frames, out_ptr or None, out_bytes, totals_ptr or None,
                                                      call.ctypes.data, MEM_DEVICE, digests_ptr or None)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    def encode_streams(self, pcm, streams, cfg: FrameConfig, block_size: int, out: np.ndarray,
                       frame_lengths: np.ndarray | None = None, totals: np.ndarray | None = None,
                       max_frames: int | None = None, check: bool = True):
        """flacenc_hip_encode_streams on host arrays: `pcm` (bytes, or a uint8 array -- pinned or not) holds every
        stream's packed PCM, `streams` is a PCM_STREAM_DESC_DTYPE array (or rows of its eight fields), `out` the caller's
        uint8 buffer that holds every slot (written in place).  -> (frame lengths uint32 [frames], totals uint64
        [n_streams, 4], call totals [frames, bytes], the call's code); with check=False a failure is returned instead of
        raised."""
        buf = pcm if isinstance(pcm, np.ndarray) else np.frombuffer(bytes(pcm), np.uint8)
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table = pcm_stream_descs(streams)
        n_frames = int(self._lib.flacenc_hip_encode_streams_frames(table.ctypes.data, len(table), block_size))
        if frame_lengths is None:
            frame_lengths = np.zeros(max(1, min(n_frames, 1 << 31)), np.uint32)
        assert frame_lengths.dtype == np.uint32 and frame_lengths.flags["C_CONTIGUOUS"]
        if totals is None:
            totals = np.zeros((max(1, len(table)), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(table)
        call = np.zeros(2, np.uint64)
        base = buf if buf.size else np.zeros(1, np.uint8)
        obase = out if out.size else np.zeros(1, np.uint8)
        rc = self._lib.flacenc_hip_encode_streams(self._h, C.byref(cfg), base.ctypes.data, buf.size, table.ctypes.data,
                                                  len(table), block_size, obase.ctypes.data, out.size,
                                                  frame_lengths.ctypes.data,
                                                  frame_lengths.size if max_frames is None else max_frames,
                                                  totals.ctypes.data, call.ctypes.data, MEM_HOST)
        if check:
            self._check(rc)
        return frame_lengths[:n_frames] if rc == OK else frame_lengths, totals[:len(table)], [int(call[0]), int(call[1])], rc

    def encode_streams_device(self, pcm_ptr: int, pcm_bytes: int, streams, cfg: FrameConfig, block_size: int,
                              out_ptr: int, out_bytes: int, frame_lengths_ptr: int, max_frames: int, totals_ptr: int,
                              check: bool = True):
        """flacenc_hip_encode_streams on device pointers (the table stays host memory); blocks on the handle's stream.
        -> (call totals, the call's code)."""
        table = pcm_stream_descs(streams)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_encode_streams(self._h, C.byref(cfg), pcm_ptr or None, pcm_bytes, table.ctypes.data,
                                                  len(table), block_size, out_ptr or None, out_bytes,
                                                  frame_lengths_ptr or None, max_frames, totals_ptr or None,
                                                  call.ctypes.data, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    def encode_streams_planar(self, samples: np.ndarray, sample_format: int, row_pitch: int, streams, cfg: FrameConfig,
                              block_size: int, out: np.ndarray, frame_lengths: np.ndarray | None = None,
                              totals: np.ndarray | None = None, max_frames: int | None = None, digests: bool = True,
                              clipped: bool = True, samples_bytes: int | None = None, check: bool = True):
        """flacenc_hip_encode_streams_planar on host arrays: `samples` is a C-contiguous array of 4-byte elements (int32
        for SAMPLE_I32, float32 for SAMPLE_F32; any shape: the table's offsets are bytes into it), `streams` the table of
        encode_streams, `out` the caller's uint8 buffer (written in place).  -> (frame lengths, totals, call totals,
        digests uint8 [n_streams, 16] or None, clipped uint64 [n_streams] or None, the call's code)."""
        assert samples.dtype.itemsize == 4 and samples.flags["C_CONTIGUOUS"]
        assert out.dtype == np.uint8 and out.flags["C_CONTIGUOUS"] and out.flags["WRITEABLE"]
        table = pcm_stream_descs(streams)
        n_frames = int(self._lib.flacenc_hip_encode_streams_frames(table.ctypes.data, len(table), block_size))
        if frame_lengths is None:
            frame_lengths = np.zeros(max(1, min(n_frames, 1 << 31)), np.uint32)
        assert frame_lengths.dtype == np.uint32 and frame_lengths.flags["C_CONTIGUOUS"]
        if totals is None:
            totals = np.zeros((max(1, len(table)), 4), np.uint64)
        assert totals.dtype == np.uint64 and totals.flags["C_CONTIGUOUS"] and totals.size >= 4 * len(table)
        call = np.zeros(2, np.uint64)
        dig = np.zeros((max(1, len(table)), 16), np.uint8) if digests else None
        clip = np.zeros(max(1, len(table)), np.uint64) if clipped else None
        base = samples if samples.size else np.zeros(1, np.int32)
        obase = out if out.size else np.zeros(1, np.uint8)
        rc = self._lib.flacenc_hip_encode_streams_planar(
            self._h, C.byref(cfg), base.ctypes.data, samples.nbytes if samples_bytes is None else samples_bytes,
            sample_format, row_pitch, table.ctypes.data, len(table), block_size, obase.ctypes.data, out.size,
            frame_lengths.ctypes.data, frame_lengths.size if max_frames is None else max_frames, totals.ctypes.data,
            call.ctypes.data, dig.ctypes.data if digests else None, clip.ctypes.data if clipped else None, MEM_HOST)
        if check:
            self._check(rc)
        return (frame_lengths[:n_frames] if rc == OK else frame_lengths, totals[:len(table)], [int(call[0]), int(call[1])],
                dig[:len(table)] if digests else None, clip[:len(table)] if clipped else None, rc)

    def encode_streams_planar_device(self, samples_ptr: int, samples_bytes: int, sample_format: int, row_pitch: int, streams,
                                     cfg: FrameConfig, block_size: int, out_ptr: int, out_bytes: int,
                                     frame_lengths_ptr: int, max_frames: int, totals_ptr: int, digests_ptr: int = 0,
                                     clipped_ptr: int = 0, check: bool = True):
        """flacenc_hip_encode_streams_planar on device pointers (the table stays host memory; digests_ptr / clipped_ptr 0:
        not asked for); blocks on the handle's stream.  -> (call totals, the call's code)."""
        table = pcm_stream_descs(streams)
        call = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_encode_streams_planar(
            self._h, C.byref(cfg), samples_ptr or None, samples_bytes, sample_format, row_pitch, table.ctypes.data,
            len(table), block_size, out_ptr or None, out_bytes, frame_lengths_ptr or None, max_frames, totals_ptr or None,
            call.ctypes.data, digests_ptr or None, clipped_ptr or None, MEM_DEVICE)
        if check:
            self._check(rc)
        return [int(call[0]), int(call[1])], rc

    # -- block-size search: variable-blocking streams ---------------------------------------------------------
    def encode_variable(self, frames, bits_per_sample: int, cfg: FrameConfig, levels: int, total_samples: int | None = None,
                        block_size: int | None = None, sample_rate: int = 44100, first_sample_number: int = 0,
                        out_capacity: int | None = None, max_frames: int | None = None):
        """flacenc_hip_encode_variable on host arrays.  frames: int32 [superblocks, channels, stride] in FrameBuf layout
        (zero beyond total_samples); block_size (the superblock S) defaults to the stride, total_samples to all rows.
        -> dict(data=bytes of the frames back to back, offsets, lengths, block_sizes, split_masks, frames=count,
        bytes=total, overflow=bool); on overflow data and the per-frame arrays are empty."""
        x = np.ascontiguousarray(frames, np.int32)
        n_sb, channels, stride = x.shape
        block_size = block_size or stride
        total = n_sb * block_size if total_samples is None else total_samples
        cap = variable_bytes_bound(channels, block_size, levels, bits_per_sample, total) if out_capacity is None \
            else out_capacity
        mf = variable_max_frames(block_size, levels, total) if max_frames is None else max_frames
        out = np.zeros(max(1, cap), np.uint8)
        off = np.zeros(max(1, mf), np.uint64)
        ln = np.zeros(max(1, mf), np.uint32)
        bs = np.zeros(max(1, mf), np.uint32)
        masks = np.zeros(max(1, n_sb), np.uint32)
        tot = np.zeros(2, np.uint64)
        rc = self._lib.flacenc_hip_encode_variable(self._h, C.byref(cfg), x.ctypes.data, total, channels, block_size,
                                                   levels, stride, bits_per_sample, sample_rate, first_sample_number,
                                                   out.ctypes.data, cap, off.ctypes.data, ln.ctypes.data, bs.ctypes.data,
                                                   mf, masks.ctypes.data, tot.ctypes.data, MEM_HOST)
        self._check(rc)
        raw = int(tot[0])
        n = raw & (VARIABLE_OVERFLOW - 1)
        overflow = bool(raw & VARIABLE_OVERFLOW)
        k = 0 if overflow else n
        return dict(data=out[:int(tot[1])].tobytes() if not overflow else b"", offsets=off[:k].copy(),
                    lengths=ln[:k].copy(), block_sizes=bs[:k].copy(), split_masks=masks[:n_sb].copy(), frames=n,
                    bytes=int(tot[1]), overflow=overflow)

    def encode_variable_device(self, cfg: FrameConfig, frames_ptr: int, total_samples: int, channels: int,
                               block_size: int, levels: int, stride: int, bits_per_sample: int, sample_rate: int,
                               first_sample_number: int, out_ptr: int, out_capacity: int, offsets_ptr: int,
                               lengths_ptr: int, block_sizes_ptr: int, max_frames: int, split_masks_ptr: int | None,
                               totals_ptr: int, stream: int | None = None):
        """flacenc_hip_encode_variable_async: device pointers, enqueued on `stream`."""
        rc = self._lib.flacenc_hip_encode_variable_async(
            self._h, C.byref(cfg), frames_ptr, total_samples, channels, block_size, levels, stride, bits_per_sample,
            sample_rate, first_sample_number, out_ptr or None, out_capacity, offsets_ptr or None, lengths_ptr or None,
            block_sizes_ptr or None, max_frames, split_masks_ptr or None, totals_ptr, stream or None)
        self._check(rc)

    # -- the ordered gather's collective (RCCL communicator owned by the handle) ----------
    @staticmethod
    def comm_unique_id() -> bytes:
        """ncclGetUniqueId: 128 bytes rank 0 hands to the other ranks."""
        buf = (C.c_uint8 * COMM_ID_BYTES)()
        rc = load().flacenc_hip_comm_unique_id(C.cast(buf, C.c_void_p))
        if rc != OK:
            raise FlacencHipError(rc, "flacenc_hip_comm_unique_id")
        return bytes(buf)

    def comm_create(self, unique_id: bytes, rank: int, world: int):
        assert len(unique_id) == COMM_ID_BYTES
        buf = (C.c_uint8 * COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._check(self._lib.flacenc_hip_comm_create(self._h, C.cast(buf, C.c_void_p), rank, world))

    def comm_destroy(self):
        self._check(self._lib.flacenc_hip_comm_destroy(self._h))

    def comm_info(self):
        r, w = C.c_int(0), C.c_int(0)
        self._check(self._lib.flacenc_hip_comm_info(self._h, C.byref(r), C.byref(w)))
        return r.value, w.value

    def allgather_device(self, send_ptr: int, recv_ptr: int, bytes_per_rank: int, stream: int | None = None):
        self._check(self._lib.flacenc_hip_allgather_async(self._h, send_ptr, recv_ptr, bytes_per_rank, stream or None))

    def allgather_records_device(self, local_ptr: int, n_local: int, n_total: int, record_bytes: int, gathered_ptr: int,
                                 stream: int | None = None):
        """The ordered gather's exchange: rank-major, short ranks zero-padded (all_gather_rank_major's layout)."""
        self._check(self._lib.flacenc_hip_allgather_records_async(self._h, local_ptr or None, n_local, n_total, record_bytes,
                                                                  gathered_ptr, stream or None))

    def frame_bytes_bound_channels(self, channels: int, block_size: int, bits_per_sample: int) -> int:
        return int(self._lib.flacenc_hip_frame_bytes_bound(channels, block_size, bits_per_sample))

    def encode_frames_device(self, cfg: FrameConfig, frames_ptr: int, n_frames: int, channels: int, block_size: int,
                             stride: int, bits_per_sample: int, results_ptr: int, residual_ptr: int,
                             residual_stride: int, stream: int | None = None):
        """flacenc_hip_encode_frames_async: Independent(channels) frames, device pointers."""
        rc = self._lib.flacenc_hip_encode_frames_async(
            self._h, C.byref(cfg), frames_ptr, n_frames, channels, block_size, stride, bits_per_sample, results_ptr,
            residual_ptr, residual_stride, stream or None)
        self._check(rc)

    def pack_frames_device(self, frames_ptr: int, n_frames: int, channels: int, block_size: int, stride: int,
                           results_ptr: int, residual_ptr: int, residual_stride: int, bits_per_sample: int,
                           sample_rate: int, first_frame_number: int, frame_number_step: int, out_ptr: int,
                           out_stride: int, out_len_ptr: int, stream: int | None = None):
        """flacenc_hip_pack_frames_async: Frame::write for the frames encode_frames_device decided."""
        rc = self._lib.flacenc_hip_pack_frames_async(
            self._h, frames_ptr, n_frames, channels, block_size, stride, results_ptr, residual_ptr, residual_stride,
            bits_per_sample, sample_rate, first_frame_number, frame_number_step, out_ptr, out_stride, out_len_ptr,
            stream or None)
        self._check(rc)

    def encode_frames(self, frames, bits_per_sample: int, cfg: FrameConfig):
        """encode_frame for Independent(channels) frames: `frames` int32 [n_frames, channels, n] ->
        (results CHANNEL_RESULT_DTYPE [n_frames, channels], residual [n_frames, channels, n])."""
        x = np.ascontiguousarray(frames, np.int32)
        nf, ch, n = x.shape
        results = np.zeros((nf, ch), CHANNEL_RESULT_DTYPE)
        residual = np.zeros((nf, ch, n), np.int32)
        rc = self._lib.flacenc_hip_encode_frames(self._h, C.byref(cfg), x.ctypes.data, nf, ch, n, n, bits_per_sample,
                                                 results.ctypes.data, residual.ctypes.data, n, MEM_HOST)
        self._check(rc)
        return results, residual

    def pack_frames(self, frames, results, residual, bits_per_sample: int, sample_rate: int,
                    first_frame_number: int = 0, frame_number_step: int = 1):
        """Frame::write for the frames encode_frames decided -> list of `bytes`."""
        x = np.ascontiguousarray(frames, np.int32)
        nf, ch, n = x.shape
        res = np.ascontiguousarray(results)
        rs = np.ascontiguousarray(residual, np.int32)
        stride = int(self._lib.flacenc_hip_frame_bytes_bound(ch, n, bits_per_sample))
        out = np.zeros((nf, stride), np.uint8)
        lens = np.zeros(nf, np.uint32)
        rc = self._lib.flacenc_hip_pack_frames(self._h, x.ctypes.data, nf, ch, n, n, res.ctypes.data, rs.ctypes.data, n,
                                               bits_per_sample, sample_rate, first_frame_number, frame_number_step,
                                               out.ctypes.data, stride, lens.ctypes.data, MEM_HOST)
        self._check(rc)
        return [bytes(out[f, :lens[f]]) for f in range(nf)]

    def encode_stereo_frames(self, frames, bits_per_sample: int, cfg: FrameConfig):
        """encode_frame with the decision on the GPU: `frames` int32 [n_frames, 2, block_size] ->
        (results FRAME_RESULT_DTYPE [n_frames], residual [n_frames, 2, block_size])."""
        x = np.ascontiguousarray(frames, np.int32)
        nf, ch, n = x.shape
        assert ch == 2
        results = np.zeros(nf, FRAME_RESULT_DTYPE)
        residual = np.zeros((nf, 2, n), np.int32)
        rc = self._lib.flacenc_hip_encode_stereo_frames(
            self._h, C.byref(cfg), x.ctypes.data, nf, n, n, bits_per_sample, results.ctypes.data,
            residual.ctypes.data, n, MEM_HOST)
        self._check(rc)
        return results, residual

    def encode_stereo_frames_device(self, cfg: FrameConfig, frames_ptr: int, n_frames: int,
                                    block_size: int, stride: int, bits_per_sample: int,
                                    results_ptr: int, residual_ptr: int, residual_stride: int,
                                    stream: int | None = None):
        rc = self._lib.flacenc_hip_encode_stereo_frames_async(
            self._h, C.byref(cfg), frames_ptr, n_frames, block_size, stride, bits_per_sample,
            results_ptr, residual_ptr, residual_stride, stream or None)
        self._check(rc)

    # -- device-memory path (raw pointers; torch tensors' data_ptr()) ---------
    def qlpc_batch_device(self, cfg: QlpcConfig, samples_ptr: int, n_subframes: int, block_size: int,
                          stride: int, bps_ptr: int, params_ptr: int, residual_ptr: int,
                          residual_stride: int, autocorr_ptr: int = 0, lpc_ptr: int = 0,
                          stream: int | None = None, sync: bool = False):
        if stream is None and sync:
            rc = self._lib.flacenc_hip_qlpc_batch(
                self._h, C.byref(cfg), samples_ptr, n_subframes, block_size, stride, bps_ptr or None,
                params_ptr, residual_ptr, residual_stride, autocorr_ptr or None, lpc_ptr or None,
                MEM_DEVICE)
        else:
            rc = self._lib.flacenc_hip_qlpc_batch_async(
                self._h, C.byref(cfg), samples_ptr, n_subframes, block_size, stride, bps_ptr or None,
                params_ptr, residual_ptr, residual_stride, autocorr_ptr or None, lpc_ptr or None,
                stream or None)
        self._check(rc)
