"""ctypes binding of include/adsbdec_amd.h.

This is plumbing for tests/ and bench.py: the product's host side is C
(csrc/cli/, adsbdec_amd_cli.c and the files beside it) and everything of substance lives behind the C-ABI.
There is no Python or CPU fallback: if the shared library is missing or no
gfx950 device is present, calls fail loudly.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ADSB_LIB_PATH") or os.path.join(PKG, "lib", "libadsbdec_amd.so")  # override: A/B runs
CLI_PATH = os.path.join(PKG, "lib", "adsbdec_amd_cli")


class AdsbError(RuntimeError):
    pass


class Frame(C.Structure):
    _fields_ = [("g", C.c_uint64), ("ts", C.c_uint64), ("pw", C.c_uint32), ("len", C.c_uint8),
                ("frame", C.c_uint8 * 14), ("reserved", C.c_uint8)]


class Candidate(C.Structure):
    _fields_ = [("g", C.c_uint64), ("pw", C.c_uint32), ("len", C.c_uint8),
                ("frame", C.c_uint8 * 14), ("reserved", C.c_uint8)]


class Stats(C.Structure):
    _fields_ = [("try_", C.c_uint64 * 3), ("ok", C.c_uint64 * 3), ("fixed", C.c_uint64)]


class ShardHead(C.Structure):
    _fields_ = [("g_begin", C.c_uint64), ("g_end", C.c_uint64), ("n_frames", C.c_uint64), ("n_head", C.c_uint64),
                ("head_end", C.c_uint64), ("skipped", C.c_uint64), ("status", C.c_uint64), ("n_bases", C.c_uint64),
                ("walk_final", C.c_uint64), ("has_tries", C.c_uint64), ("tries", C.c_uint64 * 3), ("ok", C.c_uint64 * 3),
                ("fixed", C.c_uint64)]


class ShardPart(C.Structure):
    _fields_ = [("head", C.POINTER(ShardHead)), ("frames", C.POINTER(Frame)), ("head_cands", C.POINTER(Candidate)),
                ("bases", C.POINTER(C.c_uint64)),
                ("head_tries", C.POINTER(C.c_uint64)), ("n_head_tries", C.c_uint64), ("head_tries_end", C.c_uint64),
                ("tail_tries", C.POINTER(C.c_uint64)), ("n_tail_tries", C.c_uint64), ("tail_from", C.c_uint64)]


class ShardFix(C.Structure):
    _fields_ = [("new_first", C.c_uint64), ("n_new", C.c_uint64), ("drop_front", C.c_uint64), ("keep", C.c_uint64),
                ("ts_sub", C.c_int64)]


class BatchSegment(C.Structure):
    """adsb_batch_segment (include/adsbdec_amd_diag.h): a capture's offsets [o_begin, o_end) at the virtual offsets from base on."""
    _fields_ = [("capture", C.c_uint64), ("o_begin", C.c_uint64), ("o_end", C.c_uint64), ("base", C.c_uint64),
                ("launch", C.c_uint32), ("first_tile", C.c_uint32), ("tiles", C.c_uint32), ("pad", C.c_uint32)]


class BatchLaunch(C.Structure):
    _fields_ = [("g_begin", C.c_uint64), ("g_end", C.c_uint64), ("seg_first", C.c_uint32), ("seg_end", C.c_uint32),
                ("tiles", C.c_uint32), ("passes", C.c_int32)]


class Config(C.Structure):
    """adsb_config, ABI 5 (include/adsbdec_amd.h)."""
    _fields_ = [("struct_size", C.c_uint32), ("abi", C.c_uint32), ("df18", C.c_int32), ("device", C.c_int32),
                ("collect_stats", C.c_int32), ("profile", C.c_int32), ("stage_samples", C.c_uint64), ("stream", C.c_void_p),
                ("all_candidates", C.c_int32), ("fix_1bit", C.c_int32), ("push_overlap", C.c_int32), ("host_threads", C.c_int32),
                ("wait_timeout_s", C.c_int32), ("warm_start", C.c_int32), ("debug", C.c_void_p)]


class DebugConfig(C.Structure):
    """adsb_debug_config (include/adsbdec_amd_diag.h): the test knobs behind adsb_config.debug."""
    _fields_ = [("struct_size", C.c_uint32), ("queue_cap", C.c_int32), ("cand_cap", C.c_int32), ("try_cap", C.c_int32),
                ("clist_cap", C.c_int32), ("no_streaming", C.c_int32), ("frames_cap", C.c_int32), ("reader_min_tiles", C.c_int32),
                ("shard_head", C.c_int32), ("passes", C.c_int32), ("big_tiles", C.c_int32), ("gang_min", C.c_int32),
                ("batch_launch_offsets", C.c_int32)]


class ConfigV4(C.Structure):
    """adsb_config as ABI 4 had it (rounds 4-5): only for same-box A/B runs against an older build of the library
    (ADSB_LIB_PATH); the tree's own library refuses it."""
    _fields_ = [("struct_size", C.c_uint32), ("df18", C.c_int32), ("device", C.c_int32),
                ("collect_stats", C.c_int32), ("profile", C.c_int32), ("debug_queue_cap", C.c_int32),
                ("stage_samples", C.c_uint64), ("stream", C.c_void_p), ("all_candidates", C.c_int32),
                ("fix_1bit", C.c_int32), ("debug_cand_cap", C.c_int32), ("debug_try_cap", C.c_int32),
                ("debug_clist_cap", C.c_int32), ("push_overlap", C.c_int32),
                ("host_threads", C.c_int32), ("debug_no_streaming", C.c_int32), ("debug_frames_cap", C.c_int32),
                ("debug_reader_min_tiles", C.c_int32), ("debug_shard_head", C.c_int32), ("debug_passes", C.c_int32),
                ("debug_stagger", C.c_int32), ("wait_timeout_s", C.c_int32), ("debug_gang_min", C.c_int32)]


class MultiInfo(C.Structure):
    _fields_ = [("shards", C.c_int32), ("fallback", C.c_int32), ("calls_walked", C.c_uint64), ("calls_jumped", C.c_uint64),
                ("create_ms", C.c_double), ("workers_ms", C.c_double), ("stitch_us", C.c_double), ("serial_us", C.c_double),
                ("total_ms", C.c_double), ("workers_bound", C.c_int32), ("helper_threads", C.c_int32)]


class WorkerPlacement(C.Structure):
    _fields_ = [("device", C.c_int32), ("device_node", C.c_int32), ("thread_bound", C.c_int32), ("slice_node", C.c_int32),
                ("local_fraction", C.c_double)]


class FormatReport(C.Structure):
    _fields_ = [("converted", C.c_uint64), ("inexact", C.c_uint64), ("clamped", C.c_uint64)]


class LevelReport(C.Structure):
    _fields_ = [("samples", C.c_uint64), ("negative", C.c_uint64), ("rail_lo", C.c_uint64), ("rail_hi", C.c_uint64), ("over", C.c_uint64),
                ("hist", C.c_uint64 * 2048)]


# fmt of the _as calls: the airspy_rx -t numbers (include/adsbdec_amd.h)
FMT_FLOAT32_REAL, FMT_INT16_REAL, FMT_UINT16_REAL, FMT_RAW = 1, 3, 4, 5
# fmt of the _iq calls (complex captures): arrays of shape (n, 2) = (I, Q), or flat ones of 2 n scalars
# (8 INT8_IQ is the library's own number, not an airspy_rx -t one: interleaved signed bytes, HackRF cs8 / bladeRF and USRP sc8)
FMT_FLOAT32_IQ, FMT_INT16_IQ, FMT_INT8_IQ = 0, 2, 8
IQ_DTYPES = {FMT_FLOAT32_IQ: np.dtype("<f4"), FMT_INT16_IQ: np.dtype("<i2"), FMT_INT8_IQ: np.dtype("i1")}
FMT_DTYPES = {FMT_FLOAT32_REAL: np.dtype("<f4"), FMT_INT16_REAL: np.dtype("<i2"), FMT_UINT16_REAL: np.dtype("<u2"), FMT_RAW: np.dtype("<u2")}


class TryFrame(C.Structure):
    """adsb_try_frame (include/adsbdec_amd_diag.h): an accepted frame as the try-count kernel reads it, 16 bytes."""
    _fields_ = [("g", C.c_uint64), ("span", C.c_uint32), ("pad", C.c_uint32)]


TRY_FRAME_DTYPE = np.dtype([("g", "<u8"), ("span", "<u4"), ("pad", "<u4")])   # the same record for numpy arrays
TRY_REGION = 4096                                                             # try words per tile region (csrc/scan_kernel.h kTryRegion)


class Profile(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("relaunches", C.c_uint64), ("offsets", C.c_uint64),
                ("kernel_ms", C.c_double), ("last_kernel_ms", C.c_double), ("last_offsets", C.c_uint64),
                ("candidates", C.c_uint64), ("tries", C.c_uint64), ("host_ms", C.c_double), ("wait_ms", C.c_double), ("big_offsets", C.c_uint64),
                ("big_launches", C.c_uint64), ("big_ms", C.c_double),
                ("host_threads_running", C.c_uint32), ("gang_launches", C.c_uint32), ("gang_batches", C.c_uint64)]


# every symbol include/adsbdec_amd.h and include/adsbdec_amd_diag.h declare: (restype, argtypes)
SYMBOLS = {
    "adsb_abi_version": (C.c_int, []),
    "adsb_config_default": (None, [C.c_void_p]),          # (the symbol binaries of ABI <= 4 call: leaves a struct adsb_create refuses)
    "adsb_config_init": (None, [C.c_void_p, C.c_size_t]),
    "adsb_create": (C.c_void_p, [C.c_void_p]),
    "adsb_destroy": (None, [C.c_void_p]),
    "adsb_reset": (C.c_int, [C.c_void_p]),
    "adsb_set_long_stream": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_get_wraps": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "adsb_set_flush": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_get_flush": (C.c_int, [C.c_void_p]),
    "adsb_resolver_finish_flush": (C.c_int, [C.c_void_p, C.c_uint64]),
    "adsb_batch_layout_flush": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(BatchSegment),
                                           C.c_size_t, C.POINTER(BatchLaunch), C.c_size_t, C.POINTER(C.c_size_t)]),
    "adsb_batch_resolve_flush": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_uint64, C.c_int, C.POINTER(Candidate),
                                            C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(Frame), C.c_size_t,
                                            C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_multi_set_long_streams": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_push": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_sync": (C.c_int, [C.c_void_p]),
    "adsb_device_cpulist": (C.c_int, [C.c_int, C.c_char_p, C.c_size_t]),
    "adsb_host_register": (C.c_int, [C.c_void_p, C.c_size_t]),
    "adsb_host_unregister": (C.c_int, [C.c_void_p]),
    "adsb_push_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_device_final": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_decode_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_decode_batch_device": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                            C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_decode_batch_host": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                          C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_batch_layout": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(BatchSegment), C.c_size_t,
                                     C.POINTER(BatchLaunch), C.c_size_t, C.POINTER(C.c_size_t)]),
    "adsb_batch_resolve": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.POINTER(Candidate), C.c_size_t,
                                      C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(Frame), C.c_size_t, C.POINTER(C.c_uint64),
                                      C.POINTER(Stats)]),
    "adsb_batch_layout_ex": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_uint64, C.POINTER(BatchSegment),
                                        C.c_size_t, C.POINTER(BatchLaunch), C.c_size_t, C.POINTER(C.c_size_t)]),
    "adsb_batch_resolve_ex": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_int, C.c_uint64, C.POINTER(Candidate),
                                         C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t, C.POINTER(Frame), C.c_size_t,
                                         C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_batch_records": (C.c_int, [C.c_void_p, C.POINTER(C.POINTER(Candidate)), C.POINTER(C.c_size_t),
                                     C.POINTER(C.POINTER(C.c_uint64)), C.POINTER(C.c_size_t), C.POINTER(C.POINTER(BatchSegment)),
                                     C.POINTER(C.c_size_t), C.POINTER(C.POINTER(BatchLaunch)), C.POINTER(C.c_size_t)]),
    "adsb_batch_unpacked_copy": (C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_push_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_packed_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_device_packed": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_device_packed_final": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_decode_device_packed": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_unpack_packed12": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_decode_batch_device_packed": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                   C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_decode_batch_host_packed": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                 C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_format_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "adsb_push_as": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_async_as": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_device_as": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_device_final_as": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_decode_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_decode_batch_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_decode_batch_host_as": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                             C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_iq_bytes": (C.c_size_t, [C.c_int, C.c_size_t]),
    "adsb_push_iq": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_iq_async": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_device_iq": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_push_device_iq_final": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]),
    "adsb_decode_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_decode_batch_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                               C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_decode_batch_host_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                             C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_push_power": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_power_async": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_device_power": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_push_device_power_final": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_decode_device_power": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_decode_batch_device_power": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                  C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_decode_batch_host_power": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t),
                                                C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_power_window": (C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t]),
    "adsb_power_window_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_void_p, C.c_size_t]),
    "adsb_power_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_power_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_power_device_packed": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_power_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]),
    "adsb_power_batch_device": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_power_batch_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_power_batch_device_packed": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_power_batch_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_power_batch_host": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_device_packed": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_device_power": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_batch_device": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_batch_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_batch_device_packed": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_batch_device_iq": (C.c_long, [C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_batch_device_power": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_level_batch_host": (C.c_long, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_debug_set_level_batch_blocks": (C.c_int, [C.c_void_p, C.c_int]),
    "adsb_level_windows": (C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_windows_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]),
    "adsb_level_add": (None, [C.c_void_p, C.c_void_p]),
    "adsb_level_percentile": (C.c_float, [C.c_void_p, C.c_double]),
    "adsb_bursts_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "adsb_bursts_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_size_t]),
    "adsb_bursts_slice_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_bursts_slice_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_float, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]),
    "adsb_burst_tile_runs": (C.c_uint32, []),
    "adsb_gather_layout": (C.c_long, [C.c_uint64, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]),
    "adsb_gather_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                      C.c_void_p]),
    "adsb_gather_chunk_words": (C.c_uint32, []),
    "adsb_gather_pack12_layout": (C.c_long, [C.c_uint64, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(C.c_uint64)]),
    "adsb_gather_pack12_device": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                             C.POINTER(C.c_uint64)]),
    "adsb_gather_pack12_device_as": (C.c_long, [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                C.c_void_p, C.POINTER(C.c_uint64)]),
    "adsb_gather_pack12_device_packed": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                                                    C.c_void_p, C.POINTER(C.c_uint64)]),
    "adsb_convert_iq_float32": (C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]),
    "adsb_get_format_report": (C.c_int, [C.c_void_p, C.POINTER(FormatReport)]),
    "adsb_convert_samples": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_size_t, C.c_void_p, C.c_void_p]),
    "adsb_count_tries_alone": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_uint32,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "adsb_multi_decode_batch_host": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.c_int,
                                                C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_multi_decode_batch_files": (C.c_long, [C.c_void_p, C.c_size_t, C.POINTER(C.c_char_p), C.c_int,
                                                 C.POINTER(C.POINTER(Frame)), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_multi_batch_plan": (C.c_long, [C.c_size_t, C.POINTER(C.c_size_t), C.c_int, C.c_uint64, C.c_int, C.POINTER(C.c_size_t),
                                         C.POINTER(C.c_size_t), C.c_size_t]),
    "adsb_multi_set_batch_bytes": (C.c_int, [C.c_void_p, C.c_uint64]),
    "adsb_finish": (C.c_int, [C.c_void_p]),
    "adsb_host_alloc": (C.c_void_p, [C.c_size_t]),
    "adsb_host_free": (None, [C.c_void_p]),
    "adsb_drain": (C.c_long, [C.c_void_p, C.POINTER(Frame), C.c_size_t]),
    "adsb_take": (C.c_long, [C.c_void_p, C.POINTER(C.POINTER(Frame))]),
    "adsb_pending": (C.c_size_t, [C.c_void_p]),
    "adsb_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "adsb_get_profile_sized": (C.c_int, [C.c_void_p, C.POINTER(Profile), C.c_size_t]),
    "adsb_last_error": (C.c_char_p, [C.c_void_p]),
    "adsb_format_frame": (C.c_int, [C.POINTER(Frame), C.c_int, C.c_char_p]),
    "adsb_resolver_create": (C.c_void_p, []),
    "adsb_resolver_destroy": (None, [C.c_void_p]),
    "adsb_resolver_set_threads": (C.c_int, [C.c_void_p, C.c_int, C.c_size_t]),
    "adsb_resolver_feed": (C.c_int, [C.c_void_p, C.POINTER(Candidate), C.c_size_t,
                                     C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_resolver_advance": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "adsb_resolver_drain": (C.c_long, [C.c_void_p, C.POINTER(Frame), C.c_size_t]),
    "adsb_resolver_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "adsb_handoff_walk": (C.c_long, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_uint32),
                                     C.POINTER(C.c_uint32), C.POINTER(C.c_int)]),
    "adsb_shard_layout_check": (C.c_int, [C.c_size_t, C.c_size_t]),
    "adsb_host_cpu_refusal": (C.c_char_p, []),
    "adsb_device_numa_node": (C.c_int, [C.c_int]),
    "adsb_host_alloc_on": (C.c_void_p, [C.c_size_t, C.c_int]),
    "adsb_host_alloc_sharded": (C.c_void_p, [C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_int)]),
    "adsb_host_placement": (C.c_int, [C.c_void_p, C.c_size_t, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_double)]),
    "adsb_host_release_mapped": (C.c_int, [C.c_void_p]),
    "adsb_multi_host_alloc": (C.c_void_p, [C.c_void_p, C.c_uint64]),
    "adsb_multi_worker_placement": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(WorkerPlacement)]),
    "adsb_resolver_advance_stream": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_uint64,
                                                C.c_uint64, C.c_uint64, C.c_int]),
    "adsb_handoff_finish": (C.c_long, [C.c_void_p, C.c_size_t, C.c_uint32, C.c_uint32, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64,
                                       C.c_uint32, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                                       C.POINTER(Candidate), C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "adsb_scan_shard_resolved": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64,
                                           C.POINTER(ShardHead), C.POINTER(Frame), C.c_size_t, C.POINTER(Candidate),
                                           C.c_size_t]),
    "adsb_scan_shard_resolved_walk": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64,
                                                C.POINTER(ShardHead), C.POINTER(Frame), C.c_size_t, C.POINTER(Candidate),
                                                C.c_size_t, C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_scan_shard_resolved_take": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64,
                                                C.POINTER(ShardHead), C.POINTER(C.POINTER(Frame)), C.POINTER(C.POINTER(Candidate)),
                                                C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_stitch_shards": (C.c_int, [C.POINTER(ShardPart), C.c_int, C.c_uint64, C.POINTER(ShardFix), C.POINTER(Frame),
                                     C.c_size_t, C.POINTER(C.c_size_t)]),
    "adsb_stitch_shards_ex": (C.c_int, [C.POINTER(ShardPart), C.c_int, C.c_uint64, C.POINTER(ShardFix), C.POINTER(Frame),
                                        C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64)]),
    "adsb_stitch_shards_stats": (C.c_int, [C.POINTER(ShardPart), C.c_int, C.c_uint64, C.POINTER(ShardFix), C.POINTER(Frame),
                                           C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.POINTER(Stats)]),
    "adsb_shard_begin": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_shard_end": (C.c_int, [C.c_void_p, C.POINTER(ShardHead), C.POINTER(C.POINTER(Frame)), C.POINTER(C.POINTER(Candidate))]),
    "adsb_shard_walk": (C.c_size_t, [C.POINTER(ShardHead), C.POINTER(Frame), C.c_uint64, C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_shard_apply_fix": (None, [C.POINTER(Frame), C.c_size_t, C.c_int64]),
    "adsb_resolver_start_chain": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
    "adsb_resolver_start_walk": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_uint64), C.c_size_t]),
    "adsb_resolver_walk_result": (C.c_size_t, [C.c_void_p, C.POINTER(C.c_int)]),
    "adsb_resolver_head": (C.c_long, [C.c_void_p, C.POINTER(Candidate), C.c_size_t]),
    "adsb_resolver_skipped": (C.c_uint64, [C.c_void_p]),
    "adsb_plan_shards": (C.c_int, [C.c_uint64, C.c_int, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                   C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "adsb_scan_shard_host": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64,
                                       C.c_uint64, C.POINTER(Candidate), C.c_size_t,
                                       C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.c_size_t,
                                       C.POINTER(C.c_size_t)]),
    "adsb_multi_create": (C.c_void_p, [C.c_void_p, C.c_int, C.POINTER(C.c_int)]),
    "adsb_multi_destroy": (None, [C.c_void_p]),
    "adsb_multi_devices": (C.c_int, [C.c_void_p]),
    "adsb_multi_decode_host": (C.c_long, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.POINTER(Frame))]),
    "adsb_multi_decode_file": (C.c_long, [C.c_void_p, C.c_char_p, C.POINTER(C.POINTER(Frame))]),
    "adsb_multi_decode_device": (C.c_long, [C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.POINTER(Frame))]),
    "adsb_multi_plan": (C.c_int, [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                  C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "adsb_multi_get_stats": (C.c_int, [C.c_void_p, C.POINTER(Stats)]),
    "adsb_multi_decode_streams_host": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t)]),
    "adsb_multi_decode_streams_file": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_char_p)]),
    "adsb_multi_stream_frames": (C.c_long, [C.c_void_p, C.c_int, C.POINTER(C.POINTER(Frame))]),
    "adsb_multi_stream_stats": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Stats)]),
    "adsb_multi_get_info": (C.c_int, [C.c_void_p, C.POINTER(MultiInfo)]),
    "adsb_multi_worker_profile_sized": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(Profile), C.c_size_t]),
    "adsb_multi_last_error": (C.c_char_p, [C.c_void_p]),
    "adsb_scan_shard": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64,
                                  C.c_uint64, C.POINTER(Candidate), C.c_size_t,
                                  C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.c_size_t,
                                  C.POINTER(C.c_size_t)]),
    "adsb_scan_wrap_window": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64,
                                        C.c_uint64, C.POINTER(Candidate), C.c_size_t,
                                        C.POINTER(C.c_size_t), C.POINTER(C.c_uint64), C.c_size_t,
                                        C.POINTER(C.c_size_t)]),
    "adsb_seam_power": (C.c_long, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_size_t, C.c_uint64, C.c_uint64, C.c_uint64,
                                   C.POINTER(C.c_float), C.c_size_t]),
}

_lib = None


def load():
    """dlopen the in-tree library and bind every declared symbol. Raises if absent.
    In a process that also uses PyTorch, import torch BEFORE calling this: torch ships its own
    libamdhip64, and two HIP runtimes in one process do not share the device (the second one
    reports "no ROCm-capable device")."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AdsbError(f"{LIB_PATH} is missing: run `python -m adsbdec_amd._build` "
                            "(there is no fallback implementation)")
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SYMBOLS.items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                if os.environ.get("ADSB_LIB_PATH"):  # an A/B run against an older build of the library: it has what it has
                    continue
                raise
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def _frames_to_dicts(arr, n):
    return [dict(g=int(f.g), ts=int(f.ts), pw=int(f.pw), frame=bytes(f.frame[: f.len])) for f in arr[:n]]


def _stats_to_dict(st: Stats, with_fixed: bool = False):
    d = {"try": {11: int(st.try_[0]), 17: int(st.try_[1]), 18: int(st.try_[2])},
         "ok": {11: int(st.ok[0]), 17: int(st.ok[1]), 18: int(st.ok[2])}}
    if with_fixed:
        d["fixed"] = int(st.fixed)
    return d


def format_frame(fr: dict, outformat: int) -> bytes:
    f = Frame()
    f.g, f.ts, f.pw, f.len = fr.get("g", 0), fr["ts"], fr["pw"], len(fr["frame"])
    for i, b in enumerate(fr["frame"]):
        f.frame[i] = b
    buf = C.create_string_buffer(256)
    n = load().adsb_format_frame(C.byref(f), outformat, buf)
    return buf.raw[:n]


DEBUG_KNOBS = ("queue_cap", "cand_cap", "try_cap", "clist_cap", "no_streaming", "frames_cap", "reader_min_tiles", "shard_head",
               "passes", "big_tiles", "gang_min", "batch_launch_offsets")


def make_config(df18: bool = False, device: int = -1, collect_stats: bool = False,
                profile: bool = False, stage_samples: int = 0, stream: int | None = None,
                all_candidates: bool = False, fix_1bit: bool = False, push_overlap: bool = False,
                host_threads: int = 0, wait_timeout_s: int = 0, warm_start: bool = False, **debug):
    """adsb_config from keywords (adsb_config_default + the members named).  Keywords debug_<knob> (DEBUG_KNOBS) fill an
    adsb_debug_config that the returned struct points at (and keeps alive: cfg._debug)."""
    L = load()
    unknown = [k for k in debug if not k.startswith("debug_") or k[6:] not in DEBUG_KNOBS]
    if unknown:
        raise TypeError(f"make_config: unknown keyword(s) {unknown}")
    if L.adsb_abi_version() < 5:   # an A/B run against a build of rounds 4-5 (ADSB_LIB_PATH): its struct, its member names
        cfg = ConfigV4()
        L.adsb_config_init(C.byref(cfg), C.sizeof(cfg))
        for k, v in debug.items():
            if hasattr(ConfigV4, k) and cfg.struct_size >= getattr(ConfigV4, k).offset + 4:
                setattr(cfg, k, int(v))
        if cfg.struct_size >= ConfigV4.wait_timeout_s.offset + 4:
            cfg.wait_timeout_s = wait_timeout_s
    else:
        cfg = Config()
        L.adsb_config_init(C.byref(cfg), C.sizeof(cfg))
        cfg.wait_timeout_s = wait_timeout_s
        cfg.warm_start = int(warm_start)
        if any(debug.values()):
            dbg = DebugConfig()
            dbg.struct_size = C.sizeof(dbg)
            for k, v in debug.items():
                setattr(dbg, k[6:], int(v))
            cfg._debug = dbg                      # (the library copies it in adsb_create; until then it must live)
            cfg.debug = C.addressof(dbg)
    cfg.df18 = int(df18)
    cfg.device = device
    cfg.collect_stats = int(collect_stats)
    cfg.profile = int(profile)
    cfg.stage_samples = stage_samples
    cfg.stream = stream
    cfg.all_candidates = int(all_candidates)
    cfg.fix_1bit = int(fix_1bit)
    cfg.push_overlap = int(push_overlap)
    cfg.host_threads = int(host_threads)
    return cfg


class Decoder:
    """One stream (== the statics of air.c / demod.c / valid.c).  Keywords: make_config."""

    def __init__(self, long_stream: bool = False, flush: bool = False, **cfg_kw):
        L = load()
        cfg = make_config(**cfg_kw)
        self._L = L
        self._fix = bool(cfg_kw.get("fix_1bit"))
        self._h = L.adsb_create(C.byref(cfg))
        if not self._h:
            raise AdsbError("adsb_create failed: " + (L.adsb_last_error(None) or b"").decode())
        if long_stream:
            self.set_long_stream(True)
        if flush:
            self.set_flush(True)
        self._out = C.POINTER(Frame)()          # decode_device_raw's result pointer and its reference, made once
        self._out_ref = C.byref(self._out)
        self._decode_device = L.adsb_decode_device

    def _check(self, rc, what):
        if rc != 0:
            raise AdsbError(f"{what} failed: " + (self._L.adsb_last_error(self._h) or b"").decode())

    def close(self):
        if self._h:
            self._L.adsb_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        self._check(self._L.adsb_reset(self._h), "adsb_reset")

    def set_long_stream(self, on: bool = True):
        """adsb_set_long_stream: streams of 2^32 samples and more (fresh or reset handle, before the first push)."""
        self._check(self._L.adsb_set_long_stream(self._h, int(bool(on))), "adsb_set_long_stream")

    def set_flush(self, on: bool = True):
        """adsb_set_flush: decode a capture to its last sample -- every decode call, batch call and finished stream of the handle
        then returns what the reference returns for the capture's silent twin (fresh or reset handle, before the first push;
        sticky across reset)."""
        self._check(self._L.adsb_set_flush(self._h, int(bool(on))), "adsb_set_flush")

    @property
    def flush(self) -> bool:
        """adsb_get_flush."""
        return self._L.adsb_get_flush(self._h) == 1

    def wraps(self):
        """(wraps of the reference's sample counter in the current stream, offsets that went through the seam kernel)."""
        w, s = C.c_uint64(0), C.c_uint64(0)
        self._check(self._L.adsb_get_wraps(self._h, C.byref(w), C.byref(s)), "adsb_get_wraps")
        return int(w.value), int(s.value)

    def push(self, x: np.ndarray):
        x = np.ascontiguousarray(x)
        assert x.dtype == np.uint16
        self._check(self._L.adsb_push(self._h, x.ctypes.data, x.size), "adsb_push")

    def push_async(self, x):
        """adsb_push_async: x (ndarray or (ptr, n)) stays borrowed until the next push/finish/sync returns."""
        if isinstance(x, tuple):
            ptr, n = x
        else:
            assert x.dtype == np.uint16 and x.flags["C_CONTIGUOUS"]
            ptr, n = x.ctypes.data, x.size
        self._check(self._L.adsb_push_async(self._h, ptr, n), "adsb_push_async")

    def sync(self):
        self._check(self._L.adsb_sync(self._h), "adsb_sync")

    def push_device(self, ptr: int, n: int):
        self._check(self._L.adsb_push_device(self._h, ptr, n), "adsb_push_device")

    def push_device_final(self, ptr: int, n: int):
        self._check(self._L.adsb_push_device_final(self._h, ptr, n), "adsb_push_device_final")

    def decode_device_raw(self, ptr: int, n: int):
        """adsb_decode_device: reset + push_device_final + take in one call -> (Frame pointer, count).  The pointer object is
        the decoder's own, reused by every call (a timed loop pays for the call, not for Python objects): what it points at
        is valid until the next call of this decoder, as adsb_take says."""
        k = self._decode_device(self._h, ptr, n, self._out_ref)
        if k < 0:
            self._check(-1, "adsb_decode_device")
        return self._out, k

    # ---- a batch of independent captures in as few launches as they fit (adsb_decode_batch_*)
    def decode_batch_device_raw(self, ptrs, ns):
        """adsb_decode_batch_device -> (Frame pointer, first: ctypes array of len(ns) + 1 indices, Stats array): capture i's
        frames are pointer[first[i] : first[i + 1]], valid until the next call of this decoder."""
        k = len(ns)
        p = (C.c_void_p * max(1, k))(*[int(v) if v else None for v in ptrs])
        n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        total = self._L.adsb_decode_batch_device(self._h, k, p, n, self._out_ref, first, st)
        if total < 0:
            self._check(-1, "adsb_decode_batch_device")
        return self._out, first, st

    def _batch_result(self, out, first, st, k, stats):
        frames = [_frames_to_dicts(out[int(first[i]):int(first[i + 1])], int(first[i + 1] - first[i])) for i in range(k)]
        return (frames, [_stats_to_dict(st[i], self._fix) for i in range(k)]) if stats else frames

    def decode_batch_device(self, ptrs, ns, stats: bool = False):
        """Captures resident in HBM (16-byte aligned pointers) -> a list of per-capture frame lists, each what decode_device
        gives for that capture alone; stats=True: (that, the per-capture Try/Ok tables)."""
        out, first, st = self.decode_batch_device_raw(ptrs, ns)
        return self._batch_result(out, first, st, len(ns), stats)

    def decode_batch(self, arrays, stats: bool = False):
        """The same for uint16 arrays in host memory (adsb_decode_batch_host copies them to scratch of the handle's)."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        assert all(a.dtype == np.uint16 for a in arrays)
        k = len(arrays)
        p = (C.c_void_p * max(1, k))(*[a.ctypes.data if a.size else None for a in arrays])
        n = (C.c_size_t * max(1, k))(*[a.size for a in arrays])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_host(self._h, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_host")
        return self._batch_result(self._out, first, st, k, stats)

    # ---- Airspy packed 12-bit input (include/adsbdec_amd.h): n always counts SAMPLES (a multiple of 8), 1.5 bytes each
    @staticmethod
    def _packed_arg(buf):
        if isinstance(buf, tuple):
            return buf
        assert buf.dtype == np.uint8 and buf.flags["C_CONTIGUOUS"] and buf.size % 12 == 0
        return buf.ctypes.data, buf.size // 12 * 8

    def push_packed(self, buf):
        """adsb_push_packed: buf = packed bytes (uint8 ndarray) or (ptr, n_samples)."""
        ptr, n = self._packed_arg(buf)
        self._check(self._L.adsb_push_packed(self._h, ptr, n), "adsb_push_packed")

    def push_packed_async(self, buf):
        """adsb_push_packed_async: buf stays borrowed until the next push/finish/sync returns."""
        ptr, n = self._packed_arg(buf)
        self._check(self._L.adsb_push_packed_async(self._h, ptr, n), "adsb_push_packed_async")

    def push_device_packed(self, ptr: int, n: int):
        self._check(self._L.adsb_push_device_packed(self._h, ptr, n), "adsb_push_device_packed")

    def push_device_packed_final(self, ptr: int, n: int):
        self._check(self._L.adsb_push_device_packed_final(self._h, ptr, n), "adsb_push_device_packed_final")

    def decode_device_packed_raw(self, ptr: int, n: int):
        """adsb_decode_device_packed -> (Frame pointer, count), as decode_device_raw."""
        k = self._L.adsb_decode_device_packed(self._h, ptr, n, self._out_ref)
        if k < 0:
            self._check(-1, "adsb_decode_device_packed")
        return self._out, k

    # ---- a batch of packed captures (adsb_decode_batch_*_packed): one unpack launch, then the batch scan
    def decode_batch_device_packed_raw(self, ptrs, ns):
        """adsb_decode_batch_device_packed (ns count samples) -> what decode_batch_device_raw gives."""
        k = len(ns)
        p = (C.c_void_p * max(1, k))(*[int(v) if v else None for v in ptrs])
        n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        total = self._L.adsb_decode_batch_device_packed(self._h, k, p, n, self._out_ref, first, st)
        if total < 0:
            self._check(-1, "adsb_decode_batch_device_packed")
        return self._out, first, st

    def decode_batch_device_packed(self, ptrs, ns, stats: bool = False):
        """Packed captures resident in HBM (4-byte aligned pointers, ns in samples) -> what decode_batch_device gives for their
        unpacked twins."""
        out, first, st = self.decode_batch_device_packed_raw(ptrs, ns)
        return self._batch_result(out, first, st, len(ns), stats)

    def decode_batch_packed(self, bufs, stats: bool = False):
        """The same for packed bytes (uint8 arrays of whole 12-byte groups) in host memory: adsb_decode_batch_host_packed."""
        bufs = [np.ascontiguousarray(b) for b in bufs]
        assert all(b.dtype == np.uint8 and b.size % 12 == 0 for b in bufs)
        k = len(bufs)
        p = (C.c_void_p * max(1, k))(*[b.ctypes.data if b.size else None for b in bufs])
        n = (C.c_size_t * max(1, k))(*[b.size // 12 * 8 for b in bufs])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_host_packed(self._h, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_host_packed")
        return self._batch_result(self._out, first, st, k, stats)

    def batch_records(self):
        """adsb_batch_records: what the last decode_batch* call collected -> (candidates as tuples (virtual g, pw, frame bytes,
        reserved), tries: uint64 (virtual g << 2 | code), segments, launches: lists of dicts as batch_layout gives them)."""
        cands, tries = C.POINTER(Candidate)(), C.POINTER(C.c_uint64)()
        segs, launches = C.POINTER(BatchSegment)(), C.POINTER(BatchLaunch)()
        nc, nt, ns, nl = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
        self._check(self._L.adsb_batch_records(self._h, C.byref(cands), C.byref(nc), C.byref(tries), C.byref(nt), C.byref(segs),
                                               C.byref(ns), C.byref(launches), C.byref(nl)), "adsb_batch_records")
        if nc.value:
            raw = np.ctypeslib.as_array(C.cast(cands, C.POINTER(C.c_uint8)), shape=(nc.value, C.sizeof(Candidate))).copy()
            g, pw = raw[:, 0:8].copy().view(np.uint64)[:, 0], raw[:, 8:12].copy().view(np.uint32)[:, 0]
            out = [(int(g[i]), int(pw[i]), raw[i, 13:13 + raw[i, 12]].tobytes(), int(raw[i, 27])) for i in range(nc.value)]
        else:
            out = []
        t = np.ctypeslib.as_array(tries, shape=(nt.value,)).copy() if nt.value else np.empty(0, np.uint64)
        return out, t, [_struct_dict(segs[i]) for i in range(ns.value)], [_struct_dict(launches[i]) for i in range(nl.value)]

    def batch_unpacked(self, capture: int, n: int):
        """adsb_batch_unpacked_copy: the first n samples of capture `capture` of the last packed or converted batch call
        (decode_batch*_packed, decode_batch*_as with a converted format, decode_batch*_iq with fmt 0), as the batch unpack or
        conversion kernel left them (n may reach into the pad behind the capture, up to its 128-byte-rounded slot).  For a
        converted IQ batch n counts int16 scalars, returned as their 16 bits.  Refused after a batch call that fills no scratch."""
        out = np.empty(n, dtype=np.uint16)
        self._check(self._L.adsb_batch_unpacked_copy(self._h, capture, out.ctypes.data, n), "adsb_batch_unpacked_copy")
        return out

    def decode_packed(self, buf: np.ndarray, chunk: int | None = None, mode: str = "sync"):
        """decode() for packed bytes: chunk counts samples (a multiple of 8); the same three modes."""
        assert buf.dtype == np.uint8 and buf.size % 12 == 0
        assert chunk is None or chunk % 8 == 0
        self.reset()
        step = (chunk if chunk else buf.size // 12 * 8) // 8 * 12   # bytes per push
        pieces = [buf[i:i + step] for i in range(0, buf.size, max(step, 12))]
        out = []
        if mode == "sync":
            for p in pieces:
                self.push_packed(p)
            self.finish()
            return self.drain()
        nbuf = 2 if mode == "async" else 1
        if mode not in ("async", "overlap"):
            raise ValueError(mode)
        with PinnedBuffers(nbuf, max(1, step // 2)) as bufs:
            for k, p in enumerate(pieces):
                b = bufs[k % nbuf].view(np.uint8)[: p.size]
                b[:] = p                    # async: the push from this buffer was two calls ago; overlap: the copy is over
                if mode == "async":
                    self.push_packed_async(b)
                else:
                    self._check(self._L.adsb_push_packed(self._h, b.ctypes.data, b.size // 12 * 8), "adsb_push_packed")
                    b[:] = 0xFF             # the buffer is the caller's again
                out += self.drain()
            self.finish()
            out += self.drain()
        return out

    # ---- signed 16-bit / float32 real input (include/adsbdec_amd.h: fmt is the airspy_rx -t number), converted on the GPU
    @staticmethod
    def _as_arg(fmt, x):
        if isinstance(x, tuple):
            return x
        assert fmt not in FMT_DTYPES or x.dtype == FMT_DTYPES[fmt], (fmt, x.dtype)
        assert x.flags["C_CONTIGUOUS"]
        return x.ctypes.data, x.size

    def push_as(self, fmt: int, x, mode: str = "sync"):
        """adsb_push_as (mode "sync") / adsb_push_async_as ("async": x stays borrowed until the next push/finish/sync returns);
        x = ndarray of the format's dtype, or (ptr, n)."""
        ptr, n = self._as_arg(fmt, x)
        if mode == "async":
            self._check(self._L.adsb_push_async_as(self._h, fmt, ptr, n), "adsb_push_async_as")
        elif mode == "sync":
            self._check(self._L.adsb_push_as(self._h, fmt, ptr, n), "adsb_push_as")
        else:
            raise ValueError(mode)

    def push_device_as(self, fmt: int, ptr: int, n: int, final: bool = False):
        if final:
            self._check(self._L.adsb_push_device_final_as(self._h, fmt, ptr, n), "adsb_push_device_final_as")
        else:
            self._check(self._L.adsb_push_device_as(self._h, fmt, ptr, n), "adsb_push_device_as")

    def decode_device_as_raw(self, fmt: int, ptr: int, n: int):
        """adsb_decode_device_as -> (Frame pointer, count), as decode_device_raw."""
        k = self._L.adsb_decode_device_as(self._h, fmt, ptr, n, self._out_ref)
        if k < 0:
            self._check(-1, "adsb_decode_device_as")
        return self._out, k

    def decode_device_as(self, fmt: int, ptr: int, n: int):
        out, k = self.decode_device_as_raw(fmt, ptr, n)
        return _frames_to_dicts(out, k)

    def decode_batch_device_as(self, fmt: int, ptrs, ns, stats: bool = False):
        """adsb_decode_batch_device_as: captures of format fmt resident in HBM -> what decode_batch_device gives for their raw twins."""
        k = len(ns)
        p = (C.c_void_p * max(1, k))(*[int(v) if v else None for v in ptrs])
        n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_device_as(self._h, fmt, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_device_as")
        return self._batch_result(self._out, first, st, k, stats)

    def decode_batch_as(self, fmt: int, arrays, stats: bool = False):
        """The same for arrays of the format's dtype in host memory: adsb_decode_batch_host_as."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        assert all(fmt not in FMT_DTYPES or a.dtype == FMT_DTYPES[fmt] for a in arrays)
        k = len(arrays)
        p = (C.c_void_p * max(1, k))(*[a.ctypes.data if a.size else None for a in arrays])
        n = (C.c_size_t * max(1, k))(*[a.size for a in arrays])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_host_as(self._h, fmt, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_host_as")
        return self._batch_result(self._out, first, st, k, stats)

    # ---- complex captures (include/adsbdec_amd.h: the _iq calls; fmt 0 FLOAT32_IQ, 2 INT16_IQ, 8 INT8_IQ); n counts COMPLEX samples
    @staticmethod
    def _iq_arg(fmt, x):
        if isinstance(x, tuple):
            return x
        assert fmt not in IQ_DTYPES or x.dtype == IQ_DTYPES[fmt], (fmt, x.dtype)
        assert x.flags["C_CONTIGUOUS"] and x.size % 2 == 0
        return x.ctypes.data, x.size // 2

    def push_iq(self, fmt: int, x, mode: str = "sync"):
        """adsb_push_iq (mode "sync") / adsb_push_iq_async ("async": x stays borrowed until the next push/finish/sync returns);
        x = ndarray of (I, Q) scalars of the format's dtype, or (ptr, n complex samples)."""
        ptr, n = self._iq_arg(fmt, x)
        if mode == "async":
            self._check(self._L.adsb_push_iq_async(self._h, fmt, ptr, n), "adsb_push_iq_async")
        elif mode == "sync":
            self._check(self._L.adsb_push_iq(self._h, fmt, ptr, n), "adsb_push_iq")
        else:
            raise ValueError(mode)

    def push_device_iq(self, fmt: int, ptr: int, n: int, final: bool = False):
        if final:
            self._check(self._L.adsb_push_device_iq_final(self._h, fmt, ptr, n), "adsb_push_device_iq_final")
        else:
            self._check(self._L.adsb_push_device_iq(self._h, fmt, ptr, n), "adsb_push_device_iq")

    def decode_device_iq(self, fmt: int, ptr: int, n: int):
        """adsb_decode_device_iq: one complex capture resident in HBM -> its frames."""
        k = self._L.adsb_decode_device_iq(self._h, fmt, ptr, n, self._out_ref)
        if k < 0:
            self._check(-1, "adsb_decode_device_iq")
        return _frames_to_dicts(self._out, k)

    def decode_iq(self, fmt: int, x: np.ndarray, chunk: int | None = None, mode: str = "sync"):
        """decode() for a complex capture in host memory: chunk counts complex samples (any number); mode "sync" or "async"."""
        x = np.ascontiguousarray(x).reshape(-1, 2)
        self.reset()
        chunk = chunk or max(1, len(x))
        pieces = [x[i:i + chunk] for i in range(0, len(x), chunk)]
        out = []
        if mode == "sync":
            for p in pieces:
                self.push_iq(fmt, p)
            self.finish()
            return self.drain()
        if mode != "async":
            raise ValueError(mode)
        elem = x.dtype.itemsize * 2
        with PinnedBuffers(2, max(1, (min(chunk, max(1, len(x))) * elem + 1) // 2)) as bufs:
            for k, p in enumerate(pieces):
                b = bufs[k % 2].view(np.uint8)[: len(p) * elem].view(x.dtype)
                b[:] = p.reshape(-1)        # the push from this buffer was two calls ago
                self.push_iq(fmt, b, "async")
                out += self.drain()
            self.finish()
            out += self.drain()
        return out

    def decode_batch_device_iq(self, fmt: int, ptrs, ns, stats: bool = False):
        """adsb_decode_batch_device_iq: complex captures resident in HBM (ns in complex samples) -> what decode_batch_device gives."""
        k = len(ns)
        p = (C.c_void_p * max(1, k))(*[int(v) if v else None for v in ptrs])
        n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_device_iq(self._h, fmt, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_device_iq")
        return self._batch_result(self._out, first, st, k, stats)

    def decode_batch_iq(self, fmt: int, arrays, stats: bool = False):
        """The same for arrays of (I, Q) scalars in host memory: adsb_decode_batch_host_iq."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        assert all((fmt not in IQ_DTYPES or a.dtype == IQ_DTYPES[fmt]) and a.size % 2 == 0 for a in arrays)
        k = len(arrays)
        p = (C.c_void_p * max(1, k))(*[a.ctypes.data if a.size else None for a in arrays])
        n = (C.c_size_t * max(1, k))(*[a.size // 2 for a in arrays])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_host_iq(self._h, fmt, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_host_iq")
        return self._batch_result(self._out, first, st, k, stats)

    # ---- float32 power samples (include/adsbdec_amd.h: the _power calls; the reference's ampbuff stream); n counts power samples
    @staticmethod
    def _power_arg(a):
        if isinstance(a, tuple):
            return a
        assert a.dtype == np.dtype("<f4") and a.ndim == 1 and a.flags["C_CONTIGUOUS"], (a.dtype, a.shape)
        return a.ctypes.data, a.size

    def push_power(self, a, mode: str = "sync"):
        """adsb_push_power (mode "sync") / adsb_push_power_async ("async": a stays borrowed until the next push/finish/sync returns);
        a = float32 ndarray of power samples, or (ptr, n)."""
        ptr, n = self._power_arg(a)
        if mode == "async":
            self._check(self._L.adsb_push_power_async(self._h, ptr, n), "adsb_push_power_async")
        elif mode == "sync":
            self._check(self._L.adsb_push_power(self._h, ptr, n), "adsb_push_power")
        else:
            raise ValueError(mode)

    def push_device_power(self, ptr: int, n: int, final: bool = False):
        if final:
            self._check(self._L.adsb_push_device_power_final(self._h, ptr, n), "adsb_push_device_power_final")
        else:
            self._check(self._L.adsb_push_device_power(self._h, ptr, n), "adsb_push_device_power")

    def decode_device_power(self, ptr: int, n: int):
        """adsb_decode_device_power: one capture of power samples resident in HBM -> its frames."""
        k = self._L.adsb_decode_device_power(self._h, ptr, n, self._out_ref)
        if k < 0:
            self._check(-1, "adsb_decode_device_power")
        return _frames_to_dicts(self._out, k)

    def decode_power(self, a: np.ndarray, chunk: int | None = None, mode: str = "sync"):
        """decode() for power samples in host memory: chunk counts power samples (any number); mode "sync" or "async"."""
        a = np.ascontiguousarray(a, dtype="<f4").reshape(-1)
        self.reset()
        chunk = chunk or max(1, len(a))
        pieces = [a[i:i + chunk] for i in range(0, len(a), chunk)]
        out = []
        if mode == "sync":
            for p in pieces:
                self.push_power(p)
            self.finish()
            return self.drain()
        if mode != "async":
            raise ValueError(mode)
        with PinnedBuffers(2, max(1, min(chunk, max(1, len(a))) * 2)) as bufs:   # (PinnedBuffers counts uint16: two per float)
            for k, p in enumerate(pieces):
                b = bufs[k % 2].view(np.uint8)[: len(p) * 4].view("<f4")
                b[:] = p                    # the push from this buffer was two calls ago
                self.push_power(b, "async")
                out += self.drain()
            self.finish()
            out += self.drain()
        return out

    def decode_batch_device_power(self, ptrs, ns, stats: bool = False):
        """adsb_decode_batch_device_power: power captures resident in HBM (ns in power samples) -> what decode_batch_device gives."""
        k = len(ns)
        p = (C.c_void_p * max(1, k))(*[int(v) if v else None for v in ptrs])
        n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_device_power(self._h, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_device_power")
        return self._batch_result(self._out, first, st, k, stats)

    def decode_batch_power(self, arrays, stats: bool = False):
        """The same for float32 arrays in host memory: adsb_decode_batch_host_power."""
        arrays = [np.ascontiguousarray(a) for a in arrays]
        assert all(a.dtype == np.dtype("<f4") and a.ndim == 1 for a in arrays)
        k = len(arrays)
        p = (C.c_void_p * max(1, k))(*[a.ctypes.data if a.size else None for a in arrays])
        n = (C.c_size_t * max(1, k))(*[a.size for a in arrays])
        first = (C.c_uint64 * (k + 1))()
        st = (Stats * max(1, k))()
        if self._L.adsb_decode_batch_host_power(self._h, k, p, n, self._out_ref, first, st) < 0:
            self._check(-1, "adsb_decode_batch_host_power")
        return self._batch_result(self._out, first, st, k, stats)

    # ---- the export calls (include/adsbdec_amd.h: adsb_power_*): the front end's float32 power samples into an array of the caller's
    def _power_call(self, name, *args):
        k = getattr(self._L, name)(self._h, *args)
        if k < 0:
            self._check(-1, name)
        return int(k)

    def power_window(self, ptr: int, first_sample: int, n: int, m_begin: int, m_end: int, out_ptr: int, cap: int) -> int:
        """adsb_power_window: the uint16 samples [first_sample, first_sample + n) in HBM -> power samples [m_begin, m_end) at out_ptr."""
        return self._power_call("adsb_power_window", ptr, first_sample, n, m_begin, m_end, out_ptr, cap)

    def power_window_host(self, x: np.ndarray, first_sample: int, m_begin: int, m_end: int) -> np.ndarray:
        """adsb_power_window_host: x holds the stream's samples from first_sample on -> float32 array of power samples [m_begin, m_end)."""
        x = np.ascontiguousarray(x, dtype=np.uint16)
        out = np.empty(max(0, m_end - m_begin), dtype=np.float32)
        k = self._power_call("adsb_power_window_host", x.ctypes.data, first_sample, x.size, m_begin, m_end, out.ctypes.data, out.size)
        return out[:k]

    def power_device(self, ptr: int, n: int, out_ptr: int, cap: int) -> int:
        """adsb_power_device: a capture of n uint16 samples in HBM as a fresh stream -> its 2 (n // 4) power samples at out_ptr."""
        return self._power_call("adsb_power_device", ptr, n, out_ptr, cap)

    def power_device_as(self, fmt: int, ptr: int, n: int, out_ptr: int, cap: int) -> int:
        return self._power_call("adsb_power_device_as", fmt, ptr, n, out_ptr, cap)

    def power_device_packed(self, ptr: int, n: int, out_ptr: int, cap: int) -> int:
        return self._power_call("adsb_power_device_packed", ptr, n, out_ptr, cap)

    def power_device_iq(self, fmt: int, ptr: int, n: int, out_ptr: int, cap: int) -> int:
        """adsb_power_device_iq: n complex samples in HBM -> n power samples at out_ptr."""
        return self._power_call("adsb_power_device_iq", fmt, ptr, n, out_ptr, cap)

    def power(self, x: np.ndarray) -> np.ndarray:
        """The power samples of a capture in host memory: power_window_host from the stream's start, 2 (n // 4) floats."""
        x = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1)
        return self.power_window_host(x, 0, 0, 2 * (x.size // 4))

    # ---- the export of a batch of captures in one launch (include/adsbdec_amd.h: adsb_power_batch_*)
    @staticmethod
    def _power_batch_args(ptrs, ns, out_ptrs, caps):
        k = len(ns)
        assert len(ptrs) == len(out_ptrs) == len(caps) == k
        arr = lambda t, vals: (t * max(1, k))(*vals)
        return (k, arr(C.c_void_p, [int(v) if v else None for v in ptrs]), arr(C.c_size_t, [int(v) for v in ns]),
                arr(C.c_void_p, [int(v) if v else None for v in out_ptrs]), arr(C.c_size_t, [int(v) for v in caps]))

    def power_batch_device(self, ptrs, ns, out_ptrs, caps) -> int:
        """adsb_power_batch_device: capture i (ns[i] uint16 samples in HBM at ptrs[i]) -> its 2 (ns[i] // 4) power samples at
        out_ptrs[i], as power_device writes them for it alone; one launch for all.  Returns the floats written in all."""
        return self._power_call("adsb_power_batch_device", *self._power_batch_args(ptrs, ns, out_ptrs, caps))

    def power_batch_device_as(self, fmt: int, ptrs, ns, out_ptrs, caps) -> int:
        return self._power_call("adsb_power_batch_device_as", fmt, *self._power_batch_args(ptrs, ns, out_ptrs, caps))

    def power_batch_device_packed(self, ptrs, ns, out_ptrs, caps) -> int:
        return self._power_call("adsb_power_batch_device_packed", *self._power_batch_args(ptrs, ns, out_ptrs, caps))

    def power_batch_device_iq(self, fmt: int, ptrs, ns, out_ptrs, caps) -> int:
        """adsb_power_batch_device_iq: ns[i] complex samples -> ns[i] power samples at out_ptrs[i]."""
        return self._power_call("adsb_power_batch_device_iq", fmt, *self._power_batch_args(ptrs, ns, out_ptrs, caps))

    def power_batch(self, arrays) -> list:
        """The power samples of uint16 captures in host memory, a float32 array of 2 (n // 4) each: adsb_power_batch_host."""
        arrays = [np.ascontiguousarray(a, dtype=np.uint16).reshape(-1) for a in arrays]
        outs = [np.empty(2 * (a.size // 4), dtype=np.float32) for a in arrays]
        args = self._power_batch_args([a.ctypes.data if a.size else None for a in arrays], [a.size for a in arrays],
                                      [o.ctypes.data if o.size else None for o in outs], [o.size for o in outs])
        assert self._power_call("adsb_power_batch_host", *args) == sum(o.size for o in outs)
        return outs

    # ---- the level calls (include/adsbdec_amd.h: adsb_level_*): the power samples the export of the same flavour writes, reduced to a
    # report (counters and a 2048-bin histogram of the floats' bit patterns) and an envelope of one float per 28 power samples
    @staticmethod
    def level_dict(r: "LevelReport", env=None) -> dict:
        """A LevelReport as the dict adsbdec_amd.levels.level_report returns (env: None, or the float32 array that goes with it)."""
        out = {k: int(getattr(r, k)) for k in ("samples", "negative", "rail_lo", "rail_hi", "over")}
        out["hist"] = np.ctypeslib.as_array(r.hist).astype(np.uint64)
        if env is not None:
            out["env"] = env
        return out

    def _level_call(self, name, *args, out=None, env_ptr=0, env_cap=0):
        """-> the report as a dict (no "env": the envelope, if any, is on the device at env_ptr).  out: a LevelReport to fill instead of a new one."""
        r = LevelReport() if out is None else out
        if getattr(self._L, name)(self._h, *args, C.byref(r), env_ptr or None, env_cap) < 0:
            self._check(-1, name)
        return self.level_dict(r)

    def level_device(self, ptr: int, n: int, env_ptr: int = 0, env_cap: int = 0, out=None) -> dict:
        """adsb_level_device: a capture of n uint16 samples in HBM as a fresh stream -> the report of its 2 (n // 4) power samples."""
        return self._level_call("adsb_level_device", ptr, n, out=out, env_ptr=env_ptr, env_cap=env_cap)

    def level_device_as(self, fmt: int, ptr: int, n: int, env_ptr: int = 0, env_cap: int = 0, out=None) -> dict:
        return self._level_call("adsb_level_device_as", fmt, ptr, n, out=out, env_ptr=env_ptr, env_cap=env_cap)

    def level_device_packed(self, ptr: int, n: int, env_ptr: int = 0, env_cap: int = 0, out=None) -> dict:
        return self._level_call("adsb_level_device_packed", ptr, n, out=out, env_ptr=env_ptr, env_cap=env_cap)

    def level_device_iq(self, fmt: int, ptr: int, n: int, env_ptr: int = 0, env_cap: int = 0, out=None) -> dict:
        """adsb_level_device_iq: n complex samples in HBM (fmt 0, 2 or 8) -> the report of their n power samples."""
        return self._level_call("adsb_level_device_iq", fmt, ptr, n, out=out, env_ptr=env_ptr, env_cap=env_cap)

    def level_device_power(self, ptr: int, n: int, env_ptr: int = 0, env_cap: int = 0, out=None) -> dict:
        """adsb_level_device_power: n float32 power samples in HBM -> their report (the domain holds iff negative == 0 and hist[1248:] is empty)."""
        return self._level_call("adsb_level_device_power", ptr, n, out=out, env_ptr=env_ptr, env_cap=env_cap)

    def level(self, x: np.ndarray, env: bool = True) -> dict:
        """The report of a uint16 capture in host memory, adsb_level_host: the counters, "hist" (np.uint64, 2048) and "env" (np.float32,
        one per 28 power samples)."""
        x = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1)
        e = np.empty(-(-(2 * (x.size // 4)) // 28) if env else 0, dtype=np.float32)
        r = LevelReport()
        if self._L.adsb_level_host(self._h, x.ctypes.data if x.size else None, x.size, C.byref(r), e.ctypes.data if e.size else None, e.size) < 0:
            self._check(-1, "adsb_level_host")
        return self.level_dict(r, e)

    # ---- the level reports of a batch of captures, one launch per 1024 (include/adsbdec_amd.h: adsb_level_batch_*)
    def _level_batch_call(self, name, *head, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        """-> a list of level_dict dicts, capture by capture.  env_ptrs / env_caps: both None (no envelope at all), or a device pointer
        (0 / None: none for that capture) and its floats per capture.  out: an array of LevelReport to fill instead of a new one."""
        k = len(ns)
        assert len(ptrs) == k and (env_ptrs is None) == (env_caps is None)
        arr = lambda t, vals: (t * max(1, k))(*vals)
        r = (LevelReport * max(1, k))() if out is None else out
        envs = (None, None) if env_ptrs is None else (arr(C.c_void_p, [int(v) if v else None for v in env_ptrs]), arr(C.c_size_t, [int(v) for v in env_caps]))
        if getattr(self._L, name)(self._h, *head, k, arr(C.c_void_p, [int(v) if v else None for v in ptrs]), arr(C.c_size_t, [int(v) for v in ns]),
                                  r, *envs) < 0:
            self._check(-1, name)
        return [self.level_dict(r[i]) for i in range(k)]

    def level_batch_device(self, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        """adsb_level_batch_device: capture i (ns[i] uint16 samples in HBM at ptrs[i]) -> the report level_device gives for it alone."""
        return self._level_batch_call("adsb_level_batch_device", ptrs=ptrs, ns=ns, env_ptrs=env_ptrs, env_caps=env_caps, out=out)

    def level_batch_device_as(self, fmt: int, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        return self._level_batch_call("adsb_level_batch_device_as", fmt, ptrs=ptrs, ns=ns, env_ptrs=env_ptrs, env_caps=env_caps, out=out)

    def level_batch_device_packed(self, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        return self._level_batch_call("adsb_level_batch_device_packed", ptrs=ptrs, ns=ns, env_ptrs=env_ptrs, env_caps=env_caps, out=out)

    def level_batch_device_iq(self, fmt: int, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        """adsb_level_batch_device_iq: ns[i] complex samples (fmt 0, 2 or 8) -> the report of their ns[i] power samples."""
        return self._level_batch_call("adsb_level_batch_device_iq", fmt, ptrs=ptrs, ns=ns, env_ptrs=env_ptrs, env_caps=env_caps, out=out)

    def level_batch_device_power(self, ptrs, ns, env_ptrs=None, env_caps=None, out=None) -> list:
        return self._level_batch_call("adsb_level_batch_device_power", ptrs=ptrs, ns=ns, env_ptrs=env_ptrs, env_caps=env_caps, out=out)

    def level_batch(self, arrays, env: bool = True) -> list:
        """The reports of uint16 captures in host memory, adsb_level_batch_host: per capture the dict level() returns ("env" where env)."""
        arrays = [np.ascontiguousarray(a, dtype=np.uint16).reshape(-1) for a in arrays]
        es = [np.empty(-(-(2 * (a.size // 4)) // 28) if env else 0, dtype=np.float32) for a in arrays]
        out = self._level_batch_call("adsb_level_batch_host", ptrs=[a.ctypes.data if a.size else None for a in arrays], ns=[a.size for a in arrays],
                                     env_ptrs=[e.ctypes.data if e.size else None for e in es] if env else None,
                                     env_caps=[e.size for e in es] if env else None)
        if env:
            for o, e in zip(out, es):
                o["env"] = e
        return out

    def set_level_batch_blocks(self, blocks: int) -> None:
        """adsb_debug_set_level_batch_blocks: cap the workgroups of a batch level launch (0: the default)."""
        self._check(self._L.adsb_debug_set_level_batch_blocks(self._h, blocks), "adsb_debug_set_level_batch_blocks")

    # ---- the level reports of K consecutive windows of one stream, one launch per 1024 (include/adsbdec_amd.h: adsb_level_windows)
    def level_windows(self, ptr: int, first_sample: int, n: int, edges, env_ptr: int = 0, env_cap: int = 0, out=None) -> list:
        """adsb_level_windows: the uint16 samples [first_sample, first_sample + n) of a stream in HBM -> a list of level_dict dicts,
        window i of power samples [edges[i], edges[i + 1]) (adsbdec_amd.levels.level_windows is the statement).  The one envelope of
        all windows, if any, is on the device at env_ptr.  out: an array of LevelReport to fill instead of a new one."""
        k = len(edges) - 1
        e = (C.c_uint64 * (k + 1))(*[int(v) for v in edges])
        r = (LevelReport * max(1, k))() if out is None else out
        if self._L.adsb_level_windows(self._h, ptr or None, first_sample, n, k, e, r, env_ptr or None, env_cap) < 0:
            self._check(-1, "adsb_level_windows")
        return [self.level_dict(r[i]) for i in range(k)]

    def level_windows_host(self, x: np.ndarray, first_sample: int, edges, env: bool = True):
        """adsb_level_windows_host: x holds the stream's samples from first_sample on -> the list level_windows returns; with env,
        (that list, the float32 envelope of power samples [edges[0], edges[-1]))."""
        x = np.ascontiguousarray(x, dtype=np.uint16).reshape(-1)
        k = len(edges) - 1
        e = (C.c_uint64 * (k + 1))(*[int(v) for v in edges])
        ev = np.empty(-(-(int(edges[-1]) - int(edges[0])) // 28) if env else 0, dtype=np.float32)
        r = (LevelReport * max(1, k))()
        if self._L.adsb_level_windows_host(self._h, x.ctypes.data if x.size else None, first_sample, x.size, k, e, r,
                                           ev.ctypes.data if ev.size else None, ev.size) < 0:
            self._check(-1, "adsb_level_windows_host")
        reports = [self.level_dict(r[i]) for i in range(k)]
        return (reports, ev) if env else reports

    # ---- the gate behind the envelope (include/adsbdec_amd.h: adsb_bursts_*; adsbdec_amd.levels.bursts is the statement)
    # The host program's defaults (-U).  hang: a decode call keeps the reference's end-of-file horizon (deqframe runs once 40 980 power
    # samples are in), so a piece must reach 1 464 runs behind its last frame or it decodes nothing.  factor: an envelope float is the
    # maximum of 28 samples, and over millions of runs the noise's largest one lies some 35 times above the median SAMPLE.  They rest
    # on ONE fixture (tests/burst_cases.py), not on live traffic.
    BURST_LEAD, BURST_HANG, BURST_FACTOR = 2, 1468, 48.0

    def _bursts_call(self, name, ptr, n_env, threshold, lead, hang, cap, table=None):
        """-> (the first min(B, cap) records as a structured array of adsbdec_amd.levels.BURST_DTYPE, B).  table: an array of that
        dtype with room for cap records to write into instead of a new one (the result is a view of its head)."""
        from .levels import BURST_DTYPE
        t = np.zeros(cap, dtype=BURST_DTYPE) if table is None else table
        b = getattr(self._L, name)(self._h, ptr or None, n_env, threshold, lead, hang, t.ctypes.data if cap else None, cap)
        if b < 0:
            self._check(-1, name)
        return t[:min(b, cap)], int(b)

    def bursts_device(self, env_ptr: int, n_env: int, threshold: float, lead: int, hang: int, cap: int, table=None):
        """adsb_bursts_device: the bursts of the n_env floats in HBM at env_ptr -> (records, B); B may exceed cap, cap 0 only counts."""
        return self._bursts_call("adsb_bursts_device", env_ptr, n_env, threshold, lead, hang, cap, table)

    def bursts_host(self, env, threshold: float, lead: int, hang: int, cap: int | None = None, table=None):
        """adsb_bursts_host: ... of a float32 array in host memory (cap None: as many as there are, by a second call where the first
        guess was short)."""
        env = np.ascontiguousarray(env, dtype=np.float32).reshape(-1)
        if cap is not None:
            return self._bursts_call("adsb_bursts_host", env.ctypes.data if env.size else 0, env.size, threshold, lead, hang, cap, table)
        recs, b = self._bursts_call("adsb_bursts_host", env.ctypes.data if env.size else 0, env.size, threshold, lead, hang, 1024)
        if b > 1024:
            recs, b = self._bursts_call("adsb_bursts_host", env.ctypes.data, env.size, threshold, lead, hang, b)
        return recs, b

    # ---- the gate of a slice of a stream (adsb_bursts_slice_*; adsbdec_amd.levels.bursts_slice is the statement)
    def _bursts_slice_call(self, name, ptr, n_env, threshold, lead, hang, carry, final, cap, table=None, out=None):
        """-> (the first min(B, cap) closed records in stream runs, B, the carry out).  carry: a burst_carry(); out: the array to write
        the carry into instead of a new one (carry itself is allowed: in == out)."""
        from .levels import BURST_DTYPE
        t = np.zeros(cap, dtype=BURST_DTYPE) if table is None else table
        o = burst_carry() if out is None else out
        b = getattr(self._L, name)(self._h, ptr or None, n_env, threshold, lead, hang, _carry_array(carry).ctypes.data, int(bool(final)),
                                   t.ctypes.data if cap else None, cap, o.ctypes.data)
        if b < 0:
            self._check(-1, name)
        return t[:min(b, cap)], int(b), o

    def bursts_slice_device(self, env_ptr: int, n_env: int, threshold: float, lead: int, hang: int, carry, final: bool, cap: int, table=None, out=None):
        """adsb_bursts_slice_device: the bursts that the n_env floats in HBM at env_ptr, the next slice of a stream, close -> (records in
        stream runs, B, carry out); B may exceed cap: the same call again with the same carry and more room."""
        return self._bursts_slice_call("adsb_bursts_slice_device", env_ptr, n_env, threshold, lead, hang, carry, final, cap, table, out)

    def bursts_slice_host(self, env, threshold: float, lead: int, hang: int, carry, final: bool, cap: int | None = None, table=None, out=None):
        """adsb_bursts_slice_host: ... of a float32 array in host memory (cap None: as many as there are, by a second call with the same
        carry where the first guess was short)."""
        env = np.ascontiguousarray(env, dtype=np.float32).reshape(-1)
        ptr = env.ctypes.data if env.size else 0
        if cap is not None:
            return self._bursts_slice_call("adsb_bursts_slice_host", ptr, env.size, threshold, lead, hang, carry, final, cap, table, out)
        carry = _carry_array(carry).copy()                       # (out may be carry: the second call needs what came in)
        recs, b, o = self._bursts_slice_call("adsb_bursts_slice_host", ptr, env.size, threshold, lead, hang, carry, final, 1024, out=out)
        if b > 1024:
            recs, b, o = self._bursts_slice_call("adsb_bursts_slice_host", ptr, env.size, threshold, lead, hang, carry, final, b, out=out)
        return recs, b, o

    def bursts(self, x: np.ndarray, q: float = 0.5, factor: float = BURST_FACTOR, lead: int = BURST_LEAD, hang: int = BURST_HANG):
        """A uint16 capture in host memory -> (every burst of its envelope, B): level() with the envelope, the threshold
        float32(factor * percentile(hist, q)) (adsb_level_percentile), and the gate (adsb_bursts_host).
        The default hang (BURST_HANG, 1468 runs) makes every piece long enough for the reference's end-of-file horizon; pieces that go
        to a handle with flush=True need no such length, and hang 4 is enough there."""
        rep = self.level(x, env=True)
        if rep["env"].size == 0:
            from .levels import BURST_DTYPE
            return np.zeros(0, dtype=BURST_DTYPE), 0
        r = LevelReport()
        for k in ("samples", "negative", "rail_lo", "rail_hi", "over"):
            setattr(r, k, rep[k])
        np.ctypeslib.as_array(r.hist)[:] = rep["hist"]
        p = self._L.adsb_level_percentile(C.byref(r), q)
        if p < 0:
            raise AdsbError("adsb_level_percentile: an empty histogram, or q outside [0, 1]")
        return self.bursts_host(rep["env"], float(np.float32(factor * float(p))), lead, hang)

    # ---- a capture's bursts as one array (include/adsbdec_amd.h: adsb_gather_*; adsbdec_amd.burst_archive.gather is the statement)
    def gather_device(self, ptr: int, capture_bytes: int, sample_bytes: int, m: int, bursts, out_ptr: int, out_cap: int):
        """adsb_gather_device: the pieces that the burst table names, of the capture in HBM at ptr, packed into out_ptr (both 16-byte
        aligned) -> offsets, a uint64 array of len(bursts) + 1 byte offsets; offsets[-1] is the total the call returned."""
        b = _burst_table(bursts)
        off = np.zeros(b.size + 1, dtype=np.uint64)
        total = self._L.adsb_gather_device(self._h, ptr or None, capture_bytes, sample_bytes, m, b.ctypes.data if b.size else None, b.size,
                                           out_ptr or None, out_cap, off.ctypes.data)
        if total < 0:
            self._check(-1, "adsb_gather_device")
        assert total == int(off[-1])
        return off

    # ---- ... of a real capture, packed to 12 bits (adsb_gather_pack12_*; adsbdec_amd.burst_archive.gather12 is the statement)
    def _gather_pack12_call(self, name, *head, n: int, bursts, out_ptr: int, out_cap: int):
        b = _burst_table(bursts)
        off = np.zeros(b.size + 1, dtype=np.uint64)
        over = C.c_uint64(0)
        total = getattr(self._L, name)(self._h, *head, n, b.ctypes.data if b.size else None, b.size, out_ptr or None, out_cap, off.ctypes.data,
                                       C.byref(over))
        if total < 0:
            self._check(-1, name)
        assert total == int(off[-1])
        return off, int(over.value)

    def gather_pack12_device(self, ptr: int, n: int, bursts, out_ptr: int, out_cap: int):
        """adsb_gather_pack12_device: the pieces that the burst table names, of the n uint16 samples in HBM at ptr, packed to 12 bits
        into out_ptr (both 16-byte aligned) -> (offsets, over): len(bursts) + 1 byte offsets, offsets[-1] the total the call returned;
        the pieces' own samples above 4095."""
        return self._gather_pack12_call("adsb_gather_pack12_device", ptr or None, n=n, bursts=bursts, out_ptr=out_ptr, out_cap=out_cap)

    def gather_pack12_device_as(self, fmt: int, ptr: int, n: int, bursts, out_ptr: int, out_cap: int):
        """adsb_gather_pack12_device_as: the same for n samples of format fmt (1 float32, 3 int16), converted first."""
        return self._gather_pack12_call("adsb_gather_pack12_device_as", fmt, ptr or None, n=n, bursts=bursts, out_ptr=out_ptr, out_cap=out_cap)

    def gather_pack12_device_packed(self, ptr: int, n: int, bursts, out_ptr: int, out_cap: int):
        """adsb_gather_pack12_device_packed: the same for n samples of packed 12-bit input (4-byte aligned, n % 8 == 0), unpacked first."""
        return self._gather_pack12_call("adsb_gather_pack12_device_packed", ptr or None, n=n, bursts=bursts, out_ptr=out_ptr, out_cap=out_cap)

    def format_report(self):
        """adsb_get_format_report -> (converted, inexact, clamped) since the handle was created or reset."""
        r = FormatReport()
        self._check(self._L.adsb_get_format_report(self._h, C.byref(r)), "adsb_get_format_report")
        return int(r.converted), int(r.inexact), int(r.clamped)

    def decode_as(self, fmt: int, x: np.ndarray, chunk: int | None = None, mode: str = "sync"):
        """decode() for samples of format fmt: chunk counts samples (any number); the same three modes."""
        self.reset()
        chunk = chunk or max(1, x.size)
        pieces = [x[i:i + chunk] for i in range(0, x.size, chunk)]
        out = []
        if mode == "sync":
            for p in pieces:
                self.push_as(fmt, p)
            self.finish()
            return self.drain()
        if mode not in ("async", "overlap"):
            raise ValueError(mode)
        nbuf = 2 if mode == "async" else 1
        elem = x.dtype.itemsize
        with PinnedBuffers(nbuf, max(1, (min(chunk, max(1, x.size)) * elem + 1) // 2)) as bufs:
            for k, p in enumerate(pieces):
                b = bufs[k % nbuf].view(np.uint8)[: p.size * elem].view(x.dtype)
                b[:] = p                    # async: the push from this buffer was two calls ago; overlap: the copy is over
                self.push_as(fmt, b, "async" if mode == "async" else "sync")
                if mode == "overlap":
                    b.view(np.uint8)[:] = 0xFF   # the buffer is the caller's again
                out += self.drain()
            self.finish()
            out += self.drain()
        return out

    def finish(self):
        self._check(self._L.adsb_finish(self._h), "adsb_finish")

    def pending(self) -> int:
        return int(self._L.adsb_pending(self._h))

    def drain_raw(self, reuse: bool = False):
        """All pending frames as one ctypes Frame array (no per-frame Python work).
        reuse=True hands out the handle's own output array (valid until the next such
        call) instead of allocating -- and page-faulting in -- a fresh one every time."""
        n = self.pending()
        if reuse:
            if getattr(self, "_out_cap", 0) < max(1, n):
                self._out_cap = max(1, n + n // 4)
                self._out_buf = (Frame * self._out_cap)()
            buf = self._out_buf
        else:
            buf = (Frame * max(1, n))()
        got = self._L.adsb_drain(self._h, buf, n) if n else 0
        if got < 0:
            raise AdsbError("adsb_drain failed")
        return buf, int(got)

    def take_raw(self):
        """All pending frames in place (adsb_take): (pointer to Frame, count); valid until the
        next push / finish / reset of this decoder."""
        p = C.POINTER(Frame)()
        n = self._L.adsb_take(self._h, C.byref(p))
        if n < 0:
            raise AdsbError("adsb_take failed")
        return p, int(n)

    def drain(self):
        buf, n = self.drain_raw()
        return _frames_to_dicts(buf, n)

    def stats(self):
        st = Stats()
        self._check(self._L.adsb_get_stats(self._h, C.byref(st)), "adsb_get_stats")
        return _stats_to_dict(st, self._fix)

    def profile(self):
        p = Profile()
        if hasattr(self._L, "adsb_get_profile_sized"):
            self._check(self._L.adsb_get_profile_sized(self._h, C.byref(p), C.sizeof(p)), "adsb_get_profile")
        else:   # (an A/B run against a build of rounds 4-5: its struct is a prefix of this one)
            self._L.adsb_get_profile.argtypes = [C.c_void_p, C.POINTER(Profile)]
            self._check(self._L.adsb_get_profile(self._h, C.byref(p)), "adsb_get_profile")
        return {k: getattr(p, k) for k, _ in Profile._fields_}

    def _scan_call(self, fn, name, ptr, first_sample, n, g_begin, g_end, cand_cap, try_cap):
        """adsb_scan_shard or its twin, with the arrays grown until they hold the answer."""
        while True:
            cands = (Candidate * cand_cap)()
            tries = np.empty(try_cap, dtype=np.uint64)
            nc, nt = C.c_size_t(0), C.c_size_t(0)
            rc = fn(self._h, ptr, first_sample, n, g_begin, g_end, cands, cand_cap,
                    C.byref(nc), tries.ctypes.data_as(C.POINTER(C.c_uint64)), try_cap, C.byref(nt))
            if rc == -2:
                cand_cap, try_cap = max(cand_cap, nc.value), max(try_cap, nt.value)
                continue
            self._check(rc, name)
            return cands, nc.value, tries[: nt.value].copy()

    def scan_shard(self, ptr: int, first_sample: int, n: int, g_begin: int, g_end: int,
                   cand_cap: int = 1 << 16, try_cap: int = 1 << 20):
        """Stateless per-shard scan -> (Candidate array, count, tries ndarray)."""
        return self._scan_call(self._L.adsb_scan_shard, "adsb_scan_shard", ptr, first_sample, n, g_begin, g_end, cand_cap, try_cap)

    def scan_wrap_window(self, ptr: int, first_sample: int, n: int, g_begin: int, g_end: int,
                         cand_cap: int = 1 << 14, try_cap: int = 1 << 16):
        """adsb_scan_wrap_window (a handle with long_stream): scan_shard at absolute stream positions, through the wraps."""
        return self._scan_call(self._L.adsb_scan_wrap_window, "adsb_scan_wrap_window", ptr, first_sample, n, g_begin, g_end,
                               cand_cap, try_cap)

    def seam_power(self, ptr: int, first_sample: int, n: int, P: int, g_begin: int, g_end: int) -> np.ndarray:
        """adsb_seam_power: the float32 power samples g_begin .. g_end - 2 + 1196 of one seam launch at the wrap P."""
        out = np.empty(1196 + 28 + 1196, dtype=np.float32)
        k = self._L.adsb_seam_power(self._h, ptr, first_sample, n, P, g_begin, g_end,
                                    out.ctypes.data_as(C.POINTER(C.c_float)), out.size)
        if k < 0:
            self._check(-1, "adsb_seam_power")
        return out[:k].copy()

    def decode(self, x: np.ndarray, chunk: int | None = None, mode: str = "sync"):
        """Whole-buffer convenience: push (optionally in chunks), finish, drain.
        mode "async": adsb_push_async from two alternating page-locked buffers, the
        double-buffered read loop of the C host program."""
        self.reset()
        if mode == "async":
            return self._decode_async(x, chunk or x.size)
        if mode == "overlap":
            return self._decode_overlap(x, chunk or x.size)
        if chunk is None:
            self.push(x)
        else:
            for i in range(0, x.size, chunk):
                self.push(x[i:i + chunk])
        self.finish()
        return self.drain()

    def _decode_async(self, x: np.ndarray, chunk: int):
        out = []
        with PinnedBuffers(2, max(1, min(chunk, max(1, x.size)))) as bufs:
            for k, i in enumerate(range(0, x.size, chunk)):
                piece = x[i:i + chunk]
                b = bufs[k % 2][: piece.size]
                b[:] = piece                # the previous push from this buffer was two calls ago: free again
                self.push_async(b)
                out += self.drain()         # frames of the previous piece
            self.finish()
            out += self.drain()
        return out


    def _decode_overlap(self, x: np.ndarray, chunk: int):
        """cfg.push_overlap: adsb_push from ONE page-locked buffer (fileInput's single iqbuff, air.c:230-239) that is
        overwritten the moment the call returns -- the copy must be complete by then; frames follow one call later."""
        out = []
        with PinnedBuffers(1, max(1, min(chunk, max(1, x.size)))) as bufs:
            for i in range(0, x.size, chunk):
                piece = x[i:i + chunk]
                b = bufs[0][: piece.size]
                b[:] = piece
                self._check(self._L.adsb_push(self._h, b.ctypes.data, b.size), "adsb_push")
                b[:] = 0xFFFF               # the buffer is the caller's again
                out += self.drain()
            self.finish()
            out += self.drain()
        return out


class PinnedBuffers:
    """n page-locked uint16 buffers from adsb_host_alloc, as numpy views."""

    def __init__(self, n: int, samples: int):
        L = load()
        self._L, self._ptrs, self.views = L, [], []
        for _ in range(n):
            p = L.adsb_host_alloc(2 * samples)
            if not p:
                raise AdsbError("adsb_host_alloc failed")
            self._ptrs.append(p)
            self.views.append(np.ctypeslib.as_array((C.c_uint16 * samples).from_address(p)))

    def __enter__(self):
        return self.views

    def __exit__(self, *exc):
        self.views = []
        for p in self._ptrs:
            self._L.adsb_host_free(p)
        self._ptrs = []


class Resolver:
    """Host-side greedy resolver handle (usable without a GPU)."""

    def __init__(self):
        self._L = load()
        self._h = self._L.adsb_resolver_create()

    def close(self):
        if self._h:
            self._L.adsb_resolver_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def feed(self, cands, tries=None):
        """cands: ctypes Candidate array slice or list of (g, pw, frame-bytes)."""
        if isinstance(cands, list):
            arr = (Candidate * max(1, len(cands)))()
            for i, (g, pw, fr) in enumerate(cands):
                arr[i].g, arr[i].pw, arr[i].len = g, pw, len(fr)
                for k, b in enumerate(fr):
                    arr[i].frame[k] = b
            n = len(cands)
        else:
            arr, n = cands
        t = np.ascontiguousarray(tries if tries is not None else np.empty(0, np.uint64), dtype=np.uint64)
        rc = self._L.adsb_resolver_feed(self._h, arr, n, t.ctypes.data_as(C.POINTER(C.c_uint64)), t.size)
        if rc != 0:
            raise AdsbError("adsb_resolver_feed failed")

    def advance(self, power_samples: int, g_complete: int):
        if self._L.adsb_resolver_advance(self._h, power_samples, g_complete) != 0:
            raise AdsbError("adsb_resolver_advance failed")

    def finish_flush(self, power_samples: int):
        """adsb_resolver_finish_flush: the end of a stream of power_samples power samples on a flush handle."""
        if self._L.adsb_resolver_finish_flush(self._h, power_samples) != 0:
            raise AdsbError("adsb_resolver_finish_flush failed")

    def drain(self):
        out = []
        buf = (Frame * 4096)()
        while True:
            n = self._L.adsb_resolver_drain(self._h, buf, 4096)
            if n <= 0:
                return out
            out.extend(_frames_to_dicts(buf, n))

    def stats(self):
        st = Stats()
        self._L.adsb_resolver_stats(self._h, C.byref(st))
        return _stats_to_dict(st)


def _struct_dict(o):
    return {f: int(getattr(o, f)) for f, _ in o._fields_ if f != "pad"}


def batch_layout(ns, cus: int = 0, passes: int = 0, launch_offsets: int = 0, flush: bool = False):
    """adsb_batch_layout_flush -> (segments, launches) as lists of dicts, or None when the batch is refused (a capture of 2^32 samples).
    launch_offsets: adsb_debug_config.batch_launch_offsets (0: the default limit of a launch); flush: as a flush handle lays it out."""
    L = load()
    k = len(ns)
    n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
    nl = C.c_size_t(0)
    ns_ = L.adsb_batch_layout_flush(k, n, cus, passes, launch_offsets, int(flush), None, 0, None, 0, C.byref(nl))
    if ns_ < 0:
        return None
    segs, launches = (BatchSegment * max(1, ns_))(), (BatchLaunch * max(1, nl.value))()
    if L.adsb_batch_layout_flush(k, n, cus, passes, launch_offsets, int(flush), segs, ns_, launches, nl.value, C.byref(nl)) != ns_:
        raise AdsbError("adsb_batch_layout failed")
    return [_struct_dict(segs[i]) for i in range(ns_)], [_struct_dict(launches[i]) for i in range(nl.value)]


def multi_batch_plan(ns, n_workers: int, batch_bytes: int = 0, packed: bool = False):
    """adsb_multi_batch_plan -> (range: n_workers + 1 capture indices, subs: the sub-batches' starts and len(ns) behind them)."""
    L = load()
    k = len(ns)
    n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
    rng = (C.c_size_t * (n_workers + 1))()
    cap = k + 1                                   # a sub-batch holds a capture at least
    subs = (C.c_size_t * cap)()
    nsub = L.adsb_multi_batch_plan(k, n, n_workers, batch_bytes, int(packed), rng, subs, cap)
    if nsub < 0:
        raise AdsbError("adsb_multi_batch_plan failed")
    return [int(v) for v in rng], [int(subs[i]) for i in range(nsub + 1)]


def batch_resolve(ns, cands, tries, cus: int = 0, passes: int = 0, launch_offsets: int = 0, flush: bool = False):
    """adsb_batch_resolve_ex (launch_offsets as batch_layout): cands = list of (virtual g, pw, frame bytes) ascending, tries = uint64 (g << 2 | code) ascending ->
    (per-capture frame lists, per-capture Try/Ok tables)."""
    L = load()
    k = len(ns)
    n = (C.c_size_t * max(1, k))(*[int(v) for v in ns])
    arr = (Candidate * max(1, len(cands)))()
    for i, (g, pw, fr) in enumerate(cands):
        arr[i].g, arr[i].pw, arr[i].len = g, pw, len(fr)
        for j, b in enumerate(fr):
            arr[i].frame[j] = b
    t = np.ascontiguousarray(tries, dtype=np.uint64)
    first, st = (C.c_uint64 * (k + 1))(), (Stats * max(1, k))()
    cap = len(cands) + 1
    out = (Frame * cap)()
    total = L.adsb_batch_resolve_flush(k, n, cus, passes, launch_offsets, int(flush), arr, len(cands), t.ctypes.data_as(C.POINTER(C.c_uint64)), t.size, out, cap, first, st)
    if total < 0 or total > cap:
        raise AdsbError("adsb_batch_resolve failed")
    return ([_frames_to_dicts(out[int(first[i]):int(first[i + 1])], int(first[i + 1] - first[i])) for i in range(k)],
            [_stats_to_dict(st[i]) for i in range(k)])


def plan_shards(total_samples: int, n_shards: int):
    arrs = [(C.c_uint64 * n_shards)() for _ in range(4)]
    if load().adsb_plan_shards(total_samples, n_shards, *arrs) != 0:
        raise AdsbError("adsb_plan_shards failed")
    return [dict(g_begin=int(arrs[0][i]), g_end=int(arrs[1][i]), first_sample=int(arrs[2][i]),
                 n_samples=int(arrs[3][i])) for i in range(n_shards)]


def _burst_table(bursts) -> np.ndarray:
    from .levels import BURST_DTYPE
    return np.ascontiguousarray(np.asarray(bursts, dtype=BURST_DTYPE).reshape(-1))


def burst_carry() -> np.ndarray:
    """A zeroed adsb_burst_carry, the start of a stream: one record of adsbdec_amd.levels.BURST_CARRY_DTYPE."""
    from .levels import burst_carry as zeroed
    return zeroed()


def _carry_array(carry) -> np.ndarray:
    from .levels import BURST_CARRY_DTYPE
    c = np.ascontiguousarray(np.asarray(carry, dtype=BURST_CARRY_DTYPE).reshape(-1))
    if c.size != 1:
        raise ValueError("a carry is one record of levels.BURST_CARRY_DTYPE")
    return c


def gather_layout(bursts, m: int, sample_bytes: int) -> np.ndarray:
    """adsb_gather_layout (no device): the byte offsets of the pieces of a burst table in what adsb_gather_device writes, a uint64
    array of len(bursts) + 1; offsets[-1] is the total.  AdsbError, naming the record, where the call refuses."""
    L = load()
    b = _burst_table(bursts)
    off = np.zeros(b.size + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    if L.adsb_gather_layout(m, sample_bytes, b.ctypes.data if b.size else None, b.size, off.ctypes.data, C.byref(total)) != 0:
        raise AdsbError((L.adsb_last_error(None) or b"").decode())
    assert int(total.value) == int(off[-1])
    return off


def gather_pack12_layout(bursts, m: int) -> np.ndarray:
    """adsb_gather_pack12_layout (no device): the byte offsets of the packed pieces of a burst table in what adsb_gather_pack12_*
    write, a uint64 array of len(bursts) + 1; offsets[-1] is the total.  AdsbError, naming the record, where the call refuses."""
    L = load()
    b = _burst_table(bursts)
    off = np.zeros(b.size + 1, dtype=np.uint64)
    total = C.c_uint64(0)
    if L.adsb_gather_pack12_layout(m, b.ctypes.data if b.size else None, b.size, off.ctypes.data, C.byref(total)) != 0:
        raise AdsbError((L.adsb_last_error(None) or b"").decode())
    assert int(total.value) == int(off[-1])
    return off


def gather_chunk_words() -> int:
    """adsb_gather_chunk_words: C, the 16-byte output words one workgroup of the gather kernel takes at once."""
    return int(load().adsb_gather_chunk_words())


def burst_tile_runs() -> int:
    """adsb_burst_tile_runs: T, the runs one workgroup of the gate's kernels takes."""
    return int(load().adsb_burst_tile_runs())


def level_percentile(hist, q: float) -> float:
    """adsb_level_percentile on a histogram of 2048 counts: what adsbdec_amd.levels.percentile states, computed by the library (-1.0: an
    empty histogram, or q outside [0, 1])."""
    r = LevelReport()
    np.ctypeslib.as_array(r.hist)[:] = np.asarray(hist, dtype=np.uint64)
    return float(load().adsb_level_percentile(C.byref(r), q))


def level_add(r: dict, s: dict) -> dict:
    """adsb_level_add on two report dicts (Decoder.level_dict's): what adsbdec_amd.levels.add states, computed by the library."""
    def struct(d):
        o = LevelReport()
        for k in ("samples", "negative", "rail_lo", "rail_hi", "over"):
            setattr(o, k, int(d[k]))
        np.ctypeslib.as_array(o.hist)[:] = np.asarray(d["hist"], dtype=np.uint64)
        return o
    a, b = struct(r), struct(s)
    load().adsb_level_add(C.byref(a), C.byref(b))
    return Decoder.level_dict(a)
