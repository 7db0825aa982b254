"""ctypes binding of libtoolame_dab_hip.so (include/toolame_batch.h).

Mirrors the reference's operator interface for this path: the six setters of
libtoolame-dab/toolame.h:13-48 become the fields of StreamConfig (same names, same argument meaning,
same validity rules), `Batch.encode()` is toolame_encode_frame() over N streams and F frames, and
`Batch.flush()` is toolame_finish().  Errors surface as ToolameError with the library's code, where
the reference returns non-zero or exit()s.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass
from pathlib import Path

import numpy as np

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("TLB_LIB_PATH") or PKG_DIR / "libtoolame_dab_hip.so")     # TLB_LIB_PATH: kernel experiments (tools/) only
FAULT_LIB_PATH = PKG_DIR / "libtoolame_dab_hip_fi.so"    # TEST build with fault injection (csrc/tlb_debug.h, `make fault`); never the product
MAX_XPAD = 256
SAMPLES = 1152

_ERR = {1: "illegal sample rate (48000/44100/32000/24000/22050/16000 Hz; the egress calls: no 32/44.1/22.05 kHz)", 2: "bad channel mode", 3: "invalid PSY model",
        4: "illegal bitrate for this MPEG version", 5: "invalid XPAD length", 16: "no usable HIP device",
        17: "HIP runtime error", 18: "bad argument", 19: "a shard missed the node's tick deadline (it is LATE)"}


class ToolameError(RuntimeError):
    def __init__(self, code, what=""):
        self.code = code
        super().__init__(f"libtoolame-dab-hip: {what or 'error'}: {_ERR.get(code, 'unknown')} (code {code})")


@dataclass(frozen=True)
class StreamConfig:
    """toolame_set_samplerate / _channel_mode / _bitrate / _psy_model / _pad (toolame.c:174-262)."""
    samplerate: int = 48000
    mode: str = "j"          # odr-audioenc's default for two channels (src/odr-audioenc.cpp:697-709)
    bitrate: int = 128
    psy_model: int = 1
    pad_len: int = 0


class _CConfig(C.Structure):
    _fields_ = [("samplerate", C.c_long), ("mode", C.c_char), ("bitrate", C.c_int), ("psy_model", C.c_int),
                ("pad_len", C.c_int)]


@dataclass(frozen=True)
class FeedConfig:
    """tlb_feed_config: a stream's source arrives as MPEG Layer II frames of this rate, bitrate and channel count (1 | 2)"""
    samplerate: int = 48000
    bitrate: int = 192
    channels: int = 2


class _CFeedConfig(C.Structure):
    _fields_ = [("samplerate", C.c_long), ("bitrate", C.c_int), ("channels", C.c_int)]


def _c_feed(cfg):
    return _CFeedConfig(int(cfg.samplerate), int(cfg.bitrate), int(cfg.channels))


_lib = None


def build(verbose=False):
    """Compile csrc/ for gfx950 into libtoolame_dab_hip.so (hipcc cross-compiles without a GPU), and the fault-injection TEST build
    of the same kernels beside it (libtoolame_dab_hip_fi.so: host files only, seconds)."""
    for target in ([], ["fault"]):
        r = subprocess.run(["make", "-j4", "-C", str(PKG_DIR / "csrc")] + target, capture_output=not verbose, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc build failed:\n" + (r.stdout or "") + (r.stderr or ""))
    return LIB_PATH


_fault_lib = None


def load_fault_library():
    """The TEST build with fault injection (csrc/tlb_debug.h) as a second, independent library object: pass it as `lib=` to Batch / Tick /
    Node.  Only tests use it -- the product library has no such entry points."""
    global _fault_lib
    if _fault_lib is None:
        if not FAULT_LIB_PATH.exists():
            raise ToolameError(16, f"{FAULT_LIB_PATH} is missing (make -C odr-audioenc_amd/csrc fault)")
        L = _bind(C.CDLL(str(FAULT_LIB_PATH)))
        L.tlb_debug_fail_next.argtypes = [C.c_void_p, C.c_int]
        L.tlb_debug_tick_fail_next.argtypes = [C.c_void_p, C.c_int]
        L.tlb_debug_node_fail_next.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tlb_debug_tick_damage_next.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        if hasattr(L, "tlb_debug_tick_cross_from"):
            L.tlb_debug_tick_cross_from.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tlb_debug_node_stall_next.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
        L.tlb_debug_alloc_fail_next.argtypes = [C.c_int]
        _fault_lib = L
    return _fault_lib


def load_library():
    """Load the HIP library or raise -- there is no CPU fallback for the product path."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise ToolameError(16, f"{LIB_PATH} is missing (run __graft_entry__.build())")
    _lib = _bind(C.CDLL(str(LIB_PATH)))
    return _lib


def _bind(L):
    """argument / result types of every entry point of include/toolame_batch.h"""
    L.tlb_create.restype = C.c_void_p
    L.tlb_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
    L.tlb_destroy.argtypes = [C.c_void_p]
    L.tlb_reset.argtypes = [C.c_void_p]
    for f in ("tlb_nstreams", "tlb_out_stride"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.tlb_frame_bytes.argtypes = [C.c_void_p, C.c_int]
    L.tlb_frames_encoded.argtypes = [C.c_void_p]
    L.tlb_frames_encoded.restype = C.c_long
    L.tlb_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_encode_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_host_alloc.restype = C.c_void_p
    L.tlb_host_alloc.argtypes = [C.c_size_t]
    L.tlb_host_free.argtypes = [C.c_void_p]
    L.tlb_host_free.restype = None
    L.tlb_flush_host.argtypes = [C.c_void_p, C.c_void_p]
    L.tlb_flush_host_len.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_encode_host_len.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_encode_device_len.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_flush_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_last_kernel_ms.argtypes = [C.c_void_p]
    L.tlb_last_kernel_ms.restype = C.c_float
    L.tlb_last_stage_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    L.tlb_version.restype = C.c_char_p
    L.tlb_set_gain_db.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.tlb_ingest_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_ingest_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    for f in ("tlb_egress_unit_bytes", "tlb_egress_units_per_frame"):
        getattr(L, f).argtypes = [C.c_void_p, C.c_int]
    L.tlb_egress_max_units_per_frame.argtypes = [C.c_void_p]
    L.tlb_zmq_msg_stride.argtypes = [C.c_void_p]
    L.tlb_zmq_frame_host.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    L.tlb_edi_state_init.argtypes = [C.c_void_p, C.c_longlong, C.c_uint, C.c_int, C.c_int]
    L.tlb_edi_state_init.restype = None
    L.tlb_edi_af_stride.argtypes = [C.c_void_p, C.c_int]
    L.tlb_edi_af_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_edi_af_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_int, C.c_void_p, C.c_void_p]
    L.tlb_edi_pft_shape.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tlb_edi_pft_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_int] * 2
    L.tlb_edi_pft_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p] + [C.c_int] * 5 + [C.c_void_p] * 3 + [C.c_int] * 2 + [C.c_void_p]
    L.tlb_stream_reset.argtypes = [C.c_void_p, C.c_int]
    L.tlb_stream_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tlb_stream_reconfigure.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.tlb_tick_stream_reset.argtypes = [C.c_void_p, C.c_int]
    L.tlb_tick_stream_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tlb_tick_stream_reconfigure.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.tlb_tick_create.restype = C.c_void_p
    L.tlb_tick_create.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.tlb_tick_destroy.argtypes = [C.c_void_p]
    L.tlb_tick_destroy.restype = None
    for f in ("tlb_tick_pcm", "tlb_tick_xpad", "tlb_tick_xpad_len", "tlb_tick_peaks"):
        getattr(L, f).restype = C.c_void_p
        getattr(L, f).argtypes = [C.c_void_p]
    for f in ("tlb_tick_run", "tlb_tick_finish", "tlb_tick_submit", "tlb_tick_wait"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.tlb_tick_count.argtypes = [C.c_void_p]
    L.tlb_tick_count.restype = C.c_long
    L.tlb_tick_set_gain_db.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.tlb_tick_units.argtypes = [C.c_void_p, C.c_int]
    L.tlb_tick_frame.restype = C.c_void_p
    L.tlb_tick_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    L.tlb_tick_packet.restype = C.c_void_p
    L.tlb_tick_packet.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tlb_tick_message.restype = C.c_void_p
    L.tlb_tick_message.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tlb_tick_silence_ms.restype = C.c_void_p
    L.tlb_tick_silence_ms.argtypes = [C.c_void_p]
    L.tlb_tick_fragments.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.tlb_tick_fragment.restype = C.c_void_p
    L.tlb_tick_fragment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tlb_tick_last_ms.argtypes = [C.c_void_p]
    L.tlb_tick_last_ms.restype = C.c_float
    # node level (include/toolame_batch.h part 3)
    L.tlb_node_partition.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.tlb_node_partition.restype = None
    L.tlb_node_plan_shard.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int] + [C.POINTER(C.c_int)] * 3 + [C.c_void_p, C.POINTER(C.c_int)]
    L.tlb_node_create.restype = C.c_void_p
    L.tlb_node_create.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]
    L.tlb_node_destroy.argtypes = [C.c_void_p]
    L.tlb_node_destroy.restype = None
    for f in ("tlb_node_nshards", "tlb_node_nstreams", "tlb_node_submit", "tlb_node_wait", "tlb_node_run", "tlb_node_finish", "tlb_node_sync"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.tlb_node_shard_of.argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_counters.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_node_parallel.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    for f in ("tlb_node_pcm", "tlb_node_xpad", "tlb_node_xpad_len", "tlb_node_peaks"):
        getattr(L, f).restype = C.c_void_p
        getattr(L, f).argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_units.argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_silence_ms.argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_silence_ms.restype = C.c_uint32
    L.tlb_node_frame.restype = C.c_void_p
    L.tlb_node_frame.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int)]
    for f in ("tlb_node_packet", "tlb_node_message"):
        getattr(L, f).restype = C.c_void_p
        getattr(L, f).argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tlb_node_fragments.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.tlb_node_fragment.restype = C.c_void_p
    L.tlb_node_fragment.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]
    L.tlb_node_set_gain_db.argtypes = [C.c_void_p, C.c_int, C.c_double]
    L.tlb_node_stream_reset.argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_stream_finish.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_size_t]
    L.tlb_node_stream_reconfigure.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.tlb_node_batch.restype = C.c_void_p
    L.tlb_node_batch.argtypes = [C.c_void_p, C.c_int]
    L.tlb_node_device_alloc.restype = C.c_void_p
    L.tlb_node_device_alloc.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    L.tlb_node_device_free.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.tlb_node_device_free.restype = None
    L.tlb_node_copy_in.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.tlb_node_copy_out.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t]
    L.tlb_node_encode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.tlb_node_flush_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "tlb_decode_device"):           # frame check / decode (an older build loaded through TLB_LIB_PATH has none of it)
        L.tlb_decode_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_decode_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_decode_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_decode_bad_frames.argtypes = [C.c_void_p]
        L.tlb_decode_bad_frames.restype = C.c_long
    if hasattr(L, "tlb_ingest_device_valid"):     # short reads (an older build loaded through TLB_LIB_PATH has none of it)
        L.tlb_ingest_device_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_ingest_host_valid.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_underrun_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_underrun_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        for f in ("tlb_tick_valid", "tlb_tick_underrun_ms", "tlb_tick_underruns"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p]
        L.tlb_tick_enable_short_reads.argtypes = [C.c_void_p]
        L.tlb_node_enable_short_reads.argtypes = [C.c_void_p]
        L.tlb_node_valid.restype = C.c_void_p
        L.tlb_node_valid.argtypes = [C.c_void_p, C.c_int]
        for f in ("tlb_node_underrun_ms", "tlb_node_underruns"):
            getattr(L, f).restype = C.c_uint32
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_monitor_device"):          # confidence monitor (an older build loaded through TLB_LIB_PATH has none of it)
        L.tlb_monitor_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_monitor_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_tick_enable_monitor.argtypes = [C.c_void_p, C.c_int]
        L.tlb_tick_monitor.restype = C.c_void_p
        L.tlb_tick_monitor.argtypes = [C.c_void_p]
        L.tlb_tick_monitor_listen.argtypes = [C.c_void_p, C.c_int]
        L.tlb_tick_monitor_pcm.restype = C.c_void_p
        L.tlb_tick_monitor_pcm.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
        L.tlb_node_enable_monitor.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_monitor.restype = C.c_void_p
        L.tlb_node_monitor.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_monitor_listen.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_monitor_pcm.restype = C.c_void_p
        L.tlb_node_monitor_pcm.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    if hasattr(L, "tlb_compare_device"):          # compare monitor
        L.tlb_compare_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_compare_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_compare_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_tick_enable_compare.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_tick_compare.restype = C.c_void_p
        L.tlb_tick_compare.argtypes = [C.c_void_p]
        L.tlb_node_enable_compare.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_node_compare.restype = C.c_void_p
        L.tlb_node_compare.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_resample_device"):         # device resampler
        L.tlb_resample_set_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_resample_source.restype = C.c_long
        L.tlb_resample_source.argtypes = [C.c_void_p, C.c_int]
        L.tlb_resample_need.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tlb_resample_need_at.argtypes = [C.c_long, C.c_long, C.c_long]
        L.tlb_resample_taps.restype = C.c_void_p
        L.tlb_resample_taps.argtypes = [C.c_long, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.tlb_resample_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_resample_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_tick_set_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_tick_need.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_set_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_node_need.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_loudness_device"):         # loudness meter
        L.tlb_loudness_enable.argtypes = [C.c_void_p]
        L.tlb_loudness_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_loudness_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_loudness_programme_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_loudness_programme_host.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_loudness_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_loudness_taps.argtypes = [C.c_long, C.c_void_p]
        L.tlb_loudness_scale.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_loudness_lufs.restype = C.c_double
        L.tlb_loudness_lufs.argtypes = [C.c_double]
        L.tlb_tick_enable_loudness.argtypes = [C.c_void_p]
        L.tlb_tick_loudness.restype = C.c_void_p
        L.tlb_tick_loudness.argtypes = [C.c_void_p]
        L.tlb_tick_loudness_programme.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_tick_loudness_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_enable_loudness.argtypes = [C.c_void_p]
        L.tlb_node_loudness.restype = C.c_void_p
        L.tlb_node_loudness.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_loudness_programme.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_node_loudness_reset.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_lra_device"):              # loudness range on top of the loudness meter
        L.tlb_lra_enable.argtypes = [C.c_void_p]
        L.tlb_lra_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_lra_host.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_lra_lu.restype = C.c_double
        L.tlb_lra_lu.argtypes = [C.c_void_p]
        L.tlb_tick_enable_lra.argtypes = [C.c_void_p]
        L.tlb_tick_lra.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_node_enable_lra.argtypes = [C.c_void_p]
        L.tlb_node_lra.argtypes = [C.c_void_p, C.c_void_p]
    if hasattr(L, "tlb_truepeak_device"):         # true-peak meter
        L.tlb_truepeak_enable.argtypes = [C.c_void_p, C.c_uint32]
        L.tlb_truepeak_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_truepeak_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_truepeak_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_truepeak_taps.argtypes = [C.c_void_p]
        L.tlb_truepeak_dbtp.restype = C.c_double
        L.tlb_truepeak_dbtp.argtypes = [C.c_uint32]
        L.tlb_tick_enable_truepeak.argtypes = [C.c_void_p, C.c_uint32]
        L.tlb_tick_truepeak.restype = C.c_void_p
        L.tlb_tick_truepeak.argtypes = [C.c_void_p]
        L.tlb_tick_truepeak_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_enable_truepeak.argtypes = [C.c_void_p, C.c_uint32]
        L.tlb_node_truepeak.restype = C.c_void_p
        L.tlb_node_truepeak.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_truepeak_reset.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_limiter_device"):          # true-peak limiter
        L.tlb_limiter_enable.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_limiter_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_limiter_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_limiter_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_limiter_step.restype = C.c_uint32
        L.tlb_limiter_step.argtypes = [C.c_uint32, C.c_long]
        L.tlb_tick_enable_limiter.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_tick_limiter.restype = C.c_void_p
        L.tlb_tick_limiter.argtypes = [C.c_void_p]
        L.tlb_tick_limiter_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_enable_limiter.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_node_limiter.restype = C.c_void_p
        L.tlb_node_limiter.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_limiter_reset.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_conceal_enable"):          # feed concealment
        L.tlb_conceal_enable.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tlb_conceal_get.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.tlb_conceal_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_conceal_records_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_conceal_records_host.argtypes = [C.c_void_p, C.c_void_p]
        L.tlb_tick_enable_conceal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tlb_tick_conceal.restype = C.c_void_p
        L.tlb_tick_conceal.argtypes = [C.c_void_p]
        L.tlb_tick_conceal_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_enable_conceal.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
        L.tlb_node_conceal.restype = C.c_void_p
        L.tlb_node_conceal.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_conceal_reset.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_feed_loss_enable"):     # ... on adapted and down feeds
        for name in ("tlb_feed_loss_enable", "tlb_tick_enable_feed_loss", "tlb_node_enable_feed_loss"):
            getattr(L, name).argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "tlb_decimate_device"):         # device decimator (down sources)
        L.tlb_decimate_set_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_decimate_source.restype = C.c_long
        L.tlb_decimate_source.argtypes = [C.c_void_p, C.c_int]
        L.tlb_decimate_need.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tlb_decimate_need_at.argtypes = [C.c_long, C.c_long, C.c_long]
        L.tlb_decimate_taps.restype = C.c_void_p
        L.tlb_decimate_taps.argtypes = [C.c_long, C.c_long, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.tlb_decimate_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_decimate_host.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_tick_set_down_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_tick_down.restype = C.c_void_p
        L.tlb_tick_down.argtypes = [C.c_void_p, C.c_int]
        L.tlb_tick_down_need.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_set_down_source.argtypes = [C.c_void_p, C.c_int, C.c_long]
        L.tlb_node_down.restype = C.c_void_p
        L.tlb_node_down.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_down_need.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_feed_set"):               # Layer II feeds
        L.tlb_feed_check_config.argtypes = [C.c_void_p]
        L.tlb_feed_frame_bytes.argtypes = [C.c_void_p]
        L.tlb_feed_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_stride.argtypes = [C.c_void_p]
        L.tlb_feed_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_feed_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        L.tlb_feed_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.tlb_tick_set_feed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in ("tlb_tick_feed", "tlb_tick_feed_len", "tlb_tick_feed_report"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p]
        L.tlb_tick_feed_stride.argtypes = [C.c_void_p]
        L.tlb_node_set_feed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in ("tlb_node_feed", "tlb_node_feed_len", "tlb_node_feed_report"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_feed_stride.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_feed_set_adapted"):       # adapted feeds: another rate or channel count than the stream's
        L.tlb_feed_set_adapted.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_adapted.argtypes = [C.c_void_p, C.c_int]
        L.tlb_feed_want.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tlb_feed_want_at.argtypes = [C.c_long, C.c_long, C.c_long]
        L.tlb_tick_set_feed_adapted.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_tick_feed_want.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_set_feed_adapted.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_node_feed_want.argtypes = [C.c_void_p, C.c_int]
    if hasattr(L, "tlb_feed_down_set"):          # down feeds: 48, 44.1 and 32 kHz Layer II feeds for 24 kHz streams, two slots per tick
        L.tlb_feed_down_set.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_down_get.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_down_want.argtypes = [C.c_void_p, C.c_int, C.c_int]
        L.tlb_feed_down_want_at.argtypes = [C.c_long, C.c_long, C.c_long]
        L.tlb_feed_down_stride.argtypes = [C.c_void_p]
        L.tlb_feed_down_reset.argtypes = [C.c_void_p, C.c_int]
        L.tlb_feed_down_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_feed_down_host.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
        L.tlb_tick_set_down_feed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in ("tlb_tick_down_feed", "tlb_tick_down_feed_len", "tlb_tick_down_feed_report"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p]
        L.tlb_tick_down_feed_stride.argtypes = [C.c_void_p]
        L.tlb_tick_down_feed_want.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_set_down_feed.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        for f in ("tlb_node_down_feed", "tlb_node_down_feed_len", "tlb_node_down_feed_report"):
            getattr(L, f).restype = C.c_void_p
            getattr(L, f).argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_down_feed_stride.argtypes = [C.c_void_p, C.c_int]
        L.tlb_node_down_feed_want.argtypes = [C.c_void_p, C.c_int]
    L.toolame_set_samplerate.argtypes = [C.c_long]
    L.toolame_set_channel_mode.argtypes = [C.c_char]
    L.toolame_encode_frame.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    L.toolame_finish.argtypes = [C.c_void_p, C.c_size_t]
    if hasattr(L, "tlb_node_shard_status"):       # (an older build loaded through TLB_LIB_PATH for a kernel A/B has none of the round-6 entry points)
        L.tlb_tick_status.argtypes = [C.c_void_p]
        L.tlb_node_describe.argtypes = [C.c_void_p]
        L.tlb_node_describe.restype = C.c_char_p
        L.tlb_node_shard_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        L.tlb_node_shard_restart.argtypes = [C.c_void_p, C.c_int, C.c_longlong]
    if hasattr(L, "tlb_node_set_deadline_ms"):
        L.tlb_node_set_deadline_ms.argtypes = [C.c_void_p, C.c_double]
        L.tlb_node_shard_deadline_status.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def resample_need_at(source_rate, encoder_rate, frame):
    """source frames frame `frame` (from the stream's reset) of a source_rate -> encoder_rate stream consumes: host arithmetic, no GPU"""
    n = load_library().tlb_resample_need_at(int(source_rate), int(encoder_rate), int(frame))
    if n < 0:
        raise ToolameError(-n, "tlb_resample_need_at")
    return n


def resample_taps(source_rate, encoder_rate):
    """the committed polyphase table of the pair -> (int16 [L, T] copy, L, M); None when the pair is not supported"""
    l, m, tt = C.c_int(0), C.c_int(0), C.c_int(0)
    p = load_library().tlb_resample_taps(int(source_rate), int(encoder_rate), C.byref(l), C.byref(m), C.byref(tt))
    if not p:
        return None
    return np.ctypeslib.as_array((C.c_int16 * (l.value * tt.value)).from_address(p)).reshape(l.value, tt.value).copy(), l.value, m.value


DECIMATE_SLOT = 4608      # int16 per wide slot (TLB_DECIMATE_SLOT)


def decimate_need_at(source_rate, encoder_rate, frame):
    """source frames frame `frame` (from the stream's reset) of a down source (48 / 44.1 / 32 kHz -> 24 kHz) consumes: host arithmetic, no GPU"""
    n = load_library().tlb_decimate_need_at(int(source_rate), int(encoder_rate), int(frame))
    if n < 0:
        raise ToolameError(-n, "tlb_decimate_need_at")
    return n


def decimate_taps(source_rate, encoder_rate):
    """the committed polyphase table of the down pair -> (int16 [L, T] copy, L, M); None when the pair is not supported"""
    l, m, tt = C.c_int(0), C.c_int(0), C.c_int(0)
    p = load_library().tlb_decimate_taps(int(source_rate), int(encoder_rate), C.byref(l), C.byref(m), C.byref(tt))
    if not p:
        return None
    return np.ctypeslib.as_array((C.c_int16 * (l.value * tt.value)).from_address(p)).reshape(l.value, tt.value).copy(), l.value, m.value


# tlb_loudness_record / tlb_loudness_programme_record: energies, LUFS = loudness_lufs(E)
LOUDNESS_DTYPE = np.dtype([("frames", np.uint32), ("bins", np.uint32), ("blocks", np.uint32), ("gated", np.uint32),
                           ("momentary", np.float64), ("short_term", np.float64), ("momentary_max", np.float64), ("short_term_max", np.float64)])
LOUDNESS_PROGRAMME_DTYPE = np.dtype([("integrated", np.float64), ("gate", np.float64), ("gated", np.uint32), ("reserved", np.uint32)])
LOUDNESS_BINS = 751


def loudness_lufs(energy):
    """-0.691 + 10 log10(energy); -inf for 0 (tlb_loudness_lufs)"""
    return float(load_library().tlb_loudness_lufs(float(energy)))


def loudness_taps(samplerate):
    """the committed K-weighting row of an encoder rate -> float64 [10]: b0 b1 b2 a1 a2 of the shelf, then of the high-pass; no GPU"""
    out = np.zeros(10, dtype=np.float64)
    rc = load_library().tlb_loudness_taps(int(samplerate), out.ctypes.data)
    if rc:
        raise ToolameError(rc, "tlb_loudness_taps")
    return out


def loudness_scale():
    """the committed gating scale -> (edges float64 [751], centres float64 [751]); no GPU"""
    edges, centres = np.zeros(LOUDNESS_BINS, dtype=np.float64), np.zeros(LOUDNESS_BINS, dtype=np.float64)
    rc = load_library().tlb_loudness_scale(edges.ctypes.data, centres.ctypes.data)
    if rc:
        raise ToolameError(rc, "tlb_loudness_scale")
    return edges, centres


# tlb_lra_record: the 10th and the 95th percentile and the relative gate as energies, the counted and the gated range blocks, the two bins
LRA_DTYPE = np.dtype([("low", np.float64), ("high", np.float64), ("gate", np.float64), ("blocks", np.uint32), ("gated", np.uint32),
                      ("low_bin", np.int32), ("high_bin", np.int32)])


def lra_lu(rec):
    """loudness range of one LRA_DTYPE record in LU: 0.1 * (high_bin - low_bin) (tlb_lra_lu)"""
    a = np.array(rec, dtype=LRA_DTYPE).reshape(1)
    return float(load_library().tlb_lra_lu(a.ctypes.data))


# tlb_truepeak_record: peaks in units of 2^-30 of full scale, dBTP = truepeak_dbtp(v); sample_max 0 .. 32768
TRUEPEAK_DTYPE = np.dtype([("frames", np.uint32), ("overs", np.uint32), ("peak", np.uint32, (2,)), ("peak_max", np.uint32, (2,)), ("sample_max", np.uint32, (2,))])
TRUEPEAK_TAPS = 12
TRUEPEAK_CEILING_DEFAULT = 956973408                                 # -1 dBTP: llround(2^30 * 10^(-1/20)), TLB_TRUEPEAK_CEILING_DEFAULT


# tlb_limiter_record: reductions as 65536 - G (0: unity), peaks in units of 2^-30 of full scale
# tlb_conceal_record: slots seen / passed / lost and synthesised from the last good frame / lost and left as zeros, loss runs begun, the longest
# one, the run now and the scalefactor-index offset of the last slot (CONCEAL_MUTE: beyond hold)
CONCEAL_DTYPE = np.dtype([(n, np.uint32) for n in ("frames", "passed", "concealed", "muted", "runs", "longest", "run", "offset")])
CONCEAL_MUTE = 0xFFFFFFFF
LIMITER_DTYPE = np.dtype([("frames", np.uint32), ("limited", np.uint32), ("samples", np.uint32), ("red_last", np.uint32), ("red_max", np.uint32),
                          ("peak_in", np.uint32), ("peak_in_max", np.uint32), ("reserved", np.uint32)])
LIMITER_DELAY = 63                                                   # samples the limited PCM is late, TLB_LIMITER_DELAY


def limiter_step(release_ms, samplerate):
    """the gain's recovery per sample in units of 2^-30, max(1, 2^30 * 1000 / (release_ms * samplerate)); 0 ms: the default 100 (tlb_limiter_step; no GPU)"""
    return int(load_library().tlb_limiter_step(int(release_ms), int(samplerate)))


def _limiter_params(ceiling, release_ms):
    return (C.c_uint32 * 2)(int(ceiling), int(release_ms))


def truepeak_dbtp(v):
    """20 log10(v / 2^30); -inf for 0 (tlb_truepeak_dbtp)"""
    return float(load_library().tlb_truepeak_dbtp(int(v)))


def truepeak_taps():
    """the committed interpolation table -> int16 [3][12]: the phases 1/4, 2/4, 3/4; no GPU"""
    out = np.zeros((3, TRUEPEAK_TAPS), dtype=np.int16)
    rc = load_library().tlb_truepeak_taps(out.ctypes.data)
    if rc:
        raise ToolameError(rc, "tlb_truepeak_taps")
    return out


def feed_check_config(cfg):
    """tlb_feed_check_config: 0, or the library's code for an illegal sample rate (1), channel count (2) or bitrate (4); host arithmetic, no GPU"""
    c = _c_feed(cfg)
    return load_library().tlb_feed_check_config(C.byref(c))


def feed_want_at(feed_rate, rate, tick):
    """tlb_feed_want_at: 1 / 0, is a feed frame of `feed_rate` wanted on tick `tick` (from the reset) of a stream at `rate`; host arithmetic, no GPU"""
    n = load_library().tlb_feed_want_at(feed_rate, rate, tick)
    if n < 0:
        raise ToolameError(-n, "tlb_feed_want_at")
    return n


def down_feed_want_at(feed_rate, rate, tick):
    """tlb_feed_down_want_at: 1 / 2, the feed frames of `feed_rate` wanted on tick `tick` (from the reset) of a stream at `rate` (24 kHz); host arithmetic, no GPU"""
    n = load_library().tlb_feed_down_want_at(feed_rate, rate, tick)
    if n < 0:
        raise ToolameError(-n, "tlb_feed_down_want_at")
    return n


def feed_frame_bytes(cfg):
    """bytes of a feed frame without its padding slot: host arithmetic, no GPU"""
    c = _c_feed(cfg)
    n = load_library().tlb_feed_frame_bytes(C.byref(c))
    if n < 0:
        raise ToolameError(-n, "tlb_feed_frame_bytes")
    return n


def lds_bytes_per_stream():
    return load_library().tlb_lds_bytes_per_stream()


def legacy_api():
    """The nine reference symbols (toolame_init ... toolame_encode_frame) as a ctypes library."""
    return load_library()


# mirror of tlb_edi_state (include/toolame_batch.h): the per-stream EDI sender state
EDI_STATE_DTYPE = np.dtype([("edi_time", np.int64), ("send_version_at_time", np.int64), ("timestamp", np.uint32),
                            ("num_seconds_sent", np.uint32), ("tai_utc_offset", np.int32), ("seq", np.uint16), ("dlfc", np.uint16),
                            ("tist", np.uint8), ("pad_", np.uint8, (7,))])


def edi_state_init(nstreams, now_s, delay_ms=0, tist=False, tai_utc_offset=37):
    """per-stream EDI sender state as EDI::write_frame sets it up on its first call (src/Outputs.cpp:200-212)"""
    st = np.zeros(nstreams, dtype=EDI_STATE_DTYPE)
    L = load_library()
    for s in range(nstreams):
        L.tlb_edi_state_init(st[s:s + 1].ctypes.data, int(now_s), int(delay_ms), 1 if tist else 0, int(tai_utc_offset))
    return st


# mirror of TlTaps (csrc/mp2_types.h) for stage-level parity tests
TAPS_DTYPE = np.dtype([
    ("sb_sample", np.float64, (2, 3, 12, 32)), ("smr", np.float64, (2, 32)), ("max_sc", np.float64, (2, 32)),
    ("subband", np.uint32, (2, 3, 12, 32)), ("scalar_pre", np.uint8, (2, 3, 32)), ("scalar", np.uint8, (2, 3, 32)),
    ("j_scale", np.uint8, (3, 32)), ("scfsi", np.uint8, (2, 32)), ("bit_alloc", np.uint8, (2, 32)),
    ("adb_left", np.int32), ("mode", np.int32), ("mode_ext", np.int32), ("jsbound", np.int32), ("crc16", np.int32),
    ("scfcrc", np.uint8, (4,)), ("pad_", np.int32, (2,)),
])


# tlb_frame_report / tlb_frame_fields (include/toolame_batch.h) and the status flags
FRAME_REPORT_DTYPE = np.dtype([("status", np.uint32), ("crc_stored", np.uint16), ("crc_computed", np.uint16), ("mode", np.uint8),
                               ("mode_ext", np.uint8), ("audio_bits", np.uint16)])
FRAME_FIELDS_DTYPE = np.dtype([("bit_alloc", np.uint8, (2, 32)), ("scfsi", np.uint8, (2, 32)), ("scalar", np.uint8, (2, 3, 32)),
                               ("subband", np.uint16, (2, 3, 12, 32))])
DEC_EMPTY, DEC_BAD_SYNC, DEC_HEADER_MISMATCH, DEC_BAD_CRC16, DEC_BAD_SCFCRC, DEC_SCFCRC_UNCHECKED, DEC_BAD_ALLOC, DEC_OVERRUN = (1 << i for i in range(8))
DEC_UNWANTED = 0x100                             # adapted feeds: the slot held bytes on a tick whose slot is not read
DEC_BAD_MASK = DEC_BAD_SYNC | DEC_HEADER_MISMATCH | DEC_BAD_CRC16 | DEC_BAD_SCFCRC | DEC_BAD_ALLOC | DEC_OVERRUN
# tlb_monitor_record (include/toolame_batch.h): the confidence monitor's fold, one per stream
MONITOR_DTYPE = np.dtype([("frames", np.uint32), ("bad_frames", np.uint32), ("bad_run", np.uint32), ("flags_seen", np.uint32),
                          ("last_status", np.uint32), ("out_silence_ms", np.uint32), ("out_peak", np.int16, (2,)), ("reserved_", np.uint32)])
MONITOR_WHAT = {"check": 1, "audio": 2}         # TLB_MONITOR_CHECK / TLB_MONITOR_AUDIO
# tlb_compare_record / tlb_compare_params (include/toolame_batch.h): the compare monitor, one record per stream
COMPARE_DTYPE = np.dtype([("sxx", np.int64, (2,)), ("syy", np.int64, (2,)), ("sxy", np.int64, (2,)), ("sxz", np.int64, (2,)),
                          ("frames_compared", np.uint32), ("frames_judged", np.uint32), ("mismatch_frames", np.uint32), ("mismatch_run", np.uint32),
                          ("swapped_frames", np.uint32), ("last_flags", np.uint32), ("reserved_", np.uint32, (2,))])
COMPARE_PARAMS_DTYPE = np.dtype([("min_energy", np.int64), ("corr_num", np.int32), ("corr_den", np.int32)])
COMPARE_DELAY = 481                             # TLB_COMPARE_DELAY
COMPARE_JUDGED0, COMPARE_JUDGED1, COMPARE_MISMATCH, COMPARE_SWAPPED, COMPARE_SKIPPED = (1 << i for i in range(5))
COMPARE_DEFAULTS = (1152 * 256 * 256, 3, 8)     # TLB_COMPARE_DEFAULT_MIN_ENERGY / _CORR_NUM / _CORR_DEN


def compare_params(params=None):
    """(min_energy, corr_num, corr_den), a dict with those keys, or None for the header's defaults -> COMPARE_PARAMS_DTYPE [1]"""
    if params is None:
        params = COMPARE_DEFAULTS
    if isinstance(params, dict):
        params = (params["min_energy"], params["corr_num"], params["corr_den"])
    out = np.zeros(1, dtype=COMPARE_PARAMS_DTYPE)
    out[0] = tuple(int(v) for v in params)
    return out


def _config_array(configs):
    arr = (_CConfig * len(configs))()
    for i, c in enumerate(configs):
        arr[i].samplerate = c.samplerate
        arr[i].mode = c.mode.encode()[:1]
        arr[i].bitrate = c.bitrate
        arr[i].psy_model = c.psy_model
        arr[i].pad_len = c.pad_len
    return arr


class _CTickConfig(C.Structure):
    _fields_ = [("egress", C.c_int), ("ngroups", C.c_int), ("with_xpad", C.c_int), ("version", C.c_char_p), ("version_len", C.c_int),
                ("now_s", C.c_longlong), ("delay_ms", C.c_uint), ("tist", C.c_int), ("tai_utc_offset", C.c_int),
                ("fec", C.c_int), ("chunk_len", C.c_int), ("transport", C.c_int), ("addr_source", C.c_int), ("dest_port", C.c_int)]


class Tick:
    """tlb_tick_*: the caller's loop body -- ingest, encode, EDI egress -- as one call per tick for every stream of a GPU
    (src/odr-audioenc.cpp:1030-1051,1139-1163,1208-1225, src/Outputs.cpp:194-261).  `pcm` (and `xpad`, `xpad_len`) are numpy
    views of the object's pinned host buffers: fill them, run(), read packets()."""
    EGRESS = {"frames": 0, "af": 1, "pft": 2, "zmq": 3}

    def __init__(self, configs, egress="af", ngroups=0, with_xpad=False, version=b"", now_s=1700000000, delay_ms=0, tist=False,
                 tai_utc_offset=37, fec=0, chunk_len=207, transport=False, addr_source=0, dest_port=0, device=0, lib=None):
        self.L = lib or load_library()
        configs = list(configs)
        self.nstreams = len(configs)
        self._version = bytes(version)
        tc = _CTickConfig(self.EGRESS[egress], ngroups, 1 if with_xpad else 0, self._version, len(self._version), int(now_s), int(delay_ms),
                          1 if tist else 0, int(tai_utc_offset), fec, chunk_len, 1 if transport else 0, addr_source, dest_port)
        err = C.c_int(0)
        self.h = self.L.tlb_tick_create(device, self.nstreams, _config_array(configs), C.byref(tc), C.byref(err))
        if not self.h:
            raise ToolameError(err.value, "tlb_tick_create")
        self.egress = egress
        n = self.nstreams
        self.with_xpad = bool(with_xpad)
        self.units = [self.L.tlb_tick_units(self.h, s) for s in range(n)]

    # The object owns TWO sets of pinned host buffers (tlb_tick_submit / tlb_tick_wait): `pcm`, `xpad`, `xpad_len` are views of the
    # input set to fill NEXT, `peaks`, `silence_ms` of the results of the tick waited for last -- fetched on every access.
    def _view(self, fn, ctype, shape):
        p = getattr(self.L, fn)(self.h)
        cnt = int(np.prod(shape))
        return np.ctypeslib.as_array((ctype * cnt).from_address(p)).reshape(shape) if p else None

    @property
    def pcm(self):
        return self._view("tlb_tick_pcm", C.c_int16, (self.nstreams, 2 * SAMPLES))

    @property
    def xpad(self):
        return self._view("tlb_tick_xpad", C.c_uint8, (self.nstreams, MAX_XPAD)) if self.with_xpad else None

    @property
    def xpad_len(self):
        return self._view("tlb_tick_xpad_len", C.c_int32, (self.nstreams,)) if self.with_xpad else None

    @property
    def peaks(self):
        return self._view("tlb_tick_peaks", C.c_int16, (self.nstreams, 2))

    @property
    def silence_ms(self):
        return self._view("tlb_tick_silence_ms", C.c_uint32, (self.nstreams,))

    # -- device resampler (tlb_tick_set_source): legal while no tick is in flight; excludes short reads --
    def set_source(self, source_rate, stream=-1):
        rc = self.L.tlb_tick_set_source(self.h, stream, int(source_rate))
        if rc:
            raise ToolameError(rc, "tlb_tick_set_source")

    def need(self, s):
        """source frames stream s's slot of `pcm` must hold for the next submit (1152 without a source)"""
        n = self.L.tlb_tick_need(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_tick_need")
        return n

    # -- down sources (tlb_tick_set_down_source): legal while no tick is in flight; exclude short reads, sources and feeds --
    def set_down_source(self, source_rate, stream=-1):
        rc = self.L.tlb_tick_set_down_source(self.h, stream, int(source_rate))
        if rc:
            raise ToolameError(rc, "tlb_tick_set_down_source")

    def down(self, s):
        """stream s's wide slot (int16 [4608] view) in the input set to fill next; None with two ticks in flight or without any down source"""
        p = self.L.tlb_tick_down(self.h, s)
        return np.ctypeslib.as_array((C.c_int16 * DECIMATE_SLOT).from_address(p)) if p else None

    def down_need(self, s):
        """source frames stream s's wide slot must hold for the next submit (1152 without a down source)"""
        n = self.L.tlb_tick_down_need(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_tick_down_need")
        return n

    # -- Layer II feeds (tlb_tick_set_feed): legal while no tick is in flight; exclude short reads and sources --
    def set_feed(self, stream, cfg, adapt=False):
        """stream = -1: every stream; cfg = None removes the feed.  `feed`, `feed_len` must be fetched again afterwards.
        adapt: tlb_tick_set_feed_adapted -- the feed may have another (legal) rate or channel count than the stream; see feed_want."""
        c = _c_feed(cfg) if cfg is not None else None
        rc = (self.L.tlb_tick_set_feed_adapted if adapt else self.L.tlb_tick_set_feed)(self.h, stream, C.byref(c) if c is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_tick_set_feed")

    def feed_want(self, s):
        """1 / 0: is a feed frame wanted in stream s's slot of the input set to fill next (always 1 for a strict feed)"""
        n = self.L.tlb_tick_feed_want(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_tick_feed_want")
        return n

    @property
    def feed_stride(self):
        return self.L.tlb_tick_feed_stride(self.h)

    @property
    def feed(self):
        """uint8 [nstreams, feed_stride] of the input set to fill next: a fed stream's frame; None when no feed is set or while two ticks are in flight"""
        return self._view("tlb_tick_feed", C.c_uint8, (self.nstreams, self.feed_stride)) if self.feed_stride else None

    @property
    def feed_len(self):
        """int32 [nstreams] of the input set to fill next: the frame's bytes, 0 (an empty slot) unless the caller writes more"""
        return self._view("tlb_tick_feed_len", C.c_int32, (self.nstreams,))

    @property
    def feed_report(self):
        """FRAME_REPORT_DTYPE [nstreams] of the tick waited for last; None when no feed is set"""
        p = self.L.tlb_tick_feed_report(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * FRAME_REPORT_DTYPE.itemsize)).from_address(p), dtype=FRAME_REPORT_DTYPE)

    # -- down feeds (tlb_tick_set_down_feed): legal while no tick is in flight; exclude short reads, sources, down sources and feeds --
    def set_down_feed(self, stream, cfg):
        """stream = -1: every stream; cfg = None removes the down feed.  `down_feed`, `down_feed_len` must be fetched again afterwards."""
        c = _c_feed(cfg) if cfg is not None else None
        rc = self.L.tlb_tick_set_down_feed(self.h, stream, C.byref(c) if c is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_tick_set_down_feed")

    def down_feed_want(self, s):
        """1 / 2: the feed frames wanted in stream s's two slots of the input set to fill next"""
        n = self.L.tlb_tick_down_feed_want(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_tick_down_feed_want")
        return n

    @property
    def down_feed_stride(self):
        return self.L.tlb_tick_down_feed_stride(self.h)

    @property
    def down_feed(self):
        """uint8 [nstreams, 2, down_feed_stride] of the input set to fill next; None when no down feed is set or while two ticks are in flight"""
        return self._view("tlb_tick_down_feed", C.c_uint8, (self.nstreams, 2, self.down_feed_stride)) if self.down_feed_stride else None

    @property
    def down_feed_len(self):
        """int32 [nstreams, 2] of the input set to fill next: the frames' bytes, 0 (an empty slot) unless the caller writes more"""
        return self._view("tlb_tick_down_feed_len", C.c_int32, (self.nstreams, 2)) if self.down_feed_stride else None

    @property
    def down_feed_report(self):
        """FRAME_REPORT_DTYPE [nstreams, 2] of the tick waited for last; None when no down feed is set"""
        p = self.L.tlb_tick_down_feed_report(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (2 * self.nstreams * FRAME_REPORT_DTYPE.itemsize)).from_address(p), dtype=FRAME_REPORT_DTYPE).reshape(self.nstreams, 2)

    # -- short reads (src/odr-audioenc.cpp:335-373,910-935): opt in before the first submit --
    def enable_short_reads(self):
        rc = self.L.tlb_tick_enable_short_reads(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_short_reads")

    @property
    def valid(self):
        """int32 [nstreams] of the input set to fill next: sample frames delivered, 1152 (a full read) unless the caller writes less;
        None when not enabled or while two ticks are in flight"""
        return self._view("tlb_tick_valid", C.c_int32, (self.nstreams,))

    @property
    def underrun_ms(self):
        """uint32 [nstreams]: milliseconds since the stream's last full read (the reference aborts above 60 s); None when not enabled"""
        return self._view("tlb_tick_underrun_ms", C.c_uint32, (self.nstreams,))

    @property
    def underruns(self):
        """uint32 [nstreams]: short reads so far; None when not enabled"""
        return self._view("tlb_tick_underruns", C.c_uint32, (self.nstreams,))

    # -- confidence monitor (tlb_decode_device + tlb_monitor_device behind every tick's egress): opt in before the first submit --
    def enable_monitor(self, what="audio"):
        """what: "check" (unpack and verify) or "audio" (also synthesise: out_peak, out_silence_ms, listen)"""
        rc = self.L.tlb_tick_enable_monitor(self.h, MONITOR_WHAT.get(what, what))
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_monitor")

    @property
    def monitor(self):
        """MONITOR_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when not enabled"""
        p = self.L.tlb_tick_monitor(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * MONITOR_DTYPE.itemsize)).from_address(p), dtype=MONITOR_DTYPE)

    # -- loudness meter (tlb_loudness_device on the tick's planar PCM): before the first submit --
    def enable_loudness(self):
        rc = self.L.tlb_tick_enable_loudness(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_loudness")

    @property
    def loudness(self):
        """LOUDNESS_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when not enabled"""
        p = self.L.tlb_tick_loudness(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * LOUDNESS_DTYPE.itemsize)).from_address(p), dtype=LOUDNESS_DTYPE)

    def loudness_programme(self):
        """LOUDNESS_PROGRAMME_DTYPE [nstreams] from the counts so far; with no tick in flight"""
        out = np.zeros(self.nstreams, dtype=LOUDNESS_PROGRAMME_DTYPE)
        rc = self.L.tlb_tick_loudness_programme(self.h, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_tick_loudness_programme")
        return out

    # -- loudness range (tlb_lra_*): after enable_loudness, before the first submit --
    def enable_lra(self):
        rc = self.L.tlb_tick_enable_lra(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_lra")
        return self

    def lra(self):
        """LRA_DTYPE [nstreams] from the range blocks so far; with no tick in flight"""
        out = np.zeros(self.nstreams, dtype=LRA_DTYPE)
        rc = self.L.tlb_tick_lra(self.h, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_tick_lra")
        return out

    def loudness_reset(self, s=-1):
        rc = self.L.tlb_tick_loudness_reset(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_tick_loudness_reset")

    # -- true-peak meter (tlb_truepeak_device on the tick's planar PCM): before the first submit --
    def enable_truepeak(self, ceiling=0):
        """ceiling in units of 2^-30 of full scale; 0: TRUEPEAK_CEILING_DEFAULT (-1 dBTP)"""
        rc = self.L.tlb_tick_enable_truepeak(self.h, int(ceiling))
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_truepeak")

    @property
    def truepeak(self):
        """TRUEPEAK_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when not enabled"""
        p = self.L.tlb_tick_truepeak(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * TRUEPEAK_DTYPE.itemsize)).from_address(p), dtype=TRUEPEAK_DTYPE)

    def truepeak_reset(self, s=-1):
        rc = self.L.tlb_tick_truepeak_reset(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_tick_truepeak_reset")

    # -- feed concealment (tlb_conceal_* of the groups' batches): per stream, while no tick is in flight --
    def enable_conceal(self, hold=4, step=3, stream=-1, any_feed=False):
        """a lost feed frame repeats the last good one, `step` scalefactor-index units (3: 6 dB) quieter per lost frame, for `hold` frames,
        then rings out; hold 0 switches it off.  stream -1: every stream (each needs a strict feed; any_feed: a feed of any kind, adapted
        and down feeds included: tlb_tick_enable_feed_loss)"""
        name = "tlb_tick_enable_feed_loss" if any_feed else "tlb_tick_enable_conceal"
        rc = getattr(self.L, name)(self.h, int(stream), int(hold), int(step))
        if rc:
            raise ToolameError(rc, name)

    def conceal(self):
        """CONCEAL_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when never enabled"""
        p = self.L.tlb_tick_conceal(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * CONCEAL_DTYPE.itemsize)).from_address(p), dtype=CONCEAL_DTYPE)

    def conceal_reset(self, s=-1):
        rc = self.L.tlb_tick_conceal_reset(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_tick_conceal_reset")

    # -- true-peak limiter (tlb_limiter_device on the tick's planar PCM, between the ingest and the encoder): before the first submit --
    def enable_limiter(self, ceiling=0, release_ms=0):
        """ceiling in units of 2^-30 of full scale, 0: TRUEPEAK_CEILING_DEFAULT (-1 dBTP); release_ms 0: 100"""
        rc = self.L.tlb_tick_enable_limiter(self.h, _limiter_params(ceiling, release_ms))
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_limiter")

    @property
    def limiter(self):
        """LIMITER_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when not enabled"""
        p = self.L.tlb_tick_limiter(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * LIMITER_DTYPE.itemsize)).from_address(p), dtype=LIMITER_DTYPE)

    def limiter_reset(self, s=-1):
        rc = self.L.tlb_tick_limiter_reset(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_tick_limiter_reset")

    # -- compare monitor (tlb_compare_device behind the decode): after enable_monitor("audio"), before the first submit --
    def enable_compare(self, params=None):
        """params: (min_energy, corr_num, corr_den) or None for the defaults"""
        rc = self.L.tlb_tick_enable_compare(self.h, compare_params(params).ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_tick_enable_compare")

    @property
    def compare(self):
        """COMPARE_DTYPE [nstreams] of the tick waited for last (a view of the object's pinned memory); None when not enabled"""
        p = self.L.tlb_tick_compare(self.h)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (self.nstreams * COMPARE_DTYPE.itemsize)).from_address(p), dtype=COMPARE_DTYPE)

    def monitor_listen(self, s):
        """select ONE stream (-1: none) whose decoded frame comes back with every tick from the next submit on ("audio" only)"""
        rc = self.L.tlb_tick_monitor_listen(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_tick_monitor_listen")

    def monitor_pcm(self):
        """(stream, int16 [2][1152] view) of the tick waited for last, or (-1, None) when that tick carried none"""
        s = C.c_int(-1)
        p = self.L.tlb_tick_monitor_pcm(self.h, C.byref(s))
        if not p:
            return -1, None
        return s.value, np.ctypeslib.as_array((C.c_int16 * (2 * SAMPLES)).from_address(p)).reshape(2, SAMPLES)

    def damage_next(self, stream, byte, xor_mask, nth=1):
        """fault-injection TEST build only: the nth submit from now XORs one byte of that stream's frame on the device, ahead of egress and monitor"""
        rc = self.L.tlb_debug_tick_damage_next(self.h, stream, byte, xor_mask, nth)
        if rc:
            raise ToolameError(rc, "tlb_debug_tick_damage_next")

    def cross_from(self, a, b, nth=1):
        """fault-injection TEST build only: from the nth submit from now on the frames of streams a and b (one group) leave in each other's slots"""
        rc = self.L.tlb_debug_tick_cross_from(self.h, a, b, nth)
        if rc:
            raise ToolameError(rc, "tlb_debug_tick_cross_from")

    def submit(self):
        """queue one tick on the input set just filled and return at once; `pcm` then shows the other input set"""
        rc = self.L.tlb_tick_submit(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_submit")

    def wait(self):
        """wait for the oldest submitted tick; frame() / packets() / peaks ... then show its results"""
        rc = self.L.tlb_tick_wait(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_wait")

    def set_gain_db(self, gain_db, stream=-1):
        rc = self.L.tlb_tick_set_gain_db(self.h, stream, float(gain_db))
        if rc:
            raise ToolameError(rc, "tlb_tick_set_gain_db")

    # -- life cycle of one stream between two runs (toolame_init / toolame_finish / the setters, per stream) --
    def stream_reset(self, s):
        rc = self.L.tlb_tick_stream_reset(self.h, s)
        if rc:
            raise ToolameError(rc, "tlb_tick_stream_reset")

    def stream_finish(self, s):
        buf = (C.c_uint8 * 2048)()
        n = self.L.tlb_tick_stream_finish(self.h, s, buf, 2048)
        if n < 0:
            raise ToolameError(-n, "tlb_tick_stream_finish")
        return bytes(buf[:n])

    def stream_reconfigure(self, s, config):
        rc = self.L.tlb_tick_stream_reconfigure(self.h, s, _config_array([config]))
        if rc:
            raise ToolameError(rc, "tlb_tick_stream_reconfigure")
        self.units[s] = self.L.tlb_tick_units(self.h, s)

    def status(self):
        """0, or 17 (TLB_ERR_HIP) once a device failure has left the object out of step with itself (sticky: destroy it)"""
        return self.L.tlb_tick_status(self.h)

    def fail_next(self, nth=1):
        """fault-injection TEST build only (lib=load_fault_library()): the nth submit from now fails in its last stream group"""
        return self.L.tlb_debug_tick_fail_next(self.h, nth)

    def run(self):
        rc = self.L.tlb_tick_run(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_run")

    def finish(self):
        rc = self.L.tlb_tick_finish(self.h)
        if rc:
            raise ToolameError(rc, "tlb_tick_finish")

    def last_ms(self):
        return float(self.L.tlb_tick_last_ms(self.h))

    def frame(self, s):
        n = C.c_int(0)
        p = self.L.tlb_tick_frame(self.h, s, C.byref(n))
        return C.string_at(p, n.value) if p and n.value else b""

    def packets(self, s):
        """the AF packets of stream s from the last run, one per unit (empty list: none this tick)"""
        out = []
        for u in range(self.units[s]):
            n = C.c_int(0)
            p = self.L.tlb_tick_packet(self.h, s, u, C.byref(n))
            if p and n.value:
                out.append(C.string_at(p, n.value))
        return out

    def messages(self, s):
        """the ZeroMQ messages (header + unit) of stream s from the last run"""
        out = []
        for u in range(self.units[s]):
            n = C.c_int(0)
            p = self.L.tlb_tick_message(self.h, s, u, C.byref(n))
            if p and n.value:
                out.append(C.string_at(p, n.value))
        return out

    def fragments(self, s):
        """per unit: the list of PFT fragments of stream s from the last run"""
        out = []
        for u in range(self.units[s]):
            fr = []
            for k in range(self.L.tlb_tick_fragments(self.h, s, u)):
                n = C.c_int(0)
                p = self.L.tlb_tick_fragment(self.h, s, u, k, C.byref(n))
                fr.append(C.string_at(p, n.value))
            if fr:
                out.append(fr)
        return out

    def close(self):
        if getattr(self, "h", None):
            self.L.tlb_tick_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Batch:
    """N independent DAB MP2 encoders on one MI355X (one wavefront per stream)."""

    def __init__(self, configs, device=0, lib=None):
        self.L = lib or load_library()
        configs = list(configs)
        if not configs:
            raise ToolameError(18, "empty batch")
        arr = _config_array(configs)
        err = C.c_int(0)
        self.h = self.L.tlb_create(device, len(configs), arr, C.byref(err))
        if not self.h:
            raise ToolameError(err.value, "tlb_create")
        self.device = device
        self.nstreams = len(configs)
        self.configs = configs
        self.frame_bytes = [self.L.tlb_frame_bytes(self.h, s) for s in range(self.nstreams)]
        self.out_stride = self.L.tlb_out_stride(self.h)
        self.unit_bytes = [self.L.tlb_egress_unit_bytes(self.h, s) for s in range(self.nstreams)]
        self.units_per_frame = [self.L.tlb_egress_units_per_frame(self.h, s) for s in range(self.nstreams)]
        self.max_upf = self.L.tlb_egress_max_units_per_frame(self.h)
        self._first = True

    def fail_next(self, nth=1):
        """fault-injection TEST build only (lib=load_fault_library()): the nth launch from now fails half way (csrc/tlb_debug.h)"""
        return self.L.tlb_debug_fail_next(self.h, nth)

    # -- host-buffer path (tests, legacy-style callers) ------------------------------------
    def encode(self, pcm, xpad=None, xpad_len=None, want_taps=False):
        """pcm int16 [nframes, nstreams, 2, 1152] -> (per stream: bytes of the frames that became
        final during this call, taps [nframes, nstreams] or None).  One frame of latency, see
        include/toolame_batch.h."""
        pcm = np.ascontiguousarray(pcm, dtype=np.int16)
        nf = pcm.shape[0]
        if pcm.shape != (nf, self.nstreams, 2, SAMPLES):
            raise ToolameError(18, f"pcm shape {pcm.shape}")
        out = np.zeros((nf, self.nstreams, self.out_stride), dtype=np.uint8)
        taps = np.zeros((nf, self.nstreams), dtype=TAPS_DTYPE) if want_taps else None
        xp = xl = None
        if xpad is not None:
            xp = np.ascontiguousarray(xpad, dtype=np.uint8)
            xl = np.ascontiguousarray(xpad_len, dtype=np.int32)
            if xp.shape != (nf, self.nstreams, MAX_XPAD) or xl.shape != (nf, self.nstreams):
                raise ToolameError(18, "xpad shape")
        lens = np.zeros((nf, self.nstreams), dtype=np.int32)
        rc = self.L.tlb_encode_host_len(self.h, pcm.ctypes.data, nf, xp.ctypes.data if xp is not None else None,
                                        xl.ctypes.data if xl is not None else None, out.ctypes.data, lens.ctypes.data,
                                        taps.ctypes.data if taps is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_encode_host_len")
        self._first = False
        # a slot's length: 0 for slot 0 of the very first call (no frame yet); frame_bytes, or one more at 44.1 / 22.05 kHz
        res = [b"".join(out[f, s, : lens[f, s]].tobytes() for f in range(nf)) for s in range(self.nstreams)]
        return res, taps

    def flush(self):
        """toolame_finish(): the last (pending) frame of every stream, carrying its own ScF-CRC."""
        out = np.zeros((self.nstreams, self.out_stride), dtype=np.uint8)
        lens = np.zeros(self.nstreams, dtype=np.int32)
        rc = self.L.tlb_flush_host_len(self.h, out.ctypes.data, lens.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_flush_host_len")
        return [out[s, : lens[s]].tobytes() for s in range(self.nstreams)]

    def reset(self):
        rc = self.L.tlb_reset(self.h)
        if rc:
            raise ToolameError(rc, "tlb_reset")

    # -- life cycle of one stream inside the live batch (toolame.c:120-166 per stream) --------
    def stream_reset(self, s):
        """toolame_init() for stream s alone: its next frame is its frame 0; no other stream notices"""
        rc = self.L.tlb_stream_reset(self.h, s)
        if rc:
            raise ToolameError(rc, "tlb_stream_reset")

    def stream_finish(self, s):
        """toolame_finish() for stream s alone: its pending frame (bytes), then as after stream_reset()"""
        buf = (C.c_uint8 * 2048)()
        n = self.L.tlb_stream_finish(self.h, s, buf, 2048)
        if n < 0:
            raise ToolameError(-n, "tlb_stream_finish")
        return bytes(buf[:n])

    def stream_reconfigure(self, s, config):
        """the six setters + toolame_init() for stream s alone"""
        rc = self.L.tlb_stream_reconfigure(self.h, s, _config_array([config]))
        if rc:
            raise ToolameError(rc, "tlb_stream_reconfigure")
        self.configs[s] = config
        self.frame_bytes[s] = self.L.tlb_frame_bytes(self.h, s)
        self.unit_bytes[s] = self.L.tlb_egress_unit_bytes(self.h, s)
        self.units_per_frame[s] = self.L.tlb_egress_units_per_frame(self.h, s)

    # -- frame check / decode: the batch's own frames read back (tlb_decode_*) ----------------
    def decode(self, frames, lens=None, want_fields=False, want_pcm=False):
        """frames uint8 [nframes, nstreams, out_stride], lens int32 [nframes, nstreams] or None (every slot full) ->
        (reports FRAME_REPORT_DTYPE [nframes, nstreams], fields FRAME_FIELDS_DTYPE [nframes, nstreams] or None,
        pcm int16 [nframes, nstreams, 2, 1152] or None)"""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        if frames.shape != (nf, self.nstreams, self.out_stride):
            raise ToolameError(18, f"frames shape {frames.shape}")
        ln = None
        if lens is not None:
            ln = np.ascontiguousarray(lens, dtype=np.int32)
            if ln.shape != (nf, self.nstreams):
                raise ToolameError(18, "lens shape")
        rep = np.zeros((nf, self.nstreams), dtype=FRAME_REPORT_DTYPE)
        fl = np.zeros((nf, self.nstreams), dtype=FRAME_FIELDS_DTYPE) if want_fields else None
        pcm = np.zeros((nf, self.nstreams, 2, SAMPLES), dtype=np.int16) if want_pcm else None
        rc = self.L.tlb_decode_host(self.h, frames.ctypes.data, ln.ctypes.data if ln is not None else None, nf, rep.ctypes.data,
                                    fl.ctypes.data if fl is not None else None, pcm.ctypes.data if pcm is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_decode_host")
        return rep, fl, pcm

    # -- Layer II feeds: a stream's source arrives as MP2 frames and is decoded into the ingest's input (tlb_feed_*) --
    def set_feed(self, stream, cfg, adapt=False):
        """stream = -1: every stream; cfg = None removes the feed.  The feed's rate and channel count must be the stream's, unless
        adapt: tlb_feed_set_adapted -- a legal rate pair (equal, 44.1 -> 48, 22.05 -> 24, 32 -> 48, 16 -> 24 kHz) and 1 or 2 channels on either side."""
        c = _c_feed(cfg) if cfg is not None else None
        rc = (self.L.tlb_feed_set_adapted if adapt else self.L.tlb_feed_set)(self.h, stream, C.byref(c) if c is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_feed_set")

    def get_feed(self, stream):
        c = _CFeedConfig()
        n = self.L.tlb_feed_get(self.h, stream, C.byref(c))
        if n < 0:
            raise ToolameError(-n, "tlb_feed_get")
        return FeedConfig(c.samplerate, c.bitrate, c.channels) if n else None

    def feed_adapted(self, s):
        n = self.L.tlb_feed_adapted(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_feed_adapted")
        return bool(n)

    def feed_want(self, s, ahead=0):
        """1 / 0: is a feed frame wanted on stream s's (ahead)-th next tick (always 1 for a strict feed); host arithmetic"""
        n = self.L.tlb_feed_want(self.h, s, ahead)
        if n < 0:
            raise ToolameError(-n, "tlb_feed_want")
        return n

    @property
    def feed_stride(self):
        """bytes per slot of feed(): it changes with set_feed"""
        return self.L.tlb_feed_stride(self.h)

    def feed_reset(self, stream=-1):
        rc = self.L.tlb_feed_reset(self.h, stream)
        if rc:
            raise ToolameError(rc, "tlb_feed_reset")

    def feed(self, frames, lens, interleaved=None):
        """frames uint8 [nframes, nstreams, feed_stride], lens int32 [nframes, nstreams] (0: an empty slot) ->
        (interleaved int16 [nframes, nstreams, 2304] as ingest() takes it, reports FRAME_REPORT_DTYPE [nframes, nstreams]).
        `interleaved`: the PCM of the streams WITHOUT a feed, whose slots the call does not touch (None: zeros); it is not changed, a copy is returned."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        if frames.shape != (nf, self.nstreams, self.feed_stride):
            raise ToolameError(18, f"frames shape {frames.shape}")
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        if ln.shape != (nf, self.nstreams):
            raise ToolameError(18, "lens shape")
        if interleaved is None:
            out = np.zeros((nf, self.nstreams, 2 * SAMPLES), dtype=np.int16)
        else:
            out = np.array(interleaved, dtype=np.int16, order="C", copy=True)
            if out.shape != (nf, self.nstreams, 2 * SAMPLES):
                raise ToolameError(18, f"interleaved shape {out.shape}")
        rep = np.zeros((nf, self.nstreams), dtype=FRAME_REPORT_DTYPE)
        rc = self.L.tlb_feed_host(self.h, frames.ctypes.data, ln.ctypes.data, nf, out.ctypes.data, rep.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_feed_host")
        return out, rep

    def feed_device(self, d_frames_ptr, d_len_ptr, nframes, d_interleaved_ptr, d_report_ptr=None, stream=None):
        rc = self.L.tlb_feed_device(self.h, d_frames_ptr, d_len_ptr, nframes, d_interleaved_ptr, d_report_ptr, stream)
        if rc:
            raise ToolameError(rc, "tlb_feed_device")

    # -- feed concealment (tlb_conceal_*): a lost frame of a strict feed is the last good one once more, quieter, and not silence --
    def enable_conceal(self, hold=4, step=3, stream=-1, any_feed=False):
        """hold 1..16 frames, step 1..21 scalefactor-index units per lost frame (3: 6 dB); hold 0 switches it off.  stream -1: every stream,
        each of which needs a strict feed (checked before anything changes).  feed() then conceals by itself.  any_feed: a feed of any
        kind will do (tlb_feed_loss_enable): an adapted or a down feed's lost WANTED slots are concealed ahead of the resampler or
        decimator, by feed() and down_feed() themselves."""
        name = "tlb_feed_loss_enable" if any_feed else "tlb_conceal_enable"
        rc = getattr(self.L, name)(self.h, int(stream), int(hold), int(step))
        if rc:
            raise ToolameError(rc, name)

    def conceal_cfg(self, s):
        """(hold, step) of stream s, None when its concealment is off"""
        hold, step = C.c_int(0), C.c_int(0)
        n = self.L.tlb_conceal_get(self.h, int(s), C.byref(hold), C.byref(step))
        if n < 0:
            raise ToolameError(-n, "tlb_conceal_get")
        return (hold.value, step.value) if n else None

    def conceal_records(self):
        """CONCEAL_DTYPE [nstreams] after the feed calls so far (waits for the device)"""
        out = np.zeros(self.nstreams, dtype=CONCEAL_DTYPE)
        rc = self.L.tlb_conceal_records_host(self.h, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_conceal_records_host")
        return out

    def conceal_reset(self, s=-1):
        """forget the last good frame, the run and the record of stream s (-1: all); the parameters stay"""
        rc = self.L.tlb_conceal_reset(self.h, int(s))
        if rc:
            raise ToolameError(rc, "tlb_conceal_reset")

    # -- down feeds: a 48, 44.1 or 32 kHz Layer II feed for a 24 kHz stream, decoded and decimated into the ingest's input (tlb_feed_down_*) --
    def set_down_feed(self, stream, cfg):
        """stream = -1: every stream; cfg = None removes the down feed.  Legal pairs: 48 / 44.1 / 32 kHz -> 24 kHz, 1 or 2 channels on either
        side; a stream that has a feed, a source or a down source is refused (a stream has one source)."""
        c = _c_feed(cfg) if cfg is not None else None
        rc = self.L.tlb_feed_down_set(self.h, stream, C.byref(c) if c is not None else None)
        if rc:
            raise ToolameError(rc, "tlb_feed_down_set")

    def down_feed_cfg(self, stream):
        c = _CFeedConfig()
        n = self.L.tlb_feed_down_get(self.h, stream, C.byref(c))
        if n < 0:
            raise ToolameError(-n, "tlb_feed_down_get")
        return FeedConfig(c.samplerate, c.bitrate, c.channels) if n else None

    def down_feed_want(self, s, ahead=0):
        """1 / 2: the feed frames wanted on stream s's (ahead)-th next tick; host arithmetic"""
        n = self.L.tlb_feed_down_want(self.h, s, ahead)
        if n < 0:
            raise ToolameError(-n, "tlb_feed_down_want")
        return n

    @property
    def down_feed_stride(self):
        """bytes per slot of down_feed(): it changes with set_down_feed"""
        return self.L.tlb_feed_down_stride(self.h)

    def down_feed_reset(self, stream=-1):
        rc = self.L.tlb_feed_down_reset(self.h, stream)
        if rc:
            raise ToolameError(rc, "tlb_feed_down_reset")

    def down_feed(self, frames, lens, interleaved=None):
        """frames uint8 [nframes, nstreams, 2, down_feed_stride], lens int32 [nframes, nstreams, 2] (0: an empty slot; slot 1 is read on a
        tick that wants two frames) -> (interleaved int16 [nframes, nstreams, 2304] as ingest() takes it, reports FRAME_REPORT_DTYPE
        [nframes, nstreams, 2]).  `interleaved`: the PCM of the streams WITHOUT a down feed, whose slots the call does not touch (None:
        zeros); it is not changed, a copy is returned."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = frames.shape[0]
        if frames.shape != (nf, self.nstreams, 2, self.down_feed_stride):
            raise ToolameError(18, f"frames shape {frames.shape}")
        ln = np.ascontiguousarray(lens, dtype=np.int32)
        if ln.shape != (nf, self.nstreams, 2):
            raise ToolameError(18, "lens shape")
        if interleaved is None:
            out = np.zeros((nf, self.nstreams, 2 * SAMPLES), dtype=np.int16)
        else:
            out = np.array(interleaved, dtype=np.int16, order="C", copy=True)
            if out.shape != (nf, self.nstreams, 2 * SAMPLES):
                raise ToolameError(18, f"interleaved shape {out.shape}")
        rep = np.zeros((nf, self.nstreams, 2), dtype=FRAME_REPORT_DTYPE)
        rc = self.L.tlb_feed_down_host(self.h, frames.ctypes.data, ln.ctypes.data, out.ctypes.data, rep.ctypes.data, nf)
        if rc:
            raise ToolameError(rc, "tlb_feed_down_host")
        return out, rep

    def down_feed_device(self, d_frames_ptr, d_len_ptr, d_interleaved_ptr, nframes, d_report_ptr=None, stream=None):
        rc = self.L.tlb_feed_down_device(self.h, d_frames_ptr, d_len_ptr, d_interleaved_ptr, d_report_ptr, nframes, stream)
        if rc:
            raise ToolameError(rc, "tlb_feed_down_device")

    def monitor(self, report, pcm=None, record=None):
        """tlb_monitor_host: fold reports FRAME_REPORT_DTYPE [nframes, nstreams] (and the decoded pcm int16 [nframes, nstreams, 2, 1152] or
        None) into record MONITOR_DTYPE [nstreams] -- advanced in place when given, else a fresh all-zero one -- and return it"""
        rep = np.ascontiguousarray(report, dtype=FRAME_REPORT_DTYPE)
        if rep.ndim != 2 or rep.shape[1] != self.nstreams:
            raise ToolameError(18, f"report shape {rep.shape}")
        nf = rep.shape[0]
        pc = None
        if pcm is not None:
            pc = np.ascontiguousarray(pcm, dtype=np.int16)
            if pc.shape != (nf, self.nstreams, 2, SAMPLES):
                raise ToolameError(18, f"pcm shape {pc.shape}")
        if record is None:
            record = np.zeros(self.nstreams, dtype=MONITOR_DTYPE)
        if record.dtype != MONITOR_DTYPE or record.shape != (self.nstreams,) or not record.flags.c_contiguous:
            raise ToolameError(18, "record: MONITOR_DTYPE [nstreams]")
        rc = self.L.tlb_monitor_host(self.h, rep.ctypes.data, pc.ctypes.data if pc is not None else None, nf, record.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_monitor_host")
        return record

    def compare(self, in_pcm, dec_pcm, report, params=None, record=None):
        """tlb_compare_host: the encoder's input in_pcm int16 [nframes, nstreams, 2, 1152] (None: the flush, one slot, the history does not
        advance) against the decoded dec_pcm of the same call's output slots and their reports, into record COMPARE_DTYPE [nstreams] --
        advanced in place when given, else a fresh all-zero one -- which is returned.  params: (min_energy, corr_num, corr_den) or None"""
        rep = np.ascontiguousarray(report, dtype=FRAME_REPORT_DTYPE)
        if rep.ndim != 2 or rep.shape[1] != self.nstreams:
            raise ToolameError(18, f"report shape {rep.shape}")
        nf = rep.shape[0]
        dec = np.ascontiguousarray(dec_pcm, dtype=np.int16)
        inp = None if in_pcm is None else np.ascontiguousarray(in_pcm, dtype=np.int16)
        if dec.shape != (nf, self.nstreams, 2, SAMPLES) or (inp is not None and inp.shape != dec.shape):
            raise ToolameError(18, f"pcm shape {dec.shape}")
        if record is None:
            record = np.zeros(self.nstreams, dtype=COMPARE_DTYPE)
        if record.dtype != COMPARE_DTYPE or record.shape != (self.nstreams,) or not record.flags.c_contiguous:
            raise ToolameError(18, "record: COMPARE_DTYPE [nstreams]")
        rc = self.L.tlb_compare_host(self.h, inp.ctypes.data if inp is not None else None, dec.ctypes.data, rep.ctypes.data, nf,
                                     compare_params(params).ctypes.data, record.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_compare_host")
        return record

    def compare_reset(self, stream=-1):
        rc = self.L.tlb_compare_reset(self.h, stream)
        if rc:
            raise ToolameError(rc, "tlb_compare_reset")

    def decode_device(self, d_frames_ptr, d_len_ptr, nframes, d_report_ptr, d_fields_ptr=None, d_pcm_ptr=None, stream=None):
        rc = self.L.tlb_decode_device(self.h, d_frames_ptr, d_len_ptr, nframes, d_report_ptr, d_fields_ptr, d_pcm_ptr, stream)
        if rc:
            raise ToolameError(rc, "tlb_decode_device")

    def decode_reset(self, stream=-1):
        rc = self.L.tlb_decode_reset(self.h, stream)
        if rc:
            raise ToolameError(rc, "tlb_decode_reset")

    def decode_bad_frames(self):
        n = self.L.tlb_decode_bad_frames(self.h)
        if n < 0:
            raise ToolameError(-n, "tlb_decode_bad_frames")
        return int(n)

    # -- device-resident path (bench, production) -------------------------------------------
    def encode_device(self, d_pcm_ptr, nframes, d_out_ptr, d_xpad_ptr=None, d_xpad_len_ptr=None, stream=None):
        rc = self.L.tlb_encode_device(self.h, d_pcm_ptr, nframes, d_xpad_ptr, d_xpad_len_ptr, d_out_ptr, stream)
        if rc:
            raise ToolameError(rc, "tlb_encode_device")
        self._first = False

    def flush_device(self, d_out_ptr, stream=None):
        rc = self.L.tlb_flush_device(self.h, d_out_ptr, stream)
        if rc:
            raise ToolameError(rc, "tlb_flush_device")

    # -- caller-side glue (gain, peak, de-interleave; src/odr-audioenc.cpp:1030-1051,1139-1152) ----
    def set_gain_db(self, gain_db, stream=-1):
        rc = self.L.tlb_set_gain_db(self.h, stream, float(gain_db))
        if rc:
            raise ToolameError(rc, "tlb_set_gain_db")

    # -- device resampler (tlb_resample_*): 44.1 / 22.05 kHz (160/147) and 32 / 16 kHz (3/2) sources to the encoder's rate --
    def set_source(self, source_rate, stream=-1):
        """0 or the stream's own rate: off; waits for queued launches and zeroes the resampler state of the streams it names"""
        rc = self.L.tlb_resample_set_source(self.h, stream, int(source_rate))
        if rc:
            raise ToolameError(rc, "tlb_resample_set_source")

    def source(self, s):
        return int(self.L.tlb_resample_source(self.h, s))

    def need(self, s, ahead=0):
        n = self.L.tlb_resample_need(self.h, s, ahead)
        if n < 0:
            raise ToolameError(-n, "tlb_resample_need")
        return n

    def resample(self, source, out=None):
        """int16 [nframes, nstreams, 2304], each slot holding need() source frames at its start -> the same shape at the encoder's rate,
        what ingest() takes.  out: the array to write into (values the kernel does not write keep what it held); None: zeros"""
        a = np.ascontiguousarray(source, dtype=np.int16)
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, 2 * SAMPLES):
            raise ToolameError(18, f"source shape {a.shape}")
        if out is None:
            out = np.zeros_like(a)
        if out.dtype != np.int16 or out.shape != a.shape or not out.flags.c_contiguous:
            raise ToolameError(18, "out array")
        rc = self.L.tlb_resample_host(self.h, a.ctypes.data, nf, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_resample_host")
        return out

    # -- device decimator (tlb_decimate_*): 48 (1/2), 32 (3/4) and 44.1 kHz (80/147) sources for a 24 kHz stream --
    def set_down_source(self, source_rate, stream=-1):
        """0 or the stream's own rate: off; waits for queued launches and zeroes the decimator state of the streams it names"""
        rc = self.L.tlb_decimate_set_source(self.h, stream, int(source_rate))
        if rc:
            raise ToolameError(rc, "tlb_decimate_set_source")

    def down_source(self, s):
        return int(self.L.tlb_decimate_source(self.h, s))

    def down_need(self, s, ahead=0):
        n = self.L.tlb_decimate_need(self.h, s, ahead)
        if n < 0:
            raise ToolameError(-n, "tlb_decimate_need")
        return n

    def decimate(self, wide, out=None):
        """int16 [nframes, nstreams, 4608], each slot of a stream with a down source holding down_need() source frames at its start ->
        int16 [nframes, nstreams, 2304] at the encoder's rate, what ingest() takes.  out: the array to write into (the slots of streams
        without a down source and whatever else the kernel does not write keep what it held); None: zeros"""
        a = np.ascontiguousarray(wide, dtype=np.int16)
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, DECIMATE_SLOT):
            raise ToolameError(18, f"wide shape {a.shape}")
        if out is None:
            out = np.zeros((nf, self.nstreams, 2 * SAMPLES), dtype=np.int16)
        if out.dtype != np.int16 or out.shape != (nf, self.nstreams, 2 * SAMPLES) or not out.flags.c_contiguous:
            raise ToolameError(18, "out array")
        rc = self.L.tlb_decimate_host(self.h, a.ctypes.data, nf, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_decimate_host")
        return out

    # -- loudness meter (tlb_loudness_*): momentary, short-term and gated programme loudness of the PCM the encoder is given --
    def enable_loudness(self):
        """allocates the meter's state on the device (about 3.4 KB per stream); a second call does nothing"""
        rc = self.L.tlb_loudness_enable(self.h)
        if rc:
            raise ToolameError(rc, "tlb_loudness_enable")

    def loudness(self, pcm_planar):
        """int16 [nframes, nstreams, 2, 1152] planar PCM as ingest() returns it -> LOUDNESS_DTYPE [nstreams] after these frames"""
        a = np.ascontiguousarray(pcm_planar, dtype=np.int16)
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, 2, SAMPLES):
            raise ToolameError(18, f"pcm shape {a.shape}")
        out = np.zeros(self.nstreams, dtype=LOUDNESS_DTYPE)
        rc = self.L.tlb_loudness_host(self.h, a.ctypes.data, nf, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_loudness_host")
        return out

    def loudness_programme(self):
        """LOUDNESS_PROGRAMME_DTYPE [nstreams]: gated programme loudness of everything measured since the streams' resets"""
        out = np.zeros(self.nstreams, dtype=LOUDNESS_PROGRAMME_DTYPE)
        rc = self.L.tlb_loudness_programme_host(self.h, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_loudness_programme_host")
        return out

    def loudness_reset(self, s=-1):
        """EBU mode's reset of one stream, or of every stream (-1)"""
        rc = self.L.tlb_loudness_reset(self.h, s)
        if rc:
            raise ToolameError(rc, "tlb_loudness_reset")

    # -- loudness range (tlb_lra_*): EBU Tech 3342's LRA from the meter's short-term values --
    def enable_lra(self):
        """after enable_loudness: allocates the range-block counts on the device (3008 bytes per stream); from here on loudness() counts
        range blocks too; a second call does nothing"""
        rc = self.L.tlb_lra_enable(self.h)
        if rc:
            raise ToolameError(rc, "tlb_lra_enable")

    def lra(self):
        """LRA_DTYPE [nstreams]: loudness range of everything measured since the streams' resets (LU: lra_lu)"""
        out = np.zeros(self.nstreams, dtype=LRA_DTYPE)
        rc = self.L.tlb_lra_host(self.h, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_lra_host")
        return out

    # -- true-peak meter (tlb_truepeak_*): the 4x oversampled maximum of the PCM the encoder is given --
    def enable_truepeak(self, ceiling=0):
        """allocates the meter's state on the device (80 bytes per stream); ceiling in units of 2^-30 of full scale, 0: -1 dBTP; a second
        call does nothing and leaves the ceiling"""
        rc = self.L.tlb_truepeak_enable(self.h, int(ceiling))
        if rc:
            raise ToolameError(rc, "tlb_truepeak_enable")

    def truepeak(self, pcm_planar):
        """int16 [nframes, nstreams, 2, 1152] planar PCM as ingest() returns it -> TRUEPEAK_DTYPE [nstreams] after these frames"""
        a = np.ascontiguousarray(pcm_planar, dtype=np.int16)
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, 2, SAMPLES):
            raise ToolameError(18, f"pcm shape {a.shape}")
        out = np.zeros(self.nstreams, dtype=TRUEPEAK_DTYPE)
        rc = self.L.tlb_truepeak_host(self.h, a.ctypes.data, nf, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_truepeak_host")
        return out

    def truepeak_reset(self, s=-1):
        """one stream's record and carried samples back to zero, or every stream's (-1)"""
        rc = self.L.tlb_truepeak_reset(self.h, s)
        if rc:
            raise ToolameError(rc, "tlb_truepeak_reset")

    # -- true-peak limiter (tlb_limiter_*): a look-ahead limiter on the PCM the encoder is given, 63 samples late --
    def enable_limiter(self, ceiling=0, release_ms=0):
        """allocates the limiter's state on the device (720 bytes per stream); ceiling in units of 2^-30 of full scale, 0: -1 dBTP;
        release_ms 0: 100; a second call must name the same parameters"""
        rc = self.L.tlb_limiter_enable(self.h, _limiter_params(ceiling, release_ms))
        if rc:
            raise ToolameError(rc, "tlb_limiter_enable")

    def limit(self, pcm_planar):
        """int16 [nframes, nstreams, 2, 1152] planar PCM as ingest() returns it -> (the limited PCM, LIMITER_DTYPE [nstreams] after these frames)"""
        a = np.array(pcm_planar, dtype=np.int16, order="C")           # a copy: the call works in place
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, 2, SAMPLES):
            raise ToolameError(18, f"pcm shape {a.shape}")
        out = np.zeros(self.nstreams, dtype=LIMITER_DTYPE)
        rc = self.L.tlb_limiter_host(self.h, a.ctypes.data, nf, out.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_limiter_host")
        return a, out

    def limiter_reset(self, s=-1):
        """one stream's record, delay line and gains back to zero, or every stream's (-1)"""
        rc = self.L.tlb_limiter_reset(self.h, s)
        if rc:
            raise ToolameError(rc, "tlb_limiter_reset")

    def ingest(self, interleaved, valid=None):
        """int16 [nframes, nstreams, 2304] interleaved s16le -> (planar [nframes, nstreams, 2, 1152], peaks [.., 2]).
        valid: int32 [nframes, nstreams] sample frames each slot delivers -- a short read is stretched over the frame as the reference
        does (tlb_ingest_host_valid); None: every read is full"""
        a = np.ascontiguousarray(interleaved, dtype=np.int16)
        nf = a.shape[0]
        if a.shape != (nf, self.nstreams, 2 * SAMPLES):
            raise ToolameError(18, f"interleaved shape {a.shape}")
        pcm = np.zeros((nf, self.nstreams, 2, SAMPLES), dtype=np.int16)
        peaks = np.zeros((nf, self.nstreams, 2), dtype=np.int16)
        if valid is None:
            rc = self.L.tlb_ingest_host(self.h, a.ctypes.data, nf, pcm.ctypes.data, peaks.ctypes.data)
            if rc:
                raise ToolameError(rc, "tlb_ingest_host")
            return pcm, peaks
        v = np.ascontiguousarray(valid, dtype=np.int32)
        if v.shape != (nf, self.nstreams):
            raise ToolameError(18, f"valid shape {v.shape}")
        rc = self.L.tlb_ingest_host_valid(self.h, a.ctypes.data, v.ctypes.data, nf, pcm.ctypes.data, peaks.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_ingest_host_valid")
        return pcm, peaks

    def underrun(self, valid, underrun_ms, underruns):
        """tlb_underrun_host over valid int32 [nframes, nstreams]: the two uint32 [nstreams] counters are advanced in place"""
        v = np.ascontiguousarray(valid, dtype=np.int32)
        if v.ndim != 2 or v.shape[1] != self.nstreams or underrun_ms.dtype != np.uint32 or underruns.dtype != np.uint32 or \
                underrun_ms.shape != (self.nstreams,) or underruns.shape != (self.nstreams,):
            raise ToolameError(18, "underrun arguments")
        rc = self.L.tlb_underrun_host(self.h, v.ctypes.data, v.shape[0], underrun_ms.ctypes.data, underruns.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_underrun_host")

    def ingest_device(self, d_in_ptr, nframes, d_pcm_ptr, d_peaks_ptr, stream=None):
        rc = self.L.tlb_ingest_device(self.h, d_in_ptr, nframes, d_pcm_ptr, d_peaks_ptr, stream)
        if rc:
            raise ToolameError(rc, "tlb_ingest_device")

    def edi_af(self, frames, levels, state, version=b""):
        """frames uint8 [nframes, nstreams, out_stride] (encode() layout), levels int16 [nframes, nstreams, 2] or None,
        state = edi_state_init(...) (advanced in place) -> (packets uint8 [nframes * max_upf, nstreams, stride], lengths int32):
        one packet per 24-ms unit in slot order frame * max_upf + unit (include/toolame_batch.h, UNITS)"""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = f.shape[0]
        if f.shape != (nf, self.nstreams, self.out_stride) or state.dtype != EDI_STATE_DTYPE or state.shape != (self.nstreams,):
            raise ToolameError(18, f"frames {f.shape} / state {state.shape}")
        lv = np.ascontiguousarray(levels, dtype=np.int16) if levels is not None else None
        ps = self.L.tlb_edi_af_stride(self.h, len(version))
        if ps <= 0:
            raise ToolameError(18, "version string too long")
        if self.max_upf <= 0:
            raise ToolameError(1, "a stream's frames are no whole number of 24-ms units (32 kHz)")
        pkts = np.zeros((nf * self.max_upf, self.nstreams, ps), dtype=np.uint8)
        plen = np.zeros((nf * self.max_upf, self.nstreams), dtype=np.int32)
        rc = self.L.tlb_edi_af_host(self.h, f.ctypes.data, lv.ctypes.data if lv is not None else None, nf, state.ctypes.data,
                                    bytes(version), len(version), pkts.ctypes.data, plen.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_edi_af_host")
        return pkts, plen

    def zmq_frames(self, frames, peaks=None):
        """frames uint8 [nframes, nstreams, out_stride] -> ZeroMQ messages uint8 [nframes * max_upf, nstreams, 12 + out_stride],
        one per 24-ms unit in slot order (struct zmq_frame_header_t + unit; datasize 0 = absent slot)"""
        f = np.ascontiguousarray(frames, dtype=np.uint8)
        nf = f.shape[0]
        if f.shape != (nf, self.nstreams, self.out_stride) or self.max_upf <= 0:
            raise ToolameError(18 if self.max_upf > 0 else 1, f"frames {f.shape}")
        pk = np.ascontiguousarray(peaks, dtype=np.int16) if peaks is not None else None
        ms = self.L.tlb_zmq_msg_stride(self.h)
        msgs = np.zeros((nf * self.max_upf, self.nstreams, ms), dtype=np.uint8)
        rc = self.L.tlb_zmq_frame_host(self.h, f.ctypes.data, pk.ctypes.data if pk is not None else None, nf, msgs.ctypes.data)
        if rc:
            raise ToolameError(rc, "tlb_zmq_frame_host")
        return msgs

    def edi_pft(self, af, af_len, pseq, fec=0, chunk_len=207, transport=False, addr_source=0, dest_port=0):
        """AF packets (edi_af() output) -> PFT fragments.  pseq uint16 [nstreams] is advanced in place.
        Returns (fragments uint8 [nframes, nstreams, max_frags, frag_stride], lengths int32 [.., max_frags], counts int32 [nframes, nstreams])"""
        a = np.ascontiguousarray(af, dtype=np.uint8)
        nf, ns, stride = a.shape
        al = np.ascontiguousarray(af_len, dtype=np.int32)
        if ns != self.nstreams or al.shape != (nf, ns) or pseq.dtype != np.uint16 or pseq.shape != (ns,):
            raise ToolameError(18, "edi_pft argument shapes")
        mf, fs = C.c_int(0), C.c_int(0)
        rc = self.L.tlb_edi_pft_shape(self.h, stride, fec, chunk_len, 1 if transport else 0, C.byref(mf), C.byref(fs))
        if rc:
            raise ToolameError(rc, "tlb_edi_pft_shape")
        frags = np.zeros((nf, ns, mf.value, fs.value), dtype=np.uint8)
        flen = np.zeros((nf, ns, mf.value), dtype=np.int32)
        nfrag = np.zeros((nf, ns), dtype=np.int32)
        rc = self.L.tlb_edi_pft_host(self.h, a.ctypes.data, al.ctypes.data, nf, stride, pseq.ctypes.data, fec, chunk_len, 1 if transport else 0,
                                     addr_source, dest_port, frags.ctypes.data, flen.ctypes.data, nfrag.ctypes.data, mf.value, fs.value)
        if rc:
            raise ToolameError(rc, "tlb_edi_pft_host")
        return frags, flen, nfrag

    def last_kernel_ms(self):
        return float(self.L.tlb_last_kernel_ms(self.h))

    def last_stage_ms(self):
        """(psy-2 kernel ms, encode kernel ms) of the last launch of an all-model-2/4 batch, else None (models 1/3: one kernel; model 0: no psy kernel)"""
        a, b = C.c_float(0), C.c_float(0)
        if self.L.tlb_last_stage_ms(self.h, C.byref(a), C.byref(b)):
            return None
        return float(a.value), float(b.value)

    def reset(self):
        rc = self.L.tlb_reset(self.h)
        if rc:
            raise ToolameError(rc, "tlb_reset")
        self._first = True

    def close(self):
        if getattr(self, "h", None):
            self.L.tlb_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ------------------------------------------------------------------------------------------
# node level: every GPU of one host behind one handle (include/toolame_batch.h part 3, csrc/tlb_node.cpp)
class _CNodeConfig(C.Structure):
    _fields_ = [("plane", C.c_int), ("tick", _CTickConfig)]


class _CNodeShardInfo(C.Structure):
    _fields_ = [("shard", C.c_int), ("device", C.c_int), ("first", C.c_int), ("nstreams", C.c_int), ("state", C.c_int), ("last_err", C.c_int),
                ("failures", C.c_long), ("restarts", C.c_long), ("lost_steps", C.c_long), ("what", C.c_char * 192),
                ("device_name", C.c_char * 64), ("pci", C.c_char * 24), ("uuid", C.c_char * 36), ("num_cu", C.c_int), ("num_xcd", C.c_int),
                ("hbm_gb", C.c_double)]


class _CNodeShardDeadline(C.Structure):
    _fields_ = [("state", C.c_int), ("late_events", C.c_long), ("rejoins", C.c_long), ("dropped_steps", C.c_long), ("missed_steps", C.c_long),
                ("last_late_step", C.c_long), ("last_rejoin_step", C.c_long), ("worst_overrun_ms", C.c_double)]


class _CNodeCounter(C.Structure):
    _fields_ = [("shard", C.c_int), ("device", C.c_int), ("first", C.c_int), ("nstreams", C.c_int), ("steps", C.c_long), ("frames", C.c_long),
                ("busy_ns", C.c_double), ("device_ms", C.c_double), ("wall_ns", C.c_double)]

    def asdict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def node_partition(nstreams, nshards):
    """[(first, n)] per shard: streams [g*N/G, (g+1)*N/G); pure arithmetic, no GPU"""
    L = load_library()
    out = []
    for g in range(nshards):
        f, n = C.c_int(0), C.c_int(0)
        L.tlb_node_partition(nstreams, nshards, g, C.byref(f), C.byref(n))
        out.append((f.value, n.value))
    return out


def node_plan(configs, nshards):
    """per shard: dict(first, n, nconfigs, lists = streams per kernel list (psy 0, 1, 2+4, 3), mono_pairs) -- what tlb_create() will make
    of each block; raises ToolameError on the first illegal configuration.  No GPU needed."""
    L = load_library()
    configs = list(configs)
    arr = _config_array(configs)
    out = []
    for g in range(nshards):
        f, n, nc, mp = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
        ls = (C.c_int * 4)()
        rc = L.tlb_node_plan_shard(len(configs), arr, nshards, g, C.byref(f), C.byref(n), C.byref(nc), ls, C.byref(mp))
        if rc:
            raise ToolameError(rc, "tlb_node_plan_shard")
        out.append(dict(first=f.value, n=n.value, nconfigs=nc.value, lists=list(ls), mono_pairs=mp.value))
    return out


class Node:
    """tlb_node_*: N streams over the shards of one host (one tlb_tick or tlb_batch + one host thread per shard; `devices[g]` is the HIP
    device of shard g and may repeat).  plane "tick": fill pcm(s), run() / submit() + wait(), read frame(s) / packets(s) ...;
    plane "batch": device-resident buffers per shard, encode(pcm) with pcm int16 [nframes][nstreams][2][1152] split by the wrapper.
    deadline_ms > 0 (plane "tick"): the node's tick deadline (include/toolame_batch.h, TICK DEADLINE); a call in which a shard goes late
    raises ToolameError code 19, shard_deadline(g) has its record."""

    def __init__(self, configs, devices=(0,), plane="tick", egress="frames", ngroups=0, with_xpad=False, version=b"", now_s=1700000000,
                 delay_ms=0, tist=False, tai_utc_offset=37, fec=0, chunk_len=207, transport=False, addr_source=0, dest_port=0, lib=None,
                 deadline_ms=0):
        self.L = lib or load_library()
        configs = list(configs)
        self.configs = configs
        self.nstreams = len(configs)
        self.plane = plane
        self.with_xpad = bool(with_xpad)
        self._version = bytes(version)
        nc = _CNodeConfig()
        nc.plane = 0 if plane == "tick" else 1
        nc.tick = _CTickConfig(Tick.EGRESS[egress], ngroups, 1 if with_xpad else 0, self._version, len(self._version), int(now_s), int(delay_ms),
                               1 if tist else 0, int(tai_utc_offset), fec, chunk_len, 1 if transport else 0, addr_source, dest_port)
        devs = (C.c_int * len(devices))(*devices)
        err = C.c_int(0)
        self.h = self.L.tlb_node_create(len(devices), devs, self.nstreams, _config_array(configs), C.byref(nc), C.byref(err))
        if not self.h:
            raise ToolameError(err.value, "tlb_node_create")
        self.nshards = self.L.tlb_node_nshards(self.h)
        self.blocks = node_partition(self.nstreams, self.nshards)
        self._dev = {}          # BATCH plane: (shard, tag) -> (device pointer, bytes)
        if plane == "tick":
            self.units = [self.L.tlb_node_units(self.h, s) for s in range(self.nstreams)]
        if deadline_ms:
            self.set_deadline_ms(deadline_ms)

    def close(self):
        if self.h:
            for (g, _), (p, _) in list(self._dev.items()):
                self.L.tlb_node_device_free(self.h, g, p)
            self._dev.clear()
            self.L.tlb_node_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _rc(self, rc, what):
        if rc:
            raise ToolameError(rc, what)

    # ---- health: fault isolation per shard (include/toolame_batch.h, FAULT ISOLATION) ----
    def describe(self):
        """one line per shard: device name, CUs, XCDs, memory, PCI address, UUID, stream block"""
        return self.L.tlb_node_describe(self.h).decode()

    def shard_status(self, g):
        info = _CNodeShardInfo()
        st = self.L.tlb_node_shard_status(self.h, g, C.byref(info))
        if st < 0:
            raise ToolameError(-st, "tlb_node_shard_status")
        d = {k: getattr(info, k) for k, _ in info._fields_}
        for k in ("what", "device_name", "pci", "uuid"):
            d[k] = d[k].decode(errors="replace")
        d["ok"] = st == 0
        return d

    def shard_ok(self, g):
        return self.L.tlb_node_shard_status(self.h, g, None) == 0

    def shard_restart(self, g, now_s=-1):
        self._rc(self.L.tlb_node_shard_restart(self.h, g, int(now_s)), "tlb_node_shard_restart")
        if self.plane == "tick":
            f, n = self.blocks[g]
            for s in range(f, f + n):
                self.units[s] = self.L.tlb_node_units(self.h, s)
        # (the wrapper's device buffers belong to the device, not to the shard's object: they stay)

    def fail_next(self, g, nth=1):
        """fault-injection TEST build only (lib=load_fault_library()): the nth launch / tick of shard g from now fails"""
        return self.L.tlb_debug_node_fail_next(self.h, g, nth)

    # ---- tick deadline (include/toolame_batch.h, TICK DEADLINE) ----
    def set_deadline_ms(self, ms):
        """ms > 0 sets the TICK plane's deadline, 0 turns it off; between steps only"""
        self._rc(self.L.tlb_node_set_deadline_ms(self.h, float(ms)), "tlb_node_set_deadline_ms")

    def shard_deadline(self, g):
        """dict(state, late_events, rejoins, dropped_steps, missed_steps, last_late_step, last_rejoin_step, worst_overrun_ms)"""
        info = _CNodeShardDeadline()
        st = self.L.tlb_node_shard_deadline_status(self.h, g, C.byref(info))
        if st < 0:
            raise ToolameError(-st, "tlb_node_shard_deadline_status")
        return {k: getattr(info, k) for k, _ in info._fields_}

    def stall_next(self, g, nth, ms, rc=0):
        """fault-injection TEST build only: the nth wait job of shard g from now holds its host thread `ms` after the tick is
        complete, then returns rc (0: the tick's results stand)"""
        self._rc(self.L.tlb_debug_node_stall_next(self.h, g, nth, int(ms), rc), "tlb_debug_node_stall_next")

    def counters(self):
        per = (_CNodeCounter * self.nshards)()
        tot = _CNodeCounter()
        self._rc(self.L.tlb_node_counters(self.h, per, C.byref(tot)), "tlb_node_counters")
        return [p.asdict() for p in per], tot.asdict()

    # ---- TICK plane ----
    def pcm(self, s):
        p = self.L.tlb_node_pcm(self.h, s)
        return np.ctypeslib.as_array((C.c_int16 * (2 * SAMPLES)).from_address(p)) if p else None

    def set_pcm(self, inter):
        """inter int16 [nstreams][2304]: every stream's interleaved frame into the current input set (block copies per shard)"""
        for g, (f, n) in enumerate(self.blocks):
            p = self.L.tlb_node_pcm(self.h, f)
            if not p:
                if not self.shard_ok(g):
                    continue                # a broken or late shard takes no input; its streams are off air until it is back
                raise ToolameError(18, "tlb_node_pcm: no input set is free (two ticks in flight)")
            np.ctypeslib.as_array((C.c_int16 * (n * 2 * SAMPLES)).from_address(p)).reshape(n, 2 * SAMPLES)[:] = inter[f:f + n]

    def set_xpad(self, s, rec, length):
        p, q = self.L.tlb_node_xpad(self.h, s), self.L.tlb_node_xpad_len(self.h, s)
        if not p or not q:
            return
        np.ctypeslib.as_array((C.c_uint8 * MAX_XPAD).from_address(p))[:] = rec
        C.c_int32.from_address(q).value = int(length)

    def submit(self):
        self._rc(self.L.tlb_node_submit(self.h), "tlb_node_submit")

    def wait(self):
        self._rc(self.L.tlb_node_wait(self.h), "tlb_node_wait")

    def run(self):
        self._rc(self.L.tlb_node_run(self.h), "tlb_node_run")

    def finish(self):
        self._rc(self.L.tlb_node_finish(self.h), "tlb_node_finish")

    def peaks(self, s):
        p = self.L.tlb_node_peaks(self.h, s)
        return tuple(np.ctypeslib.as_array((C.c_int16 * 2).from_address(p))) if p else None

    def silence_ms(self, s):
        return int(self.L.tlb_node_silence_ms(self.h, s))

    # device resampler (Tick.set_source / need with node-wide indices; remembered for shard restarts)
    def set_source(self, source_rate, stream=-1):
        self._rc(self.L.tlb_node_set_source(self.h, stream, int(source_rate)), "tlb_node_set_source")

    def need(self, s):
        n = self.L.tlb_node_need(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_node_need")
        return n

    # down sources (Tick.set_down_source / down / down_need with node-wide indices; remembered for shard restarts)
    def set_down_source(self, source_rate, stream=-1):
        self._rc(self.L.tlb_node_set_down_source(self.h, stream, int(source_rate)), "tlb_node_set_down_source")

    def down(self, s):
        """the stream's wide slot (int16 [4608] view) in its shard's current input set; None when its shard has no down source, while two
        ticks are in flight and for a broken or late shard"""
        p = self.L.tlb_node_down(self.h, s)
        return np.ctypeslib.as_array((C.c_int16 * DECIMATE_SLOT).from_address(p)) if p else None

    def down_need(self, s):
        n = self.L.tlb_node_down_need(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_node_down_need")
        return n

    # Layer II feeds (Tick.set_feed, per stream with node-wide indices)
    def set_feed(self, stream, cfg, adapt=False):
        """stream = -1: every stream; cfg = None removes the feed; between steps only.  adapt: tlb_node_set_feed_adapted"""
        c = _c_feed(cfg) if cfg is not None else None
        self._rc((self.L.tlb_node_set_feed_adapted if adapt else self.L.tlb_node_set_feed)(self.h, stream, C.byref(c) if c is not None else None), "tlb_node_set_feed")

    def feed_want(self, s):
        """1 / 0: is a feed frame wanted in the stream's slot of its shard's current input set (TICK plane)"""
        n = self.L.tlb_node_feed_want(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_node_feed_want")
        return n

    def feed(self, s):
        """the stream's slot (uint8 view) in its shard's current input set; None when its shard has no feed, while two ticks are in flight and
        for a broken or late shard"""
        p = self.L.tlb_node_feed(self.h, s)
        n = self.L.tlb_node_feed_stride(self.h, s)
        return np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)) if p and n else None

    def feed_len(self, s):
        """the stream's int32 length as a one-element view (write [0]); 0, an empty slot, unless the caller writes more"""
        p = self.L.tlb_node_feed_len(self.h, s)
        return np.ctypeslib.as_array((C.c_int32 * 1).from_address(p)) if p else None

    def feed_report(self, s):
        """the stream's report (a FRAME_REPORT_DTYPE scalar, copied) of the step waited for last; None for a broken, late or stale shard"""
        p = self.L.tlb_node_feed_report(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * FRAME_REPORT_DTYPE.itemsize).from_address(p), dtype=FRAME_REPORT_DTYPE)[0].copy()

    # down feeds (Tick.set_down_feed, per stream with node-wide indices)
    def set_down_feed(self, stream, cfg):
        """stream = -1: every stream; cfg = None removes the down feed; between steps only"""
        c = _c_feed(cfg) if cfg is not None else None
        self._rc(self.L.tlb_node_set_down_feed(self.h, stream, C.byref(c) if c is not None else None), "tlb_node_set_down_feed")

    def down_feed_want(self, s):
        """1 / 2: the feed frames wanted in the stream's two slots of its shard's current input set (TICK plane)"""
        n = self.L.tlb_node_down_feed_want(self.h, s)
        if n < 0:
            raise ToolameError(-n, "tlb_node_down_feed_want")
        return n

    def down_feed(self, s):
        """the stream's two slots (uint8 view [2, stride]) in its shard's current input set; None when its shard has no down feed, while two
        ticks are in flight and for a broken or late shard"""
        p = self.L.tlb_node_down_feed(self.h, s)
        n = self.L.tlb_node_down_feed_stride(self.h, s)
        return np.ctypeslib.as_array((C.c_uint8 * (2 * n)).from_address(p)).reshape(2, n) if p and n else None

    def down_feed_len(self, s):
        """the stream's two lengths (int32 view [2]) in its shard's current input set"""
        p = self.L.tlb_node_down_feed_len(self.h, s)
        return np.ctypeslib.as_array((C.c_int32 * 2).from_address(p)) if p else None

    def down_feed_report(self, s):
        """the stream's two reports (FRAME_REPORT_DTYPE [2], copied) of the step waited for last; None for a broken, late or stale shard"""
        p = self.L.tlb_node_down_feed_report(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * (2 * FRAME_REPORT_DTYPE.itemsize)).from_address(p), dtype=FRAME_REPORT_DTYPE).copy()

    # short reads (Tick.enable_short_reads, per stream with node-wide indices)
    def enable_short_reads(self):
        self._rc(self.L.tlb_node_enable_short_reads(self.h), "tlb_node_enable_short_reads")

    def valid(self, s):
        """the stream's int32 in its shard's current input set as a one-element view (write [0]); None when not enabled, while two ticks
        are in flight and for a broken or late shard"""
        p = self.L.tlb_node_valid(self.h, s)
        return np.ctypeslib.as_array((C.c_int32 * 1).from_address(p)) if p else None

    def underrun_ms(self, s):
        return int(self.L.tlb_node_underrun_ms(self.h, s))

    def underruns(self, s):
        return int(self.L.tlb_node_underruns(self.h, s))

    # confidence monitor (Tick.enable_monitor, per stream with node-wide indices)
    def enable_monitor(self, what="audio"):
        self._rc(self.L.tlb_node_enable_monitor(self.h, MONITOR_WHAT.get(what, what)), "tlb_node_enable_monitor")

    def monitor(self, s):
        """the stream's record (a MONITOR_DTYPE scalar, copied) of the step waited for last; None when not enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_monitor(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * MONITOR_DTYPE.itemsize).from_address(p), dtype=MONITOR_DTYPE)[0].copy()

    # loudness meter (Tick.enable_loudness, per stream with node-wide indices)
    def enable_loudness(self):
        self._rc(self.L.tlb_node_enable_loudness(self.h), "tlb_node_enable_loudness")

    def loudness(self, s):
        """the stream's record (a LOUDNESS_DTYPE scalar, copied) of the step waited for last; None when not enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_loudness(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * LOUDNESS_DTYPE.itemsize).from_address(p), dtype=LOUDNESS_DTYPE)[0].copy()

    def loudness_programme(self):
        """LOUDNESS_PROGRAMME_DTYPE [nstreams], between steps; all zero for the streams of a broken or late shard"""
        out = np.zeros(self.nstreams, dtype=LOUDNESS_PROGRAMME_DTYPE)
        self._rc(self.L.tlb_node_loudness_programme(self.h, out.ctypes.data), "tlb_node_loudness_programme")
        return out

    def loudness_reset(self, s=-1):
        self._rc(self.L.tlb_node_loudness_reset(self.h, int(s)), "tlb_node_loudness_reset")

    # loudness range (Tick.enable_lra): after enable_loudness
    def enable_lra(self):
        self._rc(self.L.tlb_node_enable_lra(self.h), "tlb_node_enable_lra")
        return self

    def lra(self):
        """LRA_DTYPE [nstreams], between steps; all zero for the streams of a broken or late shard"""
        out = np.zeros(self.nstreams, dtype=LRA_DTYPE)
        self._rc(self.L.tlb_node_lra(self.h, out.ctypes.data), "tlb_node_lra")
        return out

    # true-peak meter (Tick.enable_truepeak, per stream with node-wide indices)
    def enable_truepeak(self, ceiling=0):
        self._rc(self.L.tlb_node_enable_truepeak(self.h, int(ceiling)), "tlb_node_enable_truepeak")

    def truepeak(self, s):
        """the stream's record (a TRUEPEAK_DTYPE scalar, copied) of the step waited for last; None when not enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_truepeak(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * TRUEPEAK_DTYPE.itemsize).from_address(p), dtype=TRUEPEAK_DTYPE)[0].copy()

    def truepeak_reset(self, s=-1):
        self._rc(self.L.tlb_node_truepeak_reset(self.h, int(s)), "tlb_node_truepeak_reset")

    # feed concealment (Tick.enable_conceal, per stream with node-wide indices; between steps)
    def enable_conceal(self, hold=4, step=3, stream=-1, any_feed=False):
        name = "tlb_node_enable_feed_loss" if any_feed else "tlb_node_enable_conceal"
        self._rc(getattr(self.L, name)(self.h, int(stream), int(hold), int(step)), name)

    def conceal(self, s):
        """the stream's record (a CONCEAL_DTYPE scalar, copied) of the step waited for last; None when never enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_conceal(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * CONCEAL_DTYPE.itemsize).from_address(p), dtype=CONCEAL_DTYPE)[0].copy()

    def conceal_reset(self, s=-1):
        self._rc(self.L.tlb_node_conceal_reset(self.h, int(s)), "tlb_node_conceal_reset")

    # true-peak limiter (Tick.enable_limiter, per stream with node-wide indices)
    def enable_limiter(self, ceiling=0, release_ms=0):
        self._rc(self.L.tlb_node_enable_limiter(self.h, _limiter_params(ceiling, release_ms)), "tlb_node_enable_limiter")

    def limiter(self, s):
        """the stream's record (a LIMITER_DTYPE scalar, copied) of the step waited for last; None when not enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_limiter(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * LIMITER_DTYPE.itemsize).from_address(p), dtype=LIMITER_DTYPE)[0].copy()

    def limiter_reset(self, s=-1):
        self._rc(self.L.tlb_node_limiter_reset(self.h, int(s)), "tlb_node_limiter_reset")

    # compare monitor (Tick.enable_compare, per stream with node-wide indices)
    def enable_compare(self, params=None):
        self._rc(self.L.tlb_node_enable_compare(self.h, compare_params(params).ctypes.data), "tlb_node_enable_compare")

    def compare(self, s):
        """the stream's record (a COMPARE_DTYPE scalar, copied) of the step waited for last; None when not enabled and for a broken, late or stale shard"""
        p = self.L.tlb_node_compare(self.h, s)
        if not p:
            return None
        return np.frombuffer((C.c_uint8 * COMPARE_DTYPE.itemsize).from_address(p), dtype=COMPARE_DTYPE)[0].copy()

    def monitor_listen(self, s):
        self._rc(self.L.tlb_node_monitor_listen(self.h, int(s)), "tlb_node_monitor_listen")

    def monitor_pcm(self):
        """(node-wide stream, int16 [2][1152] view) of the step waited for last, or (-1, None)"""
        s = C.c_int(-1)
        p = self.L.tlb_node_monitor_pcm(self.h, C.byref(s))
        if not p:
            return -1, None
        return s.value, np.ctypeslib.as_array((C.c_int16 * (2 * SAMPLES)).from_address(p)).reshape(2, SAMPLES)

    def frame(self, s):
        n = C.c_int(0)
        p = self.L.tlb_node_frame(self.h, s, C.byref(n))
        return C.string_at(p, n.value) if p and n.value else b""

    def _units(self, fn, s):
        out = []
        for u in range(self.units[s]):
            n = C.c_int(0)
            p = fn(self.h, s, u, C.byref(n))
            if p and n.value:
                out.append(C.string_at(p, n.value))
        return out

    def packets(self, s):
        return self._units(self.L.tlb_node_packet, s)

    def messages(self, s):
        return self._units(self.L.tlb_node_message, s)

    def fragments(self, s):
        out = []
        for u in range(self.units[s]):
            fr = []
            for k in range(self.L.tlb_node_fragments(self.h, s, u)):
                n = C.c_int(0)
                p = self.L.tlb_node_fragment(self.h, s, u, k, C.byref(n))
                fr.append(C.string_at(p, n.value))
            if fr:
                out.append(fr)
        return out

    # ---- both planes ----
    def set_gain_db(self, gain_db, stream=-1):
        self._rc(self.L.tlb_node_set_gain_db(self.h, stream, float(gain_db)), "tlb_node_set_gain_db")

    def stream_reset(self, s):
        self._rc(self.L.tlb_node_stream_reset(self.h, s), "tlb_node_stream_reset")

    def stream_finish(self, s):
        buf = (C.c_uint8 * 2048)()
        n = self.L.tlb_node_stream_finish(self.h, s, buf, 2048)
        if n < 0:
            raise ToolameError(-n, "tlb_node_stream_finish")
        return bytes(buf[:n])

    def stream_reconfigure(self, s, config):
        self._rc(self.L.tlb_node_stream_reconfigure(self.h, s, _config_array([config])), "tlb_node_stream_reconfigure")
        if self.plane == "tick":
            self.units[s] = self.L.tlb_node_units(self.h, s)

    # ---- BATCH plane ----
    def out_stride(self, g):
        return self.L.tlb_out_stride(self.L.tlb_node_batch(self.h, g))

    def _buf(self, g, tag, nbytes):
        cur = self._dev.get((g, tag))
        if cur and cur[1] >= nbytes:
            return cur[0]
        if cur:
            self.L.tlb_node_device_free(self.h, g, cur[0])
        p = self.L.tlb_node_device_alloc(self.h, g, nbytes)
        if not p:
            raise ToolameError(17, "tlb_node_device_alloc")
        self._dev[(g, tag)] = (p, nbytes)
        return p

    def upload(self, pcm, slot=0):
        """pcm int16 [nframes][nstreams][2][1152] -> one device buffer per shard (the shard's streams, [nframes][n_g][2][1152]);
        `slot` names the buffer set (a caller alternating two resident inputs uploads slot 0 and slot 1 once)"""
        nf = pcm.shape[0]
        ptrs = (C.c_void_p * self.nshards)()
        for g, (f, n) in enumerate(self.blocks):
            blk = np.ascontiguousarray(pcm[:, f:f + n], dtype=np.int16)
            ptrs[g] = self._buf(g, ("pcm", slot), blk.nbytes)
            self._rc(self.L.tlb_node_copy_in(self.h, g, ptrs[g], blk.ctypes.data, blk.nbytes), "tlb_node_copy_in")
        self._pcm_ptrs = getattr(self, "_pcm_ptrs", {})
        self._pcm_ptrs[slot] = (ptrs, nf)
        return ptrs

    def encode_resident(self, slot=0, want_len=True):
        """queue one encode call on every shard over the PCM uploaded as `slot`; returns at once (sync() waits)"""
        ptrs, nf = self._pcm_ptrs[slot]
        outs, lens = (C.c_void_p * self.nshards)(), (C.c_void_p * self.nshards)()
        for g, (f, n) in enumerate(self.blocks):
            if not self.shard_ok(g):
                continue                    # (the node skips a broken shard: its array elements are not read)
            outs[g] = self._buf(g, "out", nf * n * self.out_stride(g))
            lens[g] = self._buf(g, "len", nf * n * 4)
        self._out_ptrs, self._len_ptrs, self._nf, self._have_len = outs, lens, nf, bool(want_len)
        self._rc(self.L.tlb_node_encode_device(self.h, ptrs, nf, None, None, outs, lens if want_len else None), "tlb_node_encode_device")

    def sync(self):
        self._rc(self.L.tlb_node_sync(self.h), "tlb_node_sync")

    def download(self, nframes=None):
        """-> per stream: the bytes of output slots 0..nframes-1 concatenated (slot lengths from the _len variant)"""
        if not getattr(self, "_have_len", True):
            raise ToolameError(18, "Node.download(): the last encode_resident() was queued with want_len=False -- no slot lengths to cut the frames by")
        nf = nframes or self._nf
        out = [b""] * self.nstreams
        for g, (f, n) in enumerate(self.blocks):
            if not self.shard_ok(g):
                continue                    # nothing of a broken shard is read (its buffers hold a half-finished step)
            st = self.out_stride(g)
            fr = np.empty((nf, n, st), dtype=np.uint8)
            ln = np.empty((nf, n), dtype=np.int32)
            self._rc(self.L.tlb_node_copy_out(self.h, g, fr.ctypes.data, self._out_ptrs[g], fr.nbytes), "tlb_node_copy_out")
            self._rc(self.L.tlb_node_copy_out(self.h, g, ln.ctypes.data, self._len_ptrs[g], ln.nbytes), "tlb_node_copy_out")
            for k in range(n):
                out[f + k] = b"".join(fr[i, k, :ln[i, k]].tobytes() for i in range(nf))
        return out

    def encode(self, pcm):
        """upload + encode + sync + download (the convenience path of the parity tests)"""
        self.upload(pcm)
        self.encode_resident()
        self.sync()
        return self.download()

    def flush(self):
        """the pending (last) frame of every stream"""
        outs, lens = (C.c_void_p * self.nshards)(), (C.c_void_p * self.nshards)()
        for g, (f, n) in enumerate(self.blocks):
            if not self.shard_ok(g):
                continue
            outs[g] = self._buf(g, "fout", n * self.out_stride(g))
            lens[g] = self._buf(g, "flen", n * 4)
        self._rc(self.L.tlb_node_flush_device(self.h, outs, lens), "tlb_node_flush_device")
        self.sync()
        out = [b""] * self.nstreams
        for g, (f, n) in enumerate(self.blocks):
            if not self.shard_ok(g):
                continue
            st = self.out_stride(g)
            fr = np.empty((n, st), dtype=np.uint8)
            ln = np.empty((n,), dtype=np.int32)
            self._rc(self.L.tlb_node_copy_out(self.h, g, fr.ctypes.data, outs[g], fr.nbytes), "tlb_node_copy_out")
            self._rc(self.L.tlb_node_copy_out(self.h, g, ln.ctypes.data, lens[g], ln.nbytes), "tlb_node_copy_out")
            for k in range(n):
                out[f + k] = fr[k, :ln[k]].tobytes()
        return out
