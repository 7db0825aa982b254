"""odr-audioenc_amd -- MI355X-native batched DAB MP2 (MPEG-1/2 Layer II) encode path.

A drop-in for ONE hot path of Opendigitalradio/ODR-AudioEnc: libtoolame-dab's per-frame encoder
(toolame_encode_frame(), libtoolame-dab/toolame.c:267-554), re-designed as hand-written HIP kernels
for gfx950 behind the reference's own C-ABI plus a batched, handle-based API
(include/toolame_batch.h).  Python is only the thin binding used by tests and bench.py; the product
is csrc/ (kernels + C-ABI, built into libtoolame_dab_hip.so).

There is NO CPU fallback: importing works anywhere, but creating an encoder raises if the HIP
library is missing or no GPU is visible.
"""
from .toolame import (  # noqa: F401
    Batch, StreamConfig, ToolameError, LIB_PATH, build, load_library, lds_bytes_per_stream, legacy_api,
    EDI_STATE_DTYPE, edi_state_init, Tick, Node, node_partition, node_plan, load_fault_library, FAULT_LIB_PATH,
    FRAME_REPORT_DTYPE, FRAME_FIELDS_DTYPE, DEC_EMPTY, DEC_BAD_MASK, DEC_SCFCRC_UNCHECKED,
    MONITOR_DTYPE, COMPARE_DTYPE, COMPARE_PARAMS_DTYPE, COMPARE_DELAY, COMPARE_DEFAULTS, compare_params,
    COMPARE_JUDGED0, COMPARE_JUDGED1, COMPARE_MISMATCH, COMPARE_SWAPPED, COMPARE_SKIPPED,
    resample_need_at, resample_taps, decimate_need_at, decimate_taps, DECIMATE_SLOT, FeedConfig, feed_check_config, feed_frame_bytes, feed_want_at, down_feed_want_at, DEC_UNWANTED,
    LOUDNESS_DTYPE, LOUDNESS_PROGRAMME_DTYPE, LOUDNESS_BINS, loudness_lufs, loudness_taps, loudness_scale,
    LRA_DTYPE, lra_lu,
    TRUEPEAK_DTYPE, TRUEPEAK_TAPS, TRUEPEAK_CEILING_DEFAULT, truepeak_dbtp, truepeak_taps,
    LIMITER_DTYPE, LIMITER_DELAY, limiter_step,
    CONCEAL_DTYPE, CONCEAL_MUTE,
)
