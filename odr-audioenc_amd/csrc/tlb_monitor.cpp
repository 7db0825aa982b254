// tlb_monitor.cpp -- the batch-level entry points of the confidence monitor (include/toolame_batch.h, tlb_monitor_*): argument checks and
// one launch of the fold kernel of toolame_monitor.hip through tl_kernels.h.  Host C++.  The tick and node planes (tlb_tick.cpp,
// tlb_node.cpp) queue tlb_decode_device and this fold behind their egress kernels.
#include <stddef.h>
#include "tlb_internal.h"
#include "mp2_monitor.h"

static_assert(sizeof(tlb_monitor_record) == 4 * TL_MON_WORDS, "C-ABI record");
static_assert(offsetof(tlb_monitor_record, frames) == 4 * TL_MON_FRAMES && offsetof(tlb_monitor_record, bad_frames) == 4 * TL_MON_BAD &&
              offsetof(tlb_monitor_record, bad_run) == 4 * TL_MON_RUN && offsetof(tlb_monitor_record, flags_seen) == 4 * TL_MON_SEEN &&
              offsetof(tlb_monitor_record, last_status) == 4 * TL_MON_LAST && offsetof(tlb_monitor_record, out_silence_ms) == 4 * TL_MON_SILENCE &&
              offsetof(tlb_monitor_record, out_peak) == 4 * TL_MON_PEAKS && offsetof(tlb_monitor_record, reserved_) == 4 * TL_MON_RESERVED, "record layout");

extern "C" {

int tlb_monitor_device(tlb_batch *b, const tlb_frame_report *d_report, const int16_t *d_pcm, int nframes, tlb_monitor_record *d_record, void *hip_stream)
{
    if (!b || !d_report || !d_record || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (((uintptr_t)d_report | (uintptr_t)d_pcm | (uintptr_t)d_record) & 3u) return TLB_ERR_ARG;        // the kernel moves 32-bit words
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_monitor((hipStream_t)hip_stream, (const TlFrameReport *)d_report, d_pcm, (uint32_t *)d_record, b->d_configs, b->d_stream_cfg, b->nstreams, nframes));
    return TLB_OK;
}

int tlb_monitor_host(tlb_batch *b, const tlb_frame_report *report, const int16_t *pcm, int nframes, tlb_monitor_record *record)
{
    if (!b || !report || !record || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (((uintptr_t)report | (uintptr_t)pcm | (uintptr_t)record) & 3u) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams, rec_bytes = (size_t)b->nstreams * sizeof(tlb_monitor_record);
    TlbMem m;
    tlb_frame_report *d_report = m.scratch<tlb_frame_report>(slots); tlb_monitor_record *d_record = m.scratch<tlb_monitor_record>((size_t)b->nstreams);
    int16_t *d_pcm = pcm ? m.scratch<int16_t>(slots * 2 * TLB_SAMPLES_PER_FRAME) : nullptr;
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_report, report, slots * sizeof(tlb_frame_report), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_record, record, rec_bytes, hipMemcpyHostToDevice));
    if (pcm) HIPCHK(hipMemcpy(d_pcm, pcm, slots * 2 * TLB_SAMPLES_PER_FRAME * sizeof(int16_t), hipMemcpyHostToDevice));
    if (int rc = tlb_monitor_device(b, d_report, d_pcm, nframes, d_record, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(record, d_record, rec_bytes, hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
