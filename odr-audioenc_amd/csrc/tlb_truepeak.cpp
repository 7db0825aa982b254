// tlb_truepeak.cpp -- the batch-level entry points of the true-peak meter (include/toolame_batch.h, tlb_truepeak_*): the committed table,
// the per-stream state (allocated by tlb_truepeak_enable alone) and one launch of the kernel of toolame_truepeak.hip through tl_kernels.h.
// Host C++.
#include <stddef.h>
#include "tlb_internal.h"
#include "tl_truepeak_taps.inc"

static_assert(sizeof(tlb_truepeak_record) == sizeof(TlTruePeakRecord) && sizeof(tlb_truepeak_record) == 32, "C-ABI record");
static_assert(offsetof(tlb_truepeak_record, frames) == offsetof(TlTruePeakRecord, frames) && offsetof(tlb_truepeak_record, overs) == offsetof(TlTruePeakRecord, overs) &&
              offsetof(tlb_truepeak_record, peak) == offsetof(TlTruePeakRecord, peak) && offsetof(tlb_truepeak_record, peak_max) == offsetof(TlTruePeakRecord, peak_max) &&
              offsetof(tlb_truepeak_record, sample_max) == offsetof(TlTruePeakRecord, sample_max), "record layout");
static_assert(sizeof tl_truepeak_taps == 3 * TL_TP_TAPS * sizeof(int16_t) && TLB_TRUEPEAK_TAPS == TL_TP_TAPS, "table shape");

// the true-peak state of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle): a stream's record and carried
// samples are contiguous
int truepeak_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_tp_rec) return TLB_OK;
    HIPCHK(hipMemset(b->d_tp_rec + s0, 0, (size_t)n * sizeof(TlTruePeakRecord)));
    HIPCHK(hipMemset(b->d_tp_hist + (size_t)s0 * TL_TP_CARRY, 0, (size_t)n * TL_TP_CARRY * sizeof(uint32_t)));
    HIPCHK(hipDeviceSynchronize());              // the callers' streams do not wait for the null stream
    return TLB_OK;
}

extern "C" {

int tlb_truepeak_taps(int16_t out[3][TLB_TRUEPEAK_TAPS])
{
    if (!out) return TLB_ERR_ARG;
    memcpy(out, tl_truepeak_taps, sizeof tl_truepeak_taps);
    return TLB_OK;
}

double tlb_truepeak_dbtp(uint32_t v) { return v ? 20.0 * log10((double)v / 1073741824.0) : -INFINITY; }

int tlb_truepeak_enable(tlb_batch *b, uint32_t ceiling)
{
    if (!b) return TLB_ERR_ARG;
    if (b->d_tp_rec) return TLB_OK;              // the ceiling stays
    HIPCHK(hipSetDevice(b->device));
    const size_t ns = (size_t)b->nstreams;
    TlbMem m;
    TlTruePeakRecord *rec = m.dev<TlTruePeakRecord>(ns);
    uint32_t *hist = m.dev<uint32_t>(TL_TP_CARRY * ns);
    int16_t *taps = m.scratch<int16_t>(3 * TL_TP_TAPS);
    m.upload(taps, tl_truepeak_taps, sizeof tl_truepeak_taps);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_tp_rec = rec; b->d_tp_hist = hist; b->d_tp_taps = taps;
    b->tp_ceiling = ceiling ? ceiling : TLB_TRUEPEAK_CEILING_DEFAULT;
    return TLB_OK;
}

int tlb_truepeak_device(tlb_batch *b, const int16_t *d_pcm_planar, int nframes, tlb_truepeak_record *d_records, void *hip_stream)
{
    if (!b || !d_pcm_planar || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (((uintptr_t)d_pcm_planar & 15u) || ((uintptr_t)d_records & 3u)) return TLB_ERR_ARG;      // the PCM comes in as 16-byte pieces
    if (!b->d_tp_rec) return TLB_ERR_ARG;        // never enabled
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    HIPCHK(hipSetDevice(b->device));
    const TlTruePeakArgs A = {d_pcm_planar, b->d_tp_rec, (TlTruePeakRecord *)d_records, b->d_tp_hist, b->d_tp_taps, b->d_configs, b->d_stream_cfg,
                              b->tp_ceiling, b->nstreams, nframes};
    HIPCHK(tlk_truepeak((hipStream_t)hip_stream, A));
    return TLB_OK;
}

int tlb_truepeak_host(tlb_batch *b, const int16_t *pcm_planar, int nframes, tlb_truepeak_record *records)
{
    return meter_host(b, b ? b->d_tp_rec : nullptr, pcm_planar, nframes, records, tlb_truepeak_device);
}

int tlb_truepeak_reset(tlb_batch *b, int stream) { return meter_reset(b, b ? b->d_tp_rec : nullptr, stream, truepeak_clear_streams); }

}  // extern "C"
