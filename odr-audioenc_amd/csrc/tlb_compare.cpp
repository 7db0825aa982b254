// tlb_compare.cpp -- the batch-level entry points of the compare monitor (include/toolame_batch.h, tlb_compare_*): argument checks, the
// per-stream input history (allocated by the first call) and one launch of the kernel of toolame_compare.hip through tl_kernels.h.
// Host C++.  The tick plane (tlb_tick.cpp) queues it behind its group's decode.
#include <stddef.h>
#include "tlb_internal.h"
#include "tlb_plan.h"

static_assert(sizeof(tlb_compare_record) == sizeof(TlCompareRecord) && sizeof(tlb_compare_params) == sizeof(TlCompareParams), "C-ABI record and parameters");
static_assert(offsetof(tlb_compare_record, sxx) == offsetof(TlCompareRecord, sxx) && offsetof(tlb_compare_record, syy) == offsetof(TlCompareRecord, syy) &&
              offsetof(tlb_compare_record, sxy) == offsetof(TlCompareRecord, sxy) && offsetof(tlb_compare_record, sxz) == offsetof(TlCompareRecord, sxz) &&
              offsetof(tlb_compare_record, frames_compared) == offsetof(TlCompareRecord, frames_compared) && offsetof(tlb_compare_record, frames_judged) == offsetof(TlCompareRecord, frames_judged) &&
              offsetof(tlb_compare_record, mismatch_frames) == offsetof(TlCompareRecord, mismatch_frames) && offsetof(tlb_compare_record, mismatch_run) == offsetof(TlCompareRecord, mismatch_run) &&
              offsetof(tlb_compare_record, swapped_frames) == offsetof(TlCompareRecord, swapped_frames) && offsetof(tlb_compare_record, last_flags) == offsetof(TlCompareRecord, last_flags) &&
              offsetof(tlb_compare_record, reserved_) == offsetof(TlCompareRecord, reserved_), "record layout");
static_assert(offsetof(tlb_compare_params, min_energy) == offsetof(TlCompareParams, min_energy) && offsetof(tlb_compare_params, corr_num) == offsetof(TlCompareParams, corr_num) &&
              offsetof(tlb_compare_params, corr_den) == offsetof(TlCompareParams, corr_den), "parameter layout");
static_assert(TLB_COMPARE_DELAY == TL_CMP_DELAY && TLB_SAMPLES_PER_FRAME == TL_CMP_FRAME && TLB_COMPARE_JUDGED0 == TL_CMP_JUDGED0 && TLB_COMPARE_JUDGED1 == TL_CMP_JUDGED1 &&
              TLB_COMPARE_MISMATCH == TL_CMP_MISMATCH && TLB_COMPARE_SWAPPED == TL_CMP_SWAPPED && TLB_COMPARE_SKIPPED == TL_CMP_SKIPPED, "delay and flags");

int compare_prepare(tlb_batch *b)
{
    if (b->d_cmp_hist) return TLB_OK;
    HIPCHK(hipSetDevice(b->device));
    TlbMem m;
    int16_t *h = m.dev<int16_t>(2 * TL_CMP_HIST * (size_t)b->nstreams);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_cmp_hist = h;
    return TLB_OK;
}

int compare_launch(tlb_batch *b, const int16_t *d_in_pcm, const int16_t *d_dec_pcm, const tlb_frame_report *d_report, int nframes,
                   const tlb_compare_params *params, tlb_compare_record *d_record, void *hip_stream)
{
    if (!b || !d_dec_pcm || !d_record || !tlb_compare_params_legal(params) || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (!d_in_pcm && nframes != 1) return TLB_ERR_ARG;
    if ((((uintptr_t)d_in_pcm | (uintptr_t)d_dec_pcm) & 15u) || ((uintptr_t)d_report & 3u) || ((uintptr_t)d_record & 7u)) return TLB_ERR_ARG;      // the kernel moves 16-byte pieces of PCM
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    if (int rc = compare_prepare(b)) return rc;
    HIPCHK(hipSetDevice(b->device));
    TlCompareParams P;
    P.min_energy = params->min_energy; P.corr_num = params->corr_num; P.corr_den = params->corr_den;
    HIPCHK(tlk_compare((hipStream_t)hip_stream, d_in_pcm, d_dec_pcm, (const TlFrameReport *)d_report, b->d_cmp_hist, (TlCompareRecord *)d_record, P,
                       b->d_configs, b->d_stream_cfg, b->nstreams, nframes));
    return TLB_OK;
}

extern "C" {

int tlb_compare_device(tlb_batch *b, const int16_t *d_in_pcm, const int16_t *d_dec_pcm, const tlb_frame_report *d_report, int nframes,
                       const tlb_compare_params *params, tlb_compare_record *d_record, void *hip_stream)
{
    if (!d_report) return TLB_ERR_ARG;
    return compare_launch(b, d_in_pcm, d_dec_pcm, d_report, nframes, params, d_record, hip_stream);
}

int tlb_compare_host(tlb_batch *b, const int16_t *in_pcm, const int16_t *dec_pcm, const tlb_frame_report *report, int nframes,
                     const tlb_compare_params *params, tlb_compare_record *record)
{
    if (!b || !dec_pcm || !report || !record || !tlb_compare_params_legal(params) || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if ((!in_pcm && nframes != 1) || (((uintptr_t)in_pcm | (uintptr_t)dec_pcm) & 1u) || ((uintptr_t)report & 3u) || ((uintptr_t)record & 7u)) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams, rec_bytes = (size_t)b->nstreams * sizeof(tlb_compare_record);
    const size_t pcm_bytes = slots * 2 * TLB_SAMPLES_PER_FRAME * sizeof(int16_t);
    TlbMem m;
    tlb_frame_report *d_report = m.scratch<tlb_frame_report>(slots); tlb_compare_record *d_record = m.scratch<tlb_compare_record>((size_t)b->nstreams);
    int16_t *d_dec = m.scratch<int16_t>(pcm_bytes / 2), *d_in = in_pcm ? m.scratch<int16_t>(pcm_bytes / 2) : nullptr;
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_report, report, slots * sizeof(tlb_frame_report), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_record, record, rec_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_dec, dec_pcm, pcm_bytes, hipMemcpyHostToDevice));
    if (in_pcm) HIPCHK(hipMemcpy(d_in, in_pcm, pcm_bytes, hipMemcpyHostToDevice));
    if (int rc = tlb_compare_device(b, d_in, d_dec, d_report, nframes, params, d_record, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(record, d_record, rec_bytes, hipMemcpyDeviceToHost));
    return TLB_OK;
}

int tlb_compare_reset(tlb_batch *b, int stream)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    if (!b->d_cmp_hist) return TLB_OK;           // never compared: every history is zeros already
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    const size_t one = sizeof(int16_t) * 2 * TL_CMP_HIST;
    if (stream < 0) HIPCHK(hipMemset(b->d_cmp_hist, 0, one * (size_t)b->nstreams));
    else HIPCHK(hipMemset(b->d_cmp_hist + (size_t)stream * 2 * TL_CMP_HIST, 0, one));
    return TLB_OK;
}

}  // extern "C"
