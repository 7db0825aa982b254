// tlb_limiter.cpp -- the batch-level entry points of the true-peak limiter (include/toolame_batch.h, tlb_limiter_*): the parameters, the
// per-stream state and steps (allocated by tlb_limiter_enable alone) and one launch of the kernel of toolame_limiter.hip through
// tl_kernels.h.  Host C++.
#include <stddef.h>
#include "tlb_internal.h"
#include "tl_truepeak_taps.inc"

static_assert(sizeof(tlb_limiter_record) == sizeof(TlLimiterRecord) && sizeof(tlb_limiter_record) == 32, "C-ABI record");
static_assert(offsetof(tlb_limiter_record, frames) == offsetof(TlLimiterRecord, frames) && offsetof(tlb_limiter_record, limited) == offsetof(TlLimiterRecord, limited) &&
              offsetof(tlb_limiter_record, samples) == offsetof(TlLimiterRecord, samples) && offsetof(tlb_limiter_record, red_last) == offsetof(TlLimiterRecord, red_last) &&
              offsetof(tlb_limiter_record, red_max) == offsetof(TlLimiterRecord, red_max) && offsetof(tlb_limiter_record, peak_in) == offsetof(TlLimiterRecord, peak_in) &&
              offsetof(tlb_limiter_record, peak_in_max) == offsetof(TlLimiterRecord, peak_in_max) && offsetof(tlb_limiter_record, reserved) == offsetof(TlLimiterRecord, reserved), "record layout");
static_assert(TLB_LIMITER_WMIN == TL_LM_WMIN && TLB_LIMITER_WBOX == TL_LM_WBOX && TLB_LIMITER_DELAY == TL_LM_DELAY, "the definition's constants");

// the parameters with their defaults filled in; false: not legal
static bool limiter_params_resolve(const tlb_limiter_params *p, tlb_limiter_params *out)
{
    out->ceiling = p && p->ceiling ? p->ceiling : TLB_TRUEPEAK_CEILING_DEFAULT;
    out->release_ms = p && p->release_ms ? p->release_ms : TLB_LIMITER_RELEASE_DEFAULT_MS;
    return out->ceiling >= (1u << 20) && out->ceiling <= (1u << 30) && out->release_ms >= 1u && out->release_ms <= 10000u;
}

// S of streams [s0, s0 + n) from their encoder rates, host to device
static int limiter_steps(tlb_batch *b, int s0, int n)
{
    std::vector<uint32_t> step((size_t)n);
    for (int k = 0; k < n; k++) step[(size_t)k] = tlb_limiter_step(b->lm_params.release_ms, batch_enc_rate(b, s0 + k));
    HIPCHK(hipMemcpy(b->d_lm_step + s0, step.data(), (size_t)n * sizeof(uint32_t), hipMemcpyHostToDevice));
    return TLB_OK;
}

// the limiter's state of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle), and their steps from the rates they
// have now (tlb_stream_reconfigure)
int limiter_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_lm_rec) return TLB_OK;
    HIPCHK(hipMemset(b->d_lm_rec + s0, 0, (size_t)n * sizeof(TlLimiterRecord)));
    HIPCHK(hipMemset(b->d_lm_state + (size_t)s0 * TL_LM_STATE, 0, (size_t)n * TL_LM_STATE * sizeof(uint32_t)));
    if (int rc = limiter_steps(b, s0, n)) return rc;
    HIPCHK(hipDeviceSynchronize());              // the callers' streams do not wait for the null stream
    return TLB_OK;
}

extern "C" {

uint32_t tlb_limiter_step(uint32_t release_ms, long samplerate)
{
    if (!release_ms) release_ms = TLB_LIMITER_RELEASE_DEFAULT_MS;
    if (release_ms > 10000u || samplerate <= 0) return 0u;
    const uint64_t s = ((uint64_t)1 << 30) * 1000u / ((uint64_t)release_ms * (uint64_t)samplerate);
    return s < 1u ? 1u : s > (1u << 30) ? (1u << 30) : (uint32_t)s;
}

int tlb_limiter_enable(tlb_batch *b, const tlb_limiter_params *params)
{
    tlb_limiter_params p;
    if (!b || !limiter_params_resolve(params, &p)) return TLB_ERR_ARG;
    if (b->d_lm_rec) return p.ceiling == b->lm_params.ceiling && p.release_ms == b->lm_params.release_ms ? (int)TLB_OK : (int)TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t ns = (size_t)b->nstreams;
    std::vector<uint32_t> step(ns);
    for (size_t s = 0; s < ns; s++) step[s] = tlb_limiter_step(p.release_ms, batch_enc_rate(b, (int)s));
    TlbMem m;
    TlLimiterRecord *rec = m.dev<TlLimiterRecord>(ns);
    uint32_t *state = m.dev<uint32_t>(TL_LM_STATE * ns);
    uint32_t *d_step = m.scratch<uint32_t>(ns);
    int16_t *taps = m.scratch<int16_t>(3 * TL_TP_TAPS);
    m.upload(d_step, step.data(), ns * sizeof(uint32_t));
    m.upload(taps, tl_truepeak_taps, sizeof tl_truepeak_taps);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_lm_rec = rec; b->d_lm_state = state; b->d_lm_step = d_step; b->d_lm_taps = taps;
    b->lm_params = p;
    return TLB_OK;
}

int tlb_limiter_device(tlb_batch *b, int16_t *d_pcm_planar, int nframes, tlb_limiter_record *d_records, void *hip_stream)
{
    if (!b || !d_pcm_planar || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (((uintptr_t)d_pcm_planar & 15u) || ((uintptr_t)d_records & 3u)) return TLB_ERR_ARG;      // the PCM comes in and goes out as 16-byte pieces
    if (!b->d_lm_rec) return TLB_ERR_ARG;        // never enabled
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    HIPCHK(hipSetDevice(b->device));
    const TlLimiterArgs A = {d_pcm_planar, b->d_lm_rec, (TlLimiterRecord *)d_records, b->d_lm_state, b->d_lm_step, b->d_lm_taps, b->d_configs, b->d_stream_cfg,
                             b->lm_params.ceiling, b->nstreams, nframes};
    HIPCHK(tlk_limiter((hipStream_t)hip_stream, A));
    return TLB_OK;
}

// (not meter_host: the PCM comes back too)
int tlb_limiter_host(tlb_batch *b, int16_t *pcm_planar, int nframes, tlb_limiter_record *records)
{
    if (!b || !pcm_planar || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30) || !b->d_lm_rec) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t vals = (size_t)nframes * (size_t)b->nstreams * 2 * TLB_SAMPLES_PER_FRAME;
    TlbMem m;
    int16_t *d_pcm = m.scratch<int16_t>(vals);
    tlb_limiter_record *d_rec = m.scratch<tlb_limiter_record>((size_t)b->nstreams);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_pcm, pcm_planar, vals * sizeof(int16_t), hipMemcpyHostToDevice));
    if (int rc = tlb_limiter_device(b, d_pcm, nframes, d_rec, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pcm_planar, d_pcm, vals * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (records) HIPCHK(hipMemcpy(records, d_rec, (size_t)b->nstreams * sizeof(tlb_limiter_record), hipMemcpyDeviceToHost));
    return TLB_OK;
}

int tlb_limiter_reset(tlb_batch *b, int stream) { return meter_reset(b, b ? b->d_lm_rec : nullptr, stream, limiter_clear_streams); }

}  // extern "C"
