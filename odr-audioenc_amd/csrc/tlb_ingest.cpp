// tlb_ingest.cpp -- the caller's glue of include/toolame_batch.h (tlb_set_gain_db, tlb_ingest_*, tlb_silence_*, tlb_underrun_*): argument
// checks and one launch of a kernel of toolame_ingest.hip through tl_kernels.h, and the host-buffer forms' round trips.  Host C++.  The rules
// themselves are csrc/mp2_ingest.h.
#include "tlb_internal.h"

// gain, peak and de-interleave of nframes x nstreams slots; d_valid int32 [nframes][nstreams], the whole sample frames each slot delivers, or
// NULL: every slot is a full read (tl_ingest_kernel, which loads no such word)
static int ingest_launch(tlb_batch *b, const int16_t *d_interleaved, const int32_t *d_valid, int nframes, int16_t *d_pcm, int16_t *d_peaks, void *hip_stream)
{
    if (!b || !d_interleaved || !d_pcm || !d_peaks || nframes <= 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_ingest((unsigned)((size_t)nframes * (size_t)b->nstreams), (hipStream_t)hip_stream, d_interleaved, d_valid, d_pcm, d_peaks, b->d_gain, b->d_configs, b->d_stream_cfg, b->nstreams));
    return TLB_OK;
}

// ... from and to host buffers: device staging kept between calls, like tlb_encode_host (an application calls this once per chunk of frames)
static int ingest_host(tlb_batch *b, const int16_t *interleaved, const int32_t *valid, int nframes, int16_t *pcm, int16_t *peaks)
{
    if (!b || !interleaved || !pcm || !peaks || nframes <= 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams;
    HIPCHK(stage_reserve(b, TLB_STAGE_INGEST_IN, slots * 2304 * 2));
    HIPCHK(stage_reserve(b, TLB_STAGE_INGEST_OUT, slots * 2304 * 2));
    HIPCHK(stage_reserve(b, TLB_STAGE_INGEST_PEAKS, slots * 2 * 2));
    int16_t *d_in = (int16_t *)b->stage[TLB_STAGE_INGEST_IN], *d_out = (int16_t *)b->stage[TLB_STAGE_INGEST_OUT], *d_pk = (int16_t *)b->stage[TLB_STAGE_INGEST_PEAKS];
    TlbMem m;
    int32_t *d_valid = valid ? m.scratch<int32_t>(slots) : nullptr;
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_in, interleaved, slots * 2304 * 2, hipMemcpyHostToDevice));
    if (valid) HIPCHK(hipMemcpy(d_valid, valid, slots * sizeof(int32_t), hipMemcpyHostToDevice));
    int rc = ingest_launch(b, d_in, d_valid, nframes, d_out, d_pk, nullptr);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(pcm, d_out, slots * 2304 * 2, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(peaks, d_pk, slots * 2 * 2, hipMemcpyDeviceToHost));
    return rc;
}

// The round trip of the two counter calls' host forms: a per-slot array of `slot_bytes` a slot and one or two per-stream counters up, the
// launch (queue(d_slots, d_c0, d_c1) on the null stream), the counters down.  The device is waited for before any buffer is released.
template <class Queue>
static int counters_host(tlb_batch *b, const void *per_slot, size_t slot_bytes, int nframes, uint32_t *c0, uint32_t *c1, Queue queue)
{
    HIPCHK(hipSetDevice(b->device));
    const size_t in_bytes = (size_t)nframes * (size_t)b->nstreams * slot_bytes, n = (size_t)b->nstreams;
    TlbMem m;
    uint8_t *d_slots = m.scratch<uint8_t>(in_bytes);
    uint32_t *d_c0 = m.scratch<uint32_t>(n), *d_c1 = c1 ? m.scratch<uint32_t>(n) : nullptr;
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_slots, per_slot, in_bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_c0, c0, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    if (c1) HIPCHK(hipMemcpy(d_c1, c1, sizeof(uint32_t) * n, hipMemcpyHostToDevice));
    int rc = queue(d_slots, d_c0, d_c1);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(c0, d_c0, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    if (c1) HIPCHK(hipMemcpy(c1, d_c1, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
    return rc;
}

extern "C" {

int tlb_set_gain_db(tlb_batch *b, int stream, double gain_db)
{   // const double linear_gain_correction = pow(10.0, gain_dB / 20.0);  (src/odr-audioenc.cpp:1032)
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const double g = pow(10.0, gain_db / 20.0);
    for (int s2 = 0; s2 < b->nstreams; s2++) if (stream < 0 || s2 == stream) b->h_gain[(size_t)s2] = g;
    HIPCHK(hipMemcpy(b->d_gain, b->h_gain.data(), sizeof(double) * (size_t)b->nstreams, hipMemcpyHostToDevice));
    return TLB_OK;
}

// Ingest (csrc/mp2_ingest.h); the _valid forms take short reads, and without the array they ARE the plain forms -- the same kernel, the same launch
int tlb_ingest_device(tlb_batch *b, const int16_t *d_interleaved, int nframes, int16_t *d_pcm, int16_t *d_peaks, void *hip_stream)
{
    return ingest_launch(b, d_interleaved, nullptr, nframes, d_pcm, d_peaks, hip_stream);
}
int tlb_ingest_device_valid(tlb_batch *b, const int16_t *d_interleaved, const int32_t *d_valid, int nframes, int16_t *d_pcm, int16_t *d_peaks, void *hip_stream)
{
    return ingest_launch(b, d_interleaved, d_valid, nframes, d_pcm, d_peaks, hip_stream);
}
int tlb_ingest_host(tlb_batch *b, const int16_t *interleaved, int nframes, int16_t *pcm, int16_t *peaks) { return ingest_host(b, interleaved, nullptr, nframes, pcm, peaks); }
int tlb_ingest_host_valid(tlb_batch *b, const int16_t *interleaved, const int32_t *valid, int nframes, int16_t *pcm, int16_t *peaks)
{
    return ingest_host(b, interleaved, valid, nframes, pcm, peaks);
}

// Underrun bookkeeping of the caller (src/odr-audioenc.cpp:919-935; tl_underrun_stream): the 60-second decision stays with the caller
int tlb_underrun_device(tlb_batch *b, const int32_t *d_valid, int nframes, uint32_t *d_underrun_ms, uint32_t *d_underruns, void *hip_stream)
{
    if (!b || !d_valid || !d_underrun_ms || !d_underruns || nframes <= 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_underrun((unsigned)((b->nstreams + 255) / 256), (hipStream_t)hip_stream, d_valid, d_underrun_ms, d_underruns, b->d_configs, b->d_stream_cfg, b->nstreams, nframes));
    return TLB_OK;
}
int tlb_underrun_host(tlb_batch *b, const int32_t *valid, int nframes, uint32_t *underrun_ms, uint32_t *underruns)
{
    if (!b || !valid || !underrun_ms || !underruns || nframes <= 0) return TLB_ERR_ARG;
    return counters_host(b, valid, sizeof(int32_t), nframes, underrun_ms, underruns, [&](const void *d_v, uint32_t *d_ms, uint32_t *d_n) {
        return tlb_underrun_device(b, (const int32_t *)d_v, nframes, d_ms, d_n, nullptr); });
}

// Silence accounting of the caller (src/odr-audioenc.cpp:1053-1079; tl_silence_stream): the decision stays with the caller
int tlb_silence_device(tlb_batch *b, const int16_t *d_peaks, int nframes, uint32_t *d_silence_ms, void *hip_stream)
{
    if (!b || !d_peaks || !d_silence_ms || nframes <= 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_silence((unsigned)((b->nstreams + 255) / 256), (hipStream_t)hip_stream, d_peaks, d_silence_ms, b->d_configs, b->d_stream_cfg, b->nstreams, nframes));
    return TLB_OK;
}
int tlb_silence_host(tlb_batch *b, const int16_t *peaks, int nframes, uint32_t *silence_ms)
{
    if (!b || !peaks || !silence_ms || nframes <= 0) return TLB_ERR_ARG;
    return counters_host(b, peaks, 2 * sizeof(int16_t), nframes, silence_ms, nullptr, [&](const void *d_p, uint32_t *d_ms, uint32_t *) {
        return tlb_silence_device(b, (const int16_t *)d_p, nframes, d_ms, nullptr); });
}

}  // extern "C"
