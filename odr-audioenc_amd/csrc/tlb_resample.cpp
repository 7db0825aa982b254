// tlb_resample.cpp -- the batch-level entry points of the device resampler (include/toolame_batch.h, tlb_resample_*): the committed tables,
// the need arithmetic (host only), the per-stream state (allocated by the first tlb_resample_set_source) and one launch of the kernel of
// toolame_resample.hip through tl_kernels.h.  Host C++.  The tick plane (tlb_tick.cpp) queues it between its group's copy-in and ingest.
#include "tlb_internal.h"
#include "tlb_plan.h"
#include "tl_resample_taps.inc"

static_assert(sizeof tl_resample_taps_160_147 == 160 * TL_RS_TAPS * 2 && sizeof tl_resample_taps_3_2 == 3 * TL_RS_TAPS * 2, "table shapes");
static_assert(TLB_RESAMPLE_TAPS == TL_RS_TAPS, "taps per phase");

static void ratio_lm(int ratio, long *L, long *M) { *L = ratio == TL_RS_160_147 ? 160 : 3; *M = ratio == TL_RS_160_147 ? 147 : 2; }
// source frames frame `frame` (counted from the reset) consumes: q(1152 (f + 1) - 1) + 1 - (f > 0 ? q(1152 f - 1) + 1 : 0)
static int need_of(int ratio, long frame)
{
    long L, M;
    ratio_lm(ratio, &L, &M);
    const long long f = frame % tl_rs_cycle(ratio);                  // the phase repeats with the cycle
    const long long hi = (1152 * (f + 1) - 1) * M / L + 1, lo = f > 0 ? (1152 * f - 1) * M / L + 1 : 0;
    return (int)(hi - lo);
}

bool resample_rate_fits(const tlb_batch *b, int stream, long rate)
{
    const long src = b->rs_rate.empty() ? 0 : b->rs_rate[(size_t)stream];
    return src == 0 || tl_rs_ratio_of(src, rate) != TL_RS_OFF;
}

int resample_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_rs_state) return TLB_OK;
    for (int k = 0; k < 2; k++)
        HIPCHK(hipMemset(b->d_rs_state + ((size_t)k * (size_t)b->nstreams + (size_t)s0) * TL_RS_STATE_WORDS, 0, sizeof(uint32_t) * TL_RS_STATE_WORDS * (size_t)n));
    for (int s = s0; s < s0 + n; s++) b->rs_pos[(size_t)s] = 0;
    return TLB_OK;
}

int16_t *resample_taps_upload(TlbMem &m)
{
    int16_t *tp = m.scratch<int16_t>((160 + 3) * TL_RS_TAPS);
    m.upload(tp, tl_resample_taps_160_147, sizeof tl_resample_taps_160_147);
    m.upload(tp + 160 * TL_RS_TAPS, tl_resample_taps_3_2, sizeof tl_resample_taps_3_2);
    return tp;
}

int resample_prepare(tlb_batch *b)
{
    if (b->d_rs_state) return TLB_OK;
    const size_t ns = (size_t)b->nstreams;
    TlbMem m;
    uint32_t *st = m.dev<uint32_t>(2 * TL_RS_STATE_WORDS * ns);
    int32_t *ra = m.dev<int32_t>(ns);
    int16_t *tp = resample_taps_upload(m);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->rs_rate.assign(ns, 0); b->rs_ratio.assign(ns, TL_RS_OFF); b->rs_pos.assign(ns, 0);
    b->d_rs_state = st; b->d_rs_ratio = ra; b->d_rs_taps = tp; b->rs_flip = 0;
    return TLB_OK;
}

extern "C" {

const int16_t *tlb_resample_taps(long source_rate, long encoder_rate, int *L, int *M, int *T)
{
    const int ratio = tl_rs_ratio_of(source_rate, encoder_rate);
    if (ratio == TL_RS_OFF) return nullptr;
    long l, m;
    ratio_lm(ratio, &l, &m);
    if (L) *L = (int)l;
    if (M) *M = (int)m;
    if (T) *T = TL_RS_TAPS;
    return ratio == TL_RS_160_147 ? &tl_resample_taps_160_147[0][0] : &tl_resample_taps_3_2[0][0];
}

int tlb_resample_need_at(long source_rate, long encoder_rate, long frame)
{
    const int ratio = tl_rs_ratio_of(source_rate, encoder_rate);
    if (ratio == TL_RS_OFF) return -TLB_ERR_SAMPLERATE;
    if (frame < 0) return -TLB_ERR_ARG;
    return need_of(ratio, frame);
}

int tlb_resample_set_source(tlb_batch *b, int stream, long source_rate)
{
    if (!b || stream < -1 || stream >= b->nstreams || source_rate < 0) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b->nstreams : stream + 1;
    bool any = false;
    if (int rc = tlb_rate_range(s0, s1, source_rate, tlb_up_pair, [b](int s) { return batch_enc_rate(b, s); }, &any)) return rc;
    for (int s = s0; any && s < s1; s++)                             // a stream has one source (csrc/tlb_inputs.h)
        if (tlb_up_pair(source_rate, batch_enc_rate(b, s)) && !batch_may_set(b, s, TLB_IN_UP_SOURCE)) return TLB_ERR_ARG;
    if (!any && !b->d_rs_state) return TLB_OK;                       // off, and never on: nothing to allocate or to clear
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = resample_prepare(b)) return rc;
    std::vector<int32_t> ratio((size_t)(s1 - s0));
    for (int s = s0; s < s1; s++) ratio[(size_t)(s - s0)] = tl_rs_ratio_of(source_rate, batch_enc_rate(b, s));
    HIPCHK(hipMemcpy(b->d_rs_ratio + s0, ratio.data(), sizeof(int32_t) * ratio.size(), hipMemcpyHostToDevice));
    for (int s = s0; s < s1; s++) {
        b->rs_ratio[(size_t)s] = ratio[(size_t)(s - s0)];
        b->rs_rate[(size_t)s] = ratio[(size_t)(s - s0)] == TL_RS_OFF ? 0 : source_rate;
    }
    return resample_clear_streams(b, s0, s1 - s0);
}

long tlb_resample_source(const tlb_batch *b, int stream)
{
    if (!b || stream < 0 || stream >= b->nstreams || b->rs_rate.empty()) return 0;
    return b->rs_rate[(size_t)stream];
}

int tlb_resample_need(const tlb_batch *b, int stream, int ahead)
{
    if (!b || stream < 0 || stream >= b->nstreams || ahead < 0) return -TLB_ERR_ARG;
    if (b->rs_ratio.empty() || b->rs_ratio[(size_t)stream] == TL_RS_OFF) return TLB_SAMPLES_PER_FRAME;
    return need_of(b->rs_ratio[(size_t)stream], (long)b->rs_pos[(size_t)stream] + ahead);
}

int tlb_resample_device(tlb_batch *b, const int16_t *d_source, int nframes, int16_t *d_interleaved, void *hip_stream)
{
    if (!b || !d_source || !d_interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if ((((uintptr_t)d_source | (uintptr_t)d_interleaved) & 15u)) return TLB_ERR_ARG;                    // a slot without a source moves as 16-byte pieces
    const size_t slots = (size_t)nframes * (size_t)b->nstreams, bytes = slots * 2304 * sizeof(int16_t);
    const uintptr_t a = (uintptr_t)d_source, o = (uintptr_t)d_interleaved;
    if (a < o + bytes && o < a + bytes) return TLB_ERR_ARG;          // a slot's history is read from the slot before it: the buffers must not overlap
    if (b->broken) return TLB_ERR_HIP;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_resample((unsigned)slots, (hipStream_t)hip_stream, d_source, d_interleaved, b->d_rs_state, b->d_rs_ratio, b->d_rs_taps, b->d_configs, b->d_stream_cfg,
                        b->nstreams, nframes, b->rs_flip));
    if (b->d_rs_state) {
        b->rs_flip ^= 1;
        for (int s = 0; s < b->nstreams; s++)
            if (b->rs_ratio[(size_t)s] != TL_RS_OFF) b->rs_pos[(size_t)s] = (int32_t)(((long long)b->rs_pos[(size_t)s] + nframes) % tl_rs_cycle(b->rs_ratio[(size_t)s]));
    }
    return TLB_OK;
}

int tlb_resample_host(tlb_batch *b, const int16_t *source, int nframes, int16_t *interleaved)
{
    if (!b || !source || !interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t bytes = (size_t)nframes * (size_t)b->nstreams * 2304 * sizeof(int16_t);
    TlbMem m;
    int16_t *d_in = m.scratch<int16_t>(bytes / 2), *d_out = m.scratch<int16_t>(bytes / 2);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_in, source, bytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out, interleaved, bytes, hipMemcpyHostToDevice));       // what the kernel does not write (behind a one-channel stream's 1152 samples) stays the caller's
    if (int rc = tlb_resample_device(b, d_in, nframes, d_out, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(interleaved, d_out, bytes, hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
