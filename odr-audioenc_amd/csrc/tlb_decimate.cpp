// tlb_decimate.cpp -- the batch-level entry points of the device decimator (include/toolame_batch.h, tlb_decimate_*): the committed tables,
// the need arithmetic (host only), the per-stream state (allocated by the first tlb_decimate_set_source) and one launch of the kernel of
// toolame_decimate.hip through tl_kernels.h.  Host C++.  The tick plane (tlb_tick.cpp) queues it between its group's copy-in and ingest.
#include "tlb_internal.h"
#include "tlb_plan.h"
#include "tl_decimate_taps.inc"

#include <assert.h>

static_assert(sizeof tl_decimate_taps_80_147 == 80 * TL_DC_TAPS * 2 && sizeof tl_decimate_taps_3_4 == 3 * TL_DC_TAPS * 2 && sizeof tl_decimate_taps_1_2 == TL_DC_TAPS * 2, "table shapes");
static_assert(TLB_DECIMATE_TAPS == TL_DC_TAPS && TLB_DECIMATE_SLOT == TL_DC_SLOT, "taps per phase, wide slot");

// S(f) = ceil(1152 f M / L): source frames consumed before frame f; need(f) = S(f + 1) - S(f)
static int need_of(int ratio, long frame)
{
    const long long L = tl_dc_L(ratio), M = tl_dc_M(ratio), f = frame % tl_dc_cycle(ratio);      // the phase repeats with the cycle
    return (int)((1152 * (f + 1) * M + L - 1) / L - (1152 * f * M + L - 1) / L);
}
static const int16_t *table_of(int ratio) { return ratio == TL_DC_80_147 ? &tl_decimate_taps_80_147[0][0] : ratio == TL_DC_3_4 ? &tl_decimate_taps_3_4[0][0] : &tl_decimate_taps_1_2[0][0]; }

bool decimate_rate_fits(const tlb_batch *b, int stream, long rate)
{
    const long src = b->dc_rate.empty() ? 0 : b->dc_rate[(size_t)stream];
    return src == 0 || tl_dc_ratio_of(src, rate) != TL_DC_OFF;
}

int decimate_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_dc_state) return TLB_OK;
    for (int k = 0; k < 2; k++)
        HIPCHK(hipMemset(b->d_dc_state + ((size_t)k * (size_t)b->nstreams + (size_t)s0) * TL_DC_STATE_WORDS, 0, sizeof(uint32_t) * TL_DC_STATE_WORDS * (size_t)n));
    for (int s = s0; s < s0 + n; s++) b->dc_pos[(size_t)s] = 0;
    return TLB_OK;
}

int16_t *decimate_taps_upload(TlbMem &m)
{
    int16_t *tp = m.scratch<int16_t>(TL_DC_TABLE_ROWS * TL_DC_TAPS);
    for (int r = TL_DC_80_147; r <= TL_DC_1_2; r++) m.upload(tp + tl_dc_first_row(r) * TL_DC_TAPS, table_of(r), sizeof(int16_t) * TL_DC_TAPS * (size_t)tl_dc_L(r));
    return tp;
}

int decimate_prepare(tlb_batch *b)
{
    if (b->d_dc_state) return TLB_OK;
    const size_t ns = (size_t)b->nstreams;
    TlbMem m;
    uint32_t *st = m.dev<uint32_t>(2 * TL_DC_STATE_WORDS * ns);
    int32_t *ra = m.dev<int32_t>(ns);
    int16_t *tp = decimate_taps_upload(m);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->dc_rate.assign(ns, 0); b->dc_ratio.assign(ns, TL_DC_OFF); b->dc_pos.assign(ns, 0);
    b->d_dc_state = st; b->d_dc_ratio = ra; b->d_dc_taps = tp; b->dc_flip = 0;
    return TLB_OK;
}

extern "C" {

const int16_t *tlb_decimate_taps(long source_rate, long encoder_rate, int *L, int *M, int *T)
{
    const int ratio = tl_dc_ratio_of(source_rate, encoder_rate);
    if (ratio == TL_DC_OFF) return nullptr;
    if (L) *L = tl_dc_L(ratio);
    if (M) *M = tl_dc_M(ratio);
    if (T) *T = TL_DC_TAPS;
    return table_of(ratio);
}

int tlb_decimate_need_at(long source_rate, long encoder_rate, long frame)
{
    const int ratio = tl_dc_ratio_of(source_rate, encoder_rate);
    if (ratio == TL_DC_OFF) return -TLB_ERR_SAMPLERATE;
    if (frame < 0) return -TLB_ERR_ARG;
    return need_of(ratio, frame);
}

int tlb_decimate_set_source(tlb_batch *b, int stream, long source_rate)
{
    if (!b || stream < -1 || stream >= b->nstreams || source_rate < 0) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b->nstreams : stream + 1;
    bool any = false;
    if (int rc = tlb_rate_range(s0, s1, source_rate, tlb_down_pair, [b](int s) { return batch_enc_rate(b, s); }, &any)) return rc;
    for (int s = s0; any && s < s1; s++)                             // a stream has one source (csrc/tlb_inputs.h)
        if (tlb_down_pair(source_rate, batch_enc_rate(b, s)) && !batch_may_set(b, s, TLB_IN_DOWN_SOURCE)) return TLB_ERR_ARG;
    if (!any && !b->d_dc_state) return TLB_OK;                       // off, and never on: nothing to allocate or to clear
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = decimate_prepare(b)) return rc;
    std::vector<int32_t> ratio((size_t)(s1 - s0));
    for (int s = s0; s < s1; s++) ratio[(size_t)(s - s0)] = tl_dc_ratio_of(source_rate, batch_enc_rate(b, s));
    HIPCHK(hipMemcpy(b->d_dc_ratio + s0, ratio.data(), sizeof(int32_t) * ratio.size(), hipMemcpyHostToDevice));
    for (int s = s0; s < s1; s++) {
        b->dc_ratio[(size_t)s] = ratio[(size_t)(s - s0)];
        b->dc_rate[(size_t)s] = ratio[(size_t)(s - s0)] == TL_DC_OFF ? 0 : source_rate;
    }
    return decimate_clear_streams(b, s0, s1 - s0);
}

long tlb_decimate_source(const tlb_batch *b, int stream)
{
    if (!b || stream < 0 || stream >= b->nstreams || b->dc_rate.empty()) return 0;
    return b->dc_rate[(size_t)stream];
}

int tlb_decimate_need(const tlb_batch *b, int stream, int ahead)
{
    if (!b || stream < 0 || stream >= b->nstreams || ahead < 0) return -TLB_ERR_ARG;
    if (b->dc_ratio.empty() || b->dc_ratio[(size_t)stream] == TL_DC_OFF) return TLB_SAMPLES_PER_FRAME;
    return need_of(b->dc_ratio[(size_t)stream], (long)b->dc_pos[(size_t)stream] + ahead);
}

int tlb_decimate_device(tlb_batch *b, const int16_t *d_wide, int nframes, int16_t *d_interleaved, void *hip_stream)
{
    if (!b || !d_wide || !d_interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if ((((uintptr_t)d_wide | (uintptr_t)d_interleaved) & 15u)) return TLB_ERR_ARG;                      // the source frames come in as 16-byte pieces
    const size_t slots = (size_t)nframes * (size_t)b->nstreams, wbytes = slots * TL_DC_SLOT * sizeof(int16_t), obytes = slots * 2304 * sizeof(int16_t);
    const uintptr_t a = (uintptr_t)d_wide, o = (uintptr_t)d_interleaved;
    if (a < o + obytes && o < a + wbytes) return TLB_ERR_ARG;        // a slot's history is read from the slot before it: the buffers must not overlap
    if (b->broken) return TLB_ERR_HIP;
    if (!b->d_dc_state) return TLB_OK;                               // no stream has ever had a down source: every slot is left alone, nothing to queue
    for (int s = 0; s < b->nstreams; s++) assert(b->dc_ratio[(size_t)s] == TL_DC_OFF || tlb_resample_source(b, s) == 0);      // one source per stream
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_decimate((unsigned)slots, (hipStream_t)hip_stream, d_wide, d_interleaved, b->d_dc_state, b->d_dc_ratio, b->d_dc_taps, b->d_configs, b->d_stream_cfg,
                        b->nstreams, nframes, b->dc_flip));
    b->dc_flip ^= 1;
    for (int s = 0; s < b->nstreams; s++)
        if (b->dc_ratio[(size_t)s] != TL_DC_OFF) b->dc_pos[(size_t)s] = (int32_t)(((long long)b->dc_pos[(size_t)s] + nframes) % tl_dc_cycle(b->dc_ratio[(size_t)s]));
    return TLB_OK;
}

int tlb_decimate_host(tlb_batch *b, const int16_t *wide, int nframes, int16_t *interleaved)
{
    if (!b || !wide || !interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams, wbytes = slots * TL_DC_SLOT * sizeof(int16_t), obytes = slots * 2304 * sizeof(int16_t);
    TlbMem m;
    int16_t *d_in = m.scratch<int16_t>(wbytes / 2), *d_out = m.scratch<int16_t>(obytes / 2);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_in, wide, wbytes, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_out, interleaved, obytes, hipMemcpyHostToDevice));      // what the kernel does not write (streams without a down source, behind a one-channel stream's 1152 samples) stays the caller's
    if (int rc = tlb_decimate_device(b, d_in, nframes, d_out, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(interleaved, d_out, obytes, hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
