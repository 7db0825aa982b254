// tlb_feed_down.cpp -- the batch-level entry points of the DOWN FEEDS (include/toolame_batch.h, tlb_feed_down_*): a 48, 44.1 or 32 kHz
// Layer II feed for a 24 kHz stream.  The schedule (host only), the per-stream feed table, history, queue heads and positions (allocated by
// the first tlb_feed_down_set), the call-sized source plane and one launch of the three kernels of toolame_feed_down.hip through
// tl_kernels.h.  Host C++.  A family of its own beside tlb_feed_* (csrc/tlb_feed.cpp), which it leaves as it is: it shares that family's
// legality check and record builder, the FeedTable type (csrc/tlb_internal.h) and the decimator's committed tables -- the records, history
// and reports themselves are its own.
#include "tlb_internal.h"

int feed_down_fits(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg)
{
    if (int rc = tlb_feed_check_config(cfg)) return rc;
    for (int s = s0; s < s1; s++) if (tl_fd_ratio_of(cfg->samplerate, batch_enc_rate(b, s)) == TL_DC_OFF) return TLB_ERR_SAMPLERATE;
    return TLB_OK;
}

int feed_down_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_fd_state) return TLB_OK;
    HIPCHK(hipMemset(b->d_fd_state + s0, 0, sizeof(TlDecStream) * (size_t)n));
    for (int k = 0; k < 2; k++) {                                    // the streams' next tick is tick 0 and their queue is empty
        HIPCHK(hipMemset(b->d_fd_carry + ((size_t)k * (size_t)b->nstreams + (size_t)s0) * (TL_FD_CARRY * 2), 0, sizeof(int16_t) * TL_FD_CARRY * 2 * (size_t)n));
        HIPCHK(hipMemset(b->d_fd_pos + (size_t)k * (size_t)b->nstreams + (size_t)s0, 0, sizeof(int32_t) * (size_t)n));
    }
    for (int s = s0; s < s0 + n; s++) b->fd_pos[(size_t)s] = 0;
    return conceal_clear_family(b, s0, n, true);                     // a stream's concealment starts again with its history (G, run, record)
}

// room for `frames` ticks per stream in the source plane: grow-only launch scratch with an owner of its own (the device is idle)
static int plane_reserve(tlb_batch *b, int frames)
{
    if (frames <= b->fd_plane_frames) return TLB_OK;
    std::unique_ptr<TlbMem> m(new TlbMem);
    int16_t *pl = m->scratch<int16_t>((size_t)b->nstreams * (size_t)frames * TL_FD_PLANE);
    if (!m->settle()) return TLB_ERR_HIP;
    b->fd_plane_mem.swap(m);
    b->d_fd_plane = pl; b->fd_plane_frames = frames;
    return TLB_OK;
}

// the first down feed: the synthesis tables (shared with the decoder), the stream -> record and ratio tables, the history records and bytes
// (one slot of the longest Layer II frame there is per stream), the queue heads and positions (two copies), the decimator's tables and a
// plane for calls of one tick; staged, settled, then committed
static int down_prepare(tlb_batch *b)
{
    if (b->d_fd_cfg) return TLB_OK;
    if (int rc = synth_prepare(b)) return rc;
    const size_t n = (size_t)b->nstreams;
    TlbMem m;
    int32_t *fc = m.scratch<int32_t>(n), *ra = m.dev<int32_t>(n), *po = m.dev<int32_t>(2 * n);
    TlDecStream *st = m.dev<TlDecStream>(n);
    uint8_t *pv = m.dev<uint8_t>(n * TL_FD_PREV_STRIDE);
    int16_t *ca = m.dev<int16_t>(2 * n * TL_FD_CARRY * 2), *tp = decimate_taps_upload(m);
    std::vector<int32_t> none(n, -1);
    m.upload(fc, none.data(), sizeof(int32_t) * n);
    if (m.failed()) return TLB_ERR_HIP;
    if (int rc = plane_reserve(b, 1)) return rc;                     // (settles; a plane without the rest is scratch nobody reads)
    m.commit(b->mem);
    b->fd.start(n); b->fd_ratio.assign(n, TL_DC_OFF); b->fd_pos.assign(n, 0);
    b->d_fd_cfg = fc; b->d_fd_ratio = ra; b->d_fd_pos = po; b->d_fd_state = st; b->d_fd_prev = pv; b->d_fd_carry = ca; b->d_fd_taps = tp; b->fd_flip = 0;
    return TLB_OK;
}

// streams [s0, s1) get down-feed record `idx` (-1: none); their position, queue and history start again
static int down_assign(tlb_batch *b, int s0, int s1, int idx, const tlb_feed_config &cfg)
{
    std::vector<int32_t> v((size_t)(s1 - s0), idx), r((size_t)(s1 - s0), TL_DC_OFF);
    for (int s = s0; s < s1 && idx >= 0; s++) r[(size_t)(s - s0)] = tl_fd_ratio_of(cfg.samplerate, batch_enc_rate(b, s));
    HIPCHK(hipMemcpy(b->d_fd_cfg + s0, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(b->d_fd_ratio + s0, r.data(), sizeof(int32_t) * r.size(), hipMemcpyHostToDevice));
    for (int s = s0; s < s1; s++) { b->fd.idx[(size_t)s] = idx; b->fd.cfg[(size_t)s] = cfg; b->fd_ratio[(size_t)s] = r[(size_t)(s - s0)]; }
    b->n_down = 0;
    for (int32_t x : b->fd.idx) b->n_down += x >= 0;
    if (int rc = conceal_clear_family(b, s0, s1 - s0, true, true)) return rc;        // another down feed, or none: concealment off, as tlb_feed_set does
    return feed_down_clear_streams(b, s0, s1 - s0);
}

int feed_down_after_reconfigure(tlb_batch *b, int stream)
{
    if (!b->fd.on(stream)) return TLB_OK;
    const tlb_feed_config fc = b->fd.cfg[(size_t)stream];
    if (tl_fd_ratio_of(fc.samplerate, batch_enc_rate(b, stream)) != TL_DC_OFF) return TLB_OK;      // kept, whatever the channel counts; the caller clears the state
    return down_assign(b, stream, stream + 1, -1, tlb_feed_config{0, 0, 0});
}

int feed_down_launch(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report, void *hip_stream, int stride)
{
    if (!b || !d_frames || !d_len || !d_interleaved || nframes <= 0 || nframes > TL_FD_MAX_FRAMES || (long long)nframes * b->nstreams > (1ll << 29)) return TLB_ERR_ARG;
    // the kernels move frames and PCM as 32-bit words and store 32-bit report fields
    if (((uintptr_t)d_frames | (uintptr_t)d_len | (uintptr_t)d_interleaved | (uintptr_t)d_report) & 3u) return TLB_ERR_ARG;
    if (tlb_feed_down_stride(b) == 0 || stride < tlb_feed_down_stride(b) || (stride & 3)) return TLB_ERR_ARG;      // (0: no stream has a down feed)
    if (b->broken) return TLB_ERR_HIP;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = b->fd.report(2 * (size_t)nframes * (size_t)b->nstreams, &d_report)) return rc;
    if (nframes > b->fd_plane_frames) {
        HIPCHK(hipDeviceSynchronize());          // (a launch before may still read the one it replaces)
        if (int rc = plane_reserve(b, nframes)) return rc;
    }
    TlFeedDownLaunch D;
    memset(&D, 0, sizeof D);
    D.F.tables = b->d_tables; D.F.configs = b->fd.d_configs; D.F.feed_cfg = b->d_fd_cfg; D.F.synth = b->d_synth;
    D.F.frames = d_frames; D.F.len = d_len; D.F.report = (TlFrameReport *)d_report; D.F.pcm = d_interleaved;
    D.F.state = b->d_fd_state; D.F.prev = b->d_fd_prev; D.F.prev_stride = TL_FD_PREV_STRIDE;
    D.F.nstreams = b->nstreams; D.F.nframes = nframes; D.F.stride = stride;
    D.ratio = b->d_fd_ratio; D.sconfigs = b->d_configs; D.stream_cfg = b->d_stream_cfg; D.taps = b->d_fd_taps;
    D.plane = b->d_fd_plane; D.carry = b->d_fd_carry; D.pos = b->d_fd_pos; D.flip = b->fd_flip;
    TlConcealConv X;                                                 // (NULL unless some stream with a down feed has concealment on: conceal behind decode, its carry behind carry)
    HIPCHK(tlk_feed_down((hipStream_t)hip_stream, D, conceal_conv(b, true, &X)));
    b->fd_flip ^= 1;
    for (int s = 0; s < b->nstreams; s++)
        if (b->fd.on(s)) b->fd_pos[(size_t)s] = (int32_t)(((long long)b->fd_pos[(size_t)s] + nframes) % tl_fd_cycle(b->fd_ratio[(size_t)s]));
    return TLB_OK;
}

extern "C" {

int tlb_feed_down_set(tlb_batch *b, int stream, const tlb_feed_config *cfg)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b->nstreams : stream + 1;
    if (!cfg) {
        if (!b->d_fd_cfg) return TLB_OK;                             // off, and never on: nothing to allocate or to clear
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());
        return down_assign(b, s0, s1, -1, tlb_feed_config{0, 0, 0});
    }
    if (int rc = feed_down_fits(b, s0, s1, cfg)) return rc;          // every named stream is checked before anything changes
    for (int s = s0; s < s1; s++) if (!batch_may_set(b, s, TLB_IN_DOWN_FEED)) return TLB_ERR_ARG;      // a stream has one source (csrc/tlb_inputs.h)
    int idx = b->fd.find(*cfg);
    TlConfig *c = new TlConfig;
    struct Free { TlConfig *c; ~Free() { delete c; } } free_{c};
    if (idx >= 0) *c = b->fd.h_configs[(size_t)idx];
    else if (int rc = feed_build(c, cfg)) return rc;
    if (tl_feed_slot_bytes(*c) > TL_FD_PREV_STRIDE) return TLB_ERR_BITRATE;      // (no Layer II frame is that long)
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = down_prepare(b)) return rc;
    if (int rc = conceal_g_reserve(b, TL_FD_PREV_STRIDE)) return rc; // (nothing unless concealment was enabled: G is as wide as the widest history slot)
    if (int rc = b->fd.reserve(b->fd.h_configs.size() + (idx < 0 ? 1 : 0))) return rc;
    if (int rc = b->fd.add(*cfg, *c, &idx)) return rc;
    return down_assign(b, s0, s1, idx, *cfg);
}

int tlb_feed_down_get(const tlb_batch *b, int stream, tlb_feed_config *cfg)
{
    if (!b || stream < 0 || stream >= b->nstreams) return -TLB_ERR_ARG;
    const bool on = b->fd.on(stream);
    if (cfg) *cfg = on ? b->fd.cfg[(size_t)stream] : tlb_feed_config{0, 0, 0};
    return on ? 1 : 0;
}

int tlb_feed_down_want_at(long feed_rate, long stream_rate, long tick)
{
    const int ratio = tl_fd_ratio_of(feed_rate, stream_rate);
    if (ratio == TL_DC_OFF) return -TLB_ERR_SAMPLERATE;
    if (tick < 0) return -TLB_ERR_ARG;
    return tl_fd_want((int)(tick % tl_fd_cycle(ratio)), ratio);     // the schedule repeats with the cycle
}

int tlb_feed_down_want(const tlb_batch *b, int stream, int ahead)
{
    if (!b || stream < 0 || stream >= b->nstreams || ahead < 0 || !b->fd.on(stream)) return -TLB_ERR_ARG;
    const int ratio = b->fd_ratio[(size_t)stream];
    return tl_fd_want((int)(((long long)b->fd_pos[(size_t)stream] + ahead) % tl_fd_cycle(ratio)), ratio);
}

int tlb_feed_down_stride(const tlb_batch *b) { return b ? b->fd.stride() : 0; }

int tlb_feed_down_reset(tlb_batch *b, int stream)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    if (!b->d_fd_state) return TLB_OK;           // never fed: every stream's next tick is tick 0 already
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    return stream < 0 ? feed_down_clear_streams(b, 0, b->nstreams) : feed_down_clear_streams(b, stream, 1);
}

int tlb_feed_down_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int16_t *d_interleaved, tlb_frame_report *d_report, int nframes,
                         void *hip_stream)
{
    return feed_down_launch(b, d_frames, d_len, nframes, d_interleaved, d_report, hip_stream, tlb_feed_down_stride(b));
}

int tlb_feed_down_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int16_t *interleaved, tlb_frame_report *report, int nframes)
{
    if (!b || !frames || !len || !interleaved || nframes <= 0 || nframes > TL_FD_MAX_FRAMES || (long long)nframes * b->nstreams > (1ll << 29)) return TLB_ERR_ARG;
    const int stride = tlb_feed_down_stride(b);
    if (stride == 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t ticks = (size_t)nframes * (size_t)b->nstreams, slots = 2 * ticks;
    TlbMem m;
    uint8_t *d_frames = m.scratch<uint8_t>(slots * (size_t)stride); int32_t *d_len = m.scratch<int32_t>(slots);
    int16_t *d_pcm = m.scratch<int16_t>(ticks * 2304); tlb_frame_report *d_report = m.scratch<tlb_frame_report>(slots);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_frames, frames, slots * (size_t)stride, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len, len, slots * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_pcm, interleaved, ticks * 2304 * sizeof(int16_t), hipMemcpyHostToDevice));      // what the kernels do not write (streams without a down feed, behind a one-channel stream's 1152 samples) stays the caller's
    if (int rc = tlb_feed_down_device(b, d_frames, d_len, d_pcm, d_report, nframes, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(interleaved, d_pcm, ticks * 2304 * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (report) HIPCHK(hipMemcpy(report, d_report, slots * sizeof(tlb_frame_report), hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
