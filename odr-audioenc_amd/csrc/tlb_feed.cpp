// tlb_feed.cpp -- the batch-level entry points of the Layer II feeds (include/toolame_batch.h, tlb_feed_*): the legality of a feed
// configuration (host only), the per-stream feed table and history (allocated by the first tlb_feed_set) and one launch of the kernels of
// toolame_feed.hip through tl_kernels.h.  Host C++.
// ADAPTED feeds (tlb_feed_set_adapted; csrc/mp2_feed_adapt.h): the schedule (host only), the queue state and the source plane (allocated by
// the first adapted feed that does not match its stream) and the launch of toolame_feed_adapt.hip behind the strict one.
#include "tlb_internal.h"

static_assert(TLB_DEC_UNWANTED == TL_DEC_UNWANTED && !(TL_DEC_UNWANTED & TL_DEC_BAD_MASK), "status flags");
static bool adapted(const tlb_batch *b, int s) { return !b->fa_ratio.empty() && b->fa_ratio[(size_t)s] >= 0; }

static char feed_mode(int channels) { return channels == 1 ? 'm' : 's'; }
// the feed's kernel-side record: the stream configuration a frame of that rate, bitrate and channel count has (allocation table, sblimit,
// frame length, header indices); the mode is the frame's own and the model plays no part
int feed_build(TlConfig *c, const tlb_feed_config *cfg)
{
    if (!cfg) return TLB_ERR_ARG;
    if (cfg->channels != 1 && cfg->channels != 2) return TLB_ERR_MODE;
    if (cfg->bitrate <= 0) return TLB_ERR_BITRATE;
    return tl_build_config(c, cfg->samplerate, feed_mode(cfg->channels), cfg->bitrate, 1, 0);
}

int feed_fits(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg)
{
    if (int rc = tlb_feed_check_config(cfg)) return rc;
    for (int s = s0; s < s1; s++) {
        const tlb_stream_config &sc = b->h_uniq[(size_t)b->h_stream_cfg[(size_t)s]];
        if (cfg->samplerate != sc.samplerate) return TLB_ERR_SAMPLERATE;
        if (cfg->channels != (sc.mode == 'm' ? 1 : 2)) return TLB_ERR_MODE;
    }
    return TLB_OK;
}

int feed_fits_adapted(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg)
{
    if (int rc = tlb_feed_check_config(cfg)) return rc;
    for (int s = s0; s < s1; s++) if (tl_fa_ratio_of(cfg->samplerate, batch_enc_rate(b, s)) < 0) return TLB_ERR_SAMPLERATE;
    return TLB_OK;
}

int feed_slot_bytes(const tlb_feed_config *cfg)
{
    TlConfig *c = new TlConfig;
    const int n = feed_build(c, cfg) ? 0 : tl_feed_slot_bytes(*c);
    delete c;
    return n;
}

int feed_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_feed_state) return TLB_OK;
    HIPCHK(hipMemset(b->d_feed_state + s0, 0, sizeof(TlDecStream) * (size_t)n));
    if (int rc = conceal_clear_family(b, s0, n, false)) return rc;   // a stream's concealment starts again with its history (G, run, record); a down feed's has its own
    if (!b->d_fa_carry) return TLB_OK;
    for (int k = 0; k < 2; k++) {                                    // an adapted stream's next tick is tick 0 and its queue is empty
        HIPCHK(hipMemset(b->d_fa_carry + ((size_t)k * (size_t)b->nstreams + (size_t)s0) * (TL_FA_CARRY * 2), 0, sizeof(int16_t) * TL_FA_CARRY * 2 * (size_t)n));
        HIPCHK(hipMemset(b->d_fa_pos + (size_t)k * (size_t)b->nstreams + (size_t)s0, 0, sizeof(int32_t) * (size_t)n));
    }
    for (int s = s0; s < s0 + n; s++) b->fa_pos[(size_t)s] = 0;
    return TLB_OK;
}

// the first tlb_feed_set: the synthesis tables (shared with the decoder), the stream -> feed table (all -1) and the history records
static int feed_prepare(tlb_batch *b)
{
    if (b->d_feed_cfg) return TLB_OK;
    if (int rc = synth_prepare(b)) return rc;
    const size_t n = (size_t)b->nstreams;
    TlbMem m;
    int32_t *fc = m.scratch<int32_t>(n);
    TlDecStream *st = m.dev<TlDecStream>(n);
    std::vector<int32_t> none(n, -1);
    m.upload(fc, none.data(), sizeof(int32_t) * n);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->feed.start(n);
    b->d_feed_cfg = fc; b->d_feed_state = st;
    return TLB_OK;
}

// room for `frames` ticks per stream in the source plane: grow-only launch scratch with an owner of its own (the device is idle)
static int adapt_plane_reserve(tlb_batch *b, int frames)
{
    if (frames <= b->fa_plane_frames) return TLB_OK;
    std::unique_ptr<TlbMem> m(new TlbMem);
    int16_t *pl = m->scratch<int16_t>((size_t)b->nstreams * (size_t)frames * 2304);
    if (!m->settle()) return TLB_ERR_HIP;
    b->fa_plane_mem.swap(m);
    b->d_fa_plane = pl; b->fa_plane_frames = frames;
    return TLB_OK;
}

// the first adapted feed: the stream -> record and ratio tables, the queue heads and positions (two copies), the resampler's tables and
// a plane for calls of one tick (what a tick object makes); staged, settled, then committed
static int adapt_prepare(tlb_batch *b)
{
    if (b->d_fa_cfg) return TLB_OK;
    const size_t n = (size_t)b->nstreams;
    TlbMem m;
    int32_t *fc = m.scratch<int32_t>(n), *ra = m.dev<int32_t>(n), *po = m.dev<int32_t>(2 * n);
    int16_t *ca = m.dev<int16_t>(2 * n * TL_FA_CARRY * 2), *tp = resample_taps_upload(m);
    std::vector<int32_t> none(n, -1);
    m.upload(fc, none.data(), sizeof(int32_t) * n);
    if (m.failed()) return TLB_ERR_HIP;
    if (int rc = adapt_plane_reserve(b, 1)) return rc;               // (settles; a plane without the rest is scratch nobody reads)
    m.commit(b->mem);
    b->fa_ratio.assign(n, -1); b->fa_pos.assign(n, 0);
    b->d_fa_cfg = fc; b->d_fa_ratio = ra; b->d_fa_pos = po; b->d_fa_carry = ca; b->d_fa_taps = tp; b->fa_flip = 0;
    return TLB_OK;
}

// room for slots of `stride` bytes in d_feed_prev; what it holds is kept (the device is idle).  An owner of its own (csrc/tlb_mem.h): the new
// buffer is staged and filled in a new owner, and only when it is complete do the owners change places
static int feed_prev_reserve(tlb_batch *b, int stride)
{
    if (stride <= b->feed_prev_stride) return TLB_OK;
    std::unique_ptr<TlbMem> m(new TlbMem);
    uint8_t *np = m->dev<uint8_t>((size_t)b->nstreams * (size_t)stride);
    if (m->failed()) return TLB_ERR_HIP;
    if (b->d_feed_prev)
        HIPCHK(hipMemcpy2D(np, (size_t)stride, b->d_feed_prev, (size_t)b->feed_prev_stride, (size_t)b->feed_prev_stride, (size_t)b->nstreams, hipMemcpyDeviceToDevice));
    if (!m->settle()) return TLB_ERR_HIP;
    b->feed_prev_mem.swap(m);
    b->d_feed_prev = np; b->feed_prev_stride = stride;
    return TLB_OK;
}

// streams [s0, s1) get feed record `idx` (-1: none); their history starts again
// adapt: the record goes into the adapted path's table and the strict kernel sees a stream without a feed
// same_feed: the streams keep the feed they have (a reconfiguration that leaves the pair legal): their concealment stays on, and
// feed_clear_streams forgets its G, run and record with the history
static int feed_assign(tlb_batch *b, int s0, int s1, int idx, const tlb_feed_config &cfg, bool adapt = false, bool same_feed = false)
{
    std::vector<int32_t> v((size_t)(s1 - s0), adapt ? -1 : idx);
    HIPCHK(hipMemcpy(b->d_feed_cfg + s0, v.data(), sizeof(int32_t) * v.size(), hipMemcpyHostToDevice));
    if (b->d_fa_cfg) {
        std::vector<int32_t> a((size_t)(s1 - s0), adapt ? idx : -1), r((size_t)(s1 - s0), 0);
        for (int s = s0; s < s1 && adapt; s++) r[(size_t)(s - s0)] = tl_fa_ratio_of(cfg.samplerate, batch_enc_rate(b, s));
        HIPCHK(hipMemcpy(b->d_fa_cfg + s0, a.data(), sizeof(int32_t) * a.size(), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(b->d_fa_ratio + s0, r.data(), sizeof(int32_t) * r.size(), hipMemcpyHostToDevice));
        for (int s = s0; s < s1; s++) b->fa_ratio[(size_t)s] = adapt && idx >= 0 ? r[(size_t)(s - s0)] : -1;
        b->n_adapted = 0;
        for (int32_t x : b->fa_ratio) b->n_adapted += x >= 0;
    }
    for (int s = s0; s < s1; s++) { b->feed.idx[(size_t)s] = idx; b->feed.cfg[(size_t)s] = cfg; }
    if (!same_feed) if (int rc = conceal_clear_family(b, s0, s1 - s0, false, true)) return rc;       // another feed, or none: concealment off (G would be a frame of another format)
    return feed_clear_streams(b, s0, s1 - s0);
}

int feed_after_reconfigure(tlb_batch *b, int stream)
{
    if (!b->feed.on(stream)) return TLB_OK;
    const tlb_stream_config &sc = b->h_uniq[(size_t)b->h_stream_cfg[(size_t)stream]];
    const tlb_feed_config fc = b->feed.cfg[(size_t)stream];
    if (adapted(b, stream)) {                                        // kept while the rates still form a legal pair, whatever the channel counts; the caller clears the state
        if (tl_fa_ratio_of(fc.samplerate, sc.samplerate) >= 0) return feed_assign(b, stream, stream + 1, b->feed.idx[(size_t)stream], fc, true, true);      // (its concealment stays, as a strict and a down feed's do)
    } else if (fc.samplerate == sc.samplerate && fc.channels == (sc.mode == 'm' ? 1 : 2)) return TLB_OK;
    return feed_assign(b, stream, stream + 1, -1, tlb_feed_config{0, 0, 0});
}

int feed_launch(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report, void *hip_stream, int stride)
{
    if (!b || !d_frames || !d_len || !d_interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    // the kernels move frames and PCM as 32-bit words and store 32-bit report fields
    if (((uintptr_t)d_frames | (uintptr_t)d_len | (uintptr_t)d_interleaved | (uintptr_t)d_report) & 3u) return TLB_ERR_ARG;
    if (tlb_feed_stride(b) == 0 || stride < tlb_feed_stride(b) || (stride & 3)) return TLB_ERR_ARG;      // (0: no stream has a feed)
    if (b->broken) return TLB_ERR_HIP;
    HIPCHK(hipSetDevice(b->device));
    if (int rc = b->feed.report((size_t)nframes * (size_t)b->nstreams, &d_report)) return rc;
    int n_strict = 0;
    for (int s = 0; s < b->nstreams; s++) n_strict += b->feed.on(s) && !adapted(b, s);
    if (b->n_adapted) {
        if (nframes > TL_FA_MAX_FRAMES) return TLB_ERR_ARG;
        if (nframes > b->fa_plane_frames) {
            HIPCHK(hipDeviceSynchronize());      // (a launch before may still read the one it replaces)
            if (int rc = adapt_plane_reserve(b, nframes)) return rc;
        }
    }
    TlFeedLaunch A;
    memset(&A, 0, sizeof A);
    A.tables = b->d_tables; A.configs = b->feed.d_configs; A.feed_cfg = b->d_feed_cfg; A.synth = b->d_synth;
    A.frames = d_frames; A.len = d_len; A.report = (TlFrameReport *)d_report; A.pcm = d_interleaved;
    A.state = b->d_feed_state; A.prev = b->d_feed_prev; A.prev_stride = b->feed_prev_stride;
    A.nstreams = b->nstreams; A.nframes = nframes; A.stride = stride;
    if (n_strict || !b->n_adapted) HIPCHK(tlk_feed((hipStream_t)hip_stream, A));
    if (int rc = conceal_launch(b, A, hip_stream)) return rc;        // (nothing unless some stream has concealment on: behind the strict launch, ahead of the adapted streams')
    if (!b->n_adapted) return TLB_OK;
    // the adapted streams, behind the strict launch (to which they are streams without a feed): decode, resample, carry
    TlFeedAdaptLaunch D;
    memset(&D, 0, sizeof D);
    D.F = A; D.F.feed_cfg = b->d_fa_cfg;
    D.ratio = b->d_fa_ratio; D.sconfigs = b->d_configs; D.stream_cfg = b->d_stream_cfg; D.taps = b->d_fa_taps;
    D.plane = b->d_fa_plane; D.carry = b->d_fa_carry; D.pos = b->d_fa_pos; D.flip = b->fa_flip; D.strict_ran = n_strict > 0;
    TlConcealConv X;                                                 // (NULL unless some adapted stream has concealment on: conceal behind decode, its carry behind carry)
    HIPCHK(tlk_feed_adapt((hipStream_t)hip_stream, D, conceal_conv(b, false, &X)));
    b->fa_flip ^= 1;
    for (int s = 0; s < b->nstreams; s++)
        if (adapted(b, s)) b->fa_pos[(size_t)s] = (int32_t)(((long long)b->fa_pos[(size_t)s] + nframes) % tl_fa_cycle(b->fa_ratio[(size_t)s]));
    return TLB_OK;
}

extern "C" {

int tlb_feed_check_config(const tlb_feed_config *cfg)
{
    TlConfig *c = new TlConfig;
    const int rc = feed_build(c, cfg);
    delete c;
    return rc;
}

int tlb_feed_frame_bytes(const tlb_feed_config *cfg)
{
    TlConfig *c = new TlConfig;
    const int rc = feed_build(c, cfg);
    const int n = rc ? -rc : c->frame_bytes;
    delete c;
    return n;
}

static int feed_set(tlb_batch *b, int stream, const tlb_feed_config *cfg, bool adapt)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b->nstreams : stream + 1;
    if (!cfg) {
        if (!b->d_feed_cfg) return TLB_OK;                           // off, and never on: nothing to allocate or to clear
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());
        return feed_assign(b, s0, s1, -1, tlb_feed_config{0, 0, 0});
    }
    for (int s = s0; s < s1; s++) if (!batch_may_set(b, s, TLB_IN_FEED)) return TLB_ERR_ARG;      // a stream has one source (csrc/tlb_inputs.h)
    if (adapt && feed_fits(b, s0, s1, cfg) == TLB_OK) adapt = false; // a configuration that matches every named stream IS a strict feed
    if (int rc = adapt ? feed_fits_adapted(b, s0, s1, cfg) : feed_fits(b, s0, s1, cfg)) return rc;       // every named stream is checked before anything changes
    int idx = b->feed.find(*cfg);
    TlConfig *c = new TlConfig;
    struct Free { TlConfig *c; ~Free() { delete c; } } free_{c};
    if (idx >= 0) *c = b->feed.h_configs[(size_t)idx];
    else if (int rc = feed_build(c, cfg)) return rc;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = feed_prepare(b)) return rc;
    if (adapt) if (int rc = adapt_prepare(b)) return rc;
    if (int rc = b->feed.reserve(b->feed.h_configs.size() + (idx < 0 ? 1 : 0))) return rc;
    if (int rc = feed_prev_reserve(b, tl_feed_slot_bytes(*c))) return rc;
    if (int rc = conceal_g_reserve(b, b->feed_prev_stride)) return rc;
    if (int rc = b->feed.add(*cfg, *c, &idx)) return rc;
    return feed_assign(b, s0, s1, idx, *cfg, adapt);
}

int tlb_feed_set(tlb_batch *b, int stream, const tlb_feed_config *cfg) { return feed_set(b, stream, cfg, false); }
int tlb_feed_set_adapted(tlb_batch *b, int stream, const tlb_feed_config *cfg) { return feed_set(b, stream, cfg, true); }

int tlb_feed_adapted(const tlb_batch *b, int stream)
{
    if (!b || stream < 0 || stream >= b->nstreams) return -TLB_ERR_ARG;
    return adapted(b, stream) ? 1 : 0;
}

int tlb_feed_want_at(long feed_rate, long stream_rate, long tick)
{
    const int ratio = tl_fa_ratio_of(feed_rate, stream_rate);
    if (ratio < 0) return -TLB_ERR_SAMPLERATE;
    if (tick < 0) return -TLB_ERR_ARG;
    return tl_fa_want((int)(tick % tl_fa_cycle(ratio)), ratio);     // the schedule repeats with the cycle
}

int tlb_feed_want(const tlb_batch *b, int stream, int ahead)
{
    if (!b || stream < 0 || stream >= b->nstreams || ahead < 0 || !b->feed.on(stream)) return -TLB_ERR_ARG;
    if (!adapted(b, stream)) return 1;
    const int ratio = b->fa_ratio[(size_t)stream];
    return tl_fa_want((int)(((long long)b->fa_pos[(size_t)stream] + ahead) % tl_fa_cycle(ratio)), ratio);
}

int tlb_feed_get(const tlb_batch *b, int stream, tlb_feed_config *cfg)
{
    if (!b || stream < 0 || stream >= b->nstreams) return -TLB_ERR_ARG;
    const bool on = b->feed.on(stream);
    if (cfg) *cfg = on ? b->feed.cfg[(size_t)stream] : tlb_feed_config{0, 0, 0};
    return on ? 1 : 0;
}

int tlb_feed_stride(const tlb_batch *b) { return b ? b->feed.stride() : 0; }

int tlb_feed_reset(tlb_batch *b, int stream)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    if (!b->d_feed_state) return TLB_OK;         // never fed: every stream's next frame is a first frame already
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    return stream < 0 ? feed_clear_streams(b, 0, b->nstreams) : feed_clear_streams(b, stream, 1);
}

int tlb_feed_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report,
                    void *hip_stream)
{
    return feed_launch(b, d_frames, d_len, nframes, d_interleaved, d_report, hip_stream, tlb_feed_stride(b));
}


int tlb_feed_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int nframes, int16_t *interleaved, tlb_frame_report *report)
{
    if (!b || !frames || !len || !interleaved || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    const int stride = tlb_feed_stride(b);
    if (stride == 0) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams;
    TlbMem m;
    uint8_t *d_frames = m.scratch<uint8_t>(slots * (size_t)stride); int32_t *d_len = m.scratch<int32_t>(slots);
    int16_t *d_pcm = m.scratch<int16_t>(slots * 2304); tlb_frame_report *d_report = m.scratch<tlb_frame_report>(slots);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_frames, frames, slots * (size_t)stride, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_len, len, slots * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_pcm, interleaved, slots * 2304 * sizeof(int16_t), hipMemcpyHostToDevice));      // what the kernel does not write (streams without a feed, behind a one-channel feed's 1152 samples) stays the caller's
    if (int rc = tlb_feed_device(b, d_frames, d_len, nframes, d_pcm, d_report, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(interleaved, d_pcm, slots * 2304 * sizeof(int16_t), hipMemcpyDeviceToHost));
    if (report) HIPCHK(hipMemcpy(report, d_report, slots * sizeof(tlb_frame_report), hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
