// tlb_tick.cpp -- the real-time loop body as one object (include/toolame_batch.h, tlb_tick_*).  Host C++ above the batch and egress entry points.
#include "tlb_blocks.h"
#include "tlb_internal.h"
#include "tlb_plan.h"

#include <memory>

// ------------------------------------------------------------------------------------------
// The caller's real-time loop body as ONE call per tick (include/toolame_batch.h, tlb_tick_*): what AudioEnc::run() does for
// one stream every 24 ms -- gain / peak / de-interleave (src/odr-audioenc.cpp:1030-1051,1139-1152), toolame_encode_frame
// (:1158), re-framing into 3*bitrate-byte units (:1208-1225), EDI::write_frame (src/Outputs.cpp:194-261, optionally the PFT
// layer) -- for every stream of a GPU at once: interleaved PCM in pinned host memory -> PCIe -> tl_ingest_kernel ->
// the encode kernels (one frame per stream) -> tl_edi_af_kernel (-> tl_edi_pft_kernel) -> PCIe -> pinned host memory.
// The streams are split into groups (contiguous ranges, a private tlb_batch each): while group g's kernels run, group g+1's
// PCM comes in and group g-1's packets go out, on three HIP streams (the link is full duplex).
// ------------------------------------------------------------------------------------------
// A FEED LANE: where a feed family (tlb_feed_*, tlb_feed_down_*) meets the tick plane.  The family names its batch-level calls and its slots per
// stream; a tick object has one TickLane per family and every group one TickLaneGroup.  The frames and their lengths travel with the input
// sets, the reports with the output sets.  `stride` is ONE slot width for every group (the widest feed the lane has had: it only grows); the
// frame buffers are replaced when it grows and have an owner of their own (the old owner goes when the new one is complete), the rest
// belongs to the object's `mem`.
struct FeedFamily {
    TlbInput input;
    int slots;                                   // per stream and tick
    int (*fits)(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg, bool adapt);
    int (*set)(tlb_batch *b, int stream, const tlb_feed_config *cfg, bool adapt);
    int (*get)(const tlb_batch *b, int stream, tlb_feed_config *cfg, bool *was_adapted);
    int (*want)(const tlb_batch *b, int stream, int ahead);
    int (*launch)(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report, void *hip_stream, int stride);
};
static const FeedFamily tick_families[2] = {
    {TLB_IN_FEED, 1,                             // adapt: through tlb_feed_set_adapted (a legal rate pair and any channel counts instead of the stream's own)
     [](const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg, bool adapt) { return (adapt ? feed_fits_adapted : feed_fits)(b, s0, s1, cfg); },
     [](tlb_batch *b, int stream, const tlb_feed_config *cfg, bool adapt) { return (adapt ? tlb_feed_set_adapted : tlb_feed_set)(b, stream, cfg); },
     [](const tlb_batch *b, int stream, tlb_feed_config *cfg, bool *was_adapted) { *was_adapted = tlb_feed_adapted(b, stream) > 0; return tlb_feed_get(b, stream, cfg); },
     tlb_feed_want, feed_launch},
    {TLB_IN_DOWN_FEED, 2,
     [](const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg, bool) { return feed_down_fits(b, s0, s1, cfg); },
     [](tlb_batch *b, int stream, const tlb_feed_config *cfg, bool) { return tlb_feed_down_set(b, stream, cfg); },
     [](const tlb_batch *b, int stream, tlb_feed_config *cfg, bool *was_adapted) { *was_adapted = false; return tlb_feed_down_get(b, stream, cfg); },
     tlb_feed_down_want, feed_down_launch},
};
enum { LANE_FEED, LANE_DOWN_FEED, LANES };       // submit order: feed before down feed, both ahead of the resampler and the decimator
struct TickLaneGroup {
    uint8_t *d_frames = nullptr; int32_t *d_len = nullptr; tlb_frame_report *d_report = nullptr;      // the group's slice of the tick's frames and lengths, the launch's reports
    bool any = false, all = false;               // some / every stream of the group has a feed of the family (all: the group's PCM is not copied in)
};
struct TickLane {
    bool on = false;                             // at least one stream has a feed of the family
    int stride = 0;
    uint8_t *h_frames[2] = {}; int32_t *h_len[2] = {}; tlb_frame_report *h_report[3] = {};
    std::unique_ptr<TlbMem> mem;                 // owns h_frames[] and the groups' d_frames
};

// A RECORD OPTION: an opt-in whose product is one fixed-size record per stream and tick that travels with the output sets.  What one has is
// stated here once: the record's size and the option whose event its copy-out runs behind (its own, but the compare monitor's records are
// written ahead of the monitor's event); per object its on flag and three pinned sets (TickRecords), per group the device array d_rec[] and
// the event ev_rec[].  tick_record_enable stages the buffers and makes the events, tick_record_out is the copy-out, tick_record the accessor,
// tlb_tick_destroy frees the events.  A PCM METER is a record option that also names its batch-level calls: enabled per batch with the
// object's ceiling (the true-peak meter's; the others ignore it), run on the tick's planar PCM whenever there is new input, reset for one
// stream or all between ticks.  tick_egress queues the meters in table order; the monitor's and the compare monitor's launches are its own.
enum { REC_MONITOR, REC_COMPARE, REC_LOUDNESS, REC_TRUEPEAK, REC_LIMITER, REC_CONCEAL, RECS };
struct RecordOption {
    size_t size;                                 // of one record
    int ev;                                      // the option behind whose event (ev_rec[ev]) the copy-out runs
    // a PCM meter's batch-level calls; NULL for the monitor and the compare monitor
    int (*enable)(tlb_batch *b, uint32_t ceiling);
    int (*launch)(tlb_batch *b, const int16_t *d_pcm_planar, int nframes, void *d_records, void *hip_stream);
    int (*reset)(tlb_batch *b, int stream);
};
static const RecordOption tick_records[RECS] = {
    {sizeof(tlb_monitor_record), REC_MONITOR, nullptr, nullptr, nullptr},
    {sizeof(tlb_compare_record), REC_MONITOR, nullptr, nullptr, nullptr},
    {sizeof(tlb_loudness_record), REC_LOUDNESS,
     [](tlb_batch *b, uint32_t) { return tlb_loudness_enable(b); },
     [](tlb_batch *b, const int16_t *d_pcm, int nframes, void *d_records, void *hip_stream) { return tlb_loudness_device(b, d_pcm, nframes, (tlb_loudness_record *)d_records, hip_stream); },
     tlb_loudness_reset},
    {sizeof(tlb_truepeak_record), REC_TRUEPEAK,
     tlb_truepeak_enable,
     [](tlb_batch *b, const int16_t *d_pcm, int nframes, void *d_records, void *hip_stream) { return tlb_truepeak_device(b, d_pcm, nframes, (tlb_truepeak_record *)d_records, hip_stream); },
     tlb_truepeak_reset},
    // the limiter is no meter: tlb_tick_submit queues it AHEAD of the encoder, with its own parameters (tlb_tick_enable_limiter); its reset is a meter's
    {sizeof(tlb_limiter_record), REC_LIMITER, nullptr, nullptr, tlb_limiter_reset},
    // the feed concealment is no meter either: the feed launch of tlb_tick_submit queues its kernels, and the batches' records are copied into
    // the groups' behind it (tlb_tick_enable_conceal: per stream, between ticks); its reset is a meter's
    {sizeof(tlb_conceal_record), REC_CONCEAL, nullptr, nullptr, tlb_conceal_reset},
};
struct TickRecords {
    bool on = false;
    void *h[3] = {};
};

struct TickGroup {
    tlb_batch *b = nullptr;
    int first = 0, n = 0, out_stride = 0, max_upf = 1, af_stride = 0, max_frags = 0, frag_stride = 0;
    int16_t *d_inter = nullptr, *d_pcm = nullptr, *d_peaks = nullptr;
    int16_t *d_rs = nullptr;                                    // resampler (tlb_tick_set_source): d_inter at the encoder's rate, what the ingest reads
    uint8_t *d_xpad = nullptr; int32_t *d_xl = nullptr;
    uint8_t *d_frames = nullptr; int32_t *d_flen = nullptr;
    tlb_edi_state *d_state = nullptr; uint8_t *d_pkts = nullptr; int32_t *d_plen = nullptr;
    uint16_t *d_pseq = nullptr; uint8_t *d_frags = nullptr; int32_t *d_fraglen = nullptr, *d_nfrag = nullptr;
    uint8_t *d_msgs = nullptr; int msg_stride = 0;              // ZeroMQ egress
    uint32_t *d_silence = nullptr;                              // milliseconds of digital silence so far, per stream
    int32_t *d_valid = nullptr;                                 // short reads (tlb_tick_enable_short_reads): sample frames delivered this tick, per stream
    uint32_t *d_underrun_ms = nullptr, *d_underruns = nullptr;  // ... milliseconds without a full read / short reads so far, per stream
    // this group's slices of the pinned host outputs, THREE sets: tick n's results land in set n % 3.  With two ticks in flight the
    // caller is still reading tick n (valid until the next wait) while tick n + 1 is on its way and tick n + 2 is being submitted:
    // three sets make "until the next wait" true without a copy (two sets let submit n + 2 overwrite what tick n showed)
    uint8_t *h_frames[3] = {}; int32_t *h_flen[3] = {}; uint8_t *h_pkts[3] = {}; int32_t *h_plen[3] = {};
    uint8_t *h_frags[3] = {}; int32_t *h_fraglen[3] = {}, *h_nfrag[3] = {};
    uint8_t *h_msgs[3] = {};
    // confidence monitor (tlb_tick_enable_monitor): the decode call's reports (and PCM under AUDIO) of this tick's frames
    tlb_frame_report *d_report = nullptr; int16_t *d_mpcm = nullptr;
    TickLaneGroup lane[LANES];                                  // Layer II feeds and down feeds (tlb_tick_set_feed, tlb_tick_set_down_feed)
    // down sources (tlb_tick_set_down_source): the group's slice of the tick's wide slots; the decimator writes the streams' slots of d_inter
    int16_t *d_wide = nullptr;
    bool any_down = false, all_down = false;                    // some / every stream of the group has a down source (all: the group's PCM is not copied in)
    void *d_rec[RECS] = {};                                     // record options: the group's records of this tick
    hipEvent_t ev_rec[RECS] = {};                               // ... written: the records' copy-out waits for it, the packets' does not (REC_MONITOR's: decode + fold (+ compare) done)
    hipEvent_t ev_in = nullptr, ev_run = nullptr;
    hipEvent_t ev_ingested = nullptr, ev_encoded = nullptr, ev_out = nullptr;   // the group's device buffers are single: the next tick's copy-in waits for this tick's
                                                                                // ingest (d_inter) / encode (X-PAD), its kernels for this tick's copy-out
};
struct tlb_tick {
    int device = 0, nstreams = 0, egress = 0, version_len = 0, with_xpad = 0;
    char version[TL_EDI_MAX_VERSION] = {};
    int fec = 0, chunk_len = 207, transport = 0, addr_source = 0, dest_port = 0;
    std::vector<TickGroup> groups;
    TlbBlocks blocks;                            // the cut of the streams into the groups, stream -> group (csrc/tlb_blocks.h)
    // pinned host buffers (tlb_tick_submit / tlb_tick_wait): two INPUT sets -- the caller fills input set `in_set` while the tick
    // submitted before is still on its way (with two ticks in flight neither set is free: the input accessors return NULL) -- and
    // three OUTPUT sets; results are read from `out_set`, the set of the tick waited for last
    int16_t *h_inter[2] = {}, *h_peaks[3] = {}; uint8_t *h_xpad[2] = {}; int32_t *h_xl[2] = {};
    uint32_t *h_silence[3] = {};
    // short reads (src/odr-audioenc.cpp:335-373,910-935), off until tlb_tick_enable_short_reads(): `valid` travels with the input sets,
    // the two underrun counters with the output sets.  A set of h_valid is all 1152 whenever the caller can see it untouched.
    bool short_reads = false;
    int32_t *h_valid[2] = {}; uint32_t *h_underrun_ms[3] = {}, *h_underruns[3] = {};
    TickRecords rec[RECS];                       // record options, each off until its enable
    bool lra = false;                            // loudness range (tlb_tick_enable_lra): the groups' batches count range blocks in the loudness meter's launch
    // confidence monitor, off (0) until tlb_tick_enable_monitor(): the listened stream's PCM travels with the output sets as the records do
    int monitor = 0;                             // TLB_MONITOR_CHECK / TLB_MONITOR_AUDIO
    int16_t *h_listen[3] = {};
    int listen = -1;                             // the stream the NEXT submit carries (tlb_tick_monitor_listen); -1: none
    int listen_of[3] = {-1, -1, -1};             // ... the tick of each output set carried
    bool resample = false;                       // at least one stream has a source: every submit queues the resampler between copy-in and ingest
                                                 // (the groups' d_rs buffers, once made, stay until destroy)
    // down sources, off until the first real tlb_tick_set_down_source: the wide slots [nstreams][TLB_DECIMATE_SLOT] travel with the input sets
    bool down = false;                           // at least one stream has a down source
    int16_t *h_wide[2] = {};
    TickLane lane[LANES];                        // Layer II feeds and down feeds, each off until its first set
    tlb_compare_params cparams = {};             // compare monitor (tlb_tick_enable_compare): needs the AUDIO monitor's decoded PCM
#ifdef TLB_FAULT_INJECT
    int damage_nth = 0, damage_stream = 0, damage_byte = 0; uint8_t damage_xor = 0, damage_val = 0;      // tlb_debug_tick_damage_next
    int cross_nth = 0, cross_a = -1, cross_b = -1; bool cross_on = false; uint8_t *d_cross_tmp = nullptr;   // tlb_debug_tick_cross_from
#endif
    int in_set = 0, out_set = 0;
    long waited = 0;                             // ticks whose results have been waited for (ticks: submitted)
    TlbMem mem;                                  // owns every pinned and device buffer of the object and its groups (csrc/tlb_mem.h)
    hipStream_t s_in = nullptr, s_run = nullptr, s_out = nullptr;
    hipEvent_t ev0[3] = {}, ev1[3] = {};          // per output set: first copy-in queued / last copy-out done
    long ticks = 0;
    bool finished = false;
    bool broken = false;                         // a device call of submit / wait / finish failed: the groups queued before the failing one have advanced by a frame,
                                                 // the later ones have not -- the object is out of step with itself and every further call but destroy is refused (sticky)
};
// a failing submit / wait / finish: drain what was queued, mark the object, hand the code on
static int tick_fail(tlb_tick *t, int rc);
// the input families that are on (csrc/tlb_inputs.h): what every opt-in and setter of the object asks tlb_input_may_set about
static unsigned tick_inputs(const tlb_tick *t)
{
    return (t->resample ? TLB_IN_BIT(TLB_IN_UP_SOURCE) : 0u) | (t->down ? TLB_IN_BIT(TLB_IN_DOWN_SOURCE) : 0u) | (t->lane[LANE_FEED].on ? TLB_IN_BIT(TLB_IN_FEED) : 0u) |
           (t->lane[LANE_DOWN_FEED].on ? TLB_IN_BIT(TLB_IN_DOWN_FEED) : 0u) | (t->short_reads ? TLB_IN_BIT(TLB_IN_SHORT_READS) : 0u);
}
static bool tick_may_set(const tlb_tick *t, TlbInput f) { return tlb_input_may_set(TLB_INPUTS_OBJECT, f, tick_inputs(t)); }
// THE STAGED OPT-IN, all or nothing: `stage` puts every buffer into a local owner and the groups' fields into a copy of the
// groups, runs the batches' *_prepare, and may fail with a code; then settle, commit -- and only after that do the caller's own fields and the
// option's flag change.  A refused attempt leaves the object as it was (what a batch made for itself stays: it is used by nothing yet).
template <class Stage> static int tick_opt_in(tlb_tick *t, Stage stage)
{
    TlbMem m;
    std::vector<TickGroup> gs = t->groups;
    if (int rc = stage(m, gs)) return rc;
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(t->mem);
    t->groups.swap(gs);
    return TLB_OK;
}
// A record option is opted into the same way (after the caller's own argument checks): the events of its groups, then in one staged opt-in its
// pinned sets and, group by group, what `stage` makes for the group (its batch's *_prepare or enable first) and the group's device array;
// then the option is on.  `also`: three more pinned sets of `also_bytes` each that travel with the records (the monitor's listened PCM).
// What else the caller sets stays with it.
template <class Stage> static int tick_record_enable(tlb_tick *t, int r, Stage stage, size_t also_bytes = 0, void **also = nullptr)
{
    const RecordOption &R = tick_records[r];
    HIPCHK(hipSetDevice(t->device));
    for (auto &G : t->groups) if (!G.ev_rec[R.ev]) HIPCHK(hipEventCreateWithFlags(&G.ev_rec[R.ev], hipEventDisableTiming));   // (a refused attempt keeps them for the next)
    void *h[3];
    if (int rc = tick_opt_in(t, [&](TlbMem &m, std::vector<TickGroup> &gs) {
            for (int k = 0; k < 3; k++) { h[k] = m.pinned<uint8_t>((size_t)t->nstreams * R.size); if (also) also[k] = m.pinned<uint8_t>(also_bytes); }
            for (auto &G : gs) {
                if (int rc = stage(m, G)) return rc;
                G.d_rec[r] = m.dev<uint8_t>((size_t)G.n * R.size);
            }
            return 0;
        })) return rc;
    memcpy(t->rec[r].h, h, sizeof h);
    t->rec[r].on = true;
    return TLB_OK;
}
// ... and read the same way: the records of the tick waited for last, NULL while the option is off
static const void *tick_record(const tlb_tick *t, int r) { return t && t->rec[r].on ? t->rec[r].h[t->out_set] : nullptr; }
#ifdef TLB_FAULT_INJECT
static int tick_cross(tlb_tick *t, TickGroup &G);
#endif

extern "C" {

void tlb_tick_destroy(tlb_tick *t)
{
    if (!t) return;
    (void)hipSetDevice(t->device);
    (void)hipDeviceSynchronize();
    for (auto &g : t->groups) {
        if (g.b) tlb_destroy(g.b);
        if (g.ev_in) (void)hipEventDestroy(g.ev_in);
        if (g.ev_run) (void)hipEventDestroy(g.ev_run);
        if (g.ev_ingested) (void)hipEventDestroy(g.ev_ingested);
        if (g.ev_encoded) (void)hipEventDestroy(g.ev_encoded);
        if (g.ev_out) (void)hipEventDestroy(g.ev_out);
        for (hipEvent_t e : g.ev_rec) if (e) (void)hipEventDestroy(e);
    }
    if (t->s_in) (void)hipStreamDestroy(t->s_in);
    if (t->s_run) (void)hipStreamDestroy(t->s_run);
    if (t->s_out) (void)hipStreamDestroy(t->s_out);
    for (int k = 0; k < 3; k++) { if (t->ev0[k]) (void)hipEventDestroy(t->ev0[k]); if (t->ev1[k]) (void)hipEventDestroy(t->ev1[k]); }
    delete t;                                    // (t->mem frees the buffers)
}

static int tick_create_impl(tlb_tick *t, int device, int nstreams, const tlb_stream_config *cfgs, const tlb_tick_config *tc)
{
    t->device = device; t->nstreams = nstreams; t->egress = tc->egress; t->with_xpad = tc->with_xpad ? 1 : 0;
    if (tc->egress < TLB_TICK_FRAMES || tc->egress > TLB_TICK_ZMQ || tc->version_len < 0 || tc->version_len > TL_EDI_MAX_VERSION ||
        (tc->version_len && !tc->version)) return TLB_ERR_ARG;
    t->version_len = tc->version_len;
    if (tc->version_len) memcpy(t->version, tc->version, (size_t)tc->version_len);
    t->fec = tc->fec; t->chunk_len = tc->chunk_len ? tc->chunk_len : 207; t->transport = tc->transport; t->addr_source = tc->addr_source; t->dest_port = tc->dest_port;
    int ng = tc->ngroups > 0 ? tc->ngroups : (nstreams >= 65536 ? 8 : nstreams >= 8192 ? 4 : nstreams >= 2048 ? 2 : 1);      // more groups = a shorter tail behind the last copy-in
    if (ng > nstreams) ng = nstreams;
    t->groups.resize((size_t)ng);
    t->blocks = TlbBlocks(nstreams, ng);
    size_t n_frames = 0, n_pkts = 0, n_slots = 0, n_frags = 0, n_fragslots = 0, n_msgs = 0;
    for (int g = 0; g < ng; g++) {
        TickGroup &G = t->groups[(size_t)g];
        G.first = t->blocks.block(g).first; G.n = t->blocks.block(g).n;
        int err = 0;
        G.b = tlb_create(device, G.n, cfgs + G.first, &err);
        if (!G.b) return err ? err : TLB_ERR_HIP;
        G.out_stride = G.b->out_stride; G.max_upf = G.b->max_upf;
        if (tc->egress == TLB_TICK_ZMQ) {
            if (!G.max_upf) return TLB_ERR_SAMPLERATE;
            G.msg_stride = tlb_zmq_msg_stride(G.b);
        } else if (tc->egress != TLB_TICK_FRAMES) {
            if (!G.max_upf) return TLB_ERR_SAMPLERATE;
            G.af_stride = tlb_edi_af_stride(G.b, tc->version_len);
            if (tc->egress == TLB_TICK_EDI_PFT)
                if (int rc = pft_shape(G.af_stride, t->fec, t->chunk_len, t->transport, &G.max_frags, &G.frag_stride)) return rc;
        } else if (!G.max_upf) G.max_upf = 1;
        n_frames += (size_t)G.n * (size_t)G.out_stride;
        n_slots += (size_t)G.n * (size_t)G.max_upf;
        n_pkts += (size_t)G.n * (size_t)G.max_upf * (size_t)G.af_stride;
        n_msgs += (size_t)G.n * (size_t)G.max_upf * (size_t)G.msg_stride;
        n_fragslots += (size_t)G.n * (size_t)G.max_upf * (size_t)G.max_frags;
        n_frags += (size_t)G.n * (size_t)G.max_upf * (size_t)G.max_frags * (size_t)G.frag_stride;
    }
    HIPCHK(hipSetDevice(device));
    TlbMem &m = t->mem;                                              // straight into the tick's owner: a failure here ends in tlb_tick_destroy
    const size_t ns = (size_t)nstreams, xp = t->with_xpad ? ns : 0;
    uint8_t *h_msgs[3], *h_frames[3], *h_pkts[3], *h_frags[3]; int32_t *h_flen[3], *h_plen[3], *h_fraglen[3], *h_nfrag[3];
    for (int k = 0; k < 2; k++) {
        t->h_inter[k] = m.pinned<int16_t>(ns * 2304);
        t->h_xpad[k] = m.pinned<uint8_t>(xp * TL_MAX_XPAD); t->h_xl[k] = m.pinned<int32_t>(xp);
    }
    for (int k = 0; k < 3; k++) {
        t->h_peaks[k] = m.pinned<int16_t>(ns * 2); t->h_silence[k] = m.pinned<uint32_t>(ns);
        h_msgs[k] = m.pinned<uint8_t>(n_msgs);
        h_frames[k] = m.pinned<uint8_t>(n_frames); h_flen[k] = m.pinned<int32_t>(ns);
        h_pkts[k] = m.pinned<uint8_t>(n_pkts); h_plen[k] = m.pinned<int32_t>(n_slots);
        h_frags[k] = m.pinned<uint8_t>(n_frags); h_fraglen[k] = m.pinned<int32_t>(n_fragslots); h_nfrag[k] = m.pinned<int32_t>(n_slots);
    }
    MEMCHK(m);
    std::vector<tlb_edi_state> st0;
    size_t o_frames = 0, o_slots = 0, o_pkts = 0, o_frags = 0, o_fragslots = 0, o_msgs = 0;
    for (auto &G : t->groups) {
        const size_t n = (size_t)G.n, slots = n * (size_t)G.max_upf;
        G.d_inter = m.dev<int16_t>(n * 2304); G.d_pcm = m.dev<int16_t>(n * 2304); G.d_peaks = m.dev<int16_t>(n * 2);
        G.d_xpad = m.dev<uint8_t>(t->with_xpad ? n * TL_MAX_XPAD : 0); G.d_xl = m.dev<int32_t>(t->with_xpad ? n : 0);
        G.d_frames = m.dev<uint8_t>(n * (size_t)G.out_stride); G.d_flen = m.dev<int32_t>(n);
        G.d_state = m.dev<tlb_edi_state>(n);
        G.d_pkts = m.dev<uint8_t>(slots * (size_t)G.af_stride); G.d_plen = m.dev<int32_t>(slots);
        G.d_pseq = m.dev<uint16_t>(n);
        G.d_msgs = m.dev<uint8_t>(slots * (size_t)G.msg_stride); G.d_silence = m.dev<uint32_t>(n);
        G.d_frags = m.dev<uint8_t>(slots * (size_t)G.max_frags * (size_t)G.frag_stride); G.d_fraglen = m.dev<int32_t>(slots * (size_t)G.max_frags); G.d_nfrag = m.dev<int32_t>(slots);
        MEMCHK(m);
        for (int k = 0; k < 3; k++) {
            G.h_msgs[k] = h_msgs[k] + o_msgs;
            G.h_frames[k] = h_frames[k] + o_frames; G.h_flen[k] = h_flen[k] + G.first; G.h_pkts[k] = h_pkts[k] + o_pkts; G.h_plen[k] = h_plen[k] + o_slots;
            G.h_frags[k] = h_frags[k] + o_frags; G.h_fraglen[k] = h_fraglen[k] + o_fragslots; G.h_nfrag[k] = h_nfrag[k] + o_slots;
        }
        o_frames += n * (size_t)G.out_stride; o_slots += slots; o_pkts += slots * (size_t)G.af_stride; o_msgs += slots * (size_t)G.msg_stride;
        o_fragslots += slots * (size_t)G.max_frags; o_frags += slots * (size_t)G.max_frags * (size_t)G.frag_stride;
        st0.resize(n);
        for (size_t i = 0; i < n; i++) tlb_edi_state_init(&st0[i], tc->now_s, tc->delay_ms, tc->tist, tc->tai_utc_offset);
        HIPCHK(hipMemcpy(G.d_state, st0.data(), n * sizeof(tlb_edi_state), hipMemcpyHostToDevice));
        HIPCHK(hipEventCreateWithFlags(&G.ev_in, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&G.ev_run, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&G.ev_ingested, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&G.ev_encoded, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&G.ev_out, hipEventDisableTiming));
    }
    HIPCHK(hipStreamCreateWithFlags(&t->s_in, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&t->s_run, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&t->s_out, hipStreamNonBlocking));
    for (int k = 0; k < 3; k++) { HIPCHK(hipEventCreate(&t->ev0[k])); HIPCHK(hipEventCreate(&t->ev1[k])); }
    return TLB_OK;
}

tlb_tick *tlb_tick_create(int device, int nstreams, const tlb_stream_config *cfgs, const tlb_tick_config *tc, int *err)
{
    if (nstreams <= 0 || !cfgs || !tc) { if (err) *err = TLB_ERR_ARG; return nullptr; }
    tlb_tick *t = new tlb_tick;
    const int rc = tick_create_impl(t, device, nstreams, cfgs, tc);
    if (err) *err = rc;
    if (rc) { tlb_tick_destroy(t); return nullptr; }
    return t;
}

// the group that owns a stream and the stream's id inside it (t->blocks); NULL for no object and for a stream outside it
static const TickGroup *tick_group_of(const tlb_tick *t, int stream, int *local)
{
    const int g = t ? t->blocks.owner(stream, local) : -1;
    return g < 0 ? nullptr : &t->groups[(size_t)g];
}

// The input accessors hand out the set the NEXT submit will read.  With two ticks in flight both sets belong to queued copy-ins (the
// set these would name is the one the older tick's host-to-device copy may still be reading): NULL until tlb_tick_wait() has
// retired that tick -- no submit is possible in that state anyway.
static bool tick_input_free(const tlb_tick *t) { return t && !t->finished && !t->broken && t->ticks - t->waited < 2; }
int16_t *tlb_tick_pcm(tlb_tick *t) { return tick_input_free(t) ? t->h_inter[t->in_set] : nullptr; }
uint8_t *tlb_tick_xpad(tlb_tick *t) { return tick_input_free(t) && t->with_xpad ? t->h_xpad[t->in_set] : nullptr; }
int32_t *tlb_tick_xpad_len(tlb_tick *t) { return tick_input_free(t) && t->with_xpad ? t->h_xl[t->in_set] : nullptr; }
const int16_t *tlb_tick_peaks(const tlb_tick *t) { return t ? t->h_peaks[t->out_set] : nullptr; }
int32_t *tlb_tick_valid(tlb_tick *t) { return tick_input_free(t) && t->short_reads ? t->h_valid[t->in_set] : nullptr; }
const uint32_t *tlb_tick_underrun_ms(const tlb_tick *t) { return t && t->short_reads ? t->h_underrun_ms[t->out_set] : nullptr; }
const uint32_t *tlb_tick_underruns(const tlb_tick *t) { return t && t->short_reads ? t->h_underruns[t->out_set] : nullptr; }
// Short reads are opted into by this call, before the first submit: the object then carries `valid` per stream in with the PCM, runs the
// ingest kernel that stretches (tlb_ingest_device_valid) and the underrun counters (tlb_underrun_device).  An object that never makes the
// call makes the device calls it always made.
int tlb_tick_enable_short_reads(tlb_tick *t)
{
    if (!t || t->finished || t->ticks > 0 || !tick_may_set(t, TLB_IN_SHORT_READS)) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (t->short_reads) return TLB_OK;
    HIPCHK(hipSetDevice(t->device));
    const size_t ns = (size_t)t->nstreams;
    int32_t *h_valid[2]; uint32_t *h_ms[3], *h_n[3];
    if (int rc = tick_opt_in(t, [&](TlbMem &m, std::vector<TickGroup> &gs) {
            for (int k = 0; k < 2; k++) h_valid[k] = m.pinned<int32_t>(ns);
            for (int k = 0; k < 3; k++) { h_ms[k] = m.pinned<uint32_t>(ns); h_n[k] = m.pinned<uint32_t>(ns); }
            for (auto &G : gs) { G.d_valid = m.dev<int32_t>((size_t)G.n); G.d_underrun_ms = m.dev<uint32_t>((size_t)G.n); G.d_underruns = m.dev<uint32_t>((size_t)G.n); }
            return 0;
        })) return rc;
    for (int k = 0; k < 2; k++) for (size_t i = 0; i < ns; i++) h_valid[k][i] = TLB_SAMPLES_PER_FRAME;
    memcpy(t->h_valid, h_valid, sizeof h_valid); memcpy(t->h_underrun_ms, h_ms, sizeof h_ms); memcpy(t->h_underruns, h_n, sizeof h_n);
    t->short_reads = true;
    return TLB_OK;
}
// The confidence monitor, a record option (tick_record_enable): the object then queues tlb_decode_device and the fold (tlb_monitor_device) behind every tick's egress kernels.  The
// decoder's tables and state are made here, not by the first tick (the first decode call of a batch waits for the device once).  An object
// that never makes the call makes the device calls it always made.
int tlb_tick_enable_monitor(tlb_tick *t, int what)
{
    if (!t || t->finished || t->ticks > 0 || (what != TLB_MONITOR_CHECK && what != TLB_MONITOR_AUDIO)) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (t->monitor) return t->monitor == what ? (int)TLB_OK : (int)TLB_ERR_ARG;
    const size_t pcm = 2 * TLB_SAMPLES_PER_FRAME;
    void *h_listen[3];
    if (int rc = tick_record_enable(t, REC_MONITOR, [&](TlbMem &m, TickGroup &G) {
            if (int rc = decode_prepare(G.b)) return rc;
            G.d_report = m.dev<tlb_frame_report>((size_t)G.n);
            if (what == TLB_MONITOR_AUDIO) G.d_mpcm = m.dev<int16_t>((size_t)G.n * pcm);
            return 0;
        }, pcm * sizeof(int16_t), h_listen)) return rc;
    memcpy(t->h_listen, h_listen, sizeof h_listen);
    t->monitor = what;
    return TLB_OK;
}
const tlb_monitor_record *tlb_tick_monitor(const tlb_tick *t) { return (const tlb_monitor_record *)tick_record(t, REC_MONITOR); }
// The compare monitor on top of it: the tick's planar PCM (d_pcm, what the encoder is given) against the decoded PCM of the frame that
// leaves in the same tick (d_mpcm), through the history of the group's batch -- made here, not by the first tick.  Opt-in like the rest.
int tlb_tick_enable_compare(tlb_tick *t, const tlb_compare_params *params)
{
    if (!t || !params || t->finished || t->ticks > 0 || t->monitor != TLB_MONITOR_AUDIO) return TLB_ERR_ARG;
    if (!tlb_compare_params_legal(params)) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (t->rec[REC_COMPARE].on) return tlb_compare_params_same(*params, t->cparams) ? (int)TLB_OK : (int)TLB_ERR_ARG;
    if (int rc = tick_record_enable(t, REC_COMPARE, [](TlbMem &, TickGroup &G) { return compare_prepare(G.b); })) return rc;
    t->cparams = *params;
    return TLB_OK;
}
const tlb_compare_record *tlb_tick_compare(const tlb_tick *t) { return (const tlb_compare_record *)tick_record(t, REC_COMPARE); }
// The PCM meters (tlb_loudness_*, tlb_truepeak_*): the state of every group's batch is made here (the true-peak meter's with the one ceiling),
// and every submit with new input then queues the meter on the tick's planar PCM (d_pcm, what the encoder is given) behind the egress
// kernels, in table order.  An object that never makes the call allocates and queues nothing new.
static int tick_meter_enable(tlb_tick *t, int r, uint32_t ceiling)
{
    if (!t || t->finished || t->ticks > 0) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (t->rec[r].on) return TLB_OK;
    return tick_record_enable(t, r, [&](TlbMem &, TickGroup &G) { return tick_records[r].enable(G.b, ceiling); });
}
// ... a meter's reset of one stream or of all (-1): legal with no tick in flight
static int tick_meter_reset(tlb_tick *t, int r, int stream)
{
    if (!t || !t->rec[r].on || stream < -1 || stream >= t->nstreams || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    return t->blocks.visit(stream, [&](int g, int k) { return tick_records[r].reset(t->groups[(size_t)g].b, k); });
}
int tlb_tick_enable_loudness(tlb_tick *t) { return tick_meter_enable(t, REC_LOUDNESS, 0); }
const tlb_loudness_record *tlb_tick_loudness(const tlb_tick *t) { return (const tlb_loudness_record *)tick_record(t, REC_LOUDNESS); }
int tlb_tick_loudness_reset(tlb_tick *t, int stream) { return tick_meter_reset(t, REC_LOUDNESS, stream); }
// Programme loudness of every stream from the counts so far: legal with no tick in flight.
int tlb_tick_loudness_programme(tlb_tick *t, tlb_loudness_programme_record *out)
{
    if (!t || !out || !t->rec[REC_LOUDNESS].on || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    for (auto &G : t->groups) if (int rc = tlb_loudness_programme_host(G.b, out + G.first)) return rc;
    return TLB_OK;
}
// The loudness range on top of the meter (tlb_lra_*): the second histogram of every group's batch is made here; the meter's one launch per
// submit is then the counting kernel, and the tick's queue is what it was.
int tlb_tick_enable_lra(tlb_tick *t)
{
    if (!t || t->finished || t->ticks > 0 || !t->rec[REC_LOUDNESS].on) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    for (auto &G : t->groups) if (int rc = tlb_lra_enable(G.b)) return rc;
    t->lra = true;
    return TLB_OK;
}
// ... the range of every stream from the counts so far: legal with no tick in flight.
int tlb_tick_lra(tlb_tick *t, tlb_lra_record *out)
{
    if (!t || !out || !t->lra || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    for (auto &G : t->groups) if (int rc = tlb_lra_host(G.b, out + G.first)) return rc;
    return TLB_OK;
}
int tlb_tick_enable_truepeak(tlb_tick *t, uint32_t ceiling) { return tick_meter_enable(t, REC_TRUEPEAK, ceiling); }
const tlb_truepeak_record *tlb_tick_truepeak(const tlb_tick *t) { return (const tlb_truepeak_record *)tick_record(t, REC_TRUEPEAK); }
int tlb_tick_truepeak_reset(tlb_tick *t, int stream) { return tick_meter_reset(t, REC_TRUEPEAK, stream); }
// The true-peak limiter (tlb_limiter_*): the state of every group's batch is made here, and every submit then queues the limiter on the
// tick's planar PCM behind the ingest and ahead of the encoder (tlb_tick_submit).  An object that never makes the call allocates and queues
// nothing new.
int tlb_tick_enable_limiter(tlb_tick *t, const tlb_limiter_params *params)
{
    if (!t || t->finished || t->ticks > 0) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (t->rec[REC_LIMITER].on) return tlb_limiter_enable(t->groups[0].b, params);      // (equal parameters: 0, others: TLB_ERR_ARG)
    return tick_record_enable(t, REC_LIMITER, [&](TlbMem &, TickGroup &G) { return tlb_limiter_enable(G.b, params); });
}
const tlb_limiter_record *tlb_tick_limiter(const tlb_tick *t) { return (const tlb_limiter_record *)tick_record(t, REC_LIMITER); }
int tlb_tick_limiter_reset(tlb_tick *t, int stream) { return tick_meter_reset(t, REC_LIMITER, stream); }
// The feed concealment (tlb_conceal_*): per stream, while no tick is in flight.  Every named stream is checked before one is changed; the first
// call that switches concealment on makes the record option's buffers.  The kernels are the feed launch's own business (feed_launch); every
// submit then copies the batches' records into the groups' behind it.  An object that never makes the call allocates and queues nothing new.
// any_feed (tlb_tick_enable_feed_loss): an adapted or a down feed will do, and the batches are asked through tlb_feed_loss_enable
static int tick_enable_conceal(tlb_tick *t, int stream, int hold, int step, bool any_feed)
{
    if (!t || t->finished || stream < -1 || stream >= t->nstreams || t->ticks != t->waited) return TLB_ERR_ARG;
    if (hold < 0 || hold > TLB_CONCEAL_MAX_HOLD || (hold > 0 && (step < 1 || step > TLB_CONCEAL_MAX_STEP))) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (hold == 0 && !t->rec[REC_CONCEAL].on) return TLB_OK;         // off, and never on
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? t->nstreams : stream + 1;
    if (hold > 0)
        if (int rc = t->blocks.visit_range(s0, s1, [&](int g, int l0, int l1) {
                const tlb_batch *b = t->groups[(size_t)g].b;
                for (int k = l0; k < l1; k++) {
                    const bool strict = tlb_feed_get(b, k, nullptr) > 0 && tlb_feed_adapted(b, k) == 0;
                    if (!strict && !(any_feed && (tlb_feed_get(b, k, nullptr) > 0 || tlb_feed_down_get(b, k, nullptr) > 0))) return (int)TLB_ERR_ARG;
                }
                return (int)TLB_OK;
            })) return rc;
    if (!t->rec[REC_CONCEAL].on) if (int rc = tick_record_enable(t, REC_CONCEAL, [](TlbMem &, TickGroup &) { return 0; })) return rc;
    return t->blocks.visit(stream, [&](int g, int k) { return (any_feed ? tlb_feed_loss_enable : tlb_conceal_enable)(t->groups[(size_t)g].b, k, hold, step); });
}
int tlb_tick_enable_conceal(tlb_tick *t, int stream, int hold, int step) { return tick_enable_conceal(t, stream, hold, step, false); }
int tlb_tick_enable_feed_loss(tlb_tick *t, int stream, int hold, int step) { return tick_enable_conceal(t, stream, hold, step, true); }
const tlb_conceal_record *tlb_tick_conceal(const tlb_tick *t) { return (const tlb_conceal_record *)tick_record(t, REC_CONCEAL); }
int tlb_tick_conceal_reset(tlb_tick *t, int stream) { return tick_meter_reset(t, REC_CONCEAL, stream); }
int tlb_tick_monitor_listen(tlb_tick *t, int stream)
{
    if (!t || t->monitor != TLB_MONITOR_AUDIO || stream < -1 || stream >= t->nstreams) return TLB_ERR_ARG;
    t->listen = stream;
    return TLB_OK;
}
const int16_t *tlb_tick_monitor_pcm(const tlb_tick *t, int *stream)
{
    const int s = t && t->monitor == TLB_MONITOR_AUDIO ? t->listen_of[t->out_set] : -1;
    if (stream) *stream = s;
    return s >= 0 ? t->h_listen[t->out_set] : nullptr;
}
// A source rate (tlb_resample_set_source of the group's batch) or a DOWN source (tlb_decimate_set_source) for one stream or all, while no tick is
// in flight.  The first real source gives every group its second device input buffer (d_rs), and from then on every submit runs the resampler;
// the first real down source gives the object its pinned wide buffers and every group its device one, and from then on, while some stream has
// a down source, every submit copies the wide slices of the groups that have one and runs the decimator ahead of their ingest.  An object that
// never sets one makes the device calls it always made.
static int tick_set_rate(tlb_tick *t, int stream, long source_rate, bool down)
{
    if (!t || t->finished || stream < -1 || stream >= t->nstreams || source_rate < 0 || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    const auto pairs = down ? tlb_down_pair : tlb_up_pair;
    const auto prepare = down ? decimate_prepare : resample_prepare;
    const auto set = down ? tlb_decimate_set_source : tlb_resample_set_source;
    const auto get = down ? tlb_decimate_source : tlb_resample_source;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? t->nstreams : stream + 1;
    bool any = false;
    std::vector<char> real(t->groups.size(), 0);                     // per group: the call gives some stream of it a real source
    if (int rc = t->blocks.visit_range(s0, s1, [&](int g, int l0, int l1) {     // every stream is checked before one is changed
            const tlb_batch *b = t->groups[(size_t)g].b;
            bool r = false;
            const int e = tlb_rate_range(l0, l1, source_rate, pairs, [b](int k) { return batch_enc_rate(b, k); }, &r);
            real[(size_t)g] = r; any |= r;
            return e;
        })) return rc;
    const bool made = down ? t->h_wide[0] != nullptr : t->groups[0].d_rs != nullptr;
    if (!any && !made) return TLB_OK;                                // off, and never on: nothing to allocate or to clear
    if (any && !tick_may_set(t, down ? TLB_IN_DOWN_SOURCE : TLB_IN_UP_SOURCE)) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(t->device));
    if (!made) {                                                     // first real source: the buffers, and the resampler or decimator of the batches that get
        int16_t *h[2] = {};                                          // one, before anything is committed or a stream is changed
        if (int rc = tick_opt_in(t, [&](TlbMem &m, std::vector<TickGroup> &gs) {
                for (int k = 0; k < 2 && down; k++) h[k] = m.pinned<int16_t>((size_t)t->nstreams * TLB_DECIMATE_SLOT);
                for (auto &G : gs) (down ? G.d_wide : G.d_rs) = m.dev<int16_t>((size_t)G.n * (down ? TLB_DECIMATE_SLOT : 2304));
                for (size_t g = 0; g < gs.size(); g++) if (real[g]) if (int rc = prepare(gs[g].b)) return rc;
                return 0;
            })) return rc;
        if (down) memcpy(t->h_wide, h, sizeof h);
    }
    const int rc = t->blocks.visit(stream, [&](int g, int k) { return set(t->groups[(size_t)g].b, k, source_rate); });
    bool on = false;                                                 // "at least one source set", as the streams stand now
    for (auto &G : t->groups) {
        int n = 0;
        for (int k = 0; k < G.n; k++) n += get(G.b, k) != 0;
        if (down) { G.any_down = n > 0; G.all_down = n == G.n; }
        on |= n > 0;
    }
    (down ? t->down : t->resample) = on;
    return rc;
}
int tlb_tick_set_source(tlb_tick *t, int stream, long source_rate) { return tick_set_rate(t, stream, source_rate, false); }
int tlb_tick_set_down_source(tlb_tick *t, int stream, long source_rate) { return tick_set_rate(t, stream, source_rate, true); }
int16_t *tlb_tick_down(tlb_tick *t, int stream)
{
    if (!tick_input_free(t) || !t->down || stream < 0 || stream >= t->nstreams) return nullptr;
    return t->h_wide[t->in_set] + (size_t)stream * TLB_DECIMATE_SLOT;
}
int tlb_tick_down_need(const tlb_tick *t, int stream)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    return G ? tlb_decimate_need(G->b, k, 0) : -TLB_ERR_ARG;
}
// A feed of the lane's family for one stream or all (the family's set of the group's batch), while no tick is in flight.  The lane's first feed
// gives the object its pinned buffers and every group its device ones; a wider feed than any before replaces the frame buffers (RE-FETCH).  An
// object that never sets one makes the device calls it always made.
static void tick_lane_refresh(tlb_tick *t, int lane)
{
    TickLane &L = t->lane[lane];
    const FeedFamily &F = tick_families[lane];
    L.on = false;
    for (auto &G : t->groups) {
        TickLaneGroup &LG = G.lane[lane];
        int fed = 0;
        bool adapted;
        for (int k = 0; k < G.n; k++) fed += F.get(G.b, k, nullptr, &adapted) > 0;
        LG.any = fed > 0; LG.all = fed == G.n;
        L.on |= LG.any;
        // a group without a fed stream runs no kernel of the family: its slots read EMPTY (no tick is in flight, or the device has been waited for)
        if (!LG.any && L.h_report[0])
            for (int k = 0; k < 3; k++) for (int i = 0; i < F.slots * G.n; i++) { tlb_frame_report r = {}; r.status = TLB_DEC_EMPTY; L.h_report[k][F.slots * G.first + i] = r; }
    }
}
static int tick_lane_set(tlb_tick *t, int lane, int stream, const tlb_feed_config *cfg, bool adapt)
{
    if (!t || t->finished || stream < -1 || stream >= t->nstreams || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    TickLane &L = t->lane[lane];
    const FeedFamily &F = tick_families[lane];
    if (!cfg && !L.h_len[0]) return TLB_OK;                          // off, and never on: nothing to allocate or to clear
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? t->nstreams : stream + 1;
    if (cfg) {
        if (!tick_may_set(t, F.input)) return TLB_ERR_ARG;
        // every stream is checked before one is changed
        if (int rc = t->blocks.visit_range(s0, s1, [&](int g, int l0, int l1) { return F.fits(t->groups[(size_t)g].b, l0, l1, cfg, adapt); })) return rc;
    }
    HIPCHK(hipSetDevice(t->device));
    const size_t ns = (size_t)t->nstreams, per = (size_t)F.slots;
    if (!L.h_len[0]) {                                               // the lane's first feed: lengths and reports, made once
        int32_t *h_len[2]; tlb_frame_report *h_rep[3];
        if (int rc = tick_opt_in(t, [&](TlbMem &m, std::vector<TickGroup> &gs) {
                for (int k = 0; k < 2; k++) h_len[k] = m.pinned<int32_t>(per * ns);
                for (int k = 0; k < 3; k++) h_rep[k] = m.pinned<tlb_frame_report>(per * ns);
                for (auto &G : gs) { G.lane[lane].d_len = m.dev<int32_t>(per * (size_t)G.n); G.lane[lane].d_report = m.dev<tlb_frame_report>(per * (size_t)G.n); }
                return 0;
            })) return rc;
        memcpy(L.h_len, h_len, sizeof h_len); memcpy(L.h_report, h_rep, sizeof h_rep);
    }
    const int want = cfg ? feed_slot_bytes(cfg) : 0;
    if (want > L.stride) {                                           // wider slots: new frame buffers, all of them before any is let go (no tick is in flight)
        std::unique_ptr<TlbMem> m(new TlbMem);                       // stage, settle, then the owners change places: the narrower buffers go with the old one
        uint8_t *h[2];
        std::vector<uint8_t *> d(t->groups.size(), nullptr);
        for (int k = 0; k < 2; k++) h[k] = m->pinned<uint8_t>(per * ns * (size_t)want);
        for (size_t g = 0; g < d.size(); g++) d[g] = m->scratch<uint8_t>(per * (size_t)t->groups[g].n * (size_t)want);
        if (!m->settle()) return TLB_ERR_HIP;
        L.mem.swap(m);
        for (int k = 0; k < 2; k++) L.h_frames[k] = h[k];
        for (size_t g = 0; g < d.size(); g++) t->groups[g].lane[lane].d_frames = d[g];
        L.stride = want;
    }
    // what the named streams have now: after a device failure half way the groups already changed get it back (fresh history), so that
    // "all or nothing" holds for the feeds themselves; the wider buffers stay
    std::vector<tlb_feed_config> before(ns, tlb_feed_config{0, 0, 0});
    std::vector<char> before_adapted(ns, 0);
    for (auto &G : t->groups) for (int k = 0; k < G.n; k++) {
        bool a = false;
        (void)F.get(G.b, k, &before[(size_t)(G.first + k)], &a);
        before_adapted[(size_t)(G.first + k)] = a;
    }
    const int rc = t->blocks.visit(stream, [&](int g, int k) {
        const int e = F.set(t->groups[(size_t)g].b, k, cfg, adapt);
        if (e) t->blocks.visit_range(s0, s1, [&](int u, int l0, int l1) {      // the named streams of the groups up to and including this one
            const TickGroup &U = t->groups[(size_t)u];
            for (int i = l0; i < l1 && u <= g; i++) {
                const tlb_feed_config &f = before[(size_t)(U.first + i)];
                (void)F.set(U.b, i, f.bitrate ? &f : nullptr, before_adapted[(size_t)(U.first + i)] != 0);
            }
            return 0;
        });
        return e;
    });
    tick_lane_refresh(t, lane);
    for (int k = 0; k < 2; k++) memset(L.h_len[k], 0, per * ns * sizeof(int32_t));
    return rc;
}
// the lane's accessors: the feed frames wanted in the stream's slots of the input set to fill next (the group's batch advances its position with
// every submit); the input set's frames and lengths, the slot width, the reports of the tick waited for last
static int tick_lane_want(const tlb_tick *t, int lane, int stream)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    return G ? tick_families[lane].want(G->b, k, 0) : -TLB_ERR_ARG;
}
static uint8_t *tick_lane_frames(tlb_tick *t, int lane) { return tick_input_free(t) && t->lane[lane].on ? t->lane[lane].h_frames[t->in_set] : nullptr; }
static int32_t *tick_lane_len(tlb_tick *t, int lane) { return tick_input_free(t) && t->lane[lane].on ? t->lane[lane].h_len[t->in_set] : nullptr; }
static int tick_lane_stride(const tlb_tick *t, int lane) { return t && t->lane[lane].on ? t->lane[lane].stride : 0; }
static const tlb_frame_report *tick_lane_report(const tlb_tick *t, int lane) { return t && t->lane[lane].on ? t->lane[lane].h_report[t->out_set] : nullptr; }
int tlb_tick_set_feed(tlb_tick *t, int stream, const tlb_feed_config *cfg) { return tick_lane_set(t, LANE_FEED, stream, cfg, false); }
int tlb_tick_set_feed_adapted(tlb_tick *t, int stream, const tlb_feed_config *cfg) { return tick_lane_set(t, LANE_FEED, stream, cfg, true); }
int tlb_tick_feed_want(const tlb_tick *t, int stream) { return tick_lane_want(t, LANE_FEED, stream); }
uint8_t *tlb_tick_feed(tlb_tick *t) { return tick_lane_frames(t, LANE_FEED); }
int32_t *tlb_tick_feed_len(tlb_tick *t) { return tick_lane_len(t, LANE_FEED); }
int tlb_tick_feed_stride(const tlb_tick *t) { return tick_lane_stride(t, LANE_FEED); }
const tlb_frame_report *tlb_tick_feed_report(const tlb_tick *t) { return tick_lane_report(t, LANE_FEED); }
int tlb_tick_set_down_feed(tlb_tick *t, int stream, const tlb_feed_config *cfg) { return tick_lane_set(t, LANE_DOWN_FEED, stream, cfg, false); }
int tlb_tick_down_feed_want(const tlb_tick *t, int stream) { return tick_lane_want(t, LANE_DOWN_FEED, stream); }
uint8_t *tlb_tick_down_feed(tlb_tick *t) { return tick_lane_frames(t, LANE_DOWN_FEED); }
int32_t *tlb_tick_down_feed_len(tlb_tick *t) { return tick_lane_len(t, LANE_DOWN_FEED); }
int tlb_tick_down_feed_stride(const tlb_tick *t) { return tick_lane_stride(t, LANE_DOWN_FEED); }
const tlb_frame_report *tlb_tick_down_feed_report(const tlb_tick *t) { return tick_lane_report(t, LANE_DOWN_FEED); }
int tlb_tick_need(const tlb_tick *t, int stream)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    return G ? tlb_resample_need(G->b, k, 0) : -TLB_ERR_ARG;
}
long tlb_tick_count(const tlb_tick *t) { return t ? t->ticks : 0; }
int tlb_tick_set_gain_db(tlb_tick *t, int stream, double gain_db)
{
    if (!t || stream < -1 || stream >= t->nstreams) return TLB_ERR_ARG;
    return t->blocks.visit(stream, [&](int g, int k) { return tlb_set_gain_db(t->groups[(size_t)g].b, k, gain_db); });
}

// Life cycle of one stream of a tick object (tlb_stream_reset / _finish / _reconfigure of its group's batch).  The EDI sender state
// of the stream (SEQ, DLFC, timestamps) is NOT touched: the receiver sees one continuous sender whose encoder was restarted, as
// with the reference, whose output object outlives an encoder re-initialisation.  Until the stream's next frame is final its
// slots are empty (length 0).
int tlb_tick_stream_reset(tlb_tick *t, int stream)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->finished) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    return tlb_stream_reset(G->b, k);
}
int tlb_tick_stream_finish(tlb_tick *t, int stream, uint8_t *out, size_t out_size)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->finished) return -TLB_ERR_ARG;
    if (t->broken) return -TLB_ERR_HIP;
    return tlb_stream_finish(G->b, k, out, out_size);
}
int tlb_tick_stream_reconfigure(tlb_tick *t, int stream, const tlb_stream_config *cfg)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->finished) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    const int rc = tlb_stream_reconfigure(G->b, k, cfg);
    for (int lane = 0; lane < LANES; lane++) if (t->lane[lane].on) tick_lane_refresh(t, lane);      // (a feed the stream's new rate or channel count no longer fits has been removed)
    return rc;
}

// the copy-out of a record option's records of this tick, queued on s_out; `wait`: behind the option's event (something wrote them this tick)
static int tick_record_out(tlb_tick *t, TickGroup &G, int r, int set, bool wait)
{
    const RecordOption &R = tick_records[r];
    if (wait) HIPCHK(hipStreamWaitEvent(t->s_out, G.ev_rec[R.ev], 0));
    HIPCHK(hipMemcpyAsync((uint8_t *)t->rec[r].h[set] + (size_t)G.first * R.size, G.d_rec[r], (size_t)G.n * R.size, hipMemcpyDeviceToHost, t->s_out));
    return TLB_OK;
}
// egress of the frames sitting in G.d_frames + copy-out, queued on s_run / s_out
static int tick_egress(tlb_tick *t, TickGroup &G, bool have_frames, int set, bool new_input = true)
{
    const size_t n = (size_t)G.n, slots = n * (size_t)G.max_upf;
#ifdef TLB_FAULT_INJECT
    if (have_frames && t->cross_on && t->cross_a >= G.first && t->cross_a < G.first + G.n) if (int rc = tick_cross(t, G)) return rc;
#endif
    if (new_input) if (int rc = tlb_silence_device(G.b, G.d_peaks, 1, G.d_silence, t->s_run)) return rc;       // odr-audioenc.cpp:1053-1079 (the decision stays with the caller)
    if (have_frames && t->egress == TLB_TICK_ZMQ) {
        if (int rc = zmq_frame_device(G.b, G.d_frames, G.d_peaks, 1, G.d_msgs, t->s_run, G.d_flen)) return rc;
    } else if (have_frames && t->egress != TLB_TICK_FRAMES) {
        if (int rc = edi_af_device(G.b, G.d_frames, G.d_peaks, 1, G.d_state, t->version, t->version_len, G.d_pkts, G.d_plen, t->s_run, G.d_flen)) return rc;
        if (t->egress == TLB_TICK_EDI_PFT)
            if (int rc = tlb_edi_pft_device(G.b, G.d_pkts, G.d_plen, G.max_upf, G.af_stride, G.d_pseq, t->fec, t->chunk_len, t->transport, t->addr_source, t->dest_port,
                                            G.d_frags, G.d_fraglen, G.d_nfrag, G.max_frags, G.frag_stride, t->s_run)) return rc;
    }
    HIPCHK(hipEventRecord(G.ev_run, t->s_run));
    const bool compare = t->rec[REC_COMPARE].on;
    if (t->monitor && have_frames) {                                 // behind the egress kernels: the packets' copy-out waits for ev_run only
        if (int rc = tlb_decode_device(G.b, G.d_frames, G.d_flen, 1, G.d_report, nullptr, G.d_mpcm, t->s_run)) return rc;
        if (int rc = tlb_monitor_device(G.b, G.d_report, G.d_mpcm, 1, (tlb_monitor_record *)G.d_rec[REC_MONITOR], t->s_run)) return rc;
        if (!compare) HIPCHK(hipEventRecord(G.ev_rec[REC_MONITOR], t->s_run));
    }
    if (compare) {                                                   // behind the decode: this tick's input against the frame that leaves with it.  The first
        // tick has no frame yet (no report: the slot counts as skipped) and only advances the history; the flush has no input and does not advance it
        if (int rc = compare_launch(G.b, new_input ? G.d_pcm : nullptr, G.d_mpcm, have_frames ? G.d_report : nullptr, 1, &t->cparams, (tlb_compare_record *)G.d_rec[REC_COMPARE], t->s_run)) return rc;
        HIPCHK(hipEventRecord(G.ev_rec[REC_MONITOR], t->s_run));
    }
    for (int r = 0; r < RECS && new_input; r++) {                    // the meters that are on, one behind the other, on the PCM that went IN this tick
        if (!t->rec[r].on || !tick_records[r].launch) continue;      // (the flush has none: its set shows the same records)
        if (int rc = tick_records[r].launch(G.b, G.d_pcm, 1, G.d_rec[r], t->s_run)) return rc;
        HIPCHK(hipEventRecord(G.ev_rec[r], t->s_run));
    }
    HIPCHK(hipStreamWaitEvent(t->s_out, G.ev_run, 0));
    HIPCHK(hipMemcpyAsync(t->h_peaks[set] + (size_t)G.first * 2, G.d_peaks, n * 4, hipMemcpyDeviceToHost, t->s_out));
    HIPCHK(hipMemcpyAsync(t->h_silence[set] + G.first, G.d_silence, n * 4, hipMemcpyDeviceToHost, t->s_out));
    // (tlb_tick_finish runs no feed kernel: its set shows the last tick's reports once more)
    for (int lane = 0; lane < LANES; lane++) {
        const size_t per = (size_t)tick_families[lane].slots;
        if (G.lane[lane].any) HIPCHK(hipMemcpyAsync(t->lane[lane].h_report[set] + per * (size_t)G.first, G.lane[lane].d_report, per * n * sizeof(tlb_frame_report), hipMemcpyDeviceToHost, t->s_out));
    }
    if (t->short_reads) {
        HIPCHK(hipMemcpyAsync(t->h_underrun_ms[set] + G.first, G.d_underrun_ms, n * 4, hipMemcpyDeviceToHost, t->s_out));
        HIPCHK(hipMemcpyAsync(t->h_underruns[set] + G.first, G.d_underruns, n * 4, hipMemcpyDeviceToHost, t->s_out));
    }
    if (have_frames) {                                               // (the very first tick: no frame is final yet, lengths stay 0)
        if (t->egress == TLB_TICK_FRAMES) {
            HIPCHK(hipMemcpyAsync(G.h_frames[set], G.d_frames, n * (size_t)G.out_stride, hipMemcpyDeviceToHost, t->s_out));
            HIPCHK(hipMemcpyAsync(G.h_flen[set], G.d_flen, n * 4, hipMemcpyDeviceToHost, t->s_out));
        } else if (t->egress == TLB_TICK_ZMQ) {
            HIPCHK(hipMemcpyAsync(G.h_msgs[set], G.d_msgs, slots * (size_t)G.msg_stride, hipMemcpyDeviceToHost, t->s_out));
        } else if (t->egress == TLB_TICK_EDI_AF) {
            HIPCHK(hipMemcpyAsync(G.h_pkts[set], G.d_pkts, slots * (size_t)G.af_stride, hipMemcpyDeviceToHost, t->s_out));
            HIPCHK(hipMemcpyAsync(G.h_plen[set], G.d_plen, slots * 4, hipMemcpyDeviceToHost, t->s_out));
        } else {
            HIPCHK(hipMemcpyAsync(G.h_frags[set], G.d_frags, slots * (size_t)G.max_frags * (size_t)G.frag_stride, hipMemcpyDeviceToHost, t->s_out));
            HIPCHK(hipMemcpyAsync(G.h_fraglen[set], G.d_fraglen, slots * (size_t)G.max_frags * 4, hipMemcpyDeviceToHost, t->s_out));
            HIPCHK(hipMemcpyAsync(G.h_nfrag[set], G.d_nfrag, slots * 4, hipMemcpyDeviceToHost, t->s_out));
        }
    }
    if (t->monitor) {                                                // the records (and the listened stream's frame) behind the packets
        if (int rc = tick_record_out(t, G, REC_MONITOR, set, have_frames || compare)) return rc;
        if (compare) if (int rc = tick_record_out(t, G, REC_COMPARE, set, false)) return rc;     // (the monitor's event is theirs too)
        const int k = t->listen_of[set] - G.first;
        if (G.d_mpcm && k >= 0 && k < G.n)
            HIPCHK(hipMemcpyAsync(t->h_listen[set], G.d_mpcm + (size_t)k * 2 * TLB_SAMPLES_PER_FRAME, 2 * TLB_SAMPLES_PER_FRAME * sizeof(int16_t), hipMemcpyDeviceToHost, t->s_out));
    }
    for (int r = 0; r < RECS; r++)                                   // ... and the meters' records, each on an event of its own
        if (t->rec[r].on && (tick_records[r].launch || r == REC_LIMITER || r == REC_CONCEAL)) if (int rc = tick_record_out(t, G, r, set, new_input)) return rc;
    HIPCHK(hipEventRecord(G.ev_out, t->s_out));                      // the group's device output buffers are free again once this has passed (the monitor's reads of d_frames included)
    return TLB_OK;
}

static void tick_drain(tlb_tick *t) { (void)hipStreamSynchronize(t->s_in); (void)hipStreamSynchronize(t->s_run); (void)hipStreamSynchronize(t->s_out); }
static int tick_fail(tlb_tick *t, int rc)
{
    tick_drain(t);
    if (!t->broken) fprintf(stderr, "libtoolame-dab-hip: a tick failed half way (code %d): its stream groups are out of step, the tick object refuses further work; destroy it\n", rc);
    t->broken = true;
    return rc;
}
int tlb_tick_status(const tlb_tick *t) { return !t ? TLB_ERR_ARG : t->broken ? TLB_ERR_HIP : TLB_OK; }
#ifdef TLB_FAULT_INJECT
// test builds only (csrc/tlb_debug.h): the nth submit from now fails in its LAST group -- after the groups before it have been queued
int tlb_debug_tick_fail_next(tlb_tick *t, int nth) { if (!t || nth < 0) return TLB_ERR_ARG; t->groups.back().b->fail_in = nth; return TLB_OK; }
// ... the nth submit from now XORs one byte of that stream's slot in d_frames, between the encode and the egress: what the caller receives
// and what the monitor sees are the same damaged bytes.  Host-queued copies on s_run, the stream waited for in between: nothing faults.
int tlb_debug_tick_damage_next(tlb_tick *t, int stream, int byte, int xor_mask, int nth)
{
    if (!t || nth < 0 || stream < 0 || stream >= t->nstreams || byte < 0 || byte >= t->groups[(size_t)t->blocks.owner(stream)].out_stride) return TLB_ERR_ARG;
    t->damage_nth = nth; t->damage_stream = stream; t->damage_byte = byte; t->damage_xor = (uint8_t)xor_mask;
    return TLB_OK;
}
// ... from the nth submit from now ON (tlb_tick_finish included) the slots of streams a and b in d_frames / d_flen are exchanged between the
// encode and the egress, tick after tick: the indexing fault of a batched encoder -- stream a's slot holds stream b's programme, in frames
// that are valid in every respect.  Both streams must lie in one group.  Device-to-device copies queued on s_run; nothing faults.
int tlb_debug_tick_cross_from(tlb_tick *t, int a, int b, int nth)
{
    if (!t || nth < 0 || a < 0 || b < 0 || a >= t->nstreams || b >= t->nstreams || a == b || t->blocks.owner(a) != t->blocks.owner(b)) return TLB_ERR_ARG;
    if (!t->d_cross_tmp) {
        HIPCHK(hipSetDevice(t->device));
        size_t widest = 0;                                           // one buffer for every later call: any group's slot fits
        for (auto &G : t->groups) if ((size_t)G.out_stride > widest) widest = (size_t)G.out_stride;
        TlbMem m;
        t->d_cross_tmp = m.scratch<uint8_t>(widest + 16);
        MEMCHK(m);
        m.commit(t->mem);
    }
    t->cross_nth = nth; t->cross_a = a; t->cross_b = b; t->cross_on = false;
    return TLB_OK;
}
static int tick_cross(tlb_tick *t, TickGroup &G)
{
    const size_t n = (size_t)G.out_stride;
    uint8_t *fa = G.d_frames + (size_t)(t->cross_a - G.first) * n, *fb = G.d_frames + (size_t)(t->cross_b - G.first) * n;
    int32_t *la = G.d_flen + (t->cross_a - G.first), *lb = G.d_flen + (t->cross_b - G.first);
    HIPCHK(hipMemcpyAsync(t->d_cross_tmp, fa, n, hipMemcpyDeviceToDevice, t->s_run));
    HIPCHK(hipMemcpyAsync(fa, fb, n, hipMemcpyDeviceToDevice, t->s_run));
    HIPCHK(hipMemcpyAsync(fb, t->d_cross_tmp, n, hipMemcpyDeviceToDevice, t->s_run));
    HIPCHK(hipMemcpyAsync(t->d_cross_tmp + n, la, 4, hipMemcpyDeviceToDevice, t->s_run));
    HIPCHK(hipMemcpyAsync(la, lb, 4, hipMemcpyDeviceToDevice, t->s_run));
    HIPCHK(hipMemcpyAsync(lb, t->d_cross_tmp + n, 4, hipMemcpyDeviceToDevice, t->s_run));
    return TLB_OK;
}
static int tick_damage(tlb_tick *t, TickGroup &G)
{
    uint8_t *p = G.d_frames + (size_t)(t->damage_stream - G.first) * (size_t)G.out_stride + (size_t)t->damage_byte;
    HIPCHK(hipMemcpyAsync(&t->damage_val, p, 1, hipMemcpyDeviceToHost, t->s_run));
    HIPCHK(hipStreamSynchronize(t->s_run));
    t->damage_val ^= t->damage_xor;
    HIPCHK(hipMemcpyAsync(p, &t->damage_val, 1, hipMemcpyHostToDevice, t->s_run));
    HIPCHK(hipStreamSynchronize(t->s_run));
    return TLB_OK;
}
#endif

// Queue one tick -- copy-in, ingest, encode, egress, copy-out of every group -- on the input set the caller has just filled, and
// return at once.  tlb_tick_pcm() then points at the OTHER input set: the caller fills the next tick while this one is on its way
// (odr-audioenc decouples capture from encoding with its input queue, src/odr-audioenc.cpp:904-986).  The device buffers of a group
// are single, so across ticks: the next copy-in waits for this tick's ingest kernel, the next kernels for this tick's copy-out --
// the host-to-device link, the limit at large stream counts, never idles between ticks.  At most two ticks may be in flight
// (two host sets): submit, submit, wait, submit, wait, ...
int tlb_tick_submit(tlb_tick *t)
{
    if (!t || t->finished || t->ticks - t->waited >= 2) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (hipSetDevice(t->device) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    const int set = (int)(t->ticks & 1);                             // == in_set: ticks and input sets alternate together
    const int oset = (int)(t->ticks % 3);                            // output set: the caller may still be reading tick - 2's
    if (hipEventRecord(t->ev0[oset], t->s_in) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    t->listen_of[oset] = t->monitor == TLB_MONITOR_AUDIO && t->ticks > 0 ? t->listen : -1;
#ifdef TLB_FAULT_INJECT
    const bool damage = t->damage_nth > 0 && --t->damage_nth == 0;
    if (t->cross_nth > 0 && --t->cross_nth == 0) t->cross_on = true;
#endif
    for (auto &G : t->groups) {
        const size_t n = (size_t)G.n;
        int rc = TLB_OK;
        hipError_t e = hipSuccess;
        if (t->ticks > 0) e = hipStreamWaitEvent(t->s_in, G.ev_ingested, 0);
        // a group all of whose streams have feeds of one family takes no PCM over the link: the family's kernels write every slot the ingest reads
        // ... nor does a group all of whose streams have down sources: its wide slice comes in instead and the decimator writes every slot
        if (e == hipSuccess && !G.lane[LANE_FEED].all && !G.all_down && !G.lane[LANE_DOWN_FEED].all) e = hipMemcpyAsync(G.d_inter, t->h_inter[set] + (size_t)G.first * 2304, n * 2304 * sizeof(int16_t), hipMemcpyHostToDevice, t->s_in);
        for (int lane = 0; lane < LANES; lane++) {
            const TickLane &L = t->lane[lane];
            const TickLaneGroup &LG = G.lane[lane];
            const size_t per = (size_t)tick_families[lane].slots;
            if (e == hipSuccess && LG.any) e = hipMemcpyAsync(LG.d_frames, L.h_frames[set] + per * (size_t)G.first * (size_t)L.stride, per * n * (size_t)L.stride, hipMemcpyHostToDevice, t->s_in);
            if (e == hipSuccess && LG.any) e = hipMemcpyAsync(LG.d_len, L.h_len[set] + per * (size_t)G.first, per * n * sizeof(int32_t), hipMemcpyHostToDevice, t->s_in);
        }
        if (e == hipSuccess && G.any_down) e = hipMemcpyAsync(G.d_wide, t->h_wide[set] + (size_t)G.first * TLB_DECIMATE_SLOT, n * TLB_DECIMATE_SLOT * sizeof(int16_t), hipMemcpyHostToDevice, t->s_in);
        if (e == hipSuccess && t->short_reads) e = hipMemcpyAsync(G.d_valid, t->h_valid[set] + G.first, n * sizeof(int32_t), hipMemcpyHostToDevice, t->s_in);
        if (e == hipSuccess && t->with_xpad && t->ticks > 0) e = hipStreamWaitEvent(t->s_in, G.ev_encoded, 0);
        if (e == hipSuccess && t->with_xpad) e = hipMemcpyAsync(G.d_xpad, t->h_xpad[set] + (size_t)G.first * TL_MAX_XPAD, n * TL_MAX_XPAD, hipMemcpyHostToDevice, t->s_in);
        if (e == hipSuccess && t->with_xpad) e = hipMemcpyAsync(G.d_xl, t->h_xl[set] + G.first, n * sizeof(int32_t), hipMemcpyHostToDevice, t->s_in);
        if (e == hipSuccess) e = hipEventRecord(G.ev_in, t->s_in);
        if (e == hipSuccess) e = hipStreamWaitEvent(t->s_run, G.ev_in, 0);
        if (e == hipSuccess && t->ticks > 0) e = hipStreamWaitEvent(t->s_run, G.ev_out, 0);
        if (e != hipSuccess) rc = TLB_ERR_HIP;
        for (int lane = 0; lane < LANES; lane++)                     // behind the copy-in, ahead of the ingest: a mixed group's fed slots are overwritten
            if (!rc && G.lane[lane].any) rc = tick_families[lane].launch(G.b, G.lane[lane].d_frames, G.lane[lane].d_len, 1, G.d_inter, G.lane[lane].d_report, t->s_run, t->lane[lane].stride);
        // the concealment's records as the feed launch has just left them (a group whose batch never enabled it shows zeros), on an event of their own
        if (!rc && t->rec[REC_CONCEAL].on && G.b->d_cc_rec) rc = tlb_conceal_records_device(G.b, (tlb_conceal_record *)G.d_rec[REC_CONCEAL], t->s_run);
        if (!rc && t->rec[REC_CONCEAL].on && hipEventRecord(G.ev_rec[REC_CONCEAL], t->s_run) != hipSuccess) rc = TLB_ERR_HIP;
        if (!rc && t->resample) rc = tlb_resample_device(G.b, G.d_inter, 1, G.d_rs, t->s_run);
        if (!rc && G.any_down) rc = tlb_decimate_device(G.b, G.d_wide, 1, G.d_inter, t->s_run);      // behind the copy-in, ahead of the ingest: a mixed group's decimated slots are overwritten
        if (!rc && !t->short_reads) rc = tlb_ingest_device(G.b, t->resample ? G.d_rs : G.d_inter, 1, G.d_pcm, G.d_peaks, t->s_run);
        if (!rc && t->short_reads) rc = tlb_ingest_device_valid(G.b, G.d_inter, G.d_valid, 1, G.d_pcm, G.d_peaks, t->s_run);
        // (the counters here and not with the silence counter: the next tick's copy-in may overwrite d_valid once ev_ingested has passed)
        if (!rc && t->short_reads) rc = tlb_underrun_device(G.b, G.d_valid, 1, G.d_underrun_ms, G.d_underruns, t->s_run);
        // the limiter, in place, between the ingest and the encoder: what follows sees the limited PCM; d_peaks stay the input's
        if (!rc && t->rec[REC_LIMITER].on) rc = tlb_limiter_device(G.b, G.d_pcm, 1, (tlb_limiter_record *)G.d_rec[REC_LIMITER], t->s_run);
        if (!rc && t->rec[REC_LIMITER].on && hipEventRecord(G.ev_rec[REC_LIMITER], t->s_run) != hipSuccess) rc = TLB_ERR_HIP;
        if (!rc && hipEventRecord(G.ev_ingested, t->s_run) != hipSuccess) rc = TLB_ERR_HIP;
        if (!rc) rc = tlb_launch(G.b, G.d_pcm, 1, t->with_xpad ? G.d_xpad : nullptr, t->with_xpad ? G.d_xl : nullptr, G.d_frames, nullptr, t->s_run, nullptr, G.d_flen);
        if (!rc && hipEventRecord(G.ev_encoded, t->s_run) != hipSuccess) rc = TLB_ERR_HIP;
#ifdef TLB_FAULT_INJECT
        if (!rc && damage && t->damage_stream >= G.first && t->damage_stream < G.first + G.n) rc = tick_damage(t, G);
#endif
        if (!rc) rc = tick_egress(t, G, t->ticks > 0, oset);
        if (rc) return tick_fail(t, rc);
    }
    if (hipEventRecord(t->ev1[oset], t->s_out) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    t->ticks++;
    t->in_set = (int)(t->ticks & 1);
    return TLB_OK;
}

// Wait for the oldest submitted tick; the read accessors then show ITS results until the next wait (three output sets: neither
// of the two ticks that can be submitted before that wait writes the set this one's results are in).
int tlb_tick_wait(tlb_tick *t)
{
    if (!t || t->waited >= t->ticks) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (hipSetDevice(t->device) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    const int set = (int)(t->waited % 3);
    if (hipEventSynchronize(t->ev1[set]) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    t->out_set = set;
    // the retired tick's input set goes back to the caller (now, or after the next submit): untouched streams are full reads
    if (t->short_reads) { int32_t *v = t->h_valid[t->waited & 1]; for (int i = 0; i < t->nstreams; i++) v[i] = TLB_SAMPLES_PER_FRAME; }
    for (int lane = 0; lane < LANES; lane++)                         // ... and feed slots are empty
        if (t->lane[lane].h_len[0]) memset(t->lane[lane].h_len[t->waited & 1], 0, (size_t)tick_families[lane].slots * (size_t)t->nstreams * sizeof(int32_t));
    t->waited++;
    return TLB_OK;
}

int tlb_tick_run(tlb_tick *t)
{   // one tick start to end: the accessors show its results when the call returns
    if (!t || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (int rc = tlb_tick_submit(t)) return rc;
    return tlb_tick_wait(t);
}

// end of the streams (toolame_finish): the pending frame of every stream through the egress stage; no further run
int tlb_tick_finish(tlb_tick *t)
{
    if (!t || t->finished || t->ticks == 0 || t->ticks != t->waited) return TLB_ERR_ARG;
    if (t->broken) return TLB_ERR_HIP;
    if (hipSetDevice(t->device) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    const int set = (int)(t->ticks % 3);
    t->listen_of[set] = t->monitor == TLB_MONITOR_AUDIO ? t->listen : -1;
    for (auto &G : t->groups) {
        int rc = hipStreamWaitEvent(t->s_run, G.ev_out, 0) == hipSuccess ? TLB_OK : TLB_ERR_HIP;
        if (!rc) rc = tlb_flush_device_len(G.b, G.d_frames, G.d_flen, t->s_run);
        if (!rc) {      // the egress sends the levels of the last run with the last frame (they are in the other host set; the device copy is current)
            rc = tick_egress(t, G, true, set, false);
        }
        if (rc) return tick_fail(t, rc);
    }
    if (hipStreamSynchronize(t->s_out) != hipSuccess) return tick_fail(t, TLB_ERR_HIP);
    t->out_set = set;
    t->finished = true;
    return TLB_OK;
}

const uint32_t *tlb_tick_silence_ms(const tlb_tick *t) { return t ? t->h_silence[t->out_set] : nullptr; }
// the per-unit outputs of a group are unit-major: slot (unit, local stream) of its packets / messages / fragment counts
static size_t tick_slot(const TickGroup &G, int unit, int k) { return (size_t)unit * (size_t)G.n + (size_t)k; }
const uint8_t *tlb_tick_message(const tlb_tick *t, int stream, int unit, int *len)
{   // ZeroMQ message = zmq_frame_header_t + unit; the header's datasize field says how much follows (0: absent)
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->egress != TLB_TICK_ZMQ || unit < 0 || unit >= G->max_upf) return nullptr;
    const uint8_t *m = G->h_msgs[t->out_set] + tick_slot(*G, unit, k) * (size_t)G->msg_stride;
    uint32_t ds; memcpy(&ds, m + 4, 4);
    if (len) *len = ds ? (int)(12 + ds) : 0;                         // (a set no tick has written yet is all zeros)
    return m;
}
int tlb_tick_units(const tlb_tick *t, int stream)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G) return 0;
    if (t->egress == TLB_TICK_FRAMES) return 1;
    return tlb_egress_units_per_frame(G->b, k);
}
const uint8_t *tlb_tick_frame(const tlb_tick *t, int stream, int *len)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->egress != TLB_TICK_FRAMES) return nullptr;
    if (len) *len = G->h_flen[t->out_set][k];
    return G->h_frames[t->out_set] + (size_t)k * (size_t)G->out_stride;
}
const uint8_t *tlb_tick_packet(const tlb_tick *t, int stream, int unit, int *len)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->egress != TLB_TICK_EDI_AF || unit < 0 || unit >= G->max_upf) return nullptr;
    const size_t slot = tick_slot(*G, unit, k);
    if (len) *len = G->h_plen[t->out_set][slot];
    return G->h_pkts[t->out_set] + slot * (size_t)G->af_stride;
}
int tlb_tick_fragments(const tlb_tick *t, int stream, int unit)
{
    int k; const TickGroup *G = tick_group_of(t, stream, &k);
    if (!G || t->egress != TLB_TICK_EDI_PFT || unit < 0 || unit >= G->max_upf) return 0;
    return G->h_nfrag[t->out_set][tick_slot(*G, unit, k)];
}
const uint8_t *tlb_tick_fragment(const tlb_tick *t, int stream, int unit, int k, int *len)
{
    if (k < 0 || k >= tlb_tick_fragments(t, stream, unit)) return nullptr;
    int ks; const TickGroup *G = tick_group_of(t, stream, &ks);
    const size_t frag = tick_slot(*G, unit, ks) * (size_t)G->max_frags + (size_t)k;
    if (len) *len = G->h_fraglen[t->out_set][frag];
    return G->h_frags[t->out_set] + frag * (size_t)G->frag_stride;
}
float tlb_tick_last_ms(tlb_tick *t)
{   // first copy-in queued -> last copy-out done, on the device's clock
    float ms = -1.0f;
    if (!t || !t->waited || hipSetDevice(t->device) != hipSuccess) return -1.0f;
    const int set = (int)((t->waited - 1) % 3);                      // the tick waited for last
    if (hipEventSynchronize(t->ev1[set]) != hipSuccess || hipEventElapsedTime(&ms, t->ev0[set], t->ev1[set]) != hipSuccess) return -1.0f;
    return ms;
}

}  // extern "C"
