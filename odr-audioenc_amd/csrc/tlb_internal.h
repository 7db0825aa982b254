// tlb_internal.h -- what the host translation units of the library share: the batch object, the error macros, and the few internal
// entry points that cross file boundaries (hidden from the dynamic symbol table by exports.map).  Host C++ only: no kernel code.
#pragma once
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <deque>
#include <memory>
#include <vector>

#include "../../include/toolame_batch.h"
#include "mp2_host.h"
#include "tl_kernels.h"
#include "tlb_inputs.h"
#include "tlb_mem.h"

static_assert(TL_MAX_XPAD == TLB_MAX_XPAD, "xpad record size");
#define TLB_HOST_CHUNKS 4            // tlb_encode_host pipelines a big call in this many chunks of frames

// the staging slots of tlb_batch::stage
enum TlbStage {
    TLB_STAGE_PCM, TLB_STAGE_OUT, TLB_STAGE_XPAD, TLB_STAGE_XPAD_LEN, TLB_STAGE_TAPS,      // tlb_encode_host: what the caller's buffers are copied to and from
    TLB_STAGE_PSY_OUT, TLB_STAGE_SCFCRC, TLB_STAGE_PADBITS,                                // tlb_launch: TlPsyOut records (models 2/4), ScF-CRC bytes, padding bits
    TLB_STAGE_OUT_LEN,                                                                     // tlb_encode_host_len: frame lengths
    TLB_STAGE_INGEST_IN, TLB_STAGE_INGEST_OUT, TLB_STAGE_INGEST_PEAKS,                     // tlb_ingest_host: interleaved in, planar out, peaks
    TLB_STAGE_COUNT
};
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { \
    fprintf(stderr, "libtoolame-dab-hip: %s failed: %s (%s:%d)\n", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
    return TLB_ERR_HIP; } } while (0)

// after a run of requests to a TlbMem (csrc/tlb_mem.h, which has printed the failing call): the one check
#define MEMCHK(m) do { if ((m).failed()) return TLB_ERR_HIP; } while (0)

static inline bool feed_same(const tlb_feed_config &a, const tlb_feed_config &b) { return a.samplerate == b.samplerate && a.bitrate == b.bitrate && a.channels == b.channels; }
// What a feed family (tlb_feed_*, tlb_feed_down_*) keeps of its records at batch level: the feed of every stream, the grow-only table of
// distinct records on host and device, and the report buffer of a launch that was given none.  Empty until the family's first set.
struct FeedTable {
    std::vector<tlb_feed_config> cfg;            // [nstreams] the stream's feed
    std::vector<int32_t> idx;                    // [nstreams] its record in h_configs, -1: none
    std::vector<tlb_feed_config> uniq;           // the three knobs of h_configs[i]; grow-only
    std::vector<TlConfig> h_configs;
    TlConfig *d_configs = nullptr;               // replaced when it grows: an owner of its own, as has d_rep
    std::unique_ptr<TlbMem> mem, rep_mem;
    size_t cap = 0, rep_slots = 0;
    tlb_frame_report *d_rep = nullptr;           // grow-only launch scratch

    void start(size_t nstreams) { cfg.assign(nstreams, tlb_feed_config{0, 0, 0}); idx.assign(nstreams, -1); }
    bool on(int s) const { return !idx.empty() && idx[(size_t)s] >= 0; }
    int find(const tlb_feed_config &c) const     // the record with these knobs, -1: none yet
    {
        int at = -1;
        for (size_t i = 0; i < uniq.size(); i++) if (feed_same(uniq[i], c)) at = (int)i;
        return at;
    }
    // the widest slot a frame of some stream's record needs; 0: no stream has a feed
    int stride() const
    {
        int w = 0;
        for (int i : idx) if (i >= 0 && tl_feed_slot_bytes(h_configs[(size_t)i]) > w) w = tl_feed_slot_bytes(h_configs[(size_t)i]);
        return w;
    }
    // room for `count` records in d_configs; what it holds is kept (the device is idle).  The new buffer is staged and filled in a new
    // owner, and only when it is complete do the owners change places (csrc/tlb_mem.h): a failure leaves everything as it was
    int reserve(size_t count)
    {
        if (count <= cap) return TLB_OK;
        std::unique_ptr<TlbMem> m(new TlbMem);
        TlConfig *nd = m->scratch<TlConfig>(count + 4);
        if (!h_configs.empty()) m->upload(nd, h_configs.data(), sizeof(TlConfig) * h_configs.size());
        if (!m->settle()) return TLB_ERR_HIP;
        mem.swap(m);
        d_configs = nd; cap = count + 4;
        return TLB_OK;
    }
    // the record of c (built as rec), added behind the others when *at is -1; room for it has been reserved
    int add(const tlb_feed_config &c, const TlConfig &rec, int *at)
    {
        if (*at >= 0) return TLB_OK;
        HIPCHK(hipMemcpy(d_configs + h_configs.size(), &rec, sizeof(TlConfig), hipMemcpyHostToDevice));
        *at = (int)h_configs.size();
        h_configs.push_back(rec); uniq.push_back(c);
        return TLB_OK;
    }
    // a launch without a report buffer: the kernels' history pass reads the last slot's status, so the family lends one of `slots` records
    int report(size_t slots, tlb_frame_report **d_report)
    {
        if (*d_report) return TLB_OK;
        if (rep_slots < slots) {
            HIPCHK(hipDeviceSynchronize());      // (a launch before may still write the one it replaces)
            std::unique_ptr<TlbMem> m(new TlbMem);
            tlb_frame_report *nr = m->scratch<tlb_frame_report>(slots);
            if (m->failed()) return TLB_ERR_HIP;
            rep_mem.swap(m);
            d_rep = nr; rep_slots = slots;
        }
        *d_report = d_rep;
        return TLB_OK;
    }
};

struct tlb_batch {
    int device = 0, nstreams = 0, out_stride = 0;
    long frames = 0;
    std::vector<TlConfig> h_configs;
    std::vector<tlb_stream_config> h_uniq;       // the six knobs of h_configs[i]
    size_t cfg_cap = 0;                          // records d_configs has room for
    std::vector<int32_t> h_stream_cfg;
    TlTables *d_tables = nullptr;
    TlConfig *d_configs = nullptr;
    int32_t *d_stream_cfg = nullptr;
    TlStreamState *d_state = nullptr;
    double *d_gain = nullptr;                    // linear gain per stream (ingest kernel)
    std::vector<double> h_gain;
    int32_t *d_list[4] = {nullptr, nullptr, nullptr, nullptr};   // stream ids per psy model
    int n_list[4] = {0, 0, 0, 0};
    TlPsy2Tables *d_psy2_tables = nullptr;     // 2 * TL_PSY2_SLOTS tables (psy 2 per sample rate, then psy 4 per sample rate; tl_psy2_slot), only when a stream uses psy 2 / 4
    TlPsy2State *d_psy2_state = nullptr;       // two copies per stream; a launch reads copy psy2_flip and writes the other (tl_psy2_chain)
    int psy2_flip = 0;
    int32_t *d_partner = nullptr;              // [nstreams] mono streams of one configuration and model share waves in pairs (tl_encode_pair); -1: alone
    int32_t *d_chain = nullptr;                // psy-2 kernel: (stream, channel) chains of the launch, first channels first
    int n_chain = 0;
    uint8_t *d_edi_version = nullptr;            // EDI: ODRv string and per-stream frame sizes (allocated on first use)
    char h_edi_version[TL_EDI_MAX_VERSION] = {}; // the string d_edi_version holds
    int edi_version_len = -1;
    int32_t *d_frame_bytes = nullptr, *d_unit_bytes = nullptr;
    int max_upf = 1;                             // egress units (3 * kbps bytes) per frame: 1 at 48 kHz, 2 at 24 kHz, 3 at 16 kHz; 0 = a stream's frames are no whole number of units
    TlEdiState *d_edi_state_tmp = nullptr;
    uint16_t *d_pseq_tmp = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_mid = nullptr;   // ev_mid: between the psy-2 kernel and the encode kernel (models 2/4)
    bool have_mid = false;
    hipStream_t last_stream = nullptr;
    bool timed = false;
    // device staging of the host-buffer entry point (tlb_encode_host): grow-only, created on first use, so a caller that
    // feeds one frame per call (the legacy shim) pays for no allocation after its first frame
    void *stage[TLB_STAGE_COUNT] = {};
    size_t stage_cap[TLB_STAGE_COUNT] = {};
    hipStream_t s_in = nullptr, s_run = nullptr, s_out = nullptr;   // host-buffer entry point: copy-in / kernels / copy-out
    hipEvent_t ev_in[TLB_HOST_CHUNKS] = {}, ev_run[TLB_HOST_CHUNKS] = {};
    uint32_t *d_newpend = nullptr;               // split path: the launch's last frame of every stream
    double *d_newlag = nullptr;                  // split path, 44.1 / 22.05 kHz: slot recurrence state after the launch
    bool pads[4] = {false, false, false, false}; // some stream of the psy model's list has frames of two lengths
    bool list_pairs[4] = {false, false, false, false};   // the model's list contains mono streams paired in one wave (kernel variant <.., true>)
    bool list_stereo[4] = {false, false, false, false};  // every stream of the model's list has two channels (kernel variant <.., false, 2>: models 1 and 3)
    int32_t *d_work = nullptr;                   // unit counters of the persistent kernels
    bool work_clean = false;                     // ... are zero (tl_finish_kernel zeroes them after use)
    bool broken = false;                         // a launch or a reconfiguration failed half way: stream state, psy-2 state copies and lists may disagree;
                                                 // every further launch is refused (TLB_ERR_HIP) until tlb_reset() has put all streams back to zero
    int num_cu = 256;
    // frame check / decode (tlb_decode.cpp): tables and per-stream state, allocated by the first decode call
    TlSynthTables *d_synth = nullptr;
    TlDecStream *d_dec_state = nullptr;          // [nstreams]
    uint8_t *d_dec_prev = nullptr;               // [nstreams][out_stride] the last slot of the call before
    unsigned long long *d_dec_bad = nullptr;     // frames with a TL_DEC_BAD_MASK flag since creation
    int16_t *d_cmp_hist = nullptr;               // compare monitor (tlb_compare.cpp): [nstreams][2][TL_CMP_HIST] the input the next decoded frame is set against, allocated by the first compare call
    // resampler (tlb_resample.cpp), allocated by the first tlb_resample_set_source: a batch that never sets a source has none of it
    uint32_t *d_rs_state = nullptr;              // [2][nstreams][TL_RS_STATE_WORDS]; a launch reads copy rs_flip and writes the other
    int32_t *d_rs_ratio = nullptr;               // [nstreams] TL_RS_*
    int16_t *d_rs_taps = nullptr;                // both tables: [160][32], then [3][32]
    int rs_flip = 0;
    std::vector<long> rs_rate;                   // [nstreams] source rate, 0: off (empty until the first set_source)
    std::vector<int32_t> rs_ratio, rs_pos;       // host copies: TL_RS_* and the frame position in the need cycle
    // decimator (tlb_decimate.cpp), allocated by the first tlb_decimate_set_source: a batch that never sets a down source has none of it
    uint32_t *d_dc_state = nullptr;              // [2][nstreams][TL_DC_STATE_WORDS]; a launch reads copy dc_flip and writes the other
    int32_t *d_dc_ratio = nullptr;               // [nstreams] TL_DC_*
    int16_t *d_dc_taps = nullptr;                // the three tables: [80][64], [3][64], [1][64]
    int dc_flip = 0;
    std::vector<long> dc_rate;                   // [nstreams] source rate, 0: off (empty until the first set_source)
    std::vector<int32_t> dc_ratio, dc_pos;       // host copies: TL_DC_* and the frame position in the need cycle
    // Layer II feeds (tlb_feed.cpp), allocated by the first tlb_feed_set: a batch that never sets a feed has none of it
    FeedTable feed;                              // the streams' feeds and their records
    std::unique_ptr<TlbMem> feed_prev_mem;       // d_feed_prev is replaced when it grows: an owner of its own
    int32_t *d_feed_cfg = nullptr;               // [nstreams] feed.idx on the device
    TlDecStream *d_feed_state = nullptr;         // [nstreams] the feed history, separate from the decoder's
    uint8_t *d_feed_prev = nullptr;              // [nstreams][feed_prev_stride] the last slot of the call before; replaced when a longer feed frame arrives
    int feed_prev_stride = 0;
    // adapted feeds (tlb_feed_set_adapted; csrc/mp2_feed_adapt.h), allocated by the first one that does not match its stream.  An adapted
    // stream keeps its record in `feed` and its history in d_feed_state / d_feed_prev, but reads -1 in d_feed_cfg: the strict
    // kernel sees it as a stream without a feed
    std::vector<int32_t> fa_ratio;               // [nstreams] -1: not adapted, else TL_RS_* of (feed rate, stream rate) (empty until the first adapted feed)
    std::vector<int32_t> fa_pos;                 // [nstreams] host copy of the tick counter modulo the cycle
    int n_adapted = 0;
    int32_t *d_fa_cfg = nullptr, *d_fa_ratio = nullptr;      // [nstreams] feed record (-1: not adapted), TL_RS_*
    int16_t *d_fa_carry = nullptr;               // [2][nstreams][TL_FA_CARRY * 2]; a call reads copy fa_flip and writes the other
    int32_t *d_fa_pos = nullptr;                 // [2][nstreams]
    int16_t *d_fa_taps = nullptr;                // both tables, a copy of the feeds' own (the resampler's state is a separate object)
    int16_t *d_fa_plane = nullptr;               // [nstreams][fa_plane_frames * 2304] grow-only launch scratch with an owner of its own
    std::unique_ptr<TlbMem> fa_plane_mem;
    int fa_plane_frames = 0, fa_flip = 0;
    // down feeds (tlb_feed_down.cpp; csrc/mp2_feed_down.h), allocated by the first tlb_feed_down_set: a batch that never sets one has none of
    // it.  Records, history and reports of their own: nothing is shared with the feeds above but the synthesis tables
    FeedTable fd;                                // the streams' down feeds and their records
    std::vector<int32_t> fd_ratio, fd_pos;       // [nstreams] TL_DC_* of (feed rate, stream rate); host copy of the tick counter modulo the cycle
    std::unique_ptr<TlbMem> fd_plane_mem;
    int n_down = 0, fd_plane_frames = 0, fd_flip = 0;
    int32_t *d_fd_cfg = nullptr, *d_fd_ratio = nullptr;      // [nstreams] fd.idx, fd_ratio on the device
    int32_t *d_fd_pos = nullptr;                 // [2][nstreams]; a call reads copy fd_flip and writes the other
    int16_t *d_fd_carry = nullptr;               // [2][nstreams][TL_FD_CARRY * 2], likewise
    TlDecStream *d_fd_state = nullptr;           // [nstreams] length and status of the last wanted slot of the call before
    uint8_t *d_fd_prev = nullptr;                // [nstreams][TL_FD_PREV_STRIDE] its bytes
    int16_t *d_fd_taps = nullptr;                // the decimator's three tables, a copy of the down feeds' own
    int16_t *d_fd_plane = nullptr;               // [nstreams][fd_plane_frames * TL_FD_PLANE] grow-only launch scratch with an owner of its own
    // loudness meter (tlb_loudness.cpp; csrc/mp2_loudness.h), allocated by tlb_loudness_enable alone: a batch that never enables it has none of it
    double *d_ld_lane = nullptr, *d_ld_ring = nullptr;       // [TL_LD_LANE_WORDS][2 nstreams] filter state, acc and bin position per (stream, channel); [TL_LD_RING][nstreams]
    TlLoudnessRecord *d_ld_rec = nullptr;        // [nstreams] the record as it is reported
    uint32_t *d_ld_hist = nullptr;               // [TL_LD_HIST_ROWS][nstreams] gating blocks per 0.1 LU
    TlLoudnessProgramme *d_ld_prog = nullptr;    // [nstreams] scratch of tlb_loudness_programme_host
    double *d_ld_tables = nullptr;               // the committed table: taps [6][10], edges [751], centres [751]
    // ... its loudness range (tlb_lra_*), allocated by tlb_lra_enable alone: a batch that never enables it has none of it and launches tl_loudness_kernel
    uint32_t *d_ld_hist_st = nullptr;            // [TL_LD_HIST_ROWS][nstreams] range blocks (short-term values) per 0.1 LU
    TlLraRecord *d_ld_lra = nullptr;             // [nstreams] scratch of tlb_lra_host
    // true-peak meter (tlb_truepeak.cpp; csrc/mp2_truepeak.h), allocated by tlb_truepeak_enable alone: a batch that never enables it has none of it
    TlTruePeakRecord *d_tp_rec = nullptr;        // [nstreams] the record as it is reported
    uint32_t *d_tp_hist = nullptr;               // [nstreams][2][TL_TP_CARRY / 2] the carried samples of either channel
    int16_t *d_tp_taps = nullptr;                // the committed table [3][TL_TP_TAPS]
    uint32_t tp_ceiling = 0;                     // in units of 2^-30 of full scale
    // true-peak limiter (tlb_limiter.cpp; csrc/mp2_limiter.h), allocated by tlb_limiter_enable alone: a batch that never enables it has none of it
    TlLimiterRecord *d_lm_rec = nullptr;         // [nstreams] the record as it is reported
    uint32_t *d_lm_state = nullptr;              // [nstreams][TL_LM_STATE] the delay line and the carried r and e
    uint32_t *d_lm_step = nullptr;               // [nstreams] S from the stream's encoder rate
    int16_t *d_lm_taps = nullptr;                // the true-peak meter's committed table, a copy of the limiter's own
    tlb_limiter_params lm_params = {0, 0};       // as enabled, the defaults filled in
    // feed concealment (tlb_conceal.cpp; csrc/mp2_conceal.h, csrc/mp2_conceal_conv.h), allocated by the first tlb_conceal_enable or
    // tlb_feed_loss_enable that switches it on: a batch that never enables it has none of it
    std::vector<TlConcealStream> cc_host;        // [nstreams] the parameters as set (g_len is not kept here); empty until allocated
    int n_conceal = 0;                           // streams with a strict feed and hold > 0: the feed launch queues the two kernels while this is not 0
    int n_conceal_adapt = 0, n_conceal_down = 0; // ... with an adapted / a down feed: that path's launch queues the two kernels of toolame_conceal_conv.hip
    TlConcealStream *d_cc_state = nullptr;       // [nstreams]
    TlConcealRecord *d_cc_rec = nullptr;         // [nstreams] the record as it is reported
    uint8_t *d_cc_g = nullptr;                   // [nstreams][cc_g_stride] the last passing slot; replaced when a longer feed frame arrives
    int cc_g_stride = 0;
    std::unique_ptr<TlbMem> cc_g_mem;            // ... hence an owner of its own
    TlbMem mem;                                 // owns every device buffer above that is made once and kept until tlb_destroy (csrc/tlb_mem.h); d_configs and
                                                 // stage[] are replaced during the object's life and are freed one by one
    int fail_in = 0;                             // test builds only (-DTLB_FAULT_INJECT, csrc/tlb_debug.h): the fail_in-th launch from now fails
};

static inline hipError_t stage_reserve(tlb_batch *b, TlbStage k, size_t bytes)
{
    if (b->stage_cap[k] >= bytes) return hipSuccess;
    if (b->stage[k]) { (void)hipFree(b->stage[k]); b->stage[k] = nullptr; b->stage_cap[k] = 0; }
    hipError_t e = hipMalloc(&b->stage[k], bytes);
    if (e == hipSuccess) b->stage_cap[k] = bytes;
    return e;
}

// tlb_batch.cpp: one launch of the encode path on `st` (every entry point ends here)
int tlb_launch(tlb_batch *b, const int16_t *d_pcm, int nframes, const uint8_t *d_xpad, const int32_t *d_xpad_len,
               uint8_t *d_out, TlTaps *d_taps, hipStream_t st, long long *d_stamps = nullptr, int32_t *d_out_len = nullptr);
// tlb_egress.cpp: the egress stages with the per-slot frame lengths a tick object has (0 = the slot holds no frame)
int zmq_frame_device(tlb_batch *b, const uint8_t *d_frames, const int16_t *d_peaks, int nframes, uint8_t *d_msgs, void *hip_stream, const int32_t *d_frame_len);
int edi_af_device(tlb_batch *b, const uint8_t *d_frames, const int16_t *d_levels, int nframes, tlb_edi_state *d_state,
                  const char *version, int version_len, uint8_t *d_pkts, int32_t *d_pkt_len, void *hip_stream, const int32_t *d_frame_len);
// tlb_decode.cpp: the decoder's tables and per-stream state, as the first decode call makes them (it waits for the device once); the
// synthesis tables alone, which the feeds share
int decode_prepare(tlb_batch *b);
int synth_prepare(tlb_batch *b);
// tlb_feed.cpp: the feed history of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle); after a reconfiguration,
// the stream's feed removed when its rate or channel count no longer is the stream's
int feed_clear_streams(tlb_batch *b, int s0, int n);
int feed_after_reconfigure(tlb_batch *b, int stream);
// ... what the tick plane needs of it: is cfg legal and does it fit streams [s0, s1) (nothing changes); the slot a frame of cfg needs;
// tlb_feed_device with slots of `stride` bytes, at least tlb_feed_stride(b) (a tick object has ONE stride for all its groups)
int feed_fits(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg);
int feed_fits_adapted(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg);      // ... for tlb_feed_set_adapted: a legal rate pair, any channel counts
int feed_slot_bytes(const tlb_feed_config *cfg);
int feed_build(TlConfig *c, const tlb_feed_config *cfg);           // the kernel-side record of a feed configuration, or why it is not legal
int feed_launch(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report, void *hip_stream, int stride);
// tlb_compare.cpp: the history as the first compare call makes it; the launch itself with a report that may be NULL (every slot skipped:
// a tick that has no frames yet still advances the history)
int compare_prepare(tlb_batch *b);
int compare_launch(tlb_batch *b, const int16_t *d_in_pcm, const int16_t *d_dec_pcm, const tlb_frame_report *d_report, int nframes,
                   const tlb_compare_params *params, tlb_compare_record *d_record, void *hip_stream);
// tlb_resample.cpp: the resampler's tables and state as the first real source makes them (waits for the device once); the resampler state of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle); the legality of a
// stream's source with a new encoder rate (tlb_stream_reconfigure)
int resample_prepare(tlb_batch *b);
int16_t *resample_taps_upload(TlbMem &m);        // both tables in one buffer of m: [160][32], then [3][32] (the resampler's copy, and the adapted feeds')
int resample_clear_streams(tlb_batch *b, int s0, int n);
bool resample_rate_fits(const tlb_batch *b, int stream, long encoder_rate);
// tlb_decimate.cpp: the same three for the decimator's down sources
int decimate_prepare(tlb_batch *b);
int decimate_clear_streams(tlb_batch *b, int s0, int n);
bool decimate_rate_fits(const tlb_batch *b, int stream, long encoder_rate);
int16_t *decimate_taps_upload(TlbMem &m);        // the three tables in one buffer of m: [80][64], [3][64], [1][64] (the decimator's copy, and the down feeds')
// tlb_feed_down.cpp: the position, queue and history of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle); after
// a reconfiguration, the stream's down feed removed when its rate no longer pairs with the stream's
int feed_down_clear_streams(tlb_batch *b, int s0, int n);
int feed_down_after_reconfigure(tlb_batch *b, int stream);
// ... what the tick plane needs of it: is cfg legal and does it pair with streams [s0, s1) (nothing changes); tlb_feed_down_device with
// slots of `stride` bytes, at least tlb_feed_down_stride(b)
int feed_down_fits(const tlb_batch *b, int s0, int s1, const tlb_feed_config *cfg);
int feed_down_launch(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report, void *hip_stream, int stride);
// tlb_conceal.cpp: nothing when concealment was never enabled.  G, run and record of streams [s0, s0 + n) forgotten (off: and their
// concealment switched off; the life-cycle calls, the device is idle); room for slots of `stride` bytes in the G buffer, what it holds
// kept; the two kernels behind the feed launch A on `hip_stream`
int conceal_clear_streams(tlb_batch *b, int s0, int n, bool off = false);
int conceal_g_reserve(tlb_batch *b, int stride);
int conceal_launch(tlb_batch *b, const TlFeedLaunch &A, void *hip_stream);
// ... the same clearing for one feed family's life-cycle calls: down = false leaves the streams with a down feed alone (tlb_feed_*),
// down = true those with a strict or an adapted feed (tlb_feed_down_*); the concealment's arrays for the adapted (down = false) or the
// down path's launch into *x, NULL: no such stream has concealment on and the path queues what it always queued
int conceal_clear_family(tlb_batch *b, int s0, int n, bool down, bool off = false);
const TlConcealConv *conceal_conv(const tlb_batch *b, bool down, TlConcealConv *x);

// The PCM meters (tlb_loudness.cpp, tlb_truepeak.cpp).  A meter's state of streams [s0, s0 + n) back to zero (the device is idle); nothing
// when the meter was never enabled
int loudness_clear_streams(tlb_batch *b, int s0, int n);
int truepeak_clear_streams(tlb_batch *b, int s0, int n);
int limiter_clear_streams(tlb_batch *b, int s0, int n);             // (tlb_limiter.cpp: the limiter's, and its steps from the streams' rates as they are now)
// ... the one body of tlb_*_host: `state`, what the meter's enable made (NULL: never enabled); scratch PCM and records, one launch of the
// meter's *_device, the records back
template <class Rec> int meter_host(tlb_batch *b, const void *state, const int16_t *pcm_planar, int nframes, Rec *records,
                                    int (*device)(tlb_batch *, const int16_t *, int, Rec *, void *))
{
    if (!b || !pcm_planar || !records || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30) || !state) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t vals = (size_t)nframes * (size_t)b->nstreams * 2 * TLB_SAMPLES_PER_FRAME;
    TlbMem m;
    int16_t *d_pcm = m.scratch<int16_t>(vals);
    Rec *d_rec = m.scratch<Rec>((size_t)b->nstreams);
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_pcm, pcm_planar, vals * sizeof(int16_t), hipMemcpyHostToDevice));
    if (int rc = device(b, d_pcm, nframes, d_rec, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(records, d_rec, (size_t)b->nstreams * sizeof(Rec), hipMemcpyDeviceToHost));
    return TLB_OK;
}
// ... and of tlb_*_reset: one stream's state, or every stream's (-1), through the meter's clear
static inline int meter_reset(tlb_batch *b, const void *state, int stream, int (*clear)(tlb_batch *, int, int))
{
    if (!b || stream < -1 || stream >= b->nstreams || !state) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    return stream < 0 ? clear(b, 0, b->nstreams) : clear(b, stream, 1);
}

// the encoder's rate of stream s
static inline long batch_enc_rate(const tlb_batch *b, int s) { return b->h_uniq[(size_t)b->h_stream_cfg[(size_t)s]].samplerate; }
// the input families stream s has (csrc/tlb_inputs.h): what a batch-level setter asks tlb_input_may_set about
static inline unsigned batch_inputs(const tlb_batch *b, int s)
{
    return (tlb_resample_source(b, s) ? TLB_IN_BIT(TLB_IN_UP_SOURCE) : 0u) | (tlb_decimate_source(b, s) ? TLB_IN_BIT(TLB_IN_DOWN_SOURCE) : 0u) |
           (tlb_feed_get(b, s, nullptr) > 0 ? TLB_IN_BIT(TLB_IN_FEED) : 0u) | (b->fd.on(s) ? TLB_IN_BIT(TLB_IN_DOWN_FEED) : 0u);
}
static inline bool batch_may_set(const tlb_batch *b, int s, TlbInput f) { return tlb_input_may_set(TLB_INPUTS_STREAM, f, batch_inputs(b, s)); }
int pft_shape(int max_af_len, int fec, int chunk_len, int transport, int *max_frags, int *frag_stride);
