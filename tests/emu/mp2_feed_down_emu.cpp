// mp2_feed_down_emu.cpp -- TEST-ONLY host emulation of the down-feed kernels (csrc/mp2_feed_down.h over csrc/mp2_feed.h, csrc/mp2_unpack.h,
// csrc/mp2_synth.h and csrc/mp2_decimate.h, compiled with -DTL_EMULATE: every lane region is a loop over 64 lanes).  tests/feeddownlib.py
// compiles it into a temporary directory together with csrc/mp2_host.cpp; the product library never contains or loads it.
// The entry points mirror tlb_feed_down_set / tlb_feed_down_reset / tlb_feed_down_device (csrc/tlb_feed_down.cpp): decode, decimate and
// carry, every unit of a kernel in DESCENDING order (nothing is carried from unit to unit inside a call).  The plane, the LDS block and the
// tables are on the heap and exactly as long as the device's: an index past one of them is an access past the allocation.
#define TL_EMULATE 1
#define TL_FD_BODY 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_unpack.h"
#include "../../odr-audioenc_amd/csrc/mp2_synth.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed.h"
#include "../../odr-audioenc_amd/csrc/mp2_decimate.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed_down.h"
#include "../../odr-audioenc_amd/csrc/tl_decimate_taps.inc"

struct Down {
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs, sconfigs;     // the feeds' records; one record per stream of which only nch is read
    std::vector<int32_t> feed_cfg, ratio, stream_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev;
    std::vector<int16_t> carry;                  // [2][nstreams][TL_FD_CARRY * 2]
    std::vector<int32_t> pos;                    // [2][nstreams]
    int16_t *taps = nullptr;
    int stride = 0, flip = 0;
};

static int16_t *load_taps()
{
    int16_t *t = (int16_t *)aligned_alloc(16, sizeof(int16_t) * TL_DC_TABLE_ROWS * TL_DC_TAPS);
    memcpy(t + tl_dc_first_row(TL_DC_80_147) * TL_DC_TAPS, tl_decimate_taps_80_147, sizeof tl_decimate_taps_80_147);
    memcpy(t + tl_dc_first_row(TL_DC_3_4) * TL_DC_TAPS, tl_decimate_taps_3_4, sizeof tl_decimate_taps_3_4);
    memcpy(t + tl_dc_first_row(TL_DC_1_2) * TL_DC_TAPS, tl_decimate_taps_1_2, sizeof tl_decimate_taps_1_2);
    return t;
}

// the decimate workgroup of tick f of stream s: the four waves' fill, the barrier, their outputs, the barrier, the copy to both channels
static void decimate_slot(const TlFeedDownLaunch &A, int s, int f)
{
    const TlFdSlot S = tl_fd_slot_of(A, s, f);
    if (S.ratio == TL_DC_OFF) return;
    TlDecimateLds *r = (TlDecimateLds *)aligned_alloc(16, sizeof(TlDecimateLds));
    int16_t *y = (int16_t *)aligned_alloc(16, sizeof(int16_t) * TL_DC_FRAME);
    memset(r, 0x55, sizeof *r); memset(y, 0x55, sizeof(int16_t) * TL_DC_FRAME);      // whatever the workgroup before left in LDS
    for (int wave = 0; wave < TL_DC_WAVES; wave++) tl_fd_fill(A, *r, S, s, wave);
    for (int wave = TL_DC_WAVES - 1; wave >= 0; wave--) tl_fd_wave(A, *r, S, y, s, f, wave);
    if (S.fch == 1 && S.sch == 2) for (int wave = 0; wave < TL_DC_WAVES; wave++) tl_fd_dup(A, y, s, f, wave);
    free(r); free(y);
}

extern "C" {
// channels[s] = 0: stream s has no down feed; enc_rate / enc_nch: the stream's own
void *fd_create(int nstreams, const long *fs, const int *kbps, const int *channels, const long *enc_rate, const int *enc_nch, int *err)
{
    Down *d = new Down;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    d->taps = load_taps();
    for (int s = 0; s < nstreams; s++) {
        TlConfig sc;
        memset(&sc, 0, sizeof sc);
        sc.nch = enc_nch[s];
        d->sconfigs.push_back(sc); d->stream_cfg.push_back(s);
        d->feed_cfg.push_back(-1); d->ratio.push_back(TL_DC_OFF);
        if (!channels[s]) continue;
        TlConfig c;
        int rc = tl_build_config(&c, fs[s], channels[s] == 1 ? 'm' : 's', kbps[s], 1, 0);
        if (!rc && tl_fd_ratio_of(fs[s], enc_rate[s]) == TL_DC_OFF) rc = 1;
        if (rc) { if (err) *err = rc; free(d->taps); delete d; return nullptr; }
        d->feed_cfg[(size_t)s] = (int32_t)d->configs.size(); d->ratio[(size_t)s] = tl_fd_ratio_of(fs[s], enc_rate[s]);
        d->configs.push_back(c);
        if (tl_feed_slot_bytes(c) > d->stride) d->stride = tl_feed_slot_bytes(c);
    }
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * TL_FD_PREV_STRIDE, 0);
    d->carry.assign((size_t)2 * nstreams * TL_FD_CARRY * 2, 0);
    d->pos.assign((size_t)2 * nstreams, 0);
    if (err) *err = 0;
    return d;
}
void fd_destroy(void *h) { free(((Down *)h)->taps); delete (Down *)h; }
int fd_stride(void *h) { return ((Down *)h)->stride; }
int fd_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int fd_carry_frames(void) { return TL_FD_CARRY; }
int fd_want_at(long fs, long es, int tick) { const int r = tl_fd_ratio_of(fs, es); return r == TL_DC_OFF ? -1 : tl_fd_want(tick % tl_fd_cycle(r), r); }
int fd_pos(void *h, int s) { Down *d = (Down *)h; return d->pos[(size_t)d->flip * d->state.size() + (size_t)s]; }
int fd_reset(void *h, int s)
{
    Down *d = (Down *)h;
    const int ns = (int)d->state.size();
    if (s < -1 || s >= ns) return 18;
    for (int i = 0; i < ns; i++) {
        if (s >= 0 && i != s) continue;
        memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
        for (int k = 0; k < 2; k++) {
            memset(&d->carry[((size_t)k * ns + i) * TL_FD_CARRY * 2], 0, sizeof(int16_t) * TL_FD_CARRY * 2);
            d->pos[(size_t)k * ns + i] = 0;
        }
    }
    return 0;
}
// frames [nframes][nstreams][2][stride], len [nframes][nstreams][2], pcm [nframes][nstreams][2304] read-modify-write, report [nframes][nstreams][2]
int fd_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, TlFrameReport *report)
{
    Down *d = (Down *)h;
    if (!frames || !len || !pcm || !report || nframes <= 0 || nframes > TL_FD_MAX_FRAMES) return 18;
    const int ns = (int)d->state.size();
    // exactly as long as a call of this many ticks needs: a read or write past it is one past the allocation
    std::vector<int16_t> plane((size_t)ns * (size_t)nframes * TL_FD_PLANE, (int16_t)0x5555);
    TlFeedDownLaunch D;
    memset(&D, 0, sizeof D);
    D.F.tables = &d->tables; D.F.configs = d->configs.data(); D.F.feed_cfg = d->feed_cfg.data(); D.F.synth = &d->synth;
    D.F.frames = frames; D.F.len = len; D.F.report = report; D.F.pcm = pcm;
    D.F.state = d->state.data(); D.F.prev = d->prev.data();
    D.F.nstreams = ns; D.F.nframes = nframes; D.F.stride = d->stride; D.F.prev_stride = TL_FD_PREV_STRIDE;
    D.ratio = d->ratio.data(); D.sconfigs = d->sconfigs.data(); D.stream_cfg = d->stream_cfg.data(); D.taps = d->taps;
    D.plane = plane.data(); D.carry = d->carry.data(); D.pos = d->pos.data(); D.flip = d->flip;
    static thread_local TlSynthLds w;
    for (int s = ns - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--)
            for (int j = 1; j >= 0; j--) tl_fd_decode_unit(w, D, s, f, j, d->synth.d);
    for (int f = nframes - 1; f >= 0; f--)
        for (int s = ns - 1; s >= 0; s--) decimate_slot(D, s, f);
    for (int s = 0; s < ns; s++) tl_fd_carry(D, s);
    d->flip ^= 1;
    return 0;
}
// The decimate and carry stages alone: ONE stream from its reset, its ticks cut into `ncuts` calls of cuts[k] ticks, over source frames
// the caller decoded.  x int16 [>= K(ticks - 1) * 1152][fch] (the feed's channel layout), out int16 [ticks][2304] read-modify-write.
int fd_decimate_plane(long feed_rate, long enc_rate, int fch, int sch, const int16_t *x, int ncuts, const int *cuts, int16_t *out)
{
    const int ratio = tl_fd_ratio_of(feed_rate, enc_rate);
    if (ratio == TL_DC_OFF || !x || !out || !cuts || ncuts <= 0 || (fch != 1 && fch != 2) || (sch != 1 && sch != 2)) return 18;
    TlConfig fc, sc;
    memset(&fc, 0, sizeof fc); memset(&sc, 0, sizeof sc);
    fc.nch = fch; sc.nch = sch;
    const int32_t zero = 0, ra = ratio;
    std::vector<int16_t> carry((size_t)2 * TL_FD_CARRY * 2, 0);
    int16_t *taps = load_taps();
    int32_t pos[2] = {0, 0};
    TlDecStream st[1];
    uint8_t prev[4] = {0, 0, 0, 0};
    long long tick = 0, rows_done = 0;                               // since the reset, in 64 bits: the position is the kernels' business
    int flip = 0;
    for (int k = 0; k < ncuts; k++) {
        const int n = cuts[k];
        if (n <= 0 || n > TL_FD_MAX_FRAMES) { free(taps); return 18; }
        const long long L = tl_dc_L(ratio), M = tl_dc_M(ratio);
        const long long rows_to = ((1152 * (tick + n) * M + L - 1) / L + 1151) / 1152;      // K(tick + n - 1)
        const size_t rows = (size_t)(rows_to - rows_done);
        std::vector<int16_t> plane((size_t)n * TL_FD_PLANE, (int16_t)0x5555);
        memcpy(plane.data(), x + (size_t)rows_done * 1152 * (size_t)fch, sizeof(int16_t) * rows * 1152 * (size_t)fch);
        std::vector<uint8_t> frames((size_t)n * 2 * 4, 0);
        std::vector<int32_t> len((size_t)n * 2, 0);
        std::vector<TlFrameReport> report((size_t)n * 2);
        memset(report.data(), 0, sizeof(TlFrameReport) * report.size());
        memset(st, 0, sizeof st);
        TlFeedDownLaunch D;
        memset(&D, 0, sizeof D);
        D.F.configs = &fc; D.F.feed_cfg = &zero; D.F.pcm = out + (size_t)tick * 2304; D.F.nstreams = 1; D.F.nframes = n;
        D.F.frames = frames.data(); D.F.len = len.data(); D.F.report = report.data(); D.F.state = st; D.F.prev = prev; D.F.stride = 4; D.F.prev_stride = 4;
        D.ratio = &ra; D.sconfigs = &sc; D.stream_cfg = &zero; D.taps = taps;
        D.plane = plane.data(); D.carry = carry.data(); D.pos = pos; D.flip = flip;
        for (int f = n - 1; f >= 0; f--) decimate_slot(D, 0, f);
        tl_fd_carry(D, 0);
        flip ^= 1; tick += n; rows_done = rows_to;
    }
    free(taps);
    return 0;
}
}
