// mp2_feed_emu.cpp -- TEST-ONLY host emulation of the Layer II feed kernels, strict and adapted (csrc/mp2_feed.h and csrc/mp2_feed_adapt.h
// over csrc/mp2_unpack.h, csrc/mp2_synth.h and csrc/mp2_resample.h, compiled with -DTL_EMULATE: every lane region is a loop over 64 lanes).
// tests/feedlib.py compiles it into a temporary directory together with csrc/mp2_host.cpp; the product library never contains or loads it.
// The entry points mirror tlb_feed_set / tlb_feed_set_adapted / tlb_feed_reset / tlb_feed_device (csrc/tlb_feed.cpp): the strict launch
// where a stream has a strict feed, then decode, resample and carry for the adapted streams, every unit of a kernel in DESCENDING order
// (nothing is carried from unit to unit inside a call).  A stream set without an adapted stream runs the strict launch alone.
#define TL_EMULATE 1
#define TL_FA_BODY 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_unpack.h"
#include "../../odr-audioenc_amd/csrc/mp2_synth.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed_adapt.h"
#include "../../odr-audioenc_amd/csrc/tl_resample_taps.inc"

struct Feed {
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs, sconfigs;     // the feeds' records; one record per stream of which only nch is read
    std::vector<int32_t> feed_cfg, fa_cfg, ratio, stream_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev;
    std::vector<int16_t> carry;                  // [2][nstreams][TL_FA_CARRY * 2]
    std::vector<int32_t> pos;                    // [2][nstreams]
    std::vector<int16_t> taps;
    int stride = 0, flip = 0, n_strict = 0, n_adapted = 0;
};

static void load_taps(std::vector<int16_t> &t)
{
    t.resize((160 + 3) * TL_RS_TAPS);
    memcpy(t.data(), tl_resample_taps_160_147, sizeof tl_resample_taps_160_147);
    memcpy(t.data() + 160 * TL_RS_TAPS, tl_resample_taps_3_2, sizeof tl_resample_taps_3_2);
}

// the resample workgroup of slot (f, s): the four waves' fill, the barrier, their outputs, the barrier, the copy to both channels
static void resample_slot(const TlFeedAdaptLaunch &A, int s, int f)
{
    static TlResampleLds r;
    static int16_t y[TL_RS_FRAME];
    memset(&r, 0x55, sizeof r); memset(y, 0x55, sizeof y);           // whatever the workgroup before left in LDS
    const TlFaSlot S = tl_fa_slot(A, s, f);
    if (S.ratio < 0) return;
    if (S.ratio == TL_RS_OFF) { for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_copy(A, S, s, f, wave); return; }
    for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_fill(A, r, S, s, wave);
    for (int wave = TL_RS_WAVES - 1; wave >= 0; wave--) tl_fa_wave(A, r, S, y, s, f, wave);
    if (S.fch == 1 && S.sch == 2) for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_dup(A, y, s, f, wave);
}

extern "C" {
// channels[s] = 0: stream s has no feed; adapted[s]: set through tlb_feed_set_adapted (a configuration that matches the stream is a strict
// feed all the same); enc_rate / enc_nch: the stream's own
void *feed_create(int nstreams, const long *fs, const int *kbps, const int *channels, const int *adapted, const long *enc_rate, const int *enc_nch, int *err)
{
    Feed *d = new Feed;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    load_taps(d->taps);
    for (int s = 0; s < nstreams; s++) {
        TlConfig sc;
        memset(&sc, 0, sizeof sc);
        sc.nch = enc_nch[s];
        d->sconfigs.push_back(sc); d->stream_cfg.push_back(s);
        d->feed_cfg.push_back(-1); d->fa_cfg.push_back(-1); d->ratio.push_back(0);
        if (!channels[s]) continue;
        TlConfig c;
        int rc = tl_build_config(&c, fs[s], channels[s] == 1 ? 'm' : 's', kbps[s], 1, 0);
        const bool match = fs[s] == enc_rate[s] && channels[s] == enc_nch[s];
        if (!rc && !match && (!adapted[s] || tl_fa_ratio_of(fs[s], enc_rate[s]) < 0)) rc = 1;
        if (rc) { if (err) *err = rc; delete d; return nullptr; }
        if (match) { d->feed_cfg[(size_t)s] = (int32_t)d->configs.size(); d->n_strict++; }
        else { d->fa_cfg[(size_t)s] = (int32_t)d->configs.size(); d->ratio[(size_t)s] = tl_fa_ratio_of(fs[s], enc_rate[s]); d->n_adapted++; }
        d->configs.push_back(c);
        if (tl_feed_slot_bytes(c) > d->stride) d->stride = tl_feed_slot_bytes(c);
    }
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * (size_t)d->stride, 0);
    d->carry.assign((size_t)2 * nstreams * TL_FA_CARRY * 2, 0);
    d->pos.assign((size_t)2 * nstreams, 0);
    if (err) *err = 0;
    return d;
}
void feed_destroy(void *h) { delete (Feed *)h; }
int feed_stride(void *h) { return ((Feed *)h)->stride; }
int feed_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int feed_reset(void *h, int s)
{
    Feed *d = (Feed *)h;
    const int ns = (int)d->state.size();
    if (s < -1 || s >= ns) return 18;
    for (int i = 0; i < ns; i++) {
        if (s >= 0 && i != s) continue;
        memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
        for (int k = 0; k < 2; k++) {
            memset(&d->carry[((size_t)k * ns + i) * TL_FA_CARRY * 2], 0, sizeof(int16_t) * TL_FA_CARRY * 2);
            d->pos[(size_t)k * ns + i] = 0;
        }
    }
    return 0;
}
// frames [nframes][nstreams][stride], len [nframes][nstreams], pcm [nframes][nstreams][2304] read-modify-write, report [nframes][nstreams]
int feed_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, TlFrameReport *report)
{
    Feed *d = (Feed *)h;
    if (!frames || !len || !pcm || !report || nframes <= 0 || (d->n_adapted && nframes > TL_FA_MAX_FRAMES)) return 18;
    TlFeedLaunch A;
    memset(&A, 0, sizeof A);
    A.tables = &d->tables; A.configs = d->configs.data(); A.feed_cfg = d->feed_cfg.data(); A.synth = &d->synth;
    A.frames = frames; A.len = len; A.report = report; A.pcm = pcm;
    A.state = d->state.data(); A.prev = d->prev.data();
    A.nstreams = (int)d->state.size(); A.nframes = nframes; A.stride = d->stride; A.prev_stride = d->stride;
    static thread_local TlSynthLds w;
    if (d->n_strict || !d->n_adapted) {
        for (int s = A.nstreams - 1; s >= 0; s--)
            for (int f = nframes - 1; f >= 0; f--) tl_feed_unit(w, A, s, f, d->synth.d);
        for (int s = 0; s < A.nstreams; s++) tl_feed_carry(A, s);
    }
    if (!d->n_adapted) return 0;
    // exactly as long as a call of this many ticks needs: a read or write past it is one past the allocation
    std::vector<int16_t> plane((size_t)A.nstreams * (size_t)nframes * 2304, (int16_t)0x5555);
    TlFeedAdaptLaunch D;
    memset(&D, 0, sizeof D);
    D.F = A; D.F.feed_cfg = d->fa_cfg.data();
    D.ratio = d->ratio.data(); D.sconfigs = d->sconfigs.data(); D.stream_cfg = d->stream_cfg.data(); D.taps = d->taps.data();
    D.plane = plane.data(); D.carry = d->carry.data(); D.pos = d->pos.data(); D.flip = d->flip; D.strict_ran = d->n_strict > 0;
    for (int s = A.nstreams - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--) tl_fa_decode_unit(w, D, s, f, d->synth.d);
    for (int f = nframes - 1; f >= 0; f--)
        for (int s = A.nstreams - 1; s >= 0; s--) resample_slot(D, s, f);
    for (int s = 0; s < A.nstreams; s++) tl_fa_carry(D, s);
    d->flip ^= 1;
    return 0;
}
// The resample stage alone: ONE stream from its reset, `nticks` ticks in one call over a source plane the caller decoded.
// x int16 [K(nticks - 1) * 1152][fch] (the feed's channel layout), out int16 [nticks][2304] read-modify-write.
int feed_resample_plane(long feed_rate, long enc_rate, int fch, int sch, const int16_t *x, int nticks, int16_t *out)
{
    const int ratio = tl_fa_ratio_of(feed_rate, enc_rate);
    if (ratio < 0 || !x || !out || nticks <= 0 || nticks > TL_FA_MAX_FRAMES || (fch != 1 && fch != 2) || (sch != 1 && sch != 2)) return 18;
    TlConfig fc, sc;
    memset(&fc, 0, sizeof fc); memset(&sc, 0, sizeof sc);
    fc.nch = fch; sc.nch = sch;
    const int32_t zero = 0, ra = ratio;
    std::vector<int16_t> taps, carry((size_t)2 * TL_FA_CARRY * 2, 0), plane((size_t)nticks * 2304, (int16_t)0x5555);
    load_taps(taps);
    memcpy(plane.data(), x, sizeof(int16_t) * (size_t)tl_fa_K(nticks - 1, ratio) * 1152 * (size_t)fch);
    int32_t pos[2] = {0, 0};
    TlFeedAdaptLaunch D;
    memset(&D, 0, sizeof D);
    D.F.configs = &fc; D.F.feed_cfg = &zero; D.F.pcm = out; D.F.nstreams = 1; D.F.nframes = nticks;
    D.ratio = &ra; D.sconfigs = &sc; D.stream_cfg = &zero; D.taps = taps.data();
    D.plane = plane.data(); D.carry = carry.data(); D.pos = pos;
    for (int f = nticks - 1; f >= 0; f--) resample_slot(D, 0, f);
    return 0;
}
}
