// mp2_conceal_conv_emu.cpp -- TEST-ONLY host emulation of the adapted and the down feed kernels with the feed concealment between and behind
// them (csrc/mp2_feed_adapt.h, csrc/mp2_feed_down.h and csrc/mp2_conceal_conv.h over csrc/mp2_feed.h, csrc/mp2_conceal.h, csrc/mp2_unpack.h,
// csrc/mp2_synth.h, csrc/mp2_resample.h and csrc/mp2_decimate.h, compiled with -DTL_EMULATE: every lane region is a loop over 64 lanes).
// tests/concealconvlib.py compiles it into a temporary directory together with csrc/mp2_host.cpp; the product library never contains or loads it.
// One object is ONE path: every fed stream has an adapted feed (down = 0; ratio 1/1 with another channel count included) or a down feed
// (down = 1).  The entry points mirror tlb_feed_set_adapted / tlb_feed_down_set, tlb_feed_loss_enable, tlb_feed_reset / tlb_feed_down_reset
// and tlb_feed_device / tlb_feed_down_device: decode, conceal, resample or decimate, carry, conceal-carry, every unit of a kernel in
// DESCENDING order (nothing is carried from unit to unit inside a call).  The source plane is exactly as long as a call of that many ticks
// needs plus GUARD words either side, G's slots are GUARD bytes wider than the launch's; both hold a pattern that ccv_guard_ok looks for.
#define TL_EMULATE 1
#define TL_CC_BODY 1
#define TL_FA_BODY 1
#define TL_FD_BODY 1
#define TL_CCV_BODY 1
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
#include "../../odr-audioenc_amd/csrc/mp2_feed_adapt.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed_down.h"
#include "../../odr-audioenc_amd/csrc/mp2_conceal.h"
#include "../../odr-audioenc_amd/csrc/mp2_conceal_conv.h"
#include "../../odr-audioenc_amd/csrc/tl_resample_taps.inc"
#include "../../odr-audioenc_amd/csrc/tl_decimate_taps.inc"

#define GUARD 64
struct Conv {
    int down = 0;
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs, sconfigs;     // the feeds' records; one record per stream of which only nch is read
    std::vector<int32_t> feed_cfg, ratio, stream_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev, g;
    std::vector<int16_t> carry;                  // [2][nstreams][carry frames * 2]
    std::vector<int32_t> pos;                    // [2][nstreams]
    std::vector<int16_t> rs_taps;
    int16_t *dc_taps = nullptr;
    std::vector<TlConcealStream> cs;
    std::vector<TlConcealRecord> rec;
    int stride = 0, prev_stride = 0, flip = 0, any = 0, guard_bad = 0;
};

static size_t carry_frames(const Conv *d) { return d->down ? TL_FD_CARRY : TL_FA_CARRY; }

// the resample workgroup of slot (f, s), as tests/emu/mp2_feed_emu.cpp has it
static void resample_slot(const TlFeedAdaptLaunch &A, int s, int f)
{
    static TlResampleLds r;
    static int16_t y[TL_RS_FRAME];
    memset(&r, 0x55, sizeof r); memset(y, 0x55, sizeof y);
    const TlFaSlot S = tl_fa_slot(A, s, f);
    if (S.ratio < 0) return;
    if (S.ratio == TL_RS_OFF) { for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_copy(A, S, s, f, wave); return; }
    for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_fill(A, r, S, s, wave);
    for (int wave = TL_RS_WAVES - 1; wave >= 0; wave--) tl_fa_wave(A, r, S, y, s, f, wave);
    if (S.fch == 1 && S.sch == 2) for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_fa_dup(A, y, s, f, wave);
}
// the decimate workgroup of tick f of stream s, as tests/emu/mp2_feed_down_emu.cpp has it
static void decimate_slot(const TlFeedDownLaunch &A, int s, int f)
{
    const TlFdSlot S = tl_fd_slot_of(A, s, f);
    if (S.ratio == TL_DC_OFF) return;
    TlDecimateLds *r = (TlDecimateLds *)aligned_alloc(16, sizeof(TlDecimateLds));
    int16_t *y = (int16_t *)aligned_alloc(16, sizeof(int16_t) * TL_DC_FRAME);
    memset(r, 0x55, sizeof *r); memset(y, 0x55, sizeof(int16_t) * TL_DC_FRAME);
    for (int wave = 0; wave < TL_DC_WAVES; wave++) tl_fd_fill(A, *r, S, s, wave);
    for (int wave = TL_DC_WAVES - 1; wave >= 0; wave--) tl_fd_wave(A, *r, S, y, s, f, wave);
    if (S.fch == 1 && S.sch == 2) for (int wave = 0; wave < TL_DC_WAVES; wave++) tl_fd_dup(A, y, s, f, wave);
    free(r); free(y);
}

extern "C" {
// channels[s] = 0: stream s has no feed; enc_rate / enc_nch: the stream's own; hold[s] = 0: no concealment
void *ccv_create(int down, int nstreams, const long *fs, const int *kbps, const int *channels, const long *enc_rate, const int *enc_nch,
                 const int *hold, const int *step, int *err)
{
    Conv *d = new Conv;
    d->down = down;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    d->rs_taps.resize((160 + 3) * TL_RS_TAPS);
    memcpy(d->rs_taps.data(), tl_resample_taps_160_147, sizeof tl_resample_taps_160_147);
    memcpy(d->rs_taps.data() + 160 * TL_RS_TAPS, tl_resample_taps_3_2, sizeof tl_resample_taps_3_2);
    d->dc_taps = (int16_t *)aligned_alloc(16, sizeof(int16_t) * TL_DC_TABLE_ROWS * TL_DC_TAPS);
    memcpy(d->dc_taps + tl_dc_first_row(TL_DC_80_147) * TL_DC_TAPS, tl_decimate_taps_80_147, sizeof tl_decimate_taps_80_147);
    memcpy(d->dc_taps + tl_dc_first_row(TL_DC_3_4) * TL_DC_TAPS, tl_decimate_taps_3_4, sizeof tl_decimate_taps_3_4);
    memcpy(d->dc_taps + tl_dc_first_row(TL_DC_1_2) * TL_DC_TAPS, tl_decimate_taps_1_2, sizeof tl_decimate_taps_1_2);
    int rc = 0;
    for (int s = 0; s < nstreams && !rc; s++) {
        TlConfig sc;
        memset(&sc, 0, sizeof sc);
        sc.nch = enc_nch[s];
        d->sconfigs.push_back(sc); d->stream_cfg.push_back(s);
        d->feed_cfg.push_back(-1); d->ratio.push_back(down ? TL_DC_OFF : 0);
        d->cs.push_back(TlConcealStream{0, 0, 0, 0});
        if (!channels[s]) { if (hold[s]) rc = 18; continue; }
        if (hold[s] < 0 || hold[s] > TL_CC_MAX_HOLD || (hold[s] && (step[s] < 1 || step[s] > TL_CC_MAX_STEP))) { rc = 18; continue; }
        TlConfig c;
        rc = tl_build_config(&c, fs[s], channels[s] == 1 ? 'm' : 's', kbps[s], 1, 0);
        const int ratio = down ? tl_fd_ratio_of(fs[s], enc_rate[s]) : tl_fa_ratio_of(fs[s], enc_rate[s]);
        if (!rc && (down ? ratio == TL_DC_OFF : ratio < 0 || (fs[s] == enc_rate[s] && channels[s] == enc_nch[s]))) rc = 1;      // (a matching feed is a strict one)
        if (rc) continue;
        d->feed_cfg[(size_t)s] = (int32_t)d->configs.size(); d->ratio[(size_t)s] = ratio;
        d->configs.push_back(c);
        if (tl_feed_slot_bytes(c) > d->stride) d->stride = tl_feed_slot_bytes(c);
        if (hold[s]) { d->cs[(size_t)s].hold = (uint32_t)hold[s]; d->cs[(size_t)s].step = (uint32_t)step[s]; d->any = 1; }
    }
    if (rc) { if (err) *err = rc; free(d->dc_taps); delete d; return nullptr; }
    d->prev_stride = down ? TL_FD_PREV_STRIDE : d->stride;
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * (size_t)d->prev_stride, 0);
    d->g.assign((size_t)nstreams * (size_t)(d->prev_stride + GUARD), 0xA5);
    d->carry.assign((size_t)2 * nstreams * carry_frames(d) * 2, 0);
    d->pos.assign((size_t)2 * nstreams, 0);
    d->rec.assign((size_t)nstreams, TlConcealRecord{0, 0, 0, 0, 0, 0, 0, 0});
    if (err) *err = 0;
    return d;
}
void ccv_destroy(void *h) { free(((Conv *)h)->dc_taps); delete (Conv *)h; }
int ccv_stride(void *h) { return ((Conv *)h)->stride; }
int ccv_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int ccv_reset(void *h, int s)
{
    Conv *d = (Conv *)h;
    const int ns = (int)d->state.size();
    if (s < -1 || s >= ns) return 18;
    for (int i = 0; i < ns; i++) {
        if (s >= 0 && i != s) continue;
        memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
        memset(&d->rec[(size_t)i], 0, sizeof(TlConcealRecord));
        d->cs[(size_t)i].g_len = 0;
        for (int k = 0; k < 2; k++) {
            memset(&d->carry[((size_t)k * ns + i) * carry_frames(d) * 2], 0, sizeof(int16_t) * carry_frames(d) * 2);
            d->pos[(size_t)k * ns + i] = 0;
        }
    }
    return 0;
}
void ccv_records(void *h, TlConcealRecord *out) { Conv *d = (Conv *)h; memcpy(out, d->rec.data(), sizeof(TlConcealRecord) * d->rec.size()); }
// 1: the words either side of every call's source plane, the guard bytes behind every G slot, and the whole slot of a stream without
// concealment, are what they were at the start
int ccv_guard_ok(void *h)
{
    Conv *d = (Conv *)h;
    if (d->guard_bad) return 0;
    const size_t gs = (size_t)(d->prev_stride + GUARD);
    for (size_t s = 0; s < d->state.size(); s++)
        for (size_t i = d->cs[s].hold ? (size_t)d->prev_stride : 0; i < gs; i++) if (d->g[s * gs + i] != 0xA5) return 0;
    return 1;
}
// adapted: frames [nframes][nstreams][stride], len and report [nframes][nstreams]; down: frames [nframes][nstreams][2][stride], len and
// report [nframes][nstreams][2]; pcm [nframes][nstreams][2304] read-modify-write
int ccv_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, TlFrameReport *report)
{
    Conv *d = (Conv *)h;
    if (!frames || !len || !pcm || !report || nframes <= 0 || nframes > (d->down ? TL_FD_MAX_FRAMES : TL_FA_MAX_FRAMES)) return 18;
    const int ns = (int)d->state.size();
    const size_t per = d->down ? TL_FD_PLANE : 2304, words = (size_t)ns * (size_t)nframes * per;
    std::vector<int16_t> plane(words + 2 * GUARD, (int16_t)0x5555);
    TlFeedLaunch F;
    memset(&F, 0, sizeof F);
    F.tables = &d->tables; F.configs = d->configs.data(); F.feed_cfg = d->feed_cfg.data(); F.synth = &d->synth;
    F.frames = frames; F.len = len; F.report = report; F.pcm = pcm;
    F.state = d->state.data(); F.prev = d->prev.data();
    F.nstreams = ns; F.nframes = nframes; F.stride = d->stride; F.prev_stride = d->prev_stride;
    const TlConcealConv X = {d->cs.data(), d->rec.data(), d->g.data(), d->prev_stride + GUARD, 0};
    static thread_local TlSynthLds w;
    if (!d->down) {
        TlConcealAdaptLaunch A;
        memset(&A, 0, sizeof A);
        TlFeedAdaptLaunch &D = A.D;
        D.F = F; D.ratio = d->ratio.data(); D.sconfigs = d->sconfigs.data(); D.stream_cfg = d->stream_cfg.data(); D.taps = d->rs_taps.data();
        D.plane = plane.data() + GUARD; D.carry = d->carry.data(); D.pos = d->pos.data(); D.flip = d->flip; D.strict_ran = 0;
        A.X = X;
        for (int s = ns - 1; s >= 0; s--)
            for (int f = nframes - 1; f >= 0; f--) tl_fa_decode_unit(w, D, s, f, d->synth.d);
        if (d->any)
            for (int s = ns - 1; s >= 0; s--)
                for (int f = nframes - 1; f >= 0; f--) { memset(&w, 0x55, sizeof w); tl_ccv_adapt_unit(w, A, s, f, d->synth.d); }      // (whatever the unit before left in LDS)
        for (int f = nframes - 1; f >= 0; f--)
            for (int s = ns - 1; s >= 0; s--) resample_slot(D, s, f);
        for (int s = 0; s < ns; s++) tl_fa_carry(D, s);
        if (d->any) for (int s = 0; s < ns; s++) tl_ccv_adapt_carry(A, s);
    } else {
        TlConcealDownLaunch A;
        memset(&A, 0, sizeof A);
        TlFeedDownLaunch &D = A.D;
        D.F = F; D.ratio = d->ratio.data(); D.sconfigs = d->sconfigs.data(); D.stream_cfg = d->stream_cfg.data(); D.taps = d->dc_taps;
        D.plane = plane.data() + GUARD; D.carry = d->carry.data(); D.pos = d->pos.data(); D.flip = d->flip;
        A.X = X;
        for (int s = ns - 1; s >= 0; s--)
            for (int f = nframes - 1; f >= 0; f--)
                for (int j = 1; j >= 0; j--) tl_fd_decode_unit(w, D, s, f, j, d->synth.d);
        if (d->any)
            for (int s = ns - 1; s >= 0; s--)
                for (int f = nframes - 1; f >= 0; f--)
                    for (int j = 1; j >= 0; j--) { memset(&w, 0x55, sizeof w); tl_ccv_down_unit(w, A, s, f, j, d->synth.d); }
        for (int f = nframes - 1; f >= 0; f--)
            for (int s = ns - 1; s >= 0; s--) decimate_slot(D, s, f);
        for (int s = 0; s < ns; s++) tl_fd_carry(D, s);
        if (d->any) for (int s = 0; s < ns; s++) tl_ccv_down_carry(A, s);
    }
    for (size_t i = 0; i < GUARD; i++) if (plane[i] != 0x5555 || plane[GUARD + words + i] != 0x5555) d->guard_bad = 1;
    d->flip ^= 1;
    return 0;
}
}
