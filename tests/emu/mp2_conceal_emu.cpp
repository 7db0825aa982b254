// mp2_conceal_emu.cpp -- TEST-ONLY host emulation of the strict feed kernels with the feed concealment behind them (csrc/mp2_feed.h and
// csrc/mp2_conceal.h over csrc/mp2_unpack.h and csrc/mp2_synth.h, compiled with -DTL_EMULATE: every lane region is a loop over 64 lanes).
// tests/conceallib.py compiles it into a temporary directory together with csrc/mp2_host.cpp; the product library never contains or loads it.
// The entry points mirror tlb_feed_set / tlb_conceal_enable / tlb_conceal_reset / tlb_feed_device (csrc/tlb_feed.cpp, csrc/tlb_conceal.cpp):
// the feed units and the feed carry, then the conceal units and the conceal carry, every unit of a kernel in DESCENDING order (nothing is
// carried from unit to unit inside a call).  The G buffer's slots are GUARD bytes wider than the launch's and hold 0xA5 before the first
// call: conceal_guard_ok says whether everything the carry may not write still does.
#define TL_EMULATE 1
#define TL_CC_BODY 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_unpack.h"
#include "../../odr-audioenc_amd/csrc/mp2_synth.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed.h"
#include "../../odr-audioenc_amd/csrc/mp2_conceal.h"

#define GUARD 64
struct Conceal {
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs;
    std::vector<int32_t> feed_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev, g;
    std::vector<TlConcealStream> cs;
    std::vector<TlConcealRecord> rec;
    int stride = 0, any = 0;
};

extern "C" {
// channels[s] = 0: stream s has no feed; hold[s] = 0: no concealment
void *conceal_create(int nstreams, const long *fs, const int *kbps, const int *channels, const int *hold, const int *step, int *err)
{
    Conceal *d = new Conceal;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    for (int s = 0; s < nstreams; s++) {
        d->feed_cfg.push_back(-1);
        d->cs.push_back(TlConcealStream{0, 0, 0, 0});
        if (!channels[s]) { if (hold[s]) { if (err) *err = 18; delete d; return nullptr; } continue; }
        TlConfig c;
        const int rc = hold[s] < 0 || hold[s] > TL_CC_MAX_HOLD || (hold[s] && (step[s] < 1 || step[s] > TL_CC_MAX_STEP)) ? 18
                     : tl_build_config(&c, fs[s], channels[s] == 1 ? 'm' : 's', kbps[s], 1, 0);
        if (rc) { if (err) *err = rc; delete d; return nullptr; }
        d->feed_cfg[(size_t)s] = (int32_t)d->configs.size();
        d->configs.push_back(c);
        if (tl_feed_slot_bytes(c) > d->stride) d->stride = tl_feed_slot_bytes(c);
        if (hold[s]) { d->cs[(size_t)s].hold = (uint32_t)hold[s]; d->cs[(size_t)s].step = (uint32_t)step[s]; d->any = 1; }
    }
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * (size_t)d->stride, 0);
    d->g.assign((size_t)nstreams * (size_t)(d->stride + GUARD), 0xA5);
    d->rec.assign((size_t)nstreams, TlConcealRecord{0, 0, 0, 0, 0, 0, 0, 0});
    if (err) *err = 0;
    return d;
}
void conceal_destroy(void *h) { delete (Conceal *)h; }
int conceal_stride(void *h) { return ((Conceal *)h)->stride; }
int conceal_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int conceal_reset(void *h, int s)
{
    Conceal *d = (Conceal *)h;
    const int ns = (int)d->state.size();
    if (s < -1 || s >= ns) return 18;
    for (int i = 0; i < ns; i++) {
        if (s >= 0 && i != s) continue;
        memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
        memset(&d->rec[(size_t)i], 0, sizeof(TlConcealRecord));
        d->cs[(size_t)i].g_len = 0;
    }
    return 0;
}
void conceal_records(void *h, TlConcealRecord *out) { Conceal *d = (Conceal *)h; memcpy(out, d->rec.data(), sizeof(TlConcealRecord) * d->rec.size()); }
// 1: the guard bytes behind every G slot, and the whole slot of a stream without concealment, are what they were at the start
int conceal_guard_ok(void *h)
{
    Conceal *d = (Conceal *)h;
    const size_t gs = (size_t)(d->stride + GUARD);
    for (size_t s = 0; s < d->state.size(); s++)
        for (size_t i = d->cs[s].hold ? (size_t)d->stride : 0; i < gs; i++) if (d->g[s * gs + i] != 0xA5) return 0;
    return 1;
}
// frames [nframes][nstreams][stride], len [nframes][nstreams], pcm [nframes][nstreams][2304] read-modify-write, report [nframes][nstreams]
int conceal_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, TlFrameReport *report)
{
    Conceal *d = (Conceal *)h;
    if (!frames || !len || !pcm || !report || nframes <= 0) return 18;
    TlConcealLaunch A;
    memset(&A, 0, sizeof A);
    TlFeedLaunch &F = A.F;
    F.tables = &d->tables; F.configs = d->configs.data(); F.feed_cfg = d->feed_cfg.data(); F.synth = &d->synth;
    F.frames = frames; F.len = len; F.report = report; F.pcm = pcm;
    F.state = d->state.data(); F.prev = d->prev.data();
    F.nstreams = (int)d->state.size(); F.nframes = nframes; F.stride = d->stride; F.prev_stride = d->stride;
    A.cs = d->cs.data(); A.rec = d->rec.data(); A.g = d->g.data(); A.g_stride = d->stride + GUARD;
    static thread_local TlSynthLds w;
    for (int s = F.nstreams - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--) tl_feed_unit(w, F, s, f, d->synth.d);
    for (int s = 0; s < F.nstreams; s++) tl_feed_carry(F, s);
    if (!d->any) return 0;
    for (int s = F.nstreams - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--) { memset(&w, 0x55, sizeof w); tl_conceal_unit(w, A, s, f, d->synth.d); }      // (whatever the unit before left in LDS)
    for (int s = 0; s < F.nstreams; s++) tl_conceal_carry(A, s);
    return 0;
}
// The carry alone: ONE stream from its reset over a status sequence cut into calls of cut[0], cut[1], ... slots (no audio: every slot is
// four bytes long and nothing is synthesised) -> its record after the last call
int conceal_fold(int hold, int step, const uint32_t *status, int n, const int *cut, int ncut, TlConcealRecord *out)
{
    if (hold < 1 || hold > TL_CC_MAX_HOLD || step < 1 || step > TL_CC_MAX_STEP || !status || !cut || !out) return 18;
    TlConcealStream cs = {(uint32_t)hold, (uint32_t)step, 0, 0};
    TlConcealRecord rec = {0, 0, 0, 0, 0, 0, 0, 0};
    const int32_t zero = 0;
    uint32_t g[1] = {0};
    int at = 0;
    for (int c = 0; c < ncut; c++) {
        if (cut[c] <= 0 || at + cut[c] > n) return 18;
        std::vector<TlFrameReport> rep((size_t)cut[c]);
        std::vector<uint32_t> frames((size_t)cut[c], 0x12345678u);
        std::vector<int32_t> len((size_t)cut[c], 4);
        for (int i = 0; i < cut[c]; i++) { memset(&rep[(size_t)i], 0, sizeof(TlFrameReport)); rep[(size_t)i].status = status[at + i]; }
        TlConcealLaunch A;
        memset(&A, 0, sizeof A);
        A.F.feed_cfg = &zero; A.F.frames = (const uint8_t *)frames.data(); A.F.len = len.data(); A.F.report = rep.data();
        A.F.nstreams = 1; A.F.nframes = cut[c]; A.F.stride = 4;
        A.cs = &cs; A.rec = &rec; A.g = (uint8_t *)g; A.g_stride = 4;
        tl_conceal_carry(A, 0);
        at += cut[c];
    }
    *out = rec;
    return at == n ? 0 : 18;
}
}
