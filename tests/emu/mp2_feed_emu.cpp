// mp2_feed_emu.cpp -- TEST-ONLY host emulation of the Layer II feed kernels (csrc/mp2_feed.h over csrc/mp2_unpack.h and csrc/mp2_synth.h,
// compiled with -DTL_EMULATE: every lane region is a loop over 64 lanes).  tests/test_feed_emu.py compiles it into a temporary directory
// together with csrc/mp2_host.cpp; the product library never contains or loads it.  The entry points mirror tlb_feed_* (csrc/tlb_feed.cpp).
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_unpack.h"
#include "../../odr-audioenc_amd/csrc/mp2_synth.h"
#include "../../odr-audioenc_amd/csrc/mp2_feed.h"

struct Feed {
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs;
    std::vector<int32_t> feed_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev;
    int stride = 0;
};

extern "C" {
// channels[s] = 0: stream s has no feed
void *feed_create(int nstreams, const long *fs, const int *kbps, const int *channels, int *err)
{
    Feed *d = new Feed;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    for (int s = 0; s < nstreams; s++) {
        if (!channels[s]) { d->feed_cfg.push_back(-1); continue; }
        TlConfig c;
        const int rc = tl_build_config(&c, fs[s], channels[s] == 1 ? 'm' : 's', kbps[s], 1, 0);
        if (rc) { if (err) *err = rc; delete d; return nullptr; }
        d->feed_cfg.push_back((int32_t)d->configs.size());
        d->configs.push_back(c);
        const int longest = (c.frame_bytes + (c.pad_frac != 0 ? 1 : 0) + 3) & ~3;
        if (longest > d->stride) d->stride = longest;
    }
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * (size_t)d->stride, 0);
    if (err) *err = 0;
    return d;
}
void feed_destroy(void *h) { delete (Feed *)h; }
int feed_stride(void *h) { return ((Feed *)h)->stride; }
int feed_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int feed_reset(void *h, int s)
{
    Feed *d = (Feed *)h;
    if (s < -1 || s >= (int)d->state.size()) return 18;
    for (int i = 0; i < (int)d->state.size(); i++) if (s < 0 || i == s) memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
    return 0;
}
// frames [nframes][nstreams][stride], len [nframes][nstreams], pcm [nframes][nstreams][2304] read-modify-write, report [nframes][nstreams].
// Units run in DESCENDING order (slots descending within streams descending): nothing is carried from unit to unit inside a call.
int feed_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, TlFrameReport *report)
{
    Feed *d = (Feed *)h;
    if (!frames || !len || !pcm || !report || nframes <= 0) return 18;
    TlFeedLaunch A;
    memset(&A, 0, sizeof A);
    A.tables = &d->tables; A.configs = d->configs.data(); A.feed_cfg = d->feed_cfg.data(); A.synth = &d->synth;
    A.frames = frames; A.len = len; A.report = report; A.pcm = pcm;
    A.state = d->state.data(); A.prev = d->prev.data();
    A.nstreams = (int)d->state.size(); A.nframes = nframes; A.stride = d->stride; A.prev_stride = d->stride;
    static thread_local TlSynthLds w;
    for (int s = A.nstreams - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--) tl_feed_unit(w, A, s, f, d->synth.d);
    for (int s = 0; s < A.nstreams; s++) tl_feed_carry(A, s);
    return 0;
}
}
