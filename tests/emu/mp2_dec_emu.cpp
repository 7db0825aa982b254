// mp2_dec_emu.cpp -- TEST-ONLY host emulation of the frame check / decode kernels (csrc/mp2_unpack.h, csrc/mp2_synth.h compiled with
// -DTL_EMULATE: every lane region is a loop over 64 lanes).  tests/test_decode_emu.py compiles it into a temporary directory together
// with csrc/mp2_host.cpp; the product library never contains or loads it.  The entry points mirror tlb_decode_* (csrc/tlb_decode.cpp).
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_unpack.h"
#include "../../odr-audioenc_amd/csrc/mp2_synth.h"

struct Dec {
    TlTables tables;
    TlSynthTables synth;
    std::vector<TlConfig> configs;
    std::vector<int32_t> stream_cfg;
    std::vector<TlDecStream> state;
    std::vector<uint8_t> prev;
    unsigned long long bad = 0;
    int out_stride = 0;
};

extern "C" {
void *dec_create(int nstreams, const long *fs, const char *mode, const int *kbps, const int *psy, const int *pad, int *err)
{
    Dec *d = new Dec;
    tl_build_tables(&d->tables);
    tl_build_synth_tables(&d->synth);
    for (int s = 0; s < nstreams; s++) {
        TlConfig c;
        const int rc = tl_build_config(&c, fs[s], mode[s], kbps[s], psy[s], pad[s]);
        if (rc) { if (err) *err = rc; delete d; return nullptr; }
        d->configs.push_back(c);
        d->stream_cfg.push_back(s);
        const int longest = (c.frame_bytes + (c.pad_frac != 0 ? 1 : 0) + 3) & ~3;
        if (longest > d->out_stride) d->out_stride = longest;
    }
    d->state.assign((size_t)nstreams, TlDecStream());
    memset(d->state.data(), 0, sizeof(TlDecStream) * (size_t)nstreams);
    d->prev.assign((size_t)nstreams * (size_t)d->out_stride, 0);
    if (err) *err = 0;
    return d;
}
void dec_destroy(void *h) { delete (Dec *)h; }
int dec_out_stride(void *h) { return ((Dec *)h)->out_stride; }
int dec_frame_bytes(void *h, int s) { return ((Dec *)h)->configs[(size_t)s].frame_bytes; }
int dec_pads(void *h, int s) { return ((Dec *)h)->configs[(size_t)s].pad_frac != 0; }
int dec_sizeof_report(void) { return (int)sizeof(TlFrameReport); }
int dec_sizeof_fields(void) { return (int)sizeof(TlFrameFields); }
long dec_bad_frames(void *h) { return (long)((Dec *)h)->bad; }
int dec_reset(void *h, int s)
{
    Dec *d = (Dec *)h;
    if (s < -1 || s >= (int)d->state.size()) return 18;
    for (int i = 0; i < (int)d->state.size(); i++) if (s < 0 || i == s) memset(&d->state[(size_t)i], 0, sizeof(TlDecStream));
    return 0;
}
// frames [nframes][nstreams][out_stride], len [nframes][nstreams] or null, report [nframes][nstreams], fields / pcm as tlb_decode_host.
// Units run in DESCENDING order (slots descending within streams descending): nothing is carried from unit to unit inside a call.
int dec_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, TlFrameReport *report, TlFrameFields *fields, int16_t *pcm)
{
    Dec *d = (Dec *)h;
    if (!frames || !report || nframes <= 0) return 18;
    TlDecLaunch A;
    memset(&A, 0, sizeof A);
    A.tables = &d->tables; A.configs = d->configs.data(); A.stream_cfg = d->stream_cfg.data(); A.synth = &d->synth;
    A.frames = frames; A.len = len; A.report = report; A.fields = fields; A.pcm = pcm;
    A.state = d->state.data(); A.prev = d->prev.data(); A.bad = &d->bad;
    A.nstreams = (int)d->state.size(); A.nframes = nframes; A.out_stride = d->out_stride;
    static thread_local TlSynthLds w;
    for (int s = A.nstreams - 1; s >= 0; s--)
        for (int f = nframes - 1; f >= 0; f--)
            if (tl_unpack_unit(w.d[0], A, s, f) & TL_DEC_BAD_MASK) d->bad++;
    if (pcm)
        for (int s = A.nstreams - 1; s >= 0; s--)
            for (int f = nframes - 1; f >= 0; f--) tl_synth_unit(w, A, s, f, d->synth.d);
    for (int s = 0; s < A.nstreams; s++) tl_dec_carry(A, s);
    return 0;
}
}
