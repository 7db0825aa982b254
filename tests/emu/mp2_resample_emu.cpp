// mp2_resample_emu.cpp -- TEST-ONLY host emulation of the device resampler's kernel (csrc/mp2_resample.h compiled with -DTL_EMULATE: the
// lane regions are loops over 64 lanes).  tests/resamplelib.py compiles it into a temporary directory; the product library never contains
// or loads it.  The entry point mirrors tl_resample_kernel: one (frame, stream) slot at a time, the four waves' fill, then (the barrier) the
// four waves' outputs.  The state the batch would keep and the tables are handed in by the caller.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_resample.h"

extern "C" {
int rs_state_words(void) { return TL_RS_STATE_WORDS; }
int rs_lds_bytes(void) { return (int)sizeof(TlResampleLds); }
// source / out int16 [nframes][nstreams][2304]; nch, ratio int32 [nstreams] (ratio: TL_RS_*); state uint32 [2][nstreams][32], copy `flip` is
// read and the other written; taps int16 [160][32] followed by [3][32].  Slots run in DESCENDING order: nothing is carried between them.
// The copies are 16-byte aligned as device memory is.
int rs_resample(const int16_t *source, int nframes, int nstreams, const int32_t *nch, const int32_t *ratio, uint32_t *state, int flip, const int16_t *taps, int16_t *out)
{
    if (!source || !out || !nch || !ratio || !state || !taps || nframes <= 0 || nstreams <= 0 || (flip != 0 && flip != 1)) return 18;
    const size_t pcm = (size_t)nframes * (size_t)nstreams * 2304 * sizeof(int16_t), sb = (size_t)2 * nstreams * TL_RS_STATE_WORDS * sizeof(uint32_t);
    const size_t tb = (size_t)(160 + 3) * TL_RS_TAPS * sizeof(int16_t);
    int16_t *a_src = (int16_t *)aligned_alloc(16, pcm), *a_out = (int16_t *)aligned_alloc(16, pcm), *a_taps = (int16_t *)aligned_alloc(16, (tb + 15) & ~(size_t)15);
    uint32_t *a_state = (uint32_t *)aligned_alloc(16, sb);
    memcpy(a_src, source, pcm); memcpy(a_out, out, pcm); memcpy(a_taps, taps, tb); memcpy(a_state, state, sb);
    static TlResampleLds w;
    for (int f = nframes - 1; f >= 0; f--)
        for (int s = nstreams - 1; s >= 0; s--) {
            memset(&w, 0x55, sizeof w);                              // whatever the workgroup before left in LDS
            const TlResampleSlot S = tl_resample_slot(ratio, a_state, nch[s], s, f, nstreams, nframes, flip);
            for (int wave = 0; wave < TL_RS_WAVES; wave++) tl_resample_before(a_src, a_state, a_taps, a_out, w, S, s, f, nstreams, flip, wave);
            for (int wave = TL_RS_WAVES - 1; wave >= 0; wave--) tl_resample_after(a_state, a_out, w, S, s, f, nstreams, nframes, flip, wave);
        }
    memcpy(out, a_out, pcm); memcpy(state, a_state, sb);
    free(a_src); free(a_out); free(a_taps); free(a_state);
    return 0;
}
}
