// mp2_limiter_emu.cpp -- TEST-ONLY host emulation of the device limiter's kernel (csrc/mp2_limiter.h compiled with -DTL_EMULATE: the lane
// regions are loops over 64 lanes).  tests/limiterlib.py compiles it into a temporary directory; the product library never contains or
// loads it.  lm_limit mirrors tl_limiter_kernel: one wave per stream.  The state the batch would keep on the device is handed in by the
// caller; the table is the committed one.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_limiter.h"
#include "../../odr-audioenc_amd/csrc/tl_truepeak_taps.inc"

static_assert(sizeof(TlLimiterRecord) == 32, "record");
static_assert(sizeof tl_truepeak_taps == 3 * TL_TP_TAPS * sizeof(int16_t), "table");
static_assert(TL_LM_STATE == 172, "state");

extern "C" {
int lm_state_words(void) { return TL_LM_STATE; }
int lm_lds_bytes(void) { return (int)sizeof(TlLimiterLds); }
void lm_paths(long *out) { out[0] = tl_emu_lm_paths[0]; out[1] = tl_emu_lm_paths[1]; }
// pcm int16 [nframes][nstreams][2][1152], limited in place; nch int32 [nstreams]; step uint32 [nstreams]; rec 32-byte records [nstreams];
// state uint32 [nstreams][172]; out 32-byte records [nstreams] or NULL.  Streams run in DESCENDING order: nothing is carried between them.
// The kernel works on a copy of the PCM exactly as long as the data and 16-byte aligned as device memory is; the LDS block is a heap
// block of exactly its size.
int lm_limit(int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const uint32_t *step, uint32_t ceiling, void *rec, uint32_t *state, void *out)
{
    if (!pcm || !nch || !step || !rec || !state || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = 0; s < nstreams; s++) if (nch[s] < 1 || nch[s] > 2) return 18;
    const size_t pb = (size_t)nframes * (size_t)nstreams * 2 * TL_TP_FRAME * sizeof(int16_t);
    int16_t *a_pcm = (int16_t *)aligned_alloc(16, pb);
    memcpy(a_pcm, pcm, pb);
    TlConfig *cfg = (TlConfig *)calloc((size_t)nstreams, sizeof(TlConfig));
    int32_t *scfg = (int32_t *)malloc(sizeof(int32_t) * (size_t)nstreams);
    for (int s = 0; s < nstreams; s++) { cfg[s].nch = nch[s]; scfg[s] = s; }
    int16_t *taps = (int16_t *)malloc(sizeof tl_truepeak_taps);
    memcpy(taps, tl_truepeak_taps, sizeof tl_truepeak_taps);
    TlLimiterLds *w = (TlLimiterLds *)aligned_alloc(16, sizeof(TlLimiterLds));
    const TlLimiterArgs A = {a_pcm, (TlLimiterRecord *)rec, (TlLimiterRecord *)out, state, step, taps, cfg, scfg, ceiling, nstreams, nframes};
    for (int s = nstreams - 1; s >= 0; s--) {
        memset(w, 0x55, sizeof *w);                                  // whatever the workgroup before left in LDS
        tl_limiter_wave(A, *w, s);
    }
    memcpy(pcm, a_pcm, pb);
    free(w); free(taps); free(scfg); free(cfg); free(a_pcm);
    return 0;
}
}
