// mp2_truepeak_emu.cpp -- TEST-ONLY host emulation of the device true-peak meter's kernel (csrc/mp2_truepeak.h compiled with -DTL_EMULATE:
// the lane regions are loops over 64 lanes).  tests/truepeaklib.py compiles it into a temporary directory; the product library never
// contains or loads it.  tp_truepeak mirrors tl_truepeak_kernel: one wave per stream.  The state the batch would keep on the device is
// handed in by the caller; the table is the committed one.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_truepeak.h"
#include "../../odr-audioenc_amd/csrc/tl_truepeak_taps.inc"

static_assert(sizeof(TlTruePeakRecord) == 32, "record");
static_assert(sizeof tl_truepeak_taps == 3 * TL_TP_TAPS * sizeof(int16_t), "table");

extern "C" {
int tp_carry(void) { return TL_TP_CARRY; }
int tp_lds_bytes(void) { return (int)sizeof(TlTruePeakLds); }
// pcm int16 [nframes][nstreams][2][1152]; nch int32 [nstreams]; rec 32-byte records [nstreams]; hist uint32 [nstreams][2][6]; out 32-byte
// records [nstreams] or NULL.  Streams run in DESCENDING order: nothing is carried between them.  The PCM copy is exactly as long as the
// data and 16-byte aligned as device memory is; the LDS block is a heap block of exactly its size.
int tp_truepeak(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, uint32_t ceiling, void *rec, uint32_t *hist, void *out)
{
    if (!pcm || !nch || !rec || !hist || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = 0; s < nstreams; s++) if (nch[s] < 1 || nch[s] > 2) return 18;
    const size_t pb = (size_t)nframes * (size_t)nstreams * 2 * TL_TP_FRAME * sizeof(int16_t);
    int16_t *a_pcm = (int16_t *)aligned_alloc(16, pb);
    memcpy(a_pcm, pcm, pb);
    TlConfig *cfg = (TlConfig *)calloc((size_t)nstreams, sizeof(TlConfig));
    int32_t *scfg = (int32_t *)malloc(sizeof(int32_t) * (size_t)nstreams);
    for (int s = 0; s < nstreams; s++) { cfg[s].nch = nch[s]; scfg[s] = s; }
    int16_t *taps = (int16_t *)malloc(sizeof tl_truepeak_taps);
    memcpy(taps, tl_truepeak_taps, sizeof tl_truepeak_taps);
    TlTruePeakLds *w = (TlTruePeakLds *)aligned_alloc(16, sizeof(TlTruePeakLds));
    const TlTruePeakArgs A = {a_pcm, (TlTruePeakRecord *)rec, (TlTruePeakRecord *)out, hist, taps, cfg, scfg, ceiling, nstreams, nframes};
    for (int s = nstreams - 1; s >= 0; s--) {
        memset(w, 0x55, sizeof *w);                                  // whatever the workgroup before left in LDS
        tl_truepeak_wave(A, *w, s);
    }
    free(w); free(taps); free(scfg); free(cfg); free(a_pcm);
    return 0;
}
}
