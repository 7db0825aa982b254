// mp2_loudness_emu.cpp -- TEST-ONLY host emulation of the device loudness meter's kernels (csrc/mp2_loudness.h compiled with -DTL_EMULATE:
// the lane regions are loops over 64 lanes).  tests/loudnesslib.py compiles it into a temporary directory; the product library never
// contains or loads it.  ld_loudness mirrors tl_loudness_kernel: one wave per 32 consecutive streams; ld_programme mirrors
// tl_loudness_programme_kernel.  The state the batch would keep on the device is handed in by the caller; the table is the committed one.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_loudness.h"
#include "../../odr-audioenc_amd/csrc/tl_loudness_tables.inc"

static_assert(sizeof(TlLoudnessRecord) == 48 && sizeof(TlLoudnessProgramme) == 24, "records");

static double *table(void)
{
    double *t = (double *)aligned_alloc(16, sizeof(double) * TL_LD_TABLE_DOUBLES);
    memcpy(t, tl_loudness_taps, sizeof tl_loudness_taps);
    memcpy(t + TL_LD_RATES * 10, tl_loudness_edges, sizeof tl_loudness_edges);
    memcpy(t + TL_LD_RATES * 10 + TL_LD_BINS, tl_loudness_centres, sizeof tl_loudness_centres);
    return t;
}

extern "C" {
int ld_lane_words(void) { return TL_LD_LANE_WORDS; }
int ld_hist_rows(void) { return TL_LD_HIST_ROWS; }
int ld_lds_bytes(void) { return (int)sizeof(TlLoudnessLds); }
// pcm int16 [nframes][nstreams][2][1152]; nch, rate int32 [nstreams]; lane double [10][2 nstreams]; ring double [30][nstreams]; rec 48-byte
// records [nstreams]; hist uint32 [752][nstreams]; out 48-byte records [nstreams] or NULL.  Waves run in DESCENDING order: nothing is
// carried between them.  The PCM copy is exactly as long as the data and 16-byte aligned as device memory is.
int ld_loudness(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const int32_t *rate, double *lane, double *ring, void *rec, uint32_t *hist, void *out)
{
    if (!pcm || !nch || !rate || !lane || !ring || !rec || !hist || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = 0; s < nstreams; s++) if (tl_ld_rate_row(rate[s]) < 0 || nch[s] < 1 || nch[s] > 2) return 18;
    const size_t pb = (size_t)nframes * (size_t)nstreams * 2 * TL_LD_FRAME * sizeof(int16_t);
    int16_t *a_pcm = (int16_t *)aligned_alloc(16, pb);
    memcpy(a_pcm, pcm, pb);
    TlConfig *cfg = (TlConfig *)calloc((size_t)nstreams, sizeof(TlConfig));
    int32_t *scfg = (int32_t *)malloc(sizeof(int32_t) * (size_t)nstreams);
    for (int s = 0; s < nstreams; s++) {
        const int row = tl_ld_rate_row(rate[s]);
        cfg[s].version = row < 3; cfg[s].fs_idx = row % 3 == 0 ? 1 : row % 3 == 1 ? 0 : 2; cfg[s].nch = nch[s];
        scfg[s] = s;
    }
    double *tab = table();
    TlLoudnessLds *w = (TlLoudnessLds *)aligned_alloc(16, sizeof(TlLoudnessLds));      // on the heap, exactly its size: an index past the block is an access past the allocation
    const TlLoudnessArgs A = {a_pcm, lane, ring, (TlLoudnessRecord *)rec, (TlLoudnessRecord *)out, hist, tab, cfg, scfg, nstreams, nframes};
    for (int wv = (nstreams + TL_LD_STREAMS - 1) / TL_LD_STREAMS - 1; wv >= 0; wv--) {
        memset(w, 0x55, sizeof *w);                                  // whatever the workgroup before left in LDS
        tl_loudness_wave(A, *w, wv);
    }
    free(w); free(tab); free(scfg); free(cfg); free(a_pcm);
    return 0;
}

int ld_programme(const uint32_t *hist, int nstreams, void *out)
{
    if (!hist || !out || nstreams <= 0) return 18;
    double *tab = table();
    for (int s = nstreams - 1; s >= 0; s--) tl_loudness_programme(hist, tab + TL_LD_RATES * 10 + TL_LD_BINS, (TlLoudnessProgramme *)out, s, nstreams);
    free(tab);
    return 0;
}
}
