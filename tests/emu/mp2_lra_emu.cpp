// mp2_lra_emu.cpp -- TEST-ONLY host emulation of the loudness range's kernels (csrc/mp2_loudness.h compiled with -DTL_EMULATE: the lane
// regions are loops over 64 lanes).  tests/lralib.py compiles it into a temporary directory; the product library never contains or loads
// it.  lra_loudness mirrors tl_lra_kernel (range != 0: the counting wave) or tl_loudness_kernel (range == 0: the plain one, which must not
// look at hist_st), one wave per 32 consecutive streams; lra_range mirrors tl_lra_range_kernel.  The state the batch would keep on the
// device is handed in by the caller; the table is the committed one.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_loudness.h"
#include "../../odr-audioenc_amd/csrc/tl_loudness_tables.inc"

static_assert(sizeof(TlLoudnessRecord) == 48 && sizeof(TlLraRecord) == 40 && offsetof(TlLraRecord, high_bin) == 36, "records");
static_assert(offsetof(TlLraArgs, A) == 0 && sizeof(TlLraArgs) == sizeof(TlLoudnessArgs) + sizeof(uint32_t *), "the meter's arguments as they are, the counts behind them");

static double *table(void)
{
    double *t = (double *)aligned_alloc(16, sizeof(double) * TL_LD_TABLE_DOUBLES);
    memcpy(t, tl_loudness_taps, sizeof tl_loudness_taps);
    memcpy(t + TL_LD_RATES * 10, tl_loudness_edges, sizeof tl_loudness_edges);
    memcpy(t + TL_LD_RATES * 10 + TL_LD_BINS, tl_loudness_centres, sizeof tl_loudness_centres);
    return t;
}

extern "C" {
int lra_hist_rows(void) { return TL_LD_HIST_ROWS; }
int lra_lds_bytes(void) { return (int)sizeof(TlLoudnessLds); }
// pcm int16 [nframes][nstreams][2][1152]; nch, rate int32 [nstreams]; lane double [10][2 nstreams]; ring double [30][nstreams]; rec 48-byte
// records [nstreams]; hist, hist_st uint32 [752][nstreams] (hist_st may be NULL when range == 0); out 48-byte records [nstreams] or NULL.
// Waves run in DESCENDING order: nothing is carried between them.  The PCM copy is exactly as long as the data and 16-byte aligned.
int lra_loudness(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const int32_t *rate, double *lane, double *ring, void *rec, uint32_t *hist,
                 uint32_t *hist_st, void *out, int range)
{
    if (!pcm || !nch || !rate || !lane || !ring || !rec || !hist || (range && !hist_st) || nframes <= 0 || nstreams <= 0) return 18;
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
    TlLoudnessLds *w = (TlLoudnessLds *)aligned_alloc(16, sizeof(TlLoudnessLds));      // on the heap, exactly its size
    const TlLoudnessArgs A = {a_pcm, lane, ring, (TlLoudnessRecord *)rec, (TlLoudnessRecord *)out, hist, tab, cfg, scfg, nstreams, nframes};
    const TlLraArgs X = {A, hist_st};
    for (int wv = (nstreams + TL_LD_STREAMS - 1) / TL_LD_STREAMS - 1; wv >= 0; wv--) {
        memset(w, 0x55, sizeof *w);                                  // whatever the workgroup before left in LDS
        if (range) tl_lra_wave(X, *w, wv); else tl_loudness_wave(A, *w, wv);
    }
    free(w); free(tab); free(scfg); free(cfg); free(a_pcm);
    return 0;
}

// hist_st uint32 [752][nstreams] -> out 40-byte records [nstreams]; streams in DESCENDING order
int lra_range(const uint32_t *hist_st, int nstreams, void *out)
{
    if (!hist_st || !out || nstreams <= 0) return 18;
    double *tab = table();
    for (int s = nstreams - 1; s >= 0; s--) tl_lra_range(hist_st, tab + TL_LD_RATES * 10 + TL_LD_BINS, (TlLraRecord *)out, s, nstreams);
    free(tab);
    return 0;
}
}
