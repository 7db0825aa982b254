// mp2_compare_emu.cpp -- TEST-ONLY host emulation of the compare monitor's kernel (csrc/mp2_compare.h compiled with -DTL_EMULATE: the
// lane regions are loops over 64 lanes, the wave sums loops over their values, the 128-bit products unsigned __int128).
// tests/comparelib.py compiles it into a temporary directory; the product library never contains or loads it.  The entry point mirrors
// tlb_compare_host, with the history the batch would keep handed in by the caller.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_compare.h"

extern "C" {
int cmp_sizeof_record(void) { return (int)sizeof(TlCompareRecord); }
int cmp_hist_samples(void) { return TL_CMP_HIST; }
int cmp_delay(void) { return TL_CMP_DELAY; }
// in [nframes][nstreams][2][1152] or null (nframes 1), dec the same, report [nframes][nstreams] (TlFrameReport), nch per stream,
// hist int16 [nstreams][2][cmp_hist_samples()] and record [nstreams] read-modify-write.  Streams run in DESCENDING order: nothing is
// carried between them.  The copies are 16-byte aligned as device memory is.
int cmp_compare(const int16_t *in, const int16_t *dec, const void *report, int nframes, int nstreams, const int32_t *nch, long long min_energy, int corr_num,
                int corr_den, int16_t *hist, void *record)
{
    if (!dec || !report || !record || !hist || !nch || nframes <= 0 || nstreams <= 0 || (!in && nframes != 1)) return 18;
    if (min_energy < 1 || corr_num <= 0 || corr_num > corr_den || corr_den > 1024) return 18;
    const size_t pcm = (size_t)nframes * (size_t)nstreams * 2 * TL_CMP_FRAME * sizeof(int16_t), hb = (size_t)nstreams * 2 * TL_CMP_HIST * sizeof(int16_t);
    int16_t *a_in = in ? (int16_t *)aligned_alloc(16, pcm) : nullptr, *a_dec = (int16_t *)aligned_alloc(16, pcm), *a_hist = (int16_t *)aligned_alloc(16, hb);
    TlCompareRecord *a_rec = (TlCompareRecord *)aligned_alloc(16, (size_t)nstreams * sizeof(TlCompareRecord));
    if (in) memcpy(a_in, in, pcm);
    memcpy(a_dec, dec, pcm); memcpy(a_hist, hist, hb); memcpy(a_rec, record, (size_t)nstreams * sizeof(TlCompareRecord));
    TlCompareParams P; P.min_energy = min_energy; P.corr_num = corr_num; P.corr_den = corr_den;
    static TlCmpLds w;
    for (int s = nstreams - 1; s >= 0; s--) {
        memset(&w, 0x55, sizeof w);                                  // whatever the wave before left in LDS
        tl_compare_stream(a_in, a_dec, (const TlFrameReport *)report, a_hist, a_rec, P, w, nch[s], s, nstreams, nframes);
    }
    memcpy(hist, a_hist, hb); memcpy(record, a_rec, (size_t)nstreams * sizeof(TlCompareRecord));
    free(a_in); free(a_dec); free(a_hist); free(a_rec);
    return 0;
}
}
