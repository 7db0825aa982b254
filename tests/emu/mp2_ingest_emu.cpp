// mp2_ingest_emu.cpp -- TEST-ONLY host emulation of the kernels of the caller's glue (csrc/mp2_ingest.h compiled with -DTL_EMULATE:
// every lane region is a loop over 64 lanes, a slot's workgroup a loop over its waves).  tests/ingestlib.py compiles it into a temporary
// directory; the product library never contains or loads it.  The entry points mirror tlb_ingest_host_valid / tlb_underrun_host / tlb_silence_host.
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_ingest.h"

extern "C" {
// in [nframes][nstreams][2304], valid [nframes][nstreams] or null (every slot full), nch / gain (linear) per stream,
// out [nframes][nstreams][2][1152], peaks [nframes][nstreams][2].  Slots and waves run in DESCENDING order: nothing is carried between them.
int ing_ingest(const int16_t *in, const int32_t *valid, int nframes, int nstreams, const int32_t *nch, const double *gain, int16_t *out, int16_t *peaks)
{
    if (!in || !nch || !gain || !out || !peaks || nframes <= 0 || nstreams <= 0) return 18;
    for (long slot = (long)nframes * nstreams - 1; slot >= 0; slot--) {
        const int s = (int)(slot % nstreams);
        const int v = valid ? tl_ingest_clamp(valid[slot]) : TL_INGEST_FRAMES;
        int m0 = 0, m1 = 0;
        for (int wave = TL_INGEST_WAVES - 1; wave >= 0; wave--) {
            int p0, p1;
            if (v == TL_INGEST_FRAMES) tl_ingest_wave<true>(in + slot * 2304, out + slot * 2304, nch[s], gain[s], v, wave, p0, p1);
            else tl_ingest_wave<false>(in + slot * 2304, out + slot * 2304, nch[s], gain[s], v, wave, p0, p1);
            m0 = p0 > m0 ? p0 : m0; m1 = p1 > m1 ? p1 : m1;
        }
        peaks[slot * 2] = (int16_t)m0; peaks[slot * 2 + 1] = (int16_t)m1;
    }
    return 0;
}
// valid [nframes][nstreams]; version (0: MPEG-2 LSF, 1: MPEG-1) / fs_idx / nch per stream as TlConfig holds them; both counters [nstreams], read-modify-write
int ing_underrun(const int32_t *valid, int nframes, int nstreams, const int32_t *version, const int32_t *fs_idx, const int32_t *nch, uint32_t *underrun_ms, uint32_t *underruns)
{
    if (!valid || !underrun_ms || !underruns || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = nstreams - 1; s >= 0; s--)
        tl_underrun_stream(valid, underrun_ms, underruns, tl_frame_ms(version[s], fs_idx[s], nch[s]), s, nstreams, nframes);
    return 0;
}
// peaks [nframes][nstreams][2]; version / fs_idx / nch as above; the counter [nstreams], read-modify-write
int ing_silence(const int16_t *peaks, int nframes, int nstreams, const int32_t *version, const int32_t *fs_idx, const int32_t *nch, uint32_t *silence_ms)
{
    if (!peaks || !silence_ms || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = nstreams - 1; s >= 0; s--)
        tl_silence_stream(peaks, silence_ms, tl_frame_ms(version[s], fs_idx[s], nch[s]), s, nstreams, nframes);
    return 0;
}
int ing_src(int i, int valid)
{   // the index map alone: source frame of output frame i, or -1 for a zero
    const int v = tl_ingest_clamp(valid), missing = TL_INGEST_FRAMES - v;
    const int q = missing >= 1 && missing <= TL_INGEST_STRETCH_MAX ? v / missing : 0;
    const int s = q ? tl_stretch_src(i, q) : i;
    return s < v ? s : -1;
}
}
