// mp2_monitor_emu.cpp -- TEST-ONLY host emulation of the confidence monitor's fold (csrc/mp2_monitor.h compiled with -DTL_EMULATE: the
// lane region is a loop over 64 lanes, the wave reduction a loop over their values).  tests/monitorlib.py compiles it into a temporary
// directory; the product library never contains or loads it.  The entry point mirrors tlb_monitor_host.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_monitor.h"

extern "C" {
int mon_sizeof_record(void) { return (int)(TL_MON_WORDS * sizeof(uint32_t)); }
// report [nframes][nstreams] (TlFrameReport), pcm [nframes][nstreams][2][1152] or null, version (0: MPEG-2 LSF, 1: MPEG-1) / fs_idx / nch per
// stream as TlConfig holds them, record [nstreams][8] read-modify-write.  Streams run in DESCENDING order: nothing is carried between them.
int mon_fold(const void *report, const int16_t *pcm, int nframes, int nstreams, const int32_t *version, const int32_t *fs_idx, const int32_t *nch, uint32_t *record)
{
    if (!report || !record || !version || !fs_idx || !nch || nframes <= 0 || nstreams <= 0) return 18;
    for (int s = nstreams - 1; s >= 0; s--)
        tl_monitor_stream((const TlFrameReport *)report, pcm, record, tl_frame_ms(version[s], fs_idx[s], nch[s]), s, nstreams, nframes);
    return 0;
}
}
