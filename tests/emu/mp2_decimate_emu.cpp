// mp2_decimate_emu.cpp -- TEST-ONLY host emulation of the device decimator's kernel (csrc/mp2_decimate.h compiled with -DTL_EMULATE: the
// lane regions are loops over 64 lanes).  tests/decimatelib.py compiles it into a temporary directory; the product library never contains
// or loads it.  The entry point mirrors tl_decimate_kernel: one (frame, stream) slot at a time, the four waves' fill, then (the barrier) the
// four waves' outputs.  The state the batch would keep and the tables are handed in by the caller.
#define TL_EMULATE 1
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_wave.h"
#include "../../odr-audioenc_amd/csrc/mp2_decimate.h"

extern "C" {
int dc_state_words(void) { return TL_DC_STATE_WORDS; }
int dc_lds_bytes(void) { return (int)sizeof(TlDecimateLds); }
int dc_table_rows(void) { return TL_DC_TABLE_ROWS; }
// wide int16 [nframes][nstreams][4608]; out int16 [nframes][nstreams][2304]; nch, ratio int32 [nstreams] (ratio: TL_DC_*); state uint32
// [2][nstreams][64], copy `flip` is read and the other written; taps int16 [80][64], [3][64], [1][64] one behind the other.  Slots run in
// DESCENDING order: nothing is carried between them.  The copies are exactly as long as the data and 16-byte aligned as device memory is.
int dc_decimate(const int16_t *wide, int nframes, int nstreams, const int32_t *nch, const int32_t *ratio, uint32_t *state, int flip, const int16_t *taps, int16_t *out)
{
    if (!wide || !out || !nch || !ratio || !state || !taps || nframes <= 0 || nstreams <= 0 || (flip != 0 && flip != 1)) return 18;
    const size_t slots = (size_t)nframes * (size_t)nstreams, wb = slots * TL_DC_SLOT * sizeof(int16_t), ob = slots * 2304 * sizeof(int16_t);
    const size_t sb = (size_t)2 * nstreams * TL_DC_STATE_WORDS * sizeof(uint32_t), tb = (size_t)TL_DC_TABLE_ROWS * TL_DC_TAPS * sizeof(int16_t);
    int16_t *a_src = (int16_t *)aligned_alloc(16, wb), *a_out = (int16_t *)aligned_alloc(16, ob), *a_taps = (int16_t *)aligned_alloc(16, tb);
    uint32_t *a_state = (uint32_t *)aligned_alloc(16, sb);
    memcpy(a_src, wide, wb); memcpy(a_out, out, ob); memcpy(a_taps, taps, tb); memcpy(a_state, state, sb);
    TlDecimateLds *w = (TlDecimateLds *)aligned_alloc(16, sizeof(TlDecimateLds));      // on the heap, exactly its size: an index past the block is an access past the allocation
    for (int f = nframes - 1; f >= 0; f--)
        for (int s = nstreams - 1; s >= 0; s--) {
            memset(w, 0x55, sizeof *w);                              // whatever the workgroup before left in LDS
            const TlDecimateSlot S = tl_decimate_slot(ratio, a_state, nch[s], s, f, nstreams, nframes, flip);
            if (S.ratio == TL_DC_OFF) continue;                      // the workgroup leaves as a whole
            for (int wave = 0; wave < TL_DC_WAVES; wave++) tl_decimate_before(a_src, a_state, a_taps, *w, S, s, f, nstreams, flip, wave);
            for (int wave = TL_DC_WAVES - 1; wave >= 0; wave--) tl_decimate_after(a_state, a_out, *w, S, s, f, nstreams, nframes, flip, wave);
        }
    memcpy(out, a_out, ob); memcpy(state, a_state, sb);
    free(w); free(a_src); free(a_out); free(a_taps); free(a_state);
    return 0;
}
}
