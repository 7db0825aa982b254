// mp2_monitor.h -- the confidence monitor's fold (include/toolame_batch.h, tlb_monitor_*): what tlb_decode_* says about a stream's frames,
// slot by slot, folded into ONE 32-byte record per stream -- how many frames were looked at, how many failed a check and how many in a
// row, every status flag seen, and the level and the silence counter of the DECODED audio (what a listener hears, as
// tlb_ingest_device's peaks and tlb_silence_device's counter are for the input).  One wavefront per stream walks the stream's slots in
// order; tl_monitor_stream is that wave's text, written with the lane macros of mp2_wave.h so that tests/emu/mp2_monitor_emu.cpp runs it
// as lane loops.  The record lives in registers as TL_MON_WORDS 32-bit words (the little-endian layout of tlb_monitor_record).
//
// Rule for one slot with status st (all integer arithmetic, so the result does not depend on how the slots are cut into calls):
//   1. last_status = st, flags_seen |= st
//   2. st & EMPTY: out_peak = {0, 0}, nothing else changes -- the slot's PCM is not read
//   3. frames++; st & BAD_MASK: bad_frames++, bad_run++; else bad_run = 0
//   4. with PCM: out_peak[c] = max(0, max_i pcm[c][i]); both 0: out_silence_ms += the frame's duration (tl_frame_ms), else it is 0 again.
//      A frame that failed decodes to zeros (mp2_synth.h) and so counts as silence.
//   5. without PCM: out_peak and out_silence_ms stay
#pragma once
#include <stdint.h>
#include "mp2_dec_types.h"

#define TL_MON_WAVES 4                // streams (wavefronts) per workgroup
enum { TL_MON_FRAMES = 0, TL_MON_BAD, TL_MON_RUN, TL_MON_SEEN, TL_MON_LAST, TL_MON_SILENCE, TL_MON_PEAKS /* int16[2] */, TL_MON_RESERVED, TL_MON_WORDS };
#define TL_MON_PCM_WORDS 1152         // a slot's [2][1152] int16 as 32-bit words: 576 per channel, 9 per lane

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the layout above and nothing else
#include "mp2_ingest.h"               // TL_WAVE_MAX_I32, tl_frame_ms

// report [nframes][nstreams], pcm [nframes][nstreams][2][1152] or NULL, record [nstreams][TL_MON_WORDS] read-modify-write.  The lanes
// read word k * 64 + lane of the slot for k = 0..17 -- each a 256-byte line of the wave -- so k < 9 is channel 0 and the rest channel 1
// whatever the lane; the two maxima come from a wave reduction and are uniform, as everything else the record holds.
TL_FN void tl_monitor_stream(const TlFrameReport *TL_RESTRICT report, const int16_t *TL_RESTRICT pcm, uint32_t *TL_RESTRICT record, uint32_t frame_ms,
                             int s, int nstreams, int nframes)
{
    uint32_t *rec = record + (size_t)s * TL_MON_WORDS;
    uint32_t frames = rec[TL_MON_FRAMES], bad = rec[TL_MON_BAD], run = rec[TL_MON_RUN], seen = rec[TL_MON_SEEN], last = rec[TL_MON_LAST];
    uint32_t silence = rec[TL_MON_SILENCE], peaks = rec[TL_MON_PEAKS];
    for (int f = 0; f < nframes; f++) {
        const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
        const uint32_t st = report[slot].status;
        last = st; seen |= st;
        if (st & TL_DEC_EMPTY) { peaks = 0u; continue; }
        frames++;
        if (st & TL_DEC_BAD_MASK) { bad++; run++; } else run = 0u;
        if (!pcm) continue;
        const uint32_t *w = (const uint32_t *)(pcm + slot * (size_t)(2 * TL_MON_PCM_WORDS));
        PV(int, m0); PV(int, m1);
        TL_LANES_BEGIN
            int a0 = 0, a1 = 0;
#pragma unroll
            for (int k = 0; k < TL_MON_PCM_WORDS / 64; k++) {
                const uint32_t v = w[k * 64 + lane];
                const int lo = (int16_t)(v & 0xffffu), hi = (int16_t)(v >> 16);
                const int m = lo > hi ? lo : hi;
                if (k < TL_MON_PCM_WORDS / 128) a0 = m > a0 ? m : a0; else a1 = m > a1 ? m : a1;
            }
            L(m0) = a0; L(m1) = a1;
        TL_LANES_END
        const int p0 = TL_WAVE_MAX_I32(m0), p1 = TL_WAVE_MAX_I32(m1);
        peaks = (uint32_t)p0 | ((uint32_t)p1 << 16);
        silence = peaks == 0u ? silence + frame_ms : 0u;
    }
    TL_LANES_BEGIN
        if (lane == 0) {
            rec[TL_MON_FRAMES] = frames; rec[TL_MON_BAD] = bad; rec[TL_MON_RUN] = run; rec[TL_MON_SEEN] = seen; rec[TL_MON_LAST] = last;
            rec[TL_MON_SILENCE] = silence; rec[TL_MON_PEAKS] = peaks; rec[TL_MON_RESERVED] = 0u;
        }
    TL_LANES_END
}
#endif
