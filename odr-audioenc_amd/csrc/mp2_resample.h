// mp2_resample.h -- the device resampler's body (include/toolame_batch.h, tlb_resample_*): 44.1 / 22.05 kHz (160/147) and 32 / 16 kHz (3/2)
// sources to the encoder's rate, ahead of the ingest.  The reference's inputs do this before AudioEnc::run() sees a sample (src/VLCInput.cpp:208,
// src/GSTInput.cpp:124-133) and it has no resampler of its own, so the arithmetic is DEFINED here, in integers, by the committed table
// csrc/tl_resample_taps.inc (int16 H[L][32], every row sums to 32768):
//   q(n) = floor(n M / L), p(n) = (n M) mod L              n: output samples of the stream since its last reset
//   acc(n) = sum_t H[p(n)][t] x[q(n) - t], t = 0..31       x: source frames since the reset, zeros before it; the exact integer sum
//   y(n)  = clamp((acc(n) + 16384) >> 15, -32768, 32767)
// One workgroup of TL_RS_WAVES waves per (frame, stream) slot.  tl_resample_fill is one wave's share of bringing the ratio's table, the
// slot's source frames and the 31 frames before them into LDS, tl_resample_wave its share of the 1152 outputs (and, for the call's last
// slot, of the stream's record), tl_resample_copy its share of a slot that has no source; all three in the lane macros of mp2_wave.h so
// that tests/emu/mp2_resample_emu.cpp runs the same text as lane loops.  The kernel puts one workgroup barrier between fill and wave.
//
// Phase.  1152 M / L is whole only for 3/2 (768 source frames a frame).  For 160/147 five frames are 5760 outputs = 5292 source frames
// exactly, so a stream's position is its frame counter mod 5 (`pos`), and frame `pos` of the cycle is the outputs n' = 1152 pos + i:
// q and p follow from n' alone.  The first output of every frame advances q (p(1152 f) < M for both ratios), so no output reaches further
// back than 31 frames before the slot's first source frame.
// The sum.  sum |H[p][0..15]| and sum |H[p][16..31]| are at most 40 309, times 32 768 below 2^31: each half of a row is summed in 32 bits, the
// two halves are added in 64 (a whole row reaches 71 674 and would not fit).  tests/test_resample_taps.py asserts the bound on the table.
// LDS.  Rows lie 80 bytes apart (TL_RS_ROW = 40 int16).  Consecutive outputs use rows 147 apart (mod 160), i.e. 13 rows DOWN: 13 * 20 dwords
// = 260 = 4 (mod 64), so the sixteen lanes of a ds_read_b128 group (whatever sixteen: each group holds every lane number mod 16 once) start
// four banks apart and tile the 64 banks; a wrap adds 160 * 20 dwords = 0 (mod 64).  For 3/2 the three rows start at banks 0, 20, 40 and
// lanes of one row read one address.  The source frames are read as one dword (an L/R pair) or one int16 per lane and tap, at addresses
// that rise by 0 or 1 frame from lane to lane.  The conflict counters have not been read on the hardware.
#pragma once
#include <stdint.h>

#define TL_RS_WAVES 4
#define TL_RS_FRAME 1152
#define TL_RS_TAPS 32                 // T
#define TL_RS_HIST (TL_RS_TAPS - 1)   // source frames of history a slot needs
#define TL_RS_ROW 40                  // int16 per table row in LDS (32 taps + 8 of padding: see LDS above)
#define TL_RS_MAXL 160
#define TL_RS_MAX_NEED 1059
#define TL_RS_STATE_WORDS 32          // per stream and copy: 31 source frames (oldest first; L | R << 16, or the sample of a one-channel stream in
                                      // the low half), then the frame position in the cycle
#define TL_RS_OFF 0
#define TL_RS_160_147 1
#define TL_RS_3_2 2

// the ratio of a legal (source, encoder) pair; TL_RS_OFF: none
static inline int tl_rs_ratio_of(long source, long encoder)
{
    if ((source == 44100 && encoder == 48000) || (source == 22050 && encoder == 24000)) return TL_RS_160_147;
    if ((source == 32000 && encoder == 48000) || (source == 16000 && encoder == 24000)) return TL_RS_3_2;
    return TL_RS_OFF;
}
#define tl_rs_cycle(ratio) ((ratio) == TL_RS_160_147 ? 5 : 1)        /* frames after which the phase repeats (a macro: host and device) */

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the constants above and nothing else
struct alignas(16) TlRsVec { int16_t v[8]; };                        // 16 bytes: one global_load_dwordx4 / ds_read_b128 per lane
struct alignas(16) TlResampleLds {
    int16_t tab[TL_RS_MAXL * TL_RS_ROW];                             // 12 800 bytes
    uint32_t x[TL_RS_HIST + TL_RS_MAX_NEED + 2];                     // history, then the slot's source frames; a one-channel stream uses it as int16
};

TL_FN unsigned tl_rs_div(unsigned v, int ratio) { return ratio == TL_RS_160_147 ? v / 160u : v / 3u; }
// first source frame of frame `pos` of the cycle, counted from the cycle's start; tl_rs_start(pos + 1) - tl_rs_start(pos) = need
TL_FN int tl_rs_start(int pos, int ratio)
{
    const unsigned M = ratio == TL_RS_160_147 ? 147u : 2u;
    return pos > 0 ? (int)tl_rs_div((unsigned)(TL_RS_FRAME * pos - 1) * M, ratio) + 1 : 0;
}

// src: the slot's source frames (the first `need` are read, nothing behind them); prev: the slot of the frame before in the same call, of
// which the last 31 of its prev_need source frames are read, or NULL: the history comes from the stream's record rec_in.  taps: the
// ratio's table int16 [L][32] in global memory.
TL_FN void tl_resample_fill(const int16_t *TL_RESTRICT src, const int16_t *TL_RESTRICT prev, const uint32_t *TL_RESTRICT rec_in, const int16_t *TL_RESTRICT taps,
                            TlResampleLds &w, int nch, int ratio, int need, int prev_need, int wave)
{
    const int L = ratio == TL_RS_160_147 ? 160 : 3;
    const TlRsVec *tg = (const TlRsVec *)taps;
    TlRsVec *tl = (TlRsVec *)w.tab;
    int16_t *x16 = (int16_t *)w.x;
    TL_LANES_BEGIN
        for (int k = wave * 64 + lane; k < 4 * L; k += 64 * TL_RS_WAVES) tl[(k >> 2) * (TL_RS_ROW / 8) + (k & 3)] = tg[k];
        if (wave == 0 && lane < TL_RS_HIST) {
            if (nch == 2) w.x[lane] = prev ? ((const uint32_t *)prev)[prev_need - TL_RS_HIST + lane] : rec_in[lane];
            else x16[lane] = prev ? prev[prev_need - TL_RS_HIST + lane] : (int16_t)(rec_in[lane] & 0xffffu);
        }
        if (nch == 2) for (int j = wave * 64 + lane; j < need; j += 64 * TL_RS_WAVES) w.x[TL_RS_HIST + j] = ((const uint32_t *)src)[j];
        else for (int j = wave * 64 + lane; j < need; j += 64 * TL_RS_WAVES) x16[TL_RS_HIST + j] = src[j];
    TL_LANES_END
}

// dst: the slot's 1152 output frames (interleaved L R, or 1152 samples of a one-channel stream; nothing behind them is written);
// rec_out: the stream's record to write, or NULL when this is not the call's last slot of the stream; newpos its position entry.
TL_FN void tl_resample_wave(int16_t *TL_RESTRICT dst, uint32_t *TL_RESTRICT rec_out, const TlResampleLds &w, int nch, int ratio, int pos, int need, int newpos, int wave)
{
    const unsigned M = ratio == TL_RS_160_147 ? 147u : 2u, L = ratio == TL_RS_160_147 ? 160u : 3u;
    const int start = tl_rs_start(pos, ratio);
    const int16_t *x16 = (const int16_t *)w.x;
    TL_LANES_BEGIN
        for (int i = wave * 64 + lane; i < TL_RS_FRAME; i += 64 * TL_RS_WAVES) {
            const unsigned nm = (unsigned)(TL_RS_FRAME * pos + i) * M, q = tl_rs_div(nm, ratio), p = nm - q * L;
            const int at = TL_RS_HIST + (int)q - start;               // index of x[q(n)]: TL_RS_HIST .. TL_RS_HIST + need - 1
            const TlRsVec *hp = (const TlRsVec *)&w.tab[p * TL_RS_ROW];
            int32_t a0[2] = {0, 0}, a1[2] = {0, 0};                  // [channel]: taps 0..15, taps 16..31
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const TlRsVec h = hp[v];
#pragma unroll
                for (int j = 0; j < 8; j++) {
                    const int t = 8 * v + j;
                    int32_t xl, xr = 0;
                    if (nch == 2) { const uint32_t s = w.x[at - t]; xl = (int16_t)(s & 0xffffu); xr = (int16_t)(s >> 16); }
                    else xl = x16[at - t];
                    if (v < 2) { a0[0] += (int32_t)h.v[j] * xl; a0[1] += (int32_t)h.v[j] * xr; }
                    else { a1[0] += (int32_t)h.v[j] * xl; a1[1] += (int32_t)h.v[j] * xr; }
                }
            }
            int32_t y[2];
#pragma unroll
            for (int c = 0; c < 2; c++) {
                const int64_t r = ((int64_t)a0[c] + (int64_t)a1[c] + 16384) >> 15;
                y[c] = r < -32768 ? -32768 : r > 32767 ? 32767 : (int32_t)r;
            }
            if (nch == 2) ((uint32_t *)dst)[i] = (uint32_t)(uint16_t)y[0] | ((uint32_t)(uint16_t)y[1] << 16);
            else dst[i] = (int16_t)y[0];
        }
        if (rec_out && wave == 0 && lane < TL_RS_STATE_WORDS)
            rec_out[lane] = lane == TL_RS_HIST ? (uint32_t)newpos : nch == 2 ? w.x[need + lane] : (uint32_t)(uint16_t)x16[need + lane];
    TL_LANES_END
}

// a stream without a source: its slot as it is, 2304 values or the first 1152 of a one-channel stream, in 16-byte pieces
TL_FN void tl_resample_copy(const int16_t *TL_RESTRICT src, int16_t *TL_RESTRICT dst, int nch, int wave)
{
    const TlRsVec *s = (const TlRsVec *)src;
    TlRsVec *d = (TlRsVec *)dst;
    TL_LANES_BEGIN
        for (int k = wave * 64 + lane; k < nch * (TL_RS_FRAME / 8); k += 64 * TL_RS_WAVES) d[k] = s[k];
    TL_LANES_END
}

// One wave of the workgroup of slot (f, s) before / after the barrier.  source / out int16 [nframes][nstreams][2304]; state uint32
// [2][nstreams][32]: the launch reads copy `flip` and writes the other (the first and the last slot of a stream are different workgroups);
// ratio int32 [nstreams] or NULL (no stream has a source).  tl_resample_slot: what is uniform over the slot's workgroup.
struct TlResampleSlot { int ratio, nch, pos, need, newpos; };
TL_FN TlResampleSlot tl_resample_slot(const int32_t *TL_RESTRICT ratio, const uint32_t *TL_RESTRICT state, int nch, int s, int f, int nstreams, int nframes, int flip)
{
    TlResampleSlot S;
    S.ratio = ratio ? ratio[s] : TL_RS_OFF; S.nch = nch; S.pos = 0; S.need = 0; S.newpos = 0;
    if (S.ratio == TL_RS_OFF) return S;
    const int cycle = tl_rs_cycle(S.ratio);
    const int pos0 = (int)state[((size_t)flip * (size_t)nstreams + (size_t)s) * TL_RS_STATE_WORDS + TL_RS_HIST] % cycle;
    S.pos = (pos0 + f) % cycle;
    S.need = tl_rs_start(S.pos + 1, S.ratio) - tl_rs_start(S.pos, S.ratio);
    S.newpos = (pos0 + nframes) % cycle;
    return S;
}
TL_FN void tl_resample_before(const int16_t *TL_RESTRICT source, const uint32_t *TL_RESTRICT state, const int16_t *TL_RESTRICT taps, int16_t *TL_RESTRICT out,
                              TlResampleLds &w, const TlResampleSlot &S, int s, int f, int nstreams, int flip, int wave)
{
    const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
    if (S.ratio == TL_RS_OFF) { tl_resample_copy(source + slot * 2304, out + slot * 2304, S.nch, wave); return; }
    const int cycle = tl_rs_cycle(S.ratio), ppos = (S.pos + cycle - 1) % cycle;
    const int prev_need = tl_rs_start(ppos + 1, S.ratio) - tl_rs_start(ppos, S.ratio);
    tl_resample_fill(source + slot * 2304, f > 0 ? source + (slot - (size_t)nstreams) * 2304 : nullptr,
                     state + ((size_t)flip * (size_t)nstreams + (size_t)s) * TL_RS_STATE_WORDS,
                     taps + (S.ratio == TL_RS_160_147 ? 0 : TL_RS_MAXL * TL_RS_TAPS), w, S.nch, S.ratio, S.need, prev_need, wave);
}
TL_FN void tl_resample_after(uint32_t *TL_RESTRICT state, int16_t *TL_RESTRICT out, const TlResampleLds &w, const TlResampleSlot &S, int s, int f,
                             int nstreams, int nframes, int flip, int wave)
{
    if (S.ratio == TL_RS_OFF) return;
    const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
    tl_resample_wave(out + slot * 2304, f == nframes - 1 ? state + ((size_t)(flip ^ 1) * (size_t)nstreams + (size_t)s) * TL_RS_STATE_WORDS : nullptr,
                     w, S.nch, S.ratio, S.pos, S.need, S.newpos, wave);
}
#endif
