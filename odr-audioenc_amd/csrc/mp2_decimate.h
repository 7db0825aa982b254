// mp2_decimate.h -- the device decimator's body (include/toolame_batch.h, tlb_decimate_*): 48 kHz (1/2), 32 kHz (3/4) and 44.1 kHz (80/147)
// sources to a 24 kHz encoder, ahead of the ingest.  The counterpart of mp2_resample.h for sources ABOVE the encoder's rate: the reference's
// inputs convert in both directions before AudioEnc::run() sees a sample (src/VLCInput.cpp:208, src/GSTInput.cpp:124-133) and it has no
// resampler of its own, so the arithmetic is DEFINED here, in integers, by the committed table csrc/tl_decimate_taps.inc (int16 H[L][64],
// every row sums to 32768):
//   q(n) = floor((n M + M - 1) / L), p(n) = (n M + M - 1) mod L     n: output samples of the stream since its last reset
//   acc(n) = sum_t H[p(n)][t] x[q(n) - t], t = 0..63                x: source frames since the reset, zeros before it; the exact integer sum
//   y(n)  = clamp((acc(n) + 16384) >> 15, -32768, 32767)
// One workgroup of TL_DC_WAVES waves per (frame, stream) slot.  tl_decimate_fill is one wave's share of bringing the ratio's table, the
// slot's source frames and the 63 before them into LDS, tl_decimate_wave its share of the 1152 outputs (and, for the call's last slot, of
// the stream's record); both in the lane macros of mp2_wave.h so that tests/emu/mp2_decimate_emu.cpp runs the same text as lane loops.  The
// kernel puts one workgroup barrier between fill and wave.  A stream without a down source has no share in either: its slots are neither
// read nor written.
//
// Phase.  The M - 1 in q makes the frames regular: the last output of frame f reaches q = ceil(1152 (f + 1) M / L) - 1, so frame f consumes
// the source frames [S(f), S(f + 1)), S(f) = ceil(1152 f M / L), f = 0 included, and its first output has q >= S(f): no output reaches
// further back than 63 frames before the slot's first source frame.  1152 M / L is whole for 1/2 (2304) and 3/4 (1536); for 80/147 five
// frames are 5760 outputs = 10 584 source frames exactly, so a stream's position is its frame counter mod 5 (`pos`), and q, p of the outputs
// n' = 1152 pos + i follow from n' alone: (5760 + 1151) * 147 + 146 < 2^31, 32-bit arithmetic throughout.
// The sum.  sum |H[p][16 k .. 16 k + 15]| is at most 40 811 for every quarter k of every row, times 32 768 below 2^31: each quarter of a row is
// summed in 32 bits, the four quarters are added in 64 (a whole row reaches 67 496 and would not fit).  tests/test_decimate_taps.py asserts
// the bound on the table.
// LDS.  Rows lie 144 bytes apart (TL_DC_ROW = 72 int16 = 36 dwords).  For 80/147 consecutive outputs use rows 147 = 67 apart (mod 80), i.e.
// 13 rows DOWN: 13 * 36 dwords = 468 = 20 (mod 64).  The sixteen lanes of a ds_read_b128 group hold every lane number mod 16 once, and
// 16 * 20 = 0 (mod 64), so they start at 20 k mod 64, k = 0..15 = every multiple of four once and tile the 64 banks; a wrap adds 80 * 36
// dwords = 2880 = 0 (mod 64).  For 3/4 the three rows start at banks 0, 36, 8 and lanes of one row read one address; 1/2 has one row.
// The source.  History and slot lie behind one word of padding (TL_DC_AT = 64), so that for 1/2, where q = 2 n + 1 and neighbouring lanes start
// two frames apart, the frames of taps t, t + 1 (t even) are an ALIGNED pair at index TL_DC_AT + 2 i - t: one 8-byte read of two L/R frames (a
// half-wave covers 64 consecutive dwords) or one 4-byte read of two samples of a one-channel stream, where single reads would put lanes i and
// i + 16 of a half-wave two dwords apart times sixteen = on one of ds_read_b32's 32 banks.  3/4 and 80/147 advance 1 or 2 frames from lane to
// lane at no fixed parity and read one frame per lane and tap; their half-waves span about 43 and 59 dwords, so some banks serve two lanes.
// None of this has been measured: the conflict counters have not been read on the hardware.
#pragma once
#include <stdint.h>

#define TL_DC_WAVES 4
#define TL_DC_FRAME 1152
#define TL_DC_TAPS 64                 // T
#define TL_DC_HIST (TL_DC_TAPS - 1)   // source frames of history a slot needs
#define TL_DC_AT 64                   // index of the slot's first source frame in LDS (history at 1 .. 63, [0] is padding: see The source above)
#define TL_DC_ROW 72                  // int16 per table row in LDS (64 taps + 8 of padding: see LDS above)
#define TL_DC_MAXL 80
#define TL_DC_MAX_NEED 2304
#define TL_DC_SLOT 4608               // int16 per wide slot
#define TL_DC_STATE_WORDS 64          // per stream and copy: 63 source frames (oldest first; L | R << 16, or the sample of a one-channel stream in
                                      // the low half), then the frame position in the cycle
#define TL_DC_TABLE_ROWS (80 + 3 + 1) // the three tables one behind the other: [80][64], [3][64], [1][64]
#define TL_DC_OFF 0
#define TL_DC_80_147 1
#define TL_DC_3_4 2
#define TL_DC_1_2 3

// the ratio of a legal (source, encoder) pair; TL_DC_OFF: none
static inline int tl_dc_ratio_of(long source, long encoder)
{
    if (encoder != 24000) return TL_DC_OFF;
    return source == 44100 ? TL_DC_80_147 : source == 32000 ? TL_DC_3_4 : source == 48000 ? TL_DC_1_2 : TL_DC_OFF;
}
#define tl_dc_cycle(ratio) ((ratio) == TL_DC_80_147 ? 5 : 1)         /* frames after which the phase repeats (a macro: host and device) */
#define tl_dc_L(ratio) ((ratio) == TL_DC_80_147 ? 80 : (ratio) == TL_DC_3_4 ? 3 : 1)
#define tl_dc_M(ratio) ((ratio) == TL_DC_80_147 ? 147 : (ratio) == TL_DC_3_4 ? 4 : 2)
#define tl_dc_first_row(ratio) ((ratio) == TL_DC_80_147 ? 0 : (ratio) == TL_DC_3_4 ? 80 : 83)       /* the ratio's table among the three */

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the constants above and nothing else
struct alignas(16) TlDcVec { int16_t v[8]; };                        // 16 bytes: one global_load_dwordx4 / ds_read_b128 per lane
struct alignas(16) TlDecimateLds {
    int16_t tab[TL_DC_MAXL * TL_DC_ROW];                             // 11 520 bytes
    uint32_t x[TL_DC_AT + TL_DC_MAX_NEED];                           // padding, history, then the slot's source frames (9472 bytes); a one-channel stream uses it as int16
};

TL_FN unsigned tl_dc_div(unsigned v, int ratio) { return ratio == TL_DC_80_147 ? v / 80u : ratio == TL_DC_3_4 ? v / 3u : v; }
// S(pos): first source frame of frame `pos` of the cycle, counted from the cycle's start; tl_dc_start(pos + 1) - tl_dc_start(pos) = need
TL_FN int tl_dc_start(int pos, int ratio)
{
    const unsigned L = (unsigned)tl_dc_L(ratio), M = (unsigned)tl_dc_M(ratio);
    return (int)tl_dc_div((unsigned)(TL_DC_FRAME * pos) * M + L - 1u, ratio);
}

// src: the slot's source frames (the first `need` are read, nothing behind them); prev: the wide slot of the frame before in the same call,
// of which the last 63 of its prev_need source frames are read, or NULL: the history comes from the stream's record rec_in.  taps: the
// ratio's table int16 [L][64] in global memory.
TL_FN void tl_decimate_fill(const int16_t *TL_RESTRICT src, const int16_t *TL_RESTRICT prev, const uint32_t *TL_RESTRICT rec_in, const int16_t *TL_RESTRICT taps,
                            TlDecimateLds &w, int nch, int ratio, int need, int prev_need, int wave)
{
    const int L = tl_dc_L(ratio);
    const TlDcVec *tg = (const TlDcVec *)taps;
    TlDcVec *tl = (TlDcVec *)w.tab;
    int16_t *x16 = (int16_t *)w.x;
    const int vals = need * nch;                                     // int16 of the slot that are read: whole 16-byte pieces, then one by one
    TL_LANES_BEGIN
        for (int k = wave * 64 + lane; k < 8 * L; k += 64 * TL_DC_WAVES) tl[(k >> 3) * (TL_DC_ROW / 8) + (k & 7)] = tg[k];
        if (wave == 0 && lane < TL_DC_HIST) {
            if (nch == 2) w.x[TL_DC_AT - TL_DC_HIST + lane] = prev ? ((const uint32_t *)prev)[prev_need - TL_DC_HIST + lane] : rec_in[lane];
            else x16[TL_DC_AT - TL_DC_HIST + lane] = prev ? prev[prev_need - TL_DC_HIST + lane] : (int16_t)(rec_in[lane] & 0xffffu);
        }
        TlDcVec *xv = (TlDcVec *)(nch == 2 ? (int16_t *)&w.x[TL_DC_AT] : &x16[TL_DC_AT]);
        for (int k = wave * 64 + lane; k < (vals >> 3); k += 64 * TL_DC_WAVES) xv[k] = ((const TlDcVec *)src)[k];
        if (wave == TL_DC_WAVES - 1 && lane < (vals & 7)) ((int16_t *)xv)[(vals & ~7) + lane] = src[(vals & ~7) + lane];
    TL_LANES_END
}

// one tap on one source frame: h * the frame's sample(s) into the quarter's sums
#define TL_DC_TAP(u, j) ((int32_t)(int16_t)((u) >> (16 * (j))))                      /* tap j of four in a 64-bit piece of a row */
#define TL_DC_MAC(a, h, s) do { (a)[0] += (h) * (int32_t)(int16_t)((s) & 0xffffu); (a)[1] += (h) * (int32_t)(int16_t)((s) >> 16); } while (0)

// The 1152 outputs of a slot, one variant per (channels, source read): NCH and PAIR are compile-time so that the 64 taps unroll into
// straight multiply-adds without a branch.  A row comes in as eight 16-byte pieces (TL_LD2: one ds_read_b128 each); PAIR (ratio 1/2)
// reads the source as aligned pairs -- `at` is odd there, so taps t, t + 1 (t even) lie on the aligned pair at index at - t - 1.
template <int NCH, bool PAIR> TL_FN void tl_decimate_outputs(int16_t *TL_RESTRICT dst, const TlDecimateLds &w, int ratio, int pos, int wave)
{
    const unsigned M = (unsigned)tl_dc_M(ratio), L = (unsigned)tl_dc_L(ratio);
    const int start = tl_dc_start(pos, ratio);
    const int16_t *x16 = (const int16_t *)w.x;
    TL_LANES_BEGIN
        for (int i = wave * 64 + lane; i < TL_DC_FRAME; i += 64 * TL_DC_WAVES) {
            const unsigned nm = (unsigned)(TL_DC_FRAME * pos + i) * M + M - 1u, q = tl_dc_div(nm, ratio), p = nm - q * L;
            const int at = TL_DC_AT + (int)q - start;                 // index of x[q(n)]: TL_DC_AT .. TL_DC_AT + need - 1
            const double *hp = (const double *)&w.tab[p * TL_DC_ROW];
            int32_t a[4][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}};      // [quarter of the row][channel]; a one-channel stream leaves [.][1] alone
#pragma unroll
            for (int v = 0; v < 8; v++) {
                double d0, d1;
                TL_LD2(hp + 2 * v, d0, d1);
                const uint64_t u[2] = {tl_d2u(d0), tl_d2u(d1)};      // taps 8 v .. 8 v + 3, 8 v + 4 .. 8 v + 7
#pragma unroll
                for (int j = 0; j < 8; j += 2) {
                    const int t = 8 * v + j;
                    const int32_t h0 = TL_DC_TAP(u[j >> 2], j & 3), h1 = TL_DC_TAP(u[j >> 2], (j & 3) + 1);
                    if (PAIR && NCH == 2) {
                        const uint64_t s = *(const uint64_t *)&w.x[at - t - 1];      // frames q - t - 1 (low) and q - t (high)
                        TL_DC_MAC(a[v >> 1], h0, (uint32_t)(s >> 32)); TL_DC_MAC(a[v >> 1], h1, (uint32_t)s);
                    } else if (PAIR) {
                        const uint32_t s = *(const uint32_t *)&x16[at - t - 1];
                        a[v >> 1][0] += h0 * (int32_t)(int16_t)(s >> 16); a[v >> 1][0] += h1 * (int32_t)(int16_t)(s & 0xffffu);
                    } else if (NCH == 2) {
                        TL_DC_MAC(a[v >> 1], h0, w.x[at - t]); TL_DC_MAC(a[v >> 1], h1, w.x[at - t - 1]);
                    } else {
                        a[v >> 1][0] += h0 * (int32_t)x16[at - t]; a[v >> 1][0] += h1 * (int32_t)x16[at - t - 1];
                    }
                }
            }
            int32_t y[2];
#pragma unroll
            for (int c = 0; c < NCH; c++) {
                const int64_t r = ((int64_t)a[0][c] + (int64_t)a[1][c] + (int64_t)a[2][c] + (int64_t)a[3][c] + 16384) >> 15;
                y[c] = r < -32768 ? -32768 : r > 32767 ? 32767 : (int32_t)r;
            }
            if (NCH == 2) ((uint32_t *)dst)[i] = (uint32_t)(uint16_t)y[0] | ((uint32_t)(uint16_t)y[1] << 16);
            else dst[i] = (int16_t)y[0];
        }
    TL_LANES_END
}

// dst: the slot's 1152 output frames (interleaved L R, or 1152 samples of a one-channel stream; nothing behind them is written);
// rec_out: the stream's record to write, or NULL when this is not the call's last slot of the stream; newpos its position entry.
TL_FN void tl_decimate_wave(int16_t *TL_RESTRICT dst, uint32_t *TL_RESTRICT rec_out, const TlDecimateLds &w, int nch, int ratio, int pos, int need, int newpos, int wave)
{
    if (ratio == TL_DC_1_2) { if (nch == 2) tl_decimate_outputs<2, true>(dst, w, ratio, pos, wave); else tl_decimate_outputs<1, true>(dst, w, ratio, pos, wave); }
    else if (nch == 2) tl_decimate_outputs<2, false>(dst, w, ratio, pos, wave);
    else tl_decimate_outputs<1, false>(dst, w, ratio, pos, wave);
    const int16_t *x16 = (const int16_t *)w.x;
    TL_LANES_BEGIN
        if (rec_out && wave == 0)
            rec_out[lane] = lane == TL_DC_HIST ? (uint32_t)newpos : nch == 2 ? w.x[TL_DC_AT + need - TL_DC_HIST + lane] : (uint32_t)(uint16_t)x16[TL_DC_AT + need - TL_DC_HIST + lane];
    TL_LANES_END
}

// One wave of the workgroup of slot (f, s) before / after the barrier.  wide int16 [nframes][nstreams][4608], out int16 [nframes][nstreams][2304];
// state uint32 [2][nstreams][64]: the launch reads copy `flip` and writes the other (the first and the last slot of a stream are different
// workgroups); ratio int32 [nstreams].  tl_decimate_slot: what is uniform over the slot's workgroup.
struct TlDecimateSlot { int ratio, nch, pos, need, newpos; };
TL_FN TlDecimateSlot tl_decimate_slot(const int32_t *TL_RESTRICT ratio, const uint32_t *TL_RESTRICT state, int nch, int s, int f, int nstreams, int nframes, int flip)
{
    TlDecimateSlot S;
    S.ratio = ratio[s]; S.nch = nch; S.pos = 0; S.need = 0; S.newpos = 0;
    if (S.ratio < TL_DC_80_147 || S.ratio > TL_DC_1_2) { S.ratio = TL_DC_OFF; return S; }
    const int cycle = tl_dc_cycle(S.ratio);
    const int pos0 = (int)(state[((size_t)flip * (size_t)nstreams + (size_t)s) * TL_DC_STATE_WORDS + TL_DC_HIST] % (unsigned)cycle);
    S.pos = (pos0 + f) % cycle;
    S.need = tl_dc_start(S.pos + 1, S.ratio) - tl_dc_start(S.pos, S.ratio);
    S.newpos = (pos0 + nframes) % cycle;
    return S;
}
TL_FN void tl_decimate_before(const int16_t *TL_RESTRICT wide, const uint32_t *TL_RESTRICT state, const int16_t *TL_RESTRICT taps,
                              TlDecimateLds &w, const TlDecimateSlot &S, int s, int f, int nstreams, int flip, int wave)
{
    if (S.ratio == TL_DC_OFF) return;
    const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
    const int cycle = tl_dc_cycle(S.ratio), ppos = (S.pos + cycle - 1) % cycle;
    const int prev_need = tl_dc_start(ppos + 1, S.ratio) - tl_dc_start(ppos, S.ratio);
    tl_decimate_fill(wide + slot * TL_DC_SLOT, f > 0 ? wide + (slot - (size_t)nstreams) * TL_DC_SLOT : nullptr,
                     state + ((size_t)flip * (size_t)nstreams + (size_t)s) * TL_DC_STATE_WORDS,
                     taps + tl_dc_first_row(S.ratio) * TL_DC_TAPS, w, S.nch, S.ratio, S.need, prev_need, wave);
}
TL_FN void tl_decimate_after(uint32_t *TL_RESTRICT state, int16_t *TL_RESTRICT out, const TlDecimateLds &w, const TlDecimateSlot &S, int s, int f,
                             int nstreams, int nframes, int flip, int wave)
{
    if (S.ratio == TL_DC_OFF) return;
    const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
    tl_decimate_wave(out + slot * 2304, f == nframes - 1 ? state + ((size_t)(flip ^ 1) * (size_t)nstreams + (size_t)s) * TL_DC_STATE_WORDS : nullptr,
                     w, S.nch, S.ratio, S.pos, S.need, S.newpos, wave);
}
#endif
