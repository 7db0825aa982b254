// mp2_truepeak.h -- the device true-peak meter's body (include/toolame_batch.h, tlb_truepeak_*): 4x oversampling after ITU-R BS.1770-4
// Annex 2 of the planar PCM the encoder is given, then the absolute maximum.  The reference measures sample peaks only (--level), so the
// arithmetic is DEFINED in the header and in the committed table csrc/tl_truepeak_taps.inc, in integers:
//   v_p(n) = sum_{t = 0 .. 11} H[p][t] x[n - t] for p = 1, 2, 3 (a row's |H| sum to at most 57 760: 32 bits hold any partial sum);
//   a frame's peak = max over its 1152 n of max(32768 |x[n]|, |v_1(n)|, |v_2(n)|, |v_3(n)|), in units of 2^-30 of full scale.
// The interpolation is a FIR: every output is independent, so the parallel axis is the SAMPLE.  One wave is one stream: it walks the call's
// frames in order and a frame's channels one after the other, each lane takes TL_TP_PER_LANE = 18 consecutive n (64 x 18 = 1152), and the
// frame's peak is one wave reduction.  One wave per workgroup: peak_max and overs need the frames in order, so a stream is one sequential
// owner, and with thousands of streams the streams fill the machine (16 384 streams are 16 waves per SIMD); nothing crosses a wave, so
// there is no workgroup barrier and no atomic.  tl_truepeak_wave is written in the lane macros of mp2_wave.h so that
// tests/emu/mp2_truepeak_emu.cpp runs the same text as lane loops.
//
// Staging.  A channel's 1152 samples are 144 pieces of 16 bytes: lane l brings in pieces l, l + 64 and (l < 16) l + 128 with
// global_load_dwordx4, requested one (frame, channel) ahead of use and kept in registers while the lanes work on the one before.
// LDS, per wave 2 x 2336 bytes.  Channel c's row holds TL_TP_HIST = 16 int16 of history, of which the last 12 are x[-12 .. -1] (the
// definition reaches back 11; twelve keep every dword whole), then the frame: row[16 + n] = x[n].  The pieces land 16-byte aligned
// (ds_write_b128; 64 consecutive lanes write 1024 contiguous bytes).  Lane l needs x[18 l - 11 .. 18 l + 17] and reads the 15 dwords
// from row dword 9 l + 2 = x[18 l - 12] on: 18 l is even, so they are whole dwords.  BANKS: the LDS serves a ds_read_b32 in two groups of
// 32 lanes over 32 banks of 4 bytes; the k-th read of lane l touches bank (9 l + 2 + k) mod 32, and 9 is odd, so l -> 9 l mod 32 is a
// permutation of the 32 banks within either group: every one of the 15 reads is conflict-free.  (A lane taking 16 outputs would start at
// dword 8 l: four banks, eight lanes on each.)  The fill's ds_write_b128 goes in groups of eight consecutive lanes = 32 contiguous
// dwords, every bank once.  Behind the frame lanes 0 .. 5 move the row's last six dwords to the history's.  Nothing of this has been
// measured on the hardware.
// Products.  Taps and samples are 16 bits, so two products are one v_dot2 (TL_TP_DOT2): the taps of a phase are six packed dwords,
// uniform over the wave, K[p][i] = H[p][2 i] << 16 | H[p][2 i + 1].  Output n = 18 l + m pairs x[n - 2 i] (high half) with x[n - 2 i - 1]
// (low half) = the window's int16 j + 1 and j for j = m + 11 - 2 i: for odd m that is dword j / 2 as loaded, for even m the dword
// that straddles two loaded ones, put together from its neighbours once per (frame, channel) (u[k] = x[k] >> 16 | x[k + 1] << 16, fourteen
// of them).  18 x 3 x 6 = 324 dot2 per lane, channel and frame.
//
// Device memory, allocated by tlb_truepeak_enable alone (80 bytes per stream):
//   rec    TlTruePeakRecord [nstreams]              the record as it is reported
//   hist   uint32 [nstreams][2][TL_TP_CARRY / 2]    x[-12 .. -1] of either channel
#pragma once
#include <stdint.h>
#include "mp2_types.h"

#define TL_TP_FRAME 1152
#define TL_TP_TAPS 12                 // per phase
#define TL_TP_PER_LANE 18             // consecutive outputs of a lane: 64 x 18 = 1152, and 9 dwords a lane (see BANKS above)
#define TL_TP_HIST 16                 // int16 ahead of the frame in a row of LDS: the pieces stay 16-byte aligned
#define TL_TP_CARRY 12                // int16 carried per channel: x[-12 .. -1]
#define TL_TP_ROW (TL_TP_HIST + TL_TP_FRAME)
#define TL_TP_PIECES (TL_TP_FRAME / 8)

struct TlTruePeakRecord { uint32_t frames, overs, peak[2], peak_max[2], sample_max[2]; };      // tlb_truepeak_record
struct TlTruePeakArgs {
    const int16_t *pcm;               // [nframes][nstreams][2][1152], 16-byte aligned
    TlTruePeakRecord *rec, *out;      // out [nstreams]: the call's report, may be NULL
    uint32_t *hist;
    const int16_t *taps;              // [3][12]
    const TlConfig *configs;
    const int32_t *stream_cfg;
    uint32_t ceiling;
    int nstreams, nframes;
};

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the constants and records above and nothing else
struct alignas(16) TlTruePeakLds { uint32_t x[2][TL_TP_ROW / 2]; };  // 4672 bytes per wave

// ---- this header's own primitives: the emulation's half and the device's --------------------------------------------------------
#ifdef TL_EMULATE
TL_FN uint32_t tlh_max_u32(const uint32_t (&v)[64]) { uint32_t m = v[0]; for (int i = 1; i < 64; i++) if (v[i] > m) m = v[i]; return m; }
#define TL_TP_WAVE_MAX(name) tlh_max_u32(name)
// acc + lo(a) lo(b) + hi(a) hi(b), the halves as int16: the plain two-product sum
#define TL_TP_DOT2(a, b, acc) ((acc) + (int32_t)(int16_t)((a) & 0xffffu) * (int32_t)(int16_t)((b) & 0xffffu) + (int32_t)(int16_t)((a) >> 16) * (int32_t)(int16_t)((b) >> 16))
#define TL_TP_LD16(dst, p, q) do { const uint32_t *p_ = (const uint32_t *)(p) + 4 * (q); (dst)[0] = p_[0]; (dst)[1] = p_[1]; (dst)[2] = p_[2]; (dst)[3] = p_[3]; } while (0)
#define TL_TP_ST16(p, q, src) do { uint32_t *p_ = (uint32_t *)(p) + 4 * (q); p_[0] = (src)[0]; p_[1] = (src)[1]; p_[2] = (src)[2]; p_[3] = (src)[3]; } while (0)
#else
TL_FN uint32_t tld_max_u32(uint32_t v) { for (int o = 32; o; o >>= 1) { const uint32_t t = (uint32_t)__shfl_xor((int)v, o, 64); v = t > v ? t : v; } return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
#define TL_TP_WAVE_MAX(name) tld_max_u32(name)
typedef short tl_tp_s16x2 __attribute__((ext_vector_type(2)));
// v_dot2_i32_i16 / v_dot2c_i32_i16 without the clamp: the sum cannot leave 32 bits (the table's bound)
TL_FN int32_t tld_dot2(uint32_t a, uint32_t b, int32_t acc) { return __builtin_amdgcn_sdot2(__builtin_bit_cast(tl_tp_s16x2, a), __builtin_bit_cast(tl_tp_s16x2, b), acc, false); }
#define TL_TP_DOT2(a, b, acc) tld_dot2((a), (b), (acc))
// 16 bytes at once, as a native vector: the compiler takes a struct of four words apart into four loads and, in these units, does not put them together again
typedef uint32_t tl_tp_u32x4 __attribute__((ext_vector_type(4)));
#define TL_TP_LD16(dst, p, q) do { const tl_tp_u32x4 v_ = ((const tl_tp_u32x4 *)(p))[q]; (dst)[0] = v_.x; (dst)[1] = v_.y; (dst)[2] = v_.z; (dst)[3] = v_.w; } while (0)      /* global_load_dwordx4 */
#define TL_TP_ST16(p, q, src) do { tl_tp_u32x4 v_; v_.x = (src)[0]; v_.y = (src)[1]; v_.z = (src)[2]; v_.w = (src)[3]; ((tl_tp_u32x4 *)(p))[q] = v_; } while (0)      /* ds_write_b128 */
#endif
// ---------------------------------------------------------------------------------------------------------------------------------

TL_FN uint32_t tl_tp_abs(int32_t v) { return v < 0 ? 0u - (uint32_t)v : (uint32_t)v; }

// Stream s over the call's frames: the wave's whole work.
TL_FN void tl_truepeak_wave(const TlTruePeakArgs &A, TlTruePeakLds &w, int s)
{
    const int ns = A.nstreams, nch = A.configs[A.stream_cfg[s]].nch, total = A.nframes * nch;
    // the record, uniform over the wave, as scalars (an array indexed by the channel would live in scratch memory); lane 0 writes it back
    uint32_t frames = A.rec[s].frames, overs = A.rec[s].overs, peak0 = A.rec[s].peak[0], peak1 = A.rec[s].peak[1];
    uint32_t pmax0 = A.rec[s].peak_max[0], pmax1 = A.rec[s].peak_max[1], smax0 = A.rec[s].sample_max[0], smax1 = A.rec[s].sample_max[1];
    uint32_t K[3][TL_TP_TAPS / 2];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int i = 0; i < TL_TP_TAPS / 2; i++)
            K[p][i] = ((uint32_t)(uint16_t)A.taps[p * TL_TP_TAPS + 2 * i] << 16) | (uint32_t)(uint16_t)A.taps[p * TL_TP_TAPS + 2 * i + 1];
    PA(uint32_t, g, 12);                                             // the three pieces in flight
    PV(uint32_t, pk); PV(uint32_t, sm0); PV(uint32_t, sm1);
    // piece lane + 64 i of item it = (frame, channel); a one-channel stream's second row is never an item
#define TL_TP_FETCH(it) do { const int f_ = (it) / nch, c_ = (it) - f_ * nch; \
        const int16_t *row_ = A.pcm + (((size_t)f_ * (size_t)ns + (size_t)s) * 2 + (size_t)c_) * TL_TP_FRAME; \
        _Pragma("unroll") for (int i = 0; i < 3; i++) if (lane + 64 * i < TL_TP_PIECES) TL_TP_LD16(L(g) + 4 * i, row_, lane + 64 * i); } while (0)
    TL_LANES_BEGIN
#pragma unroll
        for (int i = 0; i < 12; i++) L(g)[i] = 0u;
        L(sm0) = 0u; L(sm1) = 0u; L(pk) = 0u;
        TL_TP_FETCH(0);
        if (lane < nch * (TL_TP_CARRY / 2)) {                        // the carried samples: row c, dwords 2 .. 7
            const int c = lane / (TL_TP_CARRY / 2), k = lane - c * (TL_TP_CARRY / 2);
            w.x[c][(TL_TP_HIST - TL_TP_CARRY) / 2 + k] = A.hist[((size_t)s * 2 + (size_t)c) * (TL_TP_CARRY / 2) + (size_t)k];
        }
    TL_LANES_END
    for (int it = 0; it < total; it++) {
        const int c = nch == 2 ? it & 1 : 0;
        TL_LANES_BEGIN
#pragma unroll
            for (int i = 0; i < 3; i++) if (lane + 64 * i < TL_TP_PIECES) TL_TP_ST16(&w.x[c][TL_TP_HIST / 2], lane + 64 * i, L(g) + 4 * i);
        TL_LANES_END
        TL_LANES_BEGIN
            if (it + 1 < total) TL_TP_FETCH(it + 1);
            // the lane's window: int16 j of it is x[18 lane - 12 + j], j = 0 .. 29
            uint32_t x[15], u[14];
            const uint32_t *row = &w.x[c][(TL_TP_PER_LANE / 2) * lane + (TL_TP_HIST - TL_TP_CARRY) / 2];
#pragma unroll
            for (int k = 0; k < 15; k++) x[k] = row[k];
#pragma unroll
            for (int k = 0; k < 14; k++) u[k] = (x[k] >> 16) | (x[k + 1] << 16);
            uint32_t vmax = 0u, smax = 0u;
#pragma unroll
            for (int m = 0; m < TL_TP_PER_LANE; m++) {
                // x[n] itself: int16 m + 12 of the window
                const uint32_t d = x[(m + 12) >> 1];
                const uint32_t a = tl_tp_abs((int32_t)(int16_t)(m & 1 ? d >> 16 : d & 0xffffu));
                smax = a > smax ? a : smax;
#pragma unroll
                for (int p = 0; p < 3; p++) {
                    int32_t v = 0;
#pragma unroll
                    for (int i = 0; i < TL_TP_TAPS / 2; i++) {
                        const int j = m + 11 - 2 * i;                // low half: x[n - 2 i - 1], high half: x[n - 2 i]
                        v = TL_TP_DOT2(K[p][i], (j & 1) ? u[j >> 1] : x[j >> 1], v);
                    }
                    const uint32_t av = tl_tp_abs(v);
                    vmax = av > vmax ? av : vmax;
                }
            }
            const uint32_t v0 = smax << 15;                          // phase 0: 32768 |x[n]|
            L(pk) = v0 > vmax ? v0 : vmax;
            if (c) L(sm1) = smax > L(sm1) ? smax : L(sm1);
            else L(sm0) = smax > L(sm0) ? smax : L(sm0);
        TL_LANES_END
        TL_LANES_BEGIN
            // every lane has read its window: the row's last twelve samples become the next frame's history
            if (lane < TL_TP_CARRY / 2) w.x[c][(TL_TP_HIST - TL_TP_CARRY) / 2 + lane] = w.x[c][(TL_TP_ROW - TL_TP_CARRY) / 2 + lane];
        TL_LANES_END
        const uint32_t peak = TL_TP_WAVE_MAX(pk);
        if (c) { peak1 = peak; pmax1 = peak > pmax1 ? peak : pmax1; }
        else { peak0 = peak; pmax0 = peak > pmax0 ? peak : pmax0; }
        if (c == nch - 1) {                                          // behind the frame's last channel
            frames = frames + 1u;
            if (peak0 > A.ceiling || (nch == 2 && peak1 > A.ceiling)) overs = overs + 1u;
        }
    }
#undef TL_TP_FETCH
    const uint32_t s0 = TL_TP_WAVE_MAX(sm0), s1 = TL_TP_WAVE_MAX(sm1);
    smax0 = s0 > smax0 ? s0 : smax0;
    smax1 = s1 > smax1 ? s1 : smax1;
    TL_LANES_BEGIN
        if (lane < nch * (TL_TP_CARRY / 2)) {
            const int c = lane / (TL_TP_CARRY / 2), k = lane - c * (TL_TP_CARRY / 2);
            A.hist[((size_t)s * 2 + (size_t)c) * (TL_TP_CARRY / 2) + (size_t)k] = w.x[c][(TL_TP_HIST - TL_TP_CARRY) / 2 + k];
        }
        if (lane == 0) {
            const TlTruePeakRecord R = {frames, overs, {peak0, peak1}, {pmax0, pmax1}, {smax0, smax1}};
            A.rec[s] = R;
            if (A.out) A.out[s] = R;
        }
    TL_LANES_END
}
#endif
