// mp2_limiter.h -- the device true-peak limiter's body (include/toolame_batch.h, tlb_limiter_*): a look-ahead limiter on the planar PCM
// between the ingest and the encoder, in place.  The reference has none, so the arithmetic is DEFINED in the header, in integers, in six
// steps: detector P[n] (the true-peak meter's per-sample quantity, the channels linked), required gain r[n], hold m[n] = min r[n-63 .. n],
// release e[n] = min(m[n], min(U, e[n-1] + S)), smooth G[n] = (sum of 32 e) >> 19, apply y[n] = sgn x[n-63] (|x[n-63]| G[n] >> 16).
// One wave is one stream, as in mp2_truepeak.h, whose primitives (TL_TP_DOT2, TL_TP_LD16 / ST16, TL_TP_WAVE_MAX) and tap packing this
// header uses: it walks the call's frames in order, lane l takes the TL_TP_PER_LANE = 18 consecutive n = 18 l .. 18 l + 17 of a frame for
// EVERY step, so a step's 18 values stay in the lane's registers (v[] below: P, then r, then m, then e) and only what crosses a lane goes
// through LDS.  tl_limiter_wave is written in the lane macros of mp2_wave.h so that tests/emu/mp2_limiter_emu.cpp runs the same text as
// lane loops; every cross-lane step goes through LDS or one of the wave reductions, nothing here has a device-only form of its own.
//
// The steps across lanes (63 = 3 x 18 + 9, 31 = 18 + 13):
//   hold     lane l writes the SUFFIX minima of its r, sfx[i] = min r[18 l + i .. 18 l + 17] (sfx[0]: the whole lane).  The window of
//            n = 18 l + j is the lane's own prefix up to j, the whole lanes l - 1, l - 2 and, for j <= 8, lane l - 3 whole and lane l - 4
//            from j + 9 on, for j >= 9 lane l - 3 from j - 9 on: five LDS reads and the running prefix minimum per n.
//   release  a (min, +) recurrence, so not a serial one.  Lane l runs it over its 18 m with e = U coming in: a[l], what it would hand on.
//            What really comes in is min(U, min_{j >= 1} a[l - j] + (j - 1) 18 S) with a[-1] = e[-1] of the frame: at most 64 reads of
//            consecutive words (lane l reads a[l - j]: no conflict), left early, wave-uniformly, once (j - 1) 18 S has reached U.  All
//            terms saturate at U, so every sum is below 2^31.  Then the lane runs the recurrence once more with the true value coming in.
//   smooth   the box of 32: e of lane l - 1, the last 13 of lane l - 2, then a running 64-bit sum, one e in and one out per n.
//   The last lanes' values of a frame are the next frame's lanes -4 .. -1 (suffix minima) and -2, -1 (e): kept twice in LDS, read from
//   one copy while the other is written (a lane region has no order among its lanes), and carried from call to call in device memory.
// IDLE PATH, wave-uniform: a frame whose largest P is at or below the ceiling, met with all carried r and e at unity, has G = 65536
// throughout: the output is the input 63 samples late and steps 2 to 5 are skipped.  This is the common frame.  `unity` is kept
// conservatively (the last 72 r and 36 e, whole lanes); a frame that takes the active path needlessly computes the same bytes.
// Required gain: floor(ceiling 2^30 / P) as a double division (ceiling 2^30 and P are exact in a double, the quotient is below 2^30, so the
// truncated result is off by at most one) put right with the exact 64-bit remainder, in the lanes with P > ceiling only.
//
// LDS, per wave 11 152 bytes.  x[c]: channel c's row, TL_LM_HIST = 64 int16 of history, then the frame: row[64 + n] = x[n]; the pieces
// land 16-byte aligned as in the meter.  The detector's lane reads 15 dwords from row dword 9 l + 26 on (x[18 l - 12 ..]), the delay's
// lane the 10 dwords from 9 l on (row int16 18 l + 1 + j = x[18 l + j - 63]); the limited samples are written back over row dwords 9 l ..
// 9 l + 8 (row[n] = y[n]) and leave as 16-byte pieces from row dword 0 on.  BANKS: every one of these is lane stride 9 dwords, 9 is odd,
// so l -> 9 l mod 32 is a permutation of the banks within either group of 32 lanes: conflict-free, by the meter's own arithmetic.
// work[]: a lane's 18 words at 19 l (suffix minima, later e): 19 is odd, the same argument; 18 would put two lanes on every second bank.
// rh / eh: the carried lanes, two copies each.  a[]: a[64 + l], a[63] = e[-1], a[0 .. 62] = U.  This is arithmetic, not measurement.
//
// Device memory, allocated by tlb_limiter_enable alone (720 bytes per stream), all of it zero after a reset -- gains are kept as U - value:
//   rec    TlLimiterRecord [nstreams]             the record as it is reported
//   state  uint32 [nstreams][TL_LM_STATE]         [0, 64): x[-64 .. -1] of either channel; [64, 136): U - suffix minima of lanes -4 .. -1;
//                                                 [136, 172): U - e of lanes -2, -1
//   step   uint32 [nstreams]                      S, from the stream's encoder rate (host)
#pragma once
#include <stdint.h>
#include "mp2_types.h"
#include "mp2_truepeak.h"

#define TL_LM_U (1u << 30)            // unity gain
#define TL_LM_WMIN 64                 // hold: the running minimum's width
#define TL_LM_WBOX 32                 // smooth: the box's width
#define TL_LM_DELAY 63
#define TL_LM_HIST 64                 // int16 ahead of the frame in a row of LDS
#define TL_LM_ROW (TL_LM_HIST + TL_TP_FRAME)
#define TL_LM_LANE 19                 // words between two lanes' 18 in work[] (odd: see BANKS above)
#define TL_LM_STATE (TL_LM_HIST + 4 * TL_TP_PER_LANE + 2 * TL_TP_PER_LANE)

struct TlLimiterRecord { uint32_t frames, limited, samples, red_last, red_max, peak_in, peak_in_max, reserved; };      // tlb_limiter_record
struct TlLimiterArgs {
    int16_t *pcm;                     // [nframes][nstreams][2][1152], 16-byte aligned; limited in place
    TlLimiterRecord *rec, *out;       // out [nstreams]: the call's report, may be NULL
    uint32_t *state;
    const uint32_t *step;
    const int16_t *taps;              // [3][12], the meter's table
    const TlConfig *configs;
    const int32_t *stream_cfg;
    uint32_t ceiling;
    int nstreams, nframes;
};

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the constants and records above and nothing else
struct alignas(16) TlLimiterLds {
    uint32_t x[2][TL_LM_ROW / 2];
    uint32_t work[64 * TL_LM_LANE];
    uint32_t rh[2][4 * TL_LM_LANE];
    uint32_t eh[2][2 * TL_LM_LANE];
    uint32_t a[128];
};

#ifdef TL_EMULATE                     // which way a frame went, for the tests: [0] idle, [1] active
static long tl_emu_lm_paths[2] = {0, 0};
#define TL_LM_DBG_PATH(k) (tl_emu_lm_paths[k]++)
#else
#define TL_LM_DBG_PATH(k) ((void)0)
#endif

TL_FN uint32_t tl_lm_min(uint32_t a, uint32_t b) { return a < b ? a : b; }
TL_FN uint32_t tl_lm_max(uint32_t a, uint32_t b) { return a > b ? a : b; }
// floor(ceiling 2^30 / P) for P > ceiling
TL_FN uint32_t tl_lm_required(uint32_t ceiling, uint32_t P)
{
    const uint64_t num = (uint64_t)ceiling << 30;
    uint32_t q = (uint32_t)((double)num / (double)P);
    int64_t rem = (int64_t)(num - (uint64_t)q * (uint64_t)P);
    if (rem < 0) { q = q - 1u; rem += (int64_t)P; }
    if (rem >= (int64_t)P) q = q + 1u;
    return q;
}

// Stream s over the call's frames: the wave's whole work.
TL_FN void tl_limiter_wave(const TlLimiterArgs &A, TlLimiterLds &w, int s)
{
    const int ns = A.nstreams, nch = A.configs[A.stream_cfg[s]].nch;
    const uint32_t U = TL_LM_U, ceiling = A.ceiling, S = A.step[s];
    const uint32_t c18 = (uint64_t)S * TL_TP_PER_LANE < (uint64_t)U ? S * TL_TP_PER_LANE : U;
    uint32_t *st = A.state + (size_t)s * TL_LM_STATE;
    // the record, uniform over the wave, as scalars; lane 0 writes it back
    uint32_t frames = A.rec[s].frames, limited = A.rec[s].limited, samples = A.rec[s].samples, red_last = A.rec[s].red_last;
    uint32_t red_max = A.rec[s].red_max, peak_in = A.rec[s].peak_in, peak_in_max = A.rec[s].peak_in_max;
    uint32_t K[3][TL_TP_TAPS / 2];
#pragma unroll
    for (int p = 0; p < 3; p++)
#pragma unroll
        for (int i = 0; i < TL_TP_TAPS / 2; i++)
            K[p][i] = ((uint32_t)(uint16_t)A.taps[p * TL_TP_TAPS + 2 * i] << 16) | (uint32_t)(uint16_t)A.taps[p * TL_TP_TAPS + 2 * i + 1];
    PA(uint32_t, g, 24);                                             // the next frame's pieces in flight: three per channel
    PA(uint32_t, v, TL_TP_PER_LANE);                                 // the lane's 18 values of the step at hand: P, r, m, e
    PA(uint32_t, xin, 20);                                           // the lane's delayed samples, ten dwords per channel
    PV(uint32_t, pk); PV(uint32_t, z); PV(int, cnt);
    int rf = 0, ef = 0;                                              // the copies of rh / eh that hold the carried lanes
    // piece lane + 64 i of frame f_'s channel c; a one-channel stream's second row is never touched
#define TL_LM_ROWP(f_, c_) (A.pcm + (((size_t)(f_) * (size_t)ns + (size_t)s) * 2 + (size_t)(c_)) * TL_TP_FRAME)
#define TL_LM_FETCH(f_) do { _Pragma("unroll") for (int c_ = 0; c_ < 2; c_++) if (c_ < nch) { const int16_t *row_ = TL_LM_ROWP(f_, c_); \
        _Pragma("unroll") for (int i = 0; i < 3; i++) if (lane + 64 * i < TL_TP_PIECES) TL_TP_LD16(L(g) + 12 * c_ + 4 * i, row_, lane + 64 * i); } } while (0)
    TL_LANES_BEGIN
#pragma unroll
        for (int i = 0; i < 24; i++) L(g)[i] = 0u;
        TL_LM_FETCH(0);
        if (lane < TL_LM_HIST / 2) {
            w.x[0][lane] = st[lane];
            if (nch == 2) w.x[1][lane] = st[TL_LM_HIST / 2 + lane];
        }
        uint32_t zz = 0u;
        for (int k = lane; k < 4 * TL_TP_PER_LANE; k += 64) {
            const uint32_t d = st[TL_LM_HIST + k];
            zz = tl_lm_max(zz, d);
            w.rh[0][TL_LM_LANE * (k / TL_TP_PER_LANE) + k % TL_TP_PER_LANE] = U - d;
        }
        if (lane < 2 * TL_TP_PER_LANE) {
            const uint32_t d = st[TL_LM_HIST + 4 * TL_TP_PER_LANE + lane];
            zz = tl_lm_max(zz, d);
            w.eh[0][TL_LM_LANE * (lane / TL_TP_PER_LANE) + lane % TL_TP_PER_LANE] = U - d;
        }
        w.a[lane] = lane == 63 ? U - st[TL_LM_STATE - 1] : U;       // a[63]: e[-1]
        L(z) = zz;
    TL_LANES_END
    bool unity = TL_TP_WAVE_MAX(z) == 0u;                            // every carried r and e is U
    for (int f = 0; f < A.nframes; f++) {
        TL_LANES_BEGIN
#pragma unroll
            for (int c = 0; c < 2; c++) if (c < nch)
#pragma unroll
                for (int i = 0; i < 3; i++) if (lane + 64 * i < TL_TP_PIECES) TL_TP_ST16(&w.x[c][TL_LM_HIST / 2], lane + 64 * i, L(g) + 12 * c + 4 * i);
        TL_LANES_END
        TL_LANES_BEGIN                                               // 1. detector: the meter's quantity, the maximum over the channels
            if (f + 1 < A.nframes) TL_LM_FETCH(f + 1);
#pragma unroll
            for (int m = 0; m < TL_TP_PER_LANE; m++) L(v)[m] = 0u;
#pragma unroll
            for (int c = 0; c < 2; c++) if (c < nch) {
                // the lane's window: int16 j of it is x[18 lane - 12 + j], j = 0 .. 29
                uint32_t x[15], u[14];
                const uint32_t *row = &w.x[c][(TL_TP_PER_LANE / 2) * lane + (TL_LM_HIST - TL_TP_CARRY) / 2];
#pragma unroll
                for (int k = 0; k < 15; k++) x[k] = row[k];
#pragma unroll
                for (int k = 0; k < 14; k++) u[k] = (x[k] >> 16) | (x[k + 1] << 16);
#pragma unroll
                for (int m = 0; m < TL_TP_PER_LANE; m++) {
                    const uint32_t d = x[(m + 12) >> 1];
                    uint32_t pm = tl_tp_abs((int32_t)(int16_t)(m & 1 ? d >> 16 : d & 0xffffu)) << 15;
#pragma unroll
                    for (int p = 0; p < 3; p++) {
                        int32_t acc = 0;
#pragma unroll
                        for (int i = 0; i < TL_TP_TAPS / 2; i++) {
                            const int j = m + 11 - 2 * i;            // low half: x[n - 2 i - 1], high half: x[n - 2 i]
                            acc = TL_TP_DOT2(K[p][i], (j & 1) ? u[j >> 1] : x[j >> 1], acc);
                        }
                        pm = tl_lm_max(pm, tl_tp_abs(acc));
                    }
                    L(v)[m] = tl_lm_max(L(v)[m], pm);
                }
            }
            uint32_t top = 0u;
#pragma unroll
            for (int m = 0; m < TL_TP_PER_LANE; m++) top = tl_lm_max(top, L(v)[m]);
            L(pk) = top;
        TL_LANES_END
        const uint32_t peak = TL_TP_WAVE_MAX(pk);
        const bool active = peak > ceiling || !unity;
        bool unity_next = unity;
        TL_LM_DBG_PATH(active ? 1 : 0);
        if (active) {
            TL_LANES_BEGIN                                           // 2. required gain; 3. hold: the lane's suffix minima
#pragma unroll
                for (int m = 0; m < TL_TP_PER_LANE; m++) {
                    const uint32_t P = L(v)[m];
                    uint32_t r = U;
                    if (P > ceiling) r = tl_lm_required(ceiling, P);
                    L(v)[m] = r;
                }
                uint32_t sfx = U;
#pragma unroll
                for (int m = TL_TP_PER_LANE - 1; m >= 0; m--) {
                    sfx = tl_lm_min(sfx, L(v)[m]);
                    w.work[TL_LM_LANE * lane + m] = sfx;
                    if (lane >= 60) w.rh[rf ^ 1][TL_LM_LANE * (lane - 60) + m] = sfx;
                }
                L(z) = lane >= 60 ? U - sfx : 0u;
            TL_LANES_END
            TL_LANES_BEGIN                                           // ... m[n]; 4. release: what the lane would hand on with U coming in
                const uint32_t *r1 = lane >= 1 ? &w.work[TL_LM_LANE * (lane - 1)] : &w.rh[rf][TL_LM_LANE * 3];
                const uint32_t *r2 = lane >= 2 ? &w.work[TL_LM_LANE * (lane - 2)] : &w.rh[rf][TL_LM_LANE * (lane + 2)];
                const uint32_t *r3 = lane >= 3 ? &w.work[TL_LM_LANE * (lane - 3)] : &w.rh[rf][TL_LM_LANE * (lane + 1)];
                const uint32_t *r4 = lane >= 4 ? &w.work[TL_LM_LANE * (lane - 4)] : &w.rh[rf][TL_LM_LANE * lane];
                const uint32_t base = tl_lm_min(r1[0], r2[0]), base3 = tl_lm_min(base, r3[0]);
                uint32_t pre = U, t = U;
#pragma unroll
                for (int j = 0; j < TL_TP_PER_LANE; j++) {
                    pre = tl_lm_min(pre, L(v)[j]);
                    const uint32_t o = j <= 8 ? tl_lm_min(base3, r4[j + 9]) : tl_lm_min(base, r3[j - 9]);
                    const uint32_t mj = tl_lm_min(pre, o);
                    L(v)[j] = mj;
                    t = tl_lm_min(mj, tl_lm_min(U, t + S));
                }
                w.a[64 + lane] = t;
            TL_LANES_END
            TL_LANES_BEGIN                                           // ... what comes in, then the lane's e
                uint32_t e = U, d = 0u;
                for (int j = 1; j <= 64; j++) {
                    e = tl_lm_min(e, w.a[64 + lane - j] + d);
                    d = tl_lm_min(U, d + c18);
                    if (d >= U) break;                               // (uniform: every further term is U or more)
                }
                uint32_t low = U;
#pragma unroll
                for (int j = 0; j < TL_TP_PER_LANE; j++) {
                    e = tl_lm_min(L(v)[j], tl_lm_min(U, e + S));
                    L(v)[j] = e;
                    low = tl_lm_min(low, e);
                    w.work[TL_LM_LANE * lane + j] = e;
                    if (lane >= 62) w.eh[ef ^ 1][TL_LM_LANE * (lane - 62) + j] = e;
                }
                if (lane >= 62) L(z) = tl_lm_max(L(z), U - low);
            TL_LANES_END
            unity_next = TL_TP_WAVE_MAX(z) == 0u;
        }
        TL_LANES_BEGIN                                               // the delayed samples, before the row is written over
#pragma unroll
            for (int c = 0; c < 2; c++) if (c < nch)
#pragma unroll
                for (int k = 0; k < 10; k++) L(xin)[10 * c + k] = w.x[c][(TL_TP_PER_LANE / 2) * lane + k];
            if (active && lane == 63) w.a[63] = L(v)[TL_TP_PER_LANE - 1];
        TL_LANES_END
        TL_LANES_BEGIN                                               // 5. smooth; 6. apply
            uint32_t G[TL_TP_PER_LANE], red = 0u;
            int below = 0;
            if (active) {
                const uint32_t *e1 = lane >= 1 ? &w.work[TL_LM_LANE * (lane - 1)] : &w.eh[ef][TL_LM_LANE];
                const uint32_t *e2 = lane >= 2 ? &w.work[TL_LM_LANE * (lane - 2)] : &w.eh[ef][TL_LM_LANE * lane];
                uint64_t sum = 0u;
#pragma unroll
                for (int i = 5; i < TL_TP_PER_LANE; i++) sum += e2[i];
#pragma unroll
                for (int i = 0; i < TL_TP_PER_LANE; i++) sum += e1[i];
#pragma unroll
                for (int j = 0; j < TL_TP_PER_LANE; j++) {
                    sum += L(v)[j];
                    if (j) sum -= j <= 13 ? e2[j + 4] : e1[j - 14];
                    G[j] = (uint32_t)(sum >> 19);
                    red = tl_lm_max(red, 65536u - G[j]);
                    below += G[j] < 65536u ? 1 : 0;
                }
            } else {
#pragma unroll
                for (int j = 0; j < TL_TP_PER_LANE; j++) G[j] = 65536u;
            }
#pragma unroll
            for (int c = 0; c < 2; c++) if (c < nch) {
                uint32_t y[TL_TP_PER_LANE / 2];
#pragma unroll
                for (int j = 0; j < TL_TP_PER_LANE; j++) {
                    const uint32_t d = L(xin)[10 * c + ((j + 1) >> 1)];
                    const int32_t xs = (int32_t)(int16_t)((j + 1) & 1 ? d >> 16 : d & 0xffffu);
                    const uint32_t q = (tl_tp_abs(xs) * G[j]) >> 16;
                    const uint32_t h = (xs < 0 ? 0u - q : q) & 0xffffu;
                    if (j & 1) y[j >> 1] |= h << 16; else y[j >> 1] = h;
                }
#pragma unroll
                for (int k = 0; k < TL_TP_PER_LANE / 2; k++) w.x[c][(TL_TP_PER_LANE / 2) * lane + k] = y[k];
            }
            L(z) = red; L(cnt) = below;
        TL_LANES_END
        TL_LANES_BEGIN                                               // the limited frame back to where it came from, in 16-byte pieces
#pragma unroll
            for (int c = 0; c < 2; c++) if (c < nch) {
                int16_t *row_ = TL_LM_ROWP(f, c);
#pragma unroll
                for (int i = 0; i < 3; i++) if (lane + 64 * i < TL_TP_PIECES) {
                    uint32_t t4[4];
                    TL_TP_LD16(t4, &w.x[c][0], lane + 64 * i);
                    TL_TP_ST16(row_, lane + 64 * i, t4);
                }
            }
        TL_LANES_END
        TL_LANES_BEGIN                                               // the frame's last 64 samples, as they came in, become the next frame's history
            if (lane < TL_LM_HIST / 2) {
                w.x[0][lane] = w.x[0][TL_TP_FRAME / 2 + lane];
                if (nch == 2) w.x[1][lane] = w.x[1][TL_TP_FRAME / 2 + lane];
            }
        TL_LANES_END
        frames = frames + 1u;
        peak_in = peak;
        peak_in_max = tl_lm_max(peak_in_max, peak);
        red_last = 0u;
        if (active) {
            red_last = TL_TP_WAVE_MAX(z);
            const uint32_t n = (uint32_t)TL_WAVE_SUM_I32(cnt);
            if (n) limited = limited + 1u;
            samples = samples + n < samples ? 0xffffffffu : samples + n;
            red_max = tl_lm_max(red_max, red_last);
            unity = unity_next;
            rf ^= 1; ef ^= 1;
        }
    }
#undef TL_LM_FETCH
#undef TL_LM_ROWP
    TL_LANES_BEGIN
        if (lane < TL_LM_HIST / 2) {
            st[lane] = w.x[0][lane];
            if (nch == 2) st[TL_LM_HIST / 2 + lane] = w.x[1][lane];
        }
        for (int k = lane; k < 4 * TL_TP_PER_LANE; k += 64) st[TL_LM_HIST + k] = U - w.rh[rf][TL_LM_LANE * (k / TL_TP_PER_LANE) + k % TL_TP_PER_LANE];
        if (lane < 2 * TL_TP_PER_LANE) st[TL_LM_HIST + 4 * TL_TP_PER_LANE + lane] = U - w.eh[ef][TL_LM_LANE * (lane / TL_TP_PER_LANE) + lane % TL_TP_PER_LANE];
        if (lane == 0) {
            const TlLimiterRecord R = {frames, limited, samples, red_last, red_max, peak_in, peak_in_max, 0u};
            A.rec[s] = R;
            if (A.out) A.out[s] = R;
        }
    TL_LANES_END
}
#endif
