// mp2_feed_adapt.h -- ADAPTED Layer II feeds (include/toolame_batch.h, tlb_feed_set_adapted): a feed at another sample rate or channel
// count than its stream's.  The feed decoder (mp2_feed.h) and the integer resampler (mp2_resample.h) are used as they are; what is here
// is the thing between them: the schedule that says on which ticks a feed frame is wanted, a per-stream queue of decoded source frames
// on the device, and the channel map.
//   tick f of a stream (counted from its last reset) consumes the source frames [S(f), S(f + 1)) and reads back to S(f) - 31;
//   K(f) feed frames must have arrived by tick f; the slot of tick f is WANTED when K(f) > K(f - 1).
// Everything repeats after tl_fa_cycle ticks (160 ticks = 147 feed frames for 160/147; 3 ticks = 2 frames for 3/2), so a stream's position
// is its tick counter modulo the cycle and all that the kernels compute from it are DIFFERENCES of S and K, which the modulus leaves alone.
// Three kernels per call, in this order on one stream (toolame_feed_adapt.hip):
//   decode    one wavefront per (tick, stream): the feed decode itself (mp2_feed.h: tl_feed_decode) for a wanted slot of an adapted
//             stream, into row K(p) - 1 - K(p0 - 1) of the stream's part of the call's source plane (p0: the position at the call's start,
//             p = p0 + f); the slot before is the previous WANTED one: tick f - 1 or f - 2 of the call, or the carried bytes
//   resample  one workgroup of TL_RS_WAVES waves per (tick, stream): the ratio's table and the source frames [S(p) - 31, S(p + 1)) into LDS
//             -- from the stream's carried head for frames before the call's first decoded one, from the plane for the rest, the stereo to
//             mono map applied on the way --, one barrier, tl_resample_wave unchanged
//   carry     one wavefront per stream: the last TL_FA_CARRY source frames before the next call's first decoded one (into the OTHER copy:
//             a call with one tick keeps most of what it was given), the new position, and tl_feed_keep of the last wanted slot
// TL_FA_CARRY: before any tick at most 1145 decoded frames are unconsumed and a tick reads 31 frames of history: 1176, rounded to 1184 so
// that a one-channel stream's copy is a multiple of 16 bytes.  Lane-SPMD source for gfx950 and, with TL_EMULATE, lane loops; include after
// mp2_feed.h with TL_FA_BODY defined (toolame_feed_adapt.hip and the emulation: the one kernel unit and the one test that want the body; tl_kernels.h
// brings the part above it to every unit).
#pragma once
#include <stdint.h>
#include "mp2_dec_types.h"
#include "mp2_resample.h"

#define TL_DEC_UNWANTED 0x100u        // an adapted feed's slot held bytes on a tick whose slot is not read (TLB_DEC_UNWANTED); not in TL_DEC_BAD_MASK
#define TL_FA_CARRY 1184
#define tl_fa_cycle(ratio) ((ratio) == TL_RS_160_147 ? 160 : (ratio) == TL_RS_3_2 ? 3 : 1)
// the ratio of a legal (feed rate, stream rate) pair: TL_RS_OFF for equal rates; -1: none
static inline int tl_fa_ratio_of(long feed, long enc) { return feed == enc ? TL_RS_OFF : tl_rs_ratio_of(feed, enc) != TL_RS_OFF ? tl_rs_ratio_of(feed, enc) : -1; }

// ratio: TL_RS_160_147, TL_RS_3_2 or TL_RS_OFF (here: 1/1).  constexpr: host and device.  32-bit arithmetic: f is a position in the
// cycle plus a tick of one call, and a call with adapted feeds has at most TL_FA_MAX_FRAMES ticks ((1152 f - 1) 147 < 2^31 up to f = 12 680).
#define TL_FA_MAX_FRAMES 8192
// source frames consumed before tick f: f > 0 ? q(1152 f - 1) + 1 : 0
static constexpr int tl_fa_S(int f, int ratio)
{
    return ratio == TL_RS_160_147 ? (f > 0 ? (int)((unsigned)(1152 * f - 1) * 147u / 160u) + 1 : 0) : ratio == TL_RS_3_2 ? 768 * f : 1152 * f;
}
// feed frames that must have arrived by tick f; K(-1) = 0
static constexpr int tl_fa_K(int f, int ratio) { return f < 0 ? 0 : (int)((unsigned)(tl_fa_S(f + 1, ratio) + 1151) / 1152u); }
static constexpr int tl_fa_want(int f, int ratio) { return tl_fa_K(f, ratio) - tl_fa_K(f - 1, ratio); }

// One call of the adapted path.  F is the strict path's record with F.feed_cfg naming the ADAPTED streams' feed records (-1: the stream
// is not adapted: a strict feed or none) and F.state / F.prev the same history buffers (a stream is in one of the two tables only).
struct TlFeedAdaptLaunch {
    TlFeedLaunch F;
    const int32_t *ratio;             // [nstreams] TL_RS_* of (feed rate, stream rate); read for adapted streams only
    const TlConfig *sconfigs;         // the STREAMS' records and table: the channel count the ingest reads
    const int32_t *stream_cfg;
    const int16_t *taps;              // both tables: [160][32], then [3][32]
    int16_t *plane;                   // [nstreams][nframes * 2304]: a stream's decoded source frames of this call, in the feed's channel layout
    int16_t *carry;                   // [2][nstreams][TL_FA_CARRY * 2]: copy `flip` is read, the other written
    int32_t *pos;                     // [2][nstreams] tick counter modulo the cycle, likewise
    int32_t flip;
    int32_t strict_ran;               // the strict kernel ran before and has reported every stream that is not adapted
};

#ifdef TL_FA_BODY
TL_FN const int16_t *tl_fa_carry_of(const TlFeedAdaptLaunch &A, int copy, int s) { return A.carry + ((size_t)copy * (size_t)A.F.nstreams + (size_t)s) * (TL_FA_CARRY * 2); }
TL_FN const int16_t *tl_fa_plane_of(const TlFeedAdaptLaunch &A, int s) { return A.plane + (size_t)s * (size_t)A.F.nframes * 2304; }

// source frame `g` of a stream, counted from the call's first decoded frame: below 0 in the carried head `cin`, else in the plane `pl`
TL_FN const int16_t *tl_fa_frame(const int16_t *TL_RESTRICT cin, const int16_t *TL_RESTRICT pl, int g, int fch) { return g < 0 ? cin + (TL_FA_CARRY + g) * fch : pl + g * fch; }

// ---- decode: slot f of stream s -> its report and, for a wanted slot, 1152 source frames in the stream's plane.  What is here is the
// schedule; the decode is tl_feed_decode. ----
TL_FN void tl_fa_decode_unit(TlSynthLds &w, const TlFeedAdaptLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const TlFeedLaunch &F = A.F;
    const size_t slot = (size_t)f * F.nstreams + s;
    TlFrameReport *rep = &F.report[slot];
    const int ci = F.feed_cfg[s];
    if (ci < 0) { if (!A.strict_ran) tl_dec_report(rep, TL_DEC_EMPTY, nullptr); return; }
    const int ratio = TL_UNI_I(A.ratio[s]);                          // (uniform over the wave, and kept in scalar registers)
    const int p0 = TL_UNI_I(A.pos[(size_t)A.flip * (size_t)F.nstreams + (size_t)s]), p = p0 + f;
    if (!tl_fa_want(p, ratio)) { tl_dec_report(rep, F.len[slot] > 0 ? TL_DEC_EMPTY | TL_DEC_UNWANTED : TL_DEC_EMPTY, nullptr); return; }
    const TlConfig *C = &F.configs[ci];
    const int row = TL_UNI_I(tl_fa_K(p, ratio) - 1 - tl_fa_K(p0 - 1, ratio));    // 0 .. f
    int16_t *out = (int16_t *)tl_fa_plane_of(A, s) + TL_UNI_I(row * 1152 * C->nch);        // (32 bits: at most TL_FA_MAX_FRAMES rows)
    int pf = f - 1;                                                  // the WANTED slot before: never more than one unwanted tick lies between two wanted ones
    if (pf >= 0 && !tl_fa_want(p - 1, ratio)) pf--;
    pf = TL_UNI_I(pf);                                               // (-1 = TL_FEED_CARRIED: the call has no wanted slot before this one)
    tl_feed_decode(w, F, C, s, f, pf, out, dwin);
}

// ---- resample: what is uniform over the workgroup of slot (f, s) ----
struct TlFaSlot {
    int ratio;                        // -1: the stream is not adapted (the workgroup has nothing to do)
    int fch, sch;                     // channels of the feed and of the stream
    int pos5, need;                   // the resampler's frame position in its need cycle; source frames the tick consumes
    int rel;                          // source frame S(p) - 31 counted from the call's first decoded frame: -TL_FA_CARRY + 8 .. ; below 0: in the carried head
};
TL_FN TlFaSlot tl_fa_slot(const TlFeedAdaptLaunch &A, int s, int f)
{
    TlFaSlot S;
    const int ci = A.F.feed_cfg[s];
    S.ratio = -1; S.fch = S.sch = 1; S.pos5 = 0; S.need = 0; S.rel = 0;
    if (ci < 0) return S;
    S.ratio = A.ratio[s];
    S.fch = A.F.configs[ci].nch; S.sch = A.sconfigs[A.stream_cfg[s]].nch;
    const int p0 = A.pos[(size_t)A.flip * (size_t)A.F.nstreams + (size_t)s], p = p0 + f;
    S.need = tl_fa_S(p + 1, S.ratio) - tl_fa_S(p, S.ratio);
    S.rel = tl_fa_S(p, S.ratio) - TL_RS_HIST - tl_fa_K(p0 - 1, S.ratio) * 1152;
    S.pos5 = p % tl_rs_cycle(S.ratio);
    return S;
}
// source frame `g` (counted from the call's first decoded frame) under the channel map: L | R << 16 for two channels to two, else one sample
TL_FN uint32_t tl_fa_source(const int16_t *TL_RESTRICT cin, const int16_t *TL_RESTRICT pl, int g, int fch, int sch)
{
    const int16_t *p = tl_fa_frame(cin, pl, g, fch);
    if (fch == 1) return (uint32_t)(uint16_t)p[0];
    const uint32_t u = *(const uint32_t *)p;
    if (sch == 2) return u;
    const int32_t l = (int16_t)(u & 0xffffu), r = (int16_t)(u >> 16);
    return (uint32_t)(uint16_t)(int16_t)((l + r + 1) >> 1);
}
// one wave's share of the fill, as tl_resample_fill: the ratio's table, then x[0 .. 31 + need)
TL_FN void tl_fa_fill(const TlFeedAdaptLaunch &A, TlResampleLds &w, const TlFaSlot &S, int s, int wave)
{
    const int L = S.ratio == TL_RS_160_147 ? 160 : 3;
    const TlRsVec *tg = (const TlRsVec *)(A.taps + (S.ratio == TL_RS_160_147 ? 0 : TL_RS_MAXL * TL_RS_TAPS));
    TlRsVec *tl = (TlRsVec *)w.tab;
    int16_t *x16 = (int16_t *)w.x;
    const int16_t *cin = tl_fa_carry_of(A, A.flip, s), *pl = tl_fa_plane_of(A, s);
    const bool pairs = S.fch == 2 && S.sch == 2;
    TL_LANES_BEGIN
        for (int k = wave * 64 + lane; k < 4 * L; k += 64 * TL_RS_WAVES) tl[(k >> 2) * (TL_RS_ROW / 8) + (k & 3)] = tg[k];
        for (int j = wave * 64 + lane; j < TL_RS_HIST + S.need; j += 64 * TL_RS_WAVES) {
            const uint32_t v = tl_fa_source(cin, pl, S.rel + j, S.fch, S.sch);
            if (pairs) w.x[j] = v; else x16[j] = (int16_t)v;
        }
    TL_LANES_END
}
// after the barrier: the 1152 outputs.  A one-channel feed for a two-channel stream is resampled once into `y` (LDS) and written to both
// channels by tl_fa_dup after one more barrier.
TL_FN void tl_fa_wave(const TlFeedAdaptLaunch &A, const TlResampleLds &w, const TlFaSlot &S, int16_t *y, int s, int f, int wave)
{
    int16_t *dst = A.F.pcm + ((size_t)f * (size_t)A.F.nstreams + (size_t)s) * 2304;
    const bool dup = S.fch == 1 && S.sch == 2;
    tl_resample_wave(dup ? y : dst, nullptr, w, S.fch == 2 && S.sch == 2 ? 2 : 1, S.ratio, S.pos5, S.need, 0, wave);
}
TL_FN void tl_fa_dup(const TlFeedAdaptLaunch &A, const int16_t *y, int s, int f, int wave)
{
    uint32_t *dst = (uint32_t *)(A.F.pcm + ((size_t)f * (size_t)A.F.nstreams + (size_t)s) * 2304);
    TL_LANES_BEGIN
        for (int i = wave * 64 + lane; i < TL_RS_FRAME; i += 64 * TL_RS_WAVES) { const uint32_t v = (uint16_t)y[i]; dst[i] = v | (v << 16); }
    TL_LANES_END
}
// ratio 1/1: the tick's 1152 source frames under the channel map, no LDS
TL_FN void tl_fa_copy(const TlFeedAdaptLaunch &A, const TlFaSlot &S, int s, int f, int wave)
{
    int16_t *dst = A.F.pcm + ((size_t)f * (size_t)A.F.nstreams + (size_t)s) * 2304;
    const int16_t *cin = tl_fa_carry_of(A, A.flip, s), *pl = tl_fa_plane_of(A, s);
    TL_LANES_BEGIN
        for (int i = wave * 64 + lane; i < TL_RS_FRAME; i += 64 * TL_RS_WAVES) {
            const uint32_t v = tl_fa_source(cin, pl, S.rel + TL_RS_HIST + i, S.fch, S.sch);
            if (S.sch == 2) ((uint32_t *)dst)[i] = S.fch == 2 ? v : v | (v << 16);
            else dst[i] = (int16_t)v;
        }
    TL_LANES_END
}

// ---- carry: what the next call needs of stream s (after every unit of this call is done) ----
TL_FN void tl_fa_carry(const TlFeedAdaptLaunch &A, int s)
{
    const TlFeedLaunch &F = A.F;
    const int ci = F.feed_cfg[s];
    if (ci < 0) return;
    const int ratio = A.ratio[s], fch = F.configs[ci].nch;
    const int p0 = A.pos[(size_t)A.flip * (size_t)F.nstreams + (size_t)s];
    const int rows = tl_fa_K(p0 + F.nframes - 1, ratio) - tl_fa_K(p0 - 1, ratio);      // decoded in this call
    const int first = rows * 1152 - TL_FA_CARRY;               // the new head's first frame, counted from the call's first decoded frame
    const int16_t *cin = tl_fa_carry_of(A, A.flip, s), *pl = tl_fa_plane_of(A, s);
    int16_t *cout = (int16_t *)tl_fa_carry_of(A, A.flip ^ 1, s);
    int lf = F.nframes - 1;                                          // the call's last wanted slot; -1: it had none (one unwanted tick)
    if (!tl_fa_want(p0 + lf, ratio)) lf--;
    if (lf >= 0) tl_feed_keep(F, s, (size_t)lf * F.nstreams + s);
    TL_LANES_BEGIN
    if (ratio != TL_RS_OFF)                                          // (1/1 reads nothing before its own tick)
        for (int j = lane; j < TL_FA_CARRY; j += 64) {
            const int16_t *p = tl_fa_frame(cin, pl, first + j, fch);
            if (fch == 2) ((uint32_t *)cout)[j] = *(const uint32_t *)p; else cout[j] = p[0];
        }
    if (lane == 0) A.pos[(size_t)(A.flip ^ 1) * (size_t)F.nstreams + (size_t)s] = (p0 + F.nframes) % tl_fa_cycle(ratio);
    TL_LANES_END
}
#endif
