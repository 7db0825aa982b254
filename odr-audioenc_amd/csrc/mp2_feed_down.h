// mp2_feed_down.h -- DOWN FEEDS (include/toolame_batch.h, tlb_feed_down_*): a 48, 44.1 or 32 kHz Layer II feed for a 24 kHz stream.  The
// feed decoder (mp2_feed.h: tl_feed_decode) and the integer decimator (mp2_decimate.h: tl_decimate_outputs) are used as they are; what is
// here is the thing between them, as mp2_feed_adapt.h is between the decoder and the resampler: the schedule, which asks for ONE OR TWO
// feed frames per tick, a per-stream queue of decoded source frames on the device, and the channel map.
//   tick f of a stream (counted from its last reset) consumes the source frames [S(f), S(f + 1)), S(f) = ceil(1152 f M / L) (the
//   decimator's own), and reads back to S(f) - 63;  K(f) = ceil(S(f + 1) / 1152) feed frames must have arrived by tick f, K(-1) = 0;
//   want(f) = K(f) - K(f - 1) is 1 or 2: a tick has TWO slots per stream, and slot 1 is read on a tick that wants two.
// Everything repeats after tl_fd_cycle ticks (1/2: every tick; 3/4: 3 ticks = 4 feed frames; 80/147: 80 ticks = 147 feed frames), so a
// stream's position is its tick counter modulo the cycle, and what the kernels compute from it are DIFFERENCES of S and K.  The cycle of
// 80/147 is a multiple of the decimator's need cycle of five, so the decimator's own position is the tick's modulo 5.
// Three kernels per call, in this order on one stream (toolame_feed_down.hip):
//   decode    one wavefront per (tick, stream, slot j): tl_feed_decode of a wanted slot into row K(p - 1) - K(p0 - 1) + j of the stream's
//             part of the call's source plane (p0: the position at the call's start, p = p0 + f).  The slot before slot 1 is slot 0 of the
//             same tick; before slot 0 it is the last wanted slot of the tick before, or the carried bytes
//   decimate  one workgroup of TL_DC_WAVES waves per (tick, stream): the ratio's table and the source frames [S(p) - 63, S(p + 1)) into
//             TlDecimateLds -- from the stream's carried head for frames before the call's first decoded one, from the plane for the rest,
//             the two-to-one map applied on the way --, one barrier, tl_decimate_outputs unchanged
//   carry     one wavefront per stream: the last TL_FD_CARRY source frames before the next call's first decoded one (into the OTHER copy),
//             the new position, and tl_feed_keep of the last wanted slot
// TL_FD_CARRY: before any tick at most 1137 decoded frames are unconsumed (80/147; 768 for 3/4, 0 for 1/2) and a tick reads 63 frames of
// history: 1200, a multiple of 8, so a one-channel stream's copy is a multiple of 16 bytes.
// The decoder's slot arithmetic (slot = f * nstreams + s) is met with a view of the launch that has ONE stream: slot (f, s, j) of
// [nframes][nstreams][2] is "frame" (f * nstreams + s) * 2 + j of that view, whose history buffers start at the stream's own records.
// Lane-SPMD source for gfx950 and, with TL_EMULATE, lane loops; include after mp2_feed.h and mp2_decimate.h with TL_FD_BODY defined
// (toolame_feed_down.hip and tests/emu/mp2_feed_down_emu.cpp; tl_kernels.h brings the part above the body to every unit).
#pragma once
#include <stdint.h>
#include "mp2_dec_types.h"
#include "mp2_decimate.h"
#include "mp2_feed_adapt.h"      // TL_DEC_UNWANTED

#define TL_FD_CARRY 1200
#define TL_FD_PREV_STRIDE 1728        // bytes per stream of the history slot: the longest Layer II frame there is (384 kbps at 32 kHz)
#define TL_FD_MAX_FRAMES 8192         // ticks per call: 1152 (79 + 8192 + 1) 147 + 79 < 2^31, 32-bit arithmetic throughout
#define TL_FD_PLANE (2 * 2304)        // int16 per stream and tick of the source plane: two feed frames of two channels
#define tl_fd_cycle(ratio) ((ratio) == TL_DC_80_147 ? 80 : (ratio) == TL_DC_3_4 ? 3 : 1)
// the ratio of a legal (feed rate, stream rate) pair: the decimator's three; TL_DC_OFF: none
static inline int tl_fd_ratio_of(long feed, long enc) { return tl_dc_ratio_of(feed, enc); }

// ratio: TL_DC_80_147, TL_DC_3_4 or TL_DC_1_2.  constexpr: host and device.  f: a position in the cycle plus a tick of one call.
// source frames consumed before tick f
static constexpr int tl_fd_S(int f, int ratio)
{
    return ratio == TL_DC_80_147 ? (int)(((unsigned)(1152 * f) * 147u + 79u) / 80u) : ratio == TL_DC_3_4 ? 1536 * f : 2304 * f;
}
// feed frames that must have arrived by tick f; K(-1) = 0
static constexpr int tl_fd_K(int f, int ratio) { return f < 0 ? 0 : (int)((unsigned)(tl_fd_S(f + 1, ratio) + 1151) / 1152u); }
static constexpr int tl_fd_want(int f, int ratio) { return tl_fd_K(f, ratio) - tl_fd_K(f - 1, ratio); }

// One call of the down-feed path.  F is the feed launch record (mp2_dec_types.h) with F.feed_cfg naming the streams' DOWN-feed records
// (-1: the stream has no down feed), F.frames / F.len / F.report with TWO slots per (tick, stream) and F.state / F.prev the down feeds'
// own history buffers.
struct TlFeedDownLaunch {
    TlFeedLaunch F;                   // frames [nframes][nstreams][2][stride], len and report [nframes][nstreams][2]
    const int32_t *ratio;             // [nstreams] TL_DC_* of (feed rate, stream rate); read for streams with a down feed only
    const TlConfig *sconfigs;         // the STREAMS' records and table: the channel count the ingest reads
    const int32_t *stream_cfg;
    const int16_t *taps;              // the decimator's three tables: [80][64], [3][64], [1][64]
    int16_t *plane;                   // [nstreams][nframes * TL_FD_PLANE]: a stream's decoded source frames of this call, in the feed's channel layout
    int16_t *carry;                   // [2][nstreams][TL_FD_CARRY * 2]: copy `flip` is read, the other written
    int32_t *pos;                     // [2][nstreams] tick counter modulo the cycle, likewise
    int32_t flip;
};

#ifdef TL_FD_BODY
TL_FN const int16_t *tl_fd_carry_of(const TlFeedDownLaunch &A, int copy, int s) { return A.carry + ((size_t)copy * (size_t)A.F.nstreams + (size_t)s) * (TL_FD_CARRY * 2); }
TL_FN const int16_t *tl_fd_plane_of(const TlFeedDownLaunch &A, int s) { return A.plane + (size_t)s * (size_t)A.F.nframes * TL_FD_PLANE; }
// source frame `g` of a stream, counted from the call's first decoded frame: below 0 in the carried head `cin`, else in the plane `pl`
TL_FN const int16_t *tl_fd_frame(const int16_t *TL_RESTRICT cin, const int16_t *TL_RESTRICT pl, int g, int fch) { return g < 0 ? cin + (TL_FD_CARRY + g) * fch : pl + g * fch; }

// the launch as tl_feed_decode and tl_feed_keep see it for stream s: one stream, the slots of the whole call as its "frames"
TL_FN TlFeedLaunch tl_fd_view(const TlFeedLaunch &F, int s)
{
    TlFeedLaunch V = F;
    V.state = F.state + s; V.prev = F.prev + (size_t)s * (size_t)F.prev_stride;
    V.nstreams = 1;
    return V;
}
TL_FN int tl_fd_slot(const TlFeedLaunch &F, int s, int f, int j) { return (f * F.nstreams + s) * 2 + j; }      // (32 bits: the host refuses calls beyond 2^29 (tick, stream) pairs)

// ---- decode: slot j of tick f of stream s -> its report and, for a wanted slot, 1152 source frames in the stream's plane ----
TL_FN void tl_fd_decode_unit(TlSynthLds &w, const TlFeedDownLaunch &A, int s, int f, int j, const double *TL_RESTRICT dwin)
{
    const TlFeedLaunch &F = A.F;
    const int slot = tl_fd_slot(F, s, f, j);
    TlFrameReport *rep = &F.report[slot];
    const int ci = F.feed_cfg[s];
    if (ci < 0) { tl_dec_report(rep, TL_DEC_EMPTY, nullptr); return; }
    const int ratio = TL_UNI_I(A.ratio[s]);                          // (uniform over the wave, and kept in scalar registers)
    const int p0 = TL_UNI_I(A.pos[(size_t)A.flip * (size_t)F.nstreams + (size_t)s]), p = p0 + f;
    if (j >= tl_fd_want(p, ratio)) { tl_dec_report(rep, F.len[slot] > 0 ? TL_DEC_EMPTY | TL_DEC_UNWANTED : TL_DEC_EMPTY, nullptr); return; }
    const TlConfig *C = &F.configs[ci];
    const int row = TL_UNI_I(tl_fd_K(p - 1, ratio) - tl_fd_K(p0 - 1, ratio) + j);      // 0 .. 2 f + 1
    int16_t *out = (int16_t *)tl_fd_plane_of(A, s) + TL_UNI_I(row * 1152 * C->nch);
    // the WANTED slot before: slot 0 of this tick, the last wanted slot of the tick before, or TL_FEED_CARRIED
    int pf = j ? slot - 1 : f > 0 ? tl_fd_slot(F, s, f - 1, tl_fd_want(p - 1, ratio) - 1) : TL_FEED_CARRIED;
    pf = TL_UNI_I(pf);
    const TlFeedLaunch V = tl_fd_view(F, s);
    tl_feed_decode(w, V, C, 0, slot, pf, out, dwin);
}

// ---- decimate: what is uniform over the workgroup of tick f of stream s ----
struct TlFdSlot {
    int ratio;                        // TL_DC_OFF: the stream has no down feed (the workgroup has nothing to do)
    int fch, sch;                     // channels of the feed and of the stream
    int pos5, need;                   // the decimator's frame position in its need cycle; source frames the tick consumes
    int rel;                          // source frame S(p) - 63 counted from the call's first decoded frame: -TL_FD_CARRY .. ; below 0: in the carried head
};
TL_FN TlFdSlot tl_fd_slot_of(const TlFeedDownLaunch &A, int s, int f)
{
    TlFdSlot S;
    const int ci = A.F.feed_cfg[s];
    S.ratio = TL_DC_OFF; S.fch = S.sch = 1; S.pos5 = 0; S.need = 0; S.rel = 0;
    if (ci < 0) return S;
    const int ratio = A.ratio[s];
    if (ratio < TL_DC_80_147 || ratio > TL_DC_1_2) return S;
    S.ratio = ratio;
    S.fch = A.F.configs[ci].nch; S.sch = A.sconfigs[A.stream_cfg[s]].nch;
    const int p0 = A.pos[(size_t)A.flip * (size_t)A.F.nstreams + (size_t)s], p = p0 + f;
    S.need = tl_fd_S(p + 1, ratio) - tl_fd_S(p, ratio);
    S.rel = tl_fd_S(p, ratio) - TL_DC_HIST - tl_fd_K(p0 - 1, ratio) * 1152;
    S.pos5 = p % tl_dc_cycle(ratio);
    return S;
}
// source frame `g` under the channel map: L | R << 16 for two channels to two, else one sample
TL_FN uint32_t tl_fd_source(const int16_t *TL_RESTRICT cin, const int16_t *TL_RESTRICT pl, int g, int fch, int sch)
{
    const int16_t *p = tl_fd_frame(cin, pl, g, fch);
    if (fch == 1) return (uint32_t)(uint16_t)p[0];
    const uint32_t u = *(const uint32_t *)p;
    if (sch == 2) return u;
    const int32_t l = (int16_t)(u & 0xffffu), r = (int16_t)(u >> 16);
    return (uint32_t)(uint16_t)(int16_t)((l + r + 1) >> 1);
}
// one wave's share of the fill, into the layout tl_decimate_fill makes: the ratio's table at TL_DC_ROW, then the source frames
// [S - 63, S + need) at x[TL_DC_AT - 63 ..] (x[0] is the padding word)
TL_FN void tl_fd_fill(const TlFeedDownLaunch &A, TlDecimateLds &w, const TlFdSlot &S, int s, int wave)
{
    const int L = tl_dc_L(S.ratio);
    const TlDcVec *tg = (const TlDcVec *)(A.taps + tl_dc_first_row(S.ratio) * TL_DC_TAPS);
    TlDcVec *tl = (TlDcVec *)w.tab;
    int16_t *x16 = (int16_t *)w.x;
    const int16_t *cin = tl_fd_carry_of(A, A.flip, s), *pl = tl_fd_plane_of(A, s);
    const bool pairs = S.fch == 2 && S.sch == 2;
    TL_LANES_BEGIN
        for (int k = wave * 64 + lane; k < 8 * L; k += 64 * TL_DC_WAVES) tl[(k >> 3) * (TL_DC_ROW / 8) + (k & 7)] = tg[k];
        for (int i = wave * 64 + lane; i < TL_DC_HIST + S.need; i += 64 * TL_DC_WAVES) {
            const uint32_t v = tl_fd_source(cin, pl, S.rel + i, S.fch, S.sch);
            if (pairs) w.x[TL_DC_AT - TL_DC_HIST + i] = v; else x16[TL_DC_AT - TL_DC_HIST + i] = (int16_t)v;
        }
    TL_LANES_END
}
// after the barrier: the 1152 outputs.  A one-channel feed for a two-channel stream is decimated once into `y` (LDS) and written to both
// channels by tl_fd_dup after one more barrier.
TL_FN void tl_fd_wave(const TlFeedDownLaunch &A, const TlDecimateLds &w, const TlFdSlot &S, int16_t *y, int s, int f, int wave)
{
    int16_t *dst = A.F.pcm + ((size_t)f * (size_t)A.F.nstreams + (size_t)s) * 2304;
    if (S.fch == 1 && S.sch == 2) dst = y;
    const bool two = S.fch == 2 && S.sch == 2;
    if (S.ratio == TL_DC_1_2) { if (two) tl_decimate_outputs<2, true>(dst, w, S.ratio, S.pos5, wave); else tl_decimate_outputs<1, true>(dst, w, S.ratio, S.pos5, wave); }
    else if (two) tl_decimate_outputs<2, false>(dst, w, S.ratio, S.pos5, wave);
    else tl_decimate_outputs<1, false>(dst, w, S.ratio, S.pos5, wave);
}
TL_FN void tl_fd_dup(const TlFeedDownLaunch &A, const int16_t *y, int s, int f, int wave)
{
    uint32_t *dst = (uint32_t *)(A.F.pcm + ((size_t)f * (size_t)A.F.nstreams + (size_t)s) * 2304);
    TL_LANES_BEGIN
        for (int i = wave * 64 + lane; i < TL_DC_FRAME; i += 64 * TL_DC_WAVES) { const uint32_t v = (uint16_t)y[i]; dst[i] = v | (v << 16); }
    TL_LANES_END
}

// ---- carry: what the next call needs of stream s (after every unit of this call is done) ----
TL_FN void tl_fd_carry(const TlFeedDownLaunch &A, int s)
{
    const TlFeedLaunch &F = A.F;
    const int ci = F.feed_cfg[s];
    if (ci < 0) return;
    const int ratio = A.ratio[s], fch = F.configs[ci].nch;
    if (ratio < TL_DC_80_147 || ratio > TL_DC_1_2) return;
    const int p0 = A.pos[(size_t)A.flip * (size_t)F.nstreams + (size_t)s], plast = p0 + F.nframes - 1;
    const int rows = tl_fd_K(plast, ratio) - tl_fd_K(p0 - 1, ratio);       // decoded in this call
    const int first = rows * 1152 - TL_FD_CARRY;               // the new head's first frame, counted from the call's first decoded frame
    const int16_t *cin = tl_fd_carry_of(A, A.flip, s), *pl = tl_fd_plane_of(A, s);
    int16_t *cout = (int16_t *)tl_fd_carry_of(A, A.flip ^ 1, s);
    const TlFeedLaunch V = tl_fd_view(F, s);
    tl_feed_keep(V, 0, (size_t)tl_fd_slot(F, s, F.nframes - 1, tl_fd_want(plast, ratio) - 1));      // the call's last wanted slot
    TL_LANES_BEGIN
    for (int i = lane; i < TL_FD_CARRY; i += 64) {
        const int16_t *p = tl_fd_frame(cin, pl, first + i, fch);
        if (fch == 2) ((uint32_t *)cout)[i] = *(const uint32_t *)p; else cout[i] = p[0];
    }
    if (lane == 0) A.pos[(size_t)(A.flip ^ 1) * (size_t)F.nstreams + (size_t)s] = (p0 + F.nframes) % tl_fd_cycle(ratio);
    TL_LANES_END
}
#endif
