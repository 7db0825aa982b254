// mp2_conceal_conv.h -- CONCEALMENT of lost frames on ADAPTED and DOWN Layer II feeds (include/toolame_batch.h, tlb_feed_loss_enable).
// The rule is the one of mp2_conceal.h, word for word (G, k, o(k), "G at offset o", the four cases); what changes is the sequence it runs
// over: a stream with an adapted or a down feed has the sequence of its WANTED slots only, in order -- the ticks with tl_fa_want(p) == 1,
// or slots j < tl_fd_want(p) of every tick, slot 0 before slot 1.  An unwanted slot, empty or TL_DEC_UNWANTED, is no slot of the sequence:
// it neither passes nor is lost, and touches neither k nor G nor the record.  What the rule makes of a slot replaces that slot's ROW of
// 1152 decoded source frames in the stream's source plane, in the feed's channel layout, BEFORE the channel map and the resampler or
// decimator read it and before the queue's carry copies it.  So the PCM the ingest receives is, bit for bit, what a strict feed with
// tlb_conceal_enable at the feed's own rate and channel count gives over the wanted slots, mapped and then resampled or decimated; PCM
// and record depend on the sequence of wanted slots only, never on how ticks are cut into calls.  `frames` of the record counts wanted slots.
//
// A POSITION is a place a slot can have in a call, in order: tick f of an adapted feed, 2 f + j of a down feed (TlCcvAdapt, TlCcvDown:
// whether a position is wanted, and which slot of the launch's arrays it is).  Two kernels per path (toolame_conceal_conv.hip):
//   conceal  one wavefront per position of a stream, between the path's decode kernel and its resample or decimate kernel: lane j reads
//            whether position q - j is wanted and, if so, whether its report says lost: two masks from one pass over the reports (hold + 2
//            = 18 wanted slots span at most 27 ticks at 3/2 and 36 positions of a down feed, fewer than the 64 lanes).  The lost bits of
//            the wanted positions, packed, ARE the window of tl_conceal_unit; the place of G is the n-th wanted position back.  Where the
//            window reaches the call's first wanted slot the carried run is added.  A unit with nothing to do leaves, wave-uniformly, and
//            writes nothing; every other unit overwrites the row tl_fa_decode_unit / tl_fd_decode_unit computes for the slot
//   carry    one wavefront per stream behind the path's own carry kernel, the lanes over the call's positions: the record fold of
//            tl_conceal_carry with run lengths counted in wanted slots, the last passing wanted slot's bytes into G, the new run
// Parameters, records and G are the per-stream arrays of mp2_conceal.h (a stream has one feed, so one of the three paths owns its entry).
// Lane-SPMD source for gfx950 and, with TL_EMULATE, lane loops; include after mp2_feed.h, mp2_feed_adapt.h, mp2_feed_down.h and
// mp2_conceal.h with TL_CC_BODY, TL_FA_BODY, TL_FD_BODY and TL_CCV_BODY defined (toolame_conceal_conv.hip and
// tests/emu/mp2_conceal_conv_emu.cpp; tl_kernels.h brings the part above the body to every unit).
#pragma once
#include <stdint.h>
#include "mp2_conceal.h"
#include "mp2_feed_adapt.h"
#include "mp2_feed_down.h"

// the concealment's own arrays, as in TlConcealLaunch
struct TlConcealConv {
    TlConcealStream *cs;              // [nstreams]
    TlConcealRecord *rec;             // [nstreams]; rec[s].run is the carried k, in wanted slots
    uint8_t *g;                       // [nstreams][g_stride] the last passing wanted slot of the calls before
    int32_t g_stride, pad_;           // a multiple of 4, at least the longest frame of any feed of the batch
};
// One call: D is the call the path's own kernels run (decode done when the conceal kernel starts, everything done when the carry starts;
// D.pos[D.flip] is the position at the call's start throughout)
struct TlConcealAdaptLaunch { TlFeedAdaptLaunch D; TlConcealConv X; };
struct TlConcealDownLaunch { TlFeedDownLaunch D; TlConcealConv X; };

#ifdef TL_CCV_BODY
// ---- the positions of stream s in a call: is position q wanted, and which slot of frames / len / report is it ----
struct TlCcvAdapt { int ns, s, p0, ratio; };                         // q: the tick
struct TlCcvDown { int ns, s, p0, ratio; };                          // q: 2 * tick + slot of the tick
TL_FN bool tl_ccv_want(const TlCcvAdapt &g, int q) { return tl_fa_want(g.p0 + q, g.ratio) != 0; }
TL_FN size_t tl_ccv_slot(const TlCcvAdapt &g, int q) { return (size_t)q * g.ns + g.s; }
TL_FN bool tl_ccv_want(const TlCcvDown &g, int q) { return (q & 1) < tl_fd_want(g.p0 + (q >> 1), g.ratio); }
TL_FN size_t tl_ccv_slot(const TlCcvDown &g, int q) { return ((size_t)(q >> 1) * g.ns + g.s) * 2 + (q & 1); }

// ---- the unit: position q of stream s, the idx-th wanted slot of the call (from 0), after the decode kernel has written its report and
// its row `out`.  F: the path's launch record (its slot arithmetic is geo's), C: the feed's record. ----
template <class Geo>
TL_FN void tl_ccv_unit(TlSynthLds &w, const TlFeedLaunch &F, const TlConcealConv &X, const TlConfig *TL_RESTRICT C, const Geo &geo, int s, int q,
                       int idx, int16_t *TL_RESTRICT out, const double *TL_RESTRICT dwin)
{
    const int hold = TL_UNI_I((int)X.cs[s].hold), step = TL_UNI_I((int)X.cs[s].step);
    if (hold <= 0) return;
    const int W = hold + 2;                                          // wanted slots before this one that decide what it becomes
    PV(bool, wnt); PV(bool, lost);
    TL_LANES_BEGIN
    const int p = q - lane;
    const bool wl = p >= 0 && tl_ccv_want(geo, p);
    L(wnt) = wl;
    L(lost) = wl && tl_cc_lost(F.report[tl_ccv_slot(geo, p)].status);
    TL_LANES_END
    const uint64_t wm = TL_BALLOT(wnt), lm = TL_BALLOT(lost);
    if (!(wm & 1u)) return;                                          // no slot of the sequence
    // the window of tl_conceal_unit: bit j is the j-th wanted slot back, j = 0 .. W (wave-uniform: the masks are scalars)
    uint64_t m = 0;
    { int n = 0; for (uint64_t r = wm; r && n <= W; r &= r - 1, n++) m |= ((lm >> __builtin_ctzll(r)) & 1ull) << n; }
    const bool own_lost = (m & 1u) != 0u;
    // the run that ends at `base`: this slot when it is lost, else the wanted slot before; nv of the window's slots lie at or before `base`
    const uint64_t mm = own_lost ? m : m >> 1;
    const int base = own_lost ? idx : idx - 1;
    const int nv = base + 1 < (own_lost ? W + 1 : W) ? base + 1 : (own_lost ? W + 1 : W);
    const int t = (int)__builtin_ctzll(~mm);                         // (bits above the window are 0)
    uint32_t k;
    int back;                                                        // G: so many wanted slots before this one, or -1: the carried copy
    if (t >= nv) {
        if (nv < base + 1) return;                                   // the window holds nothing but the run: beyond hold + 1, muted
        const uint32_t run = (uint32_t)TL_UNI_I((int)X.rec[s].run);
        k = (uint32_t)t + (run < 64u ? run : 64u);
        back = -1;
    } else { k = (uint32_t)t; back = idx - base + t; }
    if (k == 0) return;                                              // a passing slot behind a passing slot
    const uint32_t o_hist = tl_cc_offset(own_lost ? k - 1 : k, (uint32_t)hold, (uint32_t)step);
    const uint32_t o_cur = own_lost ? tl_cc_offset(k, (uint32_t)hold, (uint32_t)step) : 0u;
    if (o_hist == TL_CC_MUTE) return;

    const uint8_t *gsrc; int glen, gmax;
    if (back >= 0) {
        uint64_t r = wm;
        for (int i = 0; i < back; i++) r &= r - 1;                   // the back-th wanted position before q
        if (!r) return;                                              // (18 wanted slots lie within the 64 lanes)
        const size_t gs = tl_ccv_slot(geo, q - (int)__builtin_ctzll(r));
        gsrc = F.frames + gs * F.stride; glen = F.len[gs]; gmax = F.stride;
    } else { gsrc = X.g + (size_t)s * X.g_stride; glen = X.cs[s].g_len; gmax = X.g_stride; }
    glen = TL_UNI_I(glen < gmax ? glen : gmax);                      // (no read leaves the slot)
    if (glen <= 0) return;                                           // no G yet

    const size_t slot = tl_ccv_slot(geo, q);
    const TlBlockShared *B = &F.tables->shared;
    const TlPackTables *K = &F.tables->pack;
    TlDecSide sdp, sd;
    TlDecCells xp, xc;
    if (tl_feed_parse(w.d[0], B, K, C, gsrc, glen, sdp, xp) & TL_DEC_BAD_MASK) return;       // (G passed when it was kept)
    tl_cc_raise(xp, o_hist);
    const uint8_t *src = gsrc; int len = glen;
    if (!own_lost) {
        src = F.frames + slot * F.stride; len = F.len[slot];
        len = TL_UNI_I(len < F.stride ? len : F.stride);
    }
    tl_feed_parse(w.d[1], B, K, C, src, len, sd, xc);
    tl_cc_raise(xc, o_cur);
    tl_synth_frame(w, B, K, F.synth, C->nch, true, sdp, xp, sd, xc, out, 1, C->nch, dwin);
}

// tick f of adapted stream s: the row is tl_fa_decode_unit's
TL_FN void tl_ccv_adapt_unit(TlSynthLds &w, const TlConcealAdaptLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const TlFeedAdaptLaunch &D = A.D;
    const TlFeedLaunch &F = D.F;
    const int ci = TL_UNI_I(F.feed_cfg[s]);
    if (ci < 0 || TL_UNI_I((int)A.X.cs[s].hold) <= 0) return;
    const int ratio = TL_UNI_I(D.ratio[s]);
    const int p0 = TL_UNI_I(D.pos[(size_t)D.flip * (size_t)F.nstreams + (size_t)s]), p = p0 + f;
    if (!tl_fa_want(p, ratio)) return;
    const TlConfig *C = &F.configs[ci];
    const int row = TL_UNI_I(tl_fa_K(p, ratio) - 1 - tl_fa_K(p0 - 1, ratio));    // 0 .. f: the wanted slots of the call before this one
    int16_t *out = (int16_t *)tl_fa_plane_of(D, s) + TL_UNI_I(row * 1152 * C->nch);
    const TlCcvAdapt geo = {F.nstreams, s, p0, ratio};
    tl_ccv_unit(w, F, A.X, C, geo, s, f, row, out, dwin);
}

// slot j of tick f of stream s with a down feed: the row is tl_fd_decode_unit's.  Slot 1 reads reports and bytes of slot 0, never its PCM
TL_FN void tl_ccv_down_unit(TlSynthLds &w, const TlConcealDownLaunch &A, int s, int f, int j, const double *TL_RESTRICT dwin)
{
    const TlFeedDownLaunch &D = A.D;
    const TlFeedLaunch &F = D.F;
    const int ci = TL_UNI_I(F.feed_cfg[s]);
    if (ci < 0 || TL_UNI_I((int)A.X.cs[s].hold) <= 0) return;
    const int ratio = TL_UNI_I(D.ratio[s]);
    if (ratio < TL_DC_80_147 || ratio > TL_DC_1_2) return;
    const int p0 = TL_UNI_I(D.pos[(size_t)D.flip * (size_t)F.nstreams + (size_t)s]), p = p0 + f;
    if (j >= tl_fd_want(p, ratio)) return;
    const TlConfig *C = &F.configs[ci];
    const int row = TL_UNI_I(tl_fd_K(p - 1, ratio) - tl_fd_K(p0 - 1, ratio) + j);      // 0 .. 2 f + 1
    int16_t *out = (int16_t *)tl_fd_plane_of(D, s) + TL_UNI_I(row * 1152 * C->nch);
    const TlCcvDown geo = {F.nstreams, s, p0, ratio};
    tl_ccv_unit(w, F, A.X, C, geo, s, 2 * f + j, row, out, dwin);
}

// ---- the carry: what a call of npos positions leaves of stream s (after every unit and the path's own carry are done) ----
template <class Geo>
TL_FN void tl_ccv_carry(const TlFeedLaunch &F, const TlConcealConv &X, const Geo &geo, int s, int npos)
{
    TlConcealStream *cs = &X.cs[s];
    TlConcealRecord *R = &X.rec[s];
    const uint32_t hold = (uint32_t)TL_UNI_I((int)cs->hold), step = (uint32_t)TL_UNI_I((int)cs->step);
    if (hold == 0u) return;
    uint32_t run = (uint32_t)TL_UNI_I((int)R->run), longest = (uint32_t)TL_UNI_I((int)R->longest);
    uint32_t frames = 0, passed = 0, conc = 0, muted = 0, runs = 0;
    bool have_g = TL_UNI_I(cs->g_len) > 0;
    int last_pass = -1;                                              // a position
    for (int c0 = 0; c0 < npos; c0 += 64) {
        const int n = npos - c0 < 64 ? npos - c0 : 64;
        PV(bool, wnt); PV(bool, pass);
        TL_LANES_BEGIN
        const bool wl = lane < n && tl_ccv_want(geo, c0 + lane);
        L(wnt) = wl;
        L(pass) = wl && !tl_cc_lost(F.report[tl_ccv_slot(geo, c0 + lane)].status);
        TL_LANES_END
        const uint64_t Wm = TL_BALLOT(wnt), P = TL_BALLOT(pass);
        PV(bool, bc); PV(bool, bm); PV(bool, br); PV(uint64_t, nk);
        TL_LANES_BEGIN
        const uint64_t upto = (2ull << lane) - 1ull;                 // the chunk's positions up to this one
        const uint64_t below = P & upto;                             // passing wanted slots among them
        const bool lostl = ((Wm & ~P) >> lane) & 1ull;
        // the run in WANTED slots: those behind the last passing one, or all of the chunk's so far and the run brought along
        const uint32_t k = below ? (uint32_t)__builtin_popcountll(Wm & upto & ~((2ull << (63 - (int)__builtin_clzll(below))) - 1ull))
                                 : (uint32_t)__builtin_popcountll(Wm & upto) + run;
        const bool synth = lostl && (have_g || below != 0ull) && k - 1u <= hold;
        L(bc) = synth; L(bm) = lostl && !synth; L(br) = lostl && k == 1u;
        L(nk) = ~(uint64_t)(lostl ? k : 0u);
        TL_LANES_END
        conc += (uint32_t)__builtin_popcountll(TL_BALLOT(bc));
        muted += (uint32_t)__builtin_popcountll(TL_BALLOT(bm));
        runs += (uint32_t)__builtin_popcountll(TL_BALLOT(br));
        passed += (uint32_t)__builtin_popcountll(P);
        frames += (uint32_t)__builtin_popcountll(Wm);
        const uint32_t kmax = (uint32_t)~TL_WAVE_MIN_U64(nk);
        longest = kmax > longest ? kmax : longest;
        if (P) {
            const int top = 63 - (int)__builtin_clzll(P);
            have_g = true; last_pass = c0 + top; run = (uint32_t)__builtin_popcountll((Wm >> top) >> 1);
        } else { const uint32_t nw = (uint32_t)__builtin_popcountll(Wm); run = run + nw < run ? 0xFFFFFFFFu : run + nw; }
    }
    if (last_pass >= 0) {                                            // G: the slot's bytes as tl_feed_keep keeps them, never beyond the slot
        const size_t slot = tl_ccv_slot(geo, last_pass);
        const int keep = F.stride < X.g_stride ? F.stride : X.g_stride;
        int len = F.len[slot];
        len = len < 0 ? 0 : len < keep ? len : keep;
        const uint32_t *src = (const uint32_t *)(F.frames + slot * F.stride);
        uint32_t *dst = (uint32_t *)(X.g + (size_t)s * X.g_stride);
        TL_LANES_BEGIN
        for (int i = lane; i < (keep >> 2); i += 64) dst[i] = src[i];
        if (lane == 0) cs->g_len = len;
        TL_LANES_END
    }
    TL_LANES_BEGIN
    if (lane == 0) {
        R->frames += frames; R->passed += passed; R->concealed += conc; R->muted += muted; R->runs += runs;
        R->longest = longest; R->run = run; R->offset = tl_cc_offset(run, hold, step);
    }
    TL_LANES_END
}

TL_FN void tl_ccv_adapt_carry(const TlConcealAdaptLaunch &A, int s)
{
    const TlFeedLaunch &F = A.D.F;
    if (F.feed_cfg[s] < 0) return;
    const TlCcvAdapt geo = {F.nstreams, s, TL_UNI_I(A.D.pos[(size_t)A.D.flip * (size_t)F.nstreams + (size_t)s]), TL_UNI_I(A.D.ratio[s])};
    tl_ccv_carry(F, A.X, geo, s, F.nframes);
}
TL_FN void tl_ccv_down_carry(const TlConcealDownLaunch &A, int s)
{
    const TlFeedLaunch &F = A.D.F;
    if (F.feed_cfg[s] < 0) return;
    const int ratio = TL_UNI_I(A.D.ratio[s]);
    if (ratio < TL_DC_80_147 || ratio > TL_DC_1_2) return;
    const TlCcvDown geo = {F.nstreams, s, TL_UNI_I(A.D.pos[(size_t)A.D.flip * (size_t)F.nstreams + (size_t)s]), ratio};
    tl_ccv_carry(F, A.X, geo, s, 2 * F.nframes);
}
#endif
