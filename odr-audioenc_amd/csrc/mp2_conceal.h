// mp2_conceal.h -- CONCEALMENT of lost frames on a strict Layer II feed (include/toolame_batch.h, tlb_conceal_*): a lost slot is the last good
// frame once more, quieter, and not 24 ms of digital zero; the good frame behind a loss is synthesised over that repeat and not over silence.
// The reference has no concealment (its inputs leave it to their decoders), so the rule is DEFINED here; tests/conceallib.py restates it.
//
// Per stream with concealment on: `hold` (1..16 frames) and `step` (1..21 scalefactor-index units per lost frame; 3 is 6.02 dB, since
// scalefactor[i] = 2^(1 - i/3) and scalefactor[63] = 1e-20).
//   A slot PASSES when its feed report has none of TL_DEC_BAD_MASK | TL_DEC_EMPTY, else it is LOST (a strict feed wants a frame every tick:
//   an empty slot is a lost packet).
//   G     the bytes of the last slot that passed; none before the first passing slot and after a reset
//   k     the number of consecutive lost slots ending at this one, 0 for a passing slot; it carries across launches
//   o(k)  o(0) = 0, o(k) = step * k for 1 <= k <= hold, o(k) = MUTE for k > hold
//   "G at offset o": G parsed by tl_feed_parse, then every cell's three scf indices replaced by min(scf + o, 63); at MUTE every index is 63
//   a lost slot with run k:     no G, or o(k - 1) = MUTE: zeros, what the feed kernel wrote.  Otherwise tl_synth_frame of G at o(k) over the
//                               history G at o(k - 1) -- so frame hold + 1 is the all-63 frame over the last audible repeat: the filterbank's
//                               tail rings out and is not cut
//   a passing slot whose predecessor was lost with run k': G (the one from BEFORE this slot) exists and o(k') != MUTE: its own bytes over the
//                               history G at o(k').  Otherwise silent history, what the feed kernel wrote
//   a passing slot whose predecessor passed: what the feed kernel wrote, untouched
// The result depends on the sequence of slots only, never on how that sequence is cut into launches.
// Why indices: attenuation by raising an index is exact (a table look-up the requantiser makes anyway) and needs no arithmetic of its own;
// synthesis keeps no state in memory (mp2_synth.h: a unit rebuilds its history from the bytes of the slot before), so a repeat is a re-parse.
//
// Two kernels behind the feed's own two, which run exactly as before (toolame_conceal.hip):
//   conceal  one wavefront per (stream, slot): lane j reads the feed report of slot f - j, j = 0 .. hold + 2, ONE ballot (hence hold <= 16);
//            where that window reaches slot 0 the carried run is added.  From the mask: k, k' and where G lies (a slot of this launch, or
//            the carried copy).  A unit with nothing to do leaves, wave-uniformly, and writes nothing; every other unit overwrites the
//            slot's PCM, interleaved as tl_feed_unit writes it
//   carry    one wavefront per stream, the lanes over the launch's slots: the record, the last passing slot's bytes into the stream's G
//            buffer, the new run.  A kernel of its own: G and run must not change before every unit of the launch has read them
// Per stream a record of eight uint32 (TlConcealRecord): frames, passed, concealed (lost slots synthesised from G, the ring-out frame
// included), muted (lost slots left as zeros), runs (loss runs begun), longest (loss run), run (k now), offset (o(k) of the last slot,
// 0 for a passing one, MUTE = 0xFFFFFFFF).
// Lane-SPMD source for gfx950 and, with TL_EMULATE, lane loops; include after mp2_feed.h with TL_CC_BODY defined (toolame_conceal.hip and
// tests/emu/mp2_conceal_emu.cpp; tl_kernels.h brings the part above the body to every unit).
#pragma once
#include <stdint.h>
#include "mp2_dec_types.h"

#define TL_CC_MAX_HOLD 16
#define TL_CC_MAX_STEP 21
#define TL_CC_MUTE 0xFFFFFFFFu

struct TlConcealRecord { uint32_t frames, passed, concealed, muted, runs, longest, run, offset; };
// a stream's parameters (hold 0: concealment off) and the length of what its G slot holds (0: no G)
struct TlConcealStream { uint32_t hold, step; int32_t g_len; uint32_t pad_; };
static_assert(sizeof(TlConcealRecord) == 32 && sizeof(TlConcealStream) == 16, "C-ABI record; 48 bytes of state per stream beside G");

// One launch: F is the feed launch the two feed kernels have just run (mp2_dec_types.h), reports and PCM written.
struct TlConcealLaunch {
    TlFeedLaunch F;
    TlConcealStream *cs;              // [nstreams]
    TlConcealRecord *rec;             // [nstreams]; rec[s].run is the carried k
    uint8_t *g;                       // [nstreams][g_stride] the last passing slot of the launches before
    int32_t g_stride, pad_;           // a multiple of 4, at least the longest frame of any feed of the batch
};

static constexpr uint32_t tl_cc_offset(uint32_t k, uint32_t hold, uint32_t step) { return k == 0 ? 0u : k <= hold ? step * k : TL_CC_MUTE; }

#ifdef TL_CC_BODY
TL_FN bool tl_cc_lost(uint32_t st) { return (st & (TL_DEC_BAD_MASK | TL_DEC_EMPTY)) != 0u; }

// the parsed frame at offset o: every index raised, none beyond 63
TL_FN void tl_cc_raise(TlDecCells &x, uint32_t o)
{
    const int add = o == TL_CC_MUTE ? 63 : (int)o;
    TL_LANES_BEGIN
    for (int j = 0; j < 3; j++) { const int v = L(x.scf)[j] + add; L(x.scf)[j] = v < 63 ? v : 63; }
    TL_LANES_END
}

// ---- the unit: slot f of stream s, after the feed kernel has written its report and its PCM ----
TL_FN void tl_conceal_unit(TlSynthLds &w, const TlConcealLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const TlFeedLaunch &F = A.F;
    const int ci = TL_UNI_I(F.feed_cfg[s]);
    const int hold = TL_UNI_I((int)A.cs[s].hold), step = TL_UNI_I((int)A.cs[s].step);
    if (ci < 0 || hold <= 0) return;
    const int W = hold + 2;                                          // slots before this one that decide what it becomes
    PV(bool, lost);
    TL_LANES_BEGIN
    const int p = f - lane;
    L(lost) = lane <= W && p >= 0 && tl_cc_lost(F.report[(size_t)p * F.nstreams + s].status);
    TL_LANES_END
    const uint64_t m = TL_BALLOT(lost);
    const bool own_lost = (m & 1u) != 0u;
    // the run that ends at `base`: this slot when it is lost, else the slot before; nv of the window's slots lie at or before `base`
    const uint64_t mm = own_lost ? m : m >> 1;
    const int base = own_lost ? f : f - 1;
    const int nv = base + 1 < (own_lost ? W + 1 : W) ? base + 1 : (own_lost ? W + 1 : W);
    const int t = (int)__builtin_ctzll(~mm);                         // (bits above the window are 0)
    uint32_t k;
    int gslot;                                                       // G: the slot before the run, or -1: the carried copy
    if (t >= nv) {
        if (nv < base + 1) return;                                   // the window holds nothing but the run: beyond hold + 1, muted
        const uint32_t run = (uint32_t)TL_UNI_I((int)A.rec[s].run);
        k = (uint32_t)t + (run < 64u ? run : 64u);
        gslot = -1;
    } else { k = (uint32_t)t; gslot = base - t; }
    if (k == 0) return;                                              // a passing slot behind a passing slot
    const uint32_t o_hist = tl_cc_offset(own_lost ? k - 1 : k, (uint32_t)hold, (uint32_t)step);
    const uint32_t o_cur = own_lost ? tl_cc_offset(k, (uint32_t)hold, (uint32_t)step) : 0u;
    if (o_hist == TL_CC_MUTE) return;

    const uint8_t *gsrc; int glen, gmax;
    if (gslot >= 0) {
        const size_t gs = (size_t)gslot * F.nstreams + s;
        gsrc = F.frames + gs * F.stride; glen = F.len[gs]; gmax = F.stride;
    } else { gsrc = A.g + (size_t)s * A.g_stride; glen = A.cs[s].g_len; gmax = A.g_stride; }
    glen = TL_UNI_I(glen < gmax ? glen : gmax);                      // (no read leaves the slot)
    if (glen <= 0) return;                                           // no G yet

    const size_t slot = (size_t)f * F.nstreams + s;
    const TlBlockShared *B = &F.tables->shared;
    const TlPackTables *K = &F.tables->pack;
    const TlConfig *C = &F.configs[ci];
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
    tl_synth_frame(w, B, K, F.synth, C->nch, true, sdp, xp, sd, xc, F.pcm + slot * 2304, 1, C->nch, dwin);
}

// ---- the carry: what the launch leaves of stream s (after every unit is done) ----
TL_FN void tl_conceal_carry(const TlConcealLaunch &A, int s)
{
    const TlFeedLaunch &F = A.F;
    TlConcealStream *cs = &A.cs[s];
    TlConcealRecord *R = &A.rec[s];
    const uint32_t hold = (uint32_t)TL_UNI_I((int)cs->hold), step = (uint32_t)TL_UNI_I((int)cs->step);
    if (F.feed_cfg[s] < 0 || hold == 0u) return;
    uint32_t run = (uint32_t)TL_UNI_I((int)R->run), longest = (uint32_t)TL_UNI_I((int)R->longest);
    uint32_t passed = 0, conc = 0, muted = 0, runs = 0;
    bool have_g = TL_UNI_I(cs->g_len) > 0;
    int last_pass = -1;
    for (int c0 = 0; c0 < F.nframes; c0 += 64) {
        const int n = F.nframes - c0 < 64 ? F.nframes - c0 : 64;
        PV(bool, pass);
        TL_LANES_BEGIN
        L(pass) = lane < n && !tl_cc_lost(F.report[(size_t)(c0 + lane) * F.nstreams + s].status);
        TL_LANES_END
        const uint64_t P = TL_BALLOT(pass);
        PV(bool, bc); PV(bool, bm); PV(bool, br); PV(uint64_t, nk);
        TL_LANES_BEGIN
        const uint64_t below = P & ((2ull << lane) - 1ull);         // passing slots of the chunk up to this one
        const bool lostl = lane < n && !((P >> lane) & 1ull);
        const uint32_t k = below ? (uint32_t)(lane - (63 - (int)__builtin_clzll(below))) : (uint32_t)(lane + 1) + run;
        const bool synth = lostl && (have_g || below != 0ull) && k - 1u <= hold;
        L(bc) = synth; L(bm) = lostl && !synth; L(br) = lostl && k == 1u;
        L(nk) = ~(uint64_t)(lostl ? k : 0u);
        TL_LANES_END
        conc += (uint32_t)__builtin_popcountll(TL_BALLOT(bc));
        muted += (uint32_t)__builtin_popcountll(TL_BALLOT(bm));
        runs += (uint32_t)__builtin_popcountll(TL_BALLOT(br));
        passed += (uint32_t)__builtin_popcountll(P);
        const uint32_t kmax = (uint32_t)~TL_WAVE_MIN_U64(nk);
        longest = kmax > longest ? kmax : longest;
        if (P) {
            const int top = 63 - (int)__builtin_clzll(P);
            have_g = true; last_pass = c0 + top; run = (uint32_t)(n - 1 - top);
        } else run = run + (uint32_t)n < run ? 0xFFFFFFFFu : run + (uint32_t)n;
    }
    if (last_pass >= 0) {                                            // G: the slot's bytes as tl_feed_keep keeps them, never beyond the slot
        const size_t slot = (size_t)last_pass * F.nstreams + s;
        const int keep = F.stride < A.g_stride ? F.stride : A.g_stride;
        int len = F.len[slot];
        len = len < 0 ? 0 : len < keep ? len : keep;
        const uint32_t *src = (const uint32_t *)(F.frames + slot * F.stride);
        uint32_t *dst = (uint32_t *)(A.g + (size_t)s * A.g_stride);
        TL_LANES_BEGIN
        for (int i = lane; i < (keep >> 2); i += 64) dst[i] = src[i];
        if (lane == 0) cs->g_len = len;
        TL_LANES_END
    }
    TL_LANES_BEGIN
    if (lane == 0) {
        R->frames += (uint32_t)F.nframes; R->passed += passed; R->concealed += conc; R->muted += muted; R->runs += runs;
        R->longest = longest; R->run = run; R->offset = tl_cc_offset(run, hold, step);
    }
    TL_LANES_END
}
#endif
