// mp2_feed.h -- Layer II FEEDS: a stream's source arrives as MP2 frames somebody else encoded and is decoded on the device into the slot
// the ingest reads (tl_feed_unit).  The parser, the requantiser and the synthesis filterbank are those of the frame check / decode path
// (mp2_unpack.h: tl_dec_side<.., true>, tl_dec_report; mp2_synth.h: tl_synth_frame) under the FEED's configuration and a foreign frame's
// rules: the protection bit is read per frame, the free header bits are ignored, the mode is the frame's own, there is no DAB tail.
// tl_feed_decode is THE decode of a feed frame: it parses the slot and the slot before it (the synthesis history) itself, so units stay
// independent and one kernel does what the decode path does in two.  A strict feed (tl_feed_unit) and an adapted one (mp2_feed_adapt.h:
// tl_fa_decode_unit) differ in where the samples go and in which slot is the one before; tl_feed_keep is the history either leaves for
// the next launch.  Include after mp2_wave.h, mp2_unpack.h and mp2_synth.h (lane-SPMD source that compiles for gfx950 and, with
// TL_EMULATE, as a lane loop).
#pragma once
#include "mp2_synth.h"

// `len` bytes at `src` (0 < len <= the slot's stride) into d, parsed and verified as a feed frame -> its status word
TL_FN uint32_t tl_feed_parse(TlDecLds &d, const TlBlockShared *TL_RESTRICT B, const TlPackTables *TL_RESTRICT K, const TlConfig *TL_RESTRICT C,
                             const uint8_t *TL_RESTRICT src, int len, TlDecSide &sd, TlDecCells &x)
{
    tl_dec_load(d, src, len);
    tl_dec_side<true, true>(d, B, K, C, len, sd, x.ba, x.qi, x.scf, x.sel, x.o_smp);
    return sd.status | (len > sd.frame_len ? TL_DEC_HEADER_MISMATCH : 0u);
}

// ---- the decode of one feed frame: slot f of stream s, a feed under configuration C -> its report and 1152 sample frames at `out`,
// interleaved as the ingest reads them (sample i of channel c at out[i * nch + c]); an empty slot or a frame that does not pass is silence.
// `pf`: the slot of this launch that holds the frame before, or TL_FEED_CARRIED: the bytes and status the launch before left ----
#define TL_FEED_CARRIED (-1)
TL_FN void tl_feed_decode(TlSynthLds &w, const TlFeedLaunch &F, const TlConfig *TL_RESTRICT C, int s, int f, int pf, int16_t *TL_RESTRICT out,
                          const double *TL_RESTRICT dwin)
{
    const size_t slot = (size_t)f * F.nstreams + s;
    TlFrameReport *rep = &F.report[slot];
    const TlBlockShared *B = &F.tables->shared;
    const TlPackTables *K = &F.tables->pack;
    const int nch = C->nch;
    int len = F.len[slot];
    len = len < F.stride ? len : F.stride;                           // (no read leaves the slot)
    if (len <= 0) { tl_dec_report(rep, TL_DEC_EMPTY, nullptr); tl_synth_zero(out, 1152 * nch); return; }

    TlDecSide sdp, sd;
    TlDecCells xp, xc;
    const uint32_t st = tl_feed_parse(w.d[1], B, K, C, F.frames + slot * F.stride, len, sd, xc);
    tl_dec_report(rep, st, &sd);
    if (st & TL_DEC_BAD_MASK) { tl_synth_zero(out, 1152 * nch); return; }

    bool hist;
    {   // the slot before: in this launch, or what the launch before left.  A slot that did not pass is silence.
        const uint8_t *psrc; int plen, pmax;
        if (pf >= 0) {
            const size_t ps = (size_t)pf * F.nstreams + s;
            psrc = F.frames + ps * F.stride; plen = F.len[ps]; pmax = F.stride; hist = true;
        } else {
            psrc = F.prev + (size_t)s * F.prev_stride; plen = F.state[s].prev_len; pmax = F.prev_stride;
            hist = !(F.state[s].prev_status & (TL_DEC_BAD_MASK | TL_DEC_EMPTY));
        }
        plen = plen < pmax ? plen : pmax;
        hist = hist && plen > 0;
        if (hist) hist = !(tl_feed_parse(w.d[0], B, K, C, psrc, plen, sdp, xp) & TL_DEC_BAD_MASK);
    }
    tl_synth_frame(w, B, K, F.synth, nch, hist, sdp, xp, sd, xc, out, 1, nch, dwin);
}

// ---- the strict unit: slot f of stream s into the start of the stream's ingest slot.  The slot of a stream without a feed is reported
// EMPTY and its PCM is not touched. ----
TL_FN void tl_feed_unit(TlSynthLds &w, const TlFeedLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const size_t slot = (size_t)f * A.nstreams + s;
    const int ci = A.feed_cfg[s];
    if (ci < 0) { tl_dec_report(&A.report[slot], TL_DEC_EMPTY, nullptr); return; }
    tl_feed_decode(w, A, &A.configs[ci], s, f, f - 1, A.pcm + slot * 2304, dwin);
}

// What the next launch's first frame needs of stream s (after every unit of this launch is done): slot `slot` -- bytes, length, status
TL_FN void tl_feed_keep(const TlFeedLaunch &F, int s, size_t slot)
{
    // the history's slots hold the longest frame of any feed of the batch; a launch's slots may be wider (the tick plane's are)
    const int keep = F.stride < F.prev_stride ? F.stride : F.prev_stride;
    int len = F.len[slot];
    len = len < 0 ? 0 : len < keep ? len : keep;
    const uint32_t st = F.report[slot].status;
    const uint32_t *src = (const uint32_t *)(F.frames + slot * F.stride);
    uint32_t *dst = (uint32_t *)(F.prev + (size_t)s * F.prev_stride);
    TlDecStream *ds = &F.state[s];
    TL_LANES_BEGIN
    for (int i = lane; i < (keep >> 2); i += 64) dst[i] = src[i];
    if (lane == 0) { ds->prev_len = len; ds->prev_status = st; }
    TL_LANES_END
}
// ... of a strict feed: the last slot
TL_FN void tl_feed_carry(const TlFeedLaunch &A, int s)
{
    if (A.feed_cfg[s] >= 0) tl_feed_keep(A, s, (size_t)(A.nframes - 1) * A.nstreams + s);
}
