// mp2_feed.h -- Layer II FEEDS: a stream's source arrives as MP2 frames somebody else encoded and is decoded on the device into the slot
// the ingest reads (tl_feed_unit).  The parser, the requantiser and the synthesis filterbank are those of the frame check / decode path
// (mp2_unpack.h: tl_dec_side<.., true>; mp2_synth.h: tl_synth_frame) under the FEED's configuration and a foreign frame's rules: the
// protection bit is read per frame, the free header bits are ignored, the mode is the frame's own, there is no DAB tail.
// One unit = slot f of stream s: it parses the slot and the slot before it (the synthesis history) itself, so units stay independent and
// one kernel does what the decode path does in two.  Include after mp2_wave.h, mp2_unpack.h and mp2_synth.h (lane-SPMD source that
// compiles for gfx950 and, with TL_EMULATE, as a lane loop).
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

TL_FN void tl_feed_report(TlFrameReport *rep, uint32_t st, const TlDecSide *sd)
{
    TL_LANES_BEGIN
    if (lane == 0) {
        rep->status = st;
        rep->crc_stored = sd ? (uint16_t)sd->crc_stored : 0; rep->crc_computed = sd ? (uint16_t)sd->crc_computed : 0;
        rep->mode = sd ? (uint8_t)sd->mode : 0; rep->mode_ext = sd ? (uint8_t)sd->mode_ext : 0;
        rep->audio_bits = sd ? (uint16_t)(sd->audio_bits < 65535 ? sd->audio_bits : 65535) : 0;
    }
    TL_LANES_END
}

// ---- the unit: slot f of stream s -> its report and 1152 interleaved sample frames at the start of the stream's ingest slot.  The slot
// of a stream without a feed is reported EMPTY and its PCM is not touched. ----
TL_FN void tl_feed_unit(TlSynthLds &w, const TlFeedLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const size_t slot = (size_t)f * A.nstreams + s;
    TlFrameReport *rep = &A.report[slot];
    const int ci = A.feed_cfg[s];
    if (ci < 0) { tl_feed_report(rep, TL_DEC_EMPTY, nullptr); return; }
    const TlConfig *C = &A.configs[ci];
    const TlBlockShared *B = &A.tables->shared;
    const TlPackTables *K = &A.tables->pack;
    const int nch = C->nch;
    int16_t *out = A.pcm + slot * 2304;
    int len = A.len[slot];
    len = len < A.stride ? len : A.stride;                           // (no read leaves the slot)
    if (len <= 0) { tl_feed_report(rep, TL_DEC_EMPTY, nullptr); tl_synth_zero(out, 1152 * nch); return; }

    TlDecSide sdp, sd;
    TlDecCells xp, xc;
    const uint32_t st = tl_feed_parse(w.d[1], B, K, C, A.frames + slot * A.stride, len, sd, xc);
    tl_feed_report(rep, st, &sd);
    if (st & TL_DEC_BAD_MASK) { tl_synth_zero(out, 1152 * nch); return; }

    bool hist;
    {   // the slot before: in this launch, or what the launch before left.  A slot that did not pass is silence.
        const uint8_t *psrc; int plen, pmax;
        if (f > 0) {
            const size_t ps = slot - (size_t)A.nstreams;
            psrc = A.frames + ps * A.stride; plen = A.len[ps]; pmax = A.stride; hist = true;
        } else {
            psrc = A.prev + (size_t)s * A.prev_stride; plen = A.state[s].prev_len; pmax = A.prev_stride;
            hist = !(A.state[s].prev_status & (TL_DEC_BAD_MASK | TL_DEC_EMPTY));
        }
        plen = plen < pmax ? plen : pmax;
        hist = hist && plen > 0;
        if (hist) hist = !(tl_feed_parse(w.d[0], B, K, C, psrc, plen, sdp, xp) & TL_DEC_BAD_MASK);
    }
    // interleaved as the ingest reads it: sample i of channel c at out[i * nch + c]
    tl_synth_frame(w, B, K, A.synth, nch, hist, sdp, xp, sd, xc, out, 1, nch, dwin);
}

// What the next launch's first frame needs of stream s (after every unit of this launch is done): the last slot -- bytes, length, status
TL_FN void tl_feed_carry(const TlFeedLaunch &A, int s)
{
    if (A.feed_cfg[s] < 0) return;
    const size_t slot = (size_t)(A.nframes - 1) * A.nstreams + s;
    // the history's slots hold the longest frame of any feed of the batch; a launch's slots may be wider (the tick plane's are)
    const int keep = A.stride < A.prev_stride ? A.stride : A.prev_stride;
    int len = A.len[slot];
    len = len < 0 ? 0 : len < keep ? len : keep;
    const uint32_t st = A.report[slot].status;
    const uint32_t *src = (const uint32_t *)(A.frames + slot * A.stride);
    uint32_t *dst = (uint32_t *)(A.prev + (size_t)s * A.prev_stride);
    TlDecStream *ds = &A.state[s];
    TL_LANES_BEGIN
    for (int i = lane; i < (keep >> 2); i += 64) dst[i] = src[i];
    if (lane == 0) { ds->prev_len = len; ds->prev_status = st; }
    TL_LANES_END
}
