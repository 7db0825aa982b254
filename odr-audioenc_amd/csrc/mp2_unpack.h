// mp2_unpack.h -- stage A of the frame check / decode path: a Layer II frame of this batch's own making read back from its bytes and
// verified against the stream's configuration (tl_unpack_unit).  The packer of mp2_pack.h in reverse: lane = 2*sb + ch owns subband sb of
// channel ch, every field's offset comes from a prefix sum over the lanes, no lane walks the bit stream.  Written from ISO/IEC 11172-3
// 2.4.1 / 2.4.2 (frame syntax) and the project's own packer; the CRCs are the packer's (crc.c:12-56, :58-113; placement toolame.c:515-551).
// Include after mp2_wave.h (its lane macros; lane-SPMD source that compiles for gfx950 and, with TL_EMULATE, as a lane loop).
#pragma once
#include "mp2_dec_types.h"

// Per-wave LDS: the frame as big-endian words (zero beyond its bytes; + 4: a 48-bit read at the last bit touches three words) and the
// per-(channel, subband) fields that lanes read from each other.
struct TlDecLds {
    alignas(16) uint32_t frame[TL_MAX_FRAME_WORDS + 4];
    uint8_t balloc[2][32];
};
// wave-uniform results of the side-information parse
struct TlDecSide {
    uint32_t status;                 // BAD_SYNC, HEADER_MISMATCH, BAD_CRC16, BAD_ALLOC, OVERRUN as far as the frame alone shows them
    int mode, mode_ext, jsbound, frame_len;      // frame_len: what the configuration and the padding bit say
    int start;                                   // first bit behind the header and its CRC-16: 48, or 32 in a feed frame without protection
    int p_smp, n_smp, audio_bits, maxpos;        // first sample bit, sample bits of one round of triples, end of the samples; last readable bit
    uint32_t crc_stored, crc_computed;
    uint32_t scfcrc[4];              // ScF-CRC of band groups 0..3 computed from the scalefactors (0 where the frame protects none)
};

// nbits (0..48) from bit `pos`, MSB first.  pos <= 8 * TL_MAX_FRAME_BYTES (callers clamp): the three words are inside TlDecLds::frame.
TL_FN uint64_t tl_get_bits48(const uint32_t *frame, int pos, int nbits)
{
    const int w = pos >> 5, o = pos & 31;
    const uint64_t hi = ((uint64_t)frame[w] << 32) | frame[w + 1];
    const uint64_t top = (hi << o) | (((uint64_t)frame[w + 2] << o) >> 32);
    return nbits > 0 ? top >> (64 - nbits) : 0;
}

// The slot's first `nbytes` bytes into the wave's LDS.  Whole words are read: `src` is 4-byte aligned and the slot a multiple of 4 bytes
// long (tlb_out_stride), so no read leaves the slot; bytes past nbytes are masked to zero, and two words of zeros follow.
TL_FN void tl_dec_load(TlDecLds &w, const uint8_t *TL_RESTRICT src, int nbytes)
{
    const int nw = (nbytes + 3) >> 2;
    TL_LANES_BEGIN
    for (int i = lane; i < nw + 3; i += 64) {
        uint32_t v = 0;
        if (i < nw) {
            v = tl_bswap(((const uint32_t *)src)[i]);
            const int rem = nbytes - 4 * i;
            if (rem < 4) v &= ~(0xffffffffu >> (8 * rem));
        }
        w.frame[i] = v;
    }
    TL_LANES_END
}

// Header and side information of the frame in w.frame (nbytes of it are real).  Per lane (sb, ch): the allocation code `ba`, the
// quantiser record `qi` (TlBlockShared::qinfo_line; 0: no samples), the three scalefactor indices, the scfsi code and the offset of the
// cell's sample field inside one round of triples.  A joint-stereo cell of channel 1 above the bound gets channel 0's code, record and
// offset (the shared samples) and its own scalefactors.  `sel` < 0 in cells that transmit none.
// Every read position is clamped to the loaded bytes, every table index comes from a field no wider than its table.
// FEED: the frame is somebody else's (mp2_feed.h), C the feed's configuration.  Sync, ID, layer, bitrate and sampling-frequency index must
// be C's; the protection bit is read (with a CRC-16 the fields start at bit 48 and the CRC is verified, without one at bit 32); private,
// copyright, original and emphasis are ignored; a two-channel feed's frames may be stereo, joint stereo with any bound or dual channel, a
// one-channel feed's are mono; behind the samples comes ancillary data: no PAD is reserved and no ScF-CRC is computed.
template <bool CRC, bool FEED = false>
TL_FN void tl_dec_side(TlDecLds &w, const TlBlockShared *TL_RESTRICT B, const TlPackTables *TL_RESTRICT K, const TlConfig *TL_RESTRICT C,
                       int nbytes, TlDecSide &sd, PARG(int, ba), PARG(unsigned, qi), PARGA(int, scf, 3), PARG(int, sel), PARG(int, o_smp))
{
    const uint32_t *frame = w.frame;
    const int nch = C->nch, sblimit = C->sblimit;
    const uint32_t h = frame[0];
    uint32_t st = 0;
    if ((h >> 20) != 0xfffu) st |= TL_DEC_BAD_SYNC;
    int mode = (int)((h >> 6) & 3u), mode_ext = (int)((h >> 4) & 3u);
    const int padding = (int)((h >> 9) & 1u);
    sd.mode = mode; sd.mode_ext = mode_ext;
    // ID, layer II, protection on, bitrate and sampling-frequency index, private bit, copyright / original / emphasis as the packer writes them
    const uint32_t want = ((uint32_t)C->version << 19) | (2u << 17) | ((uint32_t)C->br_idx << 12) | ((uint32_t)C->fs_idx << 10);
    const uint32_t hdr_mask = FEED ? 0x000efc00u : 0x000ffd0fu;
    if ((h & hdr_mask) != want) st |= TL_DEC_HEADER_MISMATCH;
    const int start = FEED && ((h >> 16) & 1u) ? 32 : 48;
    sd.start = start;
    if (padding && C->pad_frac == 0) st |= TL_DEC_HEADER_MISMATCH;
    // the mode: a joint-stereo stream's frames are stereo or joint stereo with any bound (the encoder chooses per frame), every other
    // stream's frames carry the configuration's mode and extension
    const bool mode_ok = FEED ? (C->nch == 2 ? mode != 3 : mode == 3)
                       : C->mode0 == 1 ? (mode == 1 || (mode == 0 && mode_ext == 0)) : (mode == C->mode0 && mode_ext == C->mode_ext0);
    if (!mode_ok) { st |= TL_DEC_HEADER_MISMATCH; mode = C->mode0; mode_ext = C->mode_ext0; }
    const int jsbound = mode == 1 ? (4 * (mode_ext + 1) < sblimit ? 4 * (mode_ext + 1) : sblimit) : sblimit;
    sd.jsbound = jsbound;
    sd.frame_len = C->frame_bytes + ((padding && C->pad_frac != 0) ? 1 : 0);
    const int maxpos = 8 * (nbytes < TL_MAX_FRAME_BYTES ? nbytes : TL_MAX_FRAME_BYTES);
    sd.maxpos = maxpos;

    // ---- bit_alloc ----
    PV(int, f_ba); PV(int, o_ba); PV(int, a_ln);
    TL_LANES_BEGIN
    const int c = lane & 1, sb = lane >> 1;
    const bool own = sb < sblimit && c < (sb < jsbound ? nch : 1);
    L(a_ln) = sb < sblimit ? (int)C->line[sb] : 0;
    L(f_ba) = own ? (int)C->nbal[sb] : 0;
    TL_LANES_END
    TL_WAVE_EXSCAN_I32(o_ba, f_ba);
    const int n_ba = TL_WAVE_SUM_I32(f_ba);
    TL_LANES_BEGIN
    const int c = lane & 1, sb = lane >> 1;
    int p = start + L(o_ba);
    p = p < maxpos ? p : maxpos;
    w.balloc[c][sb] = (uint8_t)tl_get_bits48(frame, p, L(f_ba));
    TL_LANES_END
    PV(int, f_sel); PV(int, o_sel);
    TL_LANES_BEGIN
    const int c = lane & 1, sb = lane >> 1;
    const bool live = c < nch && sb < sblimit;
    const bool own = sb < sblimit && c < (sb < jsbound ? nch : 1);
    const int b = live ? (int)w.balloc[own ? c : 0][sb] : 0;          // above the bound channel 1 shares channel 0's code
    L(ba) = b;
    L(qi) = b ? (unsigned)B->qinfo_line[L(a_ln)][b] : 0u;
    L(f_sel) = b ? 2 : 0;
    TL_LANES_END
    {   // a code the table has no quantiser for (none of the tables in use has such a hole; the check stands for those that might)
        PV(bool, hole);
        TL_LANES_BEGIN L(hole) = L(ba) != 0 && (L(qi) & 31u) == 0u; TL_LANES_END
        if (TL_BALLOT(hole)) st |= TL_DEC_BAD_ALLOC;
    }
    // ---- scfsi ----
    TL_WAVE_EXSCAN_I32(o_sel, f_sel);
    const int n_sel = TL_WAVE_SUM_I32(f_sel);
    const int p_sel = start + n_ba, p_scf = p_sel + n_sel;
    PV(int, f_scf); PV(int, o_scf);
    TL_LANES_BEGIN
    int p = p_sel + L(o_sel);
    p = p < maxpos ? p : maxpos;
    const int si = (int)tl_get_bits48(frame, p, L(f_sel));
    L(sel) = L(ba) ? si : -1;
    L(f_scf) = L(ba) ? 6 * tl_sfs_count((unsigned)si) : 0;
    TL_LANES_END
    // ---- scalefactors: three, two (first and last) or one index of six bits, expanded by the scfsi pattern (2.4.2.5) ----
    TL_WAVE_EXSCAN_I32(o_scf, f_scf);
    const int n_scf = TL_WAVE_SUM_I32(f_scf);
    const int p_smp = p_scf + n_scf;
    PV(int, f_smp);
    TL_LANES_BEGIN
    const int c = lane & 1, sb = lane >> 1;
    int p = p_scf + L(o_scf);
    p = p < maxpos ? p : maxpos;
    const unsigned v = (unsigned)tl_get_bits48(frame, p, L(f_scf));
    int s0 = 0, s1 = 0, s2 = 0;
    switch (L(sel)) {
    case 0: s0 = (int)(v >> 12) & 63; s1 = (int)(v >> 6) & 63; s2 = (int)v & 63; break;
    case 1: s0 = s1 = (int)(v >> 6) & 63; s2 = (int)v & 63; break;
    case 3: s0 = (int)(v >> 6) & 63; s1 = s2 = (int)v & 63; break;
    case 2: s0 = s1 = s2 = (int)v & 63; break;
    default: break;
    }
    L(scf)[0] = s0; L(scf)[1] = s1; L(scf)[2] = s2;
    const bool own = sb < sblimit && c < (sb < jsbound ? nch : 1);
    L(f_smp) = (own && L(ba)) ? (int)(((L(qi) >> 10) & 1u) ? 3u : 1u) * (int)((L(qi) >> 5) & 31u) : 0;
    TL_LANES_END
    TL_WAVE_EXSCAN_I32(o_smp, f_smp);
    const int n_smp = TL_WAVE_SUM_I32(f_smp);
    TL_LANES_BEGIN
    // a shared cell: channel 0's field, which ends where this lane's (empty) one begins
    if (L(ba) && !L(f_smp)) L(o_smp) -= (int)(((L(qi) >> 10) & 1u) ? 3u : 1u) * (int)((L(qi) >> 5) & 31u);
    TL_LANES_END
    sd.p_smp = p_smp; sd.n_smp = n_smp; sd.audio_bits = p_smp + 12 * n_smp;
    // ---- bit budget: the fields and the smallest PAD (ScF-CRC + F-PAD) fit the frame; the slot holds the whole frame ----
    {
        const int have = nbytes < sd.frame_len ? nbytes : sd.frame_len;
        if (sd.audio_bits > 8 * (FEED ? have : have - C->dab_ext - 2) || nbytes < sd.frame_len) st |= TL_DEC_OVERRUN;
    }
    sd.crc_stored = start == 48 ? (frame[1] >> 16) & 0xffffu : 0u;
    sd.crc_computed = 0;
    sd.scfcrc[0] = sd.scfcrc[1] = sd.scfcrc[2] = sd.scfcrc[3] = 0;
    if (CRC && start == 48) {
        // CRC-16 over header bits 16..31, bit_alloc and scfsi (crc.c:12-41), folded a byte per lane as the packer folds it (mp2_pack.h):
        // n <= 16 + 188 + 120 bits whatever the bytes say, so lanes 0..40 carry the message and 62 / 63 the preset
        const int n = 16 + (p_scf - start);
        PV(uint32_t, part);
        TL_LANES_BEGIN
        uint32_t acc = 0;
        const bool preset = lane >= 62;
        const int first = 8 * lane;
        if (first < n || preset) {
            const int byte = lane < 2 ? lane + 2 : lane + 4;
            const int cnt = preset ? 8 : (n - first < 8 ? n - first : 8);
            const int e0 = preset ? n + 8 * (63 - lane) : 16 + (n - first - cnt);
            const uint16_t *xt = &K->crc_xpow[e0];
            const unsigned v = preset ? 0xffu : ((frame[byte >> 2] >> (24 - 8 * (byte & 3))) & 0xffu) >> (8 - cnt);
            for (int k = 0; k < 8; k++) acc ^= (0u - ((v >> k) & 1u)) & xt[k];
        }
        L(part) = acc;
        TL_LANES_END
        sd.crc_computed = TL_WAVE_XOR_U32(part) & 0xffffu;
        if (sd.crc_computed != sd.crc_stored) st |= TL_DEC_BAD_CRC16;
    }
    if (CRC && !FEED) {
        // ScF-CRC (crc.c:58-113): per band group the CRC-8 of the three MSBs of the transmitted scalefactors, as the packer computes it
        PV(int, rlen); PV(uint32_t, rcrc); PV(int, lex);
        TL_LANES_BEGIN
        uint32_t rec = 0;
        if (L(ba)) {
            const uint32_t s0 = (uint32_t)L(scf)[0] >> 3, s1 = (uint32_t)L(scf)[1] >> 3, s2 = (uint32_t)L(scf)[2] >> 3;
            switch (L(sel)) {
            case 0: rec = (9u << 16) | (s0 << 6) | (s1 << 3) | s2; break;
            case 1: case 3: rec = (6u << 16) | (s0 << 3) | s2; break;
            default: rec = (3u << 16) | s0; break;
            }
        }
        L(rlen) = (int)(rec >> 16); L(rcrc) = rec & 0x1ffu;
        TL_LANES_END
        TL_WAVE_EXSCAN_I32(lex, rlen);
        const int fb[5] = {0, 4, 8, 16, 30};
        int gend[4], gfirst[4], glast[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
            gfirst[g] = fb[g]; glast[g] = fb[g + 1] > sblimit ? sblimit : fb[g + 1];
            gend[g] = (g < C->dab_ext && glast[g] > gfirst[g]) ? TL_READLANE_I32(lex, 2 * glast[g]) : 0;
        }
        PV(uint32_t, part8); PV(uint32_t, pscan);
        TL_LANES_BEGIN
        const int sb = lane >> 1;
        const int g = sb < 4 ? 0 : sb < 8 ? 1 : sb < 16 ? 2 : 3;
        const int after = (g == 0 ? gend[0] : g == 1 ? gend[1] : g == 2 ? gend[2] : gend[3]) - L(lex) - L(rlen);
        const int e0 = after + 8;
        unsigned xp = K->crc8_xpow[e0 < 0 ? 0 : e0 > 319 ? 319 : e0];
        unsigned acc = 0;
        const unsigned rb = L(rcrc);
        for (int b = 0; b < 9; b++) {
            acc ^= ((rb >> b) & 1u) ? xp : 0u;
            xp = ((xp << 1) & 0xffu) ^ ((xp & 0x80u) ? 0x1Du : 0u);
        }
        L(part8) = (L(rlen) && sb < sblimit) ? acc : 0u;
        TL_LANES_END
        TL_WAVE_INCL_XSCAN_U32(pscan, part8);
#pragma unroll
        for (int g = 0; g < 4; g++)
            if (g < C->dab_ext && glast[g] > gfirst[g]) {
                uint32_t v = (uint32_t)TL_READLANE_I32(pscan, 2 * glast[g] - 1);
                if (gfirst[g] > 0) v ^= (uint32_t)TL_READLANE_I32(pscan, 2 * gfirst[g] - 1);
                sd.scfcrc[g] = v & 0xffu;
            }
    }
    sd.status = st;
}

// The three sample codes of a cell in round r (0..11) of the sample field: three codewords of nb bits, or one grouped codeword
// v0 + steps (v1 + steps v2) of 3, 5 or 9 steps (2.4.3.3.4).  qi != 0.
TL_FN void tl_dec_triple(const uint32_t *frame, const TlPackTables *TL_RESTRICT K, const TlDecSide &sd, unsigned qi, int o_smp, int r, unsigned (&v)[3])
{
    const int nb = (int)((qi >> 5) & 31u);
    const bool three = ((qi >> 10) & 1u) != 0;
    int p = sd.p_smp + r * sd.n_smp + o_smp;
    p = p < 0 ? 0 : p < sd.maxpos ? p : sd.maxpos;
    const uint64_t code = tl_get_bits48(frame, p, three ? 3 * nb : nb);
    if (three) {
        const unsigned m = (1u << nb) - 1u;
        v[0] = (unsigned)(code >> (2 * nb)) & m; v[1] = (unsigned)(code >> nb) & m; v[2] = (unsigned)code & m;
    } else {
        const unsigned cw = (unsigned)code, steps = (unsigned)K->steps[qi & 31u];
        const unsigned t = steps == 3u ? cw / 3u : steps == 5u ? cw / 5u : cw / 9u;
        const unsigned u = steps == 3u ? t / 3u : steps == 5u ? t / 5u : t / 9u;
        v[0] = cw - steps * t; v[1] = t - steps * u; v[2] = u;
    }
}

// Where the ScF-CRC of slot f's frame is stored: the tail of the last non-empty slot before it in this launch, or what the launch before
// left (TlDecStream).  The tail sits at the end of the carrying frame, so its place depends on that frame's length: where the caller
// gives lengths, the slot's length and the frame's own padding bit must agree on it -- a frame cut short has lost its tail, a damaged
// padding bit would point two or four bytes off -- and where they do not, there is nothing to check against (false).
TL_FN bool tl_dec_tail(const TlDecLaunch &A, const TlConfig *TL_RESTRICT C, int s, int f, uint32_t (&tail)[4])
{
    int p = f - 1;
    if (A.len) while (p >= 0 && A.len[(size_t)p * A.nstreams + s] <= 0) p--;
    tail[0] = tail[1] = tail[2] = tail[3] = 0;
    if (p < 0) {
        const TlDecStream *ds = &A.state[s];
        tail[0] = ds->tail[0]; tail[1] = ds->tail[1]; tail[2] = ds->tail[2]; tail[3] = ds->tail[3];
        return ds->have_tail != 0;
    }
    const size_t slot = (size_t)p * A.nstreams + s;
    const uint8_t *src = A.frames + slot * A.out_stride;
    const int pad = (src[2] >> 1) & 1;
    const int flen = C->frame_bytes + ((pad && C->pad_frac != 0) ? 1 : 0);
    if (A.len && A.len[slot] != flen) return false;
    const uint8_t *tp = src + (flen - 2 - C->dab_ext);
    tail[0] = tp[0]; tail[1] = tp[1];                                  // dab_ext is 2 or 4 (tl_build_config)
    if (C->dab_ext > 2) { tail[2] = tp[2]; tail[3] = tp[3]; }
    return true;
}

// a slot's report, by lane 0: the status word and what the frame's side information says (sd = NULL: an empty slot, every field 0)
TL_FN void tl_dec_report(TlFrameReport *rep, uint32_t st, const TlDecSide *sd)
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

// ---- the unit of stage A: slot f of stream s -> its report and, when asked for, its fields.  Returns the status word. ----
TL_FN uint32_t tl_unpack_unit(TlDecLds &w, const TlDecLaunch &A, int s, int f)
{
    const TlConfig *C = &A.configs[A.stream_cfg ? A.stream_cfg[s] : 0];
    const TlBlockShared *B = &A.tables->shared;
    const TlPackTables *K = &A.tables->pack;
    const size_t slot = (size_t)f * A.nstreams + s;
    const uint8_t *src = A.frames + slot * A.out_stride;
    TlFrameReport *rep = &A.report[slot];
    TlFrameFields *fl = A.fields ? &A.fields[slot] : nullptr;
    int len = A.len ? A.len[slot] : A.out_stride;
    len = len < A.out_stride ? len : A.out_stride;
    if (len <= 0) {
        // this one report stays inline: through tl_dec_report(rep, TL_DEC_EMPTY, nullptr) its twelve constant bytes are stored as dwordx2 + dword
        // instead of one dwordx3, and the decoder's kernels (the monitor's per-tick path) are kept instruction for instruction as they were
        TL_LANES_BEGIN
        if (lane == 0) { rep->status = TL_DEC_EMPTY; rep->crc_stored = rep->crc_computed = 0; rep->mode = rep->mode_ext = 0; rep->audio_bits = 0; }
        if (fl) for (int i = lane; i < (int)(sizeof(TlFrameFields) / 4); i += 64) ((uint32_t *)fl)[i] = 0;
        TL_LANES_END
        return TL_DEC_EMPTY;
    }
    tl_dec_load(w, src, len);
    TlDecSide sd;
    PV(int, ba); PV(unsigned, qi); PA(int, scf, 3); PV(int, sel); PV(int, o_smp);
    tl_dec_side<true>(w, B, K, C, len, sd, ba, qi, scf, sel, o_smp);
    uint32_t st = sd.status;
    if (A.len && len > sd.frame_len) st |= TL_DEC_HEADER_MISMATCH;      // (no lengths given: the frame is as long as it says)
    {   // ScF-CRC against the bytes the frame before carries for this one: group g travels in byte dab_ext - 1 - g of the tail
        uint32_t tail[4];
        if (!tl_dec_tail(A, C, s, f, tail)) st |= TL_DEC_SCFCRC_UNCHECKED;
        else if (C->dab_ext > 2 ? (tail[0] != sd.scfcrc[3] || tail[1] != sd.scfcrc[2] || tail[2] != sd.scfcrc[1] || tail[3] != sd.scfcrc[0])
                                : (tail[0] != sd.scfcrc[1] || tail[1] != sd.scfcrc[0])) st |= TL_DEC_BAD_SCFCRC;
    }
    tl_dec_report(rep, st, &sd);
    if (fl) {
        TL_LANES_BEGIN
        const int c = lane & 1, sb = lane >> 1;
        fl->bit_alloc[c][sb] = (uint8_t)L(ba);
        fl->scfsi[c][sb] = (uint8_t)(L(sel) < 0 ? 0 : L(sel));
        for (int gr = 0; gr < 3; gr++) fl->scalar[c][gr][sb] = (uint8_t)L(scf)[gr];
        TL_LANES_END
        for (int r = 0; r < 12; r++) {
            TL_LANES_BEGIN
            const int c = lane & 1, sb = lane >> 1;
            const bool own = sb < C->sblimit && c < (sb < sd.jsbound ? C->nch : 1);
            unsigned v[3] = {0, 0, 0};
            if (own && L(qi)) tl_dec_triple(w.frame, K, sd, L(qi), L(o_smp), r, v);
            for (int x = 0; x < 3; x++) fl->subband[c][r >> 2][(r & 3) * 3 + x][sb] = (uint16_t)v[x];
            TL_LANES_END
        }
    }
    return st;
}

// What the next launch's first frame needs of stream s (after every unit of this launch is done): the ScF-CRC tail of the last non-empty
// slot, and the last slot itself -- bytes, length, status -- for the synthesis history.
TL_FN void tl_dec_carry(const TlDecLaunch &A, int s)
{
    const TlConfig *C = &A.configs[A.stream_cfg ? A.stream_cfg[s] : 0];
    TlDecStream *ds = &A.state[s];
    uint32_t tail[4] = {0, 0, 0, 0};
    int last = A.nframes - 1;
    if (A.len) while (last >= 0 && A.len[(size_t)last * A.nstreams + s] <= 0) last--;
    const bool any = last >= 0;
    const bool have = any ? tl_dec_tail(A, C, s, last + 1, tail) : false;
    const size_t slot = (size_t)(A.nframes - 1) * A.nstreams + s;
    int len = A.len ? A.len[slot] : A.out_stride;
    len = len < 0 ? 0 : len < A.out_stride ? len : A.out_stride;
    const uint32_t st = A.report[slot].status;
    const uint32_t *src = (const uint32_t *)(A.frames + slot * A.out_stride);
    uint32_t *dst = (uint32_t *)(A.prev + (size_t)s * A.out_stride);
    TL_LANES_BEGIN
    for (int i = lane; i < (A.out_stride >> 2); i += 64) dst[i] = src[i];
    if (lane == 0) {
        if (any) { ds->have_tail = have ? 1 : 0; ds->tail[0] = (uint8_t)tail[0]; ds->tail[1] = (uint8_t)tail[1]; ds->tail[2] = (uint8_t)tail[2]; ds->tail[3] = (uint8_t)tail[3]; }
        ds->prev_len = len; ds->prev_status = st;
    }
    TL_LANES_END
}
