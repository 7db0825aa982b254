// mp2_compare.h -- the compare monitor's body (include/toolame_batch.h, tlb_compare_*): is the decoded audio the audio that went in?
// The planar PCM the encoder was given and the PCM tlb_decode_* synthesised from the frame that left are set side by side at the codec's
// delay and correlated, per stream and slot, in integers.  One wavefront per stream walks the stream's slots in order; tl_compare_stream
// is that wave's text, written with the lane macros of mp2_wave.h so that tests/emu/mp2_compare_emu.cpp runs it as lane loops.
//
// One slot f of a call, for one stream (D = TL_CMP_DELAY, odd):
//   in[f]   the planar frame the encoder was given in that slot; dec[f] the decoded PCM of the frame in output slot f, which is the audio
//           of input frame f - 1 (one frame of latency, tlb_encode_device).
//   history the previous input frame P and the last D samples Q of the one before: h[c][0..D) = Q, h[c][D..D+1152) = P.  So the input
//           aligned with dec[f] is simply x[c][i] = h[c][i], i = 0..1151, read as 16-byte pieces; the odd offset falls on the history's
//           advance (h[c][j] = h[c][1152 + j] for j < D, then h[c][D + i] = in[f][c][i]), which runs in LDS with 2-byte writes.
//   sums    sxx[c] = sum x[c]^2, syy[c] = sum y[c]^2, sxy[c] = sum x[c] y[c], sxz[c] = sum x[c] y[1 - c], int64, |.| < 2^41; a one-channel
//           stream has c = 0 only and sxz = 0.
//   rule    channel c is JUDGED when sxx[c] >= min_energy; it MATCHES when sxy[c] > 0 and den^2 sxy[c]^2 >= num^2 sxx[c] syy[c] (128-bit
//           integers); the CROSS test is the same with sxz[c] and syy[1 - c].  MISMATCH: a judged channel that does not match.  SWAPPED: two
//           channels, both judged, neither matches, both cross tests match.
//   skipped a slot whose report has EMPTY or a BAD_MASK flag is not compared (last_flags = SKIPPED, nothing else changes); its input still
//           advances the history.  An unjudged frame leaves mismatch_run alone, a judged one that matches sets it to 0.
// Every sum is an integer sum, so neither the lanes' shares nor the cut of a stream's slots into calls can change a bit of the record.
#pragma once
#include <stdint.h>
#include "mp2_dec_types.h"

#define TL_CMP_WAVES 4                // streams (wavefronts) per workgroup
#define TL_CMP_DELAY 481              // analysis + synthesis filterbank, samples (tests/test_compare_emu.py measures it)
#define TL_CMP_FRAME 1152
#define TL_CMP_HIST ((TL_CMP_FRAME + TL_CMP_DELAY + 7) & ~7)      // int16 per channel of a stream's history, whole 16-byte pieces (the tail is 0)
#define TL_CMP_JUDGED0 0x01u
#define TL_CMP_JUDGED1 0x02u
#define TL_CMP_MISMATCH 0x04u
#define TL_CMP_SWAPPED 0x08u
#define TL_CMP_SKIPPED 0x10u
struct TlCompareRecord {              // tlb_compare_record
    int64_t sxx[2], syy[2], sxy[2], sxz[2];
    uint32_t frames_compared, frames_judged, mismatch_frames, mismatch_run, swapped_frames, last_flags, reserved_[2];
};
struct TlCompareParams { int64_t min_energy; int32_t corr_num, corr_den; };      // tlb_compare_params
static_assert(sizeof(TlCompareRecord) == 96 && sizeof(TlCompareParams) == 16, "record and parameter layout");
static_assert((TL_CMP_DELAY & 1) == 1 && TL_CMP_DELAY < TL_CMP_FRAME && TL_CMP_HIST % 8 == 0, "history geometry");

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the layout above and nothing else
struct alignas(16) TlCmpVec { int16_t v[8]; };                       // 16 bytes: one global_load_dwordx4 / ds_read_b128 per lane
struct alignas(16) TlCmpLds { int16_t h[2][TL_CMP_HIST]; };          // one wave's history while it walks its slots
#define TL_CMP_VECS (TL_CMP_FRAME / 8)                               // 144 pieces per channel and frame: 2.25 per lane
#define TL_CMP_HVECS (TL_CMP_HIST / 8)                               // 205 pieces of history per channel

#ifdef TL_EMULATE
TL_FN int64_t tlh_sum_i64(const int64_t (&v)[64][8], int k) { int64_t s = 0; for (int i = 0; i < 64; i++) s += v[i][k]; return s; }
#define TL_WAVE_SUM_I64(name, k) tlh_sum_i64(name, k)
TL_FN void tl_mul64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) { const unsigned __int128 p = (unsigned __int128)a * b; hi = (uint64_t)(p >> 64); lo = (uint64_t)p; }
#else
// sum over the 64 lanes of a 64-bit integer, DPP only: the ladder of tld_incl_scan_i32 on both halves, the carry in the 64-bit add
#define TL_CMP_DPP_STEP(ctl, rows) do { \
    const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(uint64_t)v, ctl, rows, 0xf, false); \
    const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)((uint64_t)v >> 32), ctl, rows, 0xf, false); \
    v += (int64_t)(((uint64_t)hi_ << 32) | lo_); } while (0)
TL_FN int64_t tld_sum_i64(int64_t v)
{
    TL_CMP_DPP_STEP(0x111, 0xf); TL_CMP_DPP_STEP(0x112, 0xf); TL_CMP_DPP_STEP(0x114, 0xf); TL_CMP_DPP_STEP(0x118, 0xf);
    TL_CMP_DPP_STEP(0x142, 0xa); TL_CMP_DPP_STEP(0x143, 0xc);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(uint64_t)v, 63);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)((uint64_t)v >> 32), 63);
    return (int64_t)(((uint64_t)hi << 32) | lo);
}
#define TL_WAVE_SUM_I64(name, k) tld_sum_i64(name[k])
TL_FN void tl_mul64(uint64_t a, uint64_t b, uint64_t &hi, uint64_t &lo) { hi = __umul64hi(a, b); lo = a * b; }
#endif

// k^2 a b as a 128-bit integer (hi, lo), for 0 <= a, b < 2^41 and 0 < k <= 1024: a b < 2^82, so its high word times k^2 stays below 2^38
TL_FN void tl_cmp_scaled(uint64_t a, uint64_t b, uint32_t k, uint64_t &hi, uint64_t &lo)
{
    uint64_t h1, l1, h2;
    tl_mul64(a, b, h1, l1);
    tl_mul64(l1, (uint64_t)k * k, h2, lo);
    hi = h1 * ((uint64_t)k * k) + h2;
}
// the rule: sab > 0 and den^2 sab^2 >= num^2 saa sbb
TL_FN bool tl_cmp_match(int64_t sab, int64_t saa, int64_t sbb, const TlCompareParams &P)
{
    if (sab <= 0) return false;
    uint64_t lh, ll, rh, rl;
    tl_cmp_scaled((uint64_t)sab, (uint64_t)sab, (uint32_t)P.corr_den, lh, ll);
    tl_cmp_scaled((uint64_t)saa, (uint64_t)sbb, (uint32_t)P.corr_num, rh, rl);
    return lh > rh || (lh == rh && ll >= rl);
}

// in [nframes][nstreams][2][1152] or NULL (the flush: no advance), dec the same shape, report [nframes][nstreams] or NULL (every slot
// skipped: a tick that has no frames yet), hist [nstreams][2][TL_CMP_HIST], record [nstreams] read-modify-write.  No load leaves a slot
// or the stream's history: the lanes take pieces q = k * 64 + lane < 144 of a channel and < 205 per channel of the history.
TL_FN void tl_compare_stream(const int16_t *TL_RESTRICT in, const int16_t *TL_RESTRICT dec, const TlFrameReport *TL_RESTRICT report, int16_t *TL_RESTRICT hist,
                             TlCompareRecord *TL_RESTRICT record, const TlCompareParams P, TlCmpLds &w, int nch, int s, int nstreams, int nframes)
{
    TlCompareRecord *rec = record + s;
    TlCmpVec *hg = (TlCmpVec *)(hist + (size_t)s * (size_t)(2 * TL_CMP_HIST));
    TlCmpVec *hl = (TlCmpVec *)&w.h[0][0];
    int64_t *rsum = (int64_t *)rec;                                  // sxx, syy, sxy, sxz lie one behind the other
    int64_t sum[8];
#pragma unroll
    for (int k = 0; k < 8; k++) sum[k] = rsum[k];
    uint32_t compared = rec->frames_compared, judged = rec->frames_judged, mism = rec->mismatch_frames, run = rec->mismatch_run;
    uint32_t swapped = rec->swapped_frames, last = rec->last_flags;
    TL_LANES_BEGIN
        for (int q = lane; q < nch * TL_CMP_HVECS; q += 64) hl[q] = hg[q];      // (a one-channel stream's second half is never looked at)
    TL_LANES_END
    for (int f = 0; f < nframes; f++) {
        const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
        const uint32_t st = report ? report[slot].status : (uint32_t)TL_DEC_EMPTY;
        if (st & (TL_DEC_EMPTY | TL_DEC_BAD_MASK)) last = TL_CMP_SKIPPED;
        else {
            const TlCmpVec *y0 = (const TlCmpVec *)(dec + slot * (size_t)(2 * TL_CMP_FRAME)), *y1 = y0 + TL_CMP_VECS;
            const TlCmpVec *x0 = (const TlCmpVec *)&w.h[0][0], *x1 = (const TlCmpVec *)&w.h[1][0];
            PA(int64_t, acc, 8);
            TL_LANES_BEGIN
                int64_t a[8] = {0, 0, 0, 0, 0, 0, 0, 0};             // sxx0 sxx1 syy0 syy1 sxy0 sxy1 sxz0 sxz1: a lane's share of sum x y leaves 32 bits
                for (int q = lane; q < TL_CMP_VECS; q += 64) {
                    const TlCmpVec vy0 = y0[q], vx0 = x0[q];
                    if (nch == 2) {
                        const TlCmpVec vy1 = y1[q], vx1 = x1[q];
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const int p0 = vx0.v[j], p1 = vx1.v[j], r0 = vy0.v[j], r1 = vy1.v[j];
                            a[0] += (int64_t)p0 * p0; a[1] += (int64_t)p1 * p1; a[2] += (int64_t)r0 * r0; a[3] += (int64_t)r1 * r1;
                            a[4] += (int64_t)p0 * r0; a[5] += (int64_t)p1 * r1; a[6] += (int64_t)p0 * r1; a[7] += (int64_t)p1 * r0;
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            const int p0 = vx0.v[j], r0 = vy0.v[j];
                            a[0] += (int64_t)p0 * p0; a[2] += (int64_t)r0 * r0; a[4] += (int64_t)p0 * r0;
                        }
                    }
                }
#pragma unroll
                for (int k = 0; k < 8; k++) L(acc)[k] = a[k];
            TL_LANES_END
#pragma unroll
            for (int k = 0; k < 8; k++) sum[k] = TL_WAVE_SUM_I64(acc, k);
            const int64_t *sxx = sum, *syy = sum + 2, *sxy = sum + 4, *sxz = sum + 6;
            const bool j0 = sxx[0] >= P.min_energy, j1 = nch == 2 && sxx[1] >= P.min_energy;
            const bool m0 = j0 && tl_cmp_match(sxy[0], sxx[0], syy[0], P), m1 = j1 && tl_cmp_match(sxy[1], sxx[1], syy[1], P);
            const bool bad = (j0 && !m0) || (j1 && !m1);
            const bool swp = j0 && j1 && !m0 && !m1 && tl_cmp_match(sxz[0], sxx[0], syy[1], P) && tl_cmp_match(sxz[1], sxx[1], syy[0], P);
            compared++;
            if (j0 || j1) { judged++; if (bad) { mism++; run++; } else run = 0u; }
            if (swp) swapped++;
            last = (j0 ? TL_CMP_JUDGED0 : 0u) | (j1 ? TL_CMP_JUDGED1 : 0u) | (bad ? TL_CMP_MISMATCH : 0u) | (swp ? TL_CMP_SWAPPED : 0u);
        }
        if (!in) continue;
        const TlCmpVec *n0 = (const TlCmpVec *)(in + slot * (size_t)(2 * TL_CMP_FRAME));
        TL_LANES_BEGIN                                               // the tail of the frame that was P becomes Q: source and target do not overlap
            for (int c = 0; c < nch; c++)
                for (int j = lane; j < TL_CMP_DELAY; j += 64) w.h[c][j] = w.h[c][TL_CMP_FRAME + j];
        TL_LANES_END
        TL_LANES_BEGIN                                               // in[f] becomes P, at the odd offset D
            for (int c = 0; c < nch; c++)
                for (int q = lane; q < TL_CMP_VECS; q += 64) {
                    const TlCmpVec t = n0[c * TL_CMP_VECS + q];
#pragma unroll
                    for (int j = 0; j < 8; j++) w.h[c][TL_CMP_DELAY + 8 * q + j] = t.v[j];
                }
        TL_LANES_END
    }
    TL_LANES_BEGIN
        if (in) for (int q = lane; q < nch * TL_CMP_HVECS; q += 64) hg[q] = hl[q];
        if (lane == 0) {
#pragma unroll
            for (int k = 0; k < 8; k++) rsum[k] = sum[k];
            rec->frames_compared = compared; rec->frames_judged = judged; rec->mismatch_frames = mism; rec->mismatch_run = run;
            rec->swapped_frames = swapped; rec->last_flags = last; rec->reserved_[0] = 0u; rec->reserved_[1] = 0u;
        }
    TL_LANES_END
}
#endif
