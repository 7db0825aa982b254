// mp2_synth.h -- stage B of the frame check / decode path: requantisation (ISO/IEC 11172-3 2.4.3.3.4) and the 32-band synthesis
// filterbank (Annex 3-A.2, figure 3-A.2) of one frame, fp64 without contraction, PCM rounded to nearest and saturated (tl_synth_unit).
// Include after mp2_wave.h and mp2_unpack.h (lane-SPMD source that compiles for gfx950 and, with TL_EMULATE, as a lane loop).
//
// The flow chart shifts a 1024-entry vector V by 64, matrixes the 32 new subband samples into V[0..63], builds U from V and sums 16 windowed
// entries of U per output sample.  With V_t the 64 entries matrixed from sample vector t, U's two halves are V_{t-2i}[j] and V_{t-2i-1}[32+j]:
//     out_t[j] = sum_{i<8} D[j + 64 i] V_{t-2i}[j]  +  sum_{i<8} D[j + 32 + 64 i] V_{t-2i-1}[32 + j],       j = 0..31.
// Lane l owns entry l of every V_t and keeps its last 15 values in registers (no V in memory at all): with d_l[i] = D[l + 64 i] every lane
// forms q_t[l] = sum_i d_l[i] V_{t-2i}[l], and the two sums above are q_t[j] of lane j and q_{t-1}[32 + j] of lane 32 + j -- one exchange
// between the wave's halves per output vector.  The first output vector of a frame reaches back 15 sample vectors: the unit requantises
// them from the slot before (their field offsets follow from that frame's side information alone), so units stay independent.
#pragma once
#include "mp2_unpack.h"

#define TL_SYNTH_BATCH 15                          // sample vectors requantised at a time (five rounds of triples) = entries of the register ring,
                                                   // which is indexed with constants inside a batch
static_assert(TL_SYNTH_BATCH == TL_SYNTH_HIST && TL_SYNTH_BATCH % 3 == 0, "a batch is whole rounds and covers the history");
struct TlSynthLds {
    TlDecLds d[2];                                 // the slot before and the slot itself
    alignas(16) double s[TL_SYNTH_BATCH * 32];     // requantised samples of ONE channel, one batch [vector][subband]
};
// side information of a frame as the lanes hold it (tl_dec_side)
struct TlDecCells { PV(int, ba); PV(unsigned, qi); PA(int, scf, 3); PV(int, sel); PV(int, o_smp); };

// Rounds r0..r1-1 of channel cc of a frame -> w.s[(3 (r - r0) + x) * 32 + sb].  Cells without samples give zeros.
TL_FN void tl_requantise(TlSynthLds &w, const uint32_t *frame, const TlBlockShared *TL_RESTRICT B, const TlPackTables *TL_RESTRICT K,
                         const TlSynthTables *TL_RESTRICT Y, const TlDecSide &sd, const TlDecCells &x, int cc, int r0, int r1)
{
    PV(double, rc); PV(double, rd); PV(double, rm); PV(int, msb);
    TL_LANES_BEGIN
    const unsigned q = L(x.qi) & 31u;
    L(rc) = Y->rq_c[q]; L(rd) = Y->rq_d[q];
    L(msb) = K->steps2n[q];
    L(rm) = 1.0 / (double)(L(msb) ? L(msb) : 1);                       // a power of two: the product below is the exact quotient
    TL_LANES_END
    for (int r = r0; r < r1; r++) {
        TL_LANES_BEGIN
        const int c = lane & 1, sb = lane >> 1;
        if (c == cc) {
            double o[3] = {0.0, 0.0, 0.0};
            if (L(x.qi)) {
                unsigned v[3];
                tl_dec_triple(frame, K, sd, L(x.qi), L(x.o_smp), r, v);
                const double sf = B->scalefactor[L(x.scf)[r >> 2]];
                for (int j = 0; j < 3; j++) {
                    const double frac = (double)((int)v[j] - L(msb)) * L(rm);       // MSB inverted, two's complement fraction
                    o[j] = (L(rc) * (frac + L(rd))) * sf;
                }
            }
            double *dst = &w.s[3 * (r - r0) * 32 + sb];
            dst[0] = o[0]; dst[32] = o[1]; dst[64] = o[2];
        }
        TL_LANES_END
    }
}

TL_FN void tl_synth_zero(int16_t *out, int n)
{
    TL_LANES_BEGIN
    for (int i = lane; i < (n >> 1); i += 64) ((uint32_t *)out)[i] = 0;
    TL_LANES_END
}

// ---- synthesis of ONE frame from its parsed side information (sd, xc over w.d[1]) and, with `hist`, that of the slot before it (sdp, xp over
// w.d[0]; without: silence).  Sample i of channel c goes to out[c * cstep + i * sstep]: planar for the frame check / decode path (1152, 1),
// interleaved for a feed (1, nch; mp2_feed.h).
// `dwin`: the synthesis window TlSynthTables::d where the lanes re-read their eight coefficients per vector (the workgroup's LDS copy on the
// device: 16 registers less than holding them).
TL_FN void tl_synth_frame(TlSynthLds &w, const TlBlockShared *TL_RESTRICT B, const TlPackTables *TL_RESTRICT K, const TlSynthTables *TL_RESTRICT Y, int nch,
                          bool hist, const TlDecSide &sdp, const TlDecCells &xp, const TlDecSide &sd, const TlDecCells &xc, int16_t *out, int cstep, int sstep,
                          const double *TL_RESTRICT dwin)
{
    PA(double, nk, 32);
    TL_LANES_BEGIN
    for (int k = 0; k < 32; k++) L(nk)[k] = Y->n[k][lane];
    TL_LANES_END
    for (int c = 0; c < nch; c++) {
        int16_t *oc = out + c * cstep;
        PA(double, ring, TL_SYNTH_BATCH); PV(double, q); PV(double, qprev);
        TL_LANES_BEGIN
        for (int i = 0; i < TL_SYNTH_BATCH; i++) L(ring)[i] = 0.0;
        L(q) = 0.0; L(qprev) = 0.0;
        TL_LANES_END
        // batch 0: the last 15 sample vectors of the slot before (its rounds 7..11); batches 1..3: rounds 0..4, 5..9, 10..11 of the slot itself
#pragma unroll 1
        for (int b = 0; b < 4; b++) {
            const int nvec = b < 3 ? TL_SYNTH_BATCH : 36 - 2 * TL_SYNTH_BATCH;
            if (b == 0 && !hist) {
                TL_LANES_BEGIN
                for (int i = lane; i < TL_SYNTH_BATCH * 32; i += 64) w.s[i] = 0.0;
                TL_LANES_END
            } else if (b == 0) tl_requantise(w, w.d[0].frame, B, K, Y, sdp, xp, c, 7, 12);
            else tl_requantise(w, w.d[1].frame, B, K, Y, sd, xc, c, 5 * (b - 1), b < 3 ? 5 * b : 12);
#pragma unroll
            for (int u = 0; u < TL_SYNTH_BATCH; u++) {
                if (u >= nvec) continue;                                  // (the last batch is six vectors)
                const double *sv = w.s + u * 32;
                TL_LANES_BEGIN
                // matrixing: V_t[lane] = sum_k N[lane][k] S_t[k]; every lane reads the same 32 samples (LDS broadcasts, 16 bytes each), four partial sums
                double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
                for (int k = 0; k < 32; k += 8) {
                    double s0, s1, s2, s3, s4, s5, s6, s7;
                    TL_LD2(sv + k, s0, s1); TL_LD2(sv + k + 2, s2, s3); TL_LD2(sv + k + 4, s4, s5); TL_LD2(sv + k + 6, s6, s7);
                    a0 += L(nk)[k] * s0; a1 += L(nk)[k + 1] * s1; a2 += L(nk)[k + 2] * s2; a3 += L(nk)[k + 3] * s3;
                    a0 += L(nk)[k + 4] * s4; a1 += L(nk)[k + 5] * s5; a2 += L(nk)[k + 6] * s6; a3 += L(nk)[k + 7] * s7;
                    TL_SCHED_FENCE();                                   // eight samples in flight, not thirty-two: their registers are the kernel's margin
                }
                L(ring)[u] = (a0 + a1) + (a2 + a3);
                // windowing: this lane's eight terms, V_t, V_{t-2}, ... V_{t-14} (the ring holds the last 15 vectors: slot (t mod 15))
                double b0 = 0.0, b1 = 0.0;
#pragma unroll
                for (int i = 0; i < 8; i += 2) {
                    b0 += dwin[lane + 64 * i] * L(ring)[(u + 2 * TL_SYNTH_BATCH - 2 * i) % TL_SYNTH_BATCH];
                    b1 += dwin[lane + 64 * i + 64] * L(ring)[(u + 2 * TL_SYNTH_BATCH - 2 - 2 * i) % TL_SYNTH_BATCH];
                }
                L(q) = b0 + b1;
                TL_LANES_END
                if (b > 0) {
                    TL_LANES_BEGIN
                    const double hi = TL_OTHER(qprev, , (lane + 32) & 63);      // (every lane takes part in the exchange)
                    if (lane < 32) {
                        double x = (L(q) + hi) * 32768.0;
                        x = rint(x);
                        x = x > 32767.0 ? 32767.0 : x < -32768.0 ? -32768.0 : x;
                        oc[(((b - 1) * TL_SYNTH_BATCH + u) * 32 + lane) * sstep] = (int16_t)(int)x;
                    }
                    TL_LANES_END
                }
                TL_LANES_BEGIN L(qprev) = L(q); TL_LANES_END
            }
        }
    }
}

// ---- the unit of stage B: slot f of stream s -> 2 x 1152 samples.  Reads the reports stage A wrote for this slot and the one before. ----
TL_FN void tl_synth_unit(TlSynthLds &w, const TlDecLaunch &A, int s, int f, const double *TL_RESTRICT dwin)
{
    const TlConfig *C = &A.configs[A.stream_cfg ? A.stream_cfg[s] : 0];
    const TlBlockShared *B = &A.tables->shared;
    const TlPackTables *K = &A.tables->pack;
    const TlSynthTables *Y = A.synth;
    const int nch = C->nch;
    const size_t slot = (size_t)f * A.nstreams + s;
    int16_t *out = A.pcm + slot * 2 * 1152;
    if (A.report[slot].status & (TL_DEC_BAD_MASK | TL_DEC_EMPTY)) { tl_synth_zero(out, 2 * 1152); return; }
    if (nch == 1) tl_synth_zero(out + 1152, 1152);

    TlDecSide sdp, sd;
    TlDecCells xp, xc;
    bool hist = false;
    {   // the slot before: in this launch, or what the launch before left
        const uint8_t *psrc; int plen; uint32_t pst;
        if (f > 0) {
            const size_t ps = slot - (size_t)A.nstreams;
            psrc = A.frames + ps * A.out_stride; plen = A.len ? A.len[ps] : A.out_stride; pst = A.report[ps].status;
        } else { psrc = A.prev + (size_t)s * A.out_stride; plen = A.state[s].prev_len; pst = A.state[s].prev_status; }
        plen = plen < A.out_stride ? plen : A.out_stride;
        hist = plen > 0 && !(pst & (TL_DEC_BAD_MASK | TL_DEC_EMPTY));
        if (hist) {
            tl_dec_load(w.d[0], psrc, plen);
            tl_dec_side<false>(w.d[0], B, K, C, plen, sdp, xp.ba, xp.qi, xp.scf, xp.sel, xp.o_smp);
        }
    }
    {
        int len = A.len ? A.len[slot] : A.out_stride;
        len = len < A.out_stride ? len : A.out_stride;
        tl_dec_load(w.d[1], A.frames + slot * A.out_stride, len);
        tl_dec_side<false>(w.d[1], B, K, C, len, sd, xc.ba, xc.qi, xc.scf, xc.sel, xc.o_smp);
    }
    tl_synth_frame(w, B, K, Y, nch, hist, sdp, xp, sd, xc, out, 1152, 1, dwin);
}
