// mp2_probe_stage.h -- TEST BUILDS ONLY: the third probe family, the shared stage helpers of mp2_dbsum.h called one by one.  (The first two
// families -- the libm forms and the wave primitives -- are in mp2_probe.h; this header is its continuation and is included from there.)
//
// Every stage calls the helpers of mp2_dbsum.h: dB sums, masking terms, masker spans, the row minimum, the allocation key, the scalefactor
// index, the exact division, the bit writer and the CRC step.  Whole frames see an error there only when it tips a decision; the bodies
// below call each helper alone, the way the stage headers do: the dB-sum table is the kernels' own dblog[0..1001] in LDS, the scalefactor
// table the block's LDS copy, masker records are TlMasker made by tl_masker_consts where TL_MK4 lies, the bark list lies where TL_MK_BARK
// lies (with TL_LTG behind it: the readable slack tl_mask_spans_sorted relies on), the frame is a zeroed LDS frame written by all lanes.
// One layer up, the last form calls the bit allocation alone (mp2_alloc.h: tl_allocate, tl_allocate_pair), one wave per case, with the per-lane
// constants made as tl_encode_frame / tl_encode_pair make them (mp2_pack.h) and B the workgroup's LDS copy of TlBlockShared: whole frames seldom
// bring exact ties between cells, a budget that ends on a round's sum, or a refusal followed by a cheaper admission.
// Lane-SPMD text: it runs on the device (csrc/toolame_probe.hip) and, with -DTL_EMULATE, on the host (tests/emu/mp2_probe_emu.cpp).
// tests/probelib.py holds the argument sets and the oracles.
#pragma once
#include "mp2_host.h"
#include "mp2_wave.h"

// n = lane-arguments (one lane each) for the first group, cases (one wave each) for the second.  d = double, i = int32, u = uint32, U = uint64.
enum {
    TLS_ADD_DB = 0,     // in0 d[n] a, in1 d[n] b -> out0 d[n] tl_add_db(a, b); out1 d[4 n]: tl_add_db2 of (pair i, pair j), tl_add_db2_k of the same
                        // with k1000 from tl_mask_consts -- j = i ^ 1 (i itself where that is past the end): two independent pairs per lane
    TLS_MASK,           // in0 d[n] masker level x, in1 d[n] masker bark, in2 d[4 n]: line bark, running x0, tonal (0 | 1), live (0 | 1)
                        // -> out1 d[5 n] the record of tl_masker_consts; out0 d[8 n]: tl_mask_term(live), (!live), tl_mask_term_k(live), (!live),
                        // tl_mask_term_w(live), (!live), tl_mask_step(x0), 0
    TLS_MNR_KEY,        // in0 d[n] -> out0 U[n]
    TLS_SF_INDEX,       // in0 d[n] -> out0 i[2 n]: tl_sf_index, tl_sf_index_ref; out1 i[n]: tl_sfs_count(i)
    TLS_DIV_BY,         // in0 d[n] s, in1 d[n] d -> out0 d[n] tl_div_by(s, d, 1.0 / d made in the kernel: the quantiser), out1 d[n] tl_div_by(s, d, r) with
                        // r = 1.0 / d made on the HOST by the entry point (TlConfig::p1_linerw: the noise weights)
    TLS_LANE_FORMS,
    TLS_SPANS = TLS_LANE_FORMS,   // in0 d[192 n] the bark list and the slack behind it, in1 d[128 n] (blo, bhi) per lane, in2 i[2 n] ntone, nnoise
                        // -> out0 i[512 n] per lane a0 a1 b0 b1 of tl_mask_spans, then of tl_mask_spans_sorted<64, 32> (-2 where the caller's gate
                        // keeps it out); out1 i[2 n]: tl_maskers_sorted, the gate's decision
    TLS_MIN_ROWS,       // in0 d[136 n] the column (TL_LTG), in1 d[64 n] m, in2 i[192 n] per lane j0, n, take_first -> out0 d[64 n]
    TLS_BITS,           // in0 U[384 n] six field values per lane, in1 i[384 n] their lengths (0: no field), in2 i[2 n] start offset 0..63, wide (0: tl_put_bits,
                        // 1: tl_put_bits48) -> out0 u[3 F n]: the frame's F words, the same read through tl_get_bit, tl_bswap of each;
                        // out1 u[128 n] per lane tl_crc_upd over its own fields: CRC-16, ScF-CRC
    TLS_ALLOC,          // in0 d[64 n] the SMR of every lane, in1 i[64 n] its scfsi 0..3 (lane = 2 sb + ch; pair call: lane = 2 sb + unit), in2 i[8 n]:
                        // allocation table 0..4, nch, jsbound, call (0: tl_allocate, 1: tl_allocate_pair -- two mono streams), adb, adb of unit 1
                        // (pair call), 0, 0 -- adb as tl_encode_frame passes it: the frame's bits before bbal + 16 + 32 is taken off
                        // -> out0 i[64 n] ba of every lane (0 in a dead one); out1 i[n] the bits left that tl_allocate returns (0 for the pair call)
    TLS_NFORMS
};
#define TLS_LIST 192                                  /* TL_MASKER_MAX barks + 64 of slack: tl_mask_spans_sorted<64, 32> reads up to [ntone + 62] <= [189] */
#define TLS_ROWS 136                                  /* TL_LTG */
#define TLS_FIELDS 6
#define TLS_FRAME_WORDS (TL_MAX_FRAME_WORDS + 2)      /* TlMainLds::u.frame */
// the two parameter sets of the encoder's CRCs (mp2_pack.h: CRC-16 x^16+x^15+x^2+1 over header, allocation and scfsi, crc.c:12-56; ScF-CRC
// x^8+x^4+x^3+x^2+1, crc.c:58-113 -- the polynomials TlPackTables::crc_xpow / crc8_xpow are the powers of)
#define TLS_CRC16_POLY 0x8005u
#define TLS_CRC16_TOP 0x8000u
#define TLS_CRC8_POLY 0x1du
#define TLS_CRC8_TOP 0x80u

// A probe wave's LDS: the transform buffer of TlPsyLds (TL_MK_X, TL_MK_BARK, TL_LTG, TL_MK4 apply as they are) and a frame as in TlMainLds.
struct alignas(16) TlStageLds {
    struct { double fft[TL_FFT_WORDS]; } u;
    uint32_t frame[TLS_FRAME_WORDS];
};

// line, nbal and sblimit of the five allocation tables, as tl_build_config leaves them in TlConfig (mp2_host.cpp): read from a configuration
// that selects each table.  Global memory on the device, as the configuration record is.
struct TlsAllocTab { int32_t sblimit[5]; uint8_t line[5][32], nbal[5][32]; };
static inline const TlsAllocTab *tls_alloc_tab()
{
    static TlsAllocTab A;
    static TlConfig C;
    static bool built = false;
    if (!built) {
        static const struct { long fs; char mode; int kbps; } pick[5] = {{48000, 's', 192}, {32000, 's', 192}, {48000, 'm', 48}, {32000, 'm', 48}, {24000, 's', 64}};
        for (int t = 0; t < 5; t++) {
            if (tl_build_config(&C, pick[t].fs, pick[t].mode, pick[t].kbps, 1, 0) != TL_OK || C.tab != t) return nullptr;
            A.sblimit[t] = C.sblimit;
            for (int sb = 0; sb < 32; sb++) { A.line[t][sb] = C.line[sb]; A.nbal[t][sb] = C.nbal[sb]; }
        }
        built = true;
    }
    return &A;
}

// element counts (in bytes) of the five arrays of a call; 0: the form has no such array
static inline void tls_bytes(int form, long n, size_t by[5])
{
    const size_t N = (size_t)n;
    by[0] = by[1] = by[2] = by[3] = by[4] = 0;
    switch (form) {
    case TLS_ADD_DB: by[0] = by[1] = by[3] = 8 * N; by[4] = 32 * N; break;
    case TLS_MASK: by[0] = by[1] = 8 * N; by[2] = 32 * N; by[3] = 64 * N; by[4] = 40 * N; break;
    case TLS_MNR_KEY: by[0] = by[3] = 8 * N; break;
    case TLS_SF_INDEX: by[0] = 8 * N; by[3] = 8 * N; by[4] = 4 * N; break;
    case TLS_DIV_BY: by[0] = by[1] = by[3] = by[4] = 8 * N; break;
    case TLS_SPANS: by[0] = 8 * TLS_LIST * N; by[1] = 8 * 128 * N; by[2] = 8 * N; by[3] = 4 * 512 * N; by[4] = 8 * N; break;
    case TLS_MIN_ROWS: by[0] = 8 * TLS_ROWS * N; by[1] = 8 * 64 * N; by[2] = 4 * 192 * N; by[3] = 8 * 64 * N; break;
    case TLS_BITS: by[0] = 8 * 64 * TLS_FIELDS * N; by[1] = 4 * 64 * TLS_FIELDS * N; by[2] = 8 * N; by[3] = 4 * 3 * TLS_FRAME_WORDS * N; by[4] = 4 * 128 * N; break;
    case TLS_ALLOC: by[0] = 8 * 64 * N; by[1] = 4 * 64 * N; by[2] = 4 * 8 * N; by[3] = 4 * 64 * N; by[4] = 4 * N; break;
    }
}
static inline long tls_max_n(int form) { return form < TLS_LANE_FORMS ? (1l << 26) : (1l << 16); }

// The stated domain of each form, checked on the HOST before anything is queued: several helpers make LDS indexes from their arguments.
// Written on the bits: no NaN passes.
static inline bool tls_mag_le(double v, double lim) { return (tlm_d2u(v) & 0x7fffffffffffffffull) <= tlm_d2u(lim); }      // finite, |v| <= lim (lim > 0)
static inline bool tls_in_0_to(double v, double lim) { return tlm_d2u(v) <= tlm_d2u(lim); }                              // +0 <= v <= lim
static inline bool tls_in_domain(int form, long n, const void *in0, const void *in1, const void *in2)
{
    const double *a = (const double *)in0, *b = (const double *)in1, *c = (const double *)in2;
    const int32_t *ib = (const int32_t *)in1, *ic = (const int32_t *)in2;
    const double db_lim = 262144.0;                                          // 2^18: covers the "out of reach" level (high word 0xC0F00000); 10 (a - b) fits an int
    switch (form) {
    case TLS_ADD_DB:
        for (long i = 0; i < n; i++) if (!tls_mag_le(a[i], db_lim) || !tls_mag_le(b[i], db_lim)) return false;
        return true;
    case TLS_MASK:
        for (long i = 0; i < n; i++) {
            if (!tls_mag_le(a[i], db_lim) || !tls_in_0_to(b[i], 32.0) || !tls_in_0_to(c[4 * i], 32.0) || !tls_mag_le(c[4 * i + 1], db_lim)) return false;
            if (!(c[4 * i + 2] == 0.0 || c[4 * i + 2] == 1.0) || !(c[4 * i + 3] == 0.0 || c[4 * i + 3] == 1.0)) return false;
        }
        return true;
    case TLS_MNR_KEY:
        for (long i = 0; i < n; i++) if ((tlm_d2u(a[i]) & 0x7fffffffffffffffull) >= 0x7ff0000000000000ull) return false;       // finite
        return true;
    case TLS_SF_INDEX:
        for (long i = 0; i < n; i++) if (!(tlm_d2u(a[i]) < tlm_d2u(2.0))) return false;                                       // +0 <= cur_max < 2
        return true;
    case TLS_DIV_BY:                                                         // the divisors and dividends of tests/test_emu_parity.py test_quantiser_division
        for (long i = 0; i < n; i++) {
            const uint64_t ud = tlm_d2u(b[i]), ms = tlm_d2u(a[i]) & 0x7fffffffffffffffull, frac = ud & 0xfffffffffffffull;
            if (!(ud >= tlm_d2u(1e-20) && ud <= tlm_d2u(200.0)) || frac == 0xfffffffffffffull) return false;                  // (Markstein's exception: a significand of all ones)
            if (!(ms == 0 || (ms >= tlm_d2u(0x1p-200) && ms <= tlm_d2u(0x1p20)))) return false;
        }
        return true;
    case TLS_SPANS:
        for (long k = 0; k < n; k++) {
            const int nt = ic[2 * k], nn = ic[2 * k + 1];
            if (nt < 0 || nn < 0 || nt > TL_MASKER_MAX || nn > TL_MASKER_MAX || nt + nn > TL_MASKER_MAX) return false;
            for (int q = 0; q < TLS_LIST; q++) {
                const double v = a[TLS_LIST * k + q];
                if (q < nt + nn ? !tls_in_0_to(v, 32.0) : !tls_mag_le(v, 1e300)) return false;                               // a bark; behind the list anything finite
            }
            for (int q = 0; q < 128; q++) if (!tls_mag_le(b[128 * k + q], 1e300)) return false;
        }
        return true;
    case TLS_MIN_ROWS:
        for (long k = 0; k < n; k++) {
            for (int q = 0; q < TLS_ROWS; q++) if (!tls_mag_le(a[TLS_ROWS * k + q], 1e300)) return false;
            for (int l = 0; l < 64; l++) {
                const int32_t *r = ic + 192 * k + 3 * l;
                if (!tls_mag_le(b[64 * k + l], 1e300) || r[0] < 0 || r[0] >= TLS_ROWS || r[1] < 1 || r[1] > TLS_ROWS || r[0] + r[1] > TLS_ROWS || (r[2] != 0 && r[2] != 1)) return false;
            }
        }
        return true;
    case TLS_BITS:
        for (long k = 0; k < n; k++) {
            const int start = ic[2 * k], wide = ic[2 * k + 1];
            if (start < 0 || start > 63 || (wide != 0 && wide != 1)) return false;
            long end = start;
            for (int q = 0; q < 64 * TLS_FIELDS; q++) {
                const int nb = ib[64 * TLS_FIELDS * k + q];
                const uint64_t v = ((const uint64_t *)in0)[64 * TLS_FIELDS * k + q];
                if (nb < 0 || nb > (wide ? 48 : 32) || (v >> nb) != 0) return false;                                          // (nb <= 48: the shift is defined)
                end += nb;
            }
            if (end > TL_MAX_FRAME_BYTES * 8) return false;                                                                  // every field ends inside the frame
        }
        return true;
    case TLS_ALLOC: {
        const TlsAllocTab *A = tls_alloc_tab();
        if (!A) return false;
        for (long k = 0; k < n; k++) {
            const int32_t *p = ic + 8 * k;
            const int tab = p[0], nch = p[1], jsb = p[2], call = p[3];
            if (tab < 0 || tab > 4 || (nch != 1 && nch != 2) || (call != 0 && call != 1) || (call == 1 && nch != 1)) return false;
            const int sbl = A->sblimit[tab];
            if (jsb != 4 && jsb != 8 && jsb != 12 && jsb != 16 && jsb != sbl) return false;                                   // (above sblimit: joint stereo with tables 2 and 3)
            int bbal = 0;
            for (int sb = 0; sb < sbl; sb++) bbal += A->nbal[tab][sb] * (sb < jsb ? nch : 1);
            for (int u = 0; u <= call; u++) if (p[4 + u] < bbal + 48 || p[4 + u] > 8 * TL_MAX_FRAME_BYTES) return false;    // the budget tl_build_config lets through
            for (int l = 0; l < 64; l++) {
                if (ib[64 * k + l] < 0 || ib[64 * k + l] > 3) return false;
                if (!tls_mag_le(a[64 * k + l], 1000.0)) return false;                                                        // every MNR far from the reference's 999999.0
            }
        }
        return true;
    }
    }
    return false;
}

// 64 lane-arguments from i0 on (those below n).  db: dblog[0..1001], sf: the scalefactor table -- both the workgroup's LDS copies on the device.
TL_FN void tl_probe_stage_lanes(int form, TlStageLds &w, const double *db, const double *sf, long i0, long n,
                                const void *in0, const void *in1, const void *in2, void *out0, void *out1)
{
    const double *a = (const double *)in0, *b = (const double *)in1, *c = (const double *)in2;
    switch (form) {
    case TLS_ADD_DB:
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) {
            const long j = (i ^ 1) < n ? (i ^ 1) : i;
            double *o0 = (double *)out0, *o1 = (double *)out1;
            o0[i] = tl_add_db(db, a[i], b[i]);
            double p0 = a[i], p1 = a[j];
            tl_add_db2(db, p0, b[i], p1, b[j]);
            const TlMaskK kk = tl_mask_consts();
            double q0 = a[i], q1 = a[j];
            tl_add_db2_k(db, kk.k1000, q0, b[i], q1, b[j]);
            o1[4 * i] = p0; o1[4 * i + 1] = p1; o1[4 * i + 2] = q0; o1[4 * i + 3] = q1;
        }
        TL_LANES_END
        break;
    case TLS_MASK:
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) {
            TL_MK_X(w)[lane] = a[i]; TL_MK_BARK(w)[lane] = b[i];
            tl_masker_consts(TL_MK4(w), TL_MK_X(w), TL_MK_BARK(w), lane, c[4 * i + 2] != 0.0);
        }
        TL_LANES_END
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) {
            const TlMasker *m = &TL_MK4(w)[lane];
            const double mb = m->bark, av = m->av, g = m->g, nn = m->n, lb = c[4 * i], x0 = c[4 * i + 1];
            const bool live = c[4 * i + 3] != 0.0;
            const double dz = lb - mb, dzp = mb - lb;                       // (the walks form mb - line bark: mp2_psy13.h)
            const TlMaskK kk = tl_mask_consts();
            double *o0 = (double *)out0 + 8 * i, *o1 = (double *)out1 + 5 * i;
            o0[0] = tl_mask_term(dz, av, g, nn, live); o0[1] = tl_mask_term(dz, av, g, nn, !live);
            o0[2] = tl_mask_term_k(kk, dz, av, g, nn, live); o0[3] = tl_mask_term_k(kk, dz, av, g, nn, !live);
            o0[4] = tl_mask_term_w(m, dzp, av, kk.far_hi, live); o0[5] = tl_mask_term_w(m, dzp, av, kk.far_hi, !live);
            o0[6] = tl_mask_step(db, x0, m, dzp, av, kk.far_hi); o0[7] = 0.0;
            o1[0] = mb; o1[1] = av; o1[2] = g; o1[3] = m->c17; o1[4] = nn;
        }
        TL_LANES_END
        break;
    case TLS_MNR_KEY:
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) ((uint64_t *)out0)[i] = tl_mnr_key(a[i]);
        TL_LANES_END
        break;
    case TLS_SF_INDEX:
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) {
            int32_t *o0 = (int32_t *)out0, *o1 = (int32_t *)out1;
            o0[2 * i] = (int32_t)tl_sf_index(sf, a[i]); o0[2 * i + 1] = (int32_t)tl_sf_index_ref(sf, a[i]);
            o1[i] = tl_sfs_count((unsigned)i);
        }
        TL_LANES_END
        break;
    case TLS_DIV_BY:
        TL_LANES_BEGIN
        const long i = i0 + lane;
        if (i < n) {
            const double rk = 1.0 / b[i];                                    // as the quantiser makes it (mp2_pack.h: q_rsf)
            ((double *)out0)[i] = tl_div_by(a[i], b[i], rk);
            ((double *)out1)[i] = tl_div_by(a[i], b[i], c[i]);               // as the noise weights get it: made on the host
        }
        TL_LANES_END
        break;
    default: break;
    }
}

// one case, one wave (the helper forms; the allocation form has a body of its own below: it takes the tables the helpers do not)
TL_FN void tl_probe_stage_case(int form, TlStageLds &w, long k, const void *in0, const void *in1, const void *in2, void *out0, void *out1)
{
    const int32_t *ic = (const int32_t *)in2;
    switch (form) {
    case TLS_SPANS: {
        const double *list = (const double *)in0 + TLS_LIST * k, *bnd = (const double *)in1 + 128 * k;
        const int ntone = TL_UNI_I(ic[2 * k]), nnoise = TL_UNI_I(ic[2 * k + 1]), nm = ntone + nnoise;
        TL_LANES_BEGIN
        for (int q = lane; q < TL_MASKER_MAX; q += 64) TL_MK_X(w)[q] = 0.0;
        for (int q = lane; q < TLS_LIST; q += 64) TL_MK_BARK(w)[q] = list[q];                   // ([128..191] is the head of TL_LTG: what lies behind the list in the kernels)
        TL_LANES_END
        TL_LANES_BEGIN
        for (int t = lane; t < TL_MASKER_MAX; t += 64) {
            if (t < nm) tl_masker_consts(TL_MK4(w), TL_MK_X(w), TL_MK_BARK(w), t, t < ntone);
            else TL_MK4(w)[t].bark = TL_MK_BARK(w)[t];                                            // a stale record past the list
        }
        TL_LANES_END
        const bool sorted = tl_maskers_sorted(TL_MK_BARK(w), ntone, nnoise);
        const bool srt = ntone < 128 && nnoise < 64 && sorted;                                    // the callers' gate (mp2_psy13.h)
        TL_LANES_BEGIN
        const double blo = bnd[2 * lane], bhi = bnd[2 * lane + 1];
        int32_t *o = (int32_t *)out0 + 512 * k + 8 * lane;
        int a0, a1, b0, b1;
        tl_mask_spans(TL_MK4(w), nm, ntone, blo, bhi, a0, a1, b0, b1);
        o[0] = a0; o[1] = a1; o[2] = b0; o[3] = b1;
        a0 = a1 = b0 = b1 = -2;
        if (srt) tl_mask_spans_sorted<64, 32>(TL_MK_BARK(w), ntone, nnoise, blo, bhi, a0, a1, b0, b1);
        o[4] = a0; o[5] = a1; o[6] = b0; o[7] = b1;
        if (lane == 0) { ((int32_t *)out1)[2 * k] = sorted ? 1 : 0; ((int32_t *)out1)[2 * k + 1] = srt ? 1 : 0; }
        TL_LANES_END
    } break;
    case TLS_MIN_ROWS: {
        const double *col = (const double *)in0 + TLS_ROWS * k, *m0 = (const double *)in1 + 64 * k;
        TL_LANES_BEGIN
        for (int q = lane; q < TLS_ROWS; q += 64) TL_LTG(w)[q] = col[q];
        TL_LANES_END
        TL_LANES_BEGIN
        const int32_t *r = ic + 192 * k + 3 * lane;
        ((double *)out0)[64 * k + lane] = tl_min_rows(TL_LTG(w), r[0], r[1], m0[lane], r[2] != 0);
        TL_LANES_END
    } break;
    case TLS_BITS: {
        const uint64_t *val = (const uint64_t *)in0 + 64 * TLS_FIELDS * k;
        const int32_t *len = (const int32_t *)in1 + 64 * TLS_FIELDS * k;
        const int start = TL_UNI_I(ic[2 * k]), wide = TL_UNI_I(ic[2 * k + 1]);
        uint32_t *frame = w.frame;
        PV(int, tot); PV(int, off);
        TL_LANES_BEGIN
        for (int q = lane; q < TLS_FRAME_WORDS; q += 64) frame[q] = 0;
        int t = 0;
        for (int f = 0; f < TLS_FIELDS; f++) t += len[TLS_FIELDS * lane + f];
        L(tot) = t;
        TL_LANES_END
        TL_WAVE_EXSCAN_I32(off, tot);                                        // lane l's first field follows lane l - 1's last
        TL_LANES_BEGIN
        int pos = start + L(off);
        unsigned c16 = 0xffffu, c8 = 0;
        for (int f = 0; f < TLS_FIELDS; f++) {
            const uint64_t v = val[TLS_FIELDS * lane + f];
            const int nb = len[TLS_FIELDS * lane + f];
            if (wide) { if (nb) tl_put_bits48(frame, pos, v, nb); }          // (its callers skip an empty field)
            else tl_put_bits(frame, pos, (uint32_t)v, nb);
            const int hi = nb > 32 ? nb - 32 : 0;
            c16 = tl_crc_upd(c16, (unsigned)(v >> 32), hi, TLS_CRC16_POLY, TLS_CRC16_TOP); c16 = tl_crc_upd(c16, (unsigned)v, nb - hi, TLS_CRC16_POLY, TLS_CRC16_TOP);
            c8 = tl_crc_upd(c8, (unsigned)(v >> 32), hi, TLS_CRC8_POLY, TLS_CRC8_TOP); c8 = tl_crc_upd(c8, (unsigned)v, nb - hi, TLS_CRC8_POLY, TLS_CRC8_TOP);
            pos += nb;
        }
        ((uint32_t *)out1)[128 * k + 2 * lane] = c16 & 0xffffu; ((uint32_t *)out1)[128 * k + 2 * lane + 1] = c8 & 0xffu;
        TL_LANES_END
        TL_LANES_BEGIN
        uint32_t *o = (uint32_t *)out0 + 3 * TLS_FRAME_WORDS * k;
        for (int q = lane; q < TLS_FRAME_WORDS; q += 64) {
            const uint32_t word = frame[q];
            uint32_t u = 0;
            for (int bit = 0; bit < 32; bit++) u = (u << 1) | tl_get_bit(frame, 32 * q + bit);
            o[q] = word; o[TLS_FRAME_WORDS + q] = u; o[2 * TLS_FRAME_WORDS + q] = tl_bswap(word);
        }
        TL_LANES_END
    } break;
    default: break;
    }
}

// one case of TLS_ALLOC, one wave.  B: the workgroup's LDS copy of TlBlockShared on the device, A: the allocation tables
// hist: tl_allocate's 64 scratch words -- TlStageLds::frame on the device; the emulation's entry point passes none and gets a local array
TL_FN void tl_probe_alloc_case(const TlBlockShared *TL_RESTRICT B, const TlsAllocTab *TL_RESTRICT A, long k, const void *in0, const void *in1, const void *in2, void *out0, void *out1,
                               uint32_t *hist = nullptr)
{
#ifdef TL_EMULATE
    uint32_t hist_own[64];
    if (!hist) hist = hist_own;
#endif
    const int32_t *ic = (const int32_t *)in2;
    const double *smr = (const double *)in0 + 64 * k;
    const int32_t *sel = (const int32_t *)in1 + 64 * k, *p = ic + 8 * k;
    const int tab = TL_UNI_I(p[0]), nch = TL_UNI_I(p[1]), jsbound = TL_UNI_I(p[2]), call = TL_UNI_I(p[3]), adb0 = TL_UNI_I(p[4]), adb1 = TL_UNI_I(p[5]);
    const int sblimit = TL_UNI_I(A->sblimit[tab]);
    // the per-lane constants as the encoder makes them (mp2_pack.h: a_ln / a_nbal from the configuration's line and nbal, a_sfs / a_sfs_o from
    // the cell's and the partner channel's scfsi)
    PV(int, a_ln); PV(int, a_nbal); PV(int, a_sfs); PV(int, a_sfs_o); PV(double, a_smr); PV(int, ba);
    int left = 0;
    if (call == 0) {
        TL_LANES_BEGIN
        const int c = lane & 1, sb = lane >> 1;
        const bool live = c < nch && sb < sblimit;
        L(a_ln) = live ? A->line[tab][sb] : 0;
        L(a_nbal) = live ? A->nbal[tab][sb] : 0;
        L(a_sfs) = live ? 6 * tl_sfs_count((unsigned)sel[lane]) : 0;
        L(a_sfs_o) = (live && nch == 2) ? 6 * tl_sfs_count((unsigned)sel[lane ^ 1]) : 0;
        L(a_smr) = live ? smr[lane] : 0.0;
        TL_LANES_END
        left = tl_allocate(B, adb0, nch, sblimit, jsbound, a_ln, a_nbal, a_sfs, a_sfs_o, a_smr, ba, hist);
    } else {
        TL_LANES_BEGIN
        const int sb = lane >> 1;
        const bool live = sb < sblimit;
        L(a_ln) = live ? A->line[tab][sb] : 0;
        L(a_nbal) = live ? A->nbal[tab][sb] : 0;
        L(a_sfs) = live ? 6 * tl_sfs_count((unsigned)sel[lane]) : 0;
        L(a_smr) = live ? smr[lane] : 0.0;
        TL_LANES_END
        tl_allocate_pair(B, adb0, adb1, sblimit, a_ln, a_nbal, a_sfs, a_smr, ba);
    }
    TL_LANES_BEGIN
    ((int32_t *)out0)[64 * k + lane] = L(ba);
    if (lane == 0) ((int32_t *)out1)[k] = left;
    TL_LANES_END
}
