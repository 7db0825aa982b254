// mp2_probe.h -- TEST BUILDS ONLY: the device halves of tl_libm.h and of mp2_wave.h's block "where the two part", called one by one.
//
// Every byte-identical claim of the encoder rests on those two headers, and each has a host half and a device half that differ in source
// text (hardware seeds, inline v_fma_f64 / v_min_f64 / v_max_f64, tables in LDS or rearranged, DPP / permlane / ballot exchanges).  The
// bodies below call each form and each primitive the way the stage headers do, in the same lane-SPMD style (TL_LANES_BEGIN/END, PV, L()),
// so the one text runs on the device (csrc/toolame_probe.hip, linked into the fault-injection TEST library alone) and with -DTL_EMULATE on
// the host (tests/emu/mp2_probe_emu.cpp).  tests/probelib.py holds the argument sets and the oracles, tests/test_probe_emu.py compares the
// emulation with glibc and with the oracles, tests/test_probe_gpu.py the device with the emulation.  The product library has none of this.
// The third family -- the shared stage helpers of mp2_dbsum.h, one by one -- has a header of its own, mp2_probe_stage.h, included at the end.
#pragma once
#include "mp2_wave.h"

// ---- (a) the libm forms: one lane per argument; a[i] (and b[i]) in, r0[i] (and r1[i]) out
enum {
    TLP_LOG_PN = 0,          // tlm_log_pn(a, tab)                                                        table: 0 global, 1 LDS copy
    TLP_LOG10_PN,            // tlm_log10_pn(a, tab)                                                      table: 0 | 1
    TLP_LOG10_SPLIT,         // tlm_log10_main_pn, or tlm_log10_near1_pn where it says so (tl_power_db_main / tl_power_near1)   table: 0 | 1
    TLP_POW10_SL,            // tlm_pow10_sl(a)
    TLP_EXP_SL,              // tlm_exp_sl<false>(a, 0.0)
    TLP_SINCOS_SL,           // tlm_sincos_sl(a, &r0, &r1, tlm_sincostab)
    TLP_SINCOS_PHASED,       // tlm_sincos_reduce -> _poly -> _finish, the row through TL_SCT, fences between the phases
    TLP_SINCOS_PHASED_RAW,   // the same with _finish_raw for a and for b (the predicted phase) and the caller's exchange (mp2_psy24.h, the line loop):
                             // r0 / r1 = sine / cosine of a where b's quadrant is even, cosine / sine where it is odd
    TLP_ATAN2_PHASED,        // tlm_atan2_head -> _mid -> _tail of (a = y, b = x), the row from tlm_atan_cij as the line loop loads it
    TLP_ATAN2_NS,            // tlm_atan2_sl<false>(a = y, b = x, tlm_atan_cij)
    TLP_DIV_NS,              // tlm_div_ns(a, b)
    TLP_SQRT_NS,             // tlm_sqrt_ns(a)
    TLP_SQRT_NZ,             // tlm_sqrt_nz(a)
    TLP_RCP_SEED,            // tlm_rcp_seed(a): the raw seed (the two halves differ here BY DESIGN: the refinement's precondition is its error)
    TLP_RSQ_SEED,            // tlm_rsq_seed(a)
    TLP_DIV,                 // a / b as the compiler expands it
    TLP_SQRT,                // __builtin_sqrt(a) as the compiler expands it
    TLP_MIN_NN,              // TLM_MIN_NN(a, b)
    TLP_MAX_NN,              // TLM_MAX_NN(a, b)
    TLP_FMA_K,               // TLM_FMA_K(a, b, d3 of e_atan2.c): one Horner step
    TLP_RECIP,               // tlm_recip_from(a, tlm_rcp_seed(a)): the refined reciprocal every quotient by one divisor shares.  Not bit-equal between
                             // the halves either (it starts from the seed); its check is |a r - 1| <= 2^-52.  The quotients themselves come out
                             // correctly rounded from a reciprocal far worse than that, so THEY cannot say whether the refinement is whole
    TLP_NFORMS
};
static inline bool tlp_two_in(int form)
{
    return form == TLP_SINCOS_PHASED_RAW || form == TLP_ATAN2_PHASED || form == TLP_ATAN2_NS || form == TLP_DIV_NS || form == TLP_DIV ||
           form == TLP_MIN_NN || form == TLP_MAX_NN || form == TLP_FMA_K;
}
static inline bool tlp_two_out(int form) { return form == TLP_SINCOS_SL || form == TLP_SINCOS_PHASED || form == TLP_SINCOS_PHASED_RAW; }
static inline bool tlp_has_table(int form) { return form == TLP_LOG_PN || form == TLP_LOG10_PN || form == TLP_LOG10_SPLIT; }

// The stated domain of each form (tl_libm.h, at the form): checked on the HOST before anything is queued, so that no table index made from
// an argument outside it ever reaches the device.  Written on the bits: no NaN passes a test it is not meant to pass.
static inline bool tlp_in_domain(int form, double a, double b)
{
    const uint64_t ua = tlm_d2u(a), ub = tlm_d2u(b), ma = ua & 0x7fffffffffffffffull, mb = ub & 0x7fffffffffffffffull;
    const uint64_t inf = 0x7ff0000000000000ull, minn = 0x0010000000000000ull;
    const uint64_t p500 = 0x5f30000000000000ull, m500 = 0x20b0000000000000ull, m900 = 0x07b0000000000000ull, m443 = 0x2440000000000000ull;   // 2^500, 2^-500, 2^-900, 2^-443
    switch (form) {
    case TLP_LOG_PN: case TLP_LOG10_PN: case TLP_LOG10_SPLIT: return ua >= minn && ua < inf;                  // positive normal
    case TLP_POW10_SL: return ma < tlm_d2u(222.0);
    case TLP_EXP_SL: return ma < tlm_d2u(512.0);
    case TLP_SINCOS_SL: case TLP_SINCOS_PHASED: return ma < tlm_d2u(105414350.0);
    case TLP_SINCOS_PHASED_RAW: return ma < tlm_d2u(105414350.0) && mb < tlm_d2u(105414350.0);
    case TLP_ATAN2_PHASED: case TLP_ATAN2_NS: { const uint64_t big = ma > mb ? ma : mb; return big >= m443 && big <= p500; }      // (both finite then)
    case TLP_DIV_NS: return ub >= m500 && ub <= p500 && (ua == 0 || (ma >= m900 && ma <= p500));             // divisor positive; dividend +0 or of either sign (-0.0 would come out as +0)
    case TLP_SQRT_NS: return ma == 0 || (ua >= m500 && ua <= p500);
    case TLP_SQRT_NZ: case TLP_RCP_SEED: case TLP_RSQ_SEED: case TLP_RECIP: return ua >= m500 && ua <= p500;
    case TLP_DIV: case TLP_SQRT: return true;                                                                 // the language's own operations: any operand
    case TLP_MIN_NN: case TLP_MAX_NN: return ma <= inf && mb <= inf;                                          // neither a NaN
    case TLP_FMA_K: return ma < inf && mb < inf;
    }
    return false;
}

// The two LDS tables of a probe workgroup, filled as the kernels fill theirs: the log table word for word (TlTables::dblog's second part,
// TL_LOGTAB), the sincos table with its rows' halves apart (toolame_psy2.hip: what TL_SCT reads).  The emulation keeps glibc's own layout.
struct alignas(16) TlProbeTables { uint64_t lt[256]; uint64_t sct[440]; };
TL_FN void tl_probe_fill_tables(TlProbeTables &t, int first, int step)
{
    for (int i = first; i < 256; i += step) t.lt[i] = tlm_log_tab[i];
#ifdef TL_EMULATE
    for (int i = first; i < 440; i += step) t.sct[i] = tlm_sincostab[i];
#else
    for (int i = first; i < 440; i += step) t.sct[2 * (i >> 2) + (i & 1) + 220 * ((i >> 1) & 1)] = tlm_sincostab[i];      // (TL_SCT, mp2_wave.h)
#endif
}

// 64 arguments from i0 on (those below n), one per lane.  lt: the log table, tlm_log_tab itself or the LDS copy (the caller branches, so
// that each call sees one address space as the kernels do); sct: the LDS sincos table.  b and r1 are valid arrays whatever the form.
TL_FN void tl_probe_libm_unit(int form, const uint64_t *lt, const uint64_t *sct, long i0, long n, const double *a, const double *b, double *r0, double *r1)
{
    TL_LANES_BEGIN
    const long i = i0 + lane;
    if (i < n) {
        const double x = a[i], y = b[i];
        double o0 = 0, o1 = 0;
        switch (form) {
        case TLP_LOG_PN: o0 = tlm_log_pn(x, lt); break;
        case TLP_LOG10_PN: o0 = tlm_log10_pn(x, lt); break;
        case TLP_LOG10_SPLIT: {
            bool near1;
            const double v = tlm_log10_main_pn(x, lt, &near1);
            o0 = near1 ? tlm_log10_near1_pn(x) : v;
        } break;
        case TLP_POW10_SL: o0 = tlm_pow10_sl(x); break;
        case TLP_EXP_SL: o0 = tlm_exp_sl<false>(x, 0.0); break;
        case TLP_SINCOS_SL: tlm_sincos_sl(x, &o0, &o1, tlm_sincostab); break;
        case TLP_SINCOS_PHASED: {
            const TlmSinCosA s = tlm_sincos_reduce(x);
            const double sn = tl_u2d(TL_SCT(sct, s.row, 0)), ssn = tl_u2d(TL_SCT(sct, s.row, 1)), cs = tl_u2d(TL_SCT(sct, s.row, 2)), ccs = tl_u2d(TL_SCT(sct, s.row, 3));
            TL_SCHED_FENCE();
            const TlmSinCosB v = tlm_sincos_poly(s);
            TL_SCHED_FENCE();
            tlm_sincos_finish(s, v, sn, ssn, cs, ccs, &o0, &o1);
        } break;
        case TLP_SINCOS_PHASED_RAW: {                                        // the line loop of tl_psy2_pass, steps 1..7: s2 = the predicted phase, s1 = the phase
            const TlmSinCosA s2 = tlm_sincos_reduce(y);
            const double q_sn = tl_u2d(TL_SCT(sct, s2.row, 0)), q_ssn = tl_u2d(TL_SCT(sct, s2.row, 1)), q_cs = tl_u2d(TL_SCT(sct, s2.row, 2)), q_ccs = tl_u2d(TL_SCT(sct, s2.row, 3));
            TL_SCHED_FENCE();
            const TlmSinCosB v2 = tlm_sincos_poly(s2);
            TL_SCHED_FENCE();
            double spp, cpp;
            tlm_sincos_finish_raw(s2, v2, q_sn, q_ssn, q_cs, q_ccs, &spp, &cpp);
            const TlmSinCosA s1 = tlm_sincos_reduce(x);
            const double w_sn = tl_u2d(TL_SCT(sct, s1.row, 0)), w_ssn = tl_u2d(TL_SCT(sct, s1.row, 1)), w_cs = tl_u2d(TL_SCT(sct, s1.row, 2)), w_ccs = tl_u2d(TL_SCT(sct, s1.row, 3));
            TL_SCHED_FENCE();
            const TlmSinCosB v1 = tlm_sincos_poly(s1);
            TL_SCHED_FENCE();
            double ds, dc;
            tlm_sincos_finish_raw(s1, v1, w_sn, w_ssn, w_cs, w_ccs, &ds, &dc);
            const bool sw = ((s1.q ^ s2.q) & 1u) != 0;
            o0 = tlm_sel(sw, dc, ds); o1 = tlm_sel(sw, ds, dc);
            TL_KEEP(spp); TL_KEEP(cpp);                                      // (the predicted phase's pair is computed, as in the line loop)
        } break;
        case TLP_ATAN2_PHASED: {
            const TlmAtanA at = tlm_atan2_head(x, y);
            const uint64_t *arow = tlm_atan_cij + 7 * at.i;
            const double c0 = tl_u2d(arow[0]), c1 = tl_u2d(arow[1]), c2 = tl_u2d(arow[2]), c3 = tl_u2d(arow[3]), c4 = tl_u2d(arow[4]), c5 = tl_u2d(arow[5]), c6 = tl_u2d(arow[6]);
            TLM_SCHED_FENCE();
            const TlmAtanB am = tlm_atan2_mid(at);
            TLM_SCHED_FENCE();
            o0 = tlm_atan2_tail(at, am, c0, c1, c2, c3, c4, c5, c6);
        } break;
        case TLP_ATAN2_NS: o0 = tlm_atan2_sl<false>(x, y, tlm_atan_cij); break;
        case TLP_DIV_NS: o0 = tlm_div_ns(x, y); break;
        case TLP_SQRT_NS: o0 = tlm_sqrt_ns(x); break;
        case TLP_SQRT_NZ: o0 = tlm_sqrt_nz(x); break;
        case TLP_RCP_SEED: o0 = tlm_rcp_seed(x); break;
        case TLP_RSQ_SEED: o0 = tlm_rsq_seed(x); break;
        case TLP_DIV: o0 = x / y; break;
        case TLP_SQRT: o0 = __builtin_sqrt(x); break;
        case TLP_MIN_NN: o0 = TLM_MIN_NN(x, y); break;
        case TLP_MAX_NN: o0 = TLM_MAX_NN(x, y); break;
        case TLP_FMA_K: o0 = TLM_FMA_K(x, y, 0xbfd5555555555555); break;
        case TLP_RECIP: o0 = tlm_recip_from(x, tlm_rcp_seed(x)); break;
        default: break;
        }
        r0[i] = o0; r1[i] = o1;
    }
    TL_LANES_END
}

// ---- (b) the wave primitives: one wave per case.  A case is 64 input words of 64 bits (a lane's value: a u64 key, a double's bits, or an
// i32 / u32 in the low half), a second such row where the primitive takes one, and 64 output words (TLP_MIRROR4: four per lane in and out,
// TLP_LD2ST2: two out).  A wave-uniform result is written by every lane; an int result is written sign-extended.
enum {
    TLP_WAVE_MIN_U64 = 0, TLP_WAVE_ARGMIN_U64, TLP_WAVE_SUM_I32, TLP_WAVE_XOR_U32, TLP_WAVE_EXSCAN_I32, TLP_WAVE_INCL_XSCAN_U32,
    TLP_ROW16_MAX_F64,       // valid in lane 15 of each row of 16
    TLP_PAR_MIN_U64, TLP_PAR_SUM_I32,
    TLP_BALLOT,              // the predicate: the lane's word is not zero
    TLP_RANK_BELOW,          // of that ballot
    TLP_SWAP1_U64, TLP_SWAP1_F64, TLP_ROT32_F64, TLP_MIRROR1, TLP_MIRROR4,
    TLP_OTHER,               // in2: the source lane of each lane, 0..63
    TLP_READLANE_I32,        // in2[0]: the (uniform) lane read
    TLP_UNI_I,               // the input is the same in every lane: the primitive's precondition ("uniform by construction")
    TLP_SELECT,              // in2 != 0 ? in : ~in
    TLP_SIGN_BIT,
    TLP_LD2ST2,              // lane l stores (in, in2) as a pair at doubles [2 l], reads the pair of lane 63 - l
    TLP_NPRIMS
};
TLM_HD int tlp_in_words(int prim) { return prim == TLP_MIRROR4 ? 4 : 1; }
TLM_HD int tlp_out_words(int prim) { return prim == TLP_MIRROR4 ? 4 : prim == TLP_LD2ST2 ? 2 : 1; }
static inline bool tlp_wave_two_in(int prim) { return prim == TLP_OTHER || prim == TLP_READLANE_I32 || prim == TLP_SELECT || prim == TLP_LD2ST2; }
// what a case must satisfy (checked on the host): a lane number is a lane number
static inline bool tlp_wave_case_ok(int prim, const uint64_t *in, const uint64_t *in2)
{
    if (prim == TLP_OTHER) { for (int l = 0; l < 64; l++) if (in2[l] > 63) return false; }
    if (prim == TLP_READLANE_I32 && in2[0] > 63) return false;
    if (prim == TLP_UNI_I) { for (int l = 1; l < 64; l++) if (in[l] != in[0]) return false; }
    return true;
}

// one case; pair = 128 doubles of the wave's own LDS, 16-byte aligned (TLP_LD2ST2)
TL_FN void tl_probe_wave_unit(int prim, const uint64_t *in, const uint64_t *in2, uint64_t *out, double *pair)
{
    PV(uint64_t, u); PV(uint64_t, o); PV(int, iv); PV(int, io); PV(uint32_t, xv); PV(uint32_t, xo); PV(double, dv); PV(double, d2); PV(bool, pr);
    const int iw = tlp_in_words(prim);
    TL_LANES_BEGIN
    L(u) = in[iw * lane]; L(o) = 0; L(iv) = (int)(uint32_t)L(u); L(io) = 0; L(xv) = (uint32_t)L(u); L(xo) = 0; L(dv) = tl_u2d(L(u)); L(d2) = 0; L(pr) = L(u) != 0;
    TL_LANES_END
    switch (prim) {
    case TLP_WAVE_MIN_U64: { const uint64_t m = TL_WAVE_MIN_U64(u); TL_LANES_BEGIN L(o) = m; TL_LANES_END } break;
    case TLP_WAVE_ARGMIN_U64: { const int m = TL_WAVE_ARGMIN_U64(u); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)m; TL_LANES_END } break;
    case TLP_WAVE_SUM_I32: { const int m = TL_WAVE_SUM_I32(iv); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)m; TL_LANES_END } break;
    case TLP_WAVE_XOR_U32: { const uint32_t m = TL_WAVE_XOR_U32(xv); TL_LANES_BEGIN L(o) = m; TL_LANES_END } break;
    case TLP_WAVE_EXSCAN_I32: TL_WAVE_EXSCAN_I32(io, iv); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)L(io); TL_LANES_END break;
    case TLP_WAVE_INCL_XSCAN_U32: TL_WAVE_INCL_XSCAN_U32(xo, xv); TL_LANES_BEGIN L(o) = L(xo); TL_LANES_END break;
    case TLP_ROW16_MAX_F64: TL_ROW16_MAX_F64(d2, dv); TL_LANES_BEGIN L(o) = tl_d2u(L(d2)); TL_LANES_END break;
    case TLP_PAR_MIN_U64: TL_PAR_MIN_U64(o, u); break;
    case TLP_PAR_SUM_I32: TL_PAR_SUM_I32(io, iv); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)L(io); TL_LANES_END break;
    case TLP_BALLOT: { const uint64_t m = TL_BALLOT(pr); TL_LANES_BEGIN L(o) = m; TL_LANES_END } break;
    case TLP_RANK_BELOW: { const uint64_t m = TL_BALLOT(pr); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)TL_RANK_BELOW(m); TL_LANES_END } break;
    case TLP_SWAP1_U64: TL_SWAP1_U64(o, u); break;
    case TLP_SWAP1_F64: TL_SWAP1_F64(d2, , dv, ); TL_LANES_BEGIN L(o) = tl_d2u(L(d2)); TL_LANES_END break;
    case TLP_ROT32_F64: TL_ROT32_F64(d2, dv); TL_LANES_BEGIN L(o) = tl_d2u(L(d2)); TL_LANES_END break;
    case TLP_MIRROR1: {
        PA(double, s, 1); PA(double, m, 1);
        TL_LANES_BEGIN L(s)[0] = L(dv); TL_LANES_END
        TL_MIRROR_SB_F64(m, s, 1);
        TL_LANES_BEGIN L(o) = tl_d2u(L(m)[0]); TL_LANES_END
    } break;
    case TLP_MIRROR4: {
        PA(double, s, 4); PA(double, m, 4);
        TL_LANES_BEGIN
#pragma unroll
        for (int k = 0; k < 4; k++) L(s)[k] = tl_u2d(in[4 * lane + k]);
        TL_LANES_END
        TL_MIRROR_SB_F64(m, s, 4);
        TL_LANES_BEGIN
#pragma unroll
        for (int k = 0; k < 4; k++) out[4 * lane + k] = tl_d2u(L(m)[k]);
        TL_LANES_END
    } return;
    case TLP_OTHER: TL_LANES_BEGIN L(o) = tl_d2u(TL_OTHER(dv, , (int)(in2[lane] & 63))); TL_LANES_END break;
    case TLP_READLANE_I32: { const int l0 = TL_UNI_I((int)(in2[0] & 63)); const int m = TL_READLANE_I32(iv, l0); TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)m; TL_LANES_END } break;
    case TLP_UNI_I: TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)TL_UNI_I(L(iv)); TL_LANES_END break;
    case TLP_SELECT: TL_LANES_BEGIN L(o) = TL_SELECT(in2[lane] != 0, L(u), ~L(u)); TL_LANES_END break;
    case TLP_SIGN_BIT: TL_LANES_BEGIN L(o) = (uint64_t)(int64_t)tl_sign_bit(L(dv)); TL_LANES_END break;
    case TLP_LD2ST2: {
        TL_LANES_BEGIN TL_ST2(pair + 2 * lane, L(dv), tl_u2d(in2[lane])); TL_LANES_END
        TL_LANES_BEGIN
        double p, q;
        TL_LD2(pair + 2 * (63 - lane), p, q);
        out[2 * lane] = tl_d2u(p); out[2 * lane + 1] = tl_d2u(q);
        TL_LANES_END
    } return;
    default: break;
    }
    TL_LANES_BEGIN out[lane] = L(o); TL_LANES_END
}

// ---- (c) the stage helpers of mp2_dbsum.h: mp2_probe_stage.h
#include "mp2_probe_stage.h"
