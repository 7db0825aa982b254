// TEST-ONLY: csrc/mp2_probe.h as a lane loop on the host (-DTL_EMULATE): the host halves of tl_libm.h and of mp2_wave.h's primitives, and the stage
// helpers of mp2_dbsum.h (csrc/mp2_probe_stage.h), called one by one through the same text the probe kernels run (csrc/toolame_probe.hip).
// Built at first use by tests/probelib.py, together with csrc/mp2_host.cpp (the kernels' own tables).
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_probe.h"
#include "../../odr-audioenc_amd/csrc/mp2_tables.inc"

extern "C" {

// as tlb_debug_probe_libm (csrc/tlb_debug.h): 0, or 18 (TLB_ERR_ARG) for what that call refuses
__attribute__((visibility("default"))) int probe_libm(int form, int table, long n, const double *a, const double *b, double *r0, double *r1)
{
    if (form < 0 || form >= TLP_NFORMS || n <= 0 || !a || !r0) return 18;
    if (table != 0 && !(table == 1 && tlp_has_table(form))) return 18;
    const bool in2 = tlp_two_in(form), out2 = tlp_two_out(form);
    if ((in2 && !b) || (out2 && !r1)) return 18;
    for (long i = 0; i < n; i++) if (!tlp_in_domain(form, a[i], in2 ? b[i] : 0.0)) return 18;
    std::vector<double> zb, z1;
    if (!in2) { zb.assign((size_t)n, 0.0); b = zb.data(); }
    if (!out2) { z1.assign((size_t)n, 0.0); r1 = z1.data(); }
    TlProbeTables t;
    tl_probe_fill_tables(t, 0, 1);
    for (long i0 = 0; i0 < n; i0 += 64) tl_probe_libm_unit(form, table ? t.lt : tlm_log_tab, t.sct, i0, n, a, b, r0, r1);
    return 0;
}

__attribute__((visibility("default"))) int probe_wave(int prim, int nwaves, const void *in, const void *in2, void *out)
{
    if (prim < 0 || prim >= TLP_NPRIMS || nwaves <= 0 || !in || !out) return 18;
    const bool two = tlp_wave_two_in(prim);
    if (two && !in2) return 18;
    const size_t iw = (size_t)64 * tlp_in_words(prim), ow = (size_t)64 * tlp_out_words(prim);
    const uint64_t *hin = (const uint64_t *)in, *hin2 = (const uint64_t *)in2;
    for (int w = 0; w < nwaves; w++) if (!tlp_wave_case_ok(prim, hin + w * iw, two ? hin2 + (size_t)w * 64 : nullptr)) return 18;
    uint64_t zero[64] = {0};
    alignas(16) double pair[128];
    for (int w = 0; w < nwaves; w++) tl_probe_wave_unit(prim, hin + w * iw, two ? hin2 + (size_t)w * 64 : zero, (uint64_t *)out + w * ow, pair);
    return 0;
}

// as tlb_debug_probe_stage (csrc/tlb_debug.h): 0, or 18 (TLB_ERR_ARG) for what that call refuses
__attribute__((visibility("default"))) int probe_stage(int form, long n, const void *in0, const void *in1, const void *in2, void *out0, void *out1)
{
    if (form < 0 || form >= TLS_NFORMS || n <= 0 || n > tls_max_n(form)) return 18;
    size_t by[5];
    tls_bytes(form, n, by);
    const void *hin[3] = {in0, in1, in2};
    void *hout[2] = {out0, out1};
    for (int k = 0; k < 3; k++) if (by[k] && !hin[k]) return 18;
    for (int k = 0; k < 2; k++) if (by[3 + k] && !hout[k]) return 18;
    if (!tls_in_domain(form, n, in0, in1, in2)) return 18;
    static TlTables T;
    static bool built = false;
    if (!built) { tl_build_tables(&T); built = true; }
    std::vector<double> recip;
    if (form == TLS_DIV_BY) {
        recip.resize((size_t)n);
        for (long i = 0; i < n; i++) recip[(size_t)i] = 1.0 / ((const double *)in1)[i];
        in2 = recip.data();
    }
    static TlStageLds w;
    if (form < TLS_LANE_FORMS) for (long i0 = 0; i0 < n; i0 += 64) tl_probe_stage_lanes(form, w, T.dblog, T.shared.scalefactor, i0, n, in0, in1, in2, out0, out1);
    else if (form == TLS_ALLOC) for (long k = 0; k < n; k++) tl_probe_alloc_case(&T.shared, tls_alloc_tab(), k, in0, in1, in2, out0, out1);
    else for (long k = 0; k < n; k++) tl_probe_stage_case(form, w, k, in0, in1, in2, out0, out1);
    return 0;
}

// The bark values of the library's own threshold tables (csrc/mp2_host.cpp tl_build_config): psy 1 the rows of TlConfig::p1_bark, psy 3 the rows
// TlConfig::p3_subset picks of p3_bark.  out[136]; returns the number of rows, or -1 for a rate or model the library refuses.
__attribute__((visibility("default"))) int probe_bark_table(int psy, long samplerate, double *out)
{
    static TlConfig C;
    if ((psy != 1 && psy != 3) || tl_build_config(&C, samplerate, 'm', samplerate < 32000 ? 32 : 64, psy, 0) != TL_OK) return -1;
    if (psy == 1) { for (int i = 0; i < C.p1_sub; i++) out[i] = C.p1_bark[i]; return C.p1_sub; }
    for (int i = 0; i < 136; i++) out[i] = C.p3_bark[C.p3_subset[i]];
    return 136;
}
// the dB-sum table the probe's kernels read (TlTables::dblog[0..1001]: psycho_1.c:170-178 and its two closing entries) -- data for the oracles
__attribute__((visibility("default"))) void probe_dbtable(double *out) { static TlTables T; tl_build_tables(&T); for (int i = 0; i < 1002; i++) out[i] = T.dblog[i]; }
// the Layer II allocation tables of csrc/mp2_tables.inc as they stand there, none of what the kernels derive from them -- data for the oracle of the
// allocation form: TL_SNR_E2[18], TL_BITS[18], TL_GROUP[18], TL_NBAL[9], TL_STEP_INDEX[144], TL_LINE[160] (255 above sblimit), TL_TABLE_SBLIMIT[5]
__attribute__((visibility("default"))) void probe_alloc_tables(int32_t *out)
{
    int o = 0;
    for (int i = 0; i < 18; i++) out[o++] = TL_SNR_E2[i];
    for (int i = 0; i < 18; i++) out[o++] = TL_BITS[i];
    for (int i = 0; i < 18; i++) out[o++] = TL_GROUP[i];
    for (int i = 0; i < 9; i++) out[o++] = TL_NBAL[i];
    for (int i = 0; i < 144; i++) out[o++] = TL_STEP_INDEX[i];
    for (int i = 0; i < 160; i++) out[o++] = TL_LINE[i];
    for (int i = 0; i < 5; i++) out[o++] = TL_TABLE_SBLIMIT[i];
}
// the scalefactor table the probe's kernels read (TlTables::shared)
__attribute__((visibility("default"))) void probe_scalefactors(double *out) { static TlTables T; tl_build_tables(&T); for (int i = 0; i < 64; i++) out[i] = T.shared.scalefactor[i]; }

}
