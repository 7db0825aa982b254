// TEST-ONLY: csrc/mp2_probe.h as a lane loop on the host (-DTL_EMULATE): the host halves of tl_libm.h and of mp2_wave.h's primitives, called
// one by one through the same text the probe kernels run (csrc/toolame_probe.hip).  Built at first use by tests/probelib.py.
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_probe.h"

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

}
