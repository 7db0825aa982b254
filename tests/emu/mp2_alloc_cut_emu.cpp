// TEST-ONLY: the allocation form of csrc/mp2_probe_stage.h as a lane loop on the host (-DTL_EMULATE), case by case, with the path counters of
// csrc/mp2_alloc.h (TL_DBG_ALLOC: which way the closing round of tl_allocate went) returned PER CASE -- tests/emu/mp2_probe_emu.cpp runs the
// same text but keeps no counters.  Built at first use by tests/alloccutlib.py, together with csrc/mp2_host.cpp (the kernels' own tables):
// as it stands, with -DTL_CUT_PASSES=0 (the lane-by-lane pass alone: the parent's loop) and with -DTL_ALLOC_MUTANT=1..4 (the mutants
// tests/test_alloc_cut_emu.py must see fail).
#define TL_EMULATE 1
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include "../../odr-audioenc_amd/csrc/mp2_host.h"
#include "../../odr-audioenc_amd/csrc/mp2_probe.h"
#include "../../odr-audioenc_amd/csrc/mp2_tables.inc"

extern "C" {

__attribute__((visibility("default"))) int alloc_cut_ncounters(void) { return TLA_N; }
__attribute__((visibility("default"))) int alloc_cut_serial_limit(void) { return TL_CUT_SERIAL; }
__attribute__((visibility("default"))) int alloc_cut_passes(void) { return TL_CUT_PASSES; }

// the arrays of TLS_ALLOC (csrc/mp2_probe_stage.h), call 0 or 1; stats: long [n][TLA_N], the counters of each case.  0, or 18 for what the probe refuses
__attribute__((visibility("default"))) int alloc_cut_cases(long n, const void *in0, const void *in1, const void *in2, void *out0, void *out1, long *stats)
{
    if (n <= 0 || n > tls_max_n(TLS_ALLOC) || !in0 || !in1 || !in2 || !out0 || !out1 || !stats) return 18;
    if (!tls_in_domain(TLS_ALLOC, n, in0, in1, in2)) return 18;
    static TlTables T;
    static bool built = false;
    if (!built) { tl_build_tables(&T); built = true; }
    uint32_t hist[64];
    for (long k = 0; k < n; k++) {
        emu_alloc_stats(nullptr, 1);
        memset(hist, 0xa5, sizeof hist);                                   // what the encoder hands over is not zeroed either
        tl_probe_alloc_case(&T.shared, tls_alloc_tab(), k, in0, in1, in2, out0, out1, hist);
        emu_alloc_stats(stats + k * TLA_N, 0);
    }
    return 0;
}

}
