// toolame_probe.hip -- TEST BUILDS ONLY: the probe kernels over the bodies of mp2_probe.h and their C entry points (csrc/tlb_debug.h).
// A unit of the fault-injection TEST library alone (csrc/Makefile: PROBE_UNITS, the kernels' own flags -- they are what is under test);
// the product library links none of it.  Nothing here provokes anything: every argument is checked against its form's stated domain on
// the host before a byte is copied, a case of the wave probe against what its primitive requires of a lane number, and every argument
// and case of the stage probe against the domain mp2_probe_stage.h states (counts, row ranges, field lengths: all that becomes an LDS index).
#include <hip/hip_runtime.h>
#include <math.h>
#include <vector>
#include "mp2_host.h"
#include "mp2_probe.h"
#include "tlb_debug.h"
#include "tlb_mem.h"

// one lane per argument: 256 threads = four waves of 64 consecutive arguments; the grid covers n, the last block's tail is guarded per lane
__global__ void __launch_bounds__(256) tl_probe_libm_kernel(int form, int table, long n, const double *a, const double *b, double *r0, double *r1)
{
    __shared__ TlProbeTables t;
    tl_probe_fill_tables(t, (int)threadIdx.x, 256);
    __syncthreads();
    const long i0 = (long)blockIdx.x * 256 + (long)(threadIdx.x & ~63u);
    if (i0 >= n) return;                                                  // (a whole wave past the end)
    if (table) tl_probe_libm_unit(form, t.lt, t.sct, i0, n, a, b, r0, r1);
    else tl_probe_libm_unit(form, tlm_log_tab, t.sct, i0, n, a, b, r0, r1);
}

// one wave per case: 256 threads = four cases
__global__ void __launch_bounds__(256) tl_probe_wave_kernel(int prim, int nwaves, const uint64_t *in, const uint64_t *in2, uint64_t *out)
{
    __shared__ __attribute__((aligned(16))) double pair[4][128];
    const int wave = (int)(threadIdx.x >> 6), w = (int)blockIdx.x * 4 + wave;
    if (w >= nwaves) return;                                              // (wave-uniform; no workgroup barrier below)
    tl_probe_wave_unit(prim, in + (size_t)w * 64 * tlp_in_words(prim), in2 + (size_t)w * 64, out + (size_t)w * 64 * tlp_out_words(prim), pair[wave]);
}

// the stage helpers (mp2_probe_stage.h): 256 threads = four waves, each with its own TlStageLds; the dB-sum table and the scalefactor table are copied
// into the workgroup's LDS as the model phase and the encode prologue keep them, and for the allocation form TlBlockShared, where the frame kernel keeps it.
// Lane forms: 64 consecutive arguments a wave; case forms: one case a wave.
__global__ void __launch_bounds__(256) tl_probe_stage_kernel(int form, long n, const double *dblog, const double *sftab, const TlBlockShared *shared,
                                                             const TlsAllocTab *atab, const void *in0, const void *in1, const void *in2, void *out0, void *out1)
{
    static_assert(sizeof(TlBlockShared) % 8 == 0, "copied as doubles");
    __shared__ TlBlockShared blk;
    __shared__ __attribute__((aligned(16))) double dbt[1002];
    __shared__ __attribute__((aligned(16))) double sfl[64];
    __shared__ TlStageLds lds[4];
    for (int i = (int)threadIdx.x; i < 1002; i += 256) dbt[i] = dblog[i];
    if (threadIdx.x < 64) sfl[threadIdx.x] = sftab[threadIdx.x];
    if (form == TLS_ALLOC) for (int i = (int)threadIdx.x; i < (int)(sizeof(TlBlockShared) / 8); i += 256) ((double *)&blk)[i] = ((const double *)shared)[i];
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6);
    if (form < TLS_LANE_FORMS) {
        const long i0 = (long)blockIdx.x * 256 + 64 * wave;
        if (i0 >= n) return;                                              // (wave-uniform; no workgroup barrier below)
        tl_probe_stage_lanes(form, lds[wave], dbt, sfl, i0, n, in0, in1, in2, out0, out1);
    } else {
        const long k = (long)blockIdx.x * 4 + wave;
        if (k >= n) return;
        if (form == TLS_ALLOC) tl_probe_alloc_case(&blk, atab, k, in0, in1, in2, out0, out1, lds[wave].frame);
        else tl_probe_stage_case(form, lds[wave], k, in0, in1, in2, out0, out1);
    }
}

#ifdef TLB_FAULT_INJECT
#define TLP_MAX_N (1l << 26)
#define TLP_HIP(x) do { if ((x) != hipSuccess) return TLB_ERR_HIP; } while (0)

extern "C" int tlb_debug_probe_libm(int form, int table, long n, const double *a, const double *b, double *r0, double *r1)
{
    if (form < 0 || form >= TLP_NFORMS || n <= 0 || n > TLP_MAX_N || !a || !r0) return TLB_ERR_ARG;
    if (table != 0 && !(table == 1 && tlp_has_table(form))) return TLB_ERR_ARG;
    const bool in2 = tlp_two_in(form), out2 = tlp_two_out(form);
    if ((in2 && !b) || (out2 && !r1)) return TLB_ERR_ARG;
    for (long i = 0; i < n; i++) if (!tlp_in_domain(form, a[i], in2 ? b[i] : 0.0)) return TLB_ERR_ARG;
    const size_t bytes = (size_t)n * sizeof(double);
    TlbMem m;
    double *da = m.scratch<double>((size_t)n), *db = m.dev<double>((size_t)n), *d0 = m.dev<double>((size_t)n), *d1 = m.dev<double>((size_t)n);
    m.upload(da, a, bytes);
    if (in2) m.upload(db, b, bytes);
    if (!m.settle()) return TLB_ERR_HIP;
    tl_probe_libm_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0>>>(form, table, n, da, db, d0, d1);
    TLP_HIP(hipGetLastError());
    TLP_HIP(hipDeviceSynchronize());
    TLP_HIP(hipMemcpy(r0, d0, bytes, hipMemcpyDeviceToHost));
    if (out2) TLP_HIP(hipMemcpy(r1, d1, bytes, hipMemcpyDeviceToHost));
    return TLB_OK;
}

extern "C" int tlb_debug_probe_wave(int prim, int nwaves, const void *in, const void *in2, void *out)
{
    if (prim < 0 || prim >= TLP_NPRIMS || nwaves <= 0 || nwaves > (1 << 20) || !in || !out) return TLB_ERR_ARG;
    const bool two = tlp_wave_two_in(prim);
    if (two && !in2) return TLB_ERR_ARG;
    const size_t iw = (size_t)64 * tlp_in_words(prim), ow = (size_t)64 * tlp_out_words(prim), nw = (size_t)nwaves;
    const uint64_t *hin = (const uint64_t *)in, *hin2 = (const uint64_t *)in2;
    for (size_t w = 0; w < nw; w++) if (!tlp_wave_case_ok(prim, hin + w * iw, two ? hin2 + w * 64 : nullptr)) return TLB_ERR_ARG;
    TlbMem m;
    uint64_t *di = m.scratch<uint64_t>(nw * iw), *di2 = m.dev<uint64_t>(nw * 64), *dout = m.dev<uint64_t>(nw * ow);
    m.upload(di, in, nw * iw * 8);
    if (two) m.upload(di2, in2, nw * 64 * 8);
    if (!m.settle()) return TLB_ERR_HIP;
    tl_probe_wave_kernel<<<dim3((unsigned)((nwaves + 3) / 4)), dim3(256), 0, 0>>>(prim, nwaves, di, di2, dout);
    TLP_HIP(hipGetLastError());
    TLP_HIP(hipDeviceSynchronize());
    TLP_HIP(hipMemcpy(out, dout, nw * ow * 8, hipMemcpyDeviceToHost));
    return TLB_OK;
}

extern "C" int tlb_debug_probe_stage(int form, long n, const void *in0, const void *in1, const void *in2, void *out0, void *out1)
{
    if (form < 0 || form >= TLS_NFORMS || n <= 0 || n > tls_max_n(form)) return TLB_ERR_ARG;
    size_t by[5];
    tls_bytes(form, n, by);
    const void *hin[3] = {in0, in1, in2};
    void *hout[2] = {out0, out1};
    for (int k = 0; k < 3; k++) if (by[k] && !hin[k]) return TLB_ERR_ARG;
    for (int k = 0; k < 2; k++) if (by[3 + k] && !hout[k]) return TLB_ERR_ARG;
    if (!tls_in_domain(form, n, in0, in1, in2)) return TLB_ERR_ARG;
    static TlTables T;                                                    // the kernels' own tables (mp2_host.cpp), built once
    static bool built = false;
    if (!built) { tl_build_tables(&T); built = true; }
    std::vector<double> recip;
    if (form == TLS_DIV_BY) {                                             // the reciprocal the way the host makes TlConfig::p1_linerw
        recip.resize((size_t)n);
        for (long i = 0; i < n; i++) recip[(size_t)i] = 1.0 / ((const double *)in1)[i];
        hin[2] = recip.data(); by[2] = 8 * (size_t)n;
    }
    TlbMem m;
    double *ddb = m.scratch<double>(1002), *dsf = m.scratch<double>(64);
    m.upload(ddb, T.dblog, 1002 * sizeof(double));
    m.upload(dsf, T.shared.scalefactor, 64 * sizeof(double));
    TlBlockShared *dsh = m.scratch<TlBlockShared>(1);
    TlsAllocTab *dat = m.scratch<TlsAllocTab>(1);
    m.upload(dsh, &T.shared, sizeof(TlBlockShared));
    if (form == TLS_ALLOC) m.upload(dat, tls_alloc_tab(), sizeof(TlsAllocTab));      // (not NULL: tls_in_domain has passed)
    char *din[3], *dout[2];
    for (int k = 0; k < 3; k++) { din[k] = m.dev<char>(by[k]); if (by[k]) m.upload(din[k], hin[k], by[k]); }
    for (int k = 0; k < 2; k++) dout[k] = m.dev<char>(by[3 + k]);
    if (!m.settle()) return TLB_ERR_HIP;
    const long per = form < TLS_LANE_FORMS ? 256 : 4;
    tl_probe_stage_kernel<<<dim3((unsigned)((n + per - 1) / per)), dim3(256), 0, 0>>>(form, n, ddb, dsf, dsh, dat, din[0], din[1], din[2], dout[0], dout[1]);
    TLP_HIP(hipGetLastError());
    TLP_HIP(hipDeviceSynchronize());
    for (int k = 0; k < 2; k++) if (by[3 + k]) TLP_HIP(hipMemcpy(hout[k], dout[k], by[3 + k], hipMemcpyDeviceToHost));
    return TLB_OK;
}
#endif
