// toolame_probe.hip -- TEST BUILDS ONLY: the probe kernels over the bodies of mp2_probe.h and their C entry points (csrc/tlb_debug.h).
// A unit of the fault-injection TEST library alone (csrc/Makefile: PROBE_UNITS, the kernels' own flags -- they are what is under test);
// the product library links none of it.  Nothing here provokes anything: every argument is checked against its form's stated domain on
// the host before a byte is copied, and a case of the wave probe against what its primitive requires of a lane number.
#include <hip/hip_runtime.h>
#include <math.h>
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
#endif
