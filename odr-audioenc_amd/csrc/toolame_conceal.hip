// toolame_conceal.hip -- the kernels of the feed concealment (tlb_conceal_*; csrc/mp2_conceal.h), queued behind the two feed kernels of
// toolame_feed.hip when some stream of the batch has concealment on: tl_conceal_kernel (a lost slot becomes the last good frame at raised
// scalefactor indices, the good slot behind a loss is synthesised over that repeat) and tl_conceal_carry_kernel (the record, G and the run
// for the next launch).  A translation unit of its own: no other kernel's code object is touched by anything here.
// One wavefront per (stream, frame) unit, four units per workgroup, the feed kernel's geometry, LDS and occupancy.
#include <hip/hip_runtime.h>
#include <math.h>
#define TL_CC_BODY 1
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "mp2_feed.h"
#include "mp2_conceal.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_CONCEAL_WAVES 4
static_assert(3 * (TL_CONCEAL_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of the conceal kernel per CU, as of the feed kernel: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_CONCEAL_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_conceal_kernel(TlConcealLaunch A)
{
    __shared__ TlSynthLds lds[TL_CONCEAL_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_CONCEAL_WAVES, dwin, A.F.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_CONCEAL_WAVES>(A.F.nstreams, A.F.nframes, s, f)) return;
    tl_conceal_unit(lds[wave_v], A, s, f, dwin);
}

__global__ void __launch_bounds__(64 * TL_CONCEAL_WAVES) tl_conceal_carry_kernel(TlConcealLaunch A)
{
    const int s = tl_wave_index<TL_CONCEAL_WAVES>();
    if (s < A.F.nstreams) tl_conceal_carry(A, s);
}

hipError_t tlk_conceal(hipStream_t st, const TlConcealLaunch &A)
{
    const long long units = (long long)A.F.nstreams * A.F.nframes;
    hipLaunchKernelGGL(tl_conceal_kernel, dim3((unsigned)((units + TL_CONCEAL_WAVES - 1) / TL_CONCEAL_WAVES)), dim3(64 * TL_CONCEAL_WAVES), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tl_conceal_carry_kernel, dim3((unsigned)((A.F.nstreams + TL_CONCEAL_WAVES - 1) / TL_CONCEAL_WAVES)), dim3(64 * TL_CONCEAL_WAVES), 0, st, A);
    return hipGetLastError();
}
