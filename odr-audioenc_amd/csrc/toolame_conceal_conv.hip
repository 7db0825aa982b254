// toolame_conceal_conv.hip -- the kernels of the feed concealment on ADAPTED and DOWN feeds (tlb_feed_loss_enable;
// csrc/mp2_conceal_conv.h), queued between and behind the kernels of toolame_feed_adapt.hip and toolame_feed_down.hip when some adapted
// (or down) stream of the batch has concealment on: tl_conceal_adapt_kernel / tl_conceal_down_kernel between the decode and the resample
// or decimate kernel (a lost wanted slot's row of the source plane becomes the last good frame at raised scalefactor indices, the good
// slot behind a loss is synthesised over that repeat), tl_conceal_adapt_carry_kernel / tl_conceal_down_carry_kernel behind the path's own
// carry (the record, G and the run for the next call).  A translation unit of its own: no other kernel's code object is touched by
// anything here.  One wavefront per unit, four units per workgroup, the decode kernels' geometry, LDS and occupancy.
#define TL_CC_BODY 1
#define TL_FA_BODY 1
#define TL_FD_BODY 1
#define TL_CCV_BODY 1
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "mp2_feed.h"
#include "mp2_decimate.h"
#include "mp2_feed_adapt.h"
#include "mp2_feed_down.h"
#include "mp2_conceal.h"
#include "mp2_conceal_conv.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_CCV_WAVES 4
static_assert(3 * (TL_CCV_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of a conceal kernel per CU, as of the decode kernels: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_CCV_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_conceal_adapt_kernel(TlConcealAdaptLaunch A)
{
    __shared__ TlSynthLds lds[TL_CCV_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_CCV_WAVES, dwin, A.D.F.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_CCV_WAVES>(A.D.F.nstreams, A.D.F.nframes, s, f)) return;
    tl_ccv_adapt_unit(lds[wave_v], A, s, f, dwin);
}

__global__ void __launch_bounds__(64 * TL_CCV_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_conceal_down_kernel(TlConcealDownLaunch A)
{
    __shared__ TlSynthLds lds[TL_CCV_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_CCV_WAVES, dwin, A.D.F.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s2, f;                                                       // s2: (stream, slot of the tick)
    if (!tl_wave_unit<TL_CCV_WAVES>(2 * A.D.F.nstreams, A.D.F.nframes, s2, f)) return;
    tl_ccv_down_unit(lds[wave_v], A, s2 >> 1, f, s2 & 1, dwin);
}

__global__ void __launch_bounds__(64 * TL_CCV_WAVES) tl_conceal_adapt_carry_kernel(TlConcealAdaptLaunch A)
{
    const int s = tl_wave_index<TL_CCV_WAVES>();
    if (s < A.D.F.nstreams) tl_ccv_adapt_carry(A, s);
}

__global__ void __launch_bounds__(64 * TL_CCV_WAVES) tl_conceal_down_carry_kernel(TlConcealDownLaunch A)
{
    const int s = tl_wave_index<TL_CCV_WAVES>();
    if (s < A.D.F.nstreams) tl_ccv_down_carry(A, s);
}

static unsigned ccv_blocks(long long units) { return (unsigned)((units + TL_CCV_WAVES - 1) / TL_CCV_WAVES); }

hipError_t tlk_conceal_adapt(hipStream_t st, const TlConcealAdaptLaunch &A)
{
    hipLaunchKernelGGL(tl_conceal_adapt_kernel, dim3(ccv_blocks((long long)A.D.F.nstreams * A.D.F.nframes)), dim3(64 * TL_CCV_WAVES), 0, st, A);
    return hipGetLastError();
}
hipError_t tlk_conceal_adapt_carry(hipStream_t st, const TlConcealAdaptLaunch &A)
{
    hipLaunchKernelGGL(tl_conceal_adapt_carry_kernel, dim3(ccv_blocks(A.D.F.nstreams)), dim3(64 * TL_CCV_WAVES), 0, st, A);
    return hipGetLastError();
}
hipError_t tlk_conceal_down(hipStream_t st, const TlConcealDownLaunch &A)
{
    hipLaunchKernelGGL(tl_conceal_down_kernel, dim3(ccv_blocks(2ll * A.D.F.nstreams * A.D.F.nframes)), dim3(64 * TL_CCV_WAVES), 0, st, A);
    return hipGetLastError();
}
hipError_t tlk_conceal_down_carry(hipStream_t st, const TlConcealDownLaunch &A)
{
    hipLaunchKernelGGL(tl_conceal_down_carry_kernel, dim3(ccv_blocks(A.D.F.nstreams)), dim3(64 * TL_CCV_WAVES), 0, st, A);
    return hipGetLastError();
}
