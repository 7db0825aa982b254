// toolame_feed.hip -- the kernels of the Layer II feed path (tlb_feed_*): tl_feed_kernel (mp2_feed.h: tl_feed_decode -- parse, verify,
// requantise and synthesise a feed frame -- into the ingest's input slot) and the pass that leaves each fed stream's last slot for the
// next launch (tl_feed_keep).  A translation unit of its own: no other kernel's code object is touched by anything here.
// One wavefront per (stream, frame) unit, four units per workgroup; a unit's working set is its wave's LDS block and registers.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "mp2_feed.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_FEED_WAVES 4
static_assert(3 * (TL_FEED_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of the feed kernel per CU, as of the synthesis kernel: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_FEED_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_feed_kernel(TlFeedLaunch A)
{
    __shared__ TlSynthLds lds[TL_FEED_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_FEED_WAVES, dwin, A.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_FEED_WAVES>(A.nstreams, A.nframes, s, f)) return;
    tl_feed_unit(lds[wave_v], A, s, f, dwin);
}

__global__ void __launch_bounds__(64 * TL_FEED_WAVES) tl_feed_carry_kernel(TlFeedLaunch A)
{
    const int s = tl_wave_index<TL_FEED_WAVES>();
    if (s < A.nstreams) tl_feed_carry(A, s);
}

hipError_t tlk_feed(hipStream_t st, const TlFeedLaunch &A)
{
    const long long units = (long long)A.nstreams * A.nframes;
    hipLaunchKernelGGL(tl_feed_kernel, dim3((unsigned)((units + TL_FEED_WAVES - 1) / TL_FEED_WAVES)), dim3(64 * TL_FEED_WAVES), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tl_feed_carry_kernel, dim3((unsigned)((A.nstreams + TL_FEED_WAVES - 1) / TL_FEED_WAVES)), dim3(64 * TL_FEED_WAVES), 0, st, A);
    return hipGetLastError();
}
