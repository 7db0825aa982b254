// toolame_feed_down.hip -- the kernels of the DOWN FEEDS (tlb_feed_down_*; csrc/mp2_feed_down.h): decode a wanted slot into the stream's
// source plane (the strict feed's decode, mp2_feed.h: tl_feed_decode), decimate a tick's source frames out of the carried head and the
// plane into the ingest's input slot (mp2_decimate.h: tl_decimate_outputs), leave the head, the position and the last wanted slot for the
// next call.  A translation unit of its own: no other kernel's code object is touched by anything here.
// decode: one wavefront per (tick, stream, slot), four per workgroup, the synthesis kernel's LDS and occupancy (three waves per SIMD).
// decimate: one workgroup of TL_DC_WAVES waves per (tick, stream), the decimate kernel's 21.0 KB of LDS plus 2.3 KB for the outputs of a
// one-channel feed that go to both channels.  Every branch around a barrier is uniform over the workgroup.
#define TL_FD_BODY 1
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "mp2_feed.h"
#include "mp2_decimate.h"
#include "mp2_feed_down.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_FD_WAVES 4
static_assert(3 * (TL_FD_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of the decode kernel per CU, as of the feed kernel: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_FD_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_feed_down_decode_kernel(TlFeedDownLaunch A)
{
    __shared__ TlSynthLds lds[TL_FD_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_FD_WAVES, dwin, A.F.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s2, f;                                                       // s2: (stream, slot of the tick)
    if (!tl_wave_unit<TL_FD_WAVES>(2 * A.F.nstreams, A.F.nframes, s2, f)) return;
    tl_fd_decode_unit(lds[wave_v], A, s2 >> 1, f, s2 & 1, dwin);
}

__global__ void __launch_bounds__(64 * TL_DC_WAVES) tl_feed_down_decimate_kernel(TlFeedDownLaunch A)
{
    __shared__ TlDecimateLds w;
    __shared__ int16_t y[TL_DC_FRAME];
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)A.F.nstreams), f = (int)(slot / (size_t)A.F.nstreams);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TlFdSlot S = tl_fd_slot_of(A, s, f);
    if (S.ratio == TL_DC_OFF) return;
    tl_fd_fill(A, w, S, s, wave);
    __syncthreads();
    tl_fd_wave(A, w, S, y, s, f, wave);
    if (!(S.fch == 1 && S.sch == 2)) return;
    __syncthreads();
    tl_fd_dup(A, y, s, f, wave);
}

__global__ void __launch_bounds__(64 * TL_FD_WAVES) tl_feed_down_carry_kernel(TlFeedDownLaunch A)
{
    const int s = tl_wave_index<TL_FD_WAVES>();
    if (s < A.F.nstreams) tl_fd_carry(A, s);
}

hipError_t tlk_feed_down(hipStream_t st, const TlFeedDownLaunch &A, const TlConcealConv *cc)
{
    const long long units = (long long)A.F.nstreams * A.F.nframes;
    hipLaunchKernelGGL(tl_feed_down_decode_kernel, dim3((unsigned)((2 * units + TL_FD_WAVES - 1) / TL_FD_WAVES)), dim3(64 * TL_FD_WAVES), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (cc && (e = tlk_conceal_down(st, TlConcealDownLaunch{A, *cc})) != hipSuccess) return e;        // the lost slots' rows, before the decimator reads the plane
    hipLaunchKernelGGL(tl_feed_down_decimate_kernel, dim3((unsigned)units), dim3(64 * TL_DC_WAVES), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tl_feed_down_carry_kernel, dim3((unsigned)((A.F.nstreams + TL_FD_WAVES - 1) / TL_FD_WAVES)), dim3(64 * TL_FD_WAVES), 0, st, A);
    e = hipGetLastError();
    return cc && e == hipSuccess ? tlk_conceal_down_carry(st, TlConcealDownLaunch{A, *cc}) : e;
}
