// toolame_feed_adapt.hip -- the kernels of the ADAPTED Layer II feeds (tlb_feed_set_adapted; csrc/mp2_feed_adapt.h): decode a wanted slot
// into the stream's source plane (the strict feed's decode, mp2_feed.h: tl_feed_decode), resample a tick's source frames out of the
// carried head and the plane into the ingest's input slot, leave the head, the position and the last wanted slot for the next call.  A
// translation unit of its own: no other kernel's code object is touched by anything here.
// decode: one wavefront per (tick, stream), four per workgroup, the synthesis kernel's LDS and occupancy (three waves per SIMD).
// resample: one workgroup of TL_RS_WAVES waves per (tick, stream), the resample kernel's 17.2 KB of LDS plus 2.3 KB for the outputs of a
// one-channel feed that go to both channels.  Every branch around a barrier is uniform over the workgroup.
#define TL_FA_BODY 1
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "mp2_feed.h"
#include "mp2_feed_adapt.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_FA_WAVES 4
static_assert(3 * (TL_FA_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of the decode kernel per CU, as of the feed kernel: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_FA_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_feed_adapt_decode_kernel(TlFeedAdaptLaunch A)
{
    __shared__ TlSynthLds lds[TL_FA_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_FA_WAVES, dwin, A.F.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_FA_WAVES>(A.F.nstreams, A.F.nframes, s, f)) return;
    tl_fa_decode_unit(lds[wave_v], A, s, f, dwin);
}

__global__ void __launch_bounds__(64 * TL_RS_WAVES) tl_feed_adapt_resample_kernel(TlFeedAdaptLaunch A)
{
    __shared__ TlResampleLds w;
    __shared__ int16_t y[TL_RS_FRAME];
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)A.F.nstreams), f = (int)(slot / (size_t)A.F.nstreams);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TlFaSlot S = tl_fa_slot(A, s, f);
    if (S.ratio < 0) return;
    if (S.ratio == TL_RS_OFF) { tl_fa_copy(A, S, s, f, wave); return; }
    tl_fa_fill(A, w, S, s, wave);
    __syncthreads();
    tl_fa_wave(A, w, S, y, s, f, wave);
    if (!(S.fch == 1 && S.sch == 2)) return;
    __syncthreads();
    tl_fa_dup(A, y, s, f, wave);
}

__global__ void __launch_bounds__(64 * TL_FA_WAVES) tl_feed_adapt_carry_kernel(TlFeedAdaptLaunch A)
{
    const int s = tl_wave_index<TL_FA_WAVES>();
    if (s < A.F.nstreams) tl_fa_carry(A, s);
}

hipError_t tlk_feed_adapt(hipStream_t st, const TlFeedAdaptLaunch &A, const TlConcealConv *cc)
{
    const long long units = (long long)A.F.nstreams * A.F.nframes;
    hipLaunchKernelGGL(tl_feed_adapt_decode_kernel, dim3((unsigned)((units + TL_FA_WAVES - 1) / TL_FA_WAVES)), dim3(64 * TL_FA_WAVES), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (cc && (e = tlk_conceal_adapt(st, TlConcealAdaptLaunch{A, *cc})) != hipSuccess) return e;      // the lost slots' rows, before the resampler reads the plane
    hipLaunchKernelGGL(tl_feed_adapt_resample_kernel, dim3((unsigned)units), dim3(64 * TL_RS_WAVES), 0, st, A);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(tl_feed_adapt_carry_kernel, dim3((unsigned)((A.F.nstreams + TL_FA_WAVES - 1) / TL_FA_WAVES)), dim3(64 * TL_FA_WAVES), 0, st, A);
    e = hipGetLastError();
    return cc && e == hipSuccess ? tlk_conceal_adapt_carry(st, TlConcealAdaptLaunch{A, *cc}) : e;
}
