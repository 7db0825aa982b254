// toolame_dec.hip -- the kernels of the frame check / decode path (tlb_decode_*): stage A (mp2_unpack.h: unpack and verify), stage B
// (mp2_synth.h: requantise and synthesise), and the pass that leaves each stream's last slot for the next launch.  A translation unit
// of its own: the encode kernels' code objects (toolame_hip.hip, toolame_psy2.hip) are not touched by anything here.
// One wavefront per (stream, frame) unit, four units per workgroup; a unit's working set is its wave's LDS block and registers.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_unpack.h"
#include "mp2_synth.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

#define TL_DEC_WAVES 4
static_assert(3 * (TL_DEC_WAVES * sizeof(TlSynthLds) + 4096 + TL_LDS_GRANULE) <= 160 * 1024, "three workgroups of the synthesis kernel per CU: three waves per SIMD");

__global__ void __launch_bounds__(64 * TL_DEC_WAVES) tl_unpack_kernel(TlDecLaunch A)
{
    __shared__ TlDecLds lds[TL_DEC_WAVES];
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_DEC_WAVES>(A.nstreams, A.nframes, s, f)) return;
    const uint32_t st = tl_unpack_unit(lds[wave_v], A, s, f);
    if ((st & TL_DEC_BAD_MASK) && (threadIdx.x & 63u) == 0) atomicAdd(A.bad, 1ull);
}

__global__ void __launch_bounds__(64 * TL_DEC_WAVES) __attribute__((amdgpu_waves_per_eu(3, 3))) tl_synth_kernel(TlDecLaunch A)
{
    __shared__ TlSynthLds lds[TL_DEC_WAVES];
    __shared__ double dwin[512];
    TL_STAGE_DWIN(TL_DEC_WAVES, dwin, A.synth);
    int wave_v = (int)(threadIdx.x >> 6);
    asm volatile("" : "+v"(wave_v));
    int s, f;
    if (!tl_wave_unit<TL_DEC_WAVES>(A.nstreams, A.nframes, s, f)) return;
    tl_synth_unit(lds[wave_v], A, s, f, dwin);
}

__global__ void __launch_bounds__(64 * TL_DEC_WAVES) tl_dec_carry_kernel(TlDecLaunch A)
{
    const int s = tl_wave_index<TL_DEC_WAVES>();
    if (s < A.nstreams) tl_dec_carry(A, s);
}

hipError_t tlk_decode(hipStream_t st, const TlDecLaunch &A)
{
    const long long units = (long long)A.nstreams * A.nframes;
    const unsigned blocks = (unsigned)((units + TL_DEC_WAVES - 1) / TL_DEC_WAVES);
    hipLaunchKernelGGL(tl_unpack_kernel, dim3(blocks), dim3(64 * TL_DEC_WAVES), 0, st, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (A.pcm) {
        hipLaunchKernelGGL(tl_synth_kernel, dim3(blocks), dim3(64 * TL_DEC_WAVES), 0, st, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(tl_dec_carry_kernel, dim3((unsigned)((A.nstreams + TL_DEC_WAVES - 1) / TL_DEC_WAVES)), dim3(64 * TL_DEC_WAVES), 0, st, A);
    return hipGetLastError();
}
