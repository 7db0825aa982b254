// tl_kernel_util.h -- what the kernels' translation units share beside mp2_wave.h: the work list of the persistent kernels of the encode
// path (toolame_hip.hip, toolame_psy2.hip) and the prologue of the wave-per-unit kernels (toolame_dec.hip, toolame_feed.hip, toolame_feed_adapt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define TL_LDS_GRANULE 1280u          // LDS is handed out in granules of 1280 bytes on gfx950 (160 KB / 128)
#ifndef TL_PSY2_WAVES
#define TL_PSY2_WAVES 12
#endif

// Next unit of a persistent kernel's work list: ONE returning device-scope atomic add per wave, issued by lane 0 alone.
// The lane mask is narrowed inside the asm statement, not with an `if (lane == 0)`: LLVM threaded such a branch together
// with the equal test of the diagnostic stamps at the end of the previous unit into a loop that some lanes never left; and
// its wave-level atomic optimiser, which folds `atomicAdd(p, 1)` of 64 lanes into one add, only does so while it can prove the
// address uniform -- when it cannot, the 64 adds of two waves interleave and units are handed out twice or never.
// `counter` must be wave-uniform and the call site wave-uniform control flow (lane 0 active: its registers carry the operands).
static __device__ __forceinline__ int tl_next_unit(int32_t *counter)
{
    int u;
    uint64_t saved;
    __builtin_amdgcn_wave_barrier();
    asm volatile("s_mov_b64 %1, exec\n\t"
                 "s_mov_b64 exec, 1\n\t"
                 "global_atomic_add %0, %2, %3, %4 sc0\n\t"
                 "s_waitcnt vmcnt(0)\n\t"
                 "s_mov_b64 exec, %1"
                 : "=&v"(u), "=&s"(saved) : "v"(0), "v"(1), "s"(counter) : "memory");
    return __builtin_amdgcn_readfirstlane(u);
}

// ---- kernels of one wavefront per unit, WAVES units per workgroup ----
// this wave's index in the launch, wave-uniform (a stream index for the carry kernels)
template <int WAVES, class T = int> static __device__ __forceinline__ T tl_wave_index()
{
    return (T)blockIdx.x * WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
// ... as a unit of a launch of nframes x nstreams slots: slot f = u / nstreams of stream s = u % nstreams; false past the end
template <int WAVES> static __device__ __forceinline__ bool tl_wave_unit(int nstreams, int nframes, int &s, int &f)
{
    const long long u = tl_wave_index<WAVES, long long>();
    if (u >= (long long)nstreams * nframes) return false;
    f = (int)(u / nstreams); s = (int)(u % nstreams);
    return true;
}
// the synthesis window (TlSynthTables::d) into the workgroup's `dwin[512]` in LDS, and the barrier behind it: every wave of the WAVES comes
// here before it may leave.  A macro: the copy is compiled in the kernel's own body, where `dwin` is the LDS array and not a pointer to it.
#define TL_STAGE_DWIN(WAVES, dwin, synth) \
    do { for (int i = (int)threadIdx.x; i < 512; i += 64 * (WAVES)) (dwin)[i] = (synth)->d[i]; __syncthreads(); } while (0)
// the opening of the two encode kernels, compiled in the kernel's own body like TL_STAGE_DWIN: FIRST (the frame kernel's dB-sum table), then the
// encoder's tables into the workgroup's `sh` (TlMainShared) and the barrier; it leaves B (a TlBlockShared pointer whose dbtable part lies before
// the copied block: the encode path never touches B->dbtable), the wave's index uniform (wave) and as a vector register (wave_v, laundered), and grp
#define TL_ENCODE_PROLOGUE(sh, T, FIRST) \
    { \
        FIRST; \
        const double *src = (const double *)&(T)->shared.scalefactor[0]; \
        double *dst = (double *)&(sh).bytes[0]; \
        for (int i = (int)threadIdx.x; i < (int)(sizeof((sh).bytes) / 8); i += 64 * TL_MAIN_WAVES) dst[i] = src[i]; \
        for (int i = (int)threadIdx.x; i < 512; i += 64 * TL_MAIN_WAVES) (sh).enw_s[i] = (T)->enwindow_s[i]; \
        for (int i = (int)threadIdx.x; i < (int)(sizeof(TlPackTables) / 8); i += 64 * TL_MAIN_WAVES) ((double *)&(sh).pack)[i] = ((const double *)&(T)->pack)[i]; \
    } \
    __syncthreads(); \
    const TlBlockShared *B = (const TlBlockShared *)((const char *)&(sh).bytes[0] - offsetof(TlBlockShared, scalefactor)); \
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); \
    const int grp = (int)blockIdx.x & 7; \
    int wave_v = (int)(threadIdx.x >> 6); \
    asm volatile("" : "+v"(wave_v))
