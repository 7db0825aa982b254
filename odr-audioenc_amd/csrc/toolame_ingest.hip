// toolame_ingest.hip -- the kernels of the caller's glue (tlb_ingest_*, tlb_silence_*, tlb_underrun_*; csrc/mp2_ingest.h): gain, peak and
// de-interleave with or without short reads, the silence counter, the underrun counters.  A translation unit of its own: the code objects
// of the encode and decode kernels are not touched by anything here.  Host side: tlb_ingest.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_ingest.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

// Ingest glue of the caller (src/odr-audioenc.cpp:1030-1051 gain + peak, :1139-1152 de-interleave, and before them
// the stretch of a short read, :335-373): one workgroup per (frame, stream) slot, a wave's share is tl_ingest_wave.
// in  [nframes][nstreams][2304] int16 (L R L R ...; mono streams use the first 1152 values), valid int32 [nframes][nstreams]
// out [nframes][nstreams][2][1152] int16, peaks [nframes][nstreams][2] int16
// The two kernels are the same three steps and differ in the middle one alone.  The steps are called from the kernels' own bodies: with
// tl_ingest_wave inside one more shared function, the compiler simplified that function before it inlined it and
// tl_ingest_valid_kernel's code moved (two instructions, another schedule).
// step 1 -- this workgroup's slot, its stream's channel count and gain
static __device__ __forceinline__ size_t tl_ingest_slot(const double *gain, const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int &nch, double &g)
{
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)nstreams);
    nch = configs[stream_cfg[s]].nch;
    g = gain[s];
    return slot;
}
// step 3 -- the slot's peaks: the maximum over its waves' peaks (each uniform over its wave)
static __device__ __forceinline__ void tl_ingest_peaks(int16_t *peaks, size_t slot, int wave, int pk0, int pk1)
{
    __shared__ int red[2][TL_INGEST_WAVES];
    if ((threadIdx.x & 63) == 0) { red[0][wave] = pk0; red[1][wave] = pk1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int m = red[threadIdx.x][0];
        for (int k = 1; k < TL_INGEST_WAVES; k++) m = red[threadIdx.x][k] > m ? red[threadIdx.x][k] : m;
        peaks[slot * 2 + threadIdx.x] = (int16_t)m;
    }
}
// no `valid` array: every slot is a full read (16 bytes per lane and step); no `valid` word is loaded and the gather is not in the kernel
__global__ void __launch_bounds__(64 * TL_INGEST_WAVES) tl_ingest_kernel(const int16_t *__restrict__ in, int16_t *__restrict__ out,
                                                                         int16_t *__restrict__ peaks, const double *__restrict__ gain,
                                                                         const TlConfig *configs, const int32_t *stream_cfg, int nstreams)
{
    int nch, pk0, pk1; double g;
    const size_t slot = tl_ingest_slot(gain, configs, stream_cfg, nstreams, nch, g);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    tl_ingest_wave<true>(in + slot * 2304, out + slot * 2304, nch, g, TL_INGEST_FRAMES, wave, pk0, pk1);
    tl_ingest_peaks(peaks, slot, wave, pk0, pk1);
}
// the branch on the slot's `valid` is uniform over the workgroup: a full slot runs what tl_ingest_kernel runs, a short one the gather
__global__ void __launch_bounds__(64 * TL_INGEST_WAVES) tl_ingest_valid_kernel(const int16_t *__restrict__ in, const int32_t *__restrict__ valid_in, int16_t *__restrict__ out,
                                                                               int16_t *__restrict__ peaks, const double *__restrict__ gain,
                                                                               const TlConfig *configs, const int32_t *stream_cfg, int nstreams)
{
    int nch, pk0, pk1; double g;
    const size_t slot = tl_ingest_slot(gain, configs, stream_cfg, nstreams, nch, g);
    const int valid = tl_ingest_clamp(valid_in[slot]);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (valid == TL_INGEST_FRAMES) tl_ingest_wave<true>(in + slot * 2304, out + slot * 2304, nch, g, valid, wave, pk0, pk1);
    else tl_ingest_wave<false>(in + slot * 2304, out + slot * 2304, nch, g, valid, wave, pk0, pk1);
    tl_ingest_peaks(peaks, slot, wave, pk0, pk1);
}

// The two counters of the caller (tl_silence_stream, tl_underrun_stream): one thread per stream, frames in order
__global__ void __launch_bounds__(256) tl_silence_kernel(const int16_t *__restrict__ peaks, uint32_t *__restrict__ silence_ms, const TlConfig *configs,
                                                          const int32_t *stream_cfg, int nstreams, int nframes)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= nstreams) return;
    const TlConfig &c = configs[stream_cfg[s]];
    tl_silence_stream(peaks, silence_ms, tl_frame_ms(c.version, c.fs_idx, c.nch), s, nstreams, nframes);
}
__global__ void __launch_bounds__(256) tl_underrun_kernel(const int32_t *__restrict__ valid, uint32_t *__restrict__ underrun_ms, uint32_t *__restrict__ underruns,
                                                           const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= nstreams) return;
    const TlConfig &c = configs[stream_cfg[s]];
    tl_underrun_stream(valid, underrun_ms, underruns, tl_frame_ms(c.version, c.fs_idx, c.nch), s, nstreams, nframes);
}

#define TLK_GO(...) do { hipLaunchKernelGGL(__VA_ARGS__); return hipGetLastError(); } while (0)
hipError_t tlk_ingest(unsigned blocks, hipStream_t st, const int16_t *in, const int32_t *valid, int16_t *out, int16_t *peaks, const double *gain,
                      const TlConfig *configs, const int32_t *stream_cfg, int nstreams)
{
    const dim3 g(blocks), t(64 * TL_INGEST_WAVES);
    if (valid) TLK_GO(tl_ingest_valid_kernel, g, t, 0, st, in, valid, out, peaks, gain, configs, stream_cfg, nstreams);
    TLK_GO(tl_ingest_kernel, g, t, 0, st, in, out, peaks, gain, configs, stream_cfg, nstreams);
}
hipError_t tlk_silence(unsigned blocks, hipStream_t st, const int16_t *peaks, uint32_t *silence_ms, const TlConfig *configs,
                       const int32_t *stream_cfg, int nstreams, int nframes)
{
    TLK_GO(tl_silence_kernel, dim3(blocks), dim3(256), 0, st, peaks, silence_ms, configs, stream_cfg, nstreams, nframes);
}
hipError_t tlk_underrun(unsigned blocks, hipStream_t st, const int32_t *valid, uint32_t *underrun_ms, uint32_t *underruns, const TlConfig *configs,
                        const int32_t *stream_cfg, int nstreams, int nframes)
{
    TLK_GO(tl_underrun_kernel, dim3(blocks), dim3(256), 0, st, valid, underrun_ms, underruns, configs, stream_cfg, nstreams, nframes);
}
#undef TLK_GO
