// toolame_ingest.hip -- the kernels of the ingest path with short reads (tlb_ingest_*_valid, tlb_underrun_*; csrc/mp2_ingest.h).  A translation
// unit of its own: the code objects of the encode and decode kernels are not touched by anything here, and tl_ingest_kernel (toolame_hip.hip)
// stays what runs when the caller gives no `valid` array.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_ingest.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

// One workgroup per (frame, stream) slot, as tl_ingest_kernel; in / out / peaks as there, valid int32 [nframes][nstreams].  The branch on the
// slot's `valid` is uniform over the workgroup: a full slot runs the text of tl_ingest_kernel (16-byte loads), a short one the gather.
__global__ void __launch_bounds__(64 * TL_INGEST_WAVES) tl_ingest_valid_kernel(const int16_t *__restrict__ in, const int32_t *__restrict__ valid_in, int16_t *__restrict__ out,
                                                                               int16_t *__restrict__ peaks, const double *__restrict__ gain,
                                                                               const TlConfig *configs, const int32_t *stream_cfg, int nstreams)
{
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)nstreams);
    const int nch = configs[stream_cfg[s]].nch;
    const double g = gain[s];
    const int valid = tl_ingest_clamp(valid_in[slot]);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    int pk0, pk1;
    if (valid == TL_INGEST_FRAMES) tl_ingest_wave<true>(in + slot * 2304, out + slot * 2304, nch, g, valid, wave, pk0, pk1);
    else tl_ingest_wave<false>(in + slot * 2304, out + slot * 2304, nch, g, valid, wave, pk0, pk1);
    __shared__ int red[2][TL_INGEST_WAVES];
    if ((threadIdx.x & 63) == 0) { red[0][wave] = pk0; red[1][wave] = pk1; }
    __syncthreads();
    if (threadIdx.x < 2) {
        int m = red[threadIdx.x][0];
        for (int k = 1; k < TL_INGEST_WAVES; k++) m = red[threadIdx.x][k] > m ? red[threadIdx.x][k] : m;
        peaks[slot * 2 + threadIdx.x] = (int16_t)m;
    }
}

// One thread per stream, frames in order (as tl_silence_kernel)
__global__ void __launch_bounds__(256) tl_underrun_kernel(const int32_t *__restrict__ valid, uint32_t *__restrict__ underrun_ms, uint32_t *__restrict__ underruns,
                                                           const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (s >= nstreams) return;
    const TlConfig &c = configs[stream_cfg[s]];
    tl_underrun_stream(valid, underrun_ms, underruns, tl_frame_ms(c.version, c.fs_idx, c.nch), s, nstreams, nframes);
}

hipError_t tlk_ingest_valid(unsigned blocks, hipStream_t st, const int16_t *in, const int32_t *valid, int16_t *out, int16_t *peaks, const double *gain,
                            const TlConfig *configs, const int32_t *stream_cfg, int nstreams)
{
    hipLaunchKernelGGL(tl_ingest_valid_kernel, dim3(blocks), dim3(64 * TL_INGEST_WAVES), 0, st, in, valid, out, peaks, gain, configs, stream_cfg, nstreams);
    return hipGetLastError();
}
hipError_t tlk_underrun(unsigned blocks, hipStream_t st, const int32_t *valid, uint32_t *underrun_ms, uint32_t *underruns, const TlConfig *configs,
                        const int32_t *stream_cfg, int nstreams, int nframes)
{
    hipLaunchKernelGGL(tl_underrun_kernel, dim3(blocks), dim3(256), 0, st, valid, underrun_ms, underruns, configs, stream_cfg, nstreams, nframes);
    return hipGetLastError();
}
