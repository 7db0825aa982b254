// toolame_monitor.hip -- the kernel of the confidence monitor's fold (tlb_monitor_*; csrc/mp2_monitor.h).  A translation unit of its own:
// the code objects of the encode, decode and ingest kernels are not touched by anything here.
// One wavefront per stream, TL_MON_WAVES streams per workgroup; the kernel reads 4.6 KB of decoded PCM per (stream, frame) and is bound by
// that read.  The record is written back by one lane with ordinary vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_monitor.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64 * TL_MON_WAVES) tl_monitor_kernel(const TlFrameReport *__restrict__ report, const int16_t *__restrict__ pcm, uint32_t *__restrict__ record,
                                                                       const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes)
{
    const int s = (int)blockIdx.x * TL_MON_WAVES + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (s >= nstreams) return;
    const TlConfig &c = configs[stream_cfg[s]];
    tl_monitor_stream(report, pcm, record, tl_frame_ms(c.version, c.fs_idx, c.nch), s, nstreams, nframes);
}

hipError_t tlk_monitor(hipStream_t st, const TlFrameReport *report, const int16_t *pcm, uint32_t *record, const TlConfig *configs,
                       const int32_t *stream_cfg, int nstreams, int nframes)
{
    hipLaunchKernelGGL(tl_monitor_kernel, dim3((unsigned)((nstreams + TL_MON_WAVES - 1) / TL_MON_WAVES)), dim3(64 * TL_MON_WAVES), 0, st,
                       report, pcm, record, configs, stream_cfg, nstreams, nframes);
    return hipGetLastError();
}
