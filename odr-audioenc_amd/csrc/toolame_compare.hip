// toolame_compare.hip -- the kernel of the compare monitor (tlb_compare_*; csrc/mp2_compare.h).  A translation unit of its own: the code
// objects of the encode, decode, ingest and monitor kernels are not touched by anything here.
// One wavefront per stream, TL_CMP_WAVES streams per workgroup, each with its stream's history (3.2 KB per channel) in LDS while it walks
// the call's slots.  Memory-bound, all of it in 16-byte pieces: per (stream, frame) 9.2 KB of PCM are read (4.6 KB for one channel), and per
// CALL the history comes in and goes back out, 6.4 KB each way for two channels.  Over a call of many frames the PCM read is the bound; in
// the tick, where a call is one frame, the history's round trip (12.8 KB) outweighs it.  The record is written back by one lane with
// ordinary vector stores.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_compare.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64 * TL_CMP_WAVES) tl_compare_kernel(const int16_t *__restrict__ in, const int16_t *__restrict__ dec, const TlFrameReport *__restrict__ report,
                                                                       int16_t *__restrict__ hist, TlCompareRecord *__restrict__ record, TlCompareParams P,
                                                                       const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes)
{
    __shared__ TlCmpLds lds[TL_CMP_WAVES];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = (int)blockIdx.x * TL_CMP_WAVES + wave;
    if (s >= nstreams) return;                   // (no workgroup barrier anywhere below: the waves of a workgroup are independent)
    tl_compare_stream(in, dec, report, hist, record, P, lds[wave], configs[stream_cfg[s]].nch, s, nstreams, nframes);
}

hipError_t tlk_compare(hipStream_t st, const int16_t *in, const int16_t *dec, const TlFrameReport *report, int16_t *hist, TlCompareRecord *record,
                       const TlCompareParams &P, const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes)
{
    hipLaunchKernelGGL(tl_compare_kernel, dim3((unsigned)((nstreams + TL_CMP_WAVES - 1) / TL_CMP_WAVES)), dim3(64 * TL_CMP_WAVES), 0, st,
                       in, dec, report, hist, record, P, configs, stream_cfg, nstreams, nframes);
    return hipGetLastError();
}
