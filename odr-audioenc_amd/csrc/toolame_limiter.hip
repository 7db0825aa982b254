// toolame_limiter.hip -- the kernel of the device true-peak limiter (tlb_limiter_*; csrc/mp2_limiter.h).  A translation unit of its own: the
// code objects of the encode, decode, ingest, monitor, compare, resample, decimate, feed, loudness and true-peak kernels are not touched by
// anything here.
// tl_limiter_kernel: one wave per workgroup and per stream, a lane per 18 consecutive samples, 11 152 bytes of LDS (two rows of 64 + 1152
// int16, the lanes' suffix minima / gains at 19 words a lane, the carried lanes twice); per stereo frame and stream the meter's 2 x 64 x 324
// packed dot2 for the detector, 4608 bytes of PCM read once and written once.
#include <hip/hip_runtime.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_limiter.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64) tl_limiter_kernel(const TlLimiterArgs A)
{
    __shared__ TlLimiterLds w;
    tl_limiter_wave(A, w, (int)blockIdx.x);
}

hipError_t tlk_limiter(hipStream_t st, const TlLimiterArgs &A)
{
    hipLaunchKernelGGL(tl_limiter_kernel, dim3((unsigned)A.nstreams), dim3(64), 0, st, A);
    return hipGetLastError();
}
