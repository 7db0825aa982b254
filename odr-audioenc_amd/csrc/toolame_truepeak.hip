// toolame_truepeak.hip -- the kernel of the device true-peak meter (tlb_truepeak_*; csrc/mp2_truepeak.h).  A translation unit of its own: the
// code objects of the encode, decode, ingest, monitor, compare, resample, decimate, feed and loudness kernels are not touched by anything here.
// tl_truepeak_kernel: one wave per workgroup and per stream, a lane per 18 consecutive samples of a channel, 4672 bytes of LDS (two rows of
// 16 + 1152 int16); per stereo frame and stream 2 x 1152 x 3 x 12 multiply-adds as 2 x 64 x 324 packed dot2, and 4608 bytes of PCM read once.
#include <hip/hip_runtime.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_truepeak.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64) tl_truepeak_kernel(const TlTruePeakArgs A)
{
    __shared__ TlTruePeakLds w;
    tl_truepeak_wave(A, w, (int)blockIdx.x);
}

hipError_t tlk_truepeak(hipStream_t st, const TlTruePeakArgs &A)
{
    hipLaunchKernelGGL(tl_truepeak_kernel, dim3((unsigned)A.nstreams), dim3(64), 0, st, A);
    return hipGetLastError();
}
