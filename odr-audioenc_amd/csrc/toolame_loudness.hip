// toolame_loudness.hip -- the kernels of the device loudness meter (tlb_loudness_*; csrc/mp2_loudness.h).  A translation unit of its own: the
// code objects of the encode, decode, ingest, monitor, compare, resample, decimate and feed kernels are not touched by anything here.
// tl_loudness_kernel: one wave per workgroup and per 32 consecutive streams, one lane per (stream, channel), 9216 bytes of LDS (64 rows of
// 64 samples at a pitch of 144 bytes); per stereo frame and stream 2 x 1152 x 20 dependent fp64 operations.  At 16 384 streams that is
// 512 waves, two per CU: the kernel is bound by the latency of the recurrence, not by the PCM it reads once (4.6 KB per stream and frame).
// tl_loudness_programme_kernel: one lane per stream over its 751 counts, twice.
// tl_lra_kernel: tl_loudness_kernel's body counting every short-term value as a range block too (tlb_lra_*), same geometry and LDS; a batch
// that enabled the loudness range launches it INSTEAD, and tl_loudness_kernel is the code it was.  tl_lra_range_kernel: one lane per stream
// over its 751 range-block counts, three times.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_loudness.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64) tl_loudness_kernel(const TlLoudnessArgs A)
{
    __shared__ TlLoudnessLds w;
    tl_loudness_wave(A, w, (int)blockIdx.x);
}

__global__ void __launch_bounds__(256) tl_loudness_programme_kernel(const uint32_t *__restrict__ hist, const double *__restrict__ centres,
                                                                    TlLoudnessProgramme *__restrict__ out, int nstreams)
{
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s < nstreams) tl_loudness_programme(hist, centres, out, s, nstreams);
}

__global__ void __launch_bounds__(64) tl_lra_kernel(const TlLraArgs X)
{
    __shared__ TlLoudnessLds w;
    tl_lra_wave(X, w, (int)blockIdx.x);
}

__global__ void __launch_bounds__(256) tl_lra_range_kernel(const uint32_t *__restrict__ hist, const double *__restrict__ centres,
                                                           TlLraRecord *__restrict__ out, int nstreams)
{
    const int s = (int)(blockIdx.x * 256u + threadIdx.x);
    if (s < nstreams) tl_lra_range(hist, centres, out, s, nstreams);
}

hipError_t tlk_loudness(hipStream_t st, const TlLoudnessArgs &A)
{
    hipLaunchKernelGGL(tl_loudness_kernel, dim3((unsigned)((A.nstreams + TL_LD_STREAMS - 1) / TL_LD_STREAMS)), dim3(64), 0, st, A);
    return hipGetLastError();
}

hipError_t tlk_loudness_programme(hipStream_t st, const uint32_t *hist, const double *tables, TlLoudnessProgramme *out, int nstreams)
{
    hipLaunchKernelGGL(tl_loudness_programme_kernel, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, st, hist, tables + TL_LD_RATES * 10 + TL_LD_BINS, out, nstreams);
    return hipGetLastError();
}

hipError_t tlk_lra(hipStream_t st, const TlLraArgs &X)
{
    hipLaunchKernelGGL(tl_lra_kernel, dim3((unsigned)((X.A.nstreams + TL_LD_STREAMS - 1) / TL_LD_STREAMS)), dim3(64), 0, st, X);
    return hipGetLastError();
}

hipError_t tlk_lra_range(hipStream_t st, const uint32_t *hist_st, const double *tables, TlLraRecord *out, int nstreams)
{
    hipLaunchKernelGGL(tl_lra_range_kernel, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, st, hist_st, tables + TL_LD_RATES * 10 + TL_LD_BINS, out, nstreams);
    return hipGetLastError();
}
