// toolame_resample.hip -- the kernel of the device resampler (tlb_resample_*; csrc/mp2_resample.h).  A translation unit of its own: the code
// objects of the encode, decode, ingest, monitor and compare kernels are not touched by anything here.
// One workgroup of TL_RS_WAVES waves per (frame, stream) slot, 17.2 KB of LDS: the ratio's table (12.8 KB at the padded row stride; it
// comes out of L2, 10 KB per slot) and the slot's source frames with the 31 before them (4.4 KB).  Per stereo slot 73 728 integer
// multiply-adds over 1152 x (4 ds_read_b128 + 32 ds_read_b32).  A slot without a source is copied in 16-byte pieces and takes no LDS
// traffic; the branch is uniform over the workgroup, which therefore reaches the barrier as a whole or not at all.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_resample.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64 * TL_RS_WAVES) tl_resample_kernel(const int16_t *__restrict__ source, int16_t *__restrict__ out, uint32_t *state,
                                                                       const int32_t *__restrict__ ratio, const int16_t *__restrict__ taps,
                                                                       const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip)
{
    __shared__ TlResampleLds w;
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)nstreams), f = (int)(slot / (size_t)nstreams);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TlResampleSlot S = tl_resample_slot(ratio, state, configs[stream_cfg[s]].nch, s, f, nstreams, nframes, flip);
    tl_resample_before(source, state, taps, out, w, S, s, f, nstreams, flip, wave);
    if (S.ratio == TL_RS_OFF) return;
    __syncthreads();
    tl_resample_after(state, out, w, S, s, f, nstreams, nframes, flip, wave);
}

hipError_t tlk_resample(unsigned blocks, hipStream_t st, const int16_t *source, int16_t *out, uint32_t *state, const int32_t *ratio, const int16_t *taps,
                        const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip)
{
    hipLaunchKernelGGL(tl_resample_kernel, dim3(blocks), dim3(64 * TL_RS_WAVES), 0, st, source, out, state, ratio, taps, configs, stream_cfg, nstreams, nframes, flip);
    return hipGetLastError();
}
