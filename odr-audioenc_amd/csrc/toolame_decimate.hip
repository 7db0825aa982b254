// toolame_decimate.hip -- the kernel of the device decimator (tlb_decimate_*; csrc/mp2_decimate.h).  A translation unit of its own: the code
// objects of the encode, decode, ingest, monitor, compare, resample and feed kernels are not touched by anything here.
// One workgroup of TL_DC_WAVES waves per (frame, stream) slot, 21.0 KB of LDS: the ratio's table (11.5 KB at the padded row stride; it
// comes out of L2, 10 KB per slot for 80/147) and the slot's source frames with the 63 before them (9.5 KB).  Per stereo slot 147 456 integer
// multiply-adds over 1152 x (8 ds_read_b128 + 64 ds_read_b32, or 32 ds_read_b64 for 1/2).  A slot without a down source is neither read nor
// written; the branch is uniform over the workgroup, which therefore reaches the barrier as a whole or not at all.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "mp2_decimate.h"
#include "tl_kernel_util.h"
#include "tl_kernels.h"

__global__ void __launch_bounds__(64 * TL_DC_WAVES) tl_decimate_kernel(const int16_t *__restrict__ wide, int16_t *__restrict__ out, uint32_t *state,
                                                                       const int32_t *__restrict__ ratio, const int16_t *__restrict__ taps,
                                                                       const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip)
{
    __shared__ TlDecimateLds w;
    const size_t slot = blockIdx.x;
    const int s = (int)(slot % (size_t)nstreams), f = (int)(slot / (size_t)nstreams);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const TlDecimateSlot S = tl_decimate_slot(ratio, state, configs[stream_cfg[s]].nch, s, f, nstreams, nframes, flip);
    if (S.ratio == TL_DC_OFF) return;
    tl_decimate_before(wide, state, taps, w, S, s, f, nstreams, flip, wave);
    __syncthreads();
    tl_decimate_after(state, out, w, S, s, f, nstreams, nframes, flip, wave);
}

hipError_t tlk_decimate(unsigned blocks, hipStream_t st, const int16_t *wide, int16_t *out, uint32_t *state, const int32_t *ratio, const int16_t *taps,
                        const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip)
{
    hipLaunchKernelGGL(tl_decimate_kernel, dim3(blocks), dim3(64 * TL_DC_WAVES), 0, st, wide, out, state, ratio, taps, configs, stream_cfg, nstreams, nframes, flip);
    return hipGetLastError();
}
