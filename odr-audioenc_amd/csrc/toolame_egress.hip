// toolame_egress.hip -- the kernels of the step after the encode path and their launchers (tl_kernels.h): ZeroMQ messages, EDI AF packets
// and the PFT layer (csrc/edi_af.h, csrc/edi_pft.h).  A translation unit of its own: the code objects of the other kernels are not touched
// by anything here.  Host side: tlb_egress.cpp.
#include <hip/hip_runtime.h>
#include <math.h>
#include "mp2_host.h"
#include "mp2_wave.h"
#include "edi_af.h"
#include "edi_pft.h"
#include "tl_kernels.h"

// ZeroMQ wire format of the step after the path (src/Outputs.h:76-99, Outputs.cpp:101-138):
// packed header {u16 version=1, u16 encoder=2 (MPEG L2), u32 datasize, i16 level_left, i16 level_right} + the unit's bytes.
// One message per UNIT of 3 * bitrate bytes (src/odr-audioenc.cpp:1211-1219): message slot v = f * max_upf + u carries bytes
// [u * unit, (u + 1) * unit) of frame f; a stream with fewer units per frame leaves its surplus slots empty (datasize 0 in an
// all-zero header).  msgs [nframes * max_upf][nstreams][msg_stride]; one block per slot.
__global__ void tl_zmq_frame_kernel(const uint8_t *__restrict__ frames, const int16_t *__restrict__ peaks, uint8_t *__restrict__ msgs,
                                    const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int out_stride, int msg_stride, int max_upf,
                                    const int32_t *__restrict__ frame_len)
{
    const size_t pslot = blockIdx.x;
    const int s = (int)(pslot % (size_t)nstreams), v = (int)(pslot / (size_t)nstreams), f = v / max_upf, u = v - f * max_upf;
    const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
    const TlConfig &c = configs[stream_cfg[s]];
    const int n = 3 * c.kbps, upf = c.frame_bytes / n;
    uint8_t *m = msgs + pslot * (size_t)msg_stride;
    if (u >= upf || (frame_len && frame_len[slot] == 0)) { if (threadIdx.x < 3) ((uint32_t *)m)[threadIdx.x] = 0u; return; }   // no unit here / no frame in this slot
    if (threadIdx.x < 3) {
        const int pl = peaks ? peaks[slot * 2] : 0, pr = peaks ? peaks[slot * 2 + 1] : 0;
        const uint32_t w = threadIdx.x == 0 ? (1u | (2u << 16)) : threadIdx.x == 1 ? (uint32_t)n
                                            : ((uint32_t)(uint16_t)pl | ((uint32_t)(uint16_t)pr << 16));
        ((uint32_t *)m)[threadIdx.x] = w;
    }
    const uint32_t *src = (const uint32_t *)(frames + slot * (size_t)out_stride + (size_t)u * n);      // unit sizes are multiples of 4
    for (int i = (int)threadIdx.x; i < (n >> 2); i += (int)blockDim.x) ((uint32_t *)m)[3 + i] = src[i];
}

// EDI AF packets of the step after the path (EDI part; csrc/edi_af.h): one wavefront per packet,
// blockIdx.y = packet slot (frame * max_upf + unit) of the call, four streams per workgroup.
__global__ void __launch_bounds__(256) tl_edi_af_kernel(TlEdiArgs A)
{
    const int s = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (s >= A.nstreams) return;
    tl_edi_af_packet(A, s, (int)blockIdx.y);      // blockIdx.y = packet slot
}

// EDI PFT layer (csrc/edi_pft.h): one wavefront per AF packet, blockIdx.y = frame of the call.  The Reed-Solomon tables
// (11 KB) are copied into LDS once per workgroup: the encoder's look-ups are dependent and must not go to global memory.
__global__ void __launch_bounds__(256) tl_edi_pft_kernel(TlPftArgs A, const TlTables *T)
{
    __shared__ uint8_t s_log[256], s_exp[512], s_mlog[207 * TL_PFT_PARITY];
    __shared__ TlPftScratch scratch[4];
    for (int i = (int)threadIdx.x; i < 256; i += 256) s_log[i] = T->rs_log[i];
    for (int i = (int)threadIdx.x; i < 512; i += 256) s_exp[i] = T->rs_exp[i];
    for (int i = (int)threadIdx.x; i < 207 * TL_PFT_PARITY; i += 256) s_mlog[i] = (&T->rs_mlog[0][0])[i];
    __syncthreads();
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int s = (int)blockIdx.x * 4 + wave;
    if (s >= A.nstreams) return;
    const TlPftTables R = {s_log, s_exp, s_mlog};
    tl_edi_pft_packet(A, R, s, (int)blockIdx.y, scratch[wave]);
}

#define TLK_GO(...) do { hipLaunchKernelGGL(__VA_ARGS__); return hipGetLastError(); } while (0)
hipError_t tlk_zmq_frame(unsigned blocks, hipStream_t st, const uint8_t *frames, const int16_t *peaks, uint8_t *msgs, const TlConfig *configs,
                         const int32_t *stream_cfg, int nstreams, int out_stride, int msg_stride, int max_upf, const int32_t *frame_len)
{
    TLK_GO(tl_zmq_frame_kernel, dim3(blocks), dim3(128), 0, st, frames, peaks, msgs, configs, stream_cfg, nstreams, out_stride, msg_stride, max_upf, frame_len);
}
hipError_t tlk_edi_af(unsigned bx, unsigned by, hipStream_t st, const TlEdiArgs &A) { TLK_GO(tl_edi_af_kernel, dim3(bx, by), dim3(256), 0, st, A); }
hipError_t tlk_edi_pft(unsigned bx, unsigned by, hipStream_t st, const TlPftArgs &A, const TlTables *T) { TLK_GO(tl_edi_pft_kernel, dim3(bx, by), dim3(256), 0, st, A, T); }
#undef TLK_GO
