// tlb_decode.cpp -- the frame check / decode entry points of include/toolame_batch.h (tlb_decode_*): argument checks, the decoder's tables
// and per-stream state (allocated by the first call), one launch of the kernels of toolame_dec.hip through tl_kernels.h.  Host C++.
#include "tlb_internal.h"

static_assert(TLB_DEC_EMPTY == TL_DEC_EMPTY && TLB_DEC_BAD_SYNC == TL_DEC_BAD_SYNC && TLB_DEC_HEADER_MISMATCH == TL_DEC_HEADER_MISMATCH &&
              TLB_DEC_BAD_CRC16 == TL_DEC_BAD_CRC16 && TLB_DEC_BAD_SCFCRC == TL_DEC_BAD_SCFCRC && TLB_DEC_SCFCRC_UNCHECKED == TL_DEC_SCFCRC_UNCHECKED &&
              TLB_DEC_BAD_ALLOC == TL_DEC_BAD_ALLOC && TLB_DEC_OVERRUN == TL_DEC_OVERRUN && TLB_DEC_BAD_MASK == TL_DEC_BAD_MASK, "status flags");
static_assert(sizeof(tlb_frame_report) == sizeof(TlFrameReport) && sizeof(tlb_frame_fields) == sizeof(TlFrameFields), "C-ABI records");

// The one pattern of a first-use allocation (csrc/tlb_mem.h): stage in a local owner, upload the tables, settle, commit, then set the fields.
int synth_prepare(tlb_batch *b)
{
    if (b->d_synth) return TLB_OK;
    TlbMem m;
    TlSynthTables *synth = m.scratch<TlSynthTables>(1);
    TlSynthTables *hy = new TlSynthTables;
    tl_build_synth_tables(hy);
    m.upload(synth, hy, sizeof(TlSynthTables));
    delete hy;
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_synth = synth;
    return TLB_OK;
}

int decode_prepare(tlb_batch *b)
{
    if (b->d_dec_state) return TLB_OK;
    if (int rc = synth_prepare(b)) return rc;
    const size_t n = (size_t)b->nstreams;
    TlbMem m;
    TlDecStream *state = m.dev<TlDecStream>(n);
    uint8_t *prev = m.dev<uint8_t>(n * (size_t)b->out_stride);
    unsigned long long *bad = m.dev<unsigned long long>(1);
    if (!m.settle()) return TLB_ERR_HIP;         // the first call (only) waits for the device
    m.commit(b->mem);
    b->d_dec_state = state; b->d_dec_prev = prev; b->d_dec_bad = bad;
    return TLB_OK;
}

extern "C" {

int tlb_decode_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, tlb_frame_report *d_report,
                      tlb_frame_fields *d_fields, int16_t *d_pcm, void *hip_stream)
{
    if (!b || !d_frames || !d_report || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    // the kernels move frames and PCM as 32-bit words and store 32-bit report fields
    if (((uintptr_t)d_frames | (uintptr_t)d_report | (uintptr_t)d_len | (uintptr_t)d_fields | (uintptr_t)d_pcm) & 3u) return TLB_ERR_ARG;
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    HIPCHK(hipSetDevice(b->device));
    if (int rc = decode_prepare(b)) return rc;
    TlDecLaunch A;
    memset(&A, 0, sizeof A);
    A.tables = b->d_tables; A.configs = b->d_configs; A.stream_cfg = b->h_configs.size() == 1 ? nullptr : b->d_stream_cfg;
    A.synth = b->d_synth; A.frames = d_frames; A.len = d_len;
    A.report = (TlFrameReport *)d_report; A.fields = (TlFrameFields *)d_fields; A.pcm = d_pcm;
    A.state = b->d_dec_state; A.prev = b->d_dec_prev; A.bad = b->d_dec_bad;
    A.nstreams = b->nstreams; A.nframes = nframes; A.out_stride = b->out_stride;
    HIPCHK(tlk_decode((hipStream_t)hip_stream, A));
    return TLB_OK;
}

int tlb_decode_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int nframes, tlb_frame_report *report,
                    tlb_frame_fields *fields, int16_t *pcm)
{
    if (!b || !frames || !report || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    const size_t slots = (size_t)nframes * (size_t)b->nstreams;
    TlbMem m;
    uint8_t *d_frames = m.scratch<uint8_t>(slots * (size_t)b->out_stride); tlb_frame_report *d_report = m.scratch<tlb_frame_report>(slots);
    int32_t *d_len = len ? m.scratch<int32_t>(slots) : nullptr; tlb_frame_fields *d_fields = fields ? m.scratch<tlb_frame_fields>(slots) : nullptr;
    int16_t *d_pcm = pcm ? m.scratch<int16_t>(slots * 2 * TLB_SAMPLES_PER_FRAME) : nullptr;
    MEMCHK(m);
    HIPCHK(hipMemcpy(d_frames, frames, slots * (size_t)b->out_stride, hipMemcpyHostToDevice));
    if (len) HIPCHK(hipMemcpy(d_len, len, slots * sizeof(int32_t), hipMemcpyHostToDevice));
    if (int rc = tlb_decode_device(b, d_frames, d_len, nframes, d_report, d_fields, d_pcm, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(report, d_report, slots * sizeof(tlb_frame_report), hipMemcpyDeviceToHost));
    if (fields) HIPCHK(hipMemcpy(fields, d_fields, slots * sizeof(tlb_frame_fields), hipMemcpyDeviceToHost));
    if (pcm) HIPCHK(hipMemcpy(pcm, d_pcm, slots * 2 * TLB_SAMPLES_PER_FRAME * sizeof(int16_t), hipMemcpyDeviceToHost));
    return TLB_OK;
}

int tlb_decode_reset(tlb_batch *b, int stream)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    if (!b->d_dec_state) return TLB_OK;          // never decoded: every stream's next frame is a first frame already
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (stream < 0) HIPCHK(hipMemset(b->d_dec_state, 0, sizeof(TlDecStream) * (size_t)b->nstreams));
    else HIPCHK(hipMemset(b->d_dec_state + stream, 0, sizeof(TlDecStream)));
    return TLB_OK;
}

long tlb_decode_bad_frames(const tlb_batch *b)
{
    if (!b) return -TLB_ERR_ARG;
    if (!b->d_dec_bad) return 0;
    unsigned long long n = 0;
    if (hipSetDevice(b->device) != hipSuccess || hipDeviceSynchronize() != hipSuccess ||
        hipMemcpy(&n, b->d_dec_bad, sizeof n, hipMemcpyDeviceToHost) != hipSuccess) return -TLB_ERR_HIP;
    return (long)n;
}

}  // extern "C"
