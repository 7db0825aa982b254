// tl_kernels.h -- the one door between the host translation units (csrc/Makefile: HOST_UNITS, plain C++, seconds to compile) and the
// kernels (KERNEL_UNITS: the only files that see mp2_wave.h).  Each launcher queues ONE kernel on
// `st` and returns hipGetLastError(); grid shapes that depend on the kernels' wave counts are computed from the constants below.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "mp2_types.h"
#include "edi_types.h"
#include "mp2_dec_types.h"
#include "mp2_compare.h"
#include "mp2_resample.h"
#include "mp2_decimate.h"
#include "mp2_feed_adapt.h"
#include "mp2_feed_down.h"
#include "mp2_conceal.h"
#include "mp2_conceal_conv.h"
#include "mp2_loudness.h"
#include "mp2_truepeak.h"
#include "mp2_limiter.h"

#define TL_HEAD_STRIDE 32             // int32 per list head of the persistent kernels' work lists: one 128-byte line each (9 heads)
#ifndef TL_MAIN_WPE
#define TL_MAIN_WPE 3                 // waves per SIMD of the encode kernels
#endif
#define TL_MAIN_WAVES (4 * TL_MAIN_WPE)       // one workgroup per CU: one copy of the tables
#ifndef TL_PSY2_WAVES
#define TL_PSY2_WAVES 12
#endif

// toolame_hip.hip (tl_psy2_kernel: toolame_psy2.hip): the encode path
hipError_t tlk_slots(unsigned blocks, hipStream_t st, const TlLaunch &A);                         // tl_slots_kernel, 256 threads
hipError_t tlk_frame(int psy, bool pairs, bool stereo, unsigned blocks, hipStream_t st, const TlLaunch &A);    // tl_frame_kernel<1|3, pairs, stereo ? 2 : 0>
hipError_t tlk_main(int psy, bool pairs, bool stereo, unsigned blocks, hipStream_t st, const TlLaunch &A);     // tl_main_kernel<0|2, pairs, stereo ? 2 : 0>
hipError_t tlk_psy2(unsigned blocks, hipStream_t st, const TlLaunch &A);                          // tl_psy2_kernel
hipError_t tlk_finish(unsigned blocks, hipStream_t st, const TlLaunch &A);                        // tl_finish_kernel, 256 threads = 4 streams
hipError_t tlk_flush(unsigned blocks, hipStream_t st, const TlStreamState *state, const TlConfig *configs, const int32_t *stream_cfg,
                     uint8_t *out, int32_t *out_len, int nstreams, int out_stride);
// toolame_egress.hip: tl_zmq_frame_kernel (one workgroup per message slot), tl_edi_af_kernel and tl_edi_pft_kernel (one wavefront per packet)
hipError_t tlk_zmq_frame(unsigned blocks, hipStream_t st, const uint8_t *frames, const int16_t *peaks, uint8_t *msgs, const TlConfig *configs,
                         const int32_t *stream_cfg, int nstreams, int out_stride, int msg_stride, int max_upf, const int32_t *frame_len);
hipError_t tlk_edi_af(unsigned bx, unsigned by, hipStream_t st, const TlEdiArgs &A);
hipError_t tlk_edi_pft(unsigned bx, unsigned by, hipStream_t st, const TlPftArgs &A, const TlTables *T);
// toolame_dec.hip: tl_unpack_kernel over every (stream, slot) of the launch, tl_synth_kernel when A.pcm is set, then tl_dec_carry_kernel per stream
hipError_t tlk_decode(hipStream_t st, const TlDecLaunch &A);
// toolame_feed.hip: tl_feed_kernel over every (stream, slot) of the launch, then tl_feed_carry_kernel per stream
hipError_t tlk_feed(hipStream_t st, const TlFeedLaunch &A);
// toolame_conceal.hip: behind tlk_feed on the same stream when some stream has concealment on: tl_conceal_kernel over every (stream, slot)
// of the launch, then tl_conceal_carry_kernel per stream (csrc/mp2_conceal.h)
hipError_t tlk_conceal(hipStream_t st, const TlConcealLaunch &A);
// toolame_feed_adapt.hip: the decode kernel over every (stream, slot) of the call, the resample kernel (one workgroup per slot), then the carry kernel per stream.
// cc (some adapted stream has concealment on): tlk_conceal_adapt behind the decode kernel and tlk_conceal_adapt_carry behind the carry kernel
hipError_t tlk_feed_adapt(hipStream_t st, const TlFeedAdaptLaunch &A, const TlConcealConv *cc = nullptr);
// toolame_feed_down.hip: the decode kernel over every (stream, slot) of the call with two slots per tick, the decimate kernel (one workgroup per tick and stream), then the carry kernel per stream.
// cc (some stream with a down feed has concealment on): tlk_conceal_down behind the decode kernel and tlk_conceal_down_carry behind the carry kernel
hipError_t tlk_feed_down(hipStream_t st, const TlFeedDownLaunch &A, const TlConcealConv *cc = nullptr);
// toolame_conceal_conv.hip (csrc/mp2_conceal_conv.h), one kernel each: tl_conceal_adapt_kernel over every (tick, stream), tl_conceal_down_kernel over every
// (tick, stream, slot), and their carry kernels per stream
hipError_t tlk_conceal_adapt(hipStream_t st, const TlConcealAdaptLaunch &A);
hipError_t tlk_conceal_adapt_carry(hipStream_t st, const TlConcealAdaptLaunch &A);
hipError_t tlk_conceal_down(hipStream_t st, const TlConcealDownLaunch &A);
hipError_t tlk_conceal_down_carry(hipStream_t st, const TlConcealDownLaunch &A);
// toolame_ingest.hip: tl_ingest_valid_kernel, or tl_ingest_kernel when valid (int32 [nframes][nstreams]) is NULL (one workgroup per slot);
// tl_silence_kernel and tl_underrun_kernel (256 threads, one per stream)
hipError_t tlk_ingest(unsigned blocks, hipStream_t st, const int16_t *in, const int32_t *valid /* may be NULL */, int16_t *out, int16_t *peaks, const double *gain,
                      const TlConfig *configs, const int32_t *stream_cfg, int nstreams);
hipError_t tlk_silence(unsigned blocks, hipStream_t st, const int16_t *peaks, uint32_t *silence_ms, const TlConfig *configs,
                       const int32_t *stream_cfg, int nstreams, int nframes);
hipError_t tlk_underrun(unsigned blocks, hipStream_t st, const int32_t *valid, uint32_t *underrun_ms, uint32_t *underruns, const TlConfig *configs,
                        const int32_t *stream_cfg, int nstreams, int nframes);
// toolame_monitor.hip: tl_monitor_kernel, one wavefront per stream over the stream's slots in order (csrc/mp2_monitor.h); record uint32 [nstreams][8]
hipError_t tlk_monitor(hipStream_t st, const TlFrameReport *report, const int16_t *pcm, uint32_t *record, const TlConfig *configs,
                       const int32_t *stream_cfg, int nstreams, int nframes);
// toolame_compare.hip: tl_compare_kernel, one wavefront per stream over the stream's slots in order (csrc/mp2_compare.h); in / report may be NULL
hipError_t tlk_compare(hipStream_t st, const int16_t *in, const int16_t *dec, const TlFrameReport *report, int16_t *hist, TlCompareRecord *record,
                       const TlCompareParams &P, const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes);
// toolame_resample.hip: tl_resample_kernel, one workgroup per (frame, stream) slot (csrc/mp2_resample.h); state uint32 [2][nstreams][32] and ratio
// int32 [nstreams] may both be NULL (no stream has a source: every slot is copied)
hipError_t tlk_resample(unsigned blocks, hipStream_t st, const int16_t *source, int16_t *out, uint32_t *state, const int32_t *ratio, const int16_t *taps,
                        const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip);
// toolame_decimate.hip: tl_decimate_kernel, one workgroup per (frame, stream) slot (csrc/mp2_decimate.h); wide int16 [nframes][nstreams][4608], state
// uint32 [2][nstreams][64], ratio int32 [nstreams] (TL_DC_*; the slots of a TL_DC_OFF stream are left alone)
hipError_t tlk_decimate(unsigned blocks, hipStream_t st, const int16_t *wide, int16_t *out, uint32_t *state, const int32_t *ratio, const int16_t *taps,
                        const TlConfig *configs, const int32_t *stream_cfg, int nstreams, int nframes, int flip);
// toolame_loudness.hip: tl_loudness_kernel, one wave per 32 consecutive streams over the call's frames in order (csrc/mp2_loudness.h);
// tl_loudness_programme_kernel, one lane per stream (tables: the whole table, the kernel takes its centres)
hipError_t tlk_loudness(hipStream_t st, const TlLoudnessArgs &A);
hipError_t tlk_loudness_programme(hipStream_t st, const uint32_t *hist, const double *tables, TlLoudnessProgramme *out, int nstreams);
// ... tl_lra_kernel, the same wave counting range blocks too, launched in tl_loudness_kernel's place; tl_lra_range_kernel, one lane per stream
hipError_t tlk_lra(hipStream_t st, const TlLraArgs &X);
hipError_t tlk_lra_range(hipStream_t st, const uint32_t *hist_st, const double *tables, TlLraRecord *out, int nstreams);
// toolame_truepeak.hip: tl_truepeak_kernel, one wave per stream over the call's frames in order (csrc/mp2_truepeak.h)
hipError_t tlk_truepeak(hipStream_t st, const TlTruePeakArgs &A);
// toolame_limiter.hip: tl_limiter_kernel, one wave per stream over the call's frames in order, in place (csrc/mp2_limiter.h)
hipError_t tlk_limiter(hipStream_t st, const TlLimiterArgs &A);
size_t tlk_lds_bytes_per_wave(void);          // the largest per-wave LDS block among the kernels
