// mp2_ingest.h -- the ingest glue of the caller's loop: what AudioEnc::run() does to a frame between its input queue and
// toolame_encode_frame() (src/odr-audioenc.cpp): the stretch of a short read over the frame (expand_missing_samples, :335-373, called at
// :910-917), then gain and peak (:1030-1051) and the de-interleave (:1139-1152); and the two counters that go with it, underruns (:919-935)
// and silence (:1053-1079).  One workgroup of TL_INGEST_WAVES waves per (frame, stream) slot; tl_ingest_wave is one wave's share, written
// with the lane macros of mp2_wave.h so that tests/emu/mp2_ingest_emu.cpp runs the same text as lane loops.  Both ingest kernels of
// toolame_ingest.hip are this text: tl_ingest_kernel (no `valid` array) is tl_ingest_wave<true> alone.
//
// The stretch.  `valid` whole sample frames (an L/R pair, or one sample of a one-channel input) were delivered, missing = 1152 - valid.
// The queue zero-fills what it could not deliver (src/SampleQueue.h:217-276), so the stretch reads a buffer whose tail is ZERO whatever
// the caller's buffer holds behind `valid`: those bytes are never loaded here.
//   missing == 0        the frame as it is (the reference does not call the function, :913)
//   missing >= 116      the valid frames followed by zeros (:352-356; `missing * bytes_per_sample > buf.size() / 10` in integers: 115 stretches)
//   1 .. 115            output frame i is source frame src(i) of the zero-tailed buffer, q = valid / missing (integer):
//                       src(0) = 0, src(i) = i - (i - 1) / q -- the closed form of the loop at :361-371, which holds the source index back
//                       after every i that is a positive multiple of q.  With missing == 1 the last output frame is source frame 1151, a
//                       zero of the tail; with larger counts up to 22 valid frames at the end are never used (missing == 105).  Both are
//                       the reference's behaviour and are reproduced.
#pragma once
#include <stdint.h>

#define TL_INGEST_WAVES 4
#define TL_INGEST_FRAMES 1152
#define TL_INGEST_STRETCH_MAX 115     // the largest number of missing frames that is still stretched

#ifdef TL_EMULATE
TL_FN int tlh_max_i32(const int (&v)[64]) { int m = v[0]; for (int i = 1; i < 64; i++) if (v[i] > m) m = v[i]; return m; }
#define TL_WAVE_MAX_I32(name) tlh_max_i32(name)
#define TL_INGEST_LD16(dst, p, q) do { const uint32_t *p_ = (const uint32_t *)(p) + 4 * (q); (dst)[0] = p_[0]; (dst)[1] = p_[1]; (dst)[2] = p_[2]; (dst)[3] = p_[3]; } while (0)
#define TL_INGEST_ST8(p, q, a, b) do { uint32_t *p_ = (uint32_t *)(p) + 2 * (q); p_[0] = (a); p_[1] = (b); } while (0)
#define TL_INGEST_ST16(p, q, a, b, c, d) do { uint32_t *p_ = (uint32_t *)(p) + 4 * (q); p_[0] = (a); p_[1] = (b); p_[2] = (c); p_[3] = (d); } while (0)
#else
TL_FN int tld_max_i32(int v) { for (int o = 32; o; o >>= 1) { const int t = __shfl_xor(v, o, 64); v = t > v ? t : v; } return __builtin_amdgcn_readfirstlane(v); }
#define TL_WAVE_MAX_I32(name) tld_max_i32(name)
#define TL_INGEST_LD16(dst, p, q) do { const uint4 v_ = ((const uint4 *)(p))[q]; (dst)[0] = v_.x; (dst)[1] = v_.y; (dst)[2] = v_.z; (dst)[3] = v_.w; } while (0)
#define TL_INGEST_ST8(p, q, a, b) (((uint2 *)(p))[q] = make_uint2((a), (b)))
#define TL_INGEST_ST16(p, q, a, b, c, d) (((uint4 *)(p))[q] = make_uint4((a), (b), (c), (d)))
#endif

// `valid` as the entry points take it: above 1152 counts as 1152, below 0 as 0
TL_FN int tl_ingest_clamp(int valid) { return valid < 0 ? 0 : valid > TL_INGEST_FRAMES ? TL_INGEST_FRAMES : valid; }

// source frame of output frame i of a stretched slot (q = valid / missing, uniform over the slot)
TL_FN int tl_stretch_src(int i, int q) { return i < 1 ? 0 : i - (int)((unsigned)(i - 1) / (unsigned)q); }

// Wave `wave` of the TL_INGEST_WAVES of a slot: src = the slot's 2304 interleaved values (a one-channel stream uses the first 1152),
// dst = its planar [2][1152] output, valid already clamped (FULL: valid == 1152).  A full slot moves 16 bytes per lane and step (16-byte loads, 8-byte stores); a short
// one gathers the same four words frame by frame (4 bytes an L/R pair, 2 bytes a mono sample), zero where the source frame lies behind
// `valid`.  From there on the two are one text: gain with the reference's double-multiply-and-truncate, the positive peak of the values at
// even / odd positions (the level loop walks the buffer as L/R pairs in mono too, :1034-1051), the de-interleave.  The wave's two peaks
// come back uniform.
template <bool FULL>
TL_FN void tl_ingest_wave(const int16_t *TL_RESTRICT src, int16_t *TL_RESTRICT dst, int nch, double g, int valid, int wave, int &peak0, int &peak1)
{
    const int missing = TL_INGEST_FRAMES - valid;
    const int q = missing >= 1 && missing <= TL_INGEST_STRETCH_MAX ? valid / missing : 0;        // 0: no stretch, the source frame is the output frame
    const int nquads = nch == 2 ? 288 : 144;                    // 16 bytes = 4 L/R pairs (8 mono samples) per step
    PV(int, pk0); PV(int, pk1);
    TL_LANES_BEGIN
        int p0 = 0, p1 = 0;
        for (int qd = wave * 64 + lane; qd < nquads; qd += 64 * TL_INGEST_WAVES) {
            uint32_t w4[4];
            if (FULL) TL_INGEST_LD16(w4, src, qd);
            else if (nch == 2) {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = 4 * qd + k, s = q ? tl_stretch_src(i, q) : i;
                    w4[k] = s < valid ? ((const uint32_t *)src)[s] : 0u;
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int i = 8 * qd + 2 * k, s0 = q ? tl_stretch_src(i, q) : i, s1 = q ? tl_stretch_src(i + 1, q) : i + 1;
                    const uint32_t lo = s0 < valid ? (uint16_t)src[s0] : 0u, hi = s1 < valid ? (uint16_t)src[s1] : 0u;
                    w4[k] = lo | (hi << 16);
                }
            }
            int16_t l[4], r[4];
#pragma unroll
            for (int k = 0; k < 4; k++) {
                int a = (int16_t)(w4[k] & 0xffff), b = (int16_t)(w4[k] >> 16);
                if (g != 1.0) { a = (int16_t)(int)((double)a * g); b = (int16_t)(int)((double)b * g); }
                l[k] = (int16_t)a; r[k] = (int16_t)b;
                p0 = a > p0 ? a : p0; p1 = b > p1 ? b : p1;
            }
            if (nch == 2) {
                TL_INGEST_ST8(dst, qd, (uint16_t)l[0] | ((uint32_t)(uint16_t)l[1] << 16), (uint16_t)l[2] | ((uint32_t)(uint16_t)l[3] << 16));
                TL_INGEST_ST8(dst + 1152, qd, (uint16_t)r[0] | ((uint32_t)(uint16_t)r[1] << 16), (uint16_t)r[2] | ((uint32_t)(uint16_t)r[3] << 16));
            } else {                                                 // mono: consecutive samples, channel 0 only
                TL_INGEST_ST16(dst, qd, (uint16_t)l[0] | ((uint32_t)(uint16_t)r[0] << 16), (uint16_t)l[1] | ((uint32_t)(uint16_t)r[1] << 16),
                               (uint16_t)l[2] | ((uint32_t)(uint16_t)r[2] << 16), (uint16_t)l[3] | ((uint32_t)(uint16_t)r[3] << 16));
            }
        }
        if (nch == 1) for (int qd = wave * 64 + lane; qd < 288; qd += 64 * TL_INGEST_WAVES) TL_INGEST_ST8(dst + 1152, qd, 0u, 0u);
        L(pk0) = p0; L(pk1) = p1;
    TL_LANES_END
    peak0 = TL_WAVE_MAX_I32(pk0); peak1 = TL_WAVE_MAX_I32(pk1);
}

// Duration of a frame in whole milliseconds as the reference computes it for its silence counter (:1053-1062): 24 at 48 kHz, 36 at 32 kHz,
// 48 at 24 kHz, 72 at 16 kHz, 26 at 44.1 kHz.  Rates by MPEG version and sampling_frequency index, common.c:118-144.
TL_FN uint32_t tl_frame_ms(int version, int fs_idx, int nch)
{
    const int32_t half = fs_idx == 0 ? 22050 : fs_idx == 1 ? 24000 : 16000;            // MPEG-2 LSF rates; MPEG-1 doubles them
    const unsigned long rate = (unsigned long)(version ? 2 * half : half), n = (unsigned long)nch;
    return (uint32_t)(1000ul * (1152ul * 2ul * n) / (2ul * n * rate));
}

// Underrun bookkeeping of one stream over the frames of a call, in order (:919-935): a short frame raises STATUS_UNDERRUN and is what
// notify_underrun counts; the reference aborts when no full read has arrived for 60 s of wall clock, which a caller whose ticks are the
// clock reads off `underrun_ms` -- a short frame adds the frame's duration, a full one sets it to 0.  valid [nframes][nstreams].
TL_FN void tl_underrun_stream(const int32_t *TL_RESTRICT valid, uint32_t *TL_RESTRICT underrun_ms, uint32_t *TL_RESTRICT underruns, uint32_t frame_ms,
                              int s, int nstreams, int nframes)
{
    uint32_t ms = underrun_ms[s], n = underruns[s];
    for (int f = 0; f < nframes; f++) {
        const bool is_short = valid[(size_t)f * (size_t)nstreams + (size_t)s] < TL_INGEST_FRAMES;
        ms = is_short ? ms + frame_ms : 0u;
        n += is_short ? 1u : 0u;
    }
    underrun_ms[s] = ms; underruns[s] = n;
}

// Silence accounting of one stream over the frames of a call, in order (:1053-1079): a frame whose peaks are both 0 adds its duration to
// the stream's counter, any other frame resets it; the decision (`measured_silence_ms > 1000 * silence_timeout`) stays with the caller.
// peaks [nframes][nstreams][2].
TL_FN void tl_silence_stream(const int16_t *TL_RESTRICT peaks, uint32_t *TL_RESTRICT silence_ms, uint32_t frame_ms, int s, int nstreams, int nframes)
{
    uint32_t ms = silence_ms[s];
    for (int f = 0; f < nframes; f++) {
        const size_t slot = (size_t)f * (size_t)nstreams + (size_t)s;
        const int pl = peaks[slot * 2], pr = peaks[slot * 2 + 1];
        ms = (pl > pr ? pl : pr) == 0 ? ms + frame_ms : 0u;
    }
    silence_ms[s] = ms;
}
