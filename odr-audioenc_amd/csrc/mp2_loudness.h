// mp2_loudness.h -- the device loudness meter's body (include/toolame_batch.h, tlb_loudness_*): momentary, short-term and the gating
// histogram of programme loudness after ITU-R BS.1770-4 / EBU Tech 3341, of the planar PCM the encoder is given.  The reference measures
// peaks and silence only (--level, --silence), so the arithmetic is DEFINED here and in the committed table csrc/tl_loudness_tables.inc;
// every product and sum is its own rounded fp64 operation (-ffp-contract=off) in the order written:
//   x = (double)s * (1 / 32768);  two biquads in direct form I, t = ((b0 x) + (b1 x1)) + (b2 x2), y = (t - (a2 y2)) - (a1 y1), the
//   second on the first's y;  acc_c += y y;  every fs / 10 samples ms_c = acc_c / binlen, z = ms_0 (+ ms_1), z into a ring of 30;
//   momentary m = (((z[-3] + z[-2]) + z[-1]) + z[0]) * 0.25 from 4 bins on, short-term the ring summed oldest to newest / 30 from 30 on;
//   every m is a gating block: counted iff m > e_0, in bin #{k in 1..750: m >= e_k} of the stream's 751 counts.
// The recurrence is sequential, so the parallel axis is (stream, channel): ONE LANE each, a wave takes 32 consecutive streams
// (lane = 2 * local stream + channel) and walks the call's frames in order with the filter state, acc and the bin position in registers.
// tl_loudness_wave is written in the lane macros of mp2_wave.h so that tests/emu/mp2_loudness_emu.cpp runs the same text as lane loops.
//
// Staging.  A lane's samples lie 2304 bytes from its neighbour's, so the wave brings the PCM in through LDS, TL_LD_CHUNK = 64 samples of
// each of its 64 rows at a time: 64 rows x one 128-byte line = 512 pieces of 16 bytes, eight per lane, eight consecutive lanes on one line
// (global_load_dwordx4), requested one chunk ahead of use and kept in registers while the lanes work through the chunk before.
// LDS.  Rows lie TL_LD_PITCH = 72 int16 = 144 bytes = 36 dwords apart.  A lane reads its own row 16 bytes (eight samples) at a time, so the
// 64 lanes read one sample position of 64 rows with one ds_read_b128, which the LDS serves in four groups of sixteen lanes over 64 banks
// of 4 bytes.  Each group holds every lane number mod 16 once, and lane l starts at bank 36 l mod 64 = 4 (9 l mod 16): 9 is odd, so the
// sixteen lanes start at every multiple of four once and tile the 64 banks; 128 bytes (a pitch of 32 dwords) would put all of them on banks
// 0..3, and 132 or 136 bytes (the conflict-free pitches of 4- and 8-byte reads) are not 16-byte aligned.  The fill writes 16 bytes per lane,
// eight consecutive lanes one row's 128 contiguous bytes = 32 banks of ds_write_b128's 32.  Neither has been measured on the hardware.
// The close.  A frame is 1152 samples and the shortest bin 1600, so a frame closes at most one bin: the sample loop only takes ms_c
// and restarts acc -- testing for it once per 16-byte piece, not per sample, while the bin cannot close inside the piece: the lane is
// alone with its chain's latency, and eight samples in one basic block let neighbouring samples' stages overlap (profiles/tick_loudness.txt:
// 0.16 -> 0.045 ms per tick at 16 384 streams) -- and what follows from a closed bin -- one exchange of ms between the pair's lanes, the ring, the record, one histogram
// word -- happens once behind the frame, in the channel-0 lane, which owns all three: ordinary vector loads and stores, no atomics.
// Streams of different rates differ in binlen and coefficient row only.
//
// Device memory, allocated by tlb_loudness_enable alone (3456 bytes per stream, about 450 MB at 131 072 streams):
//   lane   double [TL_LD_LANE_WORDS][2 nstreams]   x1 x2 y1 y2 of stage 1, of stage 2, acc, the position in the bin (as an integer's bits)
//   ring   double [TL_LD_RING][nstreams]           z of bin k at row k mod 30
//   rec    TlLoudnessRecord [nstreams]             the record as it is reported
//   hist   uint32 [TL_LD_HIST_ROWS][nstreams]      751 counts and a row of padding: neighbouring streams' words lie together, here and in
//                                                  tl_loudness_programme
// Loudness range (tlb_lra_*).  Every short-term value st is also a RANGE BLOCK: counted iff st > e_0, in bin #{k in 1..750: st >= e_k} of a
// second histogram, by the counting instantiation of the wave's body (tl_lra_wave; tl_loudness_wave is the other and the text it always
// was).  tl_lra_range turns a stream's counts into its record: gate 0.01 * (S / N), nearest ranks over the gated bins.  Device memory,
// allocated by tlb_lra_enable alone (3008 bytes per stream):
//   hist_st uint32 [TL_LD_HIST_ROWS][nstreams]     laid out like hist; handed to the kernel beside TlLoudnessArgs (TlLraArgs), not inside it
#pragma once
#include <stdint.h>
#include "mp2_types.h"

#define TL_LD_FRAME 1152
#define TL_LD_STREAMS 32              // streams per wave
#define TL_LD_CHUNK 64                // samples of a row staged at a time: one 128-byte line
#define TL_LD_CHUNKS (TL_LD_FRAME / TL_LD_CHUNK)
#define TL_LD_PITCH 72                // int16 per row in LDS (see LDS above)
#define TL_LD_RING 30
#define TL_LD_BINS 751
#define TL_LD_HIST_ROWS 752
#define TL_LD_LANE_WORDS 10
#define TL_LD_RATES 6
#define TL_LD_TABLE_DOUBLES (TL_LD_RATES * 10 + 2 * TL_LD_BINS)      // taps [6][10], edges [751], centres [751]

// 48, 44.1, 32, 24, 22.05, 16 kHz -> row of the table, -1: no Layer II rate
static inline int tl_ld_rate_row(long rate)
{
    return rate == 48000 ? 0 : rate == 44100 ? 1 : rate == 32000 ? 2 : rate == 24000 ? 3 : rate == 22050 ? 4 : rate == 16000 ? 5 : -1;
}
#define tl_ld_row_of(version, fs_idx) ((version) == 1 ? ((fs_idx) == 1 ? 0 : (fs_idx) == 0 ? 1 : 2) : ((fs_idx) == 1 ? 3 : (fs_idx) == 0 ? 4 : 5))      /* of a TlConfig (a macro: host and device) */
#define tl_ld_binlen(row) ((row) == 0 ? 4800u : (row) == 1 ? 4410u : (row) == 2 ? 3200u : (row) == 3 ? 2400u : (row) == 4 ? 2205u : 1600u)

struct TlLoudnessRecord { uint32_t frames, bins, blocks, gated; double momentary, short_term, momentary_max, short_term_max; };      // tlb_loudness_record
struct TlLoudnessProgramme { double integrated, gate; uint32_t gated, reserved; };                                                  // tlb_loudness_programme_record
struct TlLoudnessArgs {
    const int16_t *pcm;               // [nframes][nstreams][2][1152], 16-byte aligned
    double *lane, *ring;
    TlLoudnessRecord *rec, *out;      // out [nstreams]: the call's report, may be NULL
    uint32_t *hist;
    const double *tables;             // TL_LD_TABLE_DOUBLES
    const TlConfig *configs;
    const int32_t *stream_cfg;
    int nstreams, nframes;
};

// Loudness range (tlb_lra_*): the meter's arguments as they are and the second histogram beside them, so that tl_loudness_kernel's
// argument block does not change
struct TlLraRecord { double low, high, gate; uint32_t blocks, gated; int32_t low_bin, high_bin; };                                  // tlb_lra_record
struct TlLraArgs {
    TlLoudnessArgs A;
    uint32_t *hist_st;                // [TL_LD_HIST_ROWS][nstreams] range blocks per 0.1 LU, laid out like hist
};

#ifdef TL_FN                          // behind mp2_wave.h only: the host translation units take the constants and records above and nothing else
struct alignas(16) TlLoudnessLds { int16_t x[64 * TL_LD_PITCH]; };   // 9216 bytes per wave

// one biquad step on the lane's registers q[0..3] = x1 x2 y1 y2 with k[0..4] = b0 b1 b2 a1 a2
#define TL_LD_BIQUAD(y, x, q, k) do { const double t_ = (((k)[0] * (x)) + ((k)[1] * (q)[0])) + ((k)[2] * (q)[1]); \
                                      (y) = (t_ - ((k)[4] * (q)[3])) - ((k)[3] * (q)[2]); \
                                      (q)[1] = (q)[0]; (q)[0] = (x); (q)[3] = (q)[2]; (q)[2] = (y); } while (0)

// number of k in 1..750 with m >= edges[k] (edges strictly increasing: tests/test_loudness_tables.py)
TL_FN int tl_ld_bin_of(const double *TL_RESTRICT edges, double m)
{
    int lo = 0, hi = TL_LD_BINS - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (m >= edges[mid]) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// The wave of streams [32 wv, 32 wv + 32) over the call's frames.  RANGE: every short-term value is also a range block of the loudness
// range (tlb_lra_*), counted in hist_st; without it hist_st is not looked at and the text is tl_loudness_wave's as it always was.
template <bool RANGE> TL_FN void tl_loudness_wave_t(const TlLoudnessArgs &A, uint32_t *hist_st, TlLoudnessLds &w, int wv)
{
    const int ns = A.nstreams, s0 = wv * TL_LD_STREAMS, total = A.nframes * TL_LD_CHUNKS;
    const size_t lanes = 2 * (size_t)ns;
    const double *edges = A.tables + TL_LD_RATES * 10;
    PA(double, q, 8); PA(double, k, 10); PA(double, g, 16);      // g: eight 16-byte pieces, each moved as two doubles (TL_LD2 / TL_ST2: one global_load_dwordx4, ds_write_b128)
    PV(double, acc); PV(double, ms); PV(double, ms_other);
    PV(uint32_t, pos); PV(uint32_t, binlen); PV(int, nch); PV(int, live); PV(int, closed);
    TL_LANES_BEGIN
        const int s = s0 + (lane >> 1), c = lane & 1;
        L(live) = 0; L(nch) = 0; L(binlen) = 1600u; L(pos) = 0u; L(acc) = 0.0; L(ms) = 0.0; L(closed) = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) L(q)[i] = 0.0;
#pragma unroll
        for (int i = 0; i < 10; i++) L(k)[i] = 0.0;
        if (s < ns) {
            const TlConfig *C = &A.configs[A.stream_cfg[s]];
            const int row = tl_ld_row_of(C->version, C->fs_idx);
            L(nch) = C->nch; L(binlen) = tl_ld_binlen(row); L(live) = c < C->nch;
            if (L(live)) {
                const size_t at = 2 * (size_t)s + (size_t)c;
#pragma unroll
                for (int i = 0; i < 8; i++) L(q)[i] = A.lane[(size_t)i * lanes + at];
#pragma unroll
                for (int i = 0; i < 10; i++) L(k)[i] = A.tables[row * 10 + i];
                L(acc) = A.lane[8 * lanes + at];
                L(pos) = (uint32_t)tl_d2u(A.lane[9 * lanes + at]);
            }
        }
    TL_LANES_END
    // piece 64 i + lane of a chunk: 16 bytes of row 8 i + lane / 8; a row past the batch's last stream is not read
#define TL_LD_FETCH(ch) do { const int f_ = (ch) / TL_LD_CHUNKS, at_ = ((ch) - f_ * TL_LD_CHUNKS) * TL_LD_CHUNK + (lane & 7) * 8; \
        _Pragma("unroll") for (int i = 0; i < 8; i++) { \
            const int r_ = 8 * i + (lane >> 3), s_ = s0 + (r_ >> 1); \
            if (s_ < ns) TL_LD2((const double *)&A.pcm[(((size_t)f_ * (size_t)ns + (size_t)s_) * 2 + (size_t)(r_ & 1)) * TL_LD_FRAME + (size_t)at_], L(g)[2 * i], L(g)[2 * i + 1]); \
        } } while (0)
    // sample j of the piece in u: both stages and the square
#define TL_LD_SAMPLE(j) do { const double x_ = (double)(int16_t)(u[(j) >> 2] >> (16 * ((j) & 3))) * (1.0 / 32768.0); \
        double y1_, y2_; \
        TL_LD_BIQUAD(y1_, x_, L(q), L(k)); \
        TL_LD_BIQUAD(y2_, y1_, L(q) + 4, L(k) + 5); \
        L(acc) = L(acc) + (y2_ * y2_); } while (0)
    TL_LANES_BEGIN
#pragma unroll
        for (int i = 0; i < 16; i++) L(g)[i] = 0.0;
        TL_LD_FETCH(0);
    TL_LANES_END
    for (int ch = 0; ch < total; ch++) {
        TL_LANES_BEGIN
#pragma unroll
            for (int i = 0; i < 8; i++) TL_ST2((double *)&w.x[(8 * i + (lane >> 3)) * TL_LD_PITCH + (lane & 7) * 8], L(g)[2 * i], L(g)[2 * i + 1]);
        TL_LANES_END
        TL_LANES_BEGIN
            if (ch + 1 < total) TL_LD_FETCH(ch + 1);
            if (L(live)) {
#pragma nounroll
                for (int v = 0; v < 8; v++) {
                    double d0, d1;
                    TL_LD2((const double *)&w.x[lane * TL_LD_PITCH + v * 8], d0, d1);
                    const uint64_t u[2] = {tl_d2u(d0), tl_d2u(d1)};      // samples 8 v .. 8 v + 3, 8 v + 4 .. 8 v + 7
                    // eight samples in one basic block while the bin cannot close among them (all but one piece in 200 to 600): the
                    // two stages of neighbouring samples overlap, where a test behind every sample would keep them apart
                    if (L(binlen) - L(pos) > 8u) {
#pragma unroll
                        for (int j = 0; j < 8; j++) TL_LD_SAMPLE(j);
                        L(pos) += 8u;
                    } else {
#pragma unroll
                        for (int j = 0; j < 8; j++) {
                            TL_LD_SAMPLE(j);
                            if (++L(pos) == L(binlen)) { L(ms) = L(acc) / (double)L(binlen); L(acc) = 0.0; L(pos) = 0u; L(closed) = 1; }
                        }
                    }
                }
            }
        TL_LANES_END
        if ((ch + 1) % TL_LD_CHUNKS) continue;
        // behind a frame: the bin it closed, if any
        TL_SWAP1_F64(ms_other, , ms, );
        TL_LANES_BEGIN
            const int s = s0 + (lane >> 1);
            if (L(live) && !(lane & 1) && L(closed)) {
                TlLoudnessRecord *R = &A.rec[s];
                const double z = L(nch) == 2 ? L(ms) + L(ms_other) : L(ms);
                const uint32_t bins = R->bins + 1u;                  // z is bin number bins - 1
                double *ring = A.ring + s;
                ring[(size_t)((bins - 1u) % TL_LD_RING) * (size_t)ns] = z;
                R->bins = bins;
                if (bins >= 4u) {
                    const double m = (((ring[(size_t)((bins - 4u) % TL_LD_RING) * (size_t)ns] + ring[(size_t)((bins - 3u) % TL_LD_RING) * (size_t)ns]) +
                                       ring[(size_t)((bins - 2u) % TL_LD_RING) * (size_t)ns]) + z) * 0.25;
                    R->blocks = R->blocks + 1u;
                    R->momentary = m;
                    if (m > R->momentary_max) R->momentary_max = m;
                    if (m > edges[0]) {
                        uint32_t *h = A.hist + (size_t)tl_ld_bin_of(edges, m) * (size_t)ns + (size_t)s;
                        *h = *h + 1u;
                        R->gated = R->gated + 1u;
                    }
                }
                if (bins >= (uint32_t)TL_LD_RING) {
                    double sum = ring[(size_t)(bins % TL_LD_RING) * (size_t)ns];                 // the oldest: bin number bins - 30
#pragma nounroll
                    for (uint32_t b = bins + 1u; b < bins + (uint32_t)TL_LD_RING - 1u; b++) sum = sum + ring[(size_t)(b % TL_LD_RING) * (size_t)ns];
                    sum = sum + z;
                    const double st = sum / 30.0;
                    R->short_term = st;
                    if (st > R->short_term_max) R->short_term_max = st;
                    if (RANGE && st > edges[0]) {
                        uint32_t *h = hist_st + (size_t)tl_ld_bin_of(edges, st) * (size_t)ns + (size_t)s;
                        *h = *h + 1u;
                    }
                }
            }
            L(closed) = 0;
        TL_LANES_END
    }
#undef TL_LD_FETCH
#undef TL_LD_SAMPLE
    TL_LANES_BEGIN
        const int s = s0 + (lane >> 1);
        if (L(live)) {
            const size_t at = 2 * (size_t)s + (size_t)(lane & 1);
#pragma unroll
            for (int i = 0; i < 8; i++) A.lane[(size_t)i * lanes + at] = L(q)[i];
            A.lane[8 * lanes + at] = L(acc);
            A.lane[9 * lanes + at] = tl_u2d((uint64_t)L(pos));
            if (!(lane & 1)) {
                A.rec[s].frames = A.rec[s].frames + (uint32_t)A.nframes;
                if (A.out) A.out[s] = A.rec[s];
            }
        }
    TL_LANES_END
}
TL_FN void tl_loudness_wave(const TlLoudnessArgs &A, TlLoudnessLds &w, int wv) { tl_loudness_wave_t<false>(A, nullptr, w, wv); }
TL_FN void tl_lra_wave(const TlLraArgs &X, TlLoudnessLds &w, int wv) { tl_loudness_wave_t<true>(X.A, X.hist_st, w, wv); }

// Programme loudness of stream s from its counts: the two ascending passes.  centres: the table's third part.
TL_FN void tl_loudness_programme(const uint32_t *TL_RESTRICT hist, const double *TL_RESTRICT centres, TlLoudnessProgramme *TL_RESTRICT out, int s, int nstreams)
{
    uint32_t N = 0u;
    double S = 0.0;
#pragma nounroll
    for (int j = 0; j < TL_LD_BINS; j++) {
        const uint32_t n = hist[(size_t)j * (size_t)nstreams + (size_t)s];
        N += n; S = S + ((double)n * centres[j]);
    }
    TlLoudnessProgramme P = {0.0, 0.0, 0u, 0u};
    if (N) {
        P.gate = 0.1 * (S / (double)N);
        uint32_t N2 = 0u;
        double S2 = 0.0;
#pragma nounroll
        for (int j = 0; j < TL_LD_BINS; j++) {
            if (!(centres[j] >= P.gate)) continue;
            const uint32_t n = hist[(size_t)j * (size_t)nstreams + (size_t)s];
            N2 += n; S2 = S2 + ((double)n * centres[j]);
        }
        P.integrated = S2 / (double)N2;
        P.gated = N2;
    }
    out[s] = P;
}

// Loudness range of stream s from its range-block counts (include/toolame_batch.h, "Loudness range"): the gate 20 LU below the mean of
// the counted blocks, then the nearest ranks of the 10th and the 95th percentile among the bins at or above it, in one ascending walk.
TL_FN void tl_lra_range(const uint32_t *TL_RESTRICT hist, const double *TL_RESTRICT centres, TlLraRecord *TL_RESTRICT out, int s, int nstreams)
{
    uint32_t N = 0u;
    double S = 0.0;
#pragma nounroll
    for (int j = 0; j < TL_LD_BINS; j++) {
        const uint32_t n = hist[(size_t)j * (size_t)nstreams + (size_t)s];
        N += n; S = S + ((double)n * centres[j]);
    }
    TlLraRecord P = {0.0, 0.0, 0.0, 0u, 0u, 0, 0};
    if (N) {
        P.gate = 0.01 * (S / (double)N);
        P.blocks = N;
        uint32_t N2 = 0u;
#pragma nounroll
        for (int j = 0; j < TL_LD_BINS; j++)
            if (centres[j] >= P.gate) N2 += hist[(size_t)j * (size_t)nstreams + (size_t)s];
        P.gated = N2;
        const uint64_t r_lo = ((uint64_t)N2 + 4u) / 10u, r_hi = (19u * ((uint64_t)N2 - 1u) + 10u) / 20u;
        uint64_t cum = 0u;
        int lo = -1, hi = -1;
#pragma nounroll
        for (int j = 0; j < TL_LD_BINS && hi < 0; j++) {
            if (!(centres[j] >= P.gate)) continue;
            cum += hist[(size_t)j * (size_t)nstreams + (size_t)s];
            if (lo < 0 && cum > r_lo) lo = j;
            if (cum > r_hi) hi = j;
        }
        P.low_bin = lo; P.high_bin = hi;
        P.low = centres[lo]; P.high = centres[hi];
    }
    out[s] = P;
}
#endif
