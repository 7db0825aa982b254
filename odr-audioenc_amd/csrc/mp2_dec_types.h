// mp2_dec_types.h -- data layout of the frame check / decode path (mp2_unpack.h, mp2_synth.h, toolame_dec.hip, tlb_decode.cpp), shared
// by the host runtime and the kernels.  The encode path includes none of it.
#pragma once
#include <stdint.h>
#include "mp2_types.h"

// status word of a frame: independent flags (the TLB_DEC_* values of include/toolame_batch.h; tlb_decode.cpp asserts that they agree)
#define TL_DEC_EMPTY            0x01u    // the slot holds no frame (length 0)
#define TL_DEC_BAD_SYNC         0x02u    // the first twelve bits are not the sync word
#define TL_DEC_HEADER_MISMATCH  0x04u    // a header field is not what the stream's configuration says, or the slot is longer than the frame
#define TL_DEC_BAD_CRC16        0x08u    // bytes 4..5 are not the CRC-16 of the protected bits
#define TL_DEC_BAD_SCFCRC       0x10u    // the ScF-CRC bytes the frame before carries for this frame do not fit its scalefactors
#define TL_DEC_SCFCRC_UNCHECKED 0x20u    // there is no frame before (first after a reset), or it is too short to hold them
#define TL_DEC_BAD_ALLOC        0x40u    // an allocation code the stream's table has no quantiser for
#define TL_DEC_OVERRUN          0x80u    // the fields need more bits than the frame has left beside its PAD, or the slot is shorter than the frame
#define TL_DEC_BAD_MASK (TL_DEC_BAD_SYNC | TL_DEC_HEADER_MISMATCH | TL_DEC_BAD_CRC16 | TL_DEC_BAD_SCFCRC | TL_DEC_BAD_ALLOC | TL_DEC_OVERRUN)

struct TlFrameReport {
    uint32_t status;
    uint16_t crc_stored, crc_computed;
    uint8_t mode, mode_ext;          // as the frame's header says
    uint16_t audio_bits;             // header + CRC + allocation + scfsi + scalefactors + samples
};
// the parsed fields in the layout of the encoder's taps (TlTaps); cells that the frame does not transmit are 0
struct TlFrameFields {
    uint8_t bit_alloc[2][32], scfsi[2][32], scalar[2][3][32];
    uint16_t subband[2][3][12][32];
};
static_assert(sizeof(TlFrameReport) == 12 && sizeof(TlFrameFields) == 4928, "C-ABI records (include/toolame_batch.h)");

// What one launch leaves per stream for the next one's first frame: where the ScF-CRC of that frame is (the tail of the last non-empty
// slot) and what the synthesis history is made of (the last slot, whose bytes are kept in TlDecLaunch::prev).
struct TlDecStream {
    int32_t have_tail;               // tail[] holds the ScF-CRC bytes of the last frame seen
    uint8_t tail[4];
    int32_t prev_len;                // bytes of the last slot in prev[] (0: empty or none yet)
    uint32_t prev_status;            // its status word
};

#define TL_SYNTH_HIST 15             // sample vectors before a frame that its first output vector still depends on (a 512-tap window: 16 vectors)
// matrixing N[i][k] = cos((16 + i)(2k + 1) pi / 64) as n[k][i], then the synthesis window D[i] = 32 C[i] (ISO/IEC 11172-3 Annex 3-A.2), then C and D of the
// requantisation per quantiser class (table 3-B.4)
struct TlSynthTables {
    double n[32][64];
    double d[512];
    double rq_c[18], rq_d[18];
};

struct TlDecLaunch {
    const TlTables *tables;
    const TlConfig *configs;
    const int32_t *stream_cfg;        // [nstreams] or NULL: configuration 0
    const TlSynthTables *synth;
    const uint8_t *frames;            // [nframes][nstreams][out_stride]
    const int32_t *len;               // [nframes][nstreams] or NULL: every slot holds a frame of the length its header and configuration say
    TlFrameReport *report;            // [nframes][nstreams]
    TlFrameFields *fields;            // [nframes][nstreams] or NULL
    int16_t *pcm;                     // [nframes][nstreams][2][1152] or NULL
    TlDecStream *state;               // [nstreams]
    uint8_t *prev;                    // [nstreams][out_stride]
    unsigned long long *bad;          // frames with a TL_DEC_BAD_MASK flag so far
    int32_t nstreams, nframes, out_stride, pad_;
};

// One launch of the Layer II feed path (mp2_feed.h, toolame_feed.hip, tlb_feed.cpp): frames somebody else encoded, decoded into the
// ingest's input.  A fed stream has a configuration record of its OWN here (its bitrate need not be the encoder's), and a history of
// its own in the layout of the decoder's (TlDecStream: prev_len and prev_status are used, the ScF-CRC tail is not).
struct TlFeedLaunch {
    const TlTables *tables;
    const TlConfig *configs;          // the feeds' records
    const int32_t *feed_cfg;          // [nstreams] index into configs; -1: the stream has no feed
    const TlSynthTables *synth;
    const uint8_t *frames;            // [nframes][nstreams][stride]
    const int32_t *len;               // [nframes][nstreams]; 0: an empty slot
    TlFrameReport *report;            // [nframes][nstreams]
    int16_t *pcm;                     // [nframes][nstreams][2304] interleaved: the ingest's input
    TlDecStream *state;               // [nstreams]
    uint8_t *prev;                    // [nstreams][prev_stride] the last slot of the launch before
    int32_t nstreams, nframes, stride, prev_stride;       // both multiples of 4, each at least the longest frame of any feed of the batch
};
// the slot a feed of record c needs: its longest frame (with the padding slot where the rate has one), rounded up to 4
static inline int tl_feed_slot_bytes(const TlConfig &c) { return (c.frame_bytes + (c.pad_frac != 0 ? 1 : 0) + 3) & ~3; }
