/* toolame_batch.h -- C-ABI of the MI355X-native batched DAB MP2 (MPEG-1/2 Layer II) encoder.
 *
 * Drop-in boundary.  The library exports two groups of symbols:
 *
 *  (1) The reference's own nine-function ABI, unchanged, so src/odr-audioenc.cpp:89-92,686-735,
 *      1135-1163 links against this library exactly as it links against libtoolame-dab.a.
 *      Declarations: /root/reference/libtoolame-dab/toolame.h:13-48, export list
 *      /root/reference/libtoolame-dab.sym.  They drive stream 0 of a private one-stream batch and
 *      reproduce toolame_encode_frame()'s bursty 4096-byte output cadence (bitstream.c:46-71).
 *
 *  (2) A handle-based batched API (tlb_*) -- what the reference cannot offer because all of its
 *      state is process-global (toolame.c:24-26,89-118): N independent streams, mixed
 *      configurations, whole-frame output, device-resident buffers and an explicit HIP stream.
 *
 * All pointers are plain C pointers; "d_" parameters are HIP device pointers.  No torch types.
 * Every function returns 0 on success and non-zero on error unless stated otherwise
 * (toolame.h:9-10).  The library needs a gfx950 GPU: there is no CPU fallback, tlb_create()
 * fails with TLB_ERR_NO_DEVICE when none is usable.
 */
#ifndef TOOLAME_BATCH_H
#define TOOLAME_BATCH_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---------------------------------------------------------------------------------------------
 * (1) legacy ABI -- replaces libtoolame-dab/toolame.h:13-48 one for one
 * ------------------------------------------------------------------------------------------ */
int toolame_init(void);                                     /* toolame.c:120 */
int toolame_finish(unsigned char *output_buffer, size_t output_buffer_size);   /* toolame.c:155 -> bytes written */
int toolame_enable_byteswap(void);                          /* toolame.c:168 */
int toolame_set_channel_mode(const char mode);              /* toolame.c:174  's','d','j','m' */
int toolame_set_psy_model(int new_model);                   /* toolame.c:202  0..3 */
int toolame_set_bitrate(int brate);                         /* toolame.c:212  kbps */
int toolame_set_samplerate(long sample_rate);               /* toolame.c:239  Hz */
int toolame_set_pad(int pad_len);                           /* toolame.c:250 */
int toolame_encode_frame(short buffer[2][1152], unsigned char *xpad_data, size_t xpad_len,
                         unsigned char *output_buffer, size_t output_buffer_size);   /* toolame.c:267 -> bytes written */

/* ---------------------------------------------------------------------------------------------
 * (2) batched API
 * ------------------------------------------------------------------------------------------ */
#define TLB_MAX_XPAD 256           /* X-PAD + F-PAD bytes per frame: every padlen the caller accepts, 0..255 (src/odr-audioenc.cpp:566) */
#define TLB_SAMPLES_PER_FRAME 1152

enum {
    TLB_OK = 0,
    TLB_ERR_SAMPLERATE = 1,        /* SmpFrqIndex, common.c:118-144; the egress calls: a rate whose frames are no whole number of 24-ms units */
    TLB_ERR_MODE = 2,              /* toolame.c:195-197 */
    TLB_ERR_PSY = 3,               /* toolame.c:204-207 */
    TLB_ERR_BITRATE = 4,           /* common.c:95-116 (the reference exit(-1)s; we return an error) */
    TLB_ERR_PAD = 5,               /* toolame.c:252-255 */
    TLB_ERR_NO_DEVICE = 16,
    TLB_ERR_HIP = 17,
    TLB_ERR_ARG = 18,
    TLB_ERR_LATE = 19,             /* node level, TICK plane with a deadline set: a shard missed it (tlb_node_set_deadline_ms) */
};

/* The six knobs odr-audioenc sets (src/odr-audioenc.cpp:687-722), per stream. */
typedef struct {
    long samplerate;               /* 48000, 32000, 24000, 16000, 44100, 22050 */
    char mode;                     /* 's' stereo, 'j' joint stereo, 'd' dual channel, 'm' mono */
    int bitrate;                   /* kbps; 0 = the reference default, bitrate[version][10] (toolame.c:217-218): 192 (MPEG-1) / 96 (LSF) */
    int psy_model;                 /* 0, 1, 2, 3 (toolame.c:202-210); 4 = psycho_4.c, an extension of this API only: the
                                      reference implements it (toolame.c:384-391) but its setter refuses it */
    int pad_len;                   /* toolame_set_pad(): upper bound of xpad_len, 0..TLB_MAX_XPAD; must leave room for header, CRC and
                                      bit allocation in the frame (else TLB_ERR_PAD) */
} tlb_stream_config;

typedef struct tlb_batch tlb_batch;

int tlb_device_count(void);
/* Create `nstreams` encoders on HIP device `device`.  On failure returns NULL and stores a TLB_ERR_*
 * code in *err (if err != NULL). */
tlb_batch *tlb_create(int device, int nstreams, const tlb_stream_config *cfgs, int *err);
void tlb_destroy(tlb_batch *b);
int tlb_reset(tlb_batch *b);                       /* every stream back to the state right after tlb_create(); also the way out after a launch or a
                                                      reconfiguration failed half way (TLB_ERR_HIP from an encode call: the batch refuses work until reset).
                                                      It re-derives the device's stream tables, kernel lists and mono pairing from the host's first; if THAT
                                                      fails it returns the code and the batch stays refused (tlb_destroy is then the way out) */

/* Life cycle of ONE stream inside a live batch.  The reference's unit of restart is the stream -- toolame_init() zeroes one encoder
 * (toolame.c:120-153), toolame_finish() ends one (:155-166), the six setters reconfigure one (toolame.h:13-48), and odr-audioenc
 * restarts a failed input without touching anything else (src/odr-audioenc.cpp:875-902).  With thousands of streams in one batch the
 * same three operations exist per stream.  Each waits for the launches already queued on the batch, then acts; none changes a byte
 * any OTHER stream produces.  After any of them the stream is as right after tlb_create() -- the bytes of a reference process started
 * afresh, not those of an in-process toolame_init() --: its next input frame is its frame 0
 * (history of zeros, no pending frame: the output slot of the call that analyses it is empty, length 0 in the _len variants).
 *   tlb_stream_reset        = a freshly started reference PROCESS for that stream: drops the pending frame, zeroes filterbank and
 *                             model history.  (The reference's own toolame_init(), toolame.c:120-153, called a second time inside one
 *                             process, keeps the file-scope statics of psycho_1/2 -- savebuf, r, phi_sav, lthr, init -- and the
 *                             filterbank FIFO: a re-initialised reference encoder remembers its past, this one does not.)
 *   tlb_stream_finish       = toolame_finish(): copies the pending frame (the bytes still inside the encoder) to out, returns their
 *                             number (0: none yet; a too small buffer gets a truncated copy like the reference's); < 0: -TLB_ERR_*.
 *   tlb_stream_reconfigure  = the setters + toolame_init(): a new sample rate / mode / bitrate / psy model / PAD length.  The frames
 *                             of the new configuration must fit tlb_out_stride() and its units per frame tlb_egress_max_units_per_frame()
 *                             as the batch was created with (else TLB_ERR_ARG / TLB_ERR_SAMPLERATE, nothing changed); illegal settings
 *                             return the setter's error code. */
int tlb_stream_reset(tlb_batch *b, int stream);
int tlb_stream_finish(tlb_batch *b, int stream, uint8_t *out, size_t out_size);
int tlb_stream_reconfigure(tlb_batch *b, int stream, const tlb_stream_config *cfg);

int tlb_nstreams(const tlb_batch *b);
int tlb_frame_bytes(const tlb_batch *b, int stream);   /* 144000*kbps/fs: 384 @128k/48k, 576 @192k/48k ...; at 44.1 / 22.05 kHz the frames
                                                          WITHOUT a padding slot (417 @128k/44.1k) -- some frames are one byte longer,
                                                          see the _len entry points */
int tlb_out_stride(const tlb_batch *b);                /* longest frame over the batch, rounded up to a multiple of 4 */
long tlb_frames_encoded(const tlb_batch *b);           /* per stream */

/* Encode `nframes` frames of every stream, buffers resident in HBM.
 *   d_pcm      int16  [nframes][nstreams][2][1152]   planar like `short buffer[2][1152]`; mono reads [0] only
 *   d_xpad     uint8  [nframes][nstreams][TLB_MAX_XPAD] or NULL: the xpad_len bytes in transmission order
 *              (X-PAD bytes, then the two F-PAD bytes; toolame.c:515-551)
 *   d_xpad_len int32  [nframes][nstreams] or NULL; each 0 or 2..pad_len (any other value: the frame carries no PAD)
 *   d_out      uint8  [nframes][nstreams][tlb_out_stride()]
 * Frame n of a stream is final only once frame n+1 has been analysed (its ScF-CRC is stored in frame
 * n, toolame.c:527-542), so output slot f of this call holds the frame that was pending before input
 * frame f: slot 0 = the last frame of the previous call (undefined on the very first call), slot f =
 * input frame f-1.  tlb_flush_*() hands out the final pending frame.
 * The launch is asynchronous on `hip_stream` (a hipStream_t, NULL = default stream).  Launches of ONE batch must be ordered
 * on one stream (they share the streams' state and the batch's scratch buffers); at most 2^30 (stream, frame) pairs per call. */
int tlb_encode_device(tlb_batch *b, const int16_t *d_pcm, int nframes, const uint8_t *d_xpad,
                      const int32_t *d_xpad_len, uint8_t *d_out, void *hip_stream);
/* 44.1 and 22.05 kHz (libtoolame-dab encodes them; DAB itself does not use them, src/odr-audioenc.cpp:560-563): a frame is
 * tlb_frame_bytes() or one byte more (padding slot, availbits.c:49-62, header bit 9).  The _len variants also report the length
 * of the frame in every output slot (0: none): d_out_len int32 [nframes][nstreams] / out_len [nstreams] for the flush. */
int tlb_encode_device_len(tlb_batch *b, const int16_t *d_pcm, int nframes, const uint8_t *d_xpad, const int32_t *d_xpad_len,
                          uint8_t *d_out, int32_t *d_out_len, void *hip_stream);
int tlb_encode_host_len(tlb_batch *b, const int16_t *pcm, int nframes, const uint8_t *xpad, const int32_t *xpad_len,
                        uint8_t *out, int32_t *out_len, void *taps);
int tlb_flush_host_len(tlb_batch *b, uint8_t *out, int32_t *out_len);
int tlb_flush_device_len(tlb_batch *b, uint8_t *d_out, int32_t *d_out_len, void *hip_stream);
/* Same with host buffers (synchronous; copies over PCIe).  `taps`, if not NULL, receives
 * [nframes][nstreams] TlTaps records (csrc/mp2_types.h) for stage-level parity tests. */
int tlb_encode_host(tlb_batch *b, const int16_t *pcm, int nframes, const uint8_t *xpad, const int32_t *xpad_len,
                    uint8_t *out, void *taps);
/* Pinned (page-locked) host memory for the host-buffer entry points: copies from/to it run at PCIe link rate and
 * tlb_encode_host() queues copy-in, launch and copy-out without an intermediate synchronisation.  Pageable memory works
 * too, only slower.  The batch keeps its device staging buffers between calls (no allocation per call after the first). */
void *tlb_host_alloc(size_t bytes);
void tlb_host_free(void *p);
/* Copy every stream's pending (last) frame to out[nstreams][tlb_out_stride()] (host memory).
 * Streams that have not encoded any frame yet get zero bytes.  Does not change state. */
int tlb_flush_host(tlb_batch *b, uint8_t *out);
int tlb_flush_device(tlb_batch *b, uint8_t *d_out, void *hip_stream);

/* Caller-side per-frame glue folded into the batch: what AudioEnc::run() does between the input
 * queue and toolame_encode_frame() -- linear gain with the reference's double-multiply-and-truncate and the positive
 * peak level per channel (src/odr-audioenc.cpp:1030-1051), de-interleaving into `short[2][1152]` (:1139-1152).
 *   d_interleaved int16 [nframes][nstreams][2304]: s16le L R L R ... (mono streams: 1152 samples, rest ignored)
 *   d_pcm         int16 [nframes][nstreams][2][1152]  -- exactly what tlb_encode_device() takes
 *   d_peaks       int16 [nframes][nstreams][2]  (max(0, samples) of the "left"/"right" slots; the caller's silence
 *                 detection is `max(peaks) == 0`, odr-audioenc.cpp:1064)
 * tlb_set_gain_db(stream = -1) sets every stream; gain 0 dB leaves samples untouched like the reference. */
int tlb_set_gain_db(tlb_batch *b, int stream, double gain_db);
int tlb_ingest_device(tlb_batch *b, const int16_t *d_interleaved, int nframes, int16_t *d_pcm, int16_t *d_peaks, void *hip_stream);
int tlb_ingest_host(tlb_batch *b, const int16_t *interleaved, int nframes, int16_t *pcm, int16_t *peaks);
/* Ingest with SHORT READS: the drift compensation of the caller's loop (expand_missing_samples, src/odr-audioenc.cpp:335-373, called at
 * :910-917) ahead of the steps above, which then see the stretched frame.
 *   d_valid  int32 [nframes][nstreams]: whole sample frames the slot delivers (a sample frame is one L/R pair, or one sample of a
 *            one-channel stream).  Above 1152 counts as 1152, below 0 as 0.  NULL: tlb_ingest_device exactly.
 * ZERO TAIL.  The reference's queue zero-fills what it could not deliver (src/SampleQueue.h:217-276), so whatever the caller's buffer
 * holds behind `valid` is never read as samples: the frames behind the valid ones are zeros.  With missing = 1152 - valid:
 *   missing == 0       the frame passes unchanged (the function is not called, :913-915).
 *   missing >= 116     the valid frames followed by zeros (:351-356; the test is `missing * bytes_per_sample > buf.size() / 10` in
 *                      integer arithmetic, the same 116 for one and two channels; 115 is still stretched).
 *   1 .. 115           output frame i is source frame src(i) of the zero-tailed buffer, with q = valid / missing (integer division):
 *                      src(0) = 0, src(i) = i - (i - 1) / q for i >= 1 -- the closed form of the loop at :361-371, which does not
 *                      advance its source index after an i that is a positive multiple of q.
 * Two consequences, both the reference's and both reproduced: with missing == 1 the last output frame is source frame 1151, a zero of
 * the tail (:361-371 with q = 1151); with larger counts up to 22 valid frames at the end are never used (missing == 105: q = 9). */
int tlb_ingest_device_valid(tlb_batch *b, const int16_t *d_interleaved, const int32_t *d_valid, int nframes, int16_t *d_pcm, int16_t *d_peaks,
                            void *hip_stream);
int tlb_ingest_host_valid(tlb_batch *b, const int16_t *interleaved, const int32_t *valid, int nframes, int16_t *pcm, int16_t *peaks);
/* The underrun bookkeeping that goes with it (src/odr-audioenc.cpp:919-935), per stream over the frames of the call in order, both arrays
 * uint32 [nstreams] and read-modify-write like d_silence_ms:
 *   d_underrun_ms  a short frame (valid < 1152) adds the frame's duration in whole milliseconds (as the silence counter), a full frame
 *                  sets it to 0.  The reference aborts when it exceeds 60 s (:925-931); that decision stays with the caller.
 *   d_underruns    short frames so far: what the reference reports through notify_underrun (:920-923). */
int tlb_underrun_device(tlb_batch *b, const int32_t *d_valid, int nframes, uint32_t *d_underrun_ms, uint32_t *d_underruns, void *hip_stream);
int tlb_underrun_host(tlb_batch *b, const int32_t *valid, int nframes, uint32_t *underrun_ms, uint32_t *underruns);
/* The caller's silence accounting (src/odr-audioenc.cpp:1053-1079): per stream, a frame with both peaks 0 adds its duration
 * in whole milliseconds (24 at 48 kHz, 36 at 32 kHz, 48 at 24 kHz) to d_silence_ms[stream], any other frame resets it to 0.
 * The decision itself (`measured_silence_ms > 1000 * silence_timeout` -> stop the stream) stays with the caller. */
int tlb_silence_device(tlb_batch *b, const int16_t *d_peaks, int nframes, uint32_t *d_silence_ms, void *hip_stream);
int tlb_silence_host(tlb_batch *b, const int16_t *peaks, int nframes, uint32_t *silence_ms);

/* Egress framing of the step after the path.
 *
 * UNITS.  ODR-AudioEnc does not send MP2 frames: it cuts the encoder's byte stream into pieces of 3 * bitrate bytes (24 ms)
 * and calls send_frame() once per piece (src/odr-audioenc.cpp:1211-1219, "ODR-DabMux expects frames of length 3*bitrate").
 * At 48 kHz a frame is one unit; an MPEG-2 LSF frame is two (24 kHz) or three (16 kHz).  Every egress buffer below is laid
 * out by SLOT v = frame * tlb_egress_max_units_per_frame() + unit: [nframes * max_upf][nstreams][...]; a stream with fewer
 * units per frame than the batch's maximum leaves its surplus slots absent (length / datasize 0).  For an all-48-kHz batch
 * max_upf is 1 and a slot is a frame.  32 kHz (1.5 units per frame) is not a DAB rate (odr-audioenc.cpp:560-563); a batch
 * that contains it has max_upf 0 and the egress calls return TLB_ERR_SAMPLERATE.
 * TIMING AND LEVELS differ from the reference's send loop, by the reference's burst behaviour: toolame_encode_frame() returns bytes only on
 * the calls on which its 4096-byte bit buffer fills, about one call in ten (bitstream.c:46-71), and odr-audioenc.cpp:1208-1225 then sends
 * every unit but one of what it holds (`while (toolame_buffer.size() > frame_len)`, strictly greater) in one loop with the SAME peak_left /
 * peak_right -- the values current on that call.  A live ZMQ / EDI capture of the reference therefore shows about ten units leaving
 * back to back every ten frames, sharing one level pair, and one unit always held back.  The batch calls emit the units of a frame in that
 * frame's slots with the levels the caller passes for that slot (tlb_tick_run: one frame per tick with that tick's peaks).  Payload bytes,
 * their order, DLFC / SEQ / timestamps per unit are identical; send cadence and the level pair per unit are not.  For a capture-compare
 * tlb_reference_send_schedule() gives the reference's schedule -- how many units it sends during each call -- so a caller can pass, for
 * every unit, the levels of the call the reference sends it on (pure host arithmetic on the configuration, no GPU). */
int tlb_reference_send_schedule(const tlb_stream_config *cfg, int ncalls, int32_t *units_sent);      /* -> bytes still held after the last call; < 0: -TLB_ERR_* */
int tlb_egress_unit_bytes(const tlb_batch *b, int stream);          /* 3 * kbps */
int tlb_egress_units_per_frame(const tlb_batch *b, int stream);     /* 1, 2, 3; 0 = not a whole number */
int tlb_egress_max_units_per_frame(const tlb_batch *b);
/* ZeroMQ part: one ODR-DabMux ZMQ message per unit,
 * `struct zmq_frame_header_t` (src/Outputs.h:76-89: u16 version = 1, u16 encoder = ZMQ_ENCODER_MPEG_L2 = 2, u32 datasize,
 * i16 audiolevel_left, i16 audiolevel_right, packed, little-endian) followed by the unit (Outputs.cpp:101-138).
 *   d_frames uint8 [nframes][nstreams][tlb_out_stride()]   (tlb_encode_device output)
 *   d_peaks  int16 [nframes][nstreams][2] or NULL (levels 0)  (tlb_ingest_device output; a frame's levels go with all its units)
 *   d_msgs   uint8 [nframes * max_upf][nstreams][tlb_zmq_msg_stride()]; message length of a stream = 12 + tlb_egress_unit_bytes()
 * Sockets and CURVE stay with the caller (out of scope). */
int tlb_zmq_msg_stride(const tlb_batch *b);
int tlb_zmq_frame_device(tlb_batch *b, const uint8_t *d_frames, const int16_t *d_peaks, int nframes, uint8_t *d_msgs, void *hip_stream);
int tlb_zmq_frame_host(tlb_batch *b, const uint8_t *frames, const int16_t *peaks, int nframes, uint8_t *msgs);

/* Egress framing, EDI part: the AF packet an EDI/TCP destination receives for one frame --
 * what EDI::write_frame builds (src/Outputs.cpp:194-261): TAG items *ptr("DSTI"), dsti, ss0001 (the frame), ODRa (audio
 * levels) and, every ten seconds, ODRv (version string + uptime) (contrib/edioutput/TagItems.cpp), wrapped by
 * AFPacketiser::Assemble (contrib/edioutput/AFPacket.cpp:46-94: "AF", LEN, SEQ, AR, PT 'T', payload, CRC-16/CCITT).
 * `tlb_edi_state` is the per-stream sender state (EDI::m_timestamp/m_edi_time/m_send_version_at_time/m_num_seconds_sent/
 * m_tist, AFPacketiser::m_seq, TagDSTI::dlfc); the call advances it by nframes.  tlb_edi_state_init() is the first-call
 * branch of write_frame (Outputs.cpp:200-212) with the wall clock and the TAI-UTC offset passed in by the caller.
 *   d_frames  uint8 [nframes][nstreams][tlb_out_stride()]       (tlb_encode_device output)
 *   d_levels  int16 [nframes][nstreams][2] or NULL (levels 0)   (tlb_ingest_device peaks)
 *   d_state   tlb_edi_state [nstreams]
 *   d_pkts    uint8 [nframes * max_upf][nstreams][tlb_edi_af_stride()], d_pkt_len int32 [nframes * max_upf][nstreams] = bytes used
 *             (slot order, see UNITS above: one AF packet per 24-ms unit, each advancing timestamp, DLFC and SEQ; 0 = absent slot)
 * `version` is host memory (<= 64 bytes).  The PFT layer for UDP destinations is tlb_edi_pft_* below; sockets stay with the caller. */
typedef struct tlb_edi_state {
    int64_t edi_time, send_version_at_time;
    uint32_t timestamp, num_seconds_sent;
    int32_t tai_utc_offset;
    uint16_t seq, dlfc;
    uint8_t tist, pad_[7];
} tlb_edi_state;
void tlb_edi_state_init(tlb_edi_state *st, long long now_s, unsigned delay_ms, int tist, int tai_utc_offset);
int tlb_edi_af_stride(const tlb_batch *b, int version_len);
int tlb_edi_af_device(tlb_batch *b, const uint8_t *d_frames, const int16_t *d_levels, int nframes, tlb_edi_state *d_state,
                      const char *version, int version_len, uint8_t *d_pkts, int32_t *d_pkt_len, void *hip_stream);
int tlb_edi_af_host(tlb_batch *b, const uint8_t *frames, const int16_t *levels, int nframes, tlb_edi_state *state,
                    const char *version, int version_len, uint8_t *pkts, int32_t *pkt_len);

/* EDI protection, fragmentation and transport layer (ETSI TS 102 821 clause 7): what
 * edi::PFT::Assemble (contrib/edioutput/PFT.cpp:234-320, with Protect :75-139 and ProtectAndFragment :141-232) makes of an
 * AF packet for UDP destinations -- Reed-Solomon RS(255,207) per chunk (fec = m > 0: m fragments may be lost), interleaved
 * fragments, PF header ("PF", Pseq, Findex, Fcount, FEC|Addr|Plen, [RSk, RSz], [Source, Dest], CRC-16) + payload.
 * fec = 0: fragmentation only (1400-byte slices), as the reference's default configuration (EDIConfig.h:69-70).
 *   d_af      uint8 [nframes][nstreams][af_stride], d_af_len int32 [nframes][nstreams]     (tlb_edi_af_device output)
 *   d_pseq    uint16 [nstreams]: PFT::m_pseq per stream, advanced by the number of packets present (d_af_len > 0); `nframes` here
 *             counts packet slots (nframes * max_upf of the AF call)
 *   d_frags   uint8 [nframes][nstreams][max_frags][frag_stride], d_frag_len int32 [nframes][nstreams][max_frags],
 *   d_nfrag   int32 [nframes][nstreams];  max_frags / frag_stride at least what tlb_edi_pft_shape() reports for this af_stride
 *   (every AF packet length up to af_stride is covered; at most 10 chunks per packet, i.e. chunk_len >= af_stride / 10)
 * chunk_len is edi::configuration_t::chunk_len (<= 207), transport/addr_source/dest_port the optional address header. */
int tlb_edi_pft_shape(const tlb_batch *b, int af_stride, int fec, int chunk_len, int transport, int *max_frags, int *frag_stride);
int tlb_edi_pft_device(tlb_batch *b, const uint8_t *d_af, const int32_t *d_af_len, int nframes, int af_stride, uint16_t *d_pseq,
                       int fec, int chunk_len, int transport, int addr_source, int dest_port,
                       uint8_t *d_frags, int32_t *d_frag_len, int32_t *d_nfrag, int max_frags, int frag_stride, void *hip_stream);
int tlb_edi_pft_host(tlb_batch *b, const uint8_t *af, const int32_t *af_len, int nframes, int af_stride, uint16_t *pseq,
                     int fec, int chunk_len, int transport, int addr_source, int dest_port,
                     uint8_t *frags, int32_t *frag_len, int32_t *nfrag, int max_frags, int frag_stride);

/* The real-time loop body as ONE call per tick (src/odr-audioenc.cpp:1030-1051 gain / peak, :1139-1152
 * de-interleave, :1158 toolame_encode_frame, :1208-1225 re-framing into units, src/Outputs.cpp:194-261 EDI::write_frame,
 * contrib/edioutput/PFT.cpp for UDP): one frame of EVERY stream goes host -> PCIe -> ingest -> encode -> EDI AF packets
 * (-> PFT fragments) -> PCIe -> host.  The tick object owns pinned host buffers and all device memory; streams are split into
 * `ngroups` contiguous groups whose copy-in, kernels and copy-out overlap on three HIP streams.
 *   1. fill tlb_tick_pcm(): int16 [nstreams][2304] interleaved s16le (and tlb_tick_xpad() [nstreams][TLB_MAX_XPAD] /
 *      tlb_tick_xpad_len() [nstreams] when created with_xpad)
 *   2. tlb_tick_run(): returns when everything is back in host memory
 *   3. read tlb_tick_peaks() int16 [nstreams][2] and, per stream, tlb_tick_frame() / tlb_tick_packet(unit) /
 *      tlb_tick_fragment(unit, k) (length 0 / count 0: nothing for this stream this tick)
 * What comes out of run number n is the frame that became final during it -- input frame n-1 (one frame of latency, see
 * tlb_encode_device; nothing on the very first run) -- in tlb_tick_units() units of 3*bitrate bytes (one per 48 kHz frame, two
 * per 24 kHz frame, three per 16 kHz frame: a run is one FRAME of every stream, so an LSF batch runs every 48 / 72 ms).
 * The audio levels sent with it are this run's peaks, as in the reference, whose send_frame() carries the peaks current at send
 * time (odr-audioenc.cpp:1213-1219).  tlb_tick_finish() pushes the last (pending) frame of every stream through the same
 * egress stage (toolame_finish at stream end); after it the object only answers the read accessors.
 * egress: TLB_TICK_FRAMES (raw MP2 frames, any sample rate), TLB_TICK_EDI_AF (AF packets, tlb_edi_af_device),
 * TLB_TICK_EDI_PFT (PFT fragments of those packets, tlb_edi_pft_device), TLB_TICK_ZMQ (ZeroMQ messages, tlb_zmq_frame_device).
 * Every run also advances the per-stream silence counter of src/odr-audioenc.cpp:1053-1079 (tlb_tick_silence_ms()).  The EDI sender state of every stream starts as
 * tlb_edi_state_init(now_s, delay_ms, tist, tai_utc_offset) and lives on the device. */
#define TLB_TICK_FRAMES 0
#define TLB_TICK_EDI_AF 1
#define TLB_TICK_EDI_PFT 2
#define TLB_TICK_ZMQ 3             /* ODR-DabMux ZeroMQ messages (tlb_zmq_frame_device): zmq_frame_header_t + unit */
typedef struct tlb_tick tlb_tick;
typedef struct {
    int egress;                    /* TLB_TICK_* */
    int ngroups;                   /* 0 = pick (1 below 2048 streams, 2 below 8192, 4 below 65536, else 8) */
    int with_xpad;                 /* X-PAD side input per tick */
    const char *version; int version_len;     /* ODRv string (EDI) */
    long long now_s; unsigned delay_ms; int tist; int tai_utc_offset;      /* tlb_edi_state_init() arguments */
    int fec, chunk_len, transport, addr_source, dest_port;                 /* PFT layer (chunk_len 0 = 207) */
} tlb_tick_config;
tlb_tick *tlb_tick_create(int device, int nstreams, const tlb_stream_config *cfgs, const tlb_tick_config *tc, int *err);
void tlb_tick_destroy(tlb_tick *t);
int tlb_tick_set_gain_db(tlb_tick *t, int stream, double gain_db);
/* tlb_stream_reset / _finish / _reconfigure for one stream of a tick object, between two runs.  The stream's EDI sender state (SEQ,
 * DLFC, timestamps) keeps running -- one continuous sender whose encoder restarted; until the stream's next frame is final its
 * packets / messages / frame have length 0. */
int tlb_tick_stream_reset(tlb_tick *t, int stream);
int tlb_tick_stream_finish(tlb_tick *t, int stream, uint8_t *out, size_t out_size);
int tlb_tick_stream_reconfigure(tlb_tick *t, int stream, const tlb_stream_config *cfg);
int16_t *tlb_tick_pcm(tlb_tick *t);
uint8_t *tlb_tick_xpad(tlb_tick *t);
int32_t *tlb_tick_xpad_len(tlb_tick *t);
/* SHORT READS (tlb_ingest_device_valid, tlb_underrun_device).  tlb_tick_enable_short_reads() before the first submit (TLB_ERR_ARG after
 * it) makes the object carry an int32 [nstreams] array of delivered sample frames with every input set: tlb_tick_valid() follows the
 * rules of tlb_tick_pcm() (it alternates; NULL while two ticks are in flight), and every set reads 1152 everywhere when it is handed
 * back, so a stream the caller does not touch is a full read.  The counters of tlb_underrun_device come back with the silence counter:
 * tlb_tick_underrun_ms() / tlb_tick_underruns(), uint32 [nstreams], of the tick waited for last.  The stream life-cycle calls leave
 * them alone, as they leave the silence counter.  An object that was never enabled makes the device calls it made before this existed;
 * its three accessors return NULL. */
int tlb_tick_enable_short_reads(tlb_tick *t);
int32_t *tlb_tick_valid(tlb_tick *t);
const uint32_t *tlb_tick_underrun_ms(const tlb_tick *t);
const uint32_t *tlb_tick_underruns(const tlb_tick *t);
int tlb_tick_run(tlb_tick *t);                 /* = tlb_tick_submit() + tlb_tick_wait() */
/* Ticks overlapped: the object owns TWO sets of pinned host input buffers (and three of outputs).  tlb_tick_submit() queues a tick on the input set the caller has
 * just filled and returns at once; from then on tlb_tick_pcm() / _xpad() / _xpad_len() point at the OTHER input set, which the caller
 * fills while the submitted tick is on its way (odr-audioenc decouples capture from encoding with its input queue,
 * src/odr-audioenc.cpp:904-986).  tlb_tick_wait() waits for the oldest submitted tick; the read accessors (tlb_tick_peaks, _frame,
 * _packet, _message, _fragment, _silence_ms) then show ITS results until the next wait -- the object keeps THREE sets of output buffers, so
 * neither of the two submits that may come before that wait touches them (a sender thread may ship them zero-copy).  Inputs: while two
 * ticks are in flight both input sets belong to queued copies and tlb_tick_pcm() / _xpad() / _xpad_len() return NULL; after the wait
 * the set of the retired tick is handed out again.  At most two ticks in flight: submit, submit, wait, submit, wait ...  Inside, tick t + 1's copy-in starts as soon as tick t's ingest kernel has consumed the device input buffer,
 * so the host-to-device link -- the limit at large stream counts -- never idles between ticks.  The RE-FETCH rule: call tlb_tick_pcm()
 * again after every submit / run, the pointer alternates. */
/* ERRORS.  A device failure inside submit / wait / run / finish (TLB_ERR_HIP, ...; TLB_ERR_ARG for calls out of order is NOT one) leaves the
 * object out of step with itself -- the stream groups queued before the failing one have advanced by a frame, the later ones have not --
 * so it is marked broken and STAYS so: every later submit / wait / run / finish / stream life-cycle call returns TLB_ERR_HIP, the input
 * accessors NULL; the read accessors keep showing the last tick that was waited for.  tlb_tick_status() = 0 or TLB_ERR_HIP.  The way
 * out is tlb_tick_destroy() and a new object (one level up: tlb_node_shard_restart does exactly that for one GPU of a node). */
int tlb_tick_submit(tlb_tick *t);
int tlb_tick_wait(tlb_tick *t);
int tlb_tick_status(const tlb_tick *t);
int tlb_tick_finish(tlb_tick *t);
long tlb_tick_count(const tlb_tick *t);
const int16_t *tlb_tick_peaks(const tlb_tick *t);
int tlb_tick_units(const tlb_tick *t, int stream);
const uint8_t *tlb_tick_frame(const tlb_tick *t, int stream, int *len);
const uint8_t *tlb_tick_packet(const tlb_tick *t, int stream, int unit, int *len);
const uint8_t *tlb_tick_message(const tlb_tick *t, int stream, int unit, int *len);      /* TLB_TICK_ZMQ */
const uint32_t *tlb_tick_silence_ms(const tlb_tick *t);      /* uint32 [nstreams]: the caller's silence counter (tlb_silence_device), after the run */
int tlb_tick_fragments(const tlb_tick *t, int stream, int unit);
const uint8_t *tlb_tick_fragment(const tlb_tick *t, int stream, int unit, int k, int *len);
float tlb_tick_last_ms(tlb_tick *t);           /* first copy-in queued -> last copy-out done of the last run, device clock */

/* ---------------------------------------------------------------------------------------------
 * (3) node level: every GPU of one host behind one handle (csrc/tlb_node.cpp)
 *
 * odr-audioenc is one process per service: AudioEnc::run() (src/odr-audioenc.cpp:819-1276) owns one input, one encoder, one set
 * of outputs.  A head-end that carries a fleet of services on one machine needs the step above: N streams cut into contiguous
 * blocks, block g = streams [g*N/G, (g+1)*N/G) on GPU g (section 8e), one host thread and one tlb_tick (or tlb_batch) per block,
 * nothing shared between blocks -- streams are independent, there is no collective on the data path -- and the counters added up.
 * A "shard" is such a block; `devices[g]` names the HIP device of shard g, and the same device may appear more than once (two
 * shards on one GPU behave as on two).  Every call below that acts on all shards runs on the shards' own threads in parallel and
 * returns when all of them have returned; the first non-zero code wins.  A stream keeps its node-wide index in every accessor.
 * Threading: ONE caller thread drives a node handle (the shards' threads are the node's own; the mailbox of a shard holds one job).
 * The function handed to tlb_node_parallel() runs on those threads and may use the accessors (tlb_node_pcm / _packet / ...), but
 * none of the calls that themselves go to the shards' threads (submit / wait / run / finish / sync / encode / life cycle / gain / copies):
 * they would wait for the thread they are running on.
 *
 * FAULT ISOLATION.  The reference restarts ONE failed input and nothing else (src/odr-audioenc.cpp:875-902, src/InputInterface.h:40);
 * one level up the unit of failure is a GPU.  A shard whose device call fails inside submit / wait / run / finish / encode / flush /
 * sync is marked BROKEN on the spot: its in-flight steps are dropped from the counters, every later node-wide call skips it, the
 * accessors of its streams answer NULL / 0 / length 0, the life-cycle calls of its streams TLB_ERR_HIP.  ALL OTHER SHARDS COMPLETE THE
 * CALL AND STAY IN LOCKSTEP -- their streams never notice.  The call in which a shard breaks returns that shard's code (the caller's
 * cue; later calls return 0 again, or TLB_ERR_HIP once no shard is left alive); tlb_node_shard_status() says which shard, with which TLB_ERR_* and
 * HIP's own error string; tlb_node_shard_restart() destroys the shard's object and makes a fresh one on the shard's own thread: its
 * streams start "as a freshly started reference process" (tlb_stream_reset's contract for the whole block), with the configurations
 * the streams have NOW and the caller's gains; it joins the lockstep at the next submit (first tick: nothing out, one frame of
 * latency).  Restart is legal between steps (no tick in flight / after tlb_node_sync), also on a healthy shard.
 *
 * TICK DEADLINE.  The above covers a device call that RETURNS an error; a call that does not return would hold up every shard, because
 * each node-wide call waits for all of them.  tlb_node_set_deadline_ms(ms > 0) bounds that wait on the TICK plane (the reference puts
 * its own wall-clock limits at this level of its loop: the underrun abort, src/odr-audioenc.cpp:925-931, and the silence timeout,
 * :1064-1079).  Off (0) by default; then nothing below applies and every call behaves as without the deadline.
 *   Deadline points.  tlb_node_wait: the node-level submit time of the step waited for, plus ms (the real-time budget runs from
 *   submit).  tlb_node_submit / tlb_node_finish: call start plus ms.  tlb_node_run is submit followed by wait.
 *   Going late.  A shard whose part of the call has not returned by its deadline becomes LATE (TLB_SHARD_LATE): the call returns
 *   TLB_ERR_LATE -- unless a shard broke in the same call, whose code then wins as above -- and the other shards' results of the call
 *   are readable.  Its job keeps running on its own thread; nothing is cancelled.
 *   While LATE.  Every node-wide call skips the shard (submit, wait, finish, set_gain_db(-1), tlb_node_parallel, whose fn is not called
 *   for it); the accessors of its streams answer NULL / 0 / length 0 -- tlb_node_pcm NULL, so nothing is written into buffers the shard
 *   may still use; the life-cycle calls of its streams, gain on one of them and tlb_node_shard_restart return TLB_ERR_LATE (a gain set
 *   meanwhile is remembered and applied when the shard comes back).  Each node step submitted meanwhile counts in missed_steps: its
 *   streams' input for that step is never encoded.
 *   Poll point.  Late shards are examined, without blocking, only at the end of tlb_node_wait (and so of tlb_node_run): the caller's
 *   next fill, which follows the wait in both the run() loop and the submit, submit, wait loop, reaches a shard that came back there
 *   before the next submit.  When the late job has returned
 *     - with an error: the shard is BROKEN exactly as above (its in-flight steps counted lost); that wait returns the code;
 *     - OK, with ticks of its own still in flight (the second tick of the pipelined loop): the node queues the wait for the next one and
 *       does not wait for it; the results of those ticks, and the late tick's own, are never shown (dropped_steps);
 *     - OK, with nothing in flight: the shard is OK again (rejoins) and takes part from the next submit on.  Nothing is restarted or
 *       reset: its encoders are those that have encoded every input the shard accepted.
 *   After a wait the accessors of a stream show results only if its shard took part in that node step; otherwise NULL / length 0,
 *   never the results of an older step.  tlb_node_shard_deadline_status() has the record of every shard; tlb_node_shard_status() and
 *   tlb_node_counters() report a late shard as it stood before the late call.
 *   Unit of isolation: a DEVICE.  A real hang of a GPU stalls every shard placed on it; the deadline keeps the shards on OTHER devices on
 *   air.  tlb_node_destroy() still waits for a late shard's job without a limit: a shard that never returns is the caller's cue to exit
 *   non-zero, or to drive that GPU from a fresh child process (never by re-executing the process that holds the GPU).
 *
 * Two planes, chosen at creation:
 *   TLB_NODE_TICK   the real-time loop: a tlb_tick per shard, host buffers in, packets out (everything of tlb_tick_* per stream).
 *   TLB_NODE_BATCH  device-resident buffers: a tlb_batch per shard, tlb_node_encode_device() takes one device pointer per shard.
 * ------------------------------------------------------------------------------------------ */
#define TLB_NODE_TICK 0
#define TLB_NODE_BATCH 1
typedef struct tlb_node tlb_node;
typedef struct {
    int plane;                     /* TLB_NODE_TICK / TLB_NODE_BATCH */
    tlb_tick_config tick;          /* TICK plane: egress, groups per shard, X-PAD, EDI / PFT parameters (as for tlb_tick_create) */
} tlb_node_config;
typedef struct {
    int shard, device;             /* total record: shard = -1, device = -1 */
    int first, nstreams;           /* the block [first, first + nstreams) */
    long steps;                    /* COMPLETED steps: ticks waited for (TICK) / encode calls retired by tlb_node_sync (BATCH); total record: the minimum over the shards */
    long frames;                   /* (stream, frame) pairs of the completed steps: sum of nstreams * frames per step (steps a shard lost by breaking are not counted) */
    double busy_ns;                /* host clock, this shard: submit (TICK) / the oldest queued encode call (BATCH) -> its results waited for (synced), summed; two ticks in flight overlap; total: the maximum */
    double device_ms;              /* device clock, summed over the completed steps.  TICK: tlb_tick_last_ms() of every tick.  BATCH: every queued encode call has its own
                                      pair of events on the shard's stream (first kernel queued -> last kernel done), added up at tlb_node_sync.  total: the maximum */
    double wall_ns;                /* total record only: first submit -> last wait as the node saw them, summed over steps */
} tlb_node_counter;
/* health and identity of one shard (tlb_node_shard_status) */
#define TLB_SHARD_OK 0
#define TLB_SHARD_BROKEN 1
#define TLB_SHARD_LATE 2             /* TICK plane with a deadline: its job missed the deadline and has not been seen to return (TICK DEADLINE) */
#define TLB_NODE_WHAT_LEN 192
#define TLB_NODE_NAME_LEN 64
typedef struct {
    int shard, device, first, nstreams;
    int state;                     /* TLB_SHARD_OK / TLB_SHARD_BROKEN / TLB_SHARD_LATE */
    int last_err;                  /* TLB_ERR_* of the failure that broke it last (kept after a restart), 0 = never failed */
    long failures, restarts;       /* times it broke / was restarted */
    long lost_steps;               /* steps that were in flight when it broke (not in the counters) */
    char what[TLB_NODE_WHAT_LEN];  /* the failing call, its code and HIP's error string of the shard's thread */
    char device_name[TLB_NODE_NAME_LEN];   /* hipDeviceProp_t::name */
    char pci[24];                  /* domain:bus:device.0 */
    char uuid[36];                 /* hipDeviceProp_t::uuid as 32 hex digits: two shards on DISTINCT GPUs differ here */
    int num_cu, num_xcd;           /* compute units, XCDs (hipDeviceAttributeNumberOfXccs) */
    double hbm_gb;
} tlb_node_shard_info;

/* Pure arithmetic, no GPU: the block of shard g, and what tlb_create() will make of it -- the number of distinct configurations,
 * the streams per kernel list (psy model 0, 1, 2 (with 4), 3: each list is one homogeneous launch) and the mono streams that share
 * waves in pairs.  Returns 0, or the TLB_ERR_* code of the first illegal configuration in the block. */
void tlb_node_partition(int nstreams, int nshards, int shard, int *first, int *n);
int tlb_node_plan_shard(int nstreams, const tlb_stream_config *cfgs, int nshards, int shard,
                        int *first, int *n, int *nconfigs, int list_sizes[4], int *mono_pairs);

tlb_node *tlb_node_create(int nshards, const int *devices, int nstreams, const tlb_stream_config *cfgs, const tlb_node_config *nc, int *err);
void tlb_node_destroy(tlb_node *nd);
int tlb_node_nshards(const tlb_node *nd);
int tlb_node_nstreams(const tlb_node *nd);
int tlb_node_shard_of(const tlb_node *nd, int stream);
/* per_shard: [nshards] records or NULL; total: frames summed, steps = the minimum over the shards, busy_ns / device_ms = the maximum, wall_ns; or NULL */
int tlb_node_counters(const tlb_node *nd, tlb_node_counter *per_shard, tlb_node_counter *total);
/* One line per shard: device ordinal and name, CUs, XCDs, memory, PCI address, UUID, stream block -- what a log of a multi-GPU run
 * should open with (also printed to stderr at creation when TLB_VERBOSE is set in the environment).  Valid until tlb_node_destroy. */
const char *tlb_node_describe(const tlb_node *nd);
/* Returns TLB_SHARD_OK / TLB_SHARD_BROKEN / TLB_SHARD_LATE (negative: -TLB_ERR_ARG) and fills *info (may be NULL). */
int tlb_node_shard_status(const tlb_node *nd, int shard, tlb_node_shard_info *info);
/* TICK DEADLINE (above): ms > 0 sets it, 0 turns it off (the default).  TICK plane only, between steps only: TLB_ERR_ARG on a BATCH
 * node, for a negative or non-finite value, or while a step is in flight. */
int tlb_node_set_deadline_ms(tlb_node *nd, double ms);
/* the deadline record of one shard (tlb_node_shard_deadline_status; a struct of its own: tlb_node_shard_info keeps its size) */
typedef struct {
    int state;                     /* TLB_SHARD_OK / TLB_SHARD_BROKEN / TLB_SHARD_LATE */
    long late_events;              /* times the shard went late */
    long rejoins;                  /* times it came back on its own */
    long dropped_steps;            /* steps it completed after the node had given up on them: their results are never shown */
    long missed_steps;             /* node steps submitted while it was late: its streams' input for them is never encoded */
    long last_late_step;           /* node step index (0-based count of node submits) at which it last went late; -1: never */
    long last_rejoin_step;         /* first node step it took part in after coming back; -1: never */
    double worst_overrun_ms;       /* longest a late job ran past its deadline, as seen at the node's poll points */
} tlb_node_shard_deadline;
/* Returns the state as tlb_node_shard_status does (negative: -TLB_ERR_ARG) and fills *info (may be NULL). */
int tlb_node_shard_deadline_status(const tlb_node *nd, int shard, tlb_node_shard_deadline *info);
/* Destroy + re-create one shard's object (see FAULT ISOLATION above).  now_s >= 0: the EDI timestamp origin of the restarted senders
 * (TICK plane; < 0 keeps the creation-time value).  Returns 0, TLB_ERR_ARG while a step is in flight or after finish, or the code
 * the re-creation failed with (the shard then stays broken and may be restarted again). */
int tlb_node_shard_restart(tlb_node *nd, int shard, long long now_s);
/* Run fn(ctx, shard, first, n) once per shard ON THAT SHARD'S THREAD, all at once, and wait: the caller's own per-block work --
 * filling the pinned PCM of a block from its inputs, shipping a block's packets -- parallel over the shards without a second pool. */
int tlb_node_parallel(tlb_node *nd, void (*fn)(void *ctx, int shard, int first, int n), void *ctx);

/* TICK plane.  tlb_node_pcm(stream) is that stream's int16[2304] slot (interleaved s16le) in its shard's current input set, NULL
 * while two ticks are in flight (see tlb_tick_pcm); the shards tick in lockstep, so submit / wait / run / finish follow the rules
 * of tlb_tick_submit / _wait / _run / _finish.  The read accessors are tlb_tick_*'s with node-wide stream indices. */
int16_t *tlb_node_pcm(tlb_node *nd, int stream);
uint8_t *tlb_node_xpad(tlb_node *nd, int stream);            /* uint8[TLB_MAX_XPAD] */
int32_t *tlb_node_xpad_len(tlb_node *nd, int stream);
/* short reads: tlb_tick_enable_short_reads of every shard (before the first submit; a restarted shard is enabled again);
 * tlb_node_valid(stream) is that stream's int32 in its shard's current input set -- NULL when not enabled, while two ticks are in flight
 * and for a broken or late shard, whose input is not written */
int tlb_node_enable_short_reads(tlb_node *nd);
int32_t *tlb_node_valid(tlb_node *nd, int stream);
int tlb_node_submit(tlb_node *nd);
int tlb_node_wait(tlb_node *nd);
int tlb_node_run(tlb_node *nd);
int tlb_node_finish(tlb_node *nd);
int tlb_node_units(const tlb_node *nd, int stream);
const int16_t *tlb_node_peaks(const tlb_node *nd, int stream);          /* int16[2] */
uint32_t tlb_node_silence_ms(const tlb_node *nd, int stream);
uint32_t tlb_node_underrun_ms(const tlb_node *nd, int stream);         /* 0 when not enabled, and for a broken, late or stale shard */
uint32_t tlb_node_underruns(const tlb_node *nd, int stream);
const uint8_t *tlb_node_frame(const tlb_node *nd, int stream, int *len);
const uint8_t *tlb_node_packet(const tlb_node *nd, int stream, int unit, int *len);
const uint8_t *tlb_node_message(const tlb_node *nd, int stream, int unit, int *len);
int tlb_node_fragments(const tlb_node *nd, int stream, int unit);
const uint8_t *tlb_node_fragment(const tlb_node *nd, int stream, int unit, int k, int *len);
/* both planes: gain and the life cycle of one stream (tlb_stream_* / tlb_tick_stream_* of its shard) */
int tlb_node_set_gain_db(tlb_node *nd, int stream, double gain_db);     /* stream = -1: all */
int tlb_node_stream_reset(tlb_node *nd, int stream);
int tlb_node_stream_finish(tlb_node *nd, int stream, uint8_t *out, size_t out_size);
int tlb_node_stream_reconfigure(tlb_node *nd, int stream, const tlb_stream_config *cfg);

/* BATCH plane.  tlb_node_batch(shard) is the shard's tlb_batch (sizes: tlb_out_stride, tlb_frame_bytes; do not encode on it
 * directly).  Device memory of a shard's GPU for callers without a HIP toolchain: tlb_node_device_alloc / _free / _copy_in / _copy_out
 * (synchronous).  tlb_node_encode_device(): element g of every pointer array is shard g's buffer, laid out as tlb_encode_device_len
 * wants it for THAT shard's streams ([nframes][n_g]...); d_xpad / d_xpad_len / d_out_len may be NULL (or hold NULL elements).  Each
 * shard's launch is queued on the shard's own HIP stream by the shard's thread; the call returns when all are queued,
 * tlb_node_sync() when all have finished.  tlb_node_flush_device(): the pending frames, tlb_flush_device_len per shard. */
tlb_batch *tlb_node_batch(tlb_node *nd, int shard);
void *tlb_node_device_alloc(tlb_node *nd, int shard, size_t bytes);
void tlb_node_device_free(tlb_node *nd, int shard, void *d_ptr);
int tlb_node_copy_in(tlb_node *nd, int shard, void *d_dst, const void *src, size_t bytes);
int tlb_node_copy_out(tlb_node *nd, int shard, void *dst, const void *d_src, size_t bytes);
int tlb_node_encode_device(tlb_node *nd, const int16_t *const *d_pcm, int nframes, const uint8_t *const *d_xpad,
                           const int32_t *const *d_xpad_len, uint8_t *const *d_out, int32_t *const *d_out_len);
int tlb_node_flush_device(tlb_node *nd, uint8_t *const *d_out, int32_t *const *d_out_len);
int tlb_node_sync(tlb_node *nd);

/* ---------------------------------------------------------------------------------------------
 * Frame check and decode: the confidence monitor for the batch's OWN frames.
 * tlb_decode_*() reads frames as tlb_encode_*_len / tlb_flush_*_len leave them -- slot stride tlb_out_stride(), a length per slot,
 * 0 = empty slot -- and checks each against the configuration of the stream it belongs to; on request it also hands back the parsed
 * fields and the decoded audio.  One wavefront per (stream, slot); nothing is shipped to the host unless the host variant is used.
 *   d_frames uint8  [nframes][nstreams][tlb_out_stride()]
 *   d_len    int32  [nframes][nstreams] or NULL: every slot holds a frame (of the length its padding bit and configuration say)
 *   d_report tlb_frame_report [nframes][nstreams]
 *   d_fields tlb_frame_fields [nframes][nstreams] or NULL: bit_alloc / scfsi / scalar / subband in the layout of the encoder's stage
 *            taps; cells the frame does not transmit are 0 (a joint-stereo cell above the bound: samples under channel 0 only)
 *   d_pcm    int16  [nframes][nstreams][2][1152] or NULL: planar like the encoder's input; a mono stream fills channel 0 (channel 1: zeros)
 * status is a set of independent flags.  A frame "passes" when none of TLB_DEC_BAD_MASK and not EMPTY is set.
 *   - the header is compared field by field with the stream's configuration; a joint-stereo stream's frames may be stereo or joint
 *     stereo with any bound (the encoder chooses per frame).  A slot longer than its frame is a HEADER_MISMATCH, a shorter one OVERRUN.
 *   - CRC-16 over header bits 16..31, bit_alloc and scfsi; stored and computed value are both reported.
 *   - DAB ScF-CRC: the bytes protecting frame n's scalefactors travel in the tail of frame n-1 (toolame.c:527-542), so frame n is checked
 *     against the last non-empty slot before it (in this call or, for the call's first frames, the call before).  Where there is none --
 *     the first frame after creation or a reset -- or that slot was too short to hold its tail, the flag is SCFCRC_UNCHECKED, not an error.
 *   - bit budget: header + CRC + allocation + scfsi + scalefactors + samples + the smallest PAD (ScF-CRC + F-PAD) must fit the frame.
 *     No read leaves the slot whatever its bytes say.
 * PCM: requantisation by ISO/IEC 11172-3 2.4.3.3.4, synthesis filterbank by Annex 3-A.2 in fp64, rounded to nearest, saturated.  A frame
 * that did not pass, or an empty slot, yields 1152 zero samples per channel and counts as silence for its successor's filter history.
 * The output does not depend on how a stream's frames are cut into calls: a call leaves the stream's last slot behind for the next.
 * That state and the decoder's tables are allocated by the first decode call: a batch that never decodes pays nothing.
 * Asynchronous on `hip_stream` like tlb_encode_device; decode calls of one batch must be ordered on one stream (the very first decode
 * call of a batch also waits for the device once, while it uploads its tables).  Every buffer must be 4-byte aligned (hipMalloc'ed
 * memory is): frames and PCM move as 32-bit words.  Argument errors -- a NULL batch, frames or report pointer, nframes <= 0, a
 * misaligned pointer -- return TLB_ERR_ARG and change nothing.
 *   tlb_decode_reset(b, stream)  the stream's next frame is "first after a reset" again (stream = -1: all); tlb_reset, tlb_stream_reset,
 *                                tlb_stream_finish and tlb_stream_reconfigure do the same for the streams they touch
 *   tlb_decode_bad_frames(b)     frames with any TLB_DEC_BAD_MASK flag since creation (waits for the device; < 0: -TLB_ERR_*)
 * Note on tlb_stream_finish: it resets the stream BEFORE the caller holds the frame it returns, so that frame, decoded afterwards, is a
 * "first frame" (SCFCRC_UNCHECKED, silent filter history) -- unlike the same frame obtained through tlb_flush_*, which resets nothing.
 * A caller that wants the last frame checked against its predecessor flushes (or decodes the pending frame's slot) before finishing.
 * Where lengths are given, a frame whose slot length and padding bit disagree (cut short, or its padding bit damaged) cannot be trusted
 * to hold its tail where expected: its successor is SCFCRC_UNCHECKED rather than falsely BAD_SCFCRC.
 * ------------------------------------------------------------------------------------------ */
enum {
    TLB_DEC_EMPTY = 0x01, TLB_DEC_BAD_SYNC = 0x02, TLB_DEC_HEADER_MISMATCH = 0x04, TLB_DEC_BAD_CRC16 = 0x08, TLB_DEC_BAD_SCFCRC = 0x10,
    TLB_DEC_SCFCRC_UNCHECKED = 0x20, TLB_DEC_BAD_ALLOC = 0x40, TLB_DEC_OVERRUN = 0x80,
    TLB_DEC_BAD_MASK = 0x02 | 0x04 | 0x08 | 0x10 | 0x40 | 0x80,
    TLB_DEC_UNWANTED = 0x100,     /* adapted feeds only (below): the slot held bytes on a tick whose slot is not read; not in TLB_DEC_BAD_MASK */
};
typedef struct { uint32_t status; uint16_t crc_stored, crc_computed; uint8_t mode, mode_ext; uint16_t audio_bits; } tlb_frame_report;
typedef struct { uint8_t bit_alloc[2][32], scfsi[2][32], scalar[2][3][32]; uint16_t subband[2][3][12][32]; } tlb_frame_fields;
int tlb_decode_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, tlb_frame_report *d_report,
                      tlb_frame_fields *d_fields, int16_t *d_pcm, void *hip_stream);
int tlb_decode_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int nframes, tlb_frame_report *report,
                    tlb_frame_fields *fields, int16_t *pcm);
int tlb_decode_reset(tlb_batch *b, int stream);
long tlb_decode_bad_frames(const tlb_batch *b);

/* ---------------------------------------------------------------------------------------------
 * Confidence monitor: the frame check above where the frames are -- inside the real-time loop (tlb_tick_*, tlb_node_*), which keeps them on
 * the device between encode and egress.  Three questions per stream and tick: did the frame that just left pass its checks, how many
 * failed and how many in a row, is there audio at the output when there is audio at the input.  Opt-in at every level: an object that
 * never enables it makes exactly the device calls it made before this existed.
 *
 * THE FOLD (batch level).  tlb_monitor_*() folds what tlb_decode_*() reports into ONE 32-byte record per stream (little-endian, no padding):
 *   d_report tlb_frame_report [nframes][nstreams]     (tlb_decode_device output)
 *   d_pcm    int16 [nframes][nstreams][2][1152] exactly as tlb_decode_device writes it, or NULL
 *   d_record tlb_monitor_record [nstreams], read-modify-write like d_silence_ms: the caller zeroes it once
 * A stream's slots are taken in order; with st the slot's status:
 *   1. last_status = st, flags_seen |= st.
 *   2. st & TLB_DEC_EMPTY: out_peak = {0, 0}; nothing else changes.
 *   3. frames++.  st & TLB_DEC_BAD_MASK: bad_frames++ and bad_run++; otherwise bad_run = 0.
 *   4. with PCM: out_peak[c] = max(0, max_i pcm[c][i]); out_silence_ms gains the frame's duration -- the one tlb_silence_device adds for the
 *      stream's configuration -- when both peaks are 0 and goes back to 0 otherwise.  A frame that failed decodes to zeros and so counts
 *      as silence: that is what a listener hears.
 *   5. without PCM: out_peak and out_silence_ms stay as they are.
 * Integer arithmetic throughout: the result does not depend on how a stream's slots are cut into calls.  Asynchronous on `hip_stream` and
 * ordered like the decode calls; one wavefront per stream.  A NULL batch, report or record pointer, nframes <= 0 or a pointer that is not
 * 4-byte aligned return TLB_ERR_ARG and change nothing.
 * ------------------------------------------------------------------------------------------ */
typedef struct {
    uint32_t frames;               /* non-empty slots looked at */
    uint32_t bad_frames;           /* of those, with any TLB_DEC_BAD_MASK flag */
    uint32_t bad_run;              /* bad frames in a row ending at the last non-empty slot; 0 after a frame that passed */
    uint32_t flags_seen;           /* OR of every status looked at */
    uint32_t last_status;          /* status of the last slot looked at, EMPTY included */
    uint32_t out_silence_ms;       /* the silence counter of tlb_silence_device, on the DECODED audio */
    int16_t out_peak[2];           /* max(0, samples) per channel of the last slot's decoded audio, as tlb_ingest_device's peaks */
    uint32_t reserved_;            /* 0 */
} tlb_monitor_record;
int tlb_monitor_device(tlb_batch *b, const tlb_frame_report *d_report, const int16_t *d_pcm, int nframes, tlb_monitor_record *d_record,
                       void *hip_stream);
int tlb_monitor_host(tlb_batch *b, const tlb_frame_report *report, const int16_t *pcm, int nframes, tlb_monitor_record *record);
/* TICK PLANE.  tlb_tick_enable_monitor(what) before the first submit (TLB_ERR_ARG after it, and for any other `what`; TLB_ERR_HIP on a
 * broken object; a second call with the same `what` is OK): every tick that has frames -- all but the first, and tlb_tick_finish's flushed
 * frames -- then queues tlb_decode_device on the group's frames behind its egress kernels, and the fold into the group's device records.
 * The packets' copy-out does not wait for either; the records travel behind it, in three host sets like the silence counter.
 *   TLB_MONITOR_CHECK  unpack and verify only: frames, bad_frames, bad_run, flags_seen, last_status
 *   TLB_MONITOR_AUDIO  also synthesise: out_peak, out_silence_ms, listen (implies CHECK)
 * tlb_tick_monitor() shows tlb_monitor_record [nstreams] of the tick waited for last -- NULL when the monitor is not enabled; on a broken
 * object the last good tick, like the other read accessors.  The group's batch owns the decoder state, so the stream life-cycle calls
 * reset the decoder for the stream they touch (its next frame is SCFCRC_UNCHECKED); they leave the records alone, as they leave the silence
 * counter.  A record counts the frames that LEFT: after T submits and tlb_tick_finish, frames == T.
 * LISTEN (AUDIO only; TLB_ERR_ARG otherwise, and for a stream out of range): tlb_tick_monitor_listen(stream) selects ONE stream, or -1 for
 * none (the default), between any two submits and from the next submit on; that stream's decoded frame, int16 [2][1152], then comes back
 * with every tick (one 4608-byte copy).  tlb_tick_monitor_pcm() shows it for the tick waited for last, *stream (may be NULL) = the stream
 * that tick carried; NULL with *stream = -1 when none was selected, on the first tick, or when the monitor is not enabled.
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_monitor goes to every shard before the first submit, and a
 * restarted shard is enabled again -- its records start from zero, its streams are fresh.  tlb_node_monitor(stream) takes a node-wide index
 * and answers NULL when not enabled and for a broken, late or stale shard.  tlb_node_monitor_listen routes to the stream's shard and clears
 * the selection on the others: TLB_ERR_HIP for a stream of a broken shard, TLB_ERR_LATE for one of a late shard. */
#define TLB_MONITOR_CHECK 1
#define TLB_MONITOR_AUDIO 2
int tlb_tick_enable_monitor(tlb_tick *t, int what);
const tlb_monitor_record *tlb_tick_monitor(const tlb_tick *t);
int tlb_tick_monitor_listen(tlb_tick *t, int stream);
const int16_t *tlb_tick_monitor_pcm(const tlb_tick *t, int *stream);
int tlb_node_enable_monitor(tlb_node *nd, int what);
const tlb_monitor_record *tlb_node_monitor(const tlb_node *nd, int stream);
int tlb_node_monitor_listen(tlb_node *nd, int stream);
const int16_t *tlb_node_monitor_pcm(const tlb_node *nd, int *stream);

/* ---------------------------------------------------------------------------------------------
 * Compare: is the decoded audio the audio that went in?  The record above answers "is there audio at the output" with peaks and a silence
 * counter; it cannot see a perfectly valid frame that carries the WRONG audio -- stream k's slot holding stream j's programme, left and
 * right exchanged, a mono pair crossed, a shard's block shifted by one stream, a stale frame sent again.  Those are the faults of a
 * batched encoder's indexing, and every one of them has good CRCs and non-silent audio.  tlb_compare_*() sets the planar PCM the encoder
 * was given beside the PCM tlb_decode_*() synthesised from the frame that left, at the codec's delay, and correlates them in integers.
 *   d_in_pcm  int16 [nframes][nstreams][2][1152]  the d_pcm of the tlb_encode_device call, or NULL (see FLUSH)
 *   d_dec_pcm int16 [nframes][nstreams][2][1152]  the d_pcm tlb_decode_device wrote for that call's d_out
 *   d_report  tlb_frame_report [nframes][nstreams] of that decode call
 *   d_record  tlb_compare_record [nstreams], read-modify-write like the monitor's: the caller zeroes it once
 * One stream, slot f.  Output slot f holds input frame f - 1, so dec[f] is the audio of the previous input frame.  The batch keeps, per
 * stream, that previous input frame P and the last D = TLB_COMPARE_DELAY samples Q of the one before (allocated by the first compare call,
 * as the decoder's state is).  With x[c][i] = Q[c][i] for i < D, P[c][i - D] for i >= D, and y[c][i] = dec[f][c][i], over i = 0..1151:
 *   sxx[c] = sum x^2, syy[c] = sum y^2, sxy[c] = sum x y, sxz[c] = sum x[c] y[1 - c]      (int64, below 2^41 in magnitude)
 * A one-channel stream uses c = 0 only; the rest is 0.  After the slot the history advances by in[f].
 *   channel c is JUDGED   when sxx[c] >= min_energy
 *   channel c MATCHES     when sxy[c] > 0 and corr_den^2 sxy[c]^2 >= corr_num^2 sxx[c] syy[c], compared as 128-bit integers;
 *   the CROSS test        is the same with sxz[c] and syy[1 - c]
 *   the frame is a MISMATCH when any judged channel fails to match; it is SWAPPED when the stream has two channels, both are judged, neither
 *   matches and both cross tests match.
 * frames_compared++; with a judged channel frames_judged++, and a mismatch adds to mismatch_frames and mismatch_run while a match sets
 * mismatch_run to 0 -- a frame nobody judged leaves mismatch_run alone.  The sums and last_flags are those of the last compared slot.
 * SKIPPED: a slot whose report has TLB_DEC_EMPTY or any TLB_DEC_BAD_MASK flag is not compared: last_flags = TLB_COMPARE_SKIPPED, sums and
 * counters stay; its input still advances the history.  FLUSH: with d_in_pcm == NULL (nframes must be 1) the pending frame -- tlb_flush_*'s,
 * decoded -- is compared against the history, which does not advance.  Integer arithmetic throughout, no floating point anywhere: the
 * result does not depend on how a stream's slots are cut into calls.  tlb_reset, tlb_stream_reset, tlb_stream_finish and
 * tlb_stream_reconfigure clear the history of the streams they touch (zeros: never judged until two frames have gone in) and leave the
 * records alone; tlb_compare_reset(b, stream) does only that (stream = -1: all).  Asynchronous on `hip_stream`, ordered like the decode
 * calls; one wavefront per stream.  A NULL batch, decoded PCM, report, params or record pointer, nframes <= 0, a NULL d_in_pcm with
 * nframes != 1, a PCM pointer that is not 16-byte aligned (report: 4, record: 8; hipMalloc'ed memory is) or params outside
 * 0 < corr_num <= corr_den <= 1024, min_energy >= 1 return TLB_ERR_ARG and change nothing.
 * THE DELAY is measured, not assumed (tests/test_compare_emu.py: the lag of the largest sum in dec over 0..1151, white noise, the same for
 * 48 kHz stereo, 24 kHz mono and joint stereo): 481 = the analysis and the synthesis filterbank.  THE DEFAULTS come from
 * profiles/compare_margins.txt (tools/compare_margins.py): the smallest correlation of a healthy stream and the largest
 * of a mispaired one over every (rate, mode, bitrate) of the configuration sweep; the default ratio 3/8 lies between the two.
 * COMPARE NOT MEANINGFUL WITH DEFAULT PARAMS (a healthy stream's correlation falls below the ratio or within 0.05 of it; two or three subbands
 * are transmitted): 8 kbps at 24 kHz in 's', 'j' and 'd' (0.05, 0.28, 0.05) and at 22.05 kHz in 's' and 'd' (0.376: on the ratio).
 * Usable with little room (within 0.1): 8 kbps at 22.05 kHz 'j' (0.46) and at 16 kHz 's', 'j', 'd' (0.46).  Over the other 327
 * configurations the smallest healthy correlation is 0.56 and the largest mispaired one 0.18 (0.19 with the four just named).
 * TICK PLANE.  tlb_tick_enable_compare(params) after tlb_tick_enable_monitor(TLB_MONITOR_AUDIO) and before the first submit (TLB_ERR_ARG
 * otherwise; a second call with identical params is OK): every tick then queues the compare behind the group's decode, with the tick's
 * planar PCM as input (the group's batch keeps the previous tick's through its history, 6.4 KB per stream); tlb_tick_finish's flushed
 * frames go through the NULL-input form.  tlb_tick_compare() shows tlb_compare_record [nstreams] of the tick waited for last, NULL when not
 * enabled; the records travel in three host sets behind the packets' copy-out, like the monitor's.  Nothing is allocated or launched
 * unless compare is enabled.  NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): every shard is enabled, a restarted shard is enabled
 * again with zero records, and tlb_node_compare(stream) answers NULL when not enabled and for a broken, late or stale shard.
 * ------------------------------------------------------------------------------------------ */
#define TLB_COMPARE_DELAY 481
#define TLB_COMPARE_JUDGED0 0x01u
#define TLB_COMPARE_JUDGED1 0x02u
#define TLB_COMPARE_MISMATCH 0x04u
#define TLB_COMPARE_SWAPPED 0x08u
#define TLB_COMPARE_SKIPPED 0x10u
#define TLB_COMPARE_DEFAULT_MIN_ENERGY 75497472      /* 1152 * 256^2: a frame at - 42 dBFS */
#define TLB_COMPARE_DEFAULT_CORR_NUM 3               /* 3/8: between the largest mispaired (0.18) and the smallest healthy correlation (0.56) outside the nine 8 kbps two-channel LSF configurations named above */
#define TLB_COMPARE_DEFAULT_CORR_DEN 8
typedef struct { int64_t min_energy; int32_t corr_num, corr_den; } tlb_compare_params;
typedef struct {
    int64_t sxx[2], syy[2], sxy[2], sxz[2];      /* of the last compared slot */
    uint32_t frames_compared;      /* slots that were not skipped */
    uint32_t frames_judged;        /* of those, with at least one judged channel */
    uint32_t mismatch_frames;      /* of those, with a judged channel that did not match */
    uint32_t mismatch_run;         /* mismatches in a row ending at the last judged frame; 0 after a judged frame that matched */
    uint32_t swapped_frames;       /* mismatches whose channels match crosswise */
    uint32_t last_flags;           /* TLB_COMPARE_* of the last slot */
    uint32_t reserved_[2];         /* 0 */
} tlb_compare_record;
int tlb_compare_device(tlb_batch *b, const int16_t *d_in_pcm, const int16_t *d_dec_pcm, const tlb_frame_report *d_report, int nframes,
                       const tlb_compare_params *params, tlb_compare_record *d_record, void *hip_stream);
int tlb_compare_host(tlb_batch *b, const int16_t *in_pcm, const int16_t *dec_pcm, const tlb_frame_report *report, int nframes,
                     const tlb_compare_params *params, tlb_compare_record *record);
int tlb_compare_reset(tlb_batch *b, int stream);
int tlb_tick_enable_compare(tlb_tick *t, const tlb_compare_params *params);
const tlb_compare_record *tlb_tick_compare(const tlb_tick *t);
int tlb_node_enable_compare(tlb_node *nd, const tlb_compare_params *params);
const tlb_compare_record *tlb_node_compare(const tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * Resample: 44.1 and 32 kHz sources (and their halves) to the encoder's rate, on the device, ahead of the ingest.
 * Every entry point above takes PCM at tlb_stream_config.samplerate.  The reference's users never see that: its inputs convert before the
 * samples reach AudioEnc::run() (src/VLCInput.cpp:208, `samplerate=` in the transcode chain; src/GSTInput.cpp:124-133, an audioresample
 * element).  The reference has no resampler of its own to be bit-exact against, so this section DEFINES one, in integers.
 *   source rate -> encoder rate     ratio L/M
 *   44100 -> 48000, 22050 -> 24000  160/147
 *   32000 -> 48000, 16000 -> 24000  3/2
 * Any other pair is TLB_ERR_SAMPLERATE here.  Sources ABOVE a 24 kHz encoder's rate (48, 44.1 and 32 kHz) are a family of their own with
 * wider slots: "Down sources" below (tlb_decimate_*).  48 -> 44.1 / 32 kHz is out of scope.
 * THE TAPS.  One table per ratio, int16 H[L][T], T = TLB_RESAMPLE_TAPS = 32, committed as csrc/tl_resample_taps.inc: the committed table is
 * the definition, tools/gen_resample_taps.py the record of how it was made (N = L T; c = k - (N - 1) / 2; fc = 0.95 * 0.5 / L;
 * h[k] = L 2 fc sinc(2 fc c) kaiser(N, 8)[k]; row p = h[p::L] scaled to sum 32768, rounded half up, the remainder added to the row's tap of
 * largest magnitude).  Every row sums to exactly 32768; tlb_resample_taps() hands the table out.
 * THE FORMULA.  For a stream, count output samples n and source frames from the stream's last reset; a source frame is an L/R pair, or one
 * sample of a one-channel stream.  With q(n) = floor(n M / L) and p(n) = (n M) mod L:
 *   acc(n) = sum over t = 0..T-1 of H[p(n)][t] * x[q(n) - t]      (x[j] = 0 for j < 0; the exact integer sum)
 *   y(n)   = clamp((acc(n) + 16384) >> 15, -32768, 32767)         (arithmetic shift, i.e. floor)
 * per channel, both channels with the same q and p.  Frame f of the stream is y(1152 f .. 1152 f + 1151); it consumes the source frames
 * up to q(1152 (f + 1) - 1):
 *   need(f) = q(1152 (f + 1) - 1) + 1 - (f > 0 ? q(1152 f - 1) + 1 : 0)
 * 160/147: 1058 or 1059 in a cycle of five frames that add up to 5292; 3/2: always 768.  Never above 1152: a slot of 2304 values holds it.
 * BUFFERS.  d_source and d_interleaved are both int16 [nframes][nstreams][2304] and must not overlap (TLB_ERR_ARG), 16-byte aligned.  The
 * slot of a resampled stream holds the need source frames of that frame at its start (interleaved L R for two channels); nothing behind them
 * is read.  The output slot is what tlb_ingest_device / _valid take: 1152 sample frames at the encoder's rate.  A stream without a source has
 * its slot copied as it is: 2304 values, or the first 1152 of a one-channel stream (behind a one-channel stream's 1152 values nothing is written).
 * The (frame, stream) slots of a call are independent units: slot f takes its T - 1 frames of history from the tail of slot f - 1's source
 * frames in the same buffer, the call's first slot from the stream's state record, the last slot writes the record, and a slot's phase
 * follows from the stream's frame counter plus f: the output does not depend on how a stream's frames are cut into calls.
 * STATE per stream: T - 1 source frames and the frame position within the need cycle, on the device, allocated by the first
 * tlb_resample_set_source of a batch -- a batch that never sets a source allocates nothing and makes the device calls it made before.  The host
 * keeps its own copy of the position (advanced per call, cleared by the resets): tlb_resample_need never touches the device.
 *   tlb_resample_set_source(b, stream, rate)  stream = -1: every stream; rate 0 or the stream's own encoder rate: off.  Waits for the queued
 *                                 launches and zeroes the resampler state of the streams it names; the encoder is left alone.  An illegal
 *                                 pair for any named stream: TLB_ERR_SAMPLERATE, nothing changed.  A stream that has a tlb_decimate_* down
 *                                 source: TLB_ERR_ARG, nothing changed (a stream has one source).
 *   tlb_resample_source           the stream's source rate; 0: off
 *   tlb_resample_need(b, s, ahead) source frames the stream's (ahead)-th next frame consumes (ahead = 0: the next one); 1152 for a stream
 *                                 without a source; < 0: -TLB_ERR_ARG
 *   tlb_resample_need_at          need(frame) from the rates alone, no batch, no GPU; < 0: -TLB_ERR_*
 *   tlb_resample_taps             the committed table [L][T] and its L, M, T (each may be NULL); NULL: no such pair
 * tlb_reset, tlb_stream_reset and tlb_stream_finish zero the resampler state of the streams they touch.  tlb_stream_reconfigure keeps the
 * source rate when the new encoder rate still forms a legal pair with it; otherwise it refuses with TLB_ERR_SAMPLERATE and changes nothing.
 * Asynchronous on `hip_stream`; calls of one batch must be ordered on one stream, like the encode calls.
 * TICK PLANE.  tlb_tick_set_source(t, stream, rate) is legal while no tick is in flight (TLB_ERR_ARG otherwise).  While at least one stream
 * has a source (when the last one is turned off again the object is back to what it queued before; its extra buffer stays), every submit queues the resampler on the group's run stream behind the copy-in and ahead of the ingest, into one more device buffer
 * per group; an object that never sets one queues exactly what it queued before.  The copy-in still moves whole slots.  tlb_tick_need(t,
 * stream) is the number of source frames the stream's slot in the CURRENT input set (tlb_tick_pcm) must hold for the next submit; it follows
 * the host copy of the position, advanced at submit and reset by tlb_tick_stream_reset / _finish / _reconfigure; < 0: -TLB_ERR_ARG.
 * SHORT READS and a source on the same tick or node object are refused (TLB_ERR_ARG), from either side and in either order: the stretch
 * counts encoder-rate frames, and a source that delivers too few frames would need a second convention.  At the batch level the two compose
 * by the caller's own ordering.
 * NODE LEVEL.  tlb_node_set_source routes to the owning shard (stream = -1: every stream; between steps only; every pair is checked before a
 * shard is changed, and after a device failure half way the shards already changed get back the sources they had) and is remembered:
 * tlb_node_shard_restart sets the block's sources again, with fresh state (its streams start at need(0)).  tlb_node_need is the TICK plane's;
 * a BATCH-plane node refuses it (-TLB_ERR_ARG): there the caller goes through tlb_node_batch() and tlb_resample_need.  A stream of a broken
 * or late shard answers -TLB_ERR_HIP / -TLB_ERR_LATE.
 * ------------------------------------------------------------------------------------------ */
#define TLB_RESAMPLE_TAPS 32
int tlb_resample_set_source(tlb_batch *b, int stream, long source_rate);
long tlb_resample_source(const tlb_batch *b, int stream);
int tlb_resample_need(const tlb_batch *b, int stream, int ahead);
int tlb_resample_need_at(long source_rate, long encoder_rate, long frame);
const int16_t *tlb_resample_taps(long source_rate, long encoder_rate, int *L, int *M, int *T);
int tlb_resample_device(tlb_batch *b, const int16_t *d_source, int nframes, int16_t *d_interleaved, void *hip_stream);
int tlb_resample_host(tlb_batch *b, const int16_t *source, int nframes, int16_t *interleaved);
int tlb_tick_set_source(tlb_tick *t, int stream, long source_rate);
int tlb_tick_need(const tlb_tick *t, int stream);
int tlb_node_set_source(tlb_node *nd, int stream, long source_rate);
int tlb_node_need(const tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * Down sources: 48, 44.1 and 32 kHz sources for a 24 kHz encoder, low-pass filtered and decimated on the device, ahead of the ingest.
 * Half-rate services usually get studio audio at 48 kHz; the reference's inputs convert it before AudioEnc::run() sees a sample
 * (src/VLCInput.cpp:208, src/GSTInput.cpp:124-133).  Per TICK a 48 kHz source moves twice the PCM of the service; per SECOND it does not: a
 * 24 kHz frame lasts 48 ms, so 9216 bytes per 48 ms are the 4608 bytes per 24 ms every 48 kHz service moves.  A family of its own beside
 * tlb_resample_* (which is unchanged): wider slots, regular frames, 64 taps.  Defined in integers, as the resampler is.
 *   source rate -> encoder rate     ratio L/M
 *   48000 -> 24000                  1/2
 *   32000 -> 24000                  3/4
 *   44100 -> 24000                  80/147
 * Any other pair is TLB_ERR_SAMPLERATE.
 * THE TAPS.  One table per ratio, int16 H[L][T], T = TLB_DECIMATE_TAPS = 64, committed as csrc/tl_decimate_taps.inc: the committed table is
 * the definition, tools/gen_decimate_taps.py the record of how it was made (the resampler's recipe with the cutoff on the OUTPUT side:
 * N = L T; c = k - (N - 1) / 2; fc = 0.95 * 0.5 / M; h[k] = L 2 fc sinc(2 fc c) kaiser(N, 8)[k]; row p = h[p::L] scaled to sum 32768, rounded
 * half up, the remainder added to the row's tap of largest magnitude).  Every row sums to exactly 32768.  From the table: within +- 0.01 dB up
 * to 0.8 x the output's Nyquist frequency, - 75.7 / - 78.6 / - 85.7 dB (1/2, 3/4, 80/147) from 1.2 x upwards (32 taps would give - 40 dB).
 * THE FORMULA.  For a stream, count output samples n and source frames from the stream's last reset; a source frame is an L/R pair, or one
 * sample of a one-channel stream.  With q(n) = floor((n M + M - 1) / L) and p(n) = (n M + M - 1) mod L:
 *   acc(n) = sum over t = 0..T-1 of H[p(n)][t] * x[q(n) - t]      (x[j] = 0 for j < 0; the exact integer sum)
 *   y(n)   = clamp((acc(n) + 16384) >> 15, -32768, 32767)         (arithmetic shift, i.e. floor)
 * per channel, both channels with the same q and p.  The offset M - 1 makes the frames regular: frame f of the stream is
 * y(1152 f .. 1152 f + 1151) and consumes the source frames [S(f), S(f + 1)), S(f) = ceil(1152 f M / L), f = 0 included:
 *   need(f) = S(f + 1) - S(f)
 * 1/2: always 2304; 3/4: always 1536; 80/147: 2117, 2117, 2117, 2117, 2116 in a cycle of five frames that add up to 10 584.  Never above
 * 2304 frames: a WIDE slot of TLB_DECIMATE_SLOT = 4608 values holds it.
 * BUFFERS.  d_wide is int16 [nframes][nstreams][4608], d_interleaved int16 [nframes][nstreams][2304]; both 16-byte aligned, and they must
 * not overlap (TLB_ERR_ARG).  The wide slot of a stream with a down source holds the need source frames of that frame at its start
 * (interleaved L R for two channels); nothing behind them is read.  Its output slot is what tlb_ingest_device takes: 1152 sample frames at
 * 24 kHz, interleaved L R, or 1152 samples of a one-channel stream with nothing written behind them.  The slots of a stream WITHOUT a down
 * source are left alone, both of them: not read, not written -- its PCM is the caller's to put into d_interleaved.
 * The (frame, stream) slots of a call are independent units, as the resampler's are: slot f takes its T - 1 frames of history from the tail of
 * slot f - 1 in the same buffer, the call's first slot from the stream's state record, the last slot writes the record: the output does not
 * depend on how a stream's frames are cut into calls.
 * STATE per stream: T - 1 source frames and the frame position within the need cycle, on the device, allocated by the first real
 * tlb_decimate_set_source of a batch -- a batch that never sets one allocates nothing and queues nothing (tlb_decimate_device then returns
 * after its argument checks).  The host keeps its own copy of the position: tlb_decimate_need never touches the device.
 *   tlb_decimate_set_source(b, stream, rate)  stream = -1: every stream; rate 0 or the stream's own encoder rate: off.  Waits for the queued
 *                                 launches and zeroes the decimator state of the streams it names; the encoder is left alone.  An illegal
 *                                 pair for any named stream: TLB_ERR_SAMPLERATE, nothing changed.  A stream that has a tlb_resample_* source:
 *                                 TLB_ERR_ARG, nothing changed (a stream has one source).
 *   tlb_decimate_source           the stream's down source rate; 0: off
 *   tlb_decimate_need(b, s, ahead) source frames the stream's (ahead)-th next frame consumes; 1152 for a stream without a down source;
 *                                 < 0: -TLB_ERR_ARG
 *   tlb_decimate_need_at          need(frame) from the rates alone, no batch, no GPU; < 0: -TLB_ERR_*
 *   tlb_decimate_taps             the committed table [L][T] and its L, M, T (each may be NULL); NULL: no such pair
 * tlb_reset, tlb_stream_reset and tlb_stream_finish zero the decimator state of the streams they touch.  tlb_stream_reconfigure keeps the
 * source rate when the new encoder rate still forms a legal pair with it; otherwise it refuses with TLB_ERR_SAMPLERATE and changes nothing.
 * Asynchronous on `hip_stream`; calls of one batch must be ordered on one stream.  With feeds and short reads the batch level composes by the
 * caller's own ordering, as the resampler does.
 * TICK PLANE.  tlb_tick_set_down_source(t, stream, rate) is legal while no tick is in flight (TLB_ERR_ARG otherwise).  The first real down
 * source gives the object its wide buffers: pinned ones that travel with the two input sets, one device buffer per group.  tlb_tick_down(t,
 * stream) is the stream's wide slot (4608 values) in the CURRENT input set, NULL with two ticks in flight or while no stream has a down source;
 * tlb_tick_down_need(t, stream) the source frames it must hold for the next submit.  While at least one stream has a down source every submit
 * copies in the group's PCM (unless EVERY stream of the group has a down source) and the group's wide slice, and queues the decimator on the
 * run stream ahead of the ingest, writing the streams' slots of the group's PCM buffer; an object that never sets one queues exactly what it
 * queued before.  Down sources, sources (tlb_tick_set_source), feeds and short reads exclude one another on one tick or node object
 * (TLB_ERR_ARG), from either side and in either order.
 * NODE LEVEL.  tlb_node_set_down_source / tlb_node_down / tlb_node_down_need route to the owning shard as tlb_node_set_source / tlb_node_need
 * do, with the same rules: every pair is checked before a shard is changed, a change made before a device failure half way is rolled back,
 * the source is remembered for tlb_node_shard_restart (fresh state) and forgotten by a tlb_node_stream_reconfigure it no longer pairs with;
 * a stream of a broken or late shard answers NULL, -TLB_ERR_HIP or -TLB_ERR_LATE.
 * NOT BUILT: a channel map for PCM sources (the host's (L + R + 1) >> 1 is cheap, the filter is not); 48 -> 44.1 / 32 kHz; encoder rates
 * other than 24 kHz.  (48, 44.1 and 32 kHz FEEDS for 24 kHz services: "Down feeds" below, tlb_feed_down_*.)
 * ------------------------------------------------------------------------------------------ */
#define TLB_DECIMATE_TAPS 64
#define TLB_DECIMATE_SLOT 4608
int tlb_decimate_set_source(tlb_batch *b, int stream, long source_rate);
long tlb_decimate_source(const tlb_batch *b, int stream);
int tlb_decimate_need(const tlb_batch *b, int stream, int ahead);
int tlb_decimate_need_at(long source_rate, long encoder_rate, long frame);
const int16_t *tlb_decimate_taps(long source_rate, long encoder_rate, int *L, int *M, int *T);
int tlb_decimate_device(tlb_batch *b, const int16_t *d_wide, int nframes, int16_t *d_interleaved, void *hip_stream);
int tlb_decimate_host(tlb_batch *b, const int16_t *wide, int nframes, int16_t *interleaved);
int tlb_tick_set_down_source(tlb_tick *t, int stream, long source_rate);
int16_t *tlb_tick_down(tlb_tick *t, int stream);
int tlb_tick_down_need(const tlb_tick *t, int stream);
int tlb_node_set_down_source(tlb_node *nd, int stream, long source_rate);
int16_t *tlb_node_down(tlb_node *nd, int stream);
int tlb_node_down_need(const tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * Layer II feeds: a stream's source arrives as MP2 frames SOMEBODY ELSE encoded and is decoded on the device, ahead of the ingest.
 * Every entry point above takes PCM, 4608 bytes per stream and frame over the host-to-device link.  The reference's users need not: its
 * VLC and GStreamer inputs take a compressed feed and decode it before AudioEnc::run() sees a sample (src/VLCInput.cpp, src/GSTInput.cpp),
 * and MPEG Layer II is what studio links, satellite feeds and re-multiplexed services carry.  A 192 kbps feed frame is 576 bytes.
 * A FEED is a per-stream configuration of its own -- sample rate, bitrate, channels (1 | 2) -- and tlb_feed_*() decodes a feed frame into
 * the stream's slot of tlb_ingest_device's input, with the parser, requantiser and fp64 synthesis filterbank of tlb_decode_*() above.
 * tlb_feed_set, tlb_tick_set_feed and tlb_node_set_feed take a feed whose samplerate is the stream's and whose channels are the stream's
 * channel count (else TLB_ERR_SAMPLERATE / TLB_ERR_MODE).  The bitrate is the feed's own.
 * ADAPTED FEEDS.  A feed is ADAPTED when it is set through tlb_feed_set_adapted(b, stream, cfg) (tlb_tick_set_feed_adapted,
 * tlb_node_set_feed_adapted) and cfg does not match every named stream; a cfg that does is the strict feed above, with the same device
 * calls.  Legal pairs (feed rate Fs, stream rate Es): Fs = Es (ratio 1/1) and the four pairs of the resampler, 44100 -> 48000, 22050 ->
 * 24000 (L/M = 160/147), 32000 -> 48000, 16000 -> 24000 (3/2); anything else is TLB_ERR_SAMPLERATE.  Channels may be 1 or 2 on either
 * side.  Bitrate and configuration legality are tlb_feed_check_config's.
 * SCHEDULE.  A feed frame is 1152 source frames, a tick consumes 1058 / 1059 (160/147) or 768 (3/2) of them, so a frame is not wanted on
 * every tick.  With q(n) = floor(n M / L) and ticks f counted from the stream's last reset:
 *   S(f) = f > 0 ? q(1152 f - 1) + 1 : 0     source frames consumed before tick f (S(f + 1) - S(f) is tlb_resample_need_at)
 *   K(f) = ceil(S(f + 1) / 1152), K(-1) = 0  feed frames that must have arrived by tick f
 *   want(f) = K(f) - K(f - 1)                0 or 1, never 0 on two consecutive ticks
 * 160/147: 147 of every 160 ticks are wanted, the first unwanted ones are 12, 24, 36, 49; 3/2: ticks 2, 5, 8, ... are unwanted; 1/1: every
 * tick is wanted.  Before any tick at most 1145 (160/147) or 768 (3/2) decoded source frames are unconsumed.
 * AUDIO.  d_k: the 1152 sample frames tlb_feed_* defines for the stream's k-th WANTED slot under the feed's configuration (an empty or
 * not passing slot gives zeros, the synthesis history runs over consecutive wanted slots, a bad or empty slot is silence for its successor).
 * Channel map, on the decoded int16: a two-channel feed for a one-channel stream is x = (L + R + 1) >> 1 (arithmetic shift), applied
 * BEFORE the resampler; a one-channel feed for a two-channel stream is resampled once and the output written to both channels.  y(n) is
 * the resampler's formula above over x = d_0 d_1 ... (for 1/1, y = x), and tick f's ingest slot gets y(1152 f .. 1152 f + 1151),
 * interleaved as the ingest reads it; nothing is written behind it.  The output does not depend on how a stream's ticks are cut into calls.
 * A slot on an UNWANTED tick is not read and its bytes do not enter the feed history: its report is TLB_DEC_EMPTY, and TLB_DEC_EMPTY |
 * TLB_DEC_UNWANTED when its length was > 0 (the caller broke the schedule); the tick's PCM is produced from the queue either way.
 * tlb_feed_reset, tlb_reset, tlb_stream_reset and tlb_stream_finish zero the position and the queue of the streams they touch: the next
 * tick is tick 0.  tlb_stream_reconfigure keeps an adapted feed when (Fs, new Es) is still a legal pair, whatever the channel counts,
 * with fresh state, and removes it otherwise.  The stream's own tlb_resample_* state is a separate object and is not touched.
 *   tlb_feed_set_adapted(b, stream, cfg)  stream = -1: all; cfg NULL: as tlb_feed_set(.., NULL); every named stream is checked before
 *                                 anything changes.  The first adapted feed allocates the queue state (about 9.5 KB per stream of the
 *                                 batch) and a source plane (4.6 KB per stream and tick of the longest call): a batch that never sets one
 *                                 allocates nothing new and queues the device calls it queued before.
 *   tlb_feed_adapted(b, stream)   1 / 0; < 0: -TLB_ERR_ARG
 *   tlb_feed_want(b, stream, ahead)  1 / 0 for the stream's (ahead)-th next tick, from the host's own copy of the position (advanced by
 *                                 every tlb_feed_device call, cleared by the resets; no device access, like tlb_resample_need); 1 for a
 *                                 strict feed; < 0: -TLB_ERR_ARG (also: the stream has no feed)
 *   tlb_feed_want_at(Fs, Es, tick)  host only, no batch, no GPU; < 0: -TLB_ERR_SAMPLERATE (no legal pair), -TLB_ERR_ARG (tick < 0)
 * tlb_feed_device / _host, tlb_feed_stride, tlb_feed_get and the tick and node buffers and reports are the same for both kinds, and a
 * batch may hold strict feeds, adapted feeds and streams without a feed together: the strict launch runs first where a stream has a
 * strict feed, then one sequence of three kernels (decode, resample, carry) per call, however many ticks it holds, with no host
 * synchronisation inside a call.  A call over a batch with adapted feeds holds at most 8192 ticks (TLB_ERR_ARG beyond).
 * NOT BUILT: 48 -> 44.1 / 32 kHz, 24 kHz feeds for 48 kHz services and a channel map for PCM sources.  A 48, 44.1 or 32 kHz feed for a
 * 24 kHz service is a family of its own, "Down feeds" below (tlb_feed_down_*): tlb_feed_want_at answers -TLB_ERR_SAMPLERATE for those pairs.
 *   d_frames      uint8 [nframes][nstreams][tlb_feed_stride()]
 *   d_len         int32 [nframes][nstreams], required; 0 (or less) = an empty slot
 *   d_interleaved int16 [nframes][nstreams][2304], tlb_ingest_device's input: a fed stream's slot gets 1152 sample frames, L R L R for two
 *                 channels, 1152 samples at the slot's start for one (nothing is written behind them).  THE SLOT OF A STREAM WITHOUT A
 *                 FEED IS NOT TOUCHED: a mixed batch fills those with PCM as before, in any order with this call.
 *   d_report      tlb_frame_report [nframes][nstreams] or NULL; the slot of a stream without a feed has status TLB_DEC_EMPTY
 * HEADER RULES for a feed frame (a frame "passes" as above: no TLB_DEC_BAD_MASK flag, not EMPTY):
 *   - sync, ID, layer, bitrate index and sampling-frequency index must be the feed's configuration's (BAD_SYNC, HEADER_MISMATCH);
 *   - the protection bit is read per frame: with a CRC-16 the fields start at bit 48 and the CRC is verified (BAD_CRC16), without one
 *     they start at bit 32 and crc_stored = crc_computed = 0;
 *   - private, copyright, original and emphasis bits are ignored;
 *   - the mode is the frame's: a two-channel feed accepts stereo, joint stereo with any bound and dual channel, a one-channel feed mono
 *     only; anything else is HEADER_MISMATCH;
 *   - the padding bit is honoured where the rate has padding slots (44.1 / 22.05 kHz; set elsewhere: HEADER_MISMATCH).  A slot longer
 *     than its frame is a HEADER_MISMATCH, a shorter one OVERRUN, as are fields that need more bits than the frame has;
 *   - no ScF-CRC is looked for: BAD_SCFCRC and SCFCRC_UNCHECKED are never set.  What follows the samples is ancillary data.
 * No read leaves the slot whatever its bytes say.  Rounding and saturation are tlb_decode_*()'s.  A frame that did not pass, or an empty
 * slot, yields 1152 zeros per channel and counts as silence in its successor's filter history.  The output does not depend on how a
 * stream's frames are cut into calls: a call leaves each fed stream's last slot -- bytes, length, status -- behind for the next, in arrays
 * of its own (not the decoder's), allocated by the first tlb_feed_set: a batch that never sets a feed allocates nothing and makes exactly
 * the device calls it made before.
 *   tlb_feed_check_config(cfg)    host only, no GPU: TLB_OK / TLB_ERR_SAMPLERATE / TLB_ERR_BITRATE / TLB_ERR_MODE (channels not 1 | 2).
 *                                 The bitrate must be one the rate's table has: every combination the encoder itself accepts for 'm'
 *                                 (one channel) or 's' / 'j' / 'd' (two).  THE STANDARD'S MPEG-1 LIMITS BETWEEN MODE AND BITRATE ARE NOT
 *                                 ENFORCED (32, 48, 56, 80 kbps are accepted for two channels, 224 kbps and more for one): the encoder
 *                                 does not enforce them either, and a frame it made at such a cell must be acceptable as a feed.
 *   tlb_feed_frame_bytes(cfg)     host only: the frame's length without a padding slot; < 0: -TLB_ERR_*
 *   tlb_feed_set(b, stream, cfg)  stream = -1: every stream; cfg = NULL: the feed is removed (the stream is back to PCM input).  Legal between
 *                                 launches (it waits for the queued ones), resets the feed history of the streams it names.  Every named
 *                                 stream is checked before anything changes.
 *   tlb_feed_get(b, stream, cfg)  1 and *cfg (may be NULL) when the stream has a feed, 0 when not; < 0: -TLB_ERR_ARG
 *   tlb_feed_stride(b)            the longest feed frame over the batch, with its padding slot where the rate has one, rounded up to 4;
 *                                 0: no stream has a feed.  It changes with tlb_feed_set: ask again after every set.
 *   tlb_feed_reset(b, stream)     the stream's next feed frame is decoded as after silence (stream = -1: all); tlb_reset, tlb_stream_reset,
 *                                 tlb_stream_finish and tlb_stream_reconfigure do the same for the streams they touch.
 * tlb_stream_reconfigure to a sample rate or channel count the stream's feed no longer fits REMOVES the feed (the call itself succeeds):
 * set a new one afterwards.
 * Asynchronous on `hip_stream`; feed calls of one batch must be ordered on one stream, ahead of the ingest that reads their output.  Every
 * buffer must be 4-byte aligned, as for tlb_decode_device.  Argument errors -- a NULL batch, frames, lengths or PCM pointer, nframes <= 0,
 * a misaligned pointer, no stream with a feed -- return TLB_ERR_ARG and change nothing.  tlb_feed_host takes host buffers; its
 * `interleaved` is read and written (the slots the kernel does not write come back as they went in).
 * One wavefront per (stream, frame) with a feed.
 * TICK PLANE.  tlb_tick_set_feed(t, stream, cfg) is legal while no tick is in flight (TLB_ERR_ARG otherwise; stream = -1: every stream,
 * cfg = NULL: removed; every named stream is checked before one is changed).  While at least one stream has a feed, every submit queues
 * the copy-in of the feed bytes and lengths, then the feed kernel, then the ingest, on the tick's existing streams and events; an object that
 * never sets one queues exactly what it queued before.  A GROUP ALL OF WHOSE STREAMS HAVE FEEDS SKIPS ITS PCM COPY-IN -- 576 + 4 bytes
 * per stream and tick at 192 kbps instead of 4608 --; a mixed group copies its PCM as before and the feed kernel then overwrites the fed
 * streams' slots; a group without a fed stream queues nothing new.  (The groups are the contiguous stream ranges of tlb_tick_config.ngroups.)
 *   tlb_tick_feed_stride(t)  bytes per slot of tlb_tick_feed(): the widest feed the object has had, rounded as tlb_feed_stride (it only
 *                            grows); 0 while no stream has a feed
 *   tlb_tick_feed(t)         uint8 [nstreams][tlb_tick_feed_stride()], tlb_tick_feed_len(t) int32 [nstreams]: pinned input buffers that
 *                            alternate with the input sets of tlb_tick_pcm().  RE-FETCH them after every submit and after every
 *                            tlb_tick_set_feed (a wider feed replaces the frame buffers).  NULL while two ticks are in flight and
 *                            while no stream has a feed.  A set of lengths is all 0 (empty slots) whenever the caller sees it untouched.
 *   tlb_tick_feed_report(t)  tlb_frame_report [nstreams] of the tick waited for last (it comes back with the silence counter); a stream
 *                            without a feed reads TLB_DEC_EMPTY; NULL while no stream has a feed
 * On one tick object feeds exclude SHORT READS and exclude SOURCE RATES (TLB_ERR_ARG, from either side and in either order): a feed
 * frame is always 1152 sample frames at the stream's own rate.  Feeds compose with the monitor and the compare monitor, which see the
 * planar PCM behind the ingest.  The stream life-cycle calls reset the feed history of the stream they touch;
 * tlb_tick_stream_reconfigure removes a feed that no longer fits, as above.
 * tlb_tick_set_feed is all or nothing for the feeds: after a device failure half way the groups already changed get back the feeds they
 * had (with fresh history); buffers that were widened for the call stay.  After tlb_tick_finish, which runs no feed kernel,
 * tlb_tick_feed_report shows the last tick's reports once more.
 * tlb_tick_set_feed_adapted(t, stream, cfg) is tlb_tick_set_feed for an adapted feed: the same conditions (no tick in flight), the same
 * exclusions (short reads, source rates, from either side), the same all-or-nothing rule, the same buffers and reports; a group all of
 * whose streams are fed still skips its PCM copy-in, and the monitor and the compare monitor compose with it unchanged.
 *   tlb_tick_feed_want(t, stream)  1 / 0: does the stream's slot of the input set to fill next want a frame (1 for a strict feed); the
 *                            position advances with every submit; < 0: -TLB_ERR_ARG (also: the stream has no feed)
 * NODE LEVEL.  tlb_node_set_feed routes to the owning shard (stream = -1: every stream; between steps only, TLB_ERR_ARG otherwise; every
 * named stream is checked before a shard is changed; a broken shard answers TLB_ERR_HIP, a late one TLB_ERR_LATE; after a device failure
 * half way the shards already changed get back the feeds they had) and is remembered: tlb_node_shard_restart sets the block's feeds again,
 * with fresh history, and tlb_node_stream_reconfigure forgets a feed that no longer fits.  On a TICK-plane node feeds exclude short reads
 * and source rates as on a tick object; on a BATCH-plane node the call is tlb_feed_set of the shard's batch and the caller decodes through
 * tlb_node_batch() and tlb_feed_device.  TICK plane only: tlb_node_feed(nd, stream) and tlb_node_feed_len(nd, stream) point at the STREAM'S
 * slot and length in its shard's current input set (tlb_node_feed_stride(nd, stream) bytes of room: shards differ), RE-FETCHED like
 * tlb_node_pcm; NULL for a broken or late shard, while two ticks are in flight and while no stream of the shard has a feed.
 * tlb_node_feed_report(nd, stream) is the stream's report of the step waited for last; NULL for a broken, late or stale shard and while no
 * stream of the shard has a feed.
 * tlb_node_set_feed_adapted is tlb_node_set_feed for an adapted feed, remembered as such: tlb_node_shard_restart sets the block's adapted
 * feeds again at tick 0 and tlb_node_stream_reconfigure forgets one whose rates no longer form a legal pair.  tlb_node_feed_want(nd, stream)
 * is tlb_tick_feed_want of the stream's shard (TICK plane; a broken or late shard answers as tlb_node_need does; a BATCH-plane node
 * answers -TLB_ERR_ARG: ask the shard's batch with tlb_feed_want).
 * ------------------------------------------------------------------------------------------ */
typedef struct { long samplerate; int bitrate; int channels; } tlb_feed_config;   /* channels 1 | 2 */
int tlb_feed_check_config(const tlb_feed_config *cfg);
int tlb_feed_frame_bytes(const tlb_feed_config *cfg);
int tlb_feed_set(tlb_batch *b, int stream, const tlb_feed_config *cfg);
int tlb_feed_get(const tlb_batch *b, int stream, tlb_feed_config *cfg);
int tlb_feed_stride(const tlb_batch *b);
int tlb_feed_reset(tlb_batch *b, int stream);
int tlb_feed_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int nframes, int16_t *d_interleaved, tlb_frame_report *d_report,
                    void *hip_stream);
int tlb_feed_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int nframes, int16_t *interleaved, tlb_frame_report *report);
int tlb_feed_set_adapted(tlb_batch *b, int stream, const tlb_feed_config *cfg);
int tlb_feed_adapted(const tlb_batch *b, int stream);
int tlb_feed_want(const tlb_batch *b, int stream, int ahead);
int tlb_feed_want_at(long feed_rate, long stream_rate, long tick);
int tlb_tick_set_feed_adapted(tlb_tick *t, int stream, const tlb_feed_config *cfg);
int tlb_tick_feed_want(const tlb_tick *t, int stream);
int tlb_node_set_feed_adapted(tlb_node *nd, int stream, const tlb_feed_config *cfg);
int tlb_node_feed_want(const tlb_node *nd, int stream);
int tlb_node_set_feed(tlb_node *nd, int stream, const tlb_feed_config *cfg);
uint8_t *tlb_node_feed(tlb_node *nd, int stream);
int32_t *tlb_node_feed_len(tlb_node *nd, int stream);
int tlb_node_feed_stride(const tlb_node *nd, int stream);
const tlb_frame_report *tlb_node_feed_report(const tlb_node *nd, int stream);
int tlb_tick_set_feed(tlb_tick *t, int stream, const tlb_feed_config *cfg);
int tlb_tick_feed_stride(const tlb_tick *t);
uint8_t *tlb_tick_feed(tlb_tick *t);
int32_t *tlb_tick_feed_len(tlb_tick *t);
const tlb_frame_report *tlb_tick_feed_report(const tlb_tick *t);

/* ---------------------------------------------------------------------------------------------
 * Down feeds: 48, 44.1 and 32 kHz Layer II feeds for 24 kHz services, decoded AND decimated on the device, ahead of the ingest.
 * Half-rate services get their contribution as 48 kHz MPEG Layer II over studio links and satellite; the reference's inputs decode and
 * convert it in one chain (src/VLCInput.cpp, src/GSTInput.cpp: decode, samplerate=, channels=).  As wide PCM through
 * tlb_tick_set_down_source such a stream costs 9216 bytes per tick on the link, as two 192 kbps feed frames 1152 + 8.  A family of its own
 * beside tlb_feed_* (unchanged, in behaviour and in code objects: tlb_feed_want is 0 or 1 with one slot per tick), the way tlb_decimate_*
 * stands beside tlb_resample_*.  The decode is tlb_feed_*'s, the filter tlb_decimate_*'s; what is new is the schedule with up to TWO feed
 * frames per tick and the queue between decoder and decimator.
 * LEGAL PAIRS (feed rate Fs, stream rate Es): the decimator's three, 48000 -> 24000 (L/M = 1/2), 32000 -> 24000 (3/4), 44100 -> 24000
 * (80/147); anything else is TLB_ERR_SAMPLERATE.  Channels may be 1 or 2 on either side.  Bitrate and legality are tlb_feed_check_config's.
 * SCHEDULE.  Ticks f are counted from the stream's last reset, in the decimator's own terms:
 *   S(f) = ceil(1152 f M / L)                 source frames consumed before tick f; S(f + 1) - S(f) is tlb_decimate_need_at
 *   K(f) = ceil(S(f + 1) / 1152), K(-1) = 0   feed frames that must have arrived by tick f
 *   want(f) = K(f) - K(f - 1)                 1 or 2
 * 1/2: 2 on every tick, nothing is left over; 3/4: 2, 1, 1, 2, 1, 1, ... (3 ticks = 4 feed frames), at most 768 decoded source frames are
 * unconsumed before a tick; 80/147: one frame on 13 of every 80 ticks -- the first are 6, 12, 18, 24, 30, 36, 43, 49 --, two otherwise (80
 * ticks = 147 feed frames), at most 1137 unconsumed.  A stream's position is its tick counter modulo that period (1, 3, 80), kept on the
 * device and, as a copy, on the host; with it all arithmetic is 32-bit.
 * SLOTS.  A tick has TWO slots per stream, [.][s][0] and [.][s][1].  On a tick with want = 1 slot 1 is not read and its bytes do not enter
 * the history: its report is TLB_DEC_EMPTY, and TLB_DEC_EMPTY | TLB_DEC_UNWANTED when its length was > 0.  Both slots of a stream without
 * a down feed report TLB_DEC_EMPTY.
 * AUDIO.  d_k: the 1152 sample frames tlb_feed_* defines for the stream's k-th WANTED frame under the feed's configuration (header rules,
 * rounding and saturation as there); an empty or not passing frame is zeros; the synthesis history runs over consecutive wanted frames; a
 * bad or empty frame is silence for its successor.  Channel map on the decoded int16, as for adapted feeds: two to one is (L + R + 1) >> 1,
 * applied BEFORE the filter; one to two is filtered once and written to both channels.  y(n) is tlb_decimate_*'s formula, unchanged (the
 * same q, p, table and rounding, 16-tap quarters summed in 32 bits and the quarters in 64), over x = d_0 d_1 ...; tick f's ingest slot gets
 * y(1152 f .. 1152 f + 1151), interleaved as the ingest reads it; nothing is written behind it.  The output does not depend on how a
 * stream's ticks are cut into calls.
 *   d_frames      uint8 [nframes][nstreams][2][tlb_feed_down_stride()]
 *   d_len         int32 [nframes][nstreams][2], required; 0 (or less) = an empty slot
 *   d_interleaved int16 [nframes][nstreams][2304], tlb_ingest_device's input.  THE SLOT OF A STREAM WITHOUT A DOWN FEED IS NOT TOUCHED.
 *   d_report      tlb_frame_report [nframes][nstreams][2] or NULL
 *   tlb_feed_down_set(b, stream, cfg)  stream = -1: all; cfg = NULL: removed.  Every named stream is checked before anything changes.  It
 *                                 waits for the queued launches and zeroes the named streams' position, queue and history.  The first real
 *                                 one allocates (about 11.4 KB per stream of the batch: two copies of a queue head of 1200 source frames,
 *                                 one history slot of 1728 bytes) and a source plane (9.2 KB per stream and tick of the longest call): a
 *                                 batch that never sets one allocates nothing and queues exactly the device calls it queued before.
 *   tlb_feed_down_get(b, stream, cfg)  1 and *cfg (may be NULL) / 0; < 0: -TLB_ERR_ARG
 *   tlb_feed_down_want(b, stream, ahead)  1 or 2 for the stream's (ahead)-th next tick, from the host's copy of the position (advanced by
 *                                 every tlb_feed_down_device call, cleared by the resets; no device access); < 0: -TLB_ERR_ARG (also: the
 *                                 stream has no down feed)
 *   tlb_feed_down_want_at(Fs, Es, tick)  host only, no batch, no GPU; < 0: -TLB_ERR_SAMPLERATE (no legal pair), -TLB_ERR_ARG (tick < 0)
 *   tlb_feed_down_stride(b)       the longest down-feed frame of the batch with its padding slot, rounded up to 4; 0: there is none
 *   tlb_feed_down_reset(b, stream)  the stream's next tick is tick 0, after silence (stream = -1: all)
 * A STREAM HAS ONE SOURCE.  A down feed on a stream that has a feed (strict or adapted), a tlb_resample_* source or a tlb_decimate_*
 * source is TLB_ERR_ARG, and so is setting any of those on a stream that has a down feed; removing ("off") is always allowed.  A batch may
 * hold all four families on different streams: each call leaves the other families' slots alone.
 * tlb_reset, tlb_stream_reset and tlb_stream_finish zero the position, the queue and the history of the streams they touch.
 * tlb_stream_reconfigure keeps a down feed, with fresh state, while (Fs, new Es) is still a legal pair, whatever the channel counts, and
 * removes it otherwise (the call itself succeeds).
 * Three kernels per call (decode: one wavefront per tick, stream and slot; decimate: one workgroup per tick and stream; carry: one
 * wavefront per stream), however many ticks it holds, with no host synchronisation between them.  Asynchronous on `hip_stream`; calls of
 * one batch must be ordered on one stream, ahead of the ingest.  At most 8192 ticks per call; the argument-error rules are
 * tlb_feed_device's (a NULL batch, frames, lengths or PCM pointer, nframes <= 0, a misaligned pointer, no stream with a down feed:
 * TLB_ERR_ARG, nothing changed).  tlb_feed_down_host takes host buffers; its `interleaved` is read and written.
 * TICK PLANE.  tlb_tick_set_down_feed(t, stream, cfg) is legal while no tick is in flight, all or nothing as tlb_tick_set_feed is.
 * tlb_tick_down_feed(t) is uint8 [nstreams][2][tlb_tick_down_feed_stride()], tlb_tick_down_feed_len(t) int32 [nstreams][2],
 * tlb_tick_down_feed_report(t) tlb_frame_report [nstreams][2]; lifetime and re-fetch rules are tlb_tick_feed's (pinned, alternating with
 * the input sets, NULL while two ticks are in flight and while no stream has a down feed, lengths all 0 whenever the caller sees a set
 * untouched).  tlb_tick_down_feed_want(t, stream) is 1 or 2 for the input set to fill next.  While a stream has a down feed every submit
 * copies in the group's frames and lengths and queues the three kernels on the run stream ahead of the ingest, under the events that
 * order feeds; A GROUP ALL OF WHOSE STREAMS HAVE DOWN FEEDS SKIPS ITS PCM COPY-IN; an object that never sets one queues exactly what it
 * queued before.  On one tick or node object down feeds exclude feeds, sources, down sources and short reads (TLB_ERR_ARG from either
 * side, in either order).
 * NODE LEVEL.  tlb_node_set_down_feed routes to the owning shards as tlb_node_set_feed does (every named stream is checked before a shard
 * is changed, a change made before a device failure half way is rolled back) and is remembered: tlb_node_shard_restart sets the block's
 * down feeds again at tick 0, tlb_node_stream_reconfigure forgets one that no longer pairs.  tlb_node_down_feed / _len / _report point at
 * the STREAM's two slots, lengths and reports (tlb_node_down_feed_stride(nd, stream) bytes per slot), tlb_node_down_feed_want is
 * tlb_tick_down_feed_want of the stream's shard; broken, late and stale shards answer as for tlb_node_feed.  On a BATCH-plane node the
 * call is tlb_feed_down_set of the shard's batch and tlb_node_down_feed_want answers -TLB_ERR_ARG.
 * NOT BUILT: 48 -> 44.1 / 32 kHz, 24 kHz feeds for 48 kHz services, down feeds together with short reads, mixing down feeds with the other
 * source families on ONE tick or node object (batches may mix them).
 * ------------------------------------------------------------------------------------------ */
int tlb_feed_down_set(tlb_batch *b, int stream, const tlb_feed_config *cfg);
int tlb_feed_down_get(const tlb_batch *b, int stream, tlb_feed_config *cfg);
int tlb_feed_down_want(const tlb_batch *b, int stream, int ahead);
int tlb_feed_down_want_at(long feed_rate, long stream_rate, long tick);
int tlb_feed_down_stride(const tlb_batch *b);
int tlb_feed_down_reset(tlb_batch *b, int stream);
int tlb_feed_down_device(tlb_batch *b, const uint8_t *d_frames, const int32_t *d_len, int16_t *d_interleaved, tlb_frame_report *d_report, int nframes,
                         void *hip_stream);
int tlb_feed_down_host(tlb_batch *b, const uint8_t *frames, const int32_t *len, int16_t *interleaved, tlb_frame_report *report, int nframes);
int tlb_tick_set_down_feed(tlb_tick *t, int stream, const tlb_feed_config *cfg);
int tlb_tick_down_feed_stride(const tlb_tick *t);
uint8_t *tlb_tick_down_feed(tlb_tick *t);
int32_t *tlb_tick_down_feed_len(tlb_tick *t);
int tlb_tick_down_feed_want(const tlb_tick *t, int stream);
const tlb_frame_report *tlb_tick_down_feed_report(const tlb_tick *t);
int tlb_node_set_down_feed(tlb_node *nd, int stream, const tlb_feed_config *cfg);
int tlb_node_down_feed_stride(const tlb_node *nd, int stream);
uint8_t *tlb_node_down_feed(tlb_node *nd, int stream);
int32_t *tlb_node_down_feed_len(tlb_node *nd, int stream);
int tlb_node_down_feed_want(const tlb_node *nd, int stream);
const tlb_frame_report *tlb_node_down_feed_report(const tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * Programme loudness: momentary, short-term and gated programme ("integrated") loudness after ITU-R BS.1770-4 / EBU Tech 3341 of the PCM
 * the encoder is given -- the ingest's planar output, therefore AFTER the stream's gain (tlb_set_gain_db is the actuator, this the
 * measurement).  Opt-in; the meter lives on the device and reports ENERGIES as doubles: LUFS = -0.691 + 10 log10(E), tlb_loudness_lufs.
 * THE ARITHMETIC.  The reference has no loudness meter, so this is the definition (tests/loudnesslib.py restates it in numpy, every
 * comparison against it is bit for bit).  Every product and sum is its own rounded fp64 operation in the order written.
 *   sample      x = (double)s * (1.0 / 32768.0)
 *   K-weighting two biquads per channel in direct form I, t = ((b0*x) + (b1*x1)) + (b2*x2), y = (t - (a2*y2)) - (a1*y1); the second takes
 *               the first's y as its x; state x1 x2 y1 y2 per stage and channel, zero at start, carried from frame to frame.  One
 *               coefficient row per encoder rate (48, 44.1, 32, 24, 22.05, 16 kHz), committed as csrc/tl_loudness_tables.inc: the committed
 *               table is the definition, tools/gen_loudness_tables.py the record of how it was made (the bilinear forms of BS.1770-4's
 *               shelf and high-pass; at 48 kHz they are the coefficients the recommendation prints, to 1e-15)
 *   bins        acc_c = acc_c + (y*y) sample by sample; a bin is 100 ms = rate / 10 samples (a frame closes at most one); on close
 *               ms_c = acc_c / (double)binlen, z = ms_0 for a one-channel stream, ms_0 + ms_1 for a two-channel one (dual channel counts as
 *               two channels; channel weights 1), acc = 0, z into a ring of 30
 *   momentary   once 4 bins exist: m = (((z[-3] + z[-2]) + z[-1]) + z[0]) * 0.25        (400 ms)
 *   short-term  once 30 bins exist: the ring summed oldest to newest, / 30.0             (3 s)
 *               both are 0.0 before their bins exist; the maxima are plain > updates
 *   gating      every m is one gating block.  E(L) = 10^((L + 0.691) / 10); edges e_0 = E(-70.0), e_j = E(-70.05 + 0.1 j), centres
 *               c_j = E(-70.0 + 0.1 j), j up to 750, both in the committed table.  A block counts iff m > e_0, in the bin
 *               #{k in 1..750: m >= e_k}; per stream 751 uint32 counts
 *   programme   N = sum n_j, S = sum (double)n_j * c_j in ascending j; gate = 0.1 * (S / N); integrated = the same count-weighted mean over
 *               the bins with c_j >= gate; both 0.0 when N == 0.  The 0.1 LU quantisation is part of the definition (its error of at
 *               most 0.05 LU lies inside EBU Tech 3341's +-0.1 LU)
 * RECORDS.  tlb_loudness_record: frames = PCM frames measured, bins = closed bins, blocks = gating blocks formed, gated = blocks above
 * -70 LUFS (the histogram's total), then the four energies.  tlb_loudness_programme_record: gated = blocks at or above the relative gate.
 * STATE.  About 3.4 KB of device memory per stream (filter state, ring, record, 3008 bytes of histogram: about 450 MB at 131 072
 * streams), allocated by tlb_loudness_enable ALONE: a batch that never enables loudness allocates and queues nothing new, and the other
 * calls answer TLB_ERR_ARG on it.
 *   tlb_loudness_enable(b)            allocates the state (waits for the device once); a second call answers 0
 *   tlb_loudness_device(b, d_pcm_planar, nframes, d_records, stream)
 *                                     measures nframes of every stream, int16 [nframes][nstreams][2][1152] as tlb_ingest_device writes it
 *                                     (16-byte aligned; the second row of a one-channel stream is not looked at), and writes
 *                                     tlb_loudness_record [nstreams] (may be NULL) on hip_stream
 *   tlb_loudness_host                 the same with host buffers
 *   tlb_loudness_programme_device / _host     tlb_loudness_programme_record [nstreams] from the counts so far
 *   tlb_loudness_reset(b, stream)     -1: every stream.  Waits for the queued work, then zeroes filter state, bins, ring, maxima, counters
 *                                     and histogram: EBU mode's "reset"
 *   tlb_loudness_taps(rate, out[10])  b0 b1 b2 a1 a2 of the shelf, then of the high-pass; no GPU.  TLB_ERR_SAMPLERATE for any other rate
 *   tlb_loudness_scale(edges[751], centres[751])    the gating scale (each may be NULL); no GPU
 *   tlb_loudness_lufs(energy)         -0.691 + 10 log10(energy); -inf for 0
 * tlb_stream_reset and tlb_stream_reconfigure clear the stream's loudness state (the rate, and with it the coefficients and the bin length,
 * may have changed); tlb_stream_finish leaves it.
 * TICK PLANE.  tlb_tick_enable_loudness(t) before the first submit (TLB_ERR_ARG after it; a second call answers 0) enables the meter of
 * every group's batch.  Every submit then queues the meter on the tick's planar PCM on the run stream, behind the ingest and behind the
 * tick's encode and egress kernels; the 48-byte records travel with the three output sets behind the packets, on an event of their own: the
 * packets' copy-out does not wait for them.  tlb_tick_loudness(t) is tlb_loudness_record [nstreams] of the tick waited for last (pinned,
 * valid until the next wait); NULL when loudness is off.  The records count the PCM that went IN: after T waited ticks frames == T, and
 * tlb_tick_finish adds nothing (its set shows the last tick's records).  tlb_tick_loudness_programme(t, out [nstreams]) and
 * tlb_tick_loudness_reset(t, stream) (-1: all) are legal with no tick in flight (TLB_ERR_ARG otherwise, and when loudness is off).  An object
 * that never enables loudness allocates and queues nothing new.
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_loudness goes to every shard before the first submit, and a
 * shard made by tlb_node_shard_restart is enabled again -- its records start from zero.  tlb_node_loudness(nd, stream) points at the STREAM's
 * record and answers NULL for a broken, late or stale shard; tlb_node_loudness_programme(nd, out [nstreams]) fills the blocks of the live
 * shards between steps (all zero for the others); tlb_node_loudness_reset routes like the stream life-cycle calls (TLB_ERR_HIP for a stream
 * of a broken shard, TLB_ERR_LATE for one of a late shard), -1 goes to every live shard.
 * NOT BUILT: loudness of the decoded output (the monitors own that side; loudness range is tlb_lra_* below).  Acting on the gain: the caller's loop with
 * tlb_set_gain_db, and the true-peak limiter below (tlb_limiter_*) as the net under it.
 * ------------------------------------------------------------------------------------------ */
#define TLB_LOUDNESS_BINS 751
typedef struct { uint32_t frames, bins, blocks, gated;
                 double momentary, short_term, momentary_max, short_term_max; } tlb_loudness_record;      /* 48 bytes */
typedef struct { double integrated, gate; uint32_t gated, reserved; } tlb_loudness_programme_record;     /* 24 bytes */
int tlb_loudness_enable(tlb_batch *b);
int tlb_loudness_device(tlb_batch *b, const int16_t *d_pcm_planar, int nframes, tlb_loudness_record *d_records, void *hip_stream);
int tlb_loudness_host(tlb_batch *b, const int16_t *pcm_planar, int nframes, tlb_loudness_record *records);
int tlb_loudness_programme_device(tlb_batch *b, tlb_loudness_programme_record *d_out, void *hip_stream);
int tlb_loudness_programme_host(tlb_batch *b, tlb_loudness_programme_record *out);
int tlb_loudness_reset(tlb_batch *b, int stream);
int tlb_loudness_taps(long samplerate, double out[10]);
int tlb_loudness_scale(double edges[751], double centres[751]);
double tlb_loudness_lufs(double energy);
int tlb_tick_enable_loudness(tlb_tick *t);
const tlb_loudness_record *tlb_tick_loudness(const tlb_tick *t);
int tlb_tick_loudness_programme(tlb_tick *t, tlb_loudness_programme_record *out);
int tlb_tick_loudness_reset(tlb_tick *t, int stream);
int tlb_node_enable_loudness(tlb_node *nd);
const tlb_loudness_record *tlb_node_loudness(const tlb_node *nd, int stream);
int tlb_node_loudness_programme(tlb_node *nd, tlb_loudness_programme_record *out);
int tlb_node_loudness_reset(tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * Loudness range (LRA) after EBU Tech 3342: how far apart the quiet and the loud passages of a programme lie, from the distribution of the
 * SHORT-TERM values the loudness meter above forms.  With it the meter is an "EBU Mode" meter (EBU Tech 3341 section 2); it tells whether
 * a programme can be brought to target by a static gain (tlb_set_gain_db) or needs dynamics first.  Opt-in ON TOP of tlb_loudness_enable.
 * THE ARITHMETIC.  The reference has no such meter, so this is the definition (tests/lralib.py restates it in Python ints and numpy
 * float64, every comparison against it is bit for bit).
 *   range block every short-term value st the loudness meter forms is one range block: one per closed bin from bin 30 on, so 10 per
 *               second with 2.9 s of overlap (Tech 3342 asks for at least 2 s).  A block counts iff st > e_0, in the bin
 *               #{k in 1..750: st >= e_k} of a SECOND set of 751 uint32 counts per stream; edges e and centres c are the loudness
 *               meter's (tlb_loudness_scale)
 *   range       over the bins in ascending j: N = sum n_j, S = sum (double)n_j * c_j; gate = 0.01 * (S / N), one division and one
 *               multiplication by the literal, each rounded: -20 LU relative to the absolute-gated mean.  The distribution is the bins
 *               with c_j >= gate, N2 their total.  Nearest ranks in 64-bit integers: r_lo = (N2 + 4) / 10 and
 *               r_hi = (19 (N2 - 1) + 10) / 20, which are floor((N2 - 1) * 0.10 + 0.5) and floor((N2 - 1) * 0.95 + 0.5).  low_bin is the
 *               first gated bin whose cumulative count over the gated bins exceeds r_lo, high_bin likewise for r_hi; low = c[low_bin],
 *               high = c[high_bin]; LRA = 0.1 * (high_bin - low_bin) LU, an integer number of tenths because the centres are 0.1 LU
 *               apart.  Everything is 0 when N == 0.  The 0.1 LU quantisation is part of the definition: each percentile is at most
 *               0.05 LU off, and Tech 3342's tolerance is +-1 LU
 * RECORD.  tlb_lra_record, 40 bytes, little-endian, no padding: low, high, gate are energies (LUFS = tlb_loudness_lufs), blocks = N,
 * gated = N2, then the two bins.  tlb_lra_lu(rec) = 0.1 * (high_bin - low_bin) on the host, 0 for NULL.
 * STATE.  3008 bytes of device memory per stream (the second histogram) and the scratch of tlb_lra_host, allocated by tlb_lra_enable ALONE: a
 * batch that never enables it allocates and queues nothing new, and runs the kernels it always ran.
 *   tlb_lra_enable(b)                 after tlb_loudness_enable (TLB_ERR_ARG before it); allocates the counts (waits for the device
 *                                     once); a second call answers 0.  From this call on tlb_loudness_device / _host of the batch launch
 *                                     the counting twin of their kernel INSTEAD of it: their records and the programme histogram are bit for
 *                                     bit what they are without the range
 *   tlb_lra_device(b, d_out, stream)  tlb_lra_record [nstreams] from the counts so far, on hip_stream; d_out 8-byte aligned
 *   tlb_lra_host(b, out)              the same with a host buffer
 * There is no reset of its own: EBU Mode has one reset.  tlb_loudness_reset, tlb_stream_reset and tlb_stream_reconfigure zero the stream's
 * range counts with the rest of its loudness state; tlb_stream_finish leaves them.
 * TICK PLANE.  tlb_tick_enable_lra(t) after tlb_tick_enable_loudness and before the first submit (TLB_ERR_ARG otherwise; a second call
 * answers 0).  The tick's per-submit queue is unchanged: the meter's one launch is the other kernel.  tlb_tick_lra(t, out [nstreams]) is
 * legal with no tick in flight, like tlb_tick_loudness_programme.
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_lra after tlb_node_enable_loudness goes to every shard before
 * the first submit, and a shard made by tlb_node_shard_restart is enabled again -- its counts start from zero.  tlb_node_lra(nd, out
 * [nstreams]) fills the blocks of the live shards between steps (all zero for the others).
 * NOT BUILT: the range of the decoded output, a 1 Hz block rate.  Acting on the range stays the caller's policy.
 * ------------------------------------------------------------------------------------------ */
typedef struct { double low, high, gate; uint32_t blocks, gated; int32_t low_bin, high_bin; } tlb_lra_record;      /* 40 bytes */
int tlb_lra_enable(tlb_batch *b);
int tlb_lra_device(tlb_batch *b, tlb_lra_record *d_out, void *hip_stream);
int tlb_lra_host(tlb_batch *b, tlb_lra_record *out);
double tlb_lra_lu(const tlb_lra_record *rec);
int tlb_tick_enable_lra(tlb_tick *t);
int tlb_tick_lra(tlb_tick *t, tlb_lra_record *out);
int tlb_node_enable_lra(tlb_node *nd);
int tlb_node_lra(tlb_node *nd, tlb_lra_record *out);

/* ---------------------------------------------------------------------------------------------
 * Maximum true peak: the largest value the signal reaches BETWEEN its samples, after ITU-R BS.1770-4 Annex 2, of the PCM the encoder is
 * given -- the ingest's planar output, AFTER the stream's gain, what the loudness meter reads too.  EBU R 128 holds a head-end to a maximum
 * true peak of -1 dBTP beside its -23 LUFS; the sample peaks of the ingest under-read it by up to 3 dB (a sine at fs / 4 sampled 45 degrees
 * off its crests shows -3 dBFS at 0 dBTP), and a Layer II decoder at the listener's end reconstructs exactly those peaks.  Opt-in; the
 * meter lives on the device.
 * THE ARITHMETIC.  The reference has no true-peak meter, so this is the definition, in integers (tests/truepeaklib.py restates it in numpy
 * int64, every comparison against it is byte for byte on the records).  4x oversampling by a polyphase FIR, then the absolute maximum; 4x at
 * every encoder rate, since an n-times meter's under-read depends on the signal's frequency relative to the sample rate and not on the rate.
 *   table       int16 H[3][TLB_TRUEPEAK_TAPS], committed as csrc/tl_truepeak_taps.inc: the phases 1/4, 2/4, 3/4 between two samples of a
 *               fourth-band prototype (a Kaiser-windowed sinc, beta = 8, 12 taps per phase as BS.1770-4's own filter has; the committed
 *               table is the definition, tools/gen_truepeak_taps.py the record of how it was made).  Every row sums to exactly 32768, row 3
 *               is row 1 reversed, row 2 is symmetric.  Phase 0 of such a prototype is the sample itself and is not stored:
 *               v_0(n) = 32768 x[n], so true peak >= sample peak by construction and no tap of 32768 has to fit an int16
 *   per channel x[n] are the stream's planar samples since its last reset, zeros before it.  For p = 1, 2, 3
 *               v_p(n) = sum_{t = 0 .. 11} H[p][t] x[n - t], the exact integer sum: max_p sum_t |H[p][t]| = 57 760 and 57 760 * 32768 <
 *               2^31, so a WHOLE ROW is summed in 32 bits, in any order, and no half sums in 64 bits are needed
 *   frame       peak = max over the frame's 1152 n of max(32768 |x[n]|, |v_1(n)|, |v_2(n)|, |v_3(n)|): an unsigned 32-bit number in units
 *               of 2^-30 of full scale.  An interpolated value belongs to the frame in which its NEWEST sample x[n] arrives (the point it
 *               stands for lies between x[n - 6] and x[n - 5]); the last 11 samples of a channel are carried from frame to frame and
 *               from call to call
 *   dBTP        tlb_truepeak_dbtp(v) = 20 log10(v / 2^30), -inf for 0
 * RECORD.  tlb_truepeak_record, 32 bytes: frames = PCM frames measured; overs = frames in which either channel's peak is STRICTLY above the
 * ceiling; peak[2] = the last measured frame's peak per channel; peak_max[2] = the maximum since the reset; sample_max[2] = the largest
 * |x| since the reset, 0 .. 32768.  A one-channel stream leaves index 1 zero, and its second PCM row is not looked at; dual channel counts
 * as two channels.
 * CEILING.  Given at enable time in the same 2^-30 units; 0 selects TLB_TRUEPEAK_CEILING_DEFAULT = llround(2^30 * 10^(-1/20)), -1 dBTP.
 * STATE.  80 bytes of device memory per stream (the record and 2 x 12 carried samples, of which the oldest is never used), allocated by
 * tlb_truepeak_enable ALONE: a batch that never enables it allocates and queues nothing new, and the other calls answer TLB_ERR_ARG on it.
 *   tlb_truepeak_enable(b, ceiling)   allocates the state (waits for the device once); a second call answers 0 and leaves the ceiling
 *   tlb_truepeak_device(b, d_pcm_planar, nframes, d_records, stream)
 *                                     measures nframes of every stream, int16 [nframes][nstreams][2][1152] as tlb_ingest_device writes it
 *                                     (16-byte aligned), and writes tlb_truepeak_record [nstreams] (may be NULL) on hip_stream
 *   tlb_truepeak_host                 the same with host buffers
 *   tlb_truepeak_reset(b, stream)     -1: every stream.  Waits for the queued work, then zeroes the record and the carried samples
 *   tlb_truepeak_taps(out[3][12])     the committed table; no GPU
 *   tlb_truepeak_dbtp(v)              no GPU
 * tlb_stream_reset, tlb_stream_reconfigure and tlb_reset clear the stream's true-peak state; tlb_stream_finish leaves it.
 * TICK PLANE.  tlb_tick_enable_truepeak(t, ceiling) before the first submit (TLB_ERR_ARG after it; a second call answers 0) enables the
 * meter of every group's batch.  Every submit with new input then queues the meter on the tick's planar PCM on the run stream, behind the
 * tick's encode and egress kernels and behind the loudness meter when both are on; the 32-byte records travel with the three output sets
 * behind the packets, on an event of their own: the packets' copy-out does not wait for them.  tlb_tick_truepeak(t) is tlb_truepeak_record
 * [nstreams] of the tick waited for last (pinned, valid until the next wait); NULL when the meter is off.  After T waited ticks
 * frames == T, and tlb_tick_finish adds nothing.  tlb_tick_truepeak_reset(t, stream) (-1: all) is legal with no tick in flight (TLB_ERR_ARG
 * otherwise, and when the meter is off).
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_truepeak goes to every shard before the first submit, and a
 * shard made by tlb_node_shard_restart is enabled again with the same ceiling -- its records start from zero.  tlb_node_truepeak(nd, stream)
 * points at the STREAM's record and answers NULL for a broken, late or stale shard; tlb_node_truepeak_reset routes like
 * tlb_node_loudness_reset.
 * NOT BUILT: true peak of the decoded output.  Acting on the gain: the true-peak limiter below (tlb_limiter_*).
 * ------------------------------------------------------------------------------------------ */
#define TLB_TRUEPEAK_TAPS 12
#define TLB_TRUEPEAK_CEILING_DEFAULT 956973408u
typedef struct { uint32_t frames, overs, peak[2], peak_max[2], sample_max[2]; } tlb_truepeak_record;      /* 32 bytes */
int tlb_truepeak_enable(tlb_batch *b, uint32_t ceiling);
int tlb_truepeak_device(tlb_batch *b, const int16_t *d_pcm_planar, int nframes, tlb_truepeak_record *d_records, void *hip_stream);
int tlb_truepeak_host(tlb_batch *b, const int16_t *pcm_planar, int nframes, tlb_truepeak_record *records);
int tlb_truepeak_reset(tlb_batch *b, int stream);
int tlb_truepeak_taps(int16_t out[3][TLB_TRUEPEAK_TAPS]);
double tlb_truepeak_dbtp(uint32_t v);
int tlb_tick_enable_truepeak(tlb_tick *t, uint32_t ceiling);
const tlb_truepeak_record *tlb_tick_truepeak(const tlb_tick *t);
int tlb_tick_truepeak_reset(tlb_tick *t, int stream);
int tlb_node_enable_truepeak(tlb_node *nd, uint32_t ceiling);
const tlb_truepeak_record *tlb_node_truepeak(const tlb_node *nd, int stream);
int tlb_node_truepeak_reset(tlb_node *nd, int stream);

/* ---------------------------------------------------------------------------------------------
 * True-peak limiter: a look-ahead limiter on the planar PCM between the ingest and the encoder, so that a caller who raises a quiet service
 * towards -23 LUFS with tlb_set_gain_db need not lower the whole programme for the frames the true-peak meter then counts in `overs`.
 * Opt-in, per stream, in place, on the device.
 * THE ARITHMETIC.  The reference has no limiter, so this is the definition, in integers (tests/limiterlib.py restates it in numpy int64,
 * every comparison against it is byte for byte, on the PCM and on the records).  U = 2^30 is unity gain; TLB_LIMITER_WMIN = 64,
 * TLB_LIMITER_WBOX = 32, TLB_LIMITER_DELAY = 63.  Per stream, x_c[n] are the planar samples the ingest wrote since the stream's last
 * reset, zeros before it (the true-peak meter's convention), H the committed table csrc/tl_truepeak_taps.inc, unchanged:
 *   1 detector  P[n] = max over the stream's channels c of max(32768 |x_c[n]|, |v_1|, |v_2|, |v_3|), v_p = sum_{t < 12} H[p][t] x_c[n - t]:
 *               the meter's per-sample quantity, in units of 2^-30 of full scale, a row in 32 bits by the table's bound.  The channels are
 *               LINKED; dual channel counts as two channels; a one-channel stream's second row is neither read nor written
 *   2 required  r[n] = U if P[n] <= ceiling, else floor(ceiling 2^30 / P[n]) (a 64-bit product; the result is below U)
 *   3 hold      m[n] = min(r[n - 63 .. n]); r = U before the reset
 *   4 release   e[n] = min(m[n], min(U, e[n - 1] + S)), e[-1] = U: the gain recovers linearly, S per sample.  A (min, +) recurrence, so
 *               e[n] = min(U, min_{k <= n}(m[k] + (n - k) S), e[-1] + (n + 1) S): a prefix minimum, not a serial chain
 *   5 smooth    G[n] = (sum_{i < 32} e[n - i]) >> 19 (the sum is at most 2^35: 64 bits); e = U before the reset; 0 <= G <= 65536
 *   6 apply     y_c[n] = sgn(x_c[n - 63]) ((|x_c[n - 63]| G[n]) >> 16): the product is at most 2^31 and fits unsigned 32 bits;
 *               G = 65536 returns the sample itself, -32768 included
 * The output is the input 63 samples late (1.3 ms at 48 kHz); nothing anywhere compensates that delay.
 * WHY THESE WINDOWS.  Every e[n - i], i < 32, is <= r[k] for all k in [n - 63, n - 31], so the gain on x[j], which leaves at n = j + 63, is
 * <= r[k] for every k in [j, j + 32]: every detector position k in [j, j + 11] that x[j] is a tap of.  Where r[k0] is a local minimum, G is
 * flat at r[k0] over the 33 outputs around it: all 12 samples of the offending interpolation get the same gain.
 *   THEOREM.      32768 |y_c[n]| <= ceiling for every sample, for any input.
 *   NOT A THEOREM. The output's TRUE peak can pass the ceiling: the gain varies across an interpolation's taps when overs follow each other
 *                 within a release of a few samples.  A numpy statement of this definition showed it on adversarial full-scale random
 *                 input (tests/test_limiter_emu.py measures it; DESIGN 7m has the figure); on structured signals -- sines, bursts,
 *                 squares, sweeps, gated tones -- the output's true peak stayed at or below the ceiling.
 * PARAMETERS.  tlb_limiter_params { ceiling, release_ms }: ceiling in 2^-30 units, 0 selects TLB_TRUEPEAK_CEILING_DEFAULT, any other value
 * must lie in [2^20, 2^30]; release_ms 0 selects TLB_LIMITER_RELEASE_DEFAULT_MS = 100, any other value must lie in [1, 10000].  A NULL
 * pointer is both defaults.  Per stream S = tlb_limiter_step(release_ms, samplerate) = max(1, (2^30 * 1000) / (release_ms * samplerate)),
 * computed in 64 bits on the host from the stream's ENCODER rate (no GPU; 0 for an illegal argument) and again on tlb_stream_reconfigure.
 * RECORD.  tlb_limiter_record, 32 bytes, zero after a reset: frames; limited = frames with any G < 65536; samples = outputs with
 * G < 65536, saturating; red_last = 65536 - min G of the last frame; red_max = the largest red_last since the reset; peak_in = max P of
 * the last frame; peak_in_max; reserved = 0.  An output belongs to the frame whose index n it has.
 * STATE.  720 bytes of device memory per stream (the record, 64 samples of delay line per channel, the carried r as four lanes' suffix
 * minima, the carried e of two lanes; csrc/mp2_limiter.h), allocated by tlb_limiter_enable ALONE: a batch that never enables it allocates
 * and queues nothing new, and the other calls answer TLB_ERR_ARG on it.
 *   tlb_limiter_enable(b, params)     allocates the state (waits for the device once); a second call with equal parameters answers 0, with
 *                                     different ones TLB_ERR_ARG
 *   tlb_limiter_device(b, d_pcm_planar, nframes, d_records, stream)
 *                                     limits nframes of every stream IN PLACE, int16 [nframes][nstreams][2][1152] as tlb_ingest_device
 *                                     writes it (16-byte aligned), and writes tlb_limiter_record [nstreams] (may be NULL) on hip_stream
 *   tlb_limiter_host                  the same with host buffers (records may be NULL)
 *   tlb_limiter_reset(b, stream)      -1: every stream.  Waits for the queued work, then zeroes the record, the delay line and the gains
 *   tlb_limiter_step(release_ms, samplerate)    no GPU
 * tlb_stream_reset, tlb_stream_reconfigure and tlb_reset clear the stream's limiter state; tlb_stream_finish leaves it, and the 63 samples
 * still in the delay line are NOT flushed: they leave with the stream's next frames, or never.
 * TICK PLANE.  tlb_tick_enable_limiter(t, params) before the first submit (TLB_ERR_ARG after it; a second call as above) enables the limiter
 * of every group's batch.  Every submit then queues it on the tick's planar PCM on the run stream, behind the ingest and AHEAD of the
 * encoder: the encoder, the compare monitor and both meters see the limited PCM.  The ingest's peaks and the silence counter remain those
 * of the INPUT.  The 32-byte records travel with the three output sets behind the packets, on an event of their own.  tlb_tick_limiter(t) is
 * tlb_limiter_record [nstreams] of the tick waited for last (pinned, valid until the next wait); NULL when the limiter is off.  After T
 * waited ticks frames == T, and tlb_tick_finish adds nothing.  tlb_tick_limiter_reset(t, stream) (-1: all) is legal with no tick in flight.
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_limiter goes to every shard before the first submit, and a shard
 * made by tlb_node_shard_restart is enabled again with the same parameters, from zero.  tlb_node_limiter(nd, stream) points at the STREAM's
 * record and answers NULL for a broken, late or stale shard; tlb_node_limiter_reset routes like tlb_node_loudness_reset.
 * NOT BUILT: a loudness-driven automatic gain (the caller's loop stays the policy), multiband or soft-knee dynamics, unlinked channels,
 * compensating the delay, limiting the decoded output.
 * ------------------------------------------------------------------------------------------ */
#define TLB_LIMITER_WMIN 64
#define TLB_LIMITER_WBOX 32
#define TLB_LIMITER_DELAY 63
#define TLB_LIMITER_RELEASE_DEFAULT_MS 100u
typedef struct { uint32_t ceiling; uint32_t release_ms; } tlb_limiter_params;
typedef struct { uint32_t frames, limited, samples, red_last, red_max, peak_in, peak_in_max, reserved; } tlb_limiter_record;      /* 32 bytes */
int tlb_limiter_enable(tlb_batch *b, const tlb_limiter_params *params);
int tlb_limiter_device(tlb_batch *b, int16_t *d_pcm_planar, int nframes, tlb_limiter_record *d_records, void *hip_stream);
int tlb_limiter_host(tlb_batch *b, int16_t *pcm_planar, int nframes, tlb_limiter_record *records);
int tlb_limiter_reset(tlb_batch *b, int stream);
uint32_t tlb_limiter_step(uint32_t release_ms, long samplerate);
int tlb_tick_enable_limiter(tlb_tick *t, const tlb_limiter_params *params);
const tlb_limiter_record *tlb_tick_limiter(const tlb_tick *t);
int tlb_tick_limiter_reset(tlb_tick *t, int stream);
int tlb_node_enable_limiter(tlb_node *nd, const tlb_limiter_params *params);
const tlb_limiter_record *tlb_node_limiter(const tlb_node *nd, int stream);
int tlb_node_limiter_reset(tlb_node *nd, int stream);

/* ------------------------------------------------------------------------------------------
 * CONCEALMENT of lost frames on a Layer II feed -- strict, adapted or down (tlb_conceal_*; csrc/mp2_conceal.h, csrc/toolame_conceal.hip and,
 * for adapted and down feeds, tlb_feed_loss_enable / tlb_*_enable_feed_loss -- the tlb_conceal_* names are the strict-feed family as it was
 * first shipped, and its set is closed --; csrc/mp2_conceal_conv.h, csrc/toolame_conceal_conv.hip).  Without it "an empty
 * slot or a frame that does not pass is silence" (tlb_feed_*): 24 ms of digital zero cut in hard, and the good frame behind it synthesised
 * over a silent filter history -- two discontinuities per lost packet, which the encoder then broadcasts.  With it a lost frame is the last
 * good frame once more, quieter with every repeat, and the good frame behind a loss continues from that repeat.
 * THE RULE.  The reference has no concealment (its inputs leave it to their decoders), so this is the definition (tests/conceallib.py
 * restates it).  Per stream two parameters: hold, 1..TLB_CONCEAL_MAX_HOLD frames, and step, 1..TLB_CONCEAL_MAX_STEP scalefactor-index units
 * per lost frame (scalefactor[i] = 2^(1 - i/3): 3 is 6.02 dB; index 63 is 1e-20).
 *   A slot PASSES when its feed report has none of TLB_DEC_BAD_MASK | TLB_DEC_EMPTY, else it is LOST.
 *   G     the bytes of the last slot that passed; none before the first passing slot and after a reset
 *   k     consecutive lost slots ending at this one, 0 for a passing slot; it carries across calls
 *   o(k)  o(0) = 0; o(k) = step * k for 1 <= k <= hold; o(k) = MUTE for k > hold
 *   "G at offset o" is G parsed as a feed frame, every cell's three scalefactor indices replaced by min(index + o, 63); at MUTE all are 63
 *   a lost slot with run k:      no G, or o(k - 1) = MUTE: zeros, as without concealment.  Otherwise the synthesis of G at o(k) over the
 *                                history G at o(k - 1): frame hold + 1 is the all-63 frame over the last audible repeat -- the filterbank's
 *                                tail rings out and is not cut
 *   a passing slot behind a loss of run k': G (the one from before this slot) exists and o(k') != MUTE: its own bytes over the history G at
 *                                o(k').  Otherwise silent history, as without concealment
 *   a passing slot behind a passing slot: untouched
 * The result depends on the sequence of slots only, never on how it is cut into calls or ticks.  The feed's own tlb_frame_report is
 * unchanged: a concealed slot still reports why it was lost.
 * THE SEQUENCE.  A strict feed wants a frame every tick: every slot is a slot of the sequence, and an empty one is a lost packet.  The
 * sequence of a stream with an ADAPTED or a DOWN feed is its WANTED slots only, in order: the ticks with tlb_feed_want_at == 1, or slots
 * j < tlb_feed_down_want_at of every tick, slot 0 before slot 1.  An unwanted slot, empty or TLB_DEC_UNWANTED, is no slot of the sequence:
 * it neither passes nor is lost, and touches neither k nor G nor the record.  What the rule makes of a wanted slot replaces its 1152 decoded
 * source frames, in the feed's channel layout, BEFORE the channel map and the resampler or decimator read them and before the queue keeps
 * them.  So the PCM the ingest receives is, bit for bit, that of the chain "strict feed with tlb_conceal_enable at the feed's own rate and
 * channel count over the wanted slots, the channel map, tlb_resample_* or tlb_decimate_*" -- both discontinuities are gone before the filter
 * could smear them.
 * RECORD.  tlb_conceal_record, 32 bytes: frames = slots of the sequence seen (wanted slots); passed; concealed = lost slots synthesised from G (the ring-out frame
 * included); muted = lost slots left as zeros; runs = loss runs begun; longest = the longest loss run; run = k now; offset = o(k) of the last
 * slot, 0 for a passing one, TLB_CONCEAL_MUTE for MUTE.  A stream without concealment has an all-zero record.
 * CALLS.  Opt-in per stream; a batch that never enables it allocates nothing and makes the device calls it made before.
 *   tlb_conceal_enable(b, stream, hold, step)  stream -1: every stream; every named stream is checked before anything changes.  hold 0
 *                                     switches concealment off (step is then not read).  TLB_ERR_ARG for a stream without a strict feed
 *                                     (none, an adapted one, a down feed), hold > 16, step outside 1..21.  Waits for the queued work;
 *                                     the named streams' G, run and record start again
 *   tlb_feed_loss_enable(b, stream, hold, step)  the same call for a stream with a Layer II feed of ANY kind: on a stream with a strict
 *                                     feed it is tlb_conceal_enable; on one with an adapted or a down feed it switches the concealment
 *                                     of THE SEQUENCE above on.  TLB_ERR_ARG for a stream with no feed at all, hold > 16, step outside
 *                                     1..21; -1 and hold 0 as above.  The four calls below serve every kind of stream
 *   tlb_conceal_get(b, stream, &hold, &step)  1: on, 0: off (both 0), negative: -TLB_ERR_ARG.  Either pointer may be NULL
 *   tlb_conceal_reset(b, stream)      -1: every stream.  Waits for the queued work, then forgets G, run and the record; the parameters stay
 *   tlb_conceal_records_device(b, d_records, hip_stream)  queues a copy of tlb_conceal_record [nstreams] into device memory on hip_stream
 *                                     (the stream the feed calls are queued on): the records as of the last feed call queued there
 *   tlb_conceal_records_host(b, records)  waits for the device, then the same into host memory
 * tlb_feed_device and tlb_feed_host queue the two concealment kernels themselves, behind the feed's own two (which run exactly as before),
 * whenever some stream with a strict feed has concealment on.  The adapted path then runs decode, conceal, resample, carry, conceal-carry and
 * the down path (tlb_feed_down_device / _host) decode, conceal, decimate, carry, conceal-carry, the two new kernels only when some adapted
 * (or down) stream of the batch has concealment on: a batch without one queues exactly the kernels it queued before.  tlb_feed_set,
 * tlb_feed_set_adapted and tlb_feed_down_set on a stream (removal included) switch its concealment OFF -- G would be a frame of another
 * format --, and tlb_feed_reset, tlb_feed_down_reset and every call that implies either (tlb_reset, tlb_stream_reset,
 * tlb_stream_reconfigure) forget the stream's G, run and record like tlb_conceal_reset.  tlb_stream_reconfigure keeps hold and step of a
 * stream of any kind whose feed stays legal with the new configuration; one that removes the feed takes the concealment with it.
 * Device memory per stream of a batch that has concealment on: the widest feed history slot of any kind in the batch (tlb_feed_stride at
 * the time, 576 bytes for 192 kbps at 48 kHz; 1728 once the batch has a down feed) for G, plus 48 (the record and the parameters with G's
 * length).
 * TICK PLANE.  tlb_tick_enable_conceal(t, stream, hold, step) is tlb_conceal_enable routed to the stream's group (-1: all, checked first),
 * legal while no tick is in flight (TLB_ERR_ARG otherwise); the first call that switches concealment on makes the records' pinned sets.
 * The records travel with the three output sets behind the packets, on an event of their own.  tlb_tick_conceal(t) is tlb_conceal_record
 * [nstreams] of the tick waited for last (pinned, valid until the next wait); NULL until concealment has been enabled.  tlb_tick_finish
 * adds nothing.  tlb_tick_conceal_reset(t, stream) (-1: all) is legal with no tick in flight.  tlb_tick_set_feed on a stream switches its
 * concealment off as tlb_feed_set does, and so do tlb_tick_set_feed_adapted and tlb_tick_set_down_feed.  tlb_tick_enable_feed_loss is
 * tlb_feed_loss_enable routed the same way.
 * NODE LEVEL, TICK plane only (a BATCH node: TLB_ERR_ARG): tlb_node_enable_conceal routes to the stream's shard (-1: every shard) between
 * steps; every named stream needs a strict feed set through tlb_node_set_feed, and tlb_node_set_feed on a stream switches its concealment
 * off.  A shard made by tlb_node_shard_restart gets its streams' concealment again behind their feeds, from zero.  tlb_node_conceal(nd,
 * stream) points at the STREAM's record and answers NULL for a broken, late or stale shard and for a shard none of whose streams ever
 * enabled it; tlb_node_conceal_reset routes like tlb_node_loudness_reset.  tlb_node_enable_feed_loss (TICK plane only) accepts a feed of
 * any kind the node remembers (tlb_node_set_feed, _set_feed_adapted, _set_down_feed; each of them switches the stream's concealment off) and
 * is set again on a restarted shard the same way.
 * NOT BUILT: interpolation between the frames either side of a loss, any change to the feed report.
 * ------------------------------------------------------------------------------------------ */
#define TLB_CONCEAL_MAX_HOLD 16
#define TLB_CONCEAL_MAX_STEP 21
#define TLB_CONCEAL_MUTE 0xFFFFFFFFu
typedef struct { uint32_t frames, passed, concealed, muted, runs, longest, run, offset; } tlb_conceal_record;      /* 32 bytes */
int tlb_conceal_enable(tlb_batch *b, int stream, int hold, int step);
int tlb_feed_loss_enable(tlb_batch *b, int stream, int hold, int step);
int tlb_conceal_get(const tlb_batch *b, int stream, int *hold, int *step);
int tlb_conceal_reset(tlb_batch *b, int stream);
int tlb_conceal_records_device(tlb_batch *b, tlb_conceal_record *d_records, void *hip_stream);
int tlb_conceal_records_host(tlb_batch *b, tlb_conceal_record *records);
int tlb_tick_enable_conceal(tlb_tick *t, int stream, int hold, int step);
int tlb_tick_enable_feed_loss(tlb_tick *t, int stream, int hold, int step);
const tlb_conceal_record *tlb_tick_conceal(const tlb_tick *t);
int tlb_tick_conceal_reset(tlb_tick *t, int stream);
int tlb_node_enable_conceal(tlb_node *nd, int stream, int hold, int step);
int tlb_node_enable_feed_loss(tlb_node *nd, int stream, int hold, int step);
const tlb_conceal_record *tlb_node_conceal(const tlb_node *nd, int stream);
int tlb_node_conceal_reset(tlb_node *nd, int stream);

/* Diagnostic only: per-stage cycle stamps [nframes][nstreams][32] (csrc/mp2_wave.h TL_STAMP), host buffers. */
int tlb_encode_host_stamps(tlb_batch *b, const int16_t *pcm, int nframes, long long *stamps);

/* Duration in milliseconds of the most recent tlb_encode_device()/tlb_encode_host() kernel, measured
 * with hipEvents on the launch stream (synchronises on that stream).  < 0 on error. */
float tlb_last_kernel_ms(tlb_batch *b);
/* Models 2 and 4 run as two kernels (the psychoacoustic model, then the rest of the encoder).  Their durations for the most
 * recent launch of a batch whose streams all use these models; non-zero return for any other batch (models 1 and 3 run
 * model and encoder in one kernel, model 0 has no model kernel). */
int tlb_last_stage_ms(tlb_batch *b, float *psy_ms, float *encode_ms);
/* Deployment self-check (no GPU needed): the device computes the reference's transcendental calls with its own restatement of glibc
 * 2.35's FMA-path routines (csrc/tl_libm.h), so bit-equality with a reference built on THIS host holds if this host's libm is that
 * libm.  Compares the two on `nsamples` arguments per function (<= 0: 100 000); returns the number of differing results -- 0 means
 * the reference compiled here and this library agree on log10 / pow / log / exp / sincos / atan2 bit for bit. */
long tlb_selfcheck_libm(long nsamples);
/* LDS bytes per wavefront: the largest per-wave block among the kernels (each holds 12 waves per CU). */
int tlb_lds_bytes_per_stream(void);
const char *tlb_version(void);

#ifdef __cplusplus
}
#endif
#endif
