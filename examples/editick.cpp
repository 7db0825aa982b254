// editick -- the per-tick loop body of odr-audioenc for N streams over the tick API (include/toolame_batch.h, tlb_tick_*):
// raw interleaved s16le PCM in, the EDI AF packets of stream 0 out (length-prefixed), every tick = one frame of every stream.
// Host code only (plain C++); everything between the two file accesses happens in libtoolame_dab_hip.so:
//
//   file -> pinned host PCM -> [PCIe, gain/peak/de-interleave, encode, EDI AF, PCIe: tlb_tick_run] -> packets -> file
//   (src/odr-audioenc.cpp:1030-1051,1139-1163,1208-1225 and src/Outputs.cpp:194-261 for one stream)
//
// build: g++ -O2 -std=c++17 examples/editick.cpp -Iinclude -Lodr-audioenc_amd -ltoolame_dab_hip -Wl,-rpath,$PWD/odr-audioenc_amd -o editick
// usage: editick in.s16le out.af [-r rate] [-c channels] [-b kbps] [-m s|j|d|m] [-p psy] [-g gain_dB] [-n streams] [-t now_s]
//                [--short-every N --short-by M] [--monitor check|audio] [--compare] [--loudness] [--lra] [--truepeak [DBTP]] [--limit [DBTP] --limit-release MS] [--source-rate R] [--feed FILE.mp2 --feed-bitrate K [--feed-rate R] [--feed-channels C]]
//                [--conceal [HOLD] --conceal-step N] [--feed-drop-every N --feed-drop-run M]
//   --feed FILE.mp2 --feed-bitrate K: the services' source is an MPEG Layer II file at the encoder's rate (-r) and channel count (-c) and
//   at K kbps, decoded on the device ahead of the ingest (tlb_tick_set_feed): the file is cut into frames by the arithmetic length and each
//   header's padding bit, service s takes frame (tick + s) of it (wrapping round), one tick per frame of the file.  No PCM crosses the
//   link; in.s16le is not opened (give "-").  Not together with --short-every or --source-rate.
//   --feed-rate R, --feed-channels C: the file is at another (legal) rate or channel count than the encoder's, an ADAPTED feed
//   (tlb_tick_set_feed_adapted): on the ticks tlb_tick_feed_want says want no frame the slot stays empty and the file does not advance.
//   R above the rate of a 24000 Hz encoder (48000, 44100, 32000) is a DOWN FEED (tlb_tick_set_down_feed): every tick takes the one or two
//   frames tlb_tick_down_feed_want asks for into the stream's two slots, and the device decodes, filters and decimates them.
//   --feed-drop-every N --feed-drop-run M: lost packets: the last M of every N WANTED slots (on a strict feed: ticks) stay empty in every stream
//   (the frames they would have carried are gone: the file advances).  Without --conceal each is 24 ms of silence, cut in hard.
//   --conceal [HOLD] --conceal-step N: feed concealment (tlb_tick_enable_conceal; tlb_tick_enable_feed_loss with --feed-rate / --feed-channels and
//   for a down feed, where the lost WANTED slots are concealed ahead of the resampler or decimator): a lost frame is the last good one once
//   more, N scalefactor-index units (default 3: 6 dB) quieter per lost frame, for HOLD frames (default 4), then the filterbank rings out.
//   One line at the end: the records summed over the streams -- slots, passed, concealed, muted, loss runs, the longest run.
//   --source-rate R: the input file is at R Hz (44100 for a 48000 Hz encoder, 32000; 22050 or 16000 for 24000 Hz) and is resampled to the
//   encoder's rate on the device (tlb_tick_set_source): each tick reads tlb_tick_need() source frames per stream, not 1152.  Not together
//   with --short-every.  R above the rate of a 24000 Hz encoder (48000, 44100, 32000) is a DOWN source (tlb_tick_set_down_source): each tick
//   reads tlb_tick_down_need() source frames per stream (2304 at 48 kHz) into the stream's wide slot (tlb_tick_down), and the device
//   filters and decimates them.
//   --short-every N --short-by M: short reads (src/odr-audioenc.cpp:335-373,910-935): on every Nth tick every Nth stream delivers M sample
//   frames fewer than 1152; the library stretches what came over the frame as the reference does and counts the underruns.
//   --monitor check|audio: the confidence monitor (tlb_tick_enable_monitor): every frame that leaves is checked on the device (audio: also
//   decoded).  One summary line at the end -- frames checked, bad frames, longest bad run over all streams, streams whose decoded output
//   is silent -- and a non-zero exit status when any frame was bad.
//   --compare: the compare monitor on top of it (tlb_tick_enable_compare with the header's default params; implies --monitor audio): every
//   frame that leaves is decoded and set against the audio that went in.  A stream whose mismatch_run reaches 3 is printed when it does;
//   one summary line at the end -- frames compared, judged, mismatched -- and exit status 4 when any stream got there.
//   --loudness: the loudness meter (tlb_tick_enable_loudness): the PCM the encoder is given (after -g) is measured on the device after
//   ITU-R BS.1770-4 / EBU R 128.  One line per stream at the end: momentary (400 ms), short-term (3 s) and integrated loudness in LUFS
//   (-inf where there is none yet), as "%.2f".
//   --lra: the loudness range on top of it (tlb_tick_enable_lra; implies --loudness): EBU Tech 3342's LRA from the short-term values.  One
//   more line per stream behind the loudness line: LRA in LU as "%.1f", the 10th and the 95th percentile in LUFS, gated of counted blocks.
//   --truepeak [DBTP]: the true-peak meter (tlb_tick_enable_truepeak): the same PCM oversampled four times on the device after ITU-R
//   BS.1770-4 Annex 2, against a ceiling of DBTP (default -1, EBU R 128's).  One line per stream at the end: the maximum true peak in
//   dBTP, the largest sample in dBFS and the number of frames over the ceiling.
//   --limit [DBTP] --limit-release MS: the true-peak limiter (tlb_tick_enable_limiter) between the ingest and the encoder, with a ceiling of
//   DBTP (default -1) and a release of MS milliseconds (default 100): what is encoded, and what the meters above read, is the limited PCM,
//   63 samples late.  One line per stream at the end: the frames limited, the largest reduction (65536 - G, and in dB) and the input's
//   maximum true peak.
// out.af: for every packet a little-endian uint32 length, then the packet.
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "toolame_batch.h"

static void die(const char *what, int code)
{
    std::fprintf(stderr, "editick: %s (code %d)\n", what, code);
    std::exit(1);
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s in.s16le out.af [-r rate] [-c channels] [-b kbps] [-m mode] [-p psy] [-g gain_dB] [-n streams] [-t now_s] [--short-every N --short-by M] [--monitor check|audio] [--compare] [--loudness] [--lra] [--truepeak [DBTP]] [--limit [DBTP] --limit-release MS] [--source-rate R] [--feed FILE.mp2 --feed-bitrate K [--feed-rate R] [--feed-channels C]] [--conceal [HOLD] --conceal-step N] [--feed-drop-every N --feed-drop-run M]\n", argv[0]);
        return 2;
    }
    long rate = 48000, source_rate = 0;
    long long now_s = 1700000000;
    int channels = 2, kbps = 128, psy = 1, nstreams = 1, short_every = 0, short_by = 0, monitor = 0, compare = 0, loudness = 0, lra = 0, truepeak = 0, limit = 0, limit_release = 0;
    double ceiling_db = -1.0, limit_db = -1.0;
    char mode = 0;
    double gain_db = 0.0;
    const char *feed_path = nullptr;
    int feed_kbps = 0, feed_channels = 0;
    long feed_rate = 0;
    int conceal = 0, conceal_step = 3, drop_every = 0, drop_run = 0;
    for (int i = 3; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--compare") { compare = 1; i--; continue; }    // the two options without a value
        if (k == "--loudness") { loudness = 1; i--; continue; }
        if (k == "--lra") { loudness = lra = 1; i--; continue; }
        if (k == "--truepeak") {                                 // its value is optional: taken when the next argument is a number
            truepeak = 1;
            char *end = nullptr;
            const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 < argc && end != argv[i + 1] && !*end) ceiling_db = v; else i--;
            continue;
        }
        if (k == "--limit") {                                    // likewise
            limit = 1;
            char *end = nullptr;
            const double v = i + 1 < argc ? std::strtod(argv[i + 1], &end) : 0.0;
            if (i + 1 < argc && end != argv[i + 1] && !*end) limit_db = v; else i--;
            continue;
        }
        if (k == "--conceal") {                                  // likewise: HOLD is taken when the next argument is a number
            conceal = 4;
            char *end = nullptr;
            const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 < argc && end != argv[i + 1] && !*end) conceal = (int)v; else i--;
            if (conceal < 1 || conceal > TLB_CONCEAL_MAX_HOLD) die("--conceal HOLD: 1..16", conceal);
            continue;
        }
        if (i + 1 >= argc) die("option without a value", 0);
        const char *v = argv[i + 1];
        if (k == "-r") rate = std::atol(v);
        else if (k == "-c") channels = std::atoi(v);
        else if (k == "-b") kbps = std::atoi(v);
        else if (k == "-m") mode = v[0];
        else if (k == "-p") psy = std::atoi(v);
        else if (k == "-g") gain_db = std::atof(v);
        else if (k == "-n") nstreams = std::atoi(v);
        else if (k == "-t") now_s = std::atoll(v);
        else if (k == "--short-every") short_every = std::atoi(v);
        else if (k == "--short-by") short_by = std::atoi(v);
        else if (k == "--limit-release") limit_release = std::atoi(v);
        else if (k == "--source-rate") source_rate = std::atol(v);
        else if (k == "--feed") feed_path = v;
        else if (k == "--feed-bitrate") feed_kbps = std::atoi(v);
        else if (k == "--feed-rate") feed_rate = std::atol(v);
        else if (k == "--feed-channels") feed_channels = std::atoi(v);
        else if (k == "--conceal-step") conceal_step = std::atoi(v);
        else if (k == "--feed-drop-every") drop_every = std::atoi(v);
        else if (k == "--feed-drop-run") drop_run = std::atoi(v);
        else if (k == "--monitor") { monitor = !std::strcmp(v, "check") ? TLB_MONITOR_CHECK : !std::strcmp(v, "audio") ? TLB_MONITOR_AUDIO : 0; if (!monitor) die("--monitor check|audio", 0); }
        else die("unknown option", 0);
    }
    if (compare) { if (monitor == TLB_MONITOR_CHECK) die("--compare needs --monitor audio", 0); monitor = TLB_MONITOR_AUDIO; }
    if (!mode) mode = channels == 1 ? 'm' : 'j';             // odr-audioenc's defaults (src/odr-audioenc.cpp:697-709)
    if (channels != 1 && channels != 2) die("1 or 2 channels", channels);
    if (nstreams < 1) die("streams", nstreams);
    if (short_every < 0 || short_by < 0 || short_by > 1152 || (short_every > 0) != (short_by > 0)) die("--short-every N --short-by M: N >= 1 and 1 <= M <= 1152, both or neither", 0);

    if ((feed_path != nullptr) != (feed_kbps > 0)) die("--feed FILE.mp2 --feed-bitrate K: both or neither", 0);
    std::FILE *fi = feed_path ? nullptr : std::fopen(argv[1], "rb");
    if (!feed_path && !fi) die("cannot open input", 0);
    tlb_feed_config feed = {feed_rate ? feed_rate : rate, feed_kbps, feed_channels ? feed_channels : channels};      // the encoder's unless told otherwise
    const bool down_feed = feed_path && feed.samplerate > rate;  // a feed above the encoder's rate: two slots per tick, decoded and decimated
    const bool adapt = !down_feed && (feed.samplerate != rate || feed.channels != channels);
    if (drop_every < 0 || drop_run < 0 || drop_run > drop_every || (drop_every > 0) != (drop_run > 0)) die("--feed-drop-every N --feed-drop-run M: 1 <= M <= N, both or neither", 0);
    if ((conceal || drop_every) && !feed_path) die("--conceal and --feed-drop-every need a strict --feed (the encoder's rate and channel count)", 0);
    std::vector<uint8_t> mp2;
    std::vector<size_t> fpos, flen;                              // --feed: where each frame lies in the file
    if (feed_path) {
        if (int rc = tlb_feed_check_config(&feed)) die("--feed-bitrate: no legal Layer II configuration at this rate and channel count", rc);
        std::FILE *ff = std::fopen(feed_path, "rb");
        if (!ff) die("cannot open the feed", 0);
        uint8_t buf[1 << 15];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, ff)) > 0) mp2.insert(mp2.end(), buf, buf + n);
        std::fclose(ff);
        const size_t base = (size_t)tlb_feed_frame_bytes(&feed);
        for (size_t o = 0; o + 4 <= mp2.size();) {               // the sync word, the arithmetic length, one more with the padding bit
            if (mp2[o] != 0xff || (mp2[o + 1] & 0xf0) != 0xf0) die("the feed has no sync word where a frame should begin, at byte", (int)o);
            const size_t len = base + ((mp2[o + 2] >> 1) & 1u);
            if (o + len > mp2.size()) break;
            fpos.push_back(o); flen.push_back(len);
            o += len;
        }
        if (fpos.empty()) die("the feed is shorter than one frame", 0);
    }
    std::FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) die("cannot open output", 0);

    static const char version[] = "editick example";
    std::vector<tlb_stream_config> cfg((size_t)nstreams, tlb_stream_config{rate, mode, kbps, psy, 0});
    tlb_tick_config tc;
    std::memset(&tc, 0, sizeof tc);
    tc.egress = TLB_TICK_EDI_AF;
    tc.version = version; tc.version_len = (int)std::strlen(version);
    tc.now_s = now_s; tc.delay_ms = 0; tc.tist = 1; tc.tai_utc_offset = 37;
    int err = 0;
    tlb_tick *t = tlb_tick_create(0, nstreams, cfg.data(), &tc, &err);
    if (!t) die("tlb_tick_create", err);
    if (gain_db != 0.0 && tlb_tick_set_gain_db(t, -1, gain_db)) die("gain", 0);
    if (short_every) if (int rc = tlb_tick_enable_short_reads(t)) die("tlb_tick_enable_short_reads", rc);     // before the first submit
    if (monitor) if (int rc = tlb_tick_enable_monitor(t, monitor)) die("tlb_tick_enable_monitor", rc);           // likewise
    if (loudness) if (int rc = tlb_tick_enable_loudness(t)) die("tlb_tick_enable_loudness", rc);                 // likewise
    if (lra) if (int rc = tlb_tick_enable_lra(t)) die("tlb_tick_enable_lra", rc);                                // ... behind loudness
    const uint32_t ceiling = (uint32_t)std::llround(1073741824.0 * std::pow(10.0, ceiling_db / 20.0));             // in units of 2^-30 of full scale
    if (truepeak) if (int rc = tlb_tick_enable_truepeak(t, ceiling)) die("tlb_tick_enable_truepeak", rc);        // likewise
    const tlb_limiter_params lparams = {(uint32_t)std::llround(1073741824.0 * std::pow(10.0, limit_db / 20.0)), (uint32_t)limit_release};      // release 0: the default
    if (limit) if (int rc = tlb_tick_enable_limiter(t, &lparams)) die("tlb_tick_enable_limiter", rc);             // likewise
    const bool down = source_rate > rate;                    // a source above the encoder's rate goes through the decimator and its wide slots
    if (source_rate && !down) if (int rc = tlb_tick_set_source(t, -1, source_rate)) die("tlb_tick_set_source", rc);       // while no tick is in flight
    if (down) if (int rc = tlb_tick_set_down_source(t, -1, source_rate)) die("tlb_tick_set_down_source", rc);             // likewise
    if (down_feed) { if (int rc = tlb_tick_set_down_feed(t, -1, &feed)) die("tlb_tick_set_down_feed", rc); }      // likewise
    else if (feed_path && !adapt) if (int rc = tlb_tick_set_feed(t, -1, &feed)) die("tlb_tick_set_feed", rc);
    if (feed_path && adapt) if (int rc = tlb_tick_set_feed_adapted(t, -1, &feed)) die("tlb_tick_set_feed_adapted", rc);
    if (conceal && !(adapt || down_feed)) if (int rc = tlb_tick_enable_conceal(t, -1, conceal, conceal_step)) die("tlb_tick_enable_conceal", rc);       // behind the feed, while no tick is in flight
    if (conceal && (adapt || down_feed)) if (int rc = tlb_tick_enable_feed_loss(t, -1, conceal, conceal_step)) die("tlb_tick_enable_feed_loss", rc);     // an adapted or a down feed: its WANTED slots
    const tlb_compare_params cparams = {TLB_COMPARE_DEFAULT_MIN_ENERGY, TLB_COMPARE_DEFAULT_CORR_NUM, TLB_COMPARE_DEFAULT_CORR_DEN};
    if (compare) if (int rc = tlb_tick_enable_compare(t, &cparams)) die("tlb_tick_enable_compare", rc);          // after the audio monitor, before the first submit

    size_t per_frame = 1152 * (size_t)channels;              // samples of one frame in the file
    std::vector<int16_t> frame(down ? 2304 * (size_t)channels : per_frame);
    long frames = 0, packets = 0, bad_feed = 0;
    int alarms = 0;                                              // compare monitor: times a stream's mismatch_run reached 3
    uint32_t longest_run = 0;                                    // confidence monitor: the longest bad run any stream has shown after a tick
    const auto t0 = std::chrono::steady_clock::now();
    auto emit = [&]() {
        for (int u = 0; u < tlb_tick_units(t, 0); u++) {
            int len = 0;
            const uint8_t *p = tlb_tick_packet(t, 0, u, &len);
            if (!p || !len) continue;
            const uint32_t n = (uint32_t)len;
            const uint8_t le[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
            if (std::fwrite(le, 1, 4, fo) != 4 || std::fwrite(p, 1, n, fo) != n) die("write", 0);
            packets++;
        }
        if (const tlb_monitor_record *r = tlb_tick_monitor(t))   // what an operator reads every tick: [nstreams] records of the tick just waited for
            for (int s = 0; s < nstreams; s++) if (r[s].bad_run > longest_run) longest_run = r[s].bad_run;
        if (const tlb_compare_record *c = tlb_tick_compare(t))   // likewise; a run passes 3 once: a skipped or unjudged frame leaves it alone, so look at this tick's flags too
            for (int s = 0; s < nstreams; s++)
                if (c[s].mismatch_run == 3 && (c[s].last_flags & TLB_COMPARE_MISMATCH)) {
                    std::fprintf(stderr, "editick: compare: stream %d: 3 frames in a row do not sound like their input%s (tick %ld)\n", s,
                                 c[s].last_flags & TLB_COMPARE_SWAPPED ? ", channels exchanged" : "", frames);
                    alarms++;
                }
    };
    size_t used = 0;                                             // feed frames stream 0 has been given; stream s is s frames ahead in the file
    // the packets of wanted slot k (counted from 0) are lost: the slot stays empty, and the file advances
    auto dropped = [&](size_t k) { return drop_every && k % (size_t)drop_every >= (size_t)(drop_every - drop_run); };
    for (; down_feed;) {                                         // a down feed: one or two frames of the file per tick, as the schedule says
        const size_t want = (size_t)tlb_tick_down_feed_want(t, 0);   // (every stream has the one configuration: all want the same)
        if (used + want > fpos.size()) break;
        uint8_t *fr = tlb_tick_down_feed(t);                         // pinned [nstreams][2][tlb_tick_down_feed_stride()], re-fetched every tick like the PCM
        int32_t *ln = tlb_tick_down_feed_len(t);                     // pinned [nstreams][2]: every set comes back all 0
        const size_t stride = (size_t)tlb_tick_down_feed_stride(t);
        for (int s = 0; s < nstreams; s++)
            for (size_t j = 0; j < want; j++) {
                if (dropped(used + j)) continue;
                const size_t k = (used + j + (size_t)s) % fpos.size();
                std::memcpy(fr + stride * (2 * (size_t)s + j), &mp2[fpos[k]], flen[k]);
                ln[2 * s + (int)j] = (int32_t)flen[k];
            }
        used += want;
        if (int rc = tlb_tick_run(t)) die("tlb_tick_run", rc);
        const tlb_frame_report *rep = tlb_tick_down_feed_report(t);  // [nstreams][2]; a frame that did not pass went in as silence
        for (int s = 0; s < 2 * nstreams; s++) bad_feed += (rep[s].status & TLB_DEC_BAD_MASK) != 0;
        emit();
        frames++;
    }
    for (; feed_path && !down_feed;) {                           // one tick per wanted frame of the feed, and the ticks between that want none
        const bool want = tlb_tick_feed_want(t, 0) > 0;          // (every stream has the one configuration: all want a frame or none does)
        if (want && used == fpos.size()) break;
        uint8_t *fr = tlb_tick_feed(t);                          // pinned [nstreams][tlb_tick_feed_stride()], re-fetched every tick like the PCM
        int32_t *ln = tlb_tick_feed_len(t);                      // pinned [nstreams]: every set comes back all 0
        const size_t stride = (size_t)tlb_tick_feed_stride(t);
        for (int s = 0; s < nstreams && want && !dropped(used); s++) {
            const size_t k = (used + (size_t)s) % fpos.size();
            std::memcpy(fr + stride * (size_t)s, &mp2[fpos[k]], flen[k]);
            ln[s] = (int32_t)flen[k];
        }
        used += want;
        if (int rc = tlb_tick_run(t)) die("tlb_tick_run", rc);
        const tlb_frame_report *rep = tlb_tick_feed_report(t);   // a frame that did not pass went in as silence
        for (int s = 0; s < nstreams; s++) bad_feed += (rep[s].status & TLB_DEC_BAD_MASK) != 0;
        emit();
        frames++;
    }
    for (; !feed_path;) {
        if (source_rate) per_frame = (size_t)(down ? tlb_tick_down_need(t, 0) : tlb_tick_need(t, 0)) * (size_t)channels;      // 1058 or 1059 frames at 44.1 kHz, 768 at 32 kHz; 2304 for 48 -> 24 kHz: every stream is fed the one file, so all need the same
        if (std::fread(frame.data(), sizeof(int16_t), per_frame, fi) != per_frame) break;
        int16_t *in = tlb_tick_pcm(t);                       // pinned [nstreams][2304]; mono streams use the first 1152 values
        for (int s = 0; s < nstreams; s++)                   // a down source: the stream's wide slot (pinned, 4608 values, re-fetched every tick like the PCM) instead
            std::memcpy(down ? tlb_tick_down(t, s) : in + (size_t)s * 2304, frame.data(), per_frame * sizeof(int16_t));
        if (short_every && frames % short_every == 0) {          // every set comes back all 1152: only the short streams are written
            int32_t *valid = tlb_tick_valid(t);                  // pinned [nstreams], re-fetched like the PCM
            for (int s = 0; s < nstreams; s += short_every) valid[s] = 1152 - short_by;
        }
        if (int rc = tlb_tick_run(t)) die("tlb_tick_run", rc);
        emit();
        frames++;
    }
    if (frames > 0) {
        if (int rc = tlb_tick_finish(t)) die("tlb_tick_finish", rc);     // the pending last frame (toolame_finish at stream end)
        emit();
    }
    if (short_every) {                                           // what a caller acts on: the reference gives up after 60 s without a full read (:925-931)
        const uint32_t *ms = tlb_tick_underrun_ms(t), *n = tlb_tick_underruns(t);
        std::fprintf(stderr, "editick: stream 0: %u short reads, %u ms since its last full read\n", n[0], ms[0]);
    }
    if (feed_path) std::fprintf(stderr, "editick: feed: %zu frames of %d kbps in the file, %ld feed frames did not pass\n", fpos.size(), feed_kbps, bad_feed);
    if (conceal && frames > 0) {                                 // the records of the last tick (the finish adds nothing), summed over the streams
        const tlb_conceal_record *r = tlb_tick_conceal(t);
        unsigned long c[5] = {0, 0, 0, 0, 0};
        uint32_t longest = 0;
        for (int s = 0; s < nstreams; s++) {
            c[0] += r[s].frames; c[1] += r[s].passed; c[2] += r[s].concealed; c[3] += r[s].muted; c[4] += r[s].runs;
            if (r[s].longest > longest) longest = r[s].longest;
        }
        std::fprintf(stderr, "editick: conceal: %lu slots, %lu passed, %lu concealed, %lu muted, %lu runs, longest %u\n", c[0], c[1], c[2], c[3], c[4], longest);
    }
    unsigned long checked = 0, bad = 0;
    if (monitor) {
        const tlb_monitor_record *r = tlb_tick_monitor(t);
        int silent = 0;
        for (int s = 0; s < nstreams; s++) { checked += r[s].frames; bad += r[s].bad_frames; silent += r[s].out_silence_ms > 0; }
        std::fprintf(stderr, "editick: monitor: %lu frames checked, %lu bad, longest bad run %u, %d stream(s) silent at the output\n", checked, bad, longest_run, silent);
    }
    if (compare) {
        const tlb_compare_record *c = tlb_tick_compare(t);
        unsigned long compared = 0, judged = 0, mismatched = 0;
        for (int s = 0; s < nstreams; s++) { compared += c[s].frames_compared; judged += c[s].frames_judged; mismatched += c[s].mismatch_frames; }
        std::fprintf(stderr, "editick: compare: %lu frames compared, %lu judged, %lu mismatched, %d alarm(s)\n", compared, judged, mismatched, alarms);
    }
    if (loudness && frames > 0) {                                // the records of the last tick (the finish adds nothing); the gated value on request
        const tlb_loudness_record *r = tlb_tick_loudness(t);
        std::vector<tlb_loudness_programme_record> prog((size_t)nstreams);
        if (int rc = tlb_tick_loudness_programme(t, prog.data())) die("tlb_tick_loudness_programme", rc);
        for (int s = 0; s < nstreams; s++)
            std::fprintf(stderr, "editick: loudness: stream %d: momentary %.2f LUFS, short-term %.2f LUFS, integrated %.2f LUFS (%u of %u blocks)\n", s,
                         tlb_loudness_lufs(r[s].momentary), tlb_loudness_lufs(r[s].short_term), tlb_loudness_lufs(prog[(size_t)s].integrated), prog[(size_t)s].gated, r[s].blocks);
    }
    if (lra && frames > 0) {                                     // the range of everything measured, on request like the gated value
        std::vector<tlb_lra_record> range((size_t)nstreams);
        if (int rc = tlb_tick_lra(t, range.data())) die("tlb_tick_lra", rc);
        for (int s = 0; s < nstreams; s++)
            std::fprintf(stderr, "editick: lra: stream %d: LRA %.1f LU, low %.2f LUFS, high %.2f LUFS (%u of %u blocks)\n", s, tlb_lra_lu(&range[(size_t)s]),
                         tlb_loudness_lufs(range[(size_t)s].low), tlb_loudness_lufs(range[(size_t)s].high), range[(size_t)s].gated, range[(size_t)s].blocks);
    }
    if (truepeak && frames > 0) {                                // the records of the last tick (the finish adds nothing)
        const tlb_truepeak_record *r = tlb_tick_truepeak(t);
        for (int s = 0; s < nstreams; s++) {
            const uint32_t pk = r[s].peak_max[0] > r[s].peak_max[1] ? r[s].peak_max[0] : r[s].peak_max[1];
            const uint32_t sm = r[s].sample_max[0] > r[s].sample_max[1] ? r[s].sample_max[0] : r[s].sample_max[1];
            std::fprintf(stderr, "editick: truepeak: stream %d: max %.2f dBTP, samples %.2f dBFS, %u of %u frames over %.2f dBTP\n", s,
                         tlb_truepeak_dbtp(pk), tlb_truepeak_dbtp(sm << 15), r[s].overs, r[s].frames, tlb_truepeak_dbtp(ceiling));
        }
    }
    if (limit && frames > 0) {                                   // the records of the last tick (the finish adds nothing)
        const tlb_limiter_record *r = tlb_tick_limiter(t);
        for (int s = 0; s < nstreams; s++)
            std::fprintf(stderr, "editick: limiter: stream %d: limited %u of %u frames, red_max %u (%.2f dB), input max %.2f dBTP, ceiling %.2f dBTP\n", s,
                         r[s].limited, r[s].frames, r[s].red_max, r[s].red_max < 65536u ? 20.0 * std::log10((65536.0 - r[s].red_max) / 65536.0) : -INFINITY,
                         tlb_truepeak_dbtp(r[s].peak_in_max), tlb_truepeak_dbtp(lparams.ceiling));
    }
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fprintf(stderr, "editick: %ld ticks of %d stream(s), %ld AF packets of stream 0, %.3f s (%.0f frames/s, PCIe and EDI included)\n",
                 frames, nstreams, packets, sec, sec > 0 ? (double)frames * nstreams / sec : 0.0);
    tlb_tick_destroy(t);
    if (fi) std::fclose(fi);
    std::fclose(fo);
    return bad ? 3 : alarms ? 4 : 0;
}
