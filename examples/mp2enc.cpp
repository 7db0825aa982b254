// mp2enc -- a minimal "odr-audioenc -i file -o file" over the batched C-ABI (include/toolame_batch.h): raw interleaved
// s16le PCM in, DAB MP2 frames out, for one stream or for N copies of it in one batch.  Host code only (plain C++, no
// HIP in this file); everything after the file read happens in libtoolame_dab_hip.so:
//
//   file -> [gain, peak, de-interleave: tlb_ingest_host]  (src/odr-audioenc.cpp:1030-1051,1139-1152)
//        -> [encode: tlb_encode_host_len]                 (toolame_encode_frame, libtoolame-dab/toolame.c:267-554)
//        -> whole frames -> file                          (what src/odr-audioenc.cpp:1208-1225 re-frames out of the bursts)
//
// build: g++ -O2 -std=c++17 examples/mp2enc.cpp -Iinclude -Lodr-audioenc_amd -ltoolame_dab_hip -Wl,-rpath,$PWD/odr-audioenc_amd -o mp2enc
// usage: mp2enc in.s16le out.mp2 [-r rate] [-c channels] [-b kbps] [-m s|j|d|m] [-p psy] [-g gain_dB] [-n streams] [--verify] [--from-mp2 [--conceal [HOLD]]]
// --verify: every frame is read back on the device right after it was encoded (tlb_decode_host: header, CRC-16, ScF-CRC, bit budget);
// any TLB_DEC_BAD_MASK flag ends the run with exit status 3.
// --from-mp2: the input is an MPEG Layer II file, a transcode: its first header gives the feed's rate, bitrate and channel count (which are
// then the encoder's rate and channel count unless -r / -c say otherwise), the file is cut into frames by the arithmetic length and each
// header's padding bit, and the frames are decoded on the device into the ingest's input (tlb_feed_host) instead of PCM being read.
// With -r or -c another (legal) rate or channel count than the file's, the feed is an ADAPTED one (tlb_feed_set_adapted): 44.1 kHz for a
// 48 kHz encoder, stereo for mono, ...; a slot of the call then holds a frame only on the ticks tlb_feed_want_at says want one.
// A 48, 44.1 or 32 kHz file with -r 24000 is a DOWN FEED (tlb_feed_down_set): a tick has two slots and takes the one or two frames
// tlb_feed_down_want_at asks for; the device decodes, filters and decimates them (tlb_feed_down_host).
// --conceal [HOLD] (with --from-mp2): feed concealment, step 3: a frame of the file that does not pass goes in as the last good frame
// once more, 6 dB quieter per lost frame, for HOLD frames (default 4), then the filterbank rings out -- not as silence.  At the file's own
// rate and channel count that is tlb_conceal_enable; with -r or -c (an adapted or a down feed) it is tlb_feed_loss_enable, which conceals
// the feed's WANTED slots ahead of the resampler or decimator.  One more line at the end: stream 0's record.
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "toolame_batch.h"

static void die(const char *what, int code)
{
    std::fprintf(stderr, "mp2enc: %s (code %d)\n", what, code);
    std::exit(1);
}

int main(int argc, char **argv)
{
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s in.s16le out.mp2 [-r rate] [-c channels] [-b kbps] [-m mode] [-p psy] [-g gain_dB] [-n streams] [--verify] [--from-mp2 [--conceal [HOLD]]]\n", argv[0]);
        return 2;
    }
    long rate = 48000;
    int channels = 2, kbps = 128, psy = 1, nstreams = 1;
    char mode = 0;
    double gain_db = 0.0;
    bool verify = false, from_mp2 = false, rate_given = false, channels_given = false;
    int conceal = 0;
    for (int i = 3; i < argc; i += 2) {
        const std::string k = argv[i];
        if (k == "--verify") { verify = true; i -= 1; continue; }
        if (k == "--from-mp2") { from_mp2 = true; i -= 1; continue; }
        if (k == "--conceal") {                              // HOLD is taken when the next argument is a number
            conceal = 4;
            char *end = nullptr;
            const long v = i + 1 < argc ? std::strtol(argv[i + 1], &end, 10) : 0;
            if (i + 1 < argc && end != argv[i + 1] && !*end) conceal = (int)v; else i -= 1;
            if (conceal < 1 || conceal > TLB_CONCEAL_MAX_HOLD) die("--conceal HOLD: 1..16", conceal);
            continue;
        }
        if (i + 1 >= argc) die("option without a value", 0);
        const char *v = argv[i + 1];
        if (k == "-r") { rate = std::atol(v); rate_given = true; }
        else if (k == "-c") { channels = std::atoi(v); channels_given = true; }
        else if (k == "-b") kbps = std::atoi(v);
        else if (k == "-m") mode = v[0];
        else if (k == "-p") psy = std::atoi(v);
        else if (k == "-g") gain_db = std::atof(v);
        else if (k == "-n") nstreams = std::atoi(v);
        else die("unknown option", 0);
    }
    if (nstreams < 1) die("streams", nstreams);

    // the whole input: PCM cut to whole frames of 1152 samples per channel, or (--from-mp2) Layer II frames
    std::FILE *fi = std::fopen(argv[1], "rb");
    if (!fi) die("cannot open input", 0);
    std::vector<int16_t> in;
    std::vector<uint8_t> mp2;
    if (from_mp2) {
        uint8_t buf[1 << 15];
        size_t n;
        while ((n = std::fread(buf, 1, sizeof buf, fi)) > 0) mp2.insert(mp2.end(), buf, buf + n);
    } else {
        int16_t buf[1 << 15];
        size_t n;
        while ((n = std::fread(buf, sizeof(int16_t), sizeof buf / sizeof buf[0], fi)) > 0) in.insert(in.end(), buf, buf + n);
    }
    std::fclose(fi);
    tlb_feed_config feed = {0, 0, 0};
    std::vector<size_t> fpos, flen;                           // --from-mp2: where each frame lies in the file
    std::vector<long> tick_frame;                             // ... and the frame tick f's slot holds (-1: none is wanted on that tick)
    std::vector<int> tick_want;                               // a down feed: the frames tick f holds, tick_frame[f] being the first
    bool down = false;                                        // the file's rate is above the encoder's: a down feed
    if (from_mp2) {
        if (mp2.size() < 4 || mp2[0] != 0xff || (mp2[1] & 0xf6) != 0xf4) die("the input does not begin with a Layer II header", 0);
        const int lsf = !(mp2[1] & 0x08), bi = mp2[2] >> 4, fi2 = (mp2[2] >> 2) & 3;
        static const int kb[2][16] = {{0, 32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 0}, {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160, 0}};
        static const long fs[2][4] = {{44100, 48000, 32000, 0}, {22050, 24000, 16000, 0}};
        feed = tlb_feed_config{fs[lsf][fi2], kb[lsf][bi], (mp2[3] >> 6) == 3 ? 1 : 2};
        if (tlb_feed_check_config(&feed) != TLB_OK) die("the input's first header names no legal Layer II configuration", tlb_feed_check_config(&feed));
        if (!rate_given) rate = feed.samplerate;
        if (!channels_given) channels = feed.channels;
        const size_t base = (size_t)tlb_feed_frame_bytes(&feed);
        for (size_t o = 0; o + 4 <= mp2.size();) {            // the sync word, the arithmetic length, one more with the padding bit
            if (mp2[o] != 0xff || (mp2[o + 1] & 0xf0) != 0xf0) die("the input has no sync word where a frame should begin, at byte", (int)o);
            const size_t n = base + ((mp2[o + 2] >> 1) & 1u);
            if (o + n > mp2.size()) break;
            fpos.push_back(o); flen.push_back(n);
            o += n;
        }
        down = feed.samplerate > rate;
        for (long f = 0, k = 0; down; f++) {                  // one tick per 1152 OUTPUT frames, one or two frames each, until a wanted frame is not there
            const int w = tlb_feed_down_want_at(feed.samplerate, rate, f);
            if (w < 0) die("the input's rate and -r form no legal pair", -w);
            if (k + w > (long)fpos.size()) break;
            tick_frame.push_back(k); tick_want.push_back(w);
            k += w;
        }
        for (long f = 0, k = 0; !down; f++) {                 // one tick per 1152 OUTPUT frames, until a wanted frame is not there
            const int w = tlb_feed_want_at(feed.samplerate, rate, f);
            if (w < 0) die("the input's rate and -r form no legal pair", -w);
            if (w && k == (long)fpos.size()) break;
            tick_frame.push_back(w ? k++ : -1);
        }
    }
    if (!mode) mode = channels == 1 ? 'm' : 'j';             // odr-audioenc's defaults (src/odr-audioenc.cpp:697-709)
    if (channels != 1 && channels != 2) die("1 or 2 channels", channels);
    const size_t per_frame = 1152u * (size_t)channels;
    const int nframes = from_mp2 ? (int)tick_frame.size() : (int)(in.size() / per_frame);
    if (nframes == 0) die("input shorter than one frame", 0);

    std::vector<tlb_stream_config> cfg((size_t)nstreams, tlb_stream_config{rate, mode, kbps, psy, 0});
    int err = 0;
    tlb_batch *enc = tlb_create(0, nstreams, cfg.data(), &err);
    if (!enc) die("tlb_create", err);
    if (gain_db != 0.0 && (err = tlb_set_gain_db(enc, -1, gain_db)) != TLB_OK) die("tlb_set_gain_db", err);

    const bool adapt = from_mp2 && !down && (rate != feed.samplerate || channels != feed.channels);
    if (down && (err = tlb_feed_down_set(enc, -1, &feed)) != TLB_OK) die("tlb_feed_down_set", err);
    if (from_mp2 && !adapt && !down && (err = tlb_feed_set(enc, -1, &feed)) != TLB_OK) die("tlb_feed_set", err);
    if (adapt && (err = tlb_feed_set_adapted(enc, -1, &feed)) != TLB_OK) die("tlb_feed_set_adapted", err);
    if (conceal && !from_mp2) die("--conceal needs --from-mp2 (a Layer II feed to conceal)", 0);
    if (conceal && !(adapt || down) && (err = tlb_conceal_enable(enc, -1, conceal, 3)) != TLB_OK) die("tlb_conceal_enable", err);
    if (conceal && (adapt || down) && (err = tlb_feed_loss_enable(enc, -1, conceal, 3)) != TLB_OK) die("tlb_feed_loss_enable", err);     // -r / -c: the feed's WANTED slots
    const int fstride = down ? tlb_feed_down_stride(enc) : tlb_feed_stride(enc);
    const size_t per_tick = down ? 2 : 1;                     // feed slots per stream and tick

    const int stride = tlb_out_stride(enc);
    std::FILE *fo = std::fopen(argv[2], "wb");
    if (!fo) die("cannot open output", 0);

    const int chunk = 256;                                    // frames per call
    std::vector<int16_t> inter((size_t)chunk * nstreams * 2304), pcm((size_t)chunk * nstreams * 2304), peaks((size_t)chunk * nstreams * 2);
    std::vector<uint8_t> out((size_t)chunk * nstreams * stride);
    std::vector<int32_t> len((size_t)chunk * nstreams);
    std::vector<uint8_t> ffr(from_mp2 ? (size_t)chunk * nstreams * per_tick * fstride : 0);
    std::vector<int32_t> fln(from_mp2 ? (size_t)chunk * nstreams * per_tick : 0);
    long bad_feed = 0;
    std::vector<tlb_frame_report> frep(from_mp2 ? (size_t)chunk * nstreams * per_tick : 0);
    long written = 0, checked = 0;
    std::vector<tlb_frame_report> report(verify ? (size_t)chunk * nstreams : 0);
    // TEST-ONLY hook of this example (tests/test_decode_gpu.py): a byte offset into the first call's frame buffer, flipped before the check
    const char *corrupt = std::getenv("MP2ENC_TEST_CORRUPT");
    auto check = [&](const uint8_t *frames, const int32_t *lens, int nf) {
        if ((err = tlb_decode_host(enc, frames, lens, nf, report.data(), nullptr, nullptr)) != TLB_OK) die("tlb_decode_host", err);
        for (size_t i = 0; i < (size_t)nf * nstreams; i++) {
            if (report[i].status & TLB_DEC_BAD_MASK) {
                std::fprintf(stderr, "mp2enc: verify failed: frame slot %zu, status 0x%x (CRC-16 stored %04x, computed %04x)\n", i, report[i].status,
                             report[i].crc_stored, report[i].crc_computed);
                std::exit(3);
            }
            checked += !(report[i].status & TLB_DEC_EMPTY);
        }
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (int f0 = 0; f0 < nframes; f0 += chunk) {
        const int nf = nframes - f0 < chunk ? nframes - f0 : chunk;
        for (int f = 0; f < nf; f++)                         // every stream of the batch gets the same programme
            for (int s = 0; s < nstreams; s++) {
                const size_t slot = (size_t)f * nstreams + s;
                if (down) {
                    for (size_t j = 0; j < 2; j++) {
                        const long k = tick_frame[(size_t)(f0 + f)] + (long)j;
                        const bool on = (int)j < tick_want[(size_t)(f0 + f)];
                        fln[2 * slot + j] = on ? (int32_t)flen[(size_t)k] : 0;
                        if (on) std::memcpy(&ffr[(2 * slot + j) * fstride], &mp2[fpos[(size_t)k]], flen[(size_t)k]);
                    }
                } else if (from_mp2) {
                    const long k = tick_frame[(size_t)(f0 + f)];
                    fln[slot] = k < 0 ? 0 : (int32_t)flen[(size_t)k];
                    if (k >= 0) std::memcpy(&ffr[slot * fstride], &mp2[fpos[(size_t)k]], flen[(size_t)k]);
                } else std::memcpy(&inter[slot * 2304], &in[(size_t)(f0 + f) * per_frame], per_frame * sizeof(int16_t));
            }
        if (down) {                                          // decode, filter and decimate, into what the ingest reads
            if ((err = tlb_feed_down_host(enc, ffr.data(), fln.data(), inter.data(), frep.data(), nf)) != TLB_OK) die("tlb_feed_down_host", err);
            for (size_t i = 0; i < (size_t)nf * nstreams; i += (size_t)nstreams) bad_feed += ((frep[2 * i].status | frep[2 * i + 1].status) & TLB_DEC_BAD_MASK) != 0;
        } else if (from_mp2) {                               // the decode, into what the ingest reads; a frame that does not pass goes in as silence
            if ((err = tlb_feed_host(enc, ffr.data(), fln.data(), nf, inter.data(), frep.data())) != TLB_OK) die("tlb_feed_host", err);
            // (stream 0's reports stand for all: every stream of the batch is given the same file)
            for (size_t i = 0; i < (size_t)nf * nstreams; i += (size_t)nstreams) bad_feed += (frep[i].status & TLB_DEC_BAD_MASK) != 0;
        }
        if ((err = tlb_ingest_host(enc, inter.data(), nf, pcm.data(), peaks.data())) != TLB_OK) die("tlb_ingest_host", err);
        if ((err = tlb_encode_host_len(enc, pcm.data(), nf, nullptr, nullptr, out.data(), len.data(), nullptr)) != TLB_OK) die("tlb_encode_host_len", err);
        if (verify) {
            if (corrupt && f0 == 0 && (size_t)std::atol(corrupt) < out.size()) out[(size_t)std::atol(corrupt)] ^= 0x10;
            check(out.data(), len.data(), nf);
        }
        for (int f = 0; f < nf; f++) {                       // stream 0 goes to the file; slot f = the frame before input frame f (length 0: none yet)
            const size_t slot = (size_t)f * nstreams;
            if (len[slot] > 0) { std::fwrite(&out[slot * stride], 1, (size_t)len[slot], fo); written += len[slot]; }
        }
    }
    {   // toolame_finish(): the frame that is still pending
        std::vector<uint8_t> last((size_t)nstreams * stride);
        std::vector<int32_t> llen((size_t)nstreams);
        if ((err = tlb_flush_host_len(enc, last.data(), llen.data())) != TLB_OK) die("tlb_flush_host_len", err);
        if (verify) check(last.data(), llen.data(), 1);
        if (llen[0] > 0) { std::fwrite(last.data(), 1, (size_t)llen[0], fo); written += llen[0]; }
    }
    const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    std::fclose(fo);
    std::fprintf(stderr, "mp2enc: %d frames x %d stream(s) in %.3f s = %.0f frames/s (%.0f x real time per stream); %ld bytes written; %s\n",
                 nframes, nstreams, dt, (double)nframes * nstreams / dt, (double)nframes * 1152.0 / (double)rate / dt, written, tlb_version());
    if (from_mp2) std::fprintf(stderr, "mp2enc: transcoded from %ld Hz, %d kbps, %d channel(s): %zu frames, %ld did not pass and went in as silence\n",
                               feed.samplerate, feed.bitrate, feed.channels, fpos.size(), bad_feed);
    if (conceal) {
        std::vector<tlb_conceal_record> rec((size_t)nstreams);
        if ((err = tlb_conceal_records_host(enc, rec.data())) != TLB_OK) die("tlb_conceal_records_host", err);
        std::fprintf(stderr, "mp2enc: conceal: %u slots, %u passed, %u concealed, %u muted, %u runs, longest %u\n", rec[0].frames, rec[0].passed, rec[0].concealed,
                     rec[0].muted, rec[0].runs, rec[0].longest);
    }
    if (verify) std::fprintf(stderr, "mp2enc: verify ok: %ld frames read back on the device, %ld bad\n", checked, tlb_decode_bad_frames(enc));
    tlb_destroy(enc);
    return 0;
}
