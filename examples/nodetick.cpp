// nodetick -- a FLEET of services on one host: what AudioEnc::run() (src/odr-audioenc.cpp:819-1276) does for one service, done for
// N streams spread over the machine's GPUs through the node level of the C-ABI (include/toolame_batch.h part 3, tlb_node_*).
// Host code only (plain C++); the partition, the per-GPU threads and objects, and the counters live in libtoolame_dab_hip.so.
//
//   per tick (24 ms of audio):                                          reference, one service            this program, N services
//     1. every service's PCM into its slot of the pinned input set      inputs -> queue (:904-986)        tlb_node_parallel(fill)  (one thread per GPU block)
//     2. gain / peak / de-interleave, encode, re-frame, EDI AF packets  :1030-1051,1139-1163,1208-1225    tlb_node_submit / tlb_node_wait
//                                                                       + Outputs.cpp:194-261
//     3. ship the packets                                               EDI::write_frame -> sender        tlb_node_parallel(ship)  (here: hash + count)
//   two ticks are kept in flight: while tick t's packets are shipped, tick t+1 is on the GPUs and tick t+2's PCM is being filled.
//
// build: g++ -O2 -std=c++17 examples/nodetick.cpp -Iinclude -Lodr-audioenc_amd -ltoolame_dab_hip -Wl,-rpath,$PWD/odr-audioenc_amd -o nodetick
// usage: nodetick in.s16le [-n streams] [-G shards] [-d dev,dev,...] [-k ticks] [-r rate] [-b kbps] [-p psy] [-o out.af] [--deadline-ms D]
//                 [--short-every N --short-by M] [--monitor check|audio] [--compare] [--loudness] [--lra] [--truepeak [DBTP]] [--limit [DBTP] --limit-release MS] [--source-rate R]
//   in.s16le: interleaved stereo at the services' rate (-r: 48000, the default, or 24000); stream s starts reading at frame s (so the
//   services differ), wrapping around.
//   -d: HIP device of each shard (default 0,1,...,G-1 modulo the device count; "0,0" = two shards on one GPU).
//   -o: the AF packets of the LAST stream of the node, length-prefixed (uint32 LE) -- the stream farthest from shard 0.
//   --deadline-ms: the node's tick deadline (include/toolame_batch.h, TICK DEADLINE): a shard that misses it goes off air on its own
//   while the others tick on, and comes back by itself; each shard's late / missed / dropped counts go to stderr at the end.
//   --short-every N --short-by M: short reads (src/odr-audioenc.cpp:335-373,910-935): on every Nth tick every Nth service delivers M
//   sample frames fewer than 1152; the total of short reads and the longest time without a full read go to stderr at the end.
//   --monitor check|audio: the confidence monitor (tlb_node_enable_monitor): every frame that leaves is checked on its GPU (audio: also
//   decoded); one summary line at the end -- frames checked, bad frames, longest bad run over all services, services whose decoded output
//   is silent -- and a non-zero exit status when any frame was bad.
//   --feed-drop-every N --feed-drop-run M (with --feed): the last M of every N WANTED slots of every service (on a strict feed: ticks) stay empty -- lost packets.
//   --conceal [HOLD] --conceal-step N (with --feed; tlb_node_enable_feed_loss with --feed-rate / --feed-channels and for a down feed, where a
//   dropped frame is a WANTED slot left empty): feed concealment (tlb_node_enable_conceal): a lost frame is the last good one once more,
//   N scalefactor-index units (default 3: 6 dB) quieter per lost frame, for HOLD frames (default 4), then the filterbank rings out.  One line
//   at the end: the services' records summed -- slots, passed, concealed, muted, loss runs, the longest run.
//   --feed FILE.mp2 --feed-bitrate K: the services' source is an MPEG Layer II file (the services' rate, two channels, K kbps) decoded on the GPUs ahead
//   of the ingest (tlb_node_set_feed): the file is cut into frames by the arithmetic length and each header's padding bit, service s takes
//   frame (tick + s) of it, wrapping round; no PCM crosses the link and in.s16le is not opened (give "-").  Not together with --short-every
//   or --source-rate.  --feed-rate R, --feed-channels C: the file is at another (legal) rate or channel count than the services', an ADAPTED
//   feed (tlb_node_set_feed_adapted): a service's slot gets its next frame only on the ticks tlb_node_feed_want says want one.  R above the
//   rate of 24000 Hz services (48000, 44100, 32000) is a DOWN FEED (tlb_node_set_down_feed): a service's two slots get its next one or two
//   frames, as tlb_node_down_feed_want says.
//   --source-rate R: in.s16le is at R Hz (44100 or 32000) and is resampled to 48 kHz on the GPUs (tlb_node_set_source): service s starts
//   reading at source frame 1152 s and takes tlb_node_need() consecutive frames every tick, wrapping around.  Not together with --short-every.
//   With -r 24000, R = 48000, 44100 or 32000 is a DOWN source (tlb_node_set_down_source): the tlb_node_down_need() frames of a tick go into
//   the service's wide slot (tlb_node_down) and are filtered and decimated on the GPUs.
//   --loudness: the loudness meter (tlb_node_enable_loudness): the PCM every encoder is given is measured on its GPU after ITU-R BS.1770-4 /
//   EBU R 128.  One line per service at the end: momentary, short-term and integrated loudness in LUFS (-inf where there is none yet).
//   --lra: the loudness range on top of it (tlb_node_enable_lra; implies --loudness): EBU Tech 3342's LRA from the short-term values.  One
//   more line per service behind the loudness lines: LRA in LU, the 10th and the 95th percentile in LUFS, gated of counted blocks.
//   --truepeak [DBTP]: the true-peak meter (tlb_node_enable_truepeak): the same PCM oversampled four times on its GPU after ITU-R BS.1770-4
//   Annex 2, against a ceiling of DBTP (default -1, EBU R 128's).  One line per service at the end: the maximum true peak in dBTP, the
//   largest sample in dBFS and the number of frames over the ceiling.
//   --compare: the compare monitor on top of it (tlb_node_enable_compare with the header's default params; implies --monitor audio): every
//   frame that leaves is decoded on its GPU and set against the audio that went in.  A service whose mismatch_run reaches 3 is printed when
//   it does; one summary line at the end -- frames compared, judged, mismatched -- and exit status 4 when any service got there.
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
    std::fprintf(stderr, "nodetick: %s (code %d)\n", what, code);
    std::exit(1);
}

struct Ctx {
    tlb_node *nd;
    const std::vector<int16_t> *pcm;                         // the whole input file
    size_t nframes_in;
    long tick;
    std::vector<uint64_t> *hash;                             // per shard: FNV-1a over every packet byte shipped
    std::vector<long> *packets, *bytes;
    int short_every, short_by;                               // 0: every read is full
    long source_rate;                                        // 0: the file is at the encoder's rate
    bool down;                                               // --source-rate above the services' rate: through the wide slots and the decimator
    std::vector<size_t> *spos;                               // --source-rate: the next source frame of every service
    const std::vector<uint8_t> *mp2;                         // --feed: the file and where its frames lie (NULL: PCM input)
    const std::vector<size_t> *fpos, *flen;
    std::vector<size_t> *fcur;                               // --feed-rate / --feed-channels (an adapted feed): the next frame of every service; NULL: a strict feed
    bool down_feed;                                          // --feed-rate above the services' rate: two slots per tick, one or two frames as the schedule says
    int drop_every, drop_run;                                // --feed-drop-every / --feed-drop-run; 0: no tick's packets are lost
};

// step 1 on shard `g`'s thread: the block's services copy their frame of this tick into the pinned input set
static void fill(void *vctx, int g, int first, int n)
{
    Ctx &c = *(Ctx *)vctx;
    for (int s = first; s < first + n && c.down_feed; s++) {    // a down feed: the service's next one or two frames into its two slots
        uint8_t *slot = tlb_node_down_feed(c.nd, s);
        int32_t *len = tlb_node_down_feed_len(c.nd, s);
        if (!slot || !len) {
            if (tlb_node_shard_status(c.nd, g, nullptr) != TLB_SHARD_OK) return;
            die("no down-feed set free", s);
        }
        const size_t stride = (size_t)tlb_node_down_feed_stride(c.nd, s);
        for (int j = 0; j < tlb_node_down_feed_want(c.nd, s); j++) {
            const size_t k = (*c.fcur)[(size_t)s]++, f = k % c.fpos->size();      // the service's wanted slot k - s
            if (c.drop_every && (k - (size_t)s) % (size_t)c.drop_every >= (size_t)(c.drop_every - c.drop_run)) continue;       // its packets are lost: the slot stays empty, the file advances
            std::memcpy(slot + stride * (size_t)j, c.mp2->data() + (*c.fpos)[f], (*c.flen)[f]);
            len[j] = (int32_t)(*c.flen)[f];                          // untouched, it reads 0: an empty slot
        }
    }
    if (c.down_feed) return;
    for (int s = first; s < first + n && c.mp2; s++) {          // --feed: the service's frame of this tick into its slot of the pinned feed set
        uint8_t *slot = tlb_node_feed(c.nd, s);
        int32_t *len = tlb_node_feed_len(c.nd, s);
        if (!slot || !len) {
            if (tlb_node_shard_status(c.nd, g, nullptr) != TLB_SHARD_OK) return;
            die("no feed set free", s);
        }
        size_t f = ((size_t)s + (size_t)c.tick) % c.fpos->size(), k = (size_t)c.tick;      // k: the service's wanted slot, on a strict feed the tick
        if (c.fcur) {                                            // an adapted feed: a frame only where this tick wants one, and the file advances only then
            if (tlb_node_feed_want(c.nd, s) <= 0) continue;
            k = (*c.fcur)[(size_t)s]++ - (size_t)s;
            f = (k + (size_t)s) % c.fpos->size();
        }
        if (c.drop_every && k % (size_t)c.drop_every >= (size_t)(c.drop_every - c.drop_run)) continue;       // this slot's packets are lost: it stays empty
        std::memcpy(slot, c.mp2->data() + (*c.fpos)[f], (*c.flen)[f]);
        *len = (int32_t)(*c.flen)[f];                            // untouched, it reads 0: an empty slot
    }
    if (c.mp2) return;
    for (int s = first; s < first + n; s++) {
        int16_t *dst = tlb_node_pcm(c.nd, s);
        if (!dst) {                                              // a BROKEN or LATE shard takes no input (its block is off air until it is back); anything else is a bug
            if (tlb_node_shard_status(c.nd, g, nullptr) != TLB_SHARD_OK) return;
            die("no input set free", s);
        }
        if (c.source_rate) {                                     // need source frames from where the service stands, around the end of the file
            const int need = c.down ? tlb_node_down_need(c.nd, s) : tlb_node_need(c.nd, s);
            if (need < 0) die("tlb_node_need", -need);
            if (c.down && !(dst = tlb_node_down(c.nd, s))) die("no wide slot free", s);      // (its shard took tlb_node_pcm a moment ago)
            const size_t total = c.pcm->size() / 2;
            size_t &at = (*c.spos)[(size_t)s];
            for (int i = 0; i < need; i++, at = (at + 1) % total) std::memcpy(dst + 2 * i, c.pcm->data() + 2 * at, 2 * sizeof(int16_t));
            continue;
        }
        const size_t f = ((size_t)s + (size_t)c.tick) % c.nframes_in;
        std::memcpy(dst, c.pcm->data() + f * 2304, 2304 * sizeof(int16_t));
        if (c.short_every && c.tick % c.short_every == 0 && s % c.short_every == 0)
            if (int32_t *valid = tlb_node_valid(c.nd, s)) *valid = 1152 - c.short_by;        // untouched, it reads 1152
    }
    (void)g;
}

// step 3 on shard `g`'s thread: a real sender would write each packet to its service's EDI destination
static void ship(void *vctx, int g, int first, int n)
{
    Ctx &c = *(Ctx *)vctx;
    uint64_t h = (*c.hash)[(size_t)g];
    for (int s = first; s < first + n; s++)
        for (int u = 0; u < tlb_node_units(c.nd, s); u++) {
            int len = 0;
            const uint8_t *p = tlb_node_packet(c.nd, s, u, &len);
            if (!p || !len) continue;
            for (int i = 0; i < len; i++) h = (h ^ p[i]) * 1099511628211ull;
            (*c.packets)[(size_t)g]++;
            (*c.bytes)[(size_t)g] += len;
        }
    (*c.hash)[(size_t)g] = h;
}

int main(int argc, char **argv)
{
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s in.s16le [-n streams] [-G shards] [-d dev,dev,...] [-k ticks] [-r rate] [-b kbps] [-p psy] [-o out.af] [--deadline-ms D] [--short-every N --short-by M] [--monitor check|audio] [--compare] [--loudness] [--lra] [--truepeak [DBTP]] [--limit [DBTP] --limit-release MS] [--source-rate R] [--feed FILE.mp2 --feed-bitrate K [--feed-rate R] [--feed-channels C]] [--conceal [HOLD] --conceal-step N] [--feed-drop-every N --feed-drop-run M]\n", argv[0]);
        return 2;
    }
    int nstreams = 64, G = 0, ticks = 50, kbps = 128, psy = 1, short_every = 0, short_by = 0, monitor = 0, compare = 0, loudness = 0, lra = 0, truepeak = 0, limit = 0, limit_release = 0;
    double ceiling_db = -1.0, limit_db = -1.0;
    long rate = 48000;
    double deadline_ms = 0;
    long source_rate = 0;
    int feed_kbps = 0, feed_channels = 2;
    long feed_rate = 0;                                      // 0: the services' own
    std::string devs, outpath, feed_path;
    int conceal = 0, conceal_step = 3, drop_every = 0, drop_run = 0;
    for (int i = 2; i < argc; i += 2) {
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
        if (k == "-n") nstreams = std::atoi(v);
        else if (k == "-G") G = std::atoi(v);
        else if (k == "-d") devs = v;
        else if (k == "-k") ticks = std::atoi(v);
        else if (k == "-r") rate = std::atol(v);
        else if (k == "-b") kbps = std::atoi(v);
        else if (k == "-p") psy = std::atoi(v);
        else if (k == "-o") outpath = v;
        else if (k == "--deadline-ms") { deadline_ms = std::atof(v); if (!(deadline_ms > 0)) die("--deadline-ms wants a positive number", 0); }
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
    if (short_every < 0 || short_by < 0 || short_by > 1152 || (short_every > 0) != (short_by > 0)) die("--short-every N --short-by M: N >= 1 and 1 <= M <= 1152, both or neither", 0);
    const int ndev = tlb_device_count();
    if (ndev <= 0) die("no GPU", ndev);
    std::vector<int> devices;
    for (size_t p = 0; p < devs.size();) {
        devices.push_back(std::atoi(devs.c_str() + p));
        p = devs.find(',', p);
        if (p == std::string::npos) break;
        p++;
    }
    if (devices.empty()) { if (G <= 0) G = ndev; for (int g = 0; g < G; g++) devices.push_back(g % ndev); }
    G = (int)devices.size();

    if (feed_path.empty() != (feed_kbps <= 0)) die("--feed FILE.mp2 --feed-bitrate K: both or neither", 0);
    if (!feed_rate) feed_rate = rate;
    tlb_feed_config feed = {feed_rate, feed_kbps, feed_channels};   // the services' own rate and channel count unless told otherwise
    const bool down_feed = !feed_path.empty() && feed_rate > rate;   // a feed above the services' rate (tlb_node_set_down_feed)
    const bool adapt = !down_feed && (feed_rate != rate || feed_channels != 2);
    if (drop_every < 0 || drop_run < 0 || drop_run > drop_every || (drop_every > 0) != (drop_run > 0)) die("--feed-drop-every N --feed-drop-run M: 1 <= M <= N, both or neither", 0);
    if ((conceal || drop_every) && feed_path.empty()) die("--conceal and --feed-drop-every need a strict --feed (the services' rate, two channels)", 0);
    std::vector<uint8_t> mp2;
    std::vector<size_t> fpos, flen;
    if (!feed_path.empty()) {
        if (int rc = tlb_feed_check_config(&feed)) die("--feed-bitrate: no legal Layer II configuration at this rate and channel count", rc);
        std::FILE *ff = std::fopen(feed_path.c_str(), "rb");
        if (!ff) die("cannot open the feed", 0);
        uint8_t buf[1 << 15];
        size_t got;
        while ((got = std::fread(buf, 1, sizeof buf, ff)) > 0) mp2.insert(mp2.end(), buf, buf + got);
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
    std::vector<int16_t> pcm;
    if (feed_path.empty()) {
        std::FILE *fi = std::fopen(argv[1], "rb");
        if (!fi) die("cannot open input", 0);
        int16_t buf[2304];
        while (std::fread(buf, sizeof(int16_t), 2304, fi) == 2304) pcm.insert(pcm.end(), buf, buf + 2304);
        std::fclose(fi);
    }
    const size_t nframes_in = pcm.size() / 2304;
    if (feed_path.empty() && !nframes_in) die("input shorter than one frame", 0);

    // the fleet: every service joint stereo (odr-audioenc's default mode, src/odr-audioenc.cpp:697-709) at 48 kHz unless told otherwise
    std::vector<tlb_stream_config> cfg((size_t)nstreams, tlb_stream_config{rate, 'j', kbps, psy, 0});
    static const char version[] = "nodetick example";
    tlb_node_config nc;
    std::memset(&nc, 0, sizeof nc);
    nc.plane = TLB_NODE_TICK;
    nc.tick.egress = TLB_TICK_EDI_AF;
    nc.tick.version = version; nc.tick.version_len = (int)std::strlen(version);
    nc.tick.now_s = 1712345678; nc.tick.tist = 1; nc.tick.tai_utc_offset = 37;
    for (int g = 0; g < G; g++) {                                // what each GPU will hold, before any of them is touched
        int first, n, ncfg, lists[4], pairs;
        if (int rc = tlb_node_plan_shard(nstreams, cfg.data(), G, g, &first, &n, &ncfg, lists, &pairs)) die("illegal configuration", rc);
        std::fprintf(stderr, "nodetick: shard %d on device %d: streams [%d, %d), %d configuration(s), kernel lists psy0/1/2+4/3 = %d/%d/%d/%d\n",
                     g, devices[(size_t)g], first, first + n, ncfg, lists[0], lists[1], lists[2], lists[3]);
    }
    int err = 0;
    tlb_node *nd = tlb_node_create(G, devices.data(), nstreams, cfg.data(), &nc, &err);
    if (!nd) die("tlb_node_create", err);
    if (deadline_ms > 0)
        if (int rc = tlb_node_set_deadline_ms(nd, deadline_ms)) die("tlb_node_set_deadline_ms", rc);
    if (short_every)
        if (int rc = tlb_node_enable_short_reads(nd)) die("tlb_node_enable_short_reads", rc);      // before the first submit
    if (loudness)
        if (int rc = tlb_node_enable_loudness(nd)) die("tlb_node_enable_loudness", rc);                 // likewise; a restarted shard measures again from zero
    if (lra)
        if (int rc = tlb_node_enable_lra(nd)) die("tlb_node_enable_lra", rc);                           // ... behind loudness
    const uint32_t ceiling = (uint32_t)std::llround(1073741824.0 * std::pow(10.0, ceiling_db / 20.0));    // in units of 2^-30 of full scale
    if (truepeak)
        if (int rc = tlb_node_enable_truepeak(nd, ceiling)) die("tlb_node_enable_truepeak", rc);        // likewise, with the same ceiling
    const tlb_limiter_params lparams = {(uint32_t)std::llround(1073741824.0 * std::pow(10.0, limit_db / 20.0)), (uint32_t)limit_release};      // release 0: the default
    if (limit)
        if (int rc = tlb_node_enable_limiter(nd, &lparams)) die("tlb_node_enable_limiter", rc);         // likewise, with the same parameters, from zero
    if (monitor)
        if (int rc = tlb_node_enable_monitor(nd, monitor)) die("tlb_node_enable_monitor", rc);          // likewise; a restarted shard is enabled again
    const bool down = source_rate > rate;
    if (source_rate && !down)
        if (int rc = tlb_node_set_source(nd, -1, source_rate)) die("tlb_node_set_source", rc);          // between steps; a restarted shard's sources are set again
    if (down)
        if (int rc = tlb_node_set_down_source(nd, -1, source_rate)) die("tlb_node_set_down_source", rc);      // likewise
    if (down_feed) { if (int rc = tlb_node_set_down_feed(nd, -1, &feed)) die("tlb_node_set_down_feed", rc); }       // between steps; a restarted shard's down feeds are set again at tick 0
    else if (!feed_path.empty())
        if (int rc = adapt ? tlb_node_set_feed_adapted(nd, -1, &feed) : tlb_node_set_feed(nd, -1, &feed)) die("tlb_node_set_feed", rc);                    // between steps; a restarted shard's feeds are set again
    if (conceal && !(adapt || down_feed))
        if (int rc = tlb_node_enable_conceal(nd, -1, conceal, conceal_step)) die("tlb_node_enable_conceal", rc);      // behind the feeds, between steps; a restarted shard's is set again
    if (conceal && (adapt || down_feed))                                 // an adapted or a down feed: its WANTED slots, ahead of the resampler or decimator
        if (int rc = tlb_node_enable_feed_loss(nd, -1, conceal, conceal_step)) die("tlb_node_enable_feed_loss", rc);
    const tlb_compare_params cparams = {TLB_COMPARE_DEFAULT_MIN_ENERGY, TLB_COMPARE_DEFAULT_CORR_NUM, TLB_COMPARE_DEFAULT_CORR_DEN};
    if (compare)
        if (int rc = tlb_node_enable_compare(nd, &cparams)) die("tlb_node_enable_compare", rc);         // after the audio monitor, before the first submit

    std::vector<uint64_t> hash((size_t)G, 1469598103934665603ull);
    std::vector<long> packets((size_t)G, 0), bytes((size_t)G, 0);
    std::vector<size_t> spos((size_t)nstreams), fcur((size_t)nstreams);
    for (int s = 0; s < nstreams; s++) fcur[(size_t)s] = (size_t)s;     // an adapted feed: service s starts s frames into the file
    for (int s = 0; s < nstreams && !pcm.empty(); s++) spos[(size_t)s] = ((size_t)s * 1152) % (pcm.size() / 2);
    Ctx ctx{nd, &pcm, nframes_in, 0, &hash, &packets, &bytes, short_every, short_by, source_rate, down, &spos, feed_path.empty() ? nullptr : &mp2, &fpos, &flen, adapt || down_feed ? &fcur : nullptr, down_feed, drop_every, drop_run};
    std::FILE *fo = outpath.empty() ? nullptr : std::fopen(outpath.c_str(), "wb");
    int alarms = 0; long taps = 0;                               // compare monitor: times a service's mismatch_run reached 3
    uint32_t longest_run = 0;                                    // confidence monitor: the longest bad run any service has shown after a tick
    auto tap = [&]() {                                           // the records of the step just waited for; -o: the last stream's packets
        if (monitor)
            for (int s = 0; s < nstreams; s++)
                if (const tlb_monitor_record *r = tlb_node_monitor(nd, s)) if (r->bad_run > longest_run) longest_run = r->bad_run;      // (NULL: its shard is down or late)
        if (compare)                                             // a run passes 3 once: a skipped or unjudged frame leaves it alone, so look at this step's flags too
            for (int s = 0; s < nstreams; s++)
                if (const tlb_compare_record *c = tlb_node_compare(nd, s))
                    if (c->mismatch_run == 3 && (c->last_flags & TLB_COMPARE_MISMATCH)) {
                        std::fprintf(stderr, "nodetick: compare: service %d (shard %d): 3 frames in a row do not sound like their input%s (step %ld)\n", s,
                                     tlb_node_shard_of(nd, s), c->last_flags & TLB_COMPARE_SWAPPED ? ", channels exchanged" : "", taps);
                        alarms++;
                    }
        taps++;
        if (!fo) return;
        const int s = nstreams - 1;
        for (int u = 0; u < tlb_node_units(nd, s); u++) {
            int len = 0;
            const uint8_t *p = tlb_node_packet(nd, s, u, &len);
            if (!p || !len) continue;
            const uint32_t n = (uint32_t)len;
            const uint8_t le[4] = {(uint8_t)n, (uint8_t)(n >> 8), (uint8_t)(n >> 16), (uint8_t)(n >> 24)};
            if (std::fwrite(le, 1, 4, fo) != 4 || std::fwrite(p, 1, n, fo) != n) die("write", 0);
        }
    };

    std::fputs(tlb_node_describe(nd), stderr);                            // which device every shard runs on (name, CUs, XCDs, PCI address, UUID)
    // A GPU that fails takes ITS block off air, not the node (include/toolame_batch.h, FAULT ISOLATION): the call in which a shard
    // breaks returns its code, every other shard has completed the call.  The caller's part: find out which shard, log why, restart it
    // when no tick is in flight -- the reference's "restart the failed input, nothing else stops" (src/odr-audioenc.cpp:875-902) one level up.
    // With --deadline-ms a shard whose tick does not complete in time goes LATE: the call returns TLB_ERR_LATE, the shard is off air
    // (skipped, NULL accessors) and comes back by itself at a later wait once its tick has returned; a late job that returns an error
    // leaves the shard broken, handled as above.
    long restarts = 0;
    auto shard_failed = [&](const char *where, int rc) {
        int alive = 0;
        for (int g = 0; g < G; g++) {
            tlb_node_shard_info info;
            const int st = tlb_node_shard_status(nd, g, &info);
            if (st == TLB_SHARD_BROKEN) std::fprintf(stderr, "nodetick: %s: shard %d on %s is down (%s)\n", where, g, info.device_name, info.what);
            else if (st == TLB_SHARD_LATE) { std::fprintf(stderr, "nodetick: %s: shard %d on %s is late (missed the %.1f ms deadline)\n", where, g, info.device_name, deadline_ms); alive++; }
            else alive++;
        }
        if (!alive) die(where, rc);                                       // nobody left: nothing to carry on with (a late shard may come back)
    };
    const auto t0 = std::chrono::steady_clock::now();
    // fill 0, submit 0; then per tick: fill t+1, submit t+1, wait t, ship t
    ctx.tick = 0;
    if (int rc = tlb_node_parallel(nd, fill, &ctx)) die("fill", rc);
    if (int rc = tlb_node_submit(nd)) shard_failed("tlb_node_submit", rc);
    bool in_flight2 = false;
    for (long t = 0; t < ticks; t++) {
        in_flight2 = false;
        if (t + 1 < ticks) {
            ctx.tick = t + 1;
            if (int rc = tlb_node_parallel(nd, fill, &ctx)) die("fill", rc);
            if (int rc = tlb_node_submit(nd)) shard_failed("tlb_node_submit", rc);
            in_flight2 = true;
        }
        if (int rc = tlb_node_wait(nd)) shard_failed("tlb_node_wait", rc);
        if (int rc = tlb_node_parallel(nd, ship, &ctx)) die("ship", rc);
        tap();
        if (!in_flight2)                                                  // no tick in flight: the moment a broken shard may come back
            for (int g = 0; g < G; g++)
                if (tlb_node_shard_status(nd, g, nullptr) == TLB_SHARD_BROKEN && tlb_node_shard_restart(nd, g, -1) == TLB_OK) restarts++;
    }
    if (int rc = tlb_node_finish(nd)) shard_failed("tlb_node_finish", rc); // toolame_finish for every service: the pending last frame
    if (int rc = tlb_node_parallel(nd, ship, &ctx)) die("ship", rc);
    tap();
    const double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();

    std::vector<tlb_node_counter> per((size_t)G);
    tlb_node_counter tot;
    tlb_node_counters(nd, per.data(), &tot);
    uint64_t all = 0;
    long npk = 0, nby = 0;
    for (int g = 0; g < G; g++) {
        std::fprintf(stderr, "nodetick: shard %d (device %d): %ld frames in %ld ticks, busy %.1f ms, %ld packets, %ld bytes\n", g, per[(size_t)g].device,
                     per[(size_t)g].frames, per[(size_t)g].steps, per[(size_t)g].busy_ns / 1e6, packets[(size_t)g], bytes[(size_t)g]);
        all ^= hash[(size_t)g] + 0x9e3779b97f4a7c15ull * (uint64_t)(g + 1);
        npk += packets[(size_t)g]; nby += bytes[(size_t)g];
    }
    if (deadline_ms > 0)
        for (int g = 0; g < G; g++) {
            tlb_node_shard_deadline dl;
            tlb_node_shard_deadline_status(nd, g, &dl);
            std::fprintf(stderr, "nodetick: shard %d: late_events %ld, missed_steps %ld, dropped_steps %ld (rejoins %ld, worst overrun %.1f ms)\n", g,
                         dl.late_events, dl.missed_steps, dl.dropped_steps, dl.rejoins, dl.worst_overrun_ms);
        }
    if (short_every) {                                                    // the reference aborts a service after 60 s without a full read (:925-931): the caller's decision here
        unsigned long total = 0; uint32_t worst = 0;
        for (int s = 0; s < nstreams; s++) { total += tlb_node_underruns(nd, s); const uint32_t ms = tlb_node_underrun_ms(nd, s); if (ms > worst) worst = ms; }
        std::fprintf(stderr, "nodetick: %lu short reads in all, longest time without a full read %u ms\n", total, worst);
    }
    if (conceal) {                                                        // the records of the last step, summed (NULL: the service's shard is down or late)
        unsigned long c[5] = {0, 0, 0, 0, 0};
        uint32_t longest = 0;
        for (int s = 0; s < nstreams; s++)
            if (const tlb_conceal_record *r = tlb_node_conceal(nd, s)) {
                c[0] += r->frames; c[1] += r->passed; c[2] += r->concealed; c[3] += r->muted; c[4] += r->runs;
                if (r->longest > longest) longest = r->longest;
            }
        std::fprintf(stderr, "nodetick: conceal: %lu slots, %lu passed, %lu concealed, %lu muted, %lu runs, longest %u\n", c[0], c[1], c[2], c[3], c[4], longest);
    }
    unsigned long checked = 0, bad = 0;
    if (monitor) {                                                        // (a restarted shard's records count from its restart)
        int silent = 0;
        for (int s = 0; s < nstreams; s++)
            if (const tlb_monitor_record *r = tlb_node_monitor(nd, s)) { checked += r->frames; bad += r->bad_frames; silent += r->out_silence_ms > 0; }
        std::fprintf(stderr, "nodetick: monitor: %lu frames checked, %lu bad, longest bad run %u, %d service(s) silent at the output\n", checked, bad, longest_run, silent);
    }
    if (compare) {
        unsigned long compared = 0, judged = 0, mismatched = 0;
        for (int s = 0; s < nstreams; s++)
            if (const tlb_compare_record *c = tlb_node_compare(nd, s)) { compared += c->frames_compared; judged += c->frames_judged; mismatched += c->mismatch_frames; }
        std::fprintf(stderr, "nodetick: compare: %lu frames compared, %lu judged, %lu mismatched, %d alarm(s)\n", compared, judged, mismatched, alarms);
    }
    if (loudness) {                                                       // the records of the last step; the gated value on request, between steps
        std::vector<tlb_loudness_programme_record> prog((size_t)nstreams);
        if (int rc = tlb_node_loudness_programme(nd, prog.data())) std::fprintf(stderr, "nodetick: tlb_node_loudness_programme (code %d)\n", rc);
        for (int s = 0; s < nstreams; s++)
            if (const tlb_loudness_record *r = tlb_node_loudness(nd, s))  // (NULL: its shard is down or late)
                std::fprintf(stderr, "nodetick: loudness: service %d: momentary %.2f LUFS, short-term %.2f LUFS, integrated %.2f LUFS (%u of %u blocks)\n", s,
                             tlb_loudness_lufs(r->momentary), tlb_loudness_lufs(r->short_term), tlb_loudness_lufs(prog[(size_t)s].integrated), prog[(size_t)s].gated, r->blocks);
    }
    if (lra) {                                                            // the range of everything measured, between steps (all zero: its shard is down or late)
        std::vector<tlb_lra_record> range((size_t)nstreams);
        if (int rc = tlb_node_lra(nd, range.data())) std::fprintf(stderr, "nodetick: tlb_node_lra (code %d)\n", rc);
        for (int s = 0; s < nstreams; s++)
            std::fprintf(stderr, "nodetick: lra: service %d: LRA %.1f LU, low %.2f LUFS, high %.2f LUFS (%u of %u blocks)\n", s, tlb_lra_lu(&range[(size_t)s]),
                         tlb_loudness_lufs(range[(size_t)s].low), tlb_loudness_lufs(range[(size_t)s].high), range[(size_t)s].gated, range[(size_t)s].blocks);
    }
    if (truepeak)                                                         // the records of the last step
        for (int s = 0; s < nstreams; s++)
            if (const tlb_truepeak_record *r = tlb_node_truepeak(nd, s)) {    // (NULL: its shard is down or late)
                const uint32_t pk = r->peak_max[0] > r->peak_max[1] ? r->peak_max[0] : r->peak_max[1];
                const uint32_t sm = r->sample_max[0] > r->sample_max[1] ? r->sample_max[0] : r->sample_max[1];
                std::fprintf(stderr, "nodetick: truepeak: service %d: max %.2f dBTP, samples %.2f dBFS, %u of %u frames over %.2f dBTP\n", s,
                             tlb_truepeak_dbtp(pk), tlb_truepeak_dbtp(sm << 15), r->overs, r->frames, tlb_truepeak_dbtp(ceiling));
            }
    if (limit)                                                            // the records of the last step
        for (int s = 0; s < nstreams; s++)
            if (const tlb_limiter_record *r = tlb_node_limiter(nd, s))        // (NULL: its shard is down or late)
                std::fprintf(stderr, "nodetick: limiter: service %d: limited %u of %u frames, red_max %u (%.2f dB), input max %.2f dBTP, ceiling %.2f dBTP\n", s,
                             r->limited, r->frames, r->red_max, r->red_max < 65536u ? 20.0 * std::log10((65536.0 - r->red_max) / 65536.0) : -INFINITY,
                             tlb_truepeak_dbtp(r->peak_in_max), tlb_truepeak_dbtp(lparams.ceiling));
    // one line for scripts: frames, packets, bytes, a hash of everything shipped (independent of G only per shard -- so print per-stream-order-free totals)
    std::printf("{\"streams\": %d, \"shards\": %d, \"ticks\": %d, \"frames\": %ld, \"packets\": %ld, \"bytes\": %ld, \"seconds\": %.4f, \"frames_per_s\": %.1f, \"realtime_x\": %.2f}\n",
                nstreams, G, ticks, tot.frames, npk, nby, sec, sec > 0 ? tot.frames / sec : 0.0, sec > 0 ? ticks * 0.024 / sec : 0.0);
    (void)all; (void)restarts;
    if (fo) std::fclose(fo);
    tlb_node_destroy(nd);
    return bad ? 3 : alarms ? 4 : 0;
}
