// mp2_feed_down_san_main.cpp -- TEST-ONLY driver of the down-feed emulation (mp2_feed_down_emu.cpp) as a program of its own, so that it can
// be linked with AddressSanitizer + UBSan (tests/feeddownlib.py builds it; nothing is preloaded into anything).  Reads a case file, runs
// every case's calls on a reset object, writes every result to the output file; the test compares them with the plain build's.
//   case file: int32 nstreams, ncases; per stream int64 samplerate, int32 kbps, channels (0: no down feed), int64 stream rate, int32 stream channels;
//              per case int32 ncalls; per call int32 nframes; uint8 frames[nframes][nstreams][2][stride]; int32 len[nframes][nstreams][2]
//   output:    per call report[nframes][nstreams][2], pcm[nframes][nstreams][2304] (every sample 0x1111 before the call)
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" {
void *fd_create(int nstreams, const long *fs, const int *kbps, const int *channels, const long *enc_rate, const int *enc_nch, int *err);
void fd_destroy(void *h);
int fd_stride(void *h);
int fd_sizeof_report(void);
int fd_reset(void *h, int s);
int fd_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, void *report);
}

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t ns, ncases;
    rd(fi, &ns, 4); rd(fi, &ncases, 4);
    std::vector<long> fs((size_t)ns), er((size_t)ns);
    std::vector<int> kbps((size_t)ns), ch((size_t)ns), en((size_t)ns);
    for (int s = 0; s < ns; s++) {
        int64_t r; int32_t v[2];
        rd(fi, &r, 8); rd(fi, v, 8);
        fs[(size_t)s] = (long)r; kbps[(size_t)s] = v[0]; ch[(size_t)s] = v[1];
        rd(fi, &r, 8); rd(fi, v, 4);
        er[(size_t)s] = (long)r; en[(size_t)s] = v[0];
    }
    int err = 0;
    void *h = fd_create(ns, fs.data(), kbps.data(), ch.data(), er.data(), en.data(), &err);
    if (!h) return 3;
    const size_t stride = (size_t)fd_stride(h);
    for (int k = 0; k < ncases; k++) {
        int32_t ncalls;
        rd(fi, &ncalls, 4);
        fd_reset(h, -1);
        for (int c = 0; c < ncalls; c++) {
            int32_t nf;
            rd(fi, &nf, 4);
            const size_t ticks = (size_t)nf * (size_t)ns, slots = 2 * ticks;
            // exactly as long as the data: a read past a slot's end, or past the last slot, is a read past the allocation
            std::vector<uint8_t> frames(slots * stride), report(slots * (size_t)fd_sizeof_report());
            std::vector<int32_t> len(slots);
            std::vector<int16_t> pcm(ticks * 2304, (int16_t)0x1111);
            rd(fi, frames.data(), frames.size());
            rd(fi, len.data(), 4 * slots);
            if (fd_decode(h, frames.data(), len.data(), nf, pcm.data(), report.data())) return 4;
            fwrite(report.data(), 1, report.size(), fo); fwrite(pcm.data(), 2, pcm.size(), fo);
        }
    }
    fd_destroy(h);
    fclose(fi);
    if (fclose(fo)) return 5;
    puts("sanitized ok");
    return 0;
}
