// mp2_conceal_san_main.cpp -- TEST-ONLY driver of the concealment emulation (mp2_conceal_emu.cpp) as a program of its own, so that it can be
// linked with AddressSanitizer + UBSan (tests/conceallib.py builds it; nothing is preloaded into anything).  Reads a case file, runs its calls
// as ONE run from the reset, writes every result to the output file; the test compares them with the plain build's.
//   case file: int32 nstreams, ncalls; per stream int64 samplerate, int32 kbps, channels (0: no feed), hold (0: no concealment), step;
//              per call int32 nframes; uint8 frames[nframes][nstreams][stride]; int32 len[nframes][nstreams]
//   output:    per call report[nframes][nstreams], pcm[nframes][nstreams][2304] (every sample 0x1111 before the call); then the records
//              [nstreams][8] uint32 and int32 conceal_guard_ok
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" {
void *conceal_create(int nstreams, const long *fs, const int *kbps, const int *channels, const int *hold, const int *step, int *err);
void conceal_destroy(void *h);
int conceal_stride(void *h);
int conceal_sizeof_report(void);
void conceal_records(void *h, void *out);
int conceal_guard_ok(void *h);
int conceal_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, void *report);
}

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t ns, ncalls;
    rd(fi, &ns, 4); rd(fi, &ncalls, 4);
    std::vector<long> fs((size_t)ns);
    std::vector<int> kbps((size_t)ns), ch((size_t)ns), hold((size_t)ns), step((size_t)ns);
    for (int s = 0; s < ns; s++) {
        int64_t r; int32_t v[4];
        rd(fi, &r, 8); rd(fi, v, 16);
        fs[(size_t)s] = (long)r; kbps[(size_t)s] = v[0]; ch[(size_t)s] = v[1]; hold[(size_t)s] = v[2]; step[(size_t)s] = v[3];
    }
    int err = 0;
    void *h = conceal_create(ns, fs.data(), kbps.data(), ch.data(), hold.data(), step.data(), &err);
    if (!h) return 3;
    const size_t stride = (size_t)conceal_stride(h);
    for (int c = 0; c < ncalls; c++) {
        int32_t nf;
        rd(fi, &nf, 4);
        const size_t slots = (size_t)nf * (size_t)ns;
        // exactly as long as the data: a read past a slot's end, or past the last slot, is a read past the allocation
        std::vector<uint8_t> frames(slots * stride), report(slots * (size_t)conceal_sizeof_report());
        std::vector<int32_t> len(slots);
        std::vector<int16_t> pcm(slots * 2304, (int16_t)0x1111);
        rd(fi, frames.data(), frames.size());
        rd(fi, len.data(), 4 * slots);
        if (conceal_decode(h, frames.data(), len.data(), nf, pcm.data(), report.data())) return 4;
        fwrite(report.data(), 1, report.size(), fo); fwrite(pcm.data(), 2, pcm.size(), fo);
    }
    std::vector<uint32_t> rec((size_t)ns * 8);
    conceal_records(h, rec.data());
    const int32_t guard = conceal_guard_ok(h);
    fwrite(rec.data(), 4, rec.size(), fo); fwrite(&guard, 4, 1, fo);
    conceal_destroy(h);
    fclose(fi);
    if (fclose(fo)) return 5;
    puts("sanitized ok");
    return 0;
}
