// mp2_conceal_conv_san_main.cpp -- TEST-ONLY driver of the emulation of the concealment on adapted and down feeds (mp2_conceal_conv_emu.cpp)
// as a program of its own, so that it can be linked with AddressSanitizer + UBSan (tests/concealconvlib.py builds it; nothing is preloaded
// into anything).  Reads a case file, runs its calls as ONE run from the reset, writes every result to the output file; the test compares
// them with the plain build's.
//   case file: int32 down, nstreams, ncalls; per stream int64 samplerate, int32 kbps, channels (0: no feed), hold (0: no concealment), step,
//              int64 the stream's rate, int32 the stream's channels; per call int32 nticks; uint8 frames[nticks][nstreams][per][stride];
//              int32 len[nticks][nstreams][per] (per: 2 slots a tick for a down feed, else 1)
//   output:    per call report[nticks][nstreams][per], pcm[nticks][nstreams][2304] (every sample 0x1111 before the call); then the records
//              [nstreams][8] uint32 and int32 ccv_guard_ok
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" {
void *ccv_create(int down, int nstreams, const long *fs, const int *kbps, const int *channels, const long *enc_rate, const int *enc_nch,
                 const int *hold, const int *step, int *err);
void ccv_destroy(void *h);
int ccv_stride(void *h);
int ccv_sizeof_report(void);
void ccv_records(void *h, void *out);
int ccv_guard_ok(void *h);
int ccv_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, int16_t *pcm, void *report);
}

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t down, ns, ncalls;
    rd(fi, &down, 4); rd(fi, &ns, 4); rd(fi, &ncalls, 4);
    std::vector<long> fs((size_t)ns), er((size_t)ns);
    std::vector<int> kbps((size_t)ns), ch((size_t)ns), hold((size_t)ns), step((size_t)ns), en((size_t)ns);
    for (int s = 0; s < ns; s++) {
        int64_t r, e; int32_t v[4], n;
        rd(fi, &r, 8); rd(fi, v, 16); rd(fi, &e, 8); rd(fi, &n, 4);
        fs[(size_t)s] = (long)r; kbps[(size_t)s] = v[0]; ch[(size_t)s] = v[1]; hold[(size_t)s] = v[2]; step[(size_t)s] = v[3];
        er[(size_t)s] = (long)e; en[(size_t)s] = n;
    }
    int err = 0;
    void *h = ccv_create(down, ns, fs.data(), kbps.data(), ch.data(), er.data(), en.data(), hold.data(), step.data(), &err);
    if (!h) return 3;
    const size_t stride = (size_t)ccv_stride(h), per = down ? 2 : 1;
    for (int c = 0; c < ncalls; c++) {
        int32_t nf;
        rd(fi, &nf, 4);
        const size_t ticks = (size_t)nf * (size_t)ns, slots = ticks * per;
        // exactly as long as the data: a read past a slot's end, or past the last slot, is a read past the allocation
        std::vector<uint8_t> frames(slots * stride), report(slots * (size_t)ccv_sizeof_report());
        std::vector<int32_t> len(slots);
        std::vector<int16_t> pcm(ticks * 2304, (int16_t)0x1111);
        rd(fi, frames.data(), frames.size());
        rd(fi, len.data(), 4 * slots);
        if (ccv_decode(h, frames.data(), len.data(), nf, pcm.data(), report.data())) return 4;
        fwrite(report.data(), 1, report.size(), fo); fwrite(pcm.data(), 2, pcm.size(), fo);
    }
    std::vector<uint32_t> rec((size_t)ns * 8);
    ccv_records(h, rec.data());
    const int32_t guard = ccv_guard_ok(h);
    fwrite(rec.data(), 4, rec.size(), fo); fwrite(&guard, 4, 1, fo);
    ccv_destroy(h);
    fclose(fi);
    if (fclose(fo)) return 5;
    puts("sanitized ok");
    return 0;
}
