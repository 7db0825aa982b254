// mp2_dec_san_main.cpp -- TEST-ONLY driver of the decode emulation (mp2_dec_emu.cpp) as a program of its own, so that it can be linked
// with AddressSanitizer + UBSan (tests/test_decode_emu.py builds it; nothing is preloaded into anything).  Reads a case file, decodes every
// batch in it on a reset decoder with fields and PCM, writes every result to the output file; the test compares them with the plain build's.
//   case file: int32 nstreams, ncases; per stream int64 samplerate, int32 mode, kbps, psy, pad_len;
//              per case int32 nframes, has_len; uint8 frames[nframes][nstreams][stride]; int32 len[nframes][nstreams] if has_len
//   output:    per case report[nframes][nstreams], fields[..], pcm[..][2][1152]
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

extern "C" {
void *dec_create(int nstreams, const long *fs, const char *mode, const int *kbps, const int *psy, const int *pad, int *err);
void dec_destroy(void *h);
int dec_out_stride(void *h);
int dec_sizeof_report(void);
int dec_sizeof_fields(void);
int dec_reset(void *h, int s);
int dec_decode(void *h, const uint8_t *frames, const int32_t *len, int nframes, void *report, void *fields, int16_t *pcm);
}

static void rd(FILE *f, void *p, size_t n) { if (n && fread(p, 1, n, f) != n) { fprintf(stderr, "short case file\n"); exit(2); } }

int main(int argc, char **argv)
{
    if (argc != 3) return 2;
    FILE *fi = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
    if (!fi || !fo) return 2;
    int32_t ns, ncases;
    rd(fi, &ns, 4); rd(fi, &ncases, 4);
    std::vector<long> fs((size_t)ns);
    std::vector<char> mode((size_t)ns);
    std::vector<int> kbps((size_t)ns), psy((size_t)ns), pad((size_t)ns);
    for (int s = 0; s < ns; s++) {
        int64_t r; int32_t v[4];
        rd(fi, &r, 8); rd(fi, v, 16);
        fs[(size_t)s] = (long)r; mode[(size_t)s] = (char)v[0]; kbps[(size_t)s] = v[1]; psy[(size_t)s] = v[2]; pad[(size_t)s] = v[3];
    }
    int err = 0;
    void *h = dec_create(ns, fs.data(), mode.data(), kbps.data(), psy.data(), pad.data(), &err);
    if (!h) return 3;
    const size_t stride = (size_t)dec_out_stride(h);
    for (int k = 0; k < ncases; k++) {
        int32_t nf, has_len;
        rd(fi, &nf, 4); rd(fi, &has_len, 4);
        const size_t slots = (size_t)nf * (size_t)ns;
        // exactly as long as the data: a read past a slot's end, or past the last slot, is a read past the allocation
        std::vector<uint8_t> frames(slots * stride), report(slots * (size_t)dec_sizeof_report()), fields(slots * (size_t)dec_sizeof_fields());
        std::vector<int32_t> len(has_len ? slots : 0);
        std::vector<int16_t> pcm(slots * 2304);
        rd(fi, frames.data(), frames.size());
        if (has_len) rd(fi, len.data(), 4 * slots);
        dec_reset(h, -1);
        if (dec_decode(h, frames.data(), has_len ? len.data() : nullptr, nf, report.data(), fields.data(), pcm.data())) return 4;
        fwrite(report.data(), 1, report.size(), fo); fwrite(fields.data(), 1, fields.size(), fo); fwrite(pcm.data(), 2, pcm.size(), fo);
    }
    dec_destroy(h);
    fclose(fi);
    if (fclose(fo)) return 5;
    puts("sanitized ok");
    return 0;
}
