// loudness_sanitize_main.cpp -- TEST-ONLY driver of the loudness emulation (mp2_loudness_emu.cpp) as a program of its own, so that it can be
// linked with AddressSanitizer + UBSan (tests/loudnesslib.py builds it; nothing is preloaded into anything).  The 37-stream set of
// tests/loudnesslib.py (every rate with one and with two channels: 74 lanes, a second wave half empty) over 45 frames of full-scale
// noise, in one call and frame by frame, and the hostile stream counts 1, 31 and 33 (a lone lane pair, one stream short of a wave, one
// past it).  The buffers are exactly as long as the data and the LDS block is a heap block of its own size, so an index past a row, the
// ring, the histogram or the LDS layout is an access past an allocation.  The two cuts must agree.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
int ld_lane_words(void);
int ld_hist_rows(void);
int ld_loudness(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const int32_t *rate, double *lane, double *ring, void *rec, uint32_t *hist, void *out);
int ld_programme(const uint32_t *hist, int nstreams, void *out);
}

static const int32_t RATES[6] = {48000, 44100, 32000, 24000, 22050, 16000};

struct State {
    std::vector<double> lane, ring;
    std::vector<uint8_t> rec, out, prog;
    std::vector<uint32_t> hist;
    explicit State(int ns) : lane((size_t)10 * 2 * ns, 0.0), ring((size_t)30 * ns, 0.0), rec((size_t)48 * ns, 0), out((size_t)48 * ns, 0), prog((size_t)24 * ns, 0), hist((size_t)752 * ns, 0u) {}
};

static int run(int ns, int nf)
{
    std::vector<int32_t> nch((size_t)ns), rate((size_t)ns);
    for (int s = 0; s < ns; s++) { rate[(size_t)s] = RATES[s % 6]; nch[(size_t)s] = ((s / 6 + s) % 2) ? 1 : 2; }
    std::vector<int16_t> pcm((size_t)nf * ns * 2304);
    uint32_t lcg = 12345u + (uint32_t)ns;
    for (size_t i = 0; i < pcm.size(); i++) { lcg = lcg * 1664525u + 1013904223u; pcm[i] = (int16_t)(lcg >> 16); }
    State a(ns), b(ns);
    if (ld_loudness(pcm.data(), nf, ns, nch.data(), rate.data(), a.lane.data(), a.ring.data(), a.rec.data(), a.hist.data(), a.out.data())) return 3;
    for (int f = 0; f < nf; f++) {
        std::vector<int16_t> one(pcm.begin() + (ptrdiff_t)((size_t)f * ns * 2304), pcm.begin() + (ptrdiff_t)((size_t)(f + 1) * ns * 2304));
        if (ld_loudness(one.data(), 1, ns, nch.data(), rate.data(), b.lane.data(), b.ring.data(), b.rec.data(), b.hist.data(), f & 1 ? b.out.data() : nullptr)) return 4;
    }
    if (ld_programme(a.hist.data(), ns, a.prog.data()) || ld_programme(b.hist.data(), ns, b.prog.data())) return 5;
    if (a.lane != b.lane || a.ring != b.ring || a.rec != b.rec || a.hist != b.hist || a.prog != b.prog) return 6;
    if (memcmp(a.rec.data(), a.out.data(), a.rec.size())) return 7;
    uint32_t frames0;
    memcpy(&frames0, a.rec.data(), 4);
    if (frames0 != (uint32_t)nf) return 8;
    return 0;
}

int main()
{
    if (ld_lane_words() != 10 || ld_hist_rows() != 752) return 2;
    if (int rc = run(37, 45)) return rc;
    const int hostile[3] = {1, 31, 33};
    for (int k = 0; k < 3; k++) if (int rc = run(hostile[k], 5)) return 10 + rc;
    puts("sanitized ok");
    return 0;
}
