// lra_sanitize_main.cpp -- TEST-ONLY driver of the loudness range's emulation (mp2_lra_emu.cpp) as a program of its own, so that it can be
// linked with AddressSanitizer + UBSan (tests/lralib.py builds it; nothing is preloaded into anything).  The 37-stream pattern of
// tests/loudnesslib.py (every rate with one and with two channels: 74 lanes, a second wave half empty) over 140 frames of noise whose
// level steps every 9 frames -- 33 bins at 48 kHz, so every stream forms range blocks -- in one call and frame by frame, and the hostile
// stream counts 1, 31 and 33 over the same frames.  The buffers are exactly as long as the data and the LDS block is a heap block of its own
// size, so an index past a row, the ring, either histogram or the LDS layout is an access past an allocation.  The two cuts must agree,
// the counting wave must leave the meter's own state as the plain wave leaves it, and the range of full-of-counts columns near 2^32 must
// come out without an integer overflow.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
int lra_hist_rows(void);
int lra_loudness(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const int32_t *rate, double *lane, double *ring, void *rec, uint32_t *hist,
                 uint32_t *hist_st, void *out, int range);
int lra_range(const uint32_t *hist_st, int nstreams, void *out);
}

static const int32_t RATES[6] = {48000, 44100, 32000, 24000, 22050, 16000};

struct State {
    std::vector<double> lane, ring;
    std::vector<uint8_t> rec, out, lra;
    std::vector<uint32_t> hist, hist_st;
    explicit State(int ns) : lane((size_t)10 * 2 * ns, 0.0), ring((size_t)30 * ns, 0.0), rec((size_t)48 * ns, 0), out((size_t)48 * ns, 0), lra((size_t)40 * ns, 0),
                             hist((size_t)752 * ns, 0u), hist_st((size_t)752 * ns, 0u) {}
};

static int run(int ns, int nf)
{
    std::vector<int32_t> nch((size_t)ns), rate((size_t)ns);
    for (int s = 0; s < ns; s++) { rate[(size_t)s] = RATES[s % 6]; nch[(size_t)s] = ((s / 6 + s) % 2) ? 1 : 2; }
    std::vector<int16_t> pcm((size_t)nf * ns * 2304);
    uint32_t lcg = 12345u + (uint32_t)ns;
    for (size_t i = 0; i < pcm.size(); i++) {
        lcg = lcg * 1664525u + 1013904223u;
        const int f = (int)(i / ((size_t)ns * 2304)), s = (int)(i / 2304 % (size_t)ns);
        pcm[i] = (int16_t)((int16_t)(lcg >> 16) >> ((f / 9 + s) % 5));
    }
    State a(ns), b(ns), p(ns);
    if (lra_loudness(pcm.data(), nf, ns, nch.data(), rate.data(), a.lane.data(), a.ring.data(), a.rec.data(), a.hist.data(), a.hist_st.data(), a.out.data(), 1)) return 3;
    if (lra_loudness(pcm.data(), nf, ns, nch.data(), rate.data(), p.lane.data(), p.ring.data(), p.rec.data(), p.hist.data(), nullptr, p.out.data(), 0)) return 3;
    for (int f = 0; f < nf; f++) {
        std::vector<int16_t> one(pcm.begin() + (ptrdiff_t)((size_t)f * ns * 2304), pcm.begin() + (ptrdiff_t)((size_t)(f + 1) * ns * 2304));
        if (lra_loudness(one.data(), 1, ns, nch.data(), rate.data(), b.lane.data(), b.ring.data(), b.rec.data(), b.hist.data(), b.hist_st.data(), f & 1 ? b.out.data() : nullptr, 1)) return 4;
    }
    if (lra_range(a.hist_st.data(), ns, a.lra.data()) || lra_range(b.hist_st.data(), ns, b.lra.data())) return 5;
    if (a.lane != b.lane || a.ring != b.ring || a.rec != b.rec || a.hist != b.hist || a.hist_st != b.hist_st || a.lra != b.lra) return 6;
    if (a.lane != p.lane || a.ring != p.ring || a.rec != p.rec || a.hist != p.hist || a.out != p.out) return 7;
    uint64_t blocks = 0;
    for (uint32_t v : a.hist_st) blocks += v;
    if (!blocks) return 8;
    return 0;
}

// every stream's column full of counts whose total stays below 2^32: the ranks need 64 bits
static int big(int ns)
{
    std::vector<uint32_t> h((size_t)752 * ns, 0u);
    std::vector<uint8_t> out((size_t)40 * ns, 0);
    for (int s = 0; s < ns; s++) { h[(size_t)300 * ns + s] = 2147483647u; h[(size_t)(310 + s) * ns + s] = 2147483647u; }
    if (lra_range(h.data(), ns, out.data())) return 1;
    for (int s = 0; s < ns; s++) {
        uint32_t gated; int32_t lo, hi;
        memcpy(&gated, &out[(size_t)40 * s + 28], 4); memcpy(&lo, &out[(size_t)40 * s + 32], 4); memcpy(&hi, &out[(size_t)40 * s + 36], 4);
        if (gated != 4294967294u || lo != 300 || hi != 310 + s) return 2;
    }
    return 0;
}

int main()
{
    if (lra_hist_rows() != 752) return 2;
    if (int rc = run(37, 140)) return rc;
    const int hostile[3] = {1, 31, 33};
    for (int k = 0; k < 3; k++) if (int rc = run(hostile[k], 140)) return 10 + rc;
    if (int rc = big(5)) return 20 + rc;
    puts("sanitized ok");
    return 0;
}
