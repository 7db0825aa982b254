// truepeak_sanitize_main.cpp -- TEST-ONLY driver of the true-peak emulation (mp2_truepeak_emu.cpp) as a program of its own, so that it can
// be linked with AddressSanitizer + UBSan (tests/truepeaklib.py builds it; nothing is preloaded into anything).  37 streams (one and two
// channels alternating) and a lone stream over full-scale noise, in one call and frame by frame.  Every buffer -- PCM, records, carried
// samples -- is a heap block of exactly the data's size, so the last stream's slot lies flush against the end of its allocation, and the
// emulation's LDS block is a heap block of its own size: an index past a row, the window or the carried samples is an access past an
// allocation, and a sum that leaves 32 bits is a signed overflow.  The two cuts must agree.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
int tp_carry(void);
int tp_truepeak(const int16_t *pcm, int nframes, int nstreams, const int32_t *nch, uint32_t ceiling, void *rec, uint32_t *hist, void *out);
}

struct State {
    std::vector<uint8_t> rec, out;
    std::vector<uint32_t> hist;
    explicit State(int ns) : rec((size_t)32 * ns, 0), out((size_t)32 * ns, 0), hist((size_t)12 * ns, 0u) {}
};

static int run(int ns, int nf)
{
    std::vector<int32_t> nch((size_t)ns);
    for (int s = 0; s < ns; s++) nch[(size_t)s] = ((s / 6 + s) % 2) ? 1 : 2;
    if (ns > 1) nch[(size_t)ns - 1] = 2;                             // the last slot's second row is read to its last byte
    std::vector<int16_t> pcm((size_t)nf * ns * 2304);
    uint32_t lcg = 4321u + (uint32_t)ns;
    for (size_t i = 0; i < pcm.size(); i++) { lcg = lcg * 1664525u + 1013904223u; pcm[i] = (int16_t)(lcg >> 16); }
    // the extremes of the accumulator in the last stream: a run of -32768 and a run of alternating full scale
    for (int i = 0; i < 40; i++) { pcm[pcm.size() - 1 - (size_t)i] = -32768; pcm[pcm.size() - 1152 - 1 - (size_t)i] = (int16_t)(i & 1 ? -32768 : 32767); }
    State a(ns), b(ns);
    if (tp_truepeak(pcm.data(), nf, ns, nch.data(), 0x30000000u, a.rec.data(), a.hist.data(), a.out.data())) return 3;
    for (int f = 0; f < nf; f++) {
        std::vector<int16_t> one(pcm.begin() + (ptrdiff_t)((size_t)f * ns * 2304), pcm.begin() + (ptrdiff_t)((size_t)(f + 1) * ns * 2304));
        if (tp_truepeak(one.data(), 1, ns, nch.data(), 0x30000000u, b.rec.data(), b.hist.data(), f & 1 ? b.out.data() : nullptr)) return 4;
    }
    if (a.rec != b.rec || a.hist != b.hist) return 6;
    if (memcmp(a.rec.data(), a.out.data(), a.rec.size())) return 7;
    uint32_t frames0;
    memcpy(&frames0, a.rec.data(), 4);
    if (frames0 != (uint32_t)nf) return 8;
    return 0;
}

int main()
{
    if (tp_carry() != 12) return 2;
    if (int rc = run(37, 5)) return rc;
    if (int rc = run(1, 5)) return 10 + rc;
    puts("sanitized ok");
    return 0;
}
