// limiter_sanitize_main.cpp -- TEST-ONLY driver of the limiter emulation (mp2_limiter_emu.cpp) as a program of its own, so that it can be
// linked with AddressSanitizer + UBSan (tests/limiterlib.py builds it; nothing is preloaded into anything).  37 streams (one and two
// channels alternating) and a lone stream over full-scale noise with a quiet stretch (both paths run), in one call and frame by frame,
// with a short and a long release.  Every buffer -- PCM, records, state, steps -- is a heap block of exactly the data's size, so the last
// stream's slot lies flush against the end of its allocation, and the emulation's LDS block is a heap block of its own size: an index
// past a row, a lane's words or the carried lanes is an access past an allocation, and a sum that leaves 32 bits where the header says it
// cannot is a signed overflow.  The two cuts must agree, on the PCM too.
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

extern "C" {
int lm_state_words(void);
void lm_paths(long *out);
int lm_limit(int16_t *pcm, int nframes, int nstreams, const int32_t *nch, const uint32_t *step, uint32_t ceiling, void *rec, uint32_t *state, void *out);
}

struct State {
    std::vector<uint8_t> rec, out;
    std::vector<uint32_t> state;
    explicit State(int ns) : rec((size_t)32 * ns, 0), out((size_t)32 * ns, 0), state((size_t)172 * ns, 0u) {}
};

static int run(int ns, int nf, uint32_t step0)
{
    std::vector<int32_t> nch((size_t)ns);
    std::vector<uint32_t> step((size_t)ns);
    for (int s = 0; s < ns; s++) { nch[(size_t)s] = ((s / 6 + s) % 2) ? 1 : 2; step[(size_t)s] = step0 + (uint32_t)s; }
    if (ns > 1) nch[(size_t)ns - 1] = 2;                             // the last slot's second row is read and written to its last byte
    std::vector<int16_t> pcm((size_t)nf * ns * 2304);
    uint32_t lcg = 8765u + (uint32_t)ns;
    for (size_t i = 0; i < pcm.size(); i++) {
        lcg = lcg * 1664525u + 1013904223u;
        const size_t fr = i / ((size_t)ns * 2304);
        const bool quiet = fr == 2 || fr == 3;                       // far below the ceiling: frame 3 takes the idle path where the release has ended in frame 2
        pcm[i] = quiet ? (int16_t)((int16_t)(lcg >> 16) / 64) : (int16_t)(lcg >> 16);
    }
    for (int i = 0; i < 40; i++) { pcm[pcm.size() - 1 - (size_t)i] = -32768; pcm[pcm.size() - 1152 - 1 - (size_t)i] = (int16_t)(i & 1 ? -32768 : 32767); }
    std::vector<int16_t> pa(pcm), pb(pcm);
    State a(ns), b(ns);
    if (lm_limit(pa.data(), nf, ns, nch.data(), step.data(), 0x30000000u, a.rec.data(), a.state.data(), a.out.data())) return 3;
    for (int f = 0; f < nf; f++) {
        std::vector<int16_t> one(pcm.begin() + (ptrdiff_t)((size_t)f * ns * 2304), pcm.begin() + (ptrdiff_t)((size_t)(f + 1) * ns * 2304));
        if (lm_limit(one.data(), 1, ns, nch.data(), step.data(), 0x30000000u, b.rec.data(), b.state.data(), f & 1 ? b.out.data() : nullptr)) return 4;
        memcpy(pb.data() + (size_t)f * ns * 2304, one.data(), one.size() * sizeof(int16_t));
    }
    if (a.rec != b.rec || a.state != b.state) return 6;
    if (pa != pb) return 5;
    if (memcmp(a.rec.data(), a.out.data(), a.rec.size())) return 7;
    uint32_t frames0;
    memcpy(&frames0, a.rec.data(), 4);
    if (frames0 != (uint32_t)nf) return 8;
    return 0;
}

int main()
{
    if (lm_state_words() != 172) return 2;
    if (int rc = run(37, 5, 1u << 26)) return rc;                    // a release of 16 samples: the hand-on loop leaves at its first step
    if (int rc = run(37, 5, 22369u)) return 20 + rc;                 // one second at 48 kHz
    if (int rc = run(1, 5, 1u)) return 10 + rc;
    long paths[2];
    lm_paths(paths);
    if (!paths[0] || !paths[1]) return 9;                            // both paths ran
    puts("sanitized ok");
    return 0;
}
