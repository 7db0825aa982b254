// decimate_sanitize_main.cpp -- TEST-ONLY driver of the decimator emulation (mp2_decimate_emu.cpp) as a program of its own, so that it can be
// linked with AddressSanitizer + UBSan (tests/decimatelib.py builds it; nothing is preloaded into anything).  The shared stream set of
// tests/decimatelib.py (every ratio, both channel counts, two streams that are left alone) over six frames of full-scale noise, cut three
// ways, every value behind a slot's need frames 0x7FFF: the buffers are exactly as long as the data and the LDS block is a heap block of its
// own size, so an index past a slot, a table row or the LDS layout is an access past an allocation.  The three cuts must agree.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/tl_decimate_taps.inc"

extern "C" {
int dc_state_words(void);
int dc_table_rows(void);
int dc_decimate(const int16_t *wide, int nframes, int nstreams, const int32_t *nch, const int32_t *ratio, uint32_t *state, int flip, const int16_t *taps, int16_t *out);
}

static const int NS = 6, NF = 6, WIDE = 4608;
static const int32_t NCH[NS] = {2, 1, 2, 1, 2, 2}, RATIO[NS] = {3, 3, 1, 2, 0, 0};      // TL_DC_*: 1/2, 1/2, 80/147, 3/4, none, none
static const long LM[4][2] = {{1, 1}, {80, 147}, {3, 4}, {1, 2}};
static long S(int ratio, long f) { return (1152 * f * LM[ratio][1] + LM[ratio][0] - 1) / LM[ratio][0]; }

int main()
{
    if (dc_state_words() != 64 || dc_table_rows() != 84) return 2;
    std::vector<int16_t> taps;
    taps.insert(taps.end(), &tl_decimate_taps_80_147[0][0], &tl_decimate_taps_80_147[0][0] + 80 * 64);
    taps.insert(taps.end(), &tl_decimate_taps_3_4[0][0], &tl_decimate_taps_3_4[0][0] + 3 * 64);
    taps.insert(taps.end(), &tl_decimate_taps_1_2[0][0], &tl_decimate_taps_1_2[0][0] + 64);
    std::vector<std::vector<int16_t>> sig(NS);
    uint32_t lcg = 12345u;
    for (int s = 0; s < NS; s++)
        if (RATIO[s]) for (long i = 0; i < S(RATIO[s], NF) * NCH[s]; i++) { lcg = lcg * 1664525u + 1013904223u; sig[(size_t)s].push_back((int16_t)(lcg >> 16)); }
    const int cuts[3][6] = {{6}, {1, 3, 2}, {1, 1, 1, 1, 1, 1}};
    std::vector<int16_t> first;
    for (int c = 0; c < 3; c++) {
        std::vector<uint32_t> state((size_t)2 * NS * 64, 0u);
        std::vector<int16_t> all;
        int flip = 0, f0 = 0;
        for (int k = 0; k < 6 && cuts[c][k]; k++) {
            const int nf = cuts[c][k];
            std::vector<int16_t> wide((size_t)nf * NS * WIDE, (int16_t)0x7FFF), out((size_t)nf * NS * 2304, (int16_t)0x1111);
            for (int f = 0; f < nf; f++)
                for (int s = 0; s < NS; s++) {
                    if (!RATIO[s]) continue;
                    const long a = S(RATIO[s], f0 + f), n = S(RATIO[s], f0 + f + 1) - a;
                    memcpy(&wide[((size_t)f * NS + (size_t)s) * WIDE], &sig[(size_t)s][(size_t)(a * NCH[s])], (size_t)(n * NCH[s]) * sizeof(int16_t));
                }
            if (dc_decimate(wide.data(), nf, NS, NCH, RATIO, state.data(), flip, taps.data(), out.data())) return 3;
            all.insert(all.end(), out.begin(), out.end());
            flip ^= 1; f0 += nf;
        }
        for (int f = 0; f < NF; f++) {                               // what is left alone is left alone
            for (int s = 4; s < NS; s++) for (int i = 0; i < 2304; i++) if (all[((size_t)f * NS + (size_t)s) * 2304 + (size_t)i] != 0x1111) return 4;
            for (int s = 1; s < 4; s += 2) for (int i = 1152; i < 2304; i++) if (all[((size_t)f * NS + (size_t)s) * 2304 + (size_t)i] != 0x1111) return 5;
        }
        if (c == 0) first = all;
        else if (all != first) return 6;
    }
    puts("sanitized ok");
    return 0;
}
