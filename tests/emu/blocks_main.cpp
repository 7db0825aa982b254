// blocks_main.cpp -- csrc/tlb_blocks.h walked on the CPU (tests/test_blocks.py builds this with -fsanitize=address,undefined): for every
// N in 1..40 and G in 1..min(N, 9), and for the two sizes DESIGN.md quotes, the cut, the owner of every stream and the three visits.
#include <stdio.h>

#include <vector>

#include "../../odr-audioenc_amd/csrc/tlb_blocks.h"

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (failures++ < 20) { printf("FAIL %s:%d (N %d, G %d): %s -- ", __FILE__, __LINE__, N, G, #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Seen { int g, a, b; };

static void check(int N, int G, bool all_ranges)
{
    const TlbBlocks B(N, G);
    // the cut: contiguous, covers [0, N), the formula, sizes differ by at most one
    int at = 0, least = N, most = 0;
    for (int g = 0; g < G; g++) {
        const TlbBlock b = B.block(g);
        CHECK(b.first == at, "block %d begins at %d, not %d", g, b.first, at);
        CHECK(b.first == (int)((long long)N * g / G) && b.first + b.n == (int)((long long)N * (g + 1) / G), "block %d = [%d, %d)", g, b.first, b.first + b.n);
        at = b.first + b.n;
        if (b.n < least) least = b.n;
        if (b.n > most) most = b.n;
    }
    CHECK(at == N, "the blocks end at %d", at);
    CHECK(most - least <= 1 && least >= 1, "sizes %d..%d", least, most);
    CHECK(B.block(-1).n == 0 && B.block(G).n == 0 && B.block(-1).first == 0 && B.block(G).first == 0, "a block outside is not empty");
    // owner / local of every stream, against the blocks
    for (int g = 0; g < G; g++) {
        const TlbBlock b = B.block(g);
        for (int s = b.first; s < b.first + b.n; s++) {
            int k = -7;
            CHECK(B.owner(s, &k) == g && k == s - b.first, "stream %d: owner %d local %d, block %d", s, B.owner(s), k, g);
            CHECK(B.owner(s) == g, "stream %d without local", s);
            // a visit with the stream sees exactly the owner, with s - first
            std::vector<Seen> v;
            const int rc = B.visit(s, [&](int gg, int kk) { v.push_back(Seen{gg, kk, 0}); return 0; });
            CHECK(rc == 0 && v.size() == 1 && v[0].g == g && v[0].a == s - b.first, "visit(%d) saw %d blocks", s, (int)v.size());
            CHECK(B.visit(s, [&](int, int) { return 41; }) == 41, "visit(%d) lost the code", s);
        }
    }
    // -1 and N answer "none"
    int k = -7;
    CHECK(B.owner(-1, &k) == -1 && B.owner(N, &k) == -1 && k == -7, "owner outside: %d %d, local %d", B.owner(-1), B.owner(N), k);
    int calls = 0;
    CHECK(B.visit(N, [&](int, int) { calls++; return 0; }) == 0 && B.visit(-2, [&](int, int) { calls++; return 0; }) == 0 && calls == 0, "a visit outside made %d calls", calls);
    // a visit with -1 sees every block once, in order, with local -1
    std::vector<Seen> all;
    CHECK(B.visit(-1, [&](int g, int kk) { all.push_back(Seen{g, kk, 0}); return 0; }) == 0 && (int)all.size() == G, "visit(-1) saw %d blocks", (int)all.size());
    for (int g = 0; g < (int)all.size(); g++) CHECK(all[(size_t)g].g == g && all[(size_t)g].a == -1, "visit(-1) call %d: block %d local %d", g, all[(size_t)g].g, all[(size_t)g].a);
    // a non-zero code stops the visit: block `stop` answers, the ones behind it are not asked
    for (int stop = 0; stop < G; stop++) {
        calls = 0;
        CHECK(B.visit(-1, [&](int g, int) { calls++; return g == stop ? 100 + g : 0; }) == 100 + stop && calls == stop + 1, "visit(-1) stopped by %d after %d calls", stop, calls);
        calls = 0;
        CHECK(B.visit_range(0, N, [&](int g, int, int) { calls++; return g == stop ? 100 + g : 0; }) == 100 + stop && calls == stop + 1, "visit_range stopped by %d after %d calls", stop, calls);
    }
    // a range visit sees exactly the overlapping blocks, each with its overlap in local ids
    const int step = all_ranges ? 1 : N / 7 + 1;
    for (int s0 = -1; s0 <= N; s0 += s0 < 0 || all_ranges ? 1 : step)
        for (int s1 = s0; s1 <= N + 1; s1 += all_ranges ? 1 : step) {
            std::vector<Seen> v;
            CHECK(B.visit_range(s0, s1, [&](int g, int l0, int l1) { v.push_back(Seen{g, l0, l1}); return 0; }) == 0, "visit_range(%d, %d) returned a code", s0, s1);
            size_t i = 0;
            for (int g = 0; g < G; g++) {
                const TlbBlock b = B.block(g);
                const int lo = s0 > b.first ? s0 : b.first, hi = s1 < b.first + b.n ? s1 : b.first + b.n;
                if (lo >= hi) continue;
                CHECK(i < v.size() && v[i].g == g && v[i].a == lo - b.first && v[i].b == hi - b.first, "visit_range(%d, %d): call %d is not block %d [%d, %d)", s0, s1, (int)i, g, lo - b.first, hi - b.first);
                i++;
            }
            CHECK(i == v.size(), "visit_range(%d, %d) saw %d blocks, %d overlap", s0, s1, (int)v.size(), (int)i);
        }
}

int main()
{
    int cases = 0;
    for (int N = 1; N <= 40; N++)
        for (int G = 1; G <= (N < 9 ? N : 9); G++, cases++) check(N, G, true);
    check(131072, 8, false); check(16384, 3, false); cases += 2;
    {   // no streams or no blocks: nothing to own, nothing to visit
        const int N = 0, G = 0;
        int calls = 0;
        const TlbBlocks none(0, 4), nob(4, 0);
        CHECK(none.block(0).n == 0 && nob.block(0).n == 0 && none.owner(0) == -1 && nob.owner(0) == -1, "an empty cut owns something");
        CHECK(none.visit(-1, [&](int, int) { calls++; return 0; }) == 0 && nob.visit_range(0, 4, [&](int, int, int) { calls++; return 0; }) == 0 && calls == 0, "an empty cut was visited");
    }
    if (failures) { printf("%d failures\n", failures); return 1; }
    printf("blocks ok: %d cases\n", cases);
    return 0;
}
