// tlb_blocks.h -- the ONE statement of how N streams are cut into G contiguous blocks and of how a caller's stream id finds its block:
// block g is [N*g/G, N*(g+1)/G), the cut of the node's shards (csrc/tlb_node.cpp, tlb_node_partition) and of a tick
// object's stream groups (csrc/tlb_tick.cpp).  Blocks differ in size by at most one stream; with G <= N none is empty.  A stream id of -1
// means "every stream" wherever a call takes one.  Header-only, no HIP and no allocation, so that a CPU test can walk every small (N, G)
// under the sanitizers (tests/test_blocks.py, tests/emu/blocks_main.cpp).
#pragma once

struct TlbBlock { int first, n; };               // streams [first, first + n)

struct TlbBlocks {
    int nstreams = 0, nblocks = 0;
    TlbBlocks() = default;
    TlbBlocks(int n, int g) { if (n > 0 && g > 0) { nstreams = n; nblocks = g; } }

    int first(int g) const { return (int)((long long)nstreams * g / nblocks); }      // where block g begins, g in [0, nblocks]
    TlbBlock block(int g) const                  // (empty outside [0, nblocks))
    {
        if (g < 0 || g >= nblocks) return TlbBlock{0, 0};
        return TlbBlock{first(g), first(g + 1) - first(g)};
    }
    // the block that owns a stream and, in *local, the stream's id inside it; -1 (and *local untouched) outside [0, nstreams).
    // N*g/G <= s  <=>  g <= ((s + 1)*G - 1) / N: the owner is the last block that begins at or before s.
    int owner(int stream, int *local = nullptr) const
    {
        if (stream < 0 || stream >= nstreams) return -1;
        const int g = (int)((((long long)stream + 1) * nblocks - 1) / nstreams);
        if (local) *local = stream - first(g);
        return g;
    }
    // fn(g, l0, l1) for every block g that [s0, s1) overlaps, in block order, with the overlap in block-local ids; the first non-zero
    // code ends the visit and is returned
    template <class Fn> int visit_range(int s0, int s1, Fn fn) const
    {
        if (s0 < 0) s0 = 0;
        if (s1 > nstreams) s1 = nstreams;
        if (s0 >= s1) return 0;
        for (int g = owner(s0), last = owner(s1 - 1); g <= last; g++) {
            const TlbBlock b = block(g);
            const int l0 = s0 > b.first ? s0 - b.first : 0, l1 = (s1 < b.first + b.n ? s1 : b.first + b.n) - b.first;
            if (l0 < l1) if (int rc = fn(g, l0, l1)) return rc;
        }
        return 0;
    }
    // fn(g, local) for every block a stream id touches: its owner with its local id, or with stream = -1 every block with local = -1
    // (what the per-block calls take for "all"); an id outside [-1, nstreams) touches none.  Stops as visit_range does.
    template <class Fn> int visit(int stream, Fn fn) const
    {
        if (stream >= 0) { int k = 0; const int g = owner(stream, &k); return g < 0 ? 0 : fn(g, k); }
        for (int g = 0; stream == -1 && g < nblocks; g++) if (int rc = fn(g, -1)) return rc;
        return 0;
    }
};
