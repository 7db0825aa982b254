// tlb_inputs.h -- the ONE statement of which INPUT FAMILIES may stand beside one another (include/toolame_batch.h: "a stream has one
// source; on one tick or node object the families exclude one another").  A family is a way for audio to reach a stream other than full
// reads of PCM at the encoder's rate.  Each owner builds the mask of what is present in one function of its own -- a batch for one stream
// (batch_inputs, csrc/tlb_internal.h), a tick object (tick_inputs, csrc/tlb_tick.cpp), a node (tlb_node::inputs, csrc/tlb_node.cpp) -- and
// every setter asks tlb_input_may_set once.  A new family is one enumerator and one row in each table.  Header-only, no HIP, nothing but
// <stdint.h>, so that a CPU test can print every answer under the sanitizers (tests/test_inputs_rule.py, tests/emu/inputs_main.cpp).
#pragma once
#include <stdint.h>

enum TlbInput {
    TLB_IN_UP_SOURCE,                            // tlb_resample_*: a 44.1 or 32 kHz source for a 48 kHz stream (and the pairs below it)
    TLB_IN_DOWN_SOURCE,                          // tlb_decimate_*: a 48, 44.1 or 32 kHz source for a 24 kHz stream
    TLB_IN_FEED,                                 // tlb_feed_*: a Layer II feed, strict or adapted
    TLB_IN_DOWN_FEED,                            // tlb_feed_down_*: a 48, 44.1 or 32 kHz Layer II feed for a 24 kHz stream
    TLB_IN_SHORT_READS,                          // tlb_tick_enable_short_reads: an object-level opt-in, no batch has it
    TLB_IN_COUNT
};
enum TlbInputLevel {
    TLB_INPUTS_STREAM,                           // one stream of a batch
    TLB_INPUTS_OBJECT,                           // one tick or node object, whichever streams the families are on
    TLB_INPUTS_LEVELS
};
#define TLB_IN_BIT(f) (1u << (f))
#define TLB_IN_ALL (TLB_IN_BIT(TLB_IN_COUNT) - 1u)

// row f: the families that may not be present when f is set.  Both tables are symmetric and no family excludes itself.
static const uint8_t tlb_input_clash[TLB_INPUTS_LEVELS][TLB_IN_COUNT] = {
    {   // a stream of a batch: a feed's PCM may still pass the resampler or the decimator; nothing else combines
        /* up source   */ TLB_IN_BIT(TLB_IN_DOWN_SOURCE) | TLB_IN_BIT(TLB_IN_DOWN_FEED),
        /* down source */ TLB_IN_BIT(TLB_IN_UP_SOURCE) | TLB_IN_BIT(TLB_IN_DOWN_FEED),
        /* feed        */ TLB_IN_BIT(TLB_IN_DOWN_FEED),
        /* down feed   */ TLB_IN_BIT(TLB_IN_UP_SOURCE) | TLB_IN_BIT(TLB_IN_DOWN_SOURCE) | TLB_IN_BIT(TLB_IN_FEED),
        /* short reads */ 0,
    },
    {   // a tick or node object: all five exclude one another
        TLB_IN_ALL & ~TLB_IN_BIT(TLB_IN_UP_SOURCE), TLB_IN_ALL & ~TLB_IN_BIT(TLB_IN_DOWN_SOURCE), TLB_IN_ALL & ~TLB_IN_BIT(TLB_IN_FEED),
        TLB_IN_ALL & ~TLB_IN_BIT(TLB_IN_DOWN_FEED), TLB_IN_ALL & ~TLB_IN_BIT(TLB_IN_SHORT_READS),
    },
};

// may family f be set, given the mask of the families already present?
static inline bool tlb_input_may_set(TlbInputLevel level, TlbInput f, unsigned present) { return !(tlb_input_clash[level][f] & present); }
