// tlb_plan.h -- the ONE statement of what a block of streams becomes: which streams share a configuration record and which mono
// streams share waves in pairs.  Used by tlb_create / tlb_stream_reconfigure (csrc/tlb_batch.cpp) and by the node level's planner
// (tlb_node_plan_shard, csrc/tlb_node.cpp), so that the plan a caller is shown cannot drift from what the batch does.  At the end, for
// the same reason, the rules of the opt-in calls that batch, tick plane and node level all apply.  How the streams are cut into blocks
// (shards, stream groups) is not here: csrc/tlb_blocks.h.  Host C++ only.
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/toolame_batch.h"
#include "mp2_host.h"
#include "mp2_resample.h"
#include "mp2_decimate.h"

// the knobs of toolame.h:13-48 that make a configuration record (the sixth, the PAD length of a frame, is per frame)
static inline bool tlb_same_config(const tlb_stream_config &a, const tlb_stream_config &b)
{
    return a.samplerate == b.samplerate && a.mode == b.mode && a.bitrate == b.bitrate && a.psy_model == b.psy_model && a.pad_len == b.pad_len;
}
static inline int tlb_find_config(const std::vector<tlb_stream_config> &uniq, const tlb_stream_config &c)
{
    for (size_t u = 0; u < uniq.size(); u++) if (tlb_same_config(uniq[u], c)) return (int)u;
    return -1;
}
// streams -> records: streams with the same knobs share one (keeps the tables cache resident); appends to uniq / configs.
// Returns 0 or the TLB_ERR_* of the first illegal configuration (nothing is appended for it).
static inline int tlb_plan_configs(int n, const tlb_stream_config *cfgs, std::vector<tlb_stream_config> &uniq, std::vector<TlConfig> &configs,
                                   std::vector<int32_t> &stream_cfg)
{
    stream_cfg.resize((size_t)n);
    for (int s = 0; s < n; s++) {
        int found = tlb_find_config(uniq, cfgs[s]);
        if (found < 0) {
            TlConfig c;
            if (int rc = tl_build_config(&c, cfgs[s].samplerate, cfgs[s].mode, cfgs[s].bitrate, cfgs[s].psy_model, cfgs[s].pad_len)) return rc;
            uniq.push_back(cfgs[s]); configs.push_back(c);
            found = (int)uniq.size() - 1;
        }
        stream_cfg[(size_t)s] = found;
    }
    return 0;
}
// mono streams of the same record (hence the same model and kernel) in pairs: consecutive ones of the stream order; -1 = alone.
// Returns the number of pairs.
static inline int tlb_plan_pairs(const std::vector<TlConfig> &configs, const std::vector<int32_t> &stream_cfg, std::vector<int32_t> &partner)
{
    const size_t n = stream_cfg.size();
    partner.assign(n, -1);
    std::vector<int> open(configs.size(), -1);                       // per record: a mono stream still waiting for a partner
    int pairs = 0;
    for (size_t s = 0; s < n; s++) {
        const int ci = stream_cfg[s];
        if (configs[(size_t)ci].nch != 1) continue;
        if (open[(size_t)ci] < 0) open[(size_t)ci] = (int)s;
        else { partner[s] = open[(size_t)ci]; partner[(size_t)open[(size_t)ci]] = (int32_t)s; open[(size_t)ci] = -1; pairs++; }
    }
    return pairs;
}
// the kernel list a stream's model rides in: model 4 runs the psy-2 kernels on its own tables
static inline int tlb_model_list(int psy) { return psy == 4 ? 2 : psy; }

// ---- the opt-in rules the batch, the tick plane and the node level share ----
// A source rate for the streams [s0, s1): every stream is checked before one is changed.  pairs(source, encoder) says whether the family
// has that ratio (tlb_up_pair: the resampler; tlb_down_pair: the decimator, csrc/mp2_decimate.h); enc_rate(s) is the encoder rate of
// stream s.  A rate of 0 (off) or the encoder's own is no source.  Returns TLB_ERR_SAMPLERATE when some stream's pair is none, else 0;
// *any becomes true when some stream gets a real source (it is never cleared: ranges can be checked one after another).
static inline bool tlb_up_pair(long source_rate, long enc) { return tl_rs_ratio_of(source_rate, enc) != TL_RS_OFF; }
static inline bool tlb_down_pair(long source_rate, long enc) { return tl_dc_ratio_of(source_rate, enc) != TL_DC_OFF; }
template <class Pairs, class EncRate> static inline int tlb_rate_range(int s0, int s1, long source_rate, Pairs pairs, EncRate enc_rate, bool *any)
{
    for (int s = s0; s < s1; s++) {
        const long enc = enc_rate(s);
        if (source_rate == 0 || source_rate == enc) continue;
        if (!pairs(source_rate, enc)) return TLB_ERR_SAMPLERATE;
        *any = true;
    }
    return 0;
}
// the compare monitor's parameters: legal, and the same as the ones an earlier opt-in gave
static inline bool tlb_compare_params_legal(const tlb_compare_params *p)
{
    return p && p->min_energy >= 1 && p->corr_num > 0 && p->corr_num <= p->corr_den && p->corr_den <= 1024;
}
static inline bool tlb_compare_params_same(const tlb_compare_params &a, const tlb_compare_params &b)
{
    return a.min_energy == b.min_energy && a.corr_num == b.corr_num && a.corr_den == b.corr_den;
}
