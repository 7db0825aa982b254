// tlb_node.cpp -- node level of include/toolame_batch.h, part (3): every GPU of one host behind one handle.
//
// "contiguous stream-id blocks [g*N/G, (g+1)*N/G) per GPU; one host process (or thread) + HIP streams per GPU,
// each with its own PCM ingest and bitstream egress; no collective on the data path".  The reference has no such layer -- one
// odr-audioenc process carries one service (AudioEnc::run(), src/odr-audioenc.cpp:819-1276) -- so this is the fleet-side caller the
// north star describes ("host C++ fans thousands of independent streams ... across the 8 GPUs of one node"), written against the
// library's own C-ABI: a shard is a tlb_tick or a tlb_batch plus a thread that issues every call on it.  Nothing in here touches a
// kernel; it is partition arithmetic, a mailbox per thread, and sums.
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <chrono>
#include <cmath>
#include <condition_variable>
#include <deque>
#include <functional>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/toolame_batch.h"
#include "mp2_host.h"
#include "mp2_resample.h"
#include "tlb_blocks.h"
#include "tlb_inputs.h"
#include "tlb_mailbox.h"
#include "tlb_plan.h"
#ifdef TLB_FAULT_INJECT
#include "tlb_debug.h"
#endif

namespace {

using Clock = std::chrono::steady_clock;

double now_ns()
{
    return (double)std::chrono::duration_cast<std::chrono::nanoseconds>(Clock::now().time_since_epoch()).count();
}
Clock::time_point at_ns(double ns) { return Clock::time_point(std::chrono::nanoseconds((long long)ns)); }      // (now_ns()'s clock)
Clock::duration ms_dur(double ms) { return std::chrono::duration_cast<Clock::duration>(std::chrono::duration<double, std::milli>(ms)); }

// One block of streams: the object that encodes it, the thread that talks to it (the mailbox: csrc/tlb_mailbox.h).
struct Shard : TlbMailbox {
    int index = 0, device = 0, first = 0, n = 0;
    tlb_tick *tick = nullptr;
    tlb_batch *batch = nullptr;
    hipStream_t stream = nullptr;                // BATCH plane: the shard's launches are ordered on it
    // counters (written by the shard's thread inside jobs, read by the node between jobs)
    long steps = 0, frames = 0;
    double busy_ns = 0, device_ms = 0;
    std::deque<double> t_submit;                 // host clock of the steps in flight
    std::deque<long> f_submit;                   // their (stream, frame) pairs
    // BATCH plane: one pair of timing events per queued encode call (recorded on the shard's stream around the launch), summed at sync:
    // device_ms is the device time of EVERY step, however many were queued per sync
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    std::deque<std::pair<hipEvent_t, hipEvent_t>> ev_flight;
    // health (fault isolation): a shard whose device call failed is BROKEN -- skipped by every node-wide call, its accessors answer
    // NULL / 0 -- until tlb_node_shard_restart() has made it a fresh object; the other shards never notice
    bool broken = false;
    int last_err = 0;
    long failures = 0, restarts = 0, lost_steps = 0;
    char what[TLB_NODE_WHAT_LEN] = {};
    // what the device is (filled once at creation, on the shard's thread)
    char device_name[TLB_NODE_NAME_LEN] = {}, pci[24] = {}, uuid[36] = {};
    int num_cu = 0, num_xcd = 0;
    double hbm_gb = 0;

    // TICK DEADLINE (include/toolame_batch.h).  NODE-SIDE records: read and written on the node's caller thread only, never inside a job.
    // While a shard is late its fields above belong to the job it is still running; the node reads them again only after poll() has
    // reported that job done (the mailbox mutex orders the two), and meanwhile reports the shard from `kept`.
    bool late = false;                           // its job missed a deadline and has not been seen to return
    bool late_wait = false;                      // ... and that job retires a tick (a wait), whose results the node will not show
    bool stale = false;                          // its tick's read accessors show a step the node did not wait for it in
    bool rejoined = false;                       // back from LATE: the next submit it takes part in is last_rejoin_step
    bool gain_missed = false;                    // a gain call skipped it while late: applied again when it comes back
    bool took = false;                           // the last node-wide call: its part returned in time ...
    int got = 0;                                 // ... with this code
    std::deque<long> nsteps;                     // node step index of each of its ticks in flight
    Clock::time_point due;                       // the deadline its late job missed
    long late_events = 0, rejoins = 0, dropped_steps = 0, missed_steps = 0, last_late_step = -1, last_rejoin_step = -1;
    double worst_overrun_ms = 0;
    struct Kept {
        long steps, frames, failures, restarts, lost_steps;
        double busy_ns, device_ms;
        int last_err;
        char what[TLB_NODE_WHAT_LEN];
    } kept = {};
    Kept own() const                             // the shard's record as its own fields have it (readable while it is not late)
    {
        Kept k = {steps, frames, failures, restarts, lost_steps, busy_ns, device_ms, last_err, {}};
        memcpy(k.what, what, sizeof what);
        return k;
    }
    void keep() { kept = own(); }                // before a job that may go late is posted (the shard is idle: its fields are readable)
    // What the node may see of this shard now.  A late shard is told from the node's own record (kept): its job still owns the shard's fields.
    Kept seen() const { return late ? kept : own(); }
    int state() const { return late ? TLB_SHARD_LATE : live() ? TLB_SHARD_OK : TLB_SHARD_BROKEN; }
#ifdef TLB_FAULT_INJECT
    int stall_nth = 0, stall_ms = 0, stall_rc = 0;        // tlb_debug_node_stall_next: set between jobs, read inside wait jobs
#endif

    // called on the shard's thread right after the failing call: what HIP last complained about in this thread, then the mark
    int fail(int rc, const char *where)
    {
        const hipError_t e = hipGetLastError();
        snprintf(what, sizeof what, "%s: code %d, hip: %s", where, rc, e == hipSuccess ? "no error recorded (an argument / state error, or injected)" : hipGetErrorString(e));
        if (!broken) fprintf(stderr, "libtoolame-dab-hip: node shard %d (device %d, streams [%d, %d)) is broken -- %s; the other shards go on, tlb_node_shard_restart() brings it back\n",
                             index, device, first, first + n, what);
        broken = true; last_err = rc; failures++;
        lost_steps += (long)t_submit.size();                        // what was in flight is lost with it; the queues are emptied so that the
        t_submit.clear(); f_submit.clear();                         // counters stay those of completed steps
        for (auto &e : ev_flight) ev_pool.push_back(e);
        ev_flight.clear();
        return rc;
    }
    bool live() const { return !broken && (tick || batch); }
    bool on() const { return !late && live(); }            // (`late` first: a late shard's own fields are not read)
};

// The wait part of a tick, on the shard's thread: tlb_node_wait's job, and the one the poll point queues for a tick the node has
// already given up on.  Owns nothing but the shard.
int tick_wait_job(Shard &s)
{
    if (s.t_submit.empty()) return 0;                            // (cannot happen in lockstep; a shard without a tick in flight has nothing to wait for)
    if (int r = tlb_tick_wait(s.tick)) return r;
#ifdef TLB_FAULT_INJECT
    if (s.stall_nth > 0 && --s.stall_nth == 0) {                 // the tick is complete: only this host thread is held up
        std::this_thread::sleep_for(std::chrono::milliseconds(s.stall_ms));
        if (s.stall_rc) return s.stall_rc;
    }
#endif
    const double t = now_ns();
    s.busy_ns += t - s.t_submit.front(); s.frames += s.f_submit.front(); s.t_submit.pop_front(); s.f_submit.pop_front();
    s.steps++;
    const float ms = tlb_tick_last_ms(s.tick);
    if (ms > 0) s.device_ms += ms;
    return 0;
}

}  // namespace

enum { OPT_SHORT_READS, OPT_MONITOR, OPT_COMPARE, OPT_LOUDNESS, OPT_LRA, OPT_TRUEPEAK, OPT_LIMITER, OPTS };     // in the order a restarted shard gets them back

struct tlb_node {
    int plane = TLB_NODE_TICK, nstreams = 0;
    tlb_node_config cfg;                         // as given at creation (the version string copied into `version`)
    std::string version, describe;
    std::vector<tlb_stream_config> cfgs;         // the CURRENT configuration of every stream (reconfigurations applied): what a restarted shard is made from
    std::vector<double> gain_db;                 // the caller's gains, re-applied to a restarted shard
    std::vector<Shard *> shards;
    TlbBlocks blocks;                            // the cut of the streams into the shards' blocks, stream -> shard (csrc/tlb_blocks.h)
    bool finished = false;
    // node-level clock: first submit -> last wait of a step
    std::deque<double> t_submit;
    double wall_ns = 0;
    long submitted = 0, waited = 0;              // node steps: submits / waits so far (a step's index is its submit's)
    double deadline_ms = 0;                      // TICK DEADLINE; 0 = none
    // The options of the shards' tick objects (node_options below): on, and what its enable call was given -- each option reads its own
    // member.  A restarted shard's object gets them again (the meters start from zero there).
    struct Option { bool on = false; int what = 0; tlb_compare_params cparams = {}; uint32_t ceiling = 0; tlb_limiter_params lparams = {0, 0}; };
    Option opt[OPTS];
    int monitor() const { return opt[OPT_MONITOR].what; }            // TLB_MONITOR_* of every shard's tick object; 0: off
    int listen = -1;                             // tlb_node_monitor_listen(): the node-wide stream listened to; -1: none
    // The per-stream input families (csrc/tlb_inputs.h; node_families below): what tlb_node_set_source, _set_down_source, _set_feed and
    // _set_down_feed gave every stream, set again on a restarted shard.  A source is its rate alone; samplerate 0: the stream has none;
    // adapted: set through tlb_node_set_feed_adapted, and set again that way.  A family's vector is empty until it is first turned on.
    struct Input : tlb_feed_config { int adapted; };
    std::vector<Input> kept[TLB_IN_SHORT_READS];
    // the feed concealment of every stream (tlb_node_enable_conceal, tlb_node_enable_feed_loss: any_feed, and set again that way), set again
    // on a restarted shard behind its feeds; empty until first switched on
    struct Conceal { int hold = 0, step = 0, any_feed = 0; };
    std::vector<Conceal> kept_conceal;
    // The families that are on, for tlb_input_may_set at OBJECT level.  That is the TICK plane's rule: every shard there is one tick object.
    // On the BATCH plane the node holds nothing back and the mask is empty: the shards' batches answer stream by stream (batch_inputs).
    unsigned inputs() const
    {
        unsigned m = opt[OPT_SHORT_READS].on ? TLB_IN_BIT(TLB_IN_SHORT_READS) : 0u;
        for (int f = 0; f < TLB_IN_SHORT_READS && plane == TLB_NODE_TICK; f++)
            for (const Input &v : kept[f]) if (v.samplerate) { m |= TLB_IN_BIT(f); break; }
        return m;
    }

    // Run fn(shard) on the thread of every LIVE shard at once.  A shard whose fn returns non-zero is marked broken there and then (on
    // its own thread, with HIP's last error of that thread) and is skipped from now on; the others are not disturbed.  Returns the
    // first non-zero code of THIS call -- the caller's cue to look at tlb_node_shard_status() -- or TLB_ERR_HIP when no shard is live.
    // `due` (TICK DEADLINE): a shard whose part has not returned by then goes LATE at node step `step`; its job keeps running and owns
    // what it uses (fn is shared with it).  `wait`: only shards whose oldest tick in flight is node step `step` take part.
    int live(const char *where, std::function<int(Shard &)> fn, const Clock::time_point *due = nullptr, long step = 0, bool wait = false)
    {
        const auto job = std::make_shared<const std::function<int(Shard &)>>(std::move(fn));
        std::vector<Shard *> on;
        bool any = false, late = false;
        for (Shard *s : shards) {
            s->took = false;
            if (!s->on()) continue;
            any = true;
            if (wait && (s->nsteps.empty() || s->nsteps.front() != step)) { s->stale = true; continue; }     // (back from LATE: not in this step)
            if (due) s->keep();
            on.push_back(s);
            s->post([s, job, where] { const int r = (*job)(*s); return r ? s->fail(r, where) : 0; });
        }
        int rc = 0;
        for (Shard *s : on) {
            int r = 0;
            if (!due) r = s->join_job();
            else if (!s->join_job_until(*due, &r)) {
                s->late = true; s->late_wait = wait; s->due = *due; s->late_events++; s->last_late_step = step; s->nsteps.clear();
                late = true;
                continue;
            }
            s->took = true; s->got = r;
            if (r) s->nsteps.clear();                                // (Shard::fail has emptied its queues)
            if (r && !rc) rc = r;
        }
        if (!rc && late) rc = TLB_ERR_LATE;
        if (!any) rc = any_late() ? (int)TLB_ERR_LATE : (int)TLB_ERR_HIP;
        return rc;
    }
    bool any_late() const
    {
        for (const Shard *s : shards) if (s->late) return true;
        return false;
    }
    // The poll point (end of tlb_node_wait): late shards are looked at without blocking.  Returns the code of a late job that came
    // back with an error (its shard is BROKEN now, as any other), else 0.
    int poll_late()
    {
        int rc = 0;
        Clock::time_point now{};
        for (Shard *s : shards) {
            if (!s->late) continue;
            if (now == Clock::time_point{}) now = Clock::now();
            const double over = std::chrono::duration<double, std::milli>(now - s->due).count();
            if (over > s->worst_overrun_ms) s->worst_overrun_ms = over;
            int r = 0;
            if (!s->poll(&r)) continue;
            s->late = false;                                         // the job has returned: the shard's fields are the node's to read again
            if (r) { if (!rc) rc = r; continue; }
            if (s->late_wait) { s->steps--; s->frames -= s->n; s->dropped_steps++; }      // a tick retired after the node gave up on it: not shown
            if (!s->t_submit.empty()) {                              // its next tick is still in flight: queue its wait, do not wait for it
                s->keep();
                s->late = true; s->late_wait = true; s->due = now + ms_dur(deadline_ms);
                s->post([s] { const int q = tick_wait_job(*s); return q ? s->fail(q, "tlb_tick_wait") : 0; });
                continue;
            }
            s->rejoins++; s->rejoined = true; s->stale = true;       // OK again; takes part from the next submit on
            if (s->gain_missed) {
                s->gain_missed = false;
                const int q = one(s->index, [this](Shard &sh) {
                    for (int k = 0; k < sh.n; k++)
                        if (int e = tlb_tick_set_gain_db(sh.tick, k, gain_db[(size_t)(sh.first + k)])) return sh.fail(e, "set_gain_db");
                    return 0;
                });
                if (q && !rc) rc = q;
            }
        }
        return rc;
    }
    // every shard, broken or not (creation, teardown, the caller's own per-block work) but a late one; first non-zero code wins, nothing is marked
    int all(const std::function<int(Shard &)> &fn)
    {
        std::vector<Shard *> on;
        for (Shard *s : shards) if (!s->late) { on.push_back(s); s->post([s, &fn] { return fn(*s); }); }
        int rc = 0;
        for (Shard *s : on) { const int r = s->join_job(); if (r && !rc) rc = r; }
        return rc;
    }
    int one(int shard, const std::function<int(Shard &)> &fn)
    {
        Shard *s = shards[(size_t)shard];
        s->post([s, &fn] { return fn(*s); });
        return s->join_job();
    }
    Shard *of(int stream, int *local) const
    {
        const int g = blocks.owner(stream, local);
        return g < 0 ? nullptr : shards[(size_t)g];
    }
    // the owning shard of a stream if its results may be read: NULL for a broken shard (its buffers hold a half-finished step), a late
    // one, and one that did not take part in the step last waited for
    Shard *read(int stream, int *local) const
    {
        Shard *s = of(stream, local);
        return s && s->on() && !s->stale ? s : nullptr;
    }
    // ... if its input set may be written: NULL for a broken or a late shard
    Shard *input(int stream, int *local) const
    {
        Shard *s = of(stream, local);
        return s && s->on() ? s : nullptr;
    }
    // ... whether a call may change it: a late shard answers TLB_ERR_LATE, a broken one TLB_ERR_HIP
    static int usable(const Shard &s) { return s.late ? (int)TLB_ERR_LATE : !s.live() ? (int)TLB_ERR_HIP : (int)TLB_OK; }
    // The gate of the calls on ONE stream: its owner in *s and its shard-local id in *local, TLB_ERR_ARG when there is no such stream (*s is
    // NULL then), else usable()'s answer.
    int gate(int stream, Shard **s, int *local) const
    {
        *s = of(stream, local);
        return *s ? usable(**s) : (int)TLB_ERR_ARG;
    }
    // A per-stream setting that is remembered for restarts -- shard_make() sets `kept` again on a fresh object -- for one stream or all
    // (tlb_node_set_source, tlb_node_set_feed, after their own checks).  Every shard the call touches is asked before one is changed: a
    // broken one stops the call with TLB_ERR_HIP, a late one with TLB_ERR_LATE.  `kept` is made by the first call that turns the setting
    // on (`on`); clearing what was never on is TLB_OK and touches nothing.  apply(shard, k, v) runs on the owning shards' threads, in shard
    // order, k = -1 for a whole block.  After a device failure half way (the values were checked by the caller) the shards already changed,
    // and the failing one, get what `kept` says they had, stream by stream -- with fresh state, since setting a stream is all its object
    // offers.  What went through is remembered: keep(i) for every named stream i.
    template <class T, class Apply, class Keep> int set_remembered(int stream, std::vector<T> &kept, bool on, const T &v, Apply apply, Keep keep)
    {
        if (int rc = blocks.visit(stream, [&](int g, int) { return usable(*shards[(size_t)g]); })) return rc;
        if (kept.empty()) { if (!on) return TLB_OK; kept.assign((size_t)nstreams, T{}); }
        auto restore = [&](Shard &sh) {
            for (int i = 0; i < sh.n; i++) (void)apply(sh, i, kept[(size_t)(sh.first + i)]);
            return 0;
        };
        if (int rc = blocks.visit(stream, [&](int g, int k) {
                const int r = one(g, [&](Shard &sh) { return apply(sh, k, v); });
                for (int u = stream < 0 ? 0 : g; r && u <= g; u++) (void)one(u, restore);      // (the touched shards up to the failing one)
                return r;
            })) return rc;
        for (int i = stream < 0 ? 0 : stream; i < (stream < 0 ? nstreams : stream + 1); i++) kept[(size_t)i] = keep(i);
        return TLB_OK;
    }
};

namespace {

// How a remembered value of each per-stream family reaches a shard's object, tick or batch (k = -1: the whole block; a value that is off
// clears); in the order a restarted shard gets them back
using NodeInput = tlb_node::Input;
int (*const node_families[TLB_IN_SHORT_READS])(Shard &sh, int k, const NodeInput &v) = {
    /* up source   */ [](Shard &sh, int k, const NodeInput &v) { return sh.tick ? tlb_tick_set_source(sh.tick, k, v.samplerate) : tlb_resample_set_source(sh.batch, k, v.samplerate); },
    /* down source */ [](Shard &sh, int k, const NodeInput &v) { return sh.tick ? tlb_tick_set_down_source(sh.tick, k, v.samplerate) : tlb_decimate_set_source(sh.batch, k, v.samplerate); },
    /* feed        */ [](Shard &sh, int k, const NodeInput &v) {
        const tlb_feed_config *c = v.bitrate ? &v : nullptr;        // (bitrate 0 is "none": tlb_feed_check_config lets no caller's cfg through with it)
        if (v.adapted) return sh.tick ? tlb_tick_set_feed_adapted(sh.tick, k, c) : tlb_feed_set_adapted(sh.batch, k, c);
        return sh.tick ? tlb_tick_set_feed(sh.tick, k, c) : tlb_feed_set(sh.batch, k, c);
    },
    /* down feed   */ [](Shard &sh, int k, const NodeInput &v) {
        const tlb_feed_config *c = v.bitrate ? &v : nullptr;
        return sh.tick ? tlb_tick_set_down_feed(sh.tick, k, c) : tlb_feed_down_set(sh.batch, k, c);
    },
};
// The one path of the four setters, after their own checks of the value: the exclusion rule, then tlb_node::set_remembered.  `on`: the call
// turns the family on for some stream; keep(i): what stream i is remembered with when the call goes through.
template <class Keep> int node_set_input(tlb_node *nd, TlbInput f, int stream, bool on, const NodeInput &v, Keep keep)
{
    if (on && !tlb_input_may_set(TLB_INPUTS_OBJECT, f, nd->inputs())) return TLB_ERR_ARG;
    return nd->set_remembered(stream, nd->kept[f], on, v, node_families[f], keep);
}
NodeInput node_rate(long rate) { NodeInput v = {}; v.samplerate = rate; return v; }
NodeInput node_feed(const tlb_feed_config *cfg, bool adapted)
{
    NodeInput v = {};
    if (cfg) { v.samplerate = cfg->samplerate; v.bitrate = cfg->bitrate; v.channels = cfg->channels; v.adapted = adapted; }
    return v;
}

// The options of a shard's tick object, beside the families: how a remembered one reaches the object (the node's enable calls, and
// shard_make for a restarted shard, in this order), and for a PCM meter its reset
using NodeOption = tlb_node::Option;
const struct { int (*enable)(tlb_tick *t, const NodeOption &v); int (*reset)(tlb_tick *t, int stream); const char *reset_name; } node_options[OPTS] = {
    /* short reads */ {[](tlb_tick *t, const NodeOption &) { return tlb_tick_enable_short_reads(t); }, nullptr, nullptr},
    /* monitor     */ {[](tlb_tick *t, const NodeOption &v) { return tlb_tick_enable_monitor(t, v.what); }, nullptr, nullptr},
    /* compare     */ {[](tlb_tick *t, const NodeOption &v) { return tlb_tick_enable_compare(t, &v.cparams); }, nullptr, nullptr},
    /* loudness    */ {[](tlb_tick *t, const NodeOption &) { return tlb_tick_enable_loudness(t); }, tlb_tick_loudness_reset, "loudness_reset"},
    /* range       */ {[](tlb_tick *t, const NodeOption &) { return tlb_tick_enable_lra(t); }, nullptr, nullptr},      // (behind loudness: its reset is the range's)
    /* true peak   */ {[](tlb_tick *t, const NodeOption &v) { return tlb_tick_enable_truepeak(t, v.ceiling); }, tlb_tick_truepeak_reset, "truepeak_reset"},
    /* limiter     */ {[](tlb_tick *t, const NodeOption &v) { return tlb_tick_enable_limiter(t, &v.lparams); }, tlb_tick_limiter_reset, "limiter_reset"},
};
// The one body of tlb_node_enable_*: TICK plane only, before the first submit, and `ok`, the option's own precondition.  An option that is
// on answers TLB_OK to a call that is the `same` as the one that turned it on, TLB_ERR_ARG to another.  Else every shard's tick object is
// given v, on the shards' threads, and the node remembers v.
const auto always = [](const auto &) { return true; };
template <class Ok, class Same> int node_enable(tlb_node *nd, int o, NodeOption v, Ok ok, Same same)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->finished || nd->submitted > 0 || !ok(*nd)) return TLB_ERR_ARG;
    if (nd->opt[o].on) return same(nd->opt[o]) ? (int)TLB_OK : (int)TLB_ERR_ARG;
    const int rc = nd->all([&](Shard &s) { return s.tick ? node_options[o].enable(s.tick, v) : (int)TLB_ERR_HIP; });
    v.on = true;
    if (!rc) nd->opt[o] = v;
    return rc;
}
// ... and of a meter's reset of one stream (to its shard, through the gate of the life-cycle calls) or of all (-1: every live shard), between steps
int node_meter_reset(tlb_node *nd, int o, int stream)
{
    if (!nd || !nd->opt[o].on || stream < -1 || stream >= nd->nstreams || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const auto reset = node_options[o].reset;
    if (stream < 0) return nd->live(node_options[o].reset_name, [reset](Shard &s) { return reset(s.tick, -1); });
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return rc;
    return nd->one(s->index, [&](Shard &sh) { return reset(sh.tick, k); });
}

// the objects of one shard, made on the shard's own thread (creation and restart)
int shard_make(tlb_node *nd, Shard &s, long long now_s)
{
    int e = 0;
    if (hipSetDevice(s.device) != hipSuccess) return TLB_ERR_HIP;
    if (nd->plane == TLB_NODE_TICK) {
        tlb_tick_config tc = nd->cfg.tick;
        tc.version = nd->version.data(); tc.version_len = (int)nd->version.size();
        if (now_s >= 0) tc.now_s = now_s;
        s.tick = tlb_tick_create(s.device, s.n, nd->cfgs.data() + s.first, &tc, &e);
        if (!s.tick) return e ? e : TLB_ERR_HIP;
        for (int o = 0; o < OPTS; o++) if (nd->opt[o].on) if (int rc = node_options[o].enable(s.tick, nd->opt[o])) return rc;
        int k;
        if (nd->monitor() && nd->of(nd->listen, &k) == &s) if (int rc = tlb_tick_monitor_listen(s.tick, k)) return rc;
    } else {
        s.batch = tlb_create(s.device, s.n, nd->cfgs.data() + s.first, &e);
        if (!s.batch) return e ? e : TLB_ERR_HIP;
        if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return TLB_ERR_HIP;
    }
    for (int f = 0; f < TLB_IN_SHORT_READS; f++)                      // the caller's sources and feeds, with fresh state
        for (int k = 0; k < s.n && !nd->kept[f].empty(); k++) {
            const NodeInput &v = nd->kept[f][(size_t)(s.first + k)];
            if (v.samplerate) if (int rc = node_families[f](s, k, v)) return rc;
        }
    for (int k = 0; k < s.n && s.tick && !nd->kept_conceal.empty(); k++) {      // the feeds' concealment, from zero
        const tlb_node::Conceal &c = nd->kept_conceal[(size_t)(s.first + k)];
        if (c.hold) if (int rc = (c.any_feed ? tlb_tick_enable_feed_loss : tlb_tick_enable_conceal)(s.tick, k, c.hold, c.step)) return rc;
    }
    for (int k = 0; k < s.n; k++) {                                  // the caller's gains (0 dB needs no call)
        const double g = nd->gain_db[(size_t)(s.first + k)];
        if (g == 0.0) continue;
        if (int rc = s.tick ? tlb_tick_set_gain_db(s.tick, k, g) : tlb_set_gain_db(s.batch, k, g)) return rc;
    }
    return 0;
}
void shard_unmake(Shard &s)
{
    (void)hipSetDevice(s.device);
    if (s.tick) tlb_tick_destroy(s.tick);
    if (s.batch) tlb_destroy(s.batch);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    for (auto &e : s.ev_flight) s.ev_pool.push_back(e);
    s.ev_flight.clear();
    for (auto &e : s.ev_pool) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    s.ev_pool.clear();
    s.tick = nullptr; s.batch = nullptr; s.stream = nullptr;
    s.t_submit.clear(); s.f_submit.clear();
}
// what the shard's device is: so that a record of a multi-GPU run can show N DISTINCT devices took part
void shard_identify(Shard &s)
{
    hipDeviceProp_t p;
    if (hipGetDeviceProperties(&p, s.device) != hipSuccess) { snprintf(s.device_name, sizeof s.device_name, "device %d (no properties)", s.device); return; }
    snprintf(s.device_name, sizeof s.device_name, "%s%s%s", p.name, p.name[0] ? " " : "", p.gcnArchName);     // (some boxes report no marketing name: the ISA name says what it is)
    snprintf(s.pci, sizeof s.pci, "%04x:%02x:%02x.0", (unsigned)p.pciDomainID, (unsigned)p.pciBusID, (unsigned)p.pciDeviceID);
    for (int i = 0; i < 16; i++) snprintf(s.uuid + 2 * i, 3, "%02x", (unsigned)(unsigned char)p.uuid.bytes[i]);
    s.num_cu = p.multiProcessorCount;
    s.hbm_gb = (double)p.totalGlobalMem / 1e9;
    int x = 0;
    if (hipDeviceGetAttribute(&x, hipDeviceAttributeNumberOfXccs, s.device) == hipSuccess) s.num_xcd = x;
}

// ---- the per-stream accessors of the TICK plane ----
// One stream's answer from its shard's tick object: fn(tick, shard-local id), or `empty` -- no node, no such stream, no tick object (BATCH
// plane), or a shard that the gate says may not be asked (READ: tlb_node::read, the results; INPUT: tlb_node::input, the input set).  The
// accessors that report a length pass `len`: it is cleared when the gate refuses; otherwise the tick object's accessor writes it.
// Gate and fn are template arguments: a sender calls tlb_node_packet once per stream and unit, and pays two calls for it as before.
enum Gate { READ, INPUT };
template <Gate G, class R, class Fn> inline R ask(const tlb_node *nd, int stream, R empty, Fn fn, int *len = nullptr)
{
    int k; Shard *s = !nd ? nullptr : G == READ ? nd->read(stream, &k) : nd->input(stream, &k);
    if (!s && len) *len = 0;
    return s && s->tick ? fn(s->tick, k) : empty;
}
// ... the stream's slot of a per-stream array that the tick object hands out whole: GET(tick) + k * stride, NULL where GET answers NULL
template <Gate G, auto GET> inline auto slot(const tlb_node *nd, int stream, size_t stride = 1)
{
    using P = decltype(GET(nullptr));
    return ask<G>(nd, stream, P(nullptr), [stride](tlb_tick *t, int k) { P p = GET(t); return p ? p + (size_t)k * stride : P(nullptr); });
}
// ... or what that slot holds, 0 where there is none
template <Gate G, auto GET> inline auto value(const tlb_node *nd, int stream)
{
    const auto p = slot<G, GET>(nd, stream);
    return p ? *p : 0;
}

}  // namespace

extern "C" {

void tlb_node_partition(int nstreams, int nshards, int shard, int *first, int *n)
{
    const TlbBlock b = TlbBlocks(nstreams, nshards).block(shard);
    if (first) *first = b.first;
    if (n) *n = b.n;
}

int tlb_node_plan_shard(int nstreams, const tlb_stream_config *cfgs, int nshards, int shard,
                        int *first, int *n, int *nconfigs, int list_sizes[4], int *mono_pairs)
{
    if (nstreams <= 0 || !cfgs || nshards <= 0 || shard < 0 || shard >= nshards) return TLB_ERR_ARG;
    int f, c;
    tlb_node_partition(nstreams, nshards, shard, &f, &c);
    if (first) *first = f;
    if (n) *n = c;
    // what tlb_create() derives from the block -- with tlb_create's own helpers (csrc/tlb_plan.h): streams with the same knobs share a
    // record; a kernel list per psy model (4 rides with 2); mono streams of one record pair up in stream order
    std::vector<tlb_stream_config> uniq;
    std::vector<TlConfig> configs;
    std::vector<int32_t> stream_cfg, partner;
    if (int rc = tlb_plan_configs(c, cfgs + f, uniq, configs, stream_cfg)) return rc;
    const int pairs = tlb_plan_pairs(configs, stream_cfg, partner);
    int lists[4] = {0, 0, 0, 0};
    for (int s = 0; s < c; s++) lists[tlb_model_list(configs[(size_t)stream_cfg[(size_t)s]].psy)]++;
    if (nconfigs) *nconfigs = (int)uniq.size();
    if (list_sizes) for (int p = 0; p < 4; p++) list_sizes[p] = lists[p];
    if (mono_pairs) *mono_pairs = pairs;
    return TLB_OK;
}

void tlb_node_destroy(tlb_node *nd)
{
    if (!nd) return;
    for (Shard *s : nd->shards) {
        if (s->th.joinable()) {
            if (s->late) (void)s->join_job();                        // a late shard's job is waited for WITHOUT a limit (TICK DEADLINE)
            s->post([s] { shard_unmake(*s); return 0; });            // objects are torn down on the thread that made them
            (void)s->join_job();
            s->stop();
        }
        delete s;
    }
    delete nd;
}

tlb_node *tlb_node_create(int nshards, const int *devices, int nstreams, const tlb_stream_config *cfgs, const tlb_node_config *nc, int *err)
{
    auto fail = [&](int code) -> tlb_node * { if (err) *err = code; return nullptr; };
    if (nshards <= 0 || !devices || nstreams < nshards || !cfgs || !nc || (nc->plane != TLB_NODE_TICK && nc->plane != TLB_NODE_BATCH)) return fail(TLB_ERR_ARG);
    if (nc->plane == TLB_NODE_TICK && (nc->tick.version_len < 0 || (nc->tick.version_len && !nc->tick.version))) return fail(TLB_ERR_ARG);
    const int ndev = tlb_device_count();
    if (ndev <= 0) return fail(TLB_ERR_NO_DEVICE);
    for (int g = 0; g < nshards; g++) if (devices[g] < 0 || devices[g] >= ndev) return fail(TLB_ERR_NO_DEVICE);
    for (int g = 0; g < nshards; g++)                                 // every configuration is checked before a single byte of HBM is taken
        if (int rc = tlb_node_plan_shard(nstreams, cfgs, nshards, g, nullptr, nullptr, nullptr, nullptr, nullptr)) return fail(rc);
    tlb_node *nd = new tlb_node;
    nd->plane = nc->plane; nd->nstreams = nstreams; nd->cfg = *nc;
    if (nc->plane == TLB_NODE_TICK && nc->tick.version_len) nd->version.assign(nc->tick.version, (size_t)nc->tick.version_len);
    nd->cfg.tick.version = nullptr; nd->cfg.tick.version_len = 0;    // (the caller's pointer is not kept)
    nd->cfgs.assign(cfgs, cfgs + nstreams);
    nd->gain_db.assign((size_t)nstreams, 0.0);
    nd->blocks = TlbBlocks(nstreams, nshards);
    for (int g = 0; g < nshards; g++) {
        Shard *s = new Shard;
        s->index = g; s->device = devices[g];
        s->first = nd->blocks.block(g).first; s->n = nd->blocks.block(g).n;
        nd->shards.push_back(s);
        s->start([s] { (void)hipSetDevice(s->device); });            // HIP's current device is per thread; the tlb_* calls set it again themselves
    }
    const int rc = nd->all([&](Shard &s) { shard_identify(s); return shard_make(nd, s, -1); });
    if (rc) { tlb_node_destroy(nd); return fail(rc); }
    for (Shard *s : nd->shards) {
        char line[320];
        snprintf(line, sizeof line, "shard %d: device %d %s, %d CUs in %d XCDs, %.0f GB, pci %s, uuid %s, streams [%d, %d)\n",
                 s->index, s->device, s->device_name, s->num_cu, s->num_xcd, s->hbm_gb, s->pci, s->uuid, s->first, s->first + s->n);
        nd->describe += line;
    }
    if (getenv("TLB_VERBOSE")) fprintf(stderr, "libtoolame-dab-hip: node of %d shards, %d streams\n%s", nshards, nstreams, nd->describe.c_str());
    if (err) *err = TLB_OK;
    return nd;
}

int tlb_node_nshards(const tlb_node *nd) { return nd ? (int)nd->shards.size() : 0; }
int tlb_node_nstreams(const tlb_node *nd) { return nd ? nd->nstreams : 0; }
int tlb_node_shard_of(const tlb_node *nd, int stream) { return nd ? nd->blocks.owner(stream) : -1; }
const char *tlb_node_describe(const tlb_node *nd) { return nd ? nd->describe.c_str() : ""; }

// ---- health of one shard ----
int tlb_node_shard_status(const tlb_node *nd, int shard, tlb_node_shard_info *info)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size()) return -TLB_ERR_ARG;
    const Shard &s = *nd->shards[(size_t)shard];
    if (info) {
        const Shard::Kept k = s.seen();
        memset(info, 0, sizeof *info);
        info->shard = s.index; info->device = s.device; info->first = s.first; info->nstreams = s.n;
        info->state = s.state(); info->last_err = k.last_err;
        info->failures = k.failures; info->restarts = k.restarts; info->lost_steps = k.lost_steps;
        memcpy(info->what, k.what, sizeof info->what);
        memcpy(info->device_name, s.device_name, sizeof info->device_name);
        memcpy(info->pci, s.pci, sizeof info->pci); memcpy(info->uuid, s.uuid, sizeof info->uuid);
        info->num_cu = s.num_cu; info->num_xcd = s.num_xcd; info->hbm_gb = s.hbm_gb;
    }
    return s.state();
}
// A fresh object for the block, made on the shard's own thread: its streams start "as a freshly started reference process" (tlb_stream_reset's
// contract, for the whole block: no history, no pending frame, psy 2/4 state zero, the EDI senders re-initialised from now_s), with
// the configurations the streams have NOW (reconfigurations since creation included) and the caller's gains.  The other shards are not
// touched.  Legal between steps only (no tick in flight / after tlb_node_sync): the restarted shard joins the lockstep at the next
// submit, and its first tick emits nothing (one frame of latency), exactly like a new node's.  Works on a healthy shard too.
int tlb_node_shard_restart(tlb_node *nd, int shard, long long now_s)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size()) return TLB_ERR_ARG;
    if (nd->shards[(size_t)shard]->late) return TLB_ERR_LATE;
    if (nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    nd->shards[(size_t)shard]->nsteps.clear();
    const int rc = nd->one(shard, [&](Shard &s) {
        shard_unmake(s);
        (void)hipGetLastError();                                     // the old failure is on record in `what`; start clean
        if (int r = shard_make(nd, s, now_s)) { shard_unmake(s); s.broken = true; s.last_err = r; snprintf(s.what, sizeof s.what, "restart: code %d", r); return r; }
        s.broken = false; s.restarts++;
        return 0;
    });
    return rc;
}

int tlb_node_counters(const tlb_node *nd, tlb_node_counter *per_shard, tlb_node_counter *total)
{
    if (!nd) return TLB_ERR_ARG;
    tlb_node_counter t;
    memset(&t, 0, sizeof t);
    t.shard = -1; t.device = -1; t.first = 0; t.nstreams = nd->nstreams; t.wall_ns = nd->wall_ns;
    for (size_t g = 0; g < nd->shards.size(); g++) {
        const Shard &s = *nd->shards[g];
        tlb_node_counter c;
        memset(&c, 0, sizeof c);
        c.shard = s.index; c.device = s.device; c.first = s.first; c.nstreams = s.n;
        const Shard::Kept k = s.seen();
        c.steps = k.steps; c.frames = k.frames; c.busy_ns = k.busy_ns; c.device_ms = k.device_ms;
        if (per_shard) per_shard[g] = c;
        t.frames += c.frames;
        if (g == 0 || c.steps < t.steps) t.steps = c.steps;
        if (c.busy_ns > t.busy_ns) t.busy_ns = c.busy_ns;
        if (c.device_ms > t.device_ms) t.device_ms = c.device_ms;
    }
    if (total) *total = t;
    return TLB_OK;
}

int tlb_node_parallel(tlb_node *nd, void (*fn)(void *ctx, int shard, int first, int n), void *ctx)
{
    if (!nd || !fn) return TLB_ERR_ARG;
    return nd->all([&](Shard &s) { fn(ctx, s.index, s.first, s.n); return 0; });
}

int tlb_node_set_deadline_ms(tlb_node *nd, double ms)
{
    if (!nd || nd->plane != TLB_NODE_TICK || !std::isfinite(ms) || ms < 0 || !nd->t_submit.empty()) return TLB_ERR_ARG;
    nd->deadline_ms = ms;
    return TLB_OK;
}
int tlb_node_shard_deadline_status(const tlb_node *nd, int shard, tlb_node_shard_deadline *info)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size()) return -TLB_ERR_ARG;
    const Shard &s = *nd->shards[(size_t)shard];
    const int st = s.state();
    if (info) {
        memset(info, 0, sizeof *info);
        info->state = st;
        info->late_events = s.late_events; info->rejoins = s.rejoins; info->dropped_steps = s.dropped_steps; info->missed_steps = s.missed_steps;
        info->last_late_step = s.last_late_step; info->last_rejoin_step = s.last_rejoin_step; info->worst_overrun_ms = s.worst_overrun_ms;
    }
    return st;
}

// ---- TICK plane ----
int16_t *tlb_node_pcm(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_pcm>(nd, stream, 2 * TLB_SAMPLES_PER_FRAME); }
uint8_t *tlb_node_xpad(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_xpad>(nd, stream, TLB_MAX_XPAD); }
int32_t *tlb_node_xpad_len(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_xpad_len>(nd, stream); }
// The options (node_enable: tlb_tick_enable_* of every shard, on the shards' threads, before the first submit, TICK plane only).  Short
// reads are an input family too (csrc/tlb_inputs.h).
int tlb_node_enable_short_reads(tlb_node *nd)
{
    return node_enable(nd, OPT_SHORT_READS, NodeOption{}, [](const tlb_node &n) { return tlb_input_may_set(TLB_INPUTS_OBJECT, TLB_IN_SHORT_READS, n.inputs()); }, always);
}
int tlb_node_enable_monitor(tlb_node *nd, int what)
{
    NodeOption v; v.what = what;
    return node_enable(nd, OPT_MONITOR, v, [what](const tlb_node &) { return what == TLB_MONITOR_CHECK || what == TLB_MONITOR_AUDIO; },
                       [what](const NodeOption &was) { return was.what == what; });
}
const tlb_monitor_record *tlb_node_monitor(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_monitor>(nd, stream); }
// The compare monitor: after tlb_node_enable_monitor(TLB_MONITOR_AUDIO).
int tlb_node_enable_compare(tlb_node *nd, const tlb_compare_params *params)
{
    NodeOption v; if (params) v.cparams = *params;
    return node_enable(nd, OPT_COMPARE, v, [params](const tlb_node &n) { return params && n.monitor() == TLB_MONITOR_AUDIO && tlb_compare_params_legal(params); },
                       [params](const NodeOption &was) { return tlb_compare_params_same(*params, was.cparams); });
}
const tlb_compare_record *tlb_node_compare(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_compare>(nd, stream); }
int tlb_node_enable_loudness(tlb_node *nd) { return node_enable(nd, OPT_LOUDNESS, NodeOption{}, always, always); }
const tlb_loudness_record *tlb_node_loudness(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_loudness>(nd, stream); }
int tlb_node_loudness_reset(tlb_node *nd, int stream) { return node_meter_reset(nd, OPT_LOUDNESS, stream); }     // (EBU mode's reset)
// Programme loudness of every stream, out [nstreams], between steps: each live shard fills its block on its own thread; the records of a
// broken or late shard's streams are all zero.
int tlb_node_loudness_programme(tlb_node *nd, tlb_loudness_programme_record *out)
{
    if (!nd || !out || !nd->opt[OPT_LOUDNESS].on || !nd->t_submit.empty()) return TLB_ERR_ARG;
    memset(out, 0, sizeof(tlb_loudness_programme_record) * (size_t)nd->nstreams);
    return nd->live("loudness_programme", [out](Shard &s) { return tlb_tick_loudness_programme(s.tick, out + s.first); });
}
// The loudness range: after tlb_node_enable_loudness.  The range of every stream, out [nstreams], between steps, as the programme loudness.
int tlb_node_enable_lra(tlb_node *nd) { return node_enable(nd, OPT_LRA, NodeOption{}, [](const tlb_node &n) { return n.opt[OPT_LOUDNESS].on; }, always); }
int tlb_node_lra(tlb_node *nd, tlb_lra_record *out)
{
    if (!nd || !out || !nd->opt[OPT_LRA].on || !nd->t_submit.empty()) return TLB_ERR_ARG;
    memset(out, 0, sizeof(tlb_lra_record) * (size_t)nd->nstreams);
    return nd->live("lra", [out](Shard &s) { return tlb_tick_lra(s.tick, out + s.first); });
}
int tlb_node_enable_truepeak(tlb_node *nd, uint32_t ceiling)
{
    NodeOption v; v.ceiling = ceiling;
    return node_enable(nd, OPT_TRUEPEAK, v, always, always);         // (a second call's ceiling is not looked at: the first one stays)
}
const tlb_truepeak_record *tlb_node_truepeak(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_truepeak>(nd, stream); }
int tlb_node_truepeak_reset(tlb_node *nd, int stream) { return node_meter_reset(nd, OPT_TRUEPEAK, stream); }
// The true-peak limiter: a second call must name the parameters of the first (0 and the default it selects are the same parameter).
static tlb_limiter_params limiter_params_of(const tlb_limiter_params *p)
{
    tlb_limiter_params v = {p && p->ceiling ? p->ceiling : TLB_TRUEPEAK_CEILING_DEFAULT, p && p->release_ms ? p->release_ms : TLB_LIMITER_RELEASE_DEFAULT_MS};
    return v;
}
int tlb_node_enable_limiter(tlb_node *nd, const tlb_limiter_params *params)
{
    NodeOption v; v.lparams = limiter_params_of(params);
    const tlb_limiter_params p = v.lparams;
    return node_enable(nd, OPT_LIMITER, v, [p](const tlb_node &) { return p.ceiling >= (1u << 20) && p.ceiling <= (1u << 30) && p.release_ms >= 1u && p.release_ms <= 10000u; },
                       [p](const NodeOption &was) { return was.lparams.ceiling == p.ceiling && was.lparams.release_ms == p.release_ms; });
}
const tlb_limiter_record *tlb_node_limiter(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_limiter>(nd, stream); }
int tlb_node_limiter_reset(tlb_node *nd, int stream) { return node_meter_reset(nd, OPT_LIMITER, stream); }
// One stream of the node, or none: the selection goes to the stream's shard and is cleared on the others.  It is a field of the shards'
// tick objects that their next submit reads; no shard but a late one runs a job between the node's calls, and a late one is left alone
// (it cannot be the stream's shard: TLB_ERR_LATE).
int tlb_node_monitor_listen(tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->monitor() != TLB_MONITOR_AUDIO || stream < -1 || stream >= nd->nstreams) return TLB_ERR_ARG;
    int k = 0; Shard *own = stream >= 0 ? nd->of(stream, &k) : nullptr;
    if (own) if (int rc = nd->usable(*own)) return rc;
    for (Shard *s : nd->shards)
        if (s->on() && s->tick) (void)tlb_tick_monitor_listen(s->tick, s == own ? k : -1);
    nd->listen = stream;
    return TLB_OK;
}
const int16_t *tlb_node_monitor_pcm(const tlb_node *nd, int *stream)
{
    if (stream) *stream = -1;
    if (!nd || nd->monitor() != TLB_MONITOR_AUDIO) return nullptr;
    for (const Shard *s : nd->shards) {
        if (!s->on() || s->stale || !s->tick) continue;
        int k = -1;
        const int16_t *p = tlb_tick_monitor_pcm(s->tick, &k);
        if (p) { if (stream) *stream = s->first + k; return p; }
    }
    return nullptr;
}
// A source rate or a down source rate for one stream or all: to the owning shards' objects (tlb_tick_set_source / tlb_resample_set_source,
// tlb_tick_set_down_source / tlb_decimate_set_source), on their threads, between steps (tlb_node::set_remembered).
static int node_set_rate(tlb_node *nd, TlbInput f, int stream, long source_rate)
{
    if (!nd || stream < -1 || stream >= nd->nstreams || source_rate < 0 || nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? nd->nstreams : stream + 1;
    bool any = false;
    if (int rc = tlb_rate_range(s0, s1, source_rate, f == TLB_IN_UP_SOURCE ? tlb_up_pair : tlb_down_pair, [nd](int k) { return (long)nd->cfgs[(size_t)k].samplerate; }, &any)) return rc;
    return node_set_input(nd, f, stream, any, node_rate(source_rate),
        [&](int i) { return node_rate(source_rate == nd->cfgs[(size_t)i].samplerate ? 0 : source_rate); });      // (the encoder's own rate is no source)
}
int tlb_node_set_source(tlb_node *nd, int stream, long source_rate) { return node_set_rate(nd, TLB_IN_UP_SOURCE, stream, source_rate); }
int tlb_node_set_down_source(tlb_node *nd, int stream, long source_rate) { return node_set_rate(nd, TLB_IN_DOWN_SOURCE, stream, source_rate); }
// the stream's wide slot in its shard's current input set: NULL for a broken or a late shard, while two ticks are in flight and while no
// stream of the shard has a down source
int16_t *tlb_node_down(tlb_node *nd, int stream) { return ask<INPUT>(nd, stream, (int16_t *)nullptr, [](tlb_tick *t, int k) { return tlb_tick_down(t, k); }); }
int tlb_node_down_need(const tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK) return -TLB_ERR_ARG;
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return -rc;
    return s->tick ? tlb_tick_down_need(s->tick, k) : -TLB_ERR_HIP;
}
// A Layer II feed for one stream or all (cfg = NULL: removed; remembered as bitrate 0), the same way.  Every named stream is checked
// before a shard is asked.
static bool node_rates_adapt(long feed, long enc) { return feed == enc || tlb_up_pair(feed, enc); }
static int node_set_feed(tlb_node *nd, int stream, const tlb_feed_config *cfg, bool adapt)
{
    if (!nd || stream < -1 || stream >= nd->nstreams || nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? nd->nstreams : stream + 1;
    if (cfg) {
        if (int rc = tlb_feed_check_config(cfg)) return rc;
        for (int i = s0; i < s1; i++) {
            if (adapt) { if (!node_rates_adapt(cfg->samplerate, nd->cfgs[(size_t)i].samplerate)) return TLB_ERR_SAMPLERATE; continue; }
            if (cfg->samplerate != nd->cfgs[(size_t)i].samplerate) return TLB_ERR_SAMPLERATE;
            if (cfg->channels != (nd->cfgs[(size_t)i].mode == 'm' ? 1 : 2)) return TLB_ERR_MODE;
        }
    }
    const NodeInput v = node_feed(cfg, adapt);
    const int rc = node_set_input(nd, TLB_IN_FEED, stream, cfg != nullptr, v, [&](int) { return v; });
    for (int i = s0; i < s1 && !rc && !nd->kept_conceal.empty(); i++)                // (a stream's new feed, or none, starts without concealment; a down feed's is its own family's)
        if (nd->kept[TLB_IN_DOWN_FEED].empty() || !nd->kept[TLB_IN_DOWN_FEED][(size_t)i].samplerate) nd->kept_conceal[(size_t)i] = tlb_node::Conceal{};
    return rc;
}
// The feed concealment, per stream (TICK plane): tlb_tick_enable_conceal of the owning shards' objects between steps, remembered for restarts.
// Every named stream needs a strict feed the node remembers; the rest is tlb_node::set_remembered's
// any_feed (tlb_node_enable_feed_loss): a feed of any kind the node remembers, adapted and down feeds included
static int node_enable_conceal(tlb_node *nd, int stream, int hold, int step, bool any_feed)
{
    if (!nd || nd->plane != TLB_NODE_TICK || stream < -1 || stream >= nd->nstreams || nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    if (hold < 0 || hold > TLB_CONCEAL_MAX_HOLD || (hold > 0 && (step < 1 || step > TLB_CONCEAL_MAX_STEP))) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? nd->nstreams : stream + 1;
    const std::vector<NodeInput> &feeds = nd->kept[TLB_IN_FEED], &down = nd->kept[TLB_IN_DOWN_FEED];
    for (int i = s0; i < s1 && hold > 0; i++) {
        const bool fed = !feeds.empty() && feeds[(size_t)i].samplerate;
        if (!(fed && !feeds[(size_t)i].adapted) && !(any_feed && (fed || (!down.empty() && down[(size_t)i].samplerate)))) return TLB_ERR_ARG;
    }
    tlb_node::Conceal v; v.hold = hold; v.step = hold ? step : 0; v.any_feed = hold && any_feed;
    return nd->set_remembered(stream, nd->kept_conceal, hold > 0, v,
                              [](Shard &sh, int k, const tlb_node::Conceal &c) {
                                  return sh.tick ? (c.any_feed ? tlb_tick_enable_feed_loss : tlb_tick_enable_conceal)(sh.tick, k, c.hold, c.step) : (int)TLB_ERR_HIP;
                              },
                              [&](int) { return v; });
}
int tlb_node_enable_conceal(tlb_node *nd, int stream, int hold, int step) { return node_enable_conceal(nd, stream, hold, step, false); }
int tlb_node_enable_feed_loss(tlb_node *nd, int stream, int hold, int step) { return node_enable_conceal(nd, stream, hold, step, true); }
const tlb_conceal_record *tlb_node_conceal(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_conceal>(nd, stream); }
int tlb_node_conceal_reset(tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->kept_conceal.empty() || stream < -1 || stream >= nd->nstreams || !nd->t_submit.empty()) return TLB_ERR_ARG;
    if (stream < 0) return nd->live("conceal_reset", [](Shard &s) { return tlb_tick_conceal_reset(s.tick, -1); });
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return rc;
    return nd->one(s->index, [&](Shard &sh) { return tlb_tick_conceal_reset(sh.tick, k); });
}
int tlb_node_set_feed(tlb_node *nd, int stream, const tlb_feed_config *cfg) { return node_set_feed(nd, stream, cfg, false); }
int tlb_node_set_feed_adapted(tlb_node *nd, int stream, const tlb_feed_config *cfg) { return node_set_feed(nd, stream, cfg, true); }
// is a feed frame wanted in the stream's slot of its shard's current input set (TICK plane; broken and late shards answer as tlb_node_need does)
int tlb_node_feed_want(const tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK) return -TLB_ERR_ARG;
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return -rc;
    return s->tick ? tlb_tick_feed_want(s->tick, k) : -TLB_ERR_HIP;
}
// the stream's slot of its shard's feed buffers (tlb_tick_feed / _feed_len of the shard's tick object): NULL for a broken or a late shard, while
// two ticks are in flight and while no stream of the shard has a feed
uint8_t *tlb_node_feed(tlb_node *nd, int stream)
{
    return ask<INPUT>(nd, stream, (uint8_t *)nullptr, [](tlb_tick *t, int k) {
        uint8_t *p = tlb_tick_feed(t);
        return p ? p + (size_t)k * (size_t)tlb_tick_feed_stride(t) : nullptr;      // (one slot width for the whole object: the tick's own)
    });
}
int32_t *tlb_node_feed_len(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_feed_len>(nd, stream); }
int tlb_node_feed_stride(const tlb_node *nd, int stream) { return ask<INPUT>(nd, stream, 0, [](tlb_tick *t, int) { return tlb_tick_feed_stride(t); }); }
const tlb_frame_report *tlb_node_feed_report(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_feed_report>(nd, stream); }
// A down feed for one stream or all (cfg = NULL: removed; remembered as bitrate 0), the same way (tlb_tick_set_down_feed / tlb_feed_down_set
// of the owning shards' objects).  Every named stream is checked before a shard is asked.
int tlb_node_set_down_feed(tlb_node *nd, int stream, const tlb_feed_config *cfg)
{
    if (!nd || stream < -1 || stream >= nd->nstreams || nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? nd->nstreams : stream + 1;
    if (cfg) {
        if (int rc = tlb_feed_check_config(cfg)) return rc;
        for (int i = s0; i < s1; i++) if (!tlb_down_pair(cfg->samplerate, nd->cfgs[(size_t)i].samplerate)) return TLB_ERR_SAMPLERATE;      // (the legal pairs are the decimator's three)
    }
    const NodeInput v = node_feed(cfg, false);
    const int rc = node_set_input(nd, TLB_IN_DOWN_FEED, stream, cfg != nullptr, v, [&](int) { return v; });
    for (int i = s0; i < s1 && !rc && !nd->kept_conceal.empty(); i++)                // (a stream's new down feed, or none, starts without concealment)
        if (nd->kept[TLB_IN_FEED].empty() || !nd->kept[TLB_IN_FEED][(size_t)i].samplerate) nd->kept_conceal[(size_t)i] = tlb_node::Conceal{};
    return rc;
}
// the feed frames wanted in the stream's two slots of its shard's current input set (TICK plane; broken and late shards answer as tlb_node_need does)
int tlb_node_down_feed_want(const tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK) return -TLB_ERR_ARG;
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return -rc;
    return s->tick ? tlb_tick_down_feed_want(s->tick, k) : -TLB_ERR_HIP;
}
// the stream's two slots of its shard's down-feed buffers: NULL for a broken or a late shard, while two ticks are in flight and while no
// stream of the shard has a down feed
uint8_t *tlb_node_down_feed(tlb_node *nd, int stream)
{
    return ask<INPUT>(nd, stream, (uint8_t *)nullptr, [](tlb_tick *t, int k) {
        uint8_t *p = tlb_tick_down_feed(t);
        return p ? p + 2 * (size_t)k * (size_t)tlb_tick_down_feed_stride(t) : nullptr;      // (one slot width for the whole object: the tick's own)
    });
}
int32_t *tlb_node_down_feed_len(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_down_feed_len>(nd, stream, 2); }
int tlb_node_down_feed_stride(const tlb_node *nd, int stream) { return ask<INPUT>(nd, stream, 0, [](tlb_tick *t, int) { return tlb_tick_down_feed_stride(t); }); }
const tlb_frame_report *tlb_node_down_feed_report(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_down_feed_report>(nd, stream, 2); }
int tlb_node_need(const tlb_node *nd, int stream)
{
    if (!nd || nd->plane != TLB_NODE_TICK) return -TLB_ERR_ARG;
    int k; Shard *s;
    if (int rc = nd->gate(stream, &s, &k)) return -rc;
    return s->tick ? tlb_tick_need(s->tick, k) : -TLB_ERR_HIP;
}
int32_t *tlb_node_valid(tlb_node *nd, int stream) { return slot<INPUT, tlb_tick_valid>(nd, stream); }

int tlb_node_submit(tlb_node *nd)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->finished || nd->t_submit.size() >= 2) return TLB_ERR_ARG;
    const double t0 = now_ns();
    const long step = nd->submitted;
    for (Shard *s : nd->shards) if (s->late) s->missed_steps++;      // its streams' input for this step is never encoded
    const Clock::time_point due = at_ns(t0) + ms_dur(nd->deadline_ms);
    const int rc = nd->live("tlb_tick_submit", [](Shard &s) {
        const double t = now_ns();
        if (int r = tlb_tick_submit(s.tick)) return r;
        s.t_submit.push_back(t); s.f_submit.push_back((long)s.n);
        return 0;
    }, nd->deadline_ms > 0 ? &due : nullptr, step);
    for (Shard *s : nd->shards)
        if (s->took && !s->got) {
            s->nsteps.push_back(step);
            if (s->rejoined) { s->last_rejoin_step = step; s->rejoined = false; }
        }
    nd->t_submit.push_back(t0);                                      // the node's step exists whatever a shard did: wait() retires it
    nd->submitted++;
    return rc;
}
int tlb_node_wait(tlb_node *nd)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->t_submit.empty()) return TLB_ERR_ARG;
    const Clock::time_point due = at_ns(nd->t_submit.front()) + ms_dur(nd->deadline_ms);     // the real-time budget runs from submit
    const int rc = nd->live("tlb_tick_wait", tick_wait_job, nd->deadline_ms > 0 ? &due : nullptr, nd->waited, true);
    for (Shard *s : nd->shards)
        if (s->took && !s->got) { s->stale = false; s->nsteps.pop_front(); }
    nd->wall_ns += now_ns() - nd->t_submit.front(); nd->t_submit.pop_front();
    nd->waited++;
    const int rp = nd->poll_late();                                  // the one poll point of late shards
    return rc && rc != TLB_ERR_LATE ? rc : rp ? rp : rc;
}
int tlb_node_run(tlb_node *nd)
{
    if (!nd || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const int rc = tlb_node_submit(nd);
    if (rc == TLB_ERR_ARG) return rc;
    const int rw = tlb_node_wait(nd);                                // the shards that did submit are waited for even when another broke
    return rc ? rc : rw;
}
int tlb_node_finish(tlb_node *nd)
{
    if (!nd || nd->plane != TLB_NODE_TICK || nd->finished || !nd->t_submit.empty()) return TLB_ERR_ARG;
    const Clock::time_point due = Clock::now() + ms_dur(nd->deadline_ms);
    const int rc = nd->live("tlb_tick_finish", [](Shard &s) { return tlb_tick_finish(s.tick); }, nd->deadline_ms > 0 ? &due : nullptr, nd->submitted);
    for (Shard *s : nd->shards)
        if (s->took && !s->got) s->stale = false;
    nd->finished = true;
    return rc;
}
int tlb_node_units(const tlb_node *nd, int stream) { return ask<READ>(nd, stream, 0, [](tlb_tick *t, int k) { return tlb_tick_units(t, k); }); }
const int16_t *tlb_node_peaks(const tlb_node *nd, int stream) { return slot<READ, tlb_tick_peaks>(nd, stream, 2); }
uint32_t tlb_node_silence_ms(const tlb_node *nd, int stream) { return value<READ, tlb_tick_silence_ms>(nd, stream); }
uint32_t tlb_node_underrun_ms(const tlb_node *nd, int stream) { return value<READ, tlb_tick_underrun_ms>(nd, stream); }
uint32_t tlb_node_underruns(const tlb_node *nd, int stream) { return value<READ, tlb_tick_underruns>(nd, stream); }
const uint8_t *tlb_node_frame(const tlb_node *nd, int stream, int *len)
{
    return ask<READ>(nd, stream, (const uint8_t *)nullptr, [=](tlb_tick *t, int k) { return tlb_tick_frame(t, k, len); }, len);
}
const uint8_t *tlb_node_packet(const tlb_node *nd, int stream, int unit, int *len)
{
    return ask<READ>(nd, stream, (const uint8_t *)nullptr, [=](tlb_tick *t, int k) { return tlb_tick_packet(t, k, unit, len); }, len);
}
const uint8_t *tlb_node_message(const tlb_node *nd, int stream, int unit, int *len)
{
    return ask<READ>(nd, stream, (const uint8_t *)nullptr, [=](tlb_tick *t, int k) { return tlb_tick_message(t, k, unit, len); }, len);
}
int tlb_node_fragments(const tlb_node *nd, int stream, int unit) { return ask<READ>(nd, stream, 0, [=](tlb_tick *t, int k) { return tlb_tick_fragments(t, k, unit); }); }
const uint8_t *tlb_node_fragment(const tlb_node *nd, int stream, int unit, int kf, int *len)
{
    return ask<READ>(nd, stream, (const uint8_t *)nullptr, [=](tlb_tick *t, int k) { return tlb_tick_fragment(t, k, unit, kf, len); }, len);
}

// ---- both planes: gain, life cycle of one stream (on the owning shard's thread, like every other call on the shard's object) ----
// A stream of a BROKEN shard answers TLB_ERR_HIP (the gain is remembered and applied when the shard is restarted), of a LATE one
// TLB_ERR_LATE (the gain is remembered and applied when the shard comes back).
int tlb_node_set_gain_db(tlb_node *nd, int stream, double gain_db)
{
    if (!nd || stream < -1 || stream >= nd->nstreams) return TLB_ERR_ARG;
    auto f = [&](Shard &s, int k) { return s.tick ? tlb_tick_set_gain_db(s.tick, k, gain_db) : tlb_set_gain_db(s.batch, k, gain_db); };
    if (stream < 0) {
        for (double &g : nd->gain_db) g = gain_db;
        for (Shard *s : nd->shards) if (s->late) s->gain_missed = true;
        return nd->live("set_gain_db", [&](Shard &s) { return f(s, -1); });
    }
    nd->gain_db[(size_t)stream] = gain_db;
    int k; Shard *s;
    const int rc = nd->gate(stream, &s, &k);
    if (rc == TLB_ERR_LATE) s->gain_missed = true;
    if (rc) return rc;
    return nd->one(s->index, [&](Shard &sh) { return f(sh, k); });
}
int tlb_node_stream_reset(tlb_node *nd, int stream)
{
    int k; Shard *s;
    if (int rc = nd ? nd->gate(stream, &s, &k) : (int)TLB_ERR_ARG) return rc;
    return nd->one(s->index, [&](Shard &sh) { return sh.tick ? tlb_tick_stream_reset(sh.tick, k) : tlb_stream_reset(sh.batch, k); });
}
int tlb_node_stream_finish(tlb_node *nd, int stream, uint8_t *out, size_t out_size)
{
    int k; Shard *s;
    if (int rc = nd ? nd->gate(stream, &s, &k) : (int)TLB_ERR_ARG) return -rc;
    return nd->one(s->index, [&](Shard &sh) { return sh.tick ? tlb_tick_stream_finish(sh.tick, k, out, out_size) : tlb_stream_finish(sh.batch, k, out, out_size); });
}
int tlb_node_stream_reconfigure(tlb_node *nd, int stream, const tlb_stream_config *cfg)
{
    int k; Shard *s;
    if (!nd || !cfg) return TLB_ERR_ARG;
    if (int rc = nd->gate(stream, &s, &k)) return rc;
    const int rc = nd->one(s->index, [&](Shard &sh) { return sh.tick ? tlb_tick_stream_reconfigure(sh.tick, k, cfg) : tlb_stream_reconfigure(sh.batch, k, cfg); });
    if (!rc) nd->cfgs[(size_t)stream] = *cfg;                        // a restart of the shard re-creates the stream as it is NOW
    if (rc) return rc;
    // what the stream's new rate or channel count no longer fits has been removed by its object, and is forgotten here (an up source stays)
    for (int f = TLB_IN_DOWN_SOURCE; f < TLB_IN_SHORT_READS; f++) {
        if (nd->kept[f].empty()) continue;
        NodeInput &v = nd->kept[f][(size_t)stream];
        const bool fits = f != TLB_IN_FEED ? tlb_down_pair(v.samplerate, cfg->samplerate)
                        : v.adapted    ? node_rates_adapt(v.samplerate, cfg->samplerate)
                                       : v.samplerate == cfg->samplerate && v.channels == (cfg->mode == 'm' ? 1 : 2);
        if (v.samplerate && !fits) v = NodeInput{};
    }
    return rc;
}

// ---- BATCH plane ----
tlb_batch *tlb_node_batch(tlb_node *nd, int shard)
{
    return nd && shard >= 0 && shard < (int)nd->shards.size() && nd->shards[(size_t)shard]->on() ? nd->shards[(size_t)shard]->batch : nullptr;
}
void *tlb_node_device_alloc(tlb_node *nd, int shard, size_t bytes)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size() || !bytes) return nullptr;
    void *p = nullptr;
    nd->one(shard, [&](Shard &s) {
        if (hipSetDevice(s.device) != hipSuccess || hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return (int)TLB_ERR_HIP; }
        if (hipMemset(p, 0, bytes) != hipSuccess) { (void)hipFree(p); p = nullptr; return (int)TLB_ERR_HIP; }   // never a buffer that is not zeroed
        return 0;
    });
    return p;
}
void tlb_node_device_free(tlb_node *nd, int shard, void *d_ptr)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size() || !d_ptr) return;
    nd->one(shard, [&](Shard &s) { (void)hipSetDevice(s.device); (void)hipFree(d_ptr); return 0; });
}
int tlb_node_copy_in(tlb_node *nd, int shard, void *d_dst, const void *src, size_t bytes)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size() || !d_dst || !src) return TLB_ERR_ARG;
    return nd->one(shard, [&](Shard &s) { return hipSetDevice(s.device) == hipSuccess && hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess ? 0 : (int)TLB_ERR_HIP; });
}
int tlb_node_copy_out(tlb_node *nd, int shard, void *dst, const void *d_src, size_t bytes)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size() || !dst || !d_src) return TLB_ERR_ARG;
    return nd->one(shard, [&](Shard &s) {
        if (hipSetDevice(s.device) != hipSuccess) return (int)TLB_ERR_HIP;
        if (s.stream && hipStreamSynchronize(s.stream) != hipSuccess) return (int)TLB_ERR_HIP;
        return hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess ? 0 : (int)TLB_ERR_HIP;
    });
}
int tlb_node_encode_device(tlb_node *nd, const int16_t *const *d_pcm, int nframes, const uint8_t *const *d_xpad,
                           const int32_t *const *d_xpad_len, uint8_t *const *d_out, int32_t *const *d_out_len)
{
    if (!nd || nd->plane != TLB_NODE_BATCH || !d_pcm || !d_out || nframes <= 0) return TLB_ERR_ARG;
    const double t0 = now_ns();
    const int rc = nd->live("tlb_encode_device_len", [&](Shard &s) {
        const int g = s.index;
        const double t = now_ns();
        if (hipSetDevice(s.device) != hipSuccess) return (int)TLB_ERR_HIP;
        std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
        if (!s.ev_pool.empty()) { ev = s.ev_pool.back(); s.ev_pool.pop_back(); }
        else if (hipEventCreate(&ev.first) != hipSuccess || hipEventCreate(&ev.second) != hipSuccess) return (int)TLB_ERR_HIP;
        int r = hipEventRecord(ev.first, s.stream) == hipSuccess ? 0 : (int)TLB_ERR_HIP;
        if (!r) r = tlb_encode_device_len(s.batch, d_pcm[g], nframes, d_xpad ? d_xpad[g] : nullptr, d_xpad_len ? d_xpad_len[g] : nullptr,
                                          d_out[g], d_out_len ? d_out_len[g] : nullptr, s.stream);
        if (!r && hipEventRecord(ev.second, s.stream) != hipSuccess) r = (int)TLB_ERR_HIP;
        if (r) { s.ev_pool.push_back(ev); return r; }
        s.ev_flight.push_back(ev);
        s.t_submit.push_back(t); s.f_submit.push_back((long)s.n * nframes);
        return 0;
    });
    nd->t_submit.push_back(t0);
    return rc;
}
int tlb_node_flush_device(tlb_node *nd, uint8_t *const *d_out, int32_t *const *d_out_len)
{
    if (!nd || nd->plane != TLB_NODE_BATCH || !d_out) return TLB_ERR_ARG;
    return nd->live("tlb_flush_device_len", [&](Shard &s) { return tlb_flush_device_len(s.batch, d_out[s.index], d_out_len ? d_out_len[s.index] : nullptr, s.stream); });
}
int tlb_node_sync(tlb_node *nd)
{
    if (!nd || nd->plane != TLB_NODE_BATCH) return TLB_ERR_ARG;
    const int rc = nd->live("hipStreamSynchronize", [&](Shard &s) {
        if (hipSetDevice(s.device) != hipSuccess || hipStreamSynchronize(s.stream) != hipSuccess) return (int)TLB_ERR_HIP;
        const double t = now_ns();
        if (!s.t_submit.empty()) {
            // launches of one shard run in order on its stream: what is in flight is busy from the oldest submit to now
            s.busy_ns += t - s.t_submit.front();
            for (auto &e : s.ev_flight) {                           // every queued launch has its own pair of events: the sum is exact
                float ms = 0;
                if (hipEventElapsedTime(&ms, e.first, e.second) == hipSuccess && ms > 0) s.device_ms += ms;
                s.ev_pool.push_back(e);
            }
            s.ev_flight.clear();
            while (!s.t_submit.empty()) { s.frames += s.f_submit.front(); s.steps++; s.t_submit.pop_front(); s.f_submit.pop_front(); }
        }
        return 0;
    });
    if (!nd->t_submit.empty()) { nd->wall_ns += now_ns() - nd->t_submit.front(); nd->t_submit.clear(); }
    return rc;
}
#ifdef TLB_FAULT_INJECT
// test builds only (csrc/tlb_debug.h): the nth launch / tick from now of ONE shard fails as a device call would
int tlb_debug_node_fail_next(tlb_node *nd, int shard, int nth)
{
    if (!nd || shard < 0 || shard >= (int)nd->shards.size()) return TLB_ERR_ARG;
    Shard &s = *nd->shards[(size_t)shard];
    if (s.late) return TLB_ERR_LATE;
    return s.tick ? tlb_debug_tick_fail_next(s.tick, nth) : s.batch ? tlb_debug_fail_next(s.batch, nth) : (int)TLB_ERR_ARG;
}
// ... the nth wait job of ONE shard from now holds its host thread `ms` after its tick is complete, then returns rc
int tlb_debug_node_stall_next(tlb_node *nd, int shard, int nth, int ms, int rc)
{
    if (!nd || nd->plane != TLB_NODE_TICK || shard < 0 || shard >= (int)nd->shards.size() || nth < 0 || ms < 0) return TLB_ERR_ARG;
    Shard &s = *nd->shards[(size_t)shard];
    if (s.late) return TLB_ERR_LATE;                                 // (its fields belong to the job it is running)
    s.stall_nth = nth; s.stall_ms = ms; s.stall_rc = rc;
    return TLB_OK;
}
#endif

}  // extern "C"
