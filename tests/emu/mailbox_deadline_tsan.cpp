// mailbox_deadline_tsan.cpp -- the mailbox's timed join (csrc/tlb_mailbox.h: join_job_until, poll, busy) driven with fake jobs the way
// csrc/tlb_node.cpp drives its shards under a tick deadline, for ThreadSanitizer (tests/test_mailbox_deadline_tsan.py builds this with
// -fsanitize=thread and expects a clean exit and the sentinel line).  What the node does: post one job to every shard that is not late,
// join each up to the deadline; a shard whose job is still running there goes LATE and is skipped while the others go on; at the poll
// point the node asks the late mailbox without waiting, and only once poll() has reported the job done does it read the shard's own
// fields again.  A late job that returns an error leaves its shard broken.  Jobs own what they use: they are posted from a stack frame
// that returns before they do.
//
// "Late" is not made with wall-clock slack: a job that must miss its deadline holds on a gate the poster opens only AFTER
// join_job_until() has returned false, and sets a flag when it is past the gate -- so the false answer is checked against a job that
// provably had not returned.
//
// GCC 11's ThreadSanitizer runtime has no interceptor for pthread_cond_clockwait, which libstdc++ uses under a steady_clock wait_until,
// and then misreads the wait's re-lock of the mutex as a double lock.  Under the sanitizer this driver therefore builds the mailbox on
// libstdc++'s portable path -- the same predicate and mutex, pthread_cond_timedwait underneath -- which the sanitizer does see.
#if defined(__SANITIZE_THREAD__) && __has_include(<bits/c++config.h>)
#include <bits/c++config.h>
#undef _GLIBCXX_USE_PTHREAD_COND_CLOCKWAIT
#endif
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <thread>
#include <vector>

#include "../../odr-audioenc_amd/csrc/tlb_mailbox.h"

using Clock = std::chrono::steady_clock;

struct Gate {
    std::atomic<bool> entered{false}, open{false}, passed{false};
    void hold()
    {
        entered = true;
        while (!open) std::this_thread::sleep_for(std::chrono::microseconds(50));
        passed = true;
    }
};

struct FakeShard : TlbMailbox {
    int index = 0;
    // the shard's own fields: written inside jobs, read by the poster only after a join / a poll that reported the job done
    long steps = 0, frames = 0;
    bool broken = false;
    // node-side records: the poster's alone
    bool late = false;
    long kept_steps = 0, late_events = 0, rejoins = 0, missed = 0;
    std::shared_ptr<Gate> gate;
};

static int fails = 0;
#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed line %d: %s\n", __LINE__, #c); fails++; } } while (0)

// a job posted from a frame that returns before the job does: everything it uses is owned by the job
static void post_owned(FakeShard *s, int round, std::shared_ptr<Gate> gate, int rc)
{
    auto data = std::make_shared<std::vector<long>>(64, (long)round);     // the caller's locals, copied into shared ownership
    auto fn = std::make_shared<const std::function<int(FakeShard &)>>([data, gate, rc](FakeShard &sh) {
        if (gate) gate->hold();
        long sum = 0;
        for (long v : *data) sum += v;
        if (rc) { sh.broken = true; return rc; }
        sh.steps++; sh.frames += sum / 64 + 1;
        return 0;
    });
    s->post([s, fn] { return (*fn)(*s); });
}

int main(int argc, char **argv)
{
    const int nshards = 4, rounds = argc > 1 ? atoi(argv[1]) : 400;
    std::vector<FakeShard *> sh;
    for (int g = 0; g < nshards; g++) {
        FakeShard *s = new FakeShard;
        s->index = g;
        sh.push_back(s);
        s->start();
    }
    // (1) nothing posted: a timed join and a poll answer at once, nothing is busy
    for (FakeShard *s : sh) {
        int r = -1;
        CHECK(!s->busy());
        CHECK(s->join_job_until(Clock::now(), &r) && r == 0);
        CHECK(s->poll(&r) && r == 0);
    }
    long in_time = 0, went_late = 0, came_back = 0, broke = 0, reads = 0;
    for (int r = 0; r < rounds; r++) {
        // which shard stalls this round (and whether its late job returns an error): shard 1 every 5th round, shard 3 every 7th
        const int stall = r % 5 == 2 ? 1 : r % 7 == 4 ? 3 : -1;
        const int stall_rc = r % 3 == 0 ? 17 : 0;
        // "submit / wait": post to every shard that is not late and not broken, from a frame that returns before the jobs do
        std::vector<FakeShard *> on;
        for (FakeShard *s : sh) {
            if (s->late) { s->missed++; continue; }
            if (s->broken) continue;
            s->kept_steps = s->steps;                          // the node's record of a shard, taken while it is idle
            std::shared_ptr<Gate> g = s->index == stall ? std::make_shared<Gate>() : nullptr;
            s->gate = g;
            post_owned(s, r, g, s->index == stall ? stall_rc : 0);
            on.push_back(s);
        }
        const Clock::time_point due = Clock::now() + std::chrono::seconds(20);      // the healthy jobs are far inside it
        for (FakeShard *s : on) {
            int rc = -1;
            if (s->gate) {
                while (!s->gate->entered) std::this_thread::sleep_for(std::chrono::microseconds(50));
                CHECK(s->busy());
                // its deadline has passed (a time point already behind us): the job is held on the gate, so the answer must be false
                CHECK(!s->join_job_until(Clock::now(), &rc));
                CHECK(!s->gate->passed);
                CHECK(!s->poll(&rc));
                s->late = true; s->late_events++; went_late++;
                continue;
            }
            CHECK(s->join_job_until(due, &rc));
            CHECK(rc == 0);
            in_time++;
        }
        // the poster reads counters while a late job is still running: the healthy shards' own fields, the late ones' node-side records
        long sum = 0;
        for (FakeShard *s : sh) sum += s->late ? s->kept_steps : s->steps;
        reads += sum > 0;
        // the late job may go on: open its gate (a real stall ends on its own)
        for (FakeShard *s : sh) if (s->late && s->gate) s->gate->open = true;
        // "poll point": without blocking; a shard is read again only after poll() has reported its job done
        for (int spin = 0; spin < 200000; spin++) {
            bool any = false;
            for (FakeShard *s : sh) {
                if (!s->late) continue;
                int rc = -1;
                if (!s->poll(&rc)) { any = true; continue; }
                s->late = false;
                CHECK(s->gate && s->gate->passed);
                s->gate.reset();
                if (rc) { CHECK(rc == 17 && s->broken); broke++; }
                else { CHECK(!s->broken && s->steps == s->kept_steps + 1); s->rejoins++; came_back++; }
                CHECK(!s->busy());
            }
            if (!any) break;
            std::this_thread::sleep_for(std::chrono::microseconds(100));
        }
        for (FakeShard *s : sh) CHECK(!s->late);
        // "restart" of a broken shard on its own thread, joined without a limit as the node does
        for (FakeShard *s : sh)
            if (s->broken && r % 4 == 3) {
                s->post([s] { s->broken = false; s->steps = 0; s->frames = 0; return 0; });
                CHECK(s->join_job() == 0);
            }
    }
    // teardown: a job still running would be joined without a limit first (tlb_node_destroy)
    long steps = 0;
    for (FakeShard *s : sh) {
        if (s->busy()) (void)s->join_job();
        s->post([s] { s->frames++; return 0; });
        s->join_job();
        s->stop();
        steps += s->steps;
        delete s;
    }
    if (fails || !went_late || !came_back || !broke || !in_time) { fprintf(stderr, "fails %d late %ld back %ld broke %ld\n", fails, went_late, came_back, broke); return 1; }
    printf("mailbox deadline ok: %d rounds, %ld in time, %ld late, %ld back on their own, %ld broke late, %ld steps, %ld reads\n",
           rounds, in_time, went_late, came_back, broke, steps, reads);
    return 0;
}
