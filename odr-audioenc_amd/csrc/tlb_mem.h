// tlb_mem.h -- the ONE owner of the device and pinned host memory the library's host side allocates.  A long-lived owner sits in the batch
// (tlb_batch::mem) and in the tick object (tlb_tick::mem) and frees what it holds when the object goes; a local one stages the buffers of a
// first-use *_prepare or an opt-in and hands them over in one step that cannot fail (commit), or frees them on every other way out.  The
// *_host convenience entry points keep their scratch in a local one.  Host C++ on the HIP runtime API only.  Not a general allocator.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdio.h>
#include <string.h>

#include <vector>
#ifdef TLB_FAULT_INJECT
#include <atomic>
#endif

struct TlbMem {
    TlbMem() = default;
    TlbMem(const TlbMem &) = delete;
    TlbMem &operator=(const TlbMem &) = delete;
    ~TlbMem() { for (void *p : dev_) (void)hipFree(p); for (void *p : pinned_) (void)hipHostFree(p); }

    // n elements of device memory, zeroed (on the null stream: see settle).  n = 0 gives a valid smallest buffer, never NULL: "present but empty".
    template <class T> T *dev(size_t n) { return (T *)get(n * sizeof(T), DEV_ZEROED); }
    // ... not zeroed: for a buffer the caller writes whole before anything reads it, on a path that must queue no memset
    template <class T> T *scratch(size_t n) { return (T *)get(n * sizeof(T), DEV); }
    // ... of pinned host memory, zeroed
    template <class T> T *pinned(size_t n) { return (T *)get(n * sizeof(T), PINNED); }
    // a table for a buffer of this owner, host to device; like the allocations it does nothing once the owner has failed
    void upload(void *dst, const void *src, size_t bytes) { if (!failed()) note(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy", bytes); }
    // The zeroing and the uploads ran on the null stream, and the objects' own streams are non-blocking ones that do not wait for it: before
    // a buffer made here is used on one of them the device is waited for, once.  False when that, or anything before it, failed.
    bool settle() { if (!failed()) note(hipDeviceSynchronize(), "hipDeviceSynchronize", 0); return !failed(); }
    // The first failure sticks: every later request returns NULL without a call, so a run of them is checked once, here.
    bool failed() const { return err_ != hipSuccess; }
    // everything this owner holds now belongs to `to` (the batch's or the tick's owner)
    void commit(TlbMem &to)
    {
        to.dev_.insert(to.dev_.end(), dev_.begin(), dev_.end()); dev_.clear();
        to.pinned_.insert(to.pinned_.end(), pinned_.begin(), pinned_.end()); pinned_.clear();
    }
#ifdef TLB_FAULT_INJECT
    // test builds only (csrc/tlb_debug.h, tlb_debug_alloc_fail_next): the fail_in-th request from now, process-wide, is refused without a call
    static inline std::atomic<int> fail_in{0};
#endif

private:
    enum Kind { DEV, DEV_ZEROED, PINNED };
    std::vector<void *> dev_, pinned_;
    hipError_t err_ = hipSuccess;
    void note(hipError_t e, const char *what, size_t bytes)
    {
        if (e == hipSuccess) return;
        fprintf(stderr, "libtoolame-dab-hip: %s (%zu bytes) failed: %s\n", what, bytes, hipGetErrorString(e));
        err_ = e;
    }
    void *get(size_t bytes, Kind kind)
    {
        if (failed()) return nullptr;
        if (!bytes) bytes = 4;
#ifdef TLB_FAULT_INJECT
        for (int v = fail_in.load(); v > 0;)
            if (fail_in.compare_exchange_weak(v, v - 1)) { if (v == 1) { note(hipErrorOutOfMemory, "injected refusal", bytes); return nullptr; } break; }
#endif
        void *p = nullptr;
        note(kind == PINNED ? hipHostMalloc(&p, bytes, hipHostMallocDefault) : hipMalloc(&p, bytes), kind == PINNED ? "hipHostMalloc" : "hipMalloc", bytes);
        if (failed()) return nullptr;
        (kind == PINNED ? pinned_ : dev_).push_back(p);              // owned from here on, whatever the zeroing says
        if (kind == PINNED) memset(p, 0, bytes);
        if (kind == DEV_ZEROED) note(hipMemset(p, 0, bytes), "hipMemset", bytes);
        return failed() ? nullptr : p;
    }
};
