// tlb_conceal.cpp -- the batch-level entry points of the feed concealment (include/toolame_batch.h, tlb_conceal_*): the per-stream
// parameters, record and G buffer (allocated by the first tlb_conceal_enable or tlb_feed_loss_enable that switches concealment on) and
// the launch of the kernels of toolame_conceal.hip behind the feed's own (tlb_feed.cpp: feed_launch) through tl_kernels.h.  The adapted
// and the down path queue the kernels of toolame_conceal_conv.hip themselves, with the arrays conceal_conv hands them.  Host C++.
#include <stddef.h>
#include "tlb_internal.h"

static_assert(sizeof(tlb_conceal_record) == sizeof(TlConcealRecord) && sizeof(tlb_conceal_record) == 32, "C-ABI record");
static_assert(offsetof(tlb_conceal_record, frames) == offsetof(TlConcealRecord, frames) && offsetof(tlb_conceal_record, concealed) == offsetof(TlConcealRecord, concealed) &&
              offsetof(tlb_conceal_record, longest) == offsetof(TlConcealRecord, longest) && offsetof(tlb_conceal_record, run) == offsetof(TlConcealRecord, run) &&
              offsetof(tlb_conceal_record, offset) == offsetof(TlConcealRecord, offset), "record layout");
static_assert(TLB_CONCEAL_MAX_HOLD == TL_CC_MAX_HOLD && TLB_CONCEAL_MAX_STEP == TL_CC_MAX_STEP && TLB_CONCEAL_MUTE == TL_CC_MUTE, "the rule's constants");

// streams [s0, s0 + n): the record zero, G forgotten (its length 0), the parameters as the host holds them (off: switched off first)
int conceal_clear_streams(tlb_batch *b, int s0, int n, bool off)
{
    if (!b->d_cc_state) return TLB_OK;
    for (int s = s0; s < s0 + n && off; s++) b->cc_host[(size_t)s].hold = b->cc_host[(size_t)s].step = 0;
    b->n_conceal = b->n_conceal_adapt = b->n_conceal_down = 0;
    for (int s = 0; s < b->nstreams; s++)
        if (b->cc_host[(size_t)s].hold) ++*(b->fd.on(s) ? &b->n_conceal_down : tlb_feed_adapted(b, s) > 0 ? &b->n_conceal_adapt : &b->n_conceal);
    HIPCHK(hipMemcpy(b->d_cc_state + s0, b->cc_host.data() + s0, (size_t)n * sizeof(TlConcealStream), hipMemcpyHostToDevice));
    HIPCHK(hipMemset(b->d_cc_rec + s0, 0, (size_t)n * sizeof(TlConcealRecord)));
    HIPCHK(hipDeviceSynchronize());              // the callers' streams do not wait for the null stream
    return TLB_OK;
}

int conceal_clear_family(tlb_batch *b, int s0, int n, bool down, bool off)
{
    if (!b->d_cc_state) return TLB_OK;
    const auto other = [&](int s) { return down ? b->feed.on(s) : b->fd.on(s); };     // (a stream has one feed: csrc/tlb_inputs.h)
    for (int s = s0; s < s0 + n;) {
        if (other(s)) { s++; continue; }
        int e = s;
        while (e < s0 + n && !other(e)) e++;
        if (int rc = conceal_clear_streams(b, s, e - s, off)) return rc;
        s = e;
    }
    return TLB_OK;
}

const TlConcealConv *conceal_conv(const tlb_batch *b, bool down, TlConcealConv *x)
{
    if (!(down ? b->n_conceal_down : b->n_conceal_adapt)) return nullptr;
    x->cs = b->d_cc_state; x->rec = b->d_cc_rec; x->g = b->d_cc_g; x->g_stride = b->cc_g_stride; x->pad_ = 0;
    return x;
}

// room for slots of `stride` bytes in the G buffer; what it holds is kept (the device is idle).  An owner of its own, as d_feed_prev has
int conceal_g_reserve(tlb_batch *b, int stride)
{
    if (!b->d_cc_state || stride <= b->cc_g_stride) return TLB_OK;
    std::unique_ptr<TlbMem> m(new TlbMem);
    uint8_t *ng = m->dev<uint8_t>((size_t)b->nstreams * (size_t)stride);
    if (m->failed()) return TLB_ERR_HIP;
    if (b->d_cc_g)
        HIPCHK(hipMemcpy2D(ng, (size_t)stride, b->d_cc_g, (size_t)b->cc_g_stride, (size_t)b->cc_g_stride, (size_t)b->nstreams, hipMemcpyDeviceToDevice));
    if (!m->settle()) return TLB_ERR_HIP;
    b->cc_g_mem.swap(m);
    b->d_cc_g = ng; b->cc_g_stride = stride;
    return TLB_OK;
}

// the first enable that switches concealment on: parameters (all off), records, and G as wide as the widest feed history slot of any kind
static int conceal_prepare(tlb_batch *b)
{
    if (b->d_cc_state) return TLB_OK;
    const size_t n = (size_t)b->nstreams;
    TlbMem m;
    TlConcealStream *st = m.dev<TlConcealStream>(n);
    TlConcealRecord *rec = m.dev<TlConcealRecord>(n);
    if (!m.settle()) return TLB_ERR_HIP;
    b->cc_host.assign(n, TlConcealStream{0, 0, 0, 0});
    b->d_cc_state = st;
    const int wide = b->d_fd_cfg && b->feed_prev_stride < TL_FD_PREV_STRIDE ? TL_FD_PREV_STRIDE : b->feed_prev_stride;
    if (int rc = conceal_g_reserve(b, wide)) { b->d_cc_state = nullptr; b->cc_host.clear(); return rc; }
    m.commit(b->mem);
    b->d_cc_rec = rec;
    return TLB_OK;
}

int conceal_launch(tlb_batch *b, const TlFeedLaunch &A, void *hip_stream)
{
    if (!b->n_conceal) return TLB_OK;
    TlConcealLaunch C;
    memset(&C, 0, sizeof C);
    C.F = A; C.cs = b->d_cc_state; C.rec = b->d_cc_rec; C.g = b->d_cc_g; C.g_stride = b->cc_g_stride;
    HIPCHK(tlk_conceal((hipStream_t)hip_stream, C));
    return TLB_OK;
}

// any_feed: an adapted or a down feed will do (tlb_feed_loss_enable)
static int conceal_enable(tlb_batch *b, int stream, int hold, int step, bool any_feed)
{
    if (!b || stream < -1 || stream >= b->nstreams || hold < 0 || hold > TL_CC_MAX_HOLD) return TLB_ERR_ARG;
    if (hold > 0 && (step < 1 || step > TL_CC_MAX_STEP)) return TLB_ERR_ARG;
    const int s0 = stream < 0 ? 0 : stream, s1 = stream < 0 ? b->nstreams : stream + 1;
    if (hold == 0) {
        if (!b->d_cc_state) return TLB_OK;       // off, and never on: nothing to allocate or to clear
        HIPCHK(hipSetDevice(b->device));
        HIPCHK(hipDeviceSynchronize());
        return conceal_clear_streams(b, s0, s1 - s0, true);
    }
    // every named stream is checked before anything changes: a strict feed, or with any_feed a Layer II feed of any kind
    for (int s = s0; s < s1; s++) {
        const bool strict = tlb_feed_get(b, s, nullptr) > 0 && tlb_feed_adapted(b, s) == 0;
        if (!strict && !(any_feed && (tlb_feed_get(b, s, nullptr) > 0 || tlb_feed_down_get(b, s, nullptr) > 0))) return TLB_ERR_ARG;
    }
    if (b->broken) return TLB_ERR_HIP;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    if (int rc = conceal_prepare(b)) return rc;
    for (int s = s0; s < s1; s++) { b->cc_host[(size_t)s].hold = (uint32_t)hold; b->cc_host[(size_t)s].step = (uint32_t)step; }
    return conceal_clear_streams(b, s0, s1 - s0);
}

extern "C" {

int tlb_conceal_enable(tlb_batch *b, int stream, int hold, int step) { return conceal_enable(b, stream, hold, step, false); }
int tlb_feed_loss_enable(tlb_batch *b, int stream, int hold, int step) { return conceal_enable(b, stream, hold, step, true); }

int tlb_conceal_get(const tlb_batch *b, int stream, int *hold, int *step)
{
    if (!b || stream < 0 || stream >= b->nstreams) return -TLB_ERR_ARG;
    const TlConcealStream c = b->cc_host.empty() ? TlConcealStream{0, 0, 0, 0} : b->cc_host[(size_t)stream];
    if (hold) *hold = (int)c.hold;
    if (step) *step = (int)c.step;
    return c.hold ? 1 : 0;
}

int tlb_conceal_reset(tlb_batch *b, int stream)
{
    if (!b || stream < -1 || stream >= b->nstreams) return TLB_ERR_ARG;
    if (!b->d_cc_state) return TLB_OK;           // never enabled: nothing to forget
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    return stream < 0 ? conceal_clear_streams(b, 0, b->nstreams) : conceal_clear_streams(b, stream, 1);
}

int tlb_conceal_records_device(tlb_batch *b, tlb_conceal_record *d_records, void *hip_stream)
{
    if (!b || !d_records || ((uintptr_t)d_records & 3u) || !b->d_cc_rec) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipMemcpyAsync(d_records, b->d_cc_rec, (size_t)b->nstreams * sizeof(TlConcealRecord), hipMemcpyDeviceToDevice, (hipStream_t)hip_stream));
    return TLB_OK;
}

int tlb_conceal_records_host(tlb_batch *b, tlb_conceal_record *records)
{
    if (!b || !records || !b->d_cc_rec) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(records, b->d_cc_rec, (size_t)b->nstreams * sizeof(TlConcealRecord), hipMemcpyDeviceToHost));
    return TLB_OK;
}

}  // extern "C"
