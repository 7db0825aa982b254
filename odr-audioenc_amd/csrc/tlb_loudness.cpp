// tlb_loudness.cpp -- the batch-level entry points of the loudness meter (include/toolame_batch.h, tlb_loudness_*): the committed table,
// the per-stream state (allocated by tlb_loudness_enable alone) and one launch of a kernel of toolame_loudness.hip through tl_kernels.h.
// Host C++.
#include <stddef.h>
#include "tlb_internal.h"
#include "tl_loudness_tables.inc"

static_assert(sizeof(tlb_loudness_record) == sizeof(TlLoudnessRecord) && sizeof(tlb_loudness_record) == 48, "C-ABI record");
static_assert(offsetof(tlb_loudness_record, frames) == offsetof(TlLoudnessRecord, frames) && offsetof(tlb_loudness_record, gated) == offsetof(TlLoudnessRecord, gated) &&
              offsetof(tlb_loudness_record, momentary) == offsetof(TlLoudnessRecord, momentary) && offsetof(tlb_loudness_record, short_term_max) == offsetof(TlLoudnessRecord, short_term_max), "record layout");
static_assert(sizeof(tlb_loudness_programme_record) == sizeof(TlLoudnessProgramme) && sizeof(tlb_loudness_programme_record) == 24 &&
              offsetof(tlb_loudness_programme_record, gated) == offsetof(TlLoudnessProgramme, gated), "C-ABI programme record");
static_assert(sizeof tl_loudness_taps == TL_LD_RATES * 10 * sizeof(double) && sizeof tl_loudness_edges == TL_LD_BINS * sizeof(double) &&
              sizeof tl_loudness_centres == TL_LD_BINS * sizeof(double) && TLB_LOUDNESS_BINS == TL_LD_BINS, "table shapes");
static_assert(sizeof(tlb_lra_record) == sizeof(TlLraRecord) && sizeof(tlb_lra_record) == 40 && offsetof(tlb_lra_record, gate) == offsetof(TlLraRecord, gate) &&
              offsetof(tlb_lra_record, blocks) == offsetof(TlLraRecord, blocks) && offsetof(tlb_lra_record, high_bin) == offsetof(TlLraRecord, high_bin) &&
              offsetof(tlb_lra_record, high_bin) == 36, "C-ABI range record");

// the loudness state of streams [s0, s0 + n) back to zero (the life-cycle calls; the device is idle).  The arrays are laid out by row with
// the streams side by side, so a range of streams is a column block of each
int loudness_clear_streams(tlb_batch *b, int s0, int n)
{
    if (!b->d_ld_lane) return TLB_OK;
    const size_t ns = (size_t)b->nstreams;
    HIPCHK(hipMemset2D(b->d_ld_lane + 2 * (size_t)s0, 2 * ns * sizeof(double), 0, 2 * (size_t)n * sizeof(double), TL_LD_LANE_WORDS));
    HIPCHK(hipMemset2D(b->d_ld_ring + s0, ns * sizeof(double), 0, (size_t)n * sizeof(double), TL_LD_RING));
    HIPCHK(hipMemset2D(b->d_ld_hist + s0, ns * sizeof(uint32_t), 0, (size_t)n * sizeof(uint32_t), TL_LD_HIST_ROWS));
    if (b->d_ld_hist_st) HIPCHK(hipMemset2D(b->d_ld_hist_st + s0, ns * sizeof(uint32_t), 0, (size_t)n * sizeof(uint32_t), TL_LD_HIST_ROWS));      // (tlb_lra_*: EBU Mode has one reset)
    HIPCHK(hipMemset(b->d_ld_rec + s0, 0, (size_t)n * sizeof(TlLoudnessRecord)));
    HIPCHK(hipDeviceSynchronize());              // the callers' streams do not wait for the null stream
    return TLB_OK;
}

extern "C" {

int tlb_loudness_taps(long samplerate, double out[10])
{
    const int row = tl_ld_rate_row(samplerate);
    if (!out) return TLB_ERR_ARG;
    if (row < 0) return TLB_ERR_SAMPLERATE;
    memcpy(out, tl_loudness_taps[row], sizeof tl_loudness_taps[row]);
    return TLB_OK;
}

int tlb_loudness_scale(double edges[751], double centres[751])
{
    if (edges) memcpy(edges, tl_loudness_edges, sizeof tl_loudness_edges);
    if (centres) memcpy(centres, tl_loudness_centres, sizeof tl_loudness_centres);
    return TLB_OK;
}

double tlb_loudness_lufs(double energy) { return energy > 0.0 ? -0.691 + 10.0 * log10(energy) : -INFINITY; }

int tlb_loudness_enable(tlb_batch *b)
{
    if (!b) return TLB_ERR_ARG;
    if (b->d_ld_lane) return TLB_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t ns = (size_t)b->nstreams;
    TlbMem m;
    double *lane = m.dev<double>(TL_LD_LANE_WORDS * 2 * ns), *ring = m.dev<double>(TL_LD_RING * ns);
    TlLoudnessRecord *rec = m.dev<TlLoudnessRecord>(ns);
    uint32_t *hist = m.dev<uint32_t>(TL_LD_HIST_ROWS * ns);
    TlLoudnessProgramme *prog = m.scratch<TlLoudnessProgramme>(ns);
    double *tab = m.scratch<double>(TL_LD_TABLE_DOUBLES);
    m.upload(tab, tl_loudness_taps, sizeof tl_loudness_taps);
    m.upload(tab + TL_LD_RATES * 10, tl_loudness_edges, sizeof tl_loudness_edges);
    m.upload(tab + TL_LD_RATES * 10 + TL_LD_BINS, tl_loudness_centres, sizeof tl_loudness_centres);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_ld_lane = lane; b->d_ld_ring = ring; b->d_ld_rec = rec; b->d_ld_hist = hist; b->d_ld_prog = prog; b->d_ld_tables = tab;
    return TLB_OK;
}

int tlb_loudness_device(tlb_batch *b, const int16_t *d_pcm_planar, int nframes, tlb_loudness_record *d_records, void *hip_stream)
{
    if (!b || !d_pcm_planar || nframes <= 0 || (long long)nframes * b->nstreams > (1ll << 30)) return TLB_ERR_ARG;
    if (((uintptr_t)d_pcm_planar & 15u) || ((uintptr_t)d_records & 7u)) return TLB_ERR_ARG;      // the PCM comes in as 16-byte pieces
    if (!b->d_ld_lane) return TLB_ERR_ARG;       // never enabled
    if (b->broken) return TLB_ERR_HIP;           // the device's stream -> configuration table may disagree with the host's (tlb_reset)
    HIPCHK(hipSetDevice(b->device));
    const TlLoudnessArgs A = {d_pcm_planar, b->d_ld_lane, b->d_ld_ring, b->d_ld_rec, (TlLoudnessRecord *)d_records, b->d_ld_hist, b->d_ld_tables,
                              b->d_configs, b->d_stream_cfg, b->nstreams, nframes};
    // a batch with the loudness range on runs the counting twin in the kernel's place: one launch either way
    if (b->d_ld_hist_st) { const TlLraArgs X = {A, b->d_ld_hist_st}; HIPCHK(tlk_lra((hipStream_t)hip_stream, X)); }
    else HIPCHK(tlk_loudness((hipStream_t)hip_stream, A));
    return TLB_OK;
}

int tlb_loudness_host(tlb_batch *b, const int16_t *pcm_planar, int nframes, tlb_loudness_record *records)
{
    return meter_host(b, b ? b->d_ld_lane : nullptr, pcm_planar, nframes, records, tlb_loudness_device);
}

int tlb_loudness_programme_device(tlb_batch *b, tlb_loudness_programme_record *d_out, void *hip_stream)
{
    if (!b || !d_out || ((uintptr_t)d_out & 7u) || !b->d_ld_lane) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_loudness_programme((hipStream_t)hip_stream, b->d_ld_hist, b->d_ld_tables, (TlLoudnessProgramme *)d_out, b->nstreams));
    return TLB_OK;
}

int tlb_loudness_programme_host(tlb_batch *b, tlb_loudness_programme_record *out)
{
    if (!b || !out || !b->d_ld_lane) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());              // launches queued on the caller's streams have written their counts
    if (int rc = tlb_loudness_programme_device(b, (tlb_loudness_programme_record *)b->d_ld_prog, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, b->d_ld_prog, (size_t)b->nstreams * sizeof(tlb_loudness_programme_record), hipMemcpyDeviceToHost));
    return TLB_OK;
}

int tlb_loudness_reset(tlb_batch *b, int stream) { return meter_reset(b, b ? b->d_ld_lane : nullptr, stream, loudness_clear_streams); }

// Loudness range (tlb_lra_*): the second histogram, made here alone; the counting is tlb_loudness_device's other kernel.
int tlb_lra_enable(tlb_batch *b)
{
    if (!b || !b->d_ld_lane) return TLB_ERR_ARG;         // on top of the loudness meter only
    if (b->d_ld_hist_st) return TLB_OK;
    HIPCHK(hipSetDevice(b->device));
    const size_t ns = (size_t)b->nstreams;
    TlbMem m;
    uint32_t *hist_st = m.dev<uint32_t>(TL_LD_HIST_ROWS * ns);
    TlLraRecord *lra = m.scratch<TlLraRecord>(ns);
    if (!m.settle()) return TLB_ERR_HIP;
    m.commit(b->mem);
    b->d_ld_hist_st = hist_st; b->d_ld_lra = lra;
    return TLB_OK;
}

int tlb_lra_device(tlb_batch *b, tlb_lra_record *d_out, void *hip_stream)
{
    if (!b || !d_out || ((uintptr_t)d_out & 7u) || !b->d_ld_hist_st) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(tlk_lra_range((hipStream_t)hip_stream, b->d_ld_hist_st, b->d_ld_tables, (TlLraRecord *)d_out, b->nstreams));
    return TLB_OK;
}

int tlb_lra_host(tlb_batch *b, tlb_lra_record *out)
{
    if (!b || !out || !b->d_ld_hist_st) return TLB_ERR_ARG;
    HIPCHK(hipSetDevice(b->device));
    HIPCHK(hipDeviceSynchronize());              // launches queued on the caller's streams have written their counts
    if (int rc = tlb_lra_device(b, (tlb_lra_record *)b->d_ld_lra, nullptr)) return rc;
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(out, b->d_ld_lra, (size_t)b->nstreams * sizeof(tlb_lra_record), hipMemcpyDeviceToHost));
    return TLB_OK;
}

double tlb_lra_lu(const tlb_lra_record *rec) { return rec ? 0.1 * (double)(rec->high_bin - rec->low_bin) : 0.0; }

}  // extern "C"
