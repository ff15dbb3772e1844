// pixel_batch_auto_api.cpp -- dxtlt_transform_pixels_batch_auto_device (include/dxtlt_pixels.h; docs/PIXEL_FORMAT.md, "Many buffers
// in one call"): the best of the six pixel settings for every buffer of a batch, and all of them transformed, with ONE stream wait
// and a launch count that does not grow with the number of buffers.  The pixel twin of batch_auto_api.cpp:
//   plan      (pixel_batch_plan.h) every item gets a 16-byte aligned slice of 5 x len bytes of this thread's candidate arena and
//             six counters; items are cut into chunks whose slices fit the arena cap (a larger item is a chunk by itself)
//   upload    ONE table for the whole call: per chunk the candidate launches' entries and indices and the estimator's sections
//   per chunk one candidate launch per pixel_bytes present (pixel_batch_kernels.hip) and ONE table-driven entropy launch over all
//             six sections of all items (entropy_kernels.hip; the sixth section is the item's d_input); the stream orders the
//             reuse of the arena between chunks
//   readback  all counters -- sums of q -- in one copy, ONE wait; rounded up to bytes and compared on the host, in the candidate
//             order of pixel_auto_api.cpp with strict `<` from UINT64_MAX
//   winners   the planner and kernels of dxtlt_transform_pixels_batch_device with the chosen per-item settings: enqueued, not waited for
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "../../include/dxtlt_pixels.h"
#include "batch_auto_buffers.h"
#include "entropy_launch.h"
#include "host_common.h"
#include "pixel_batch_api.h"
#include "pixel_batch_launch.h"
#include "pixel_batch_plan.h"

namespace {

using namespace dxtlt_host;
namespace pb = dxtlt_host::pixel_batch;
using pb::kCandidates;

struct PixelCandidate {
    uint8_t decorrelate, layout;
};
// the order of pixel_auto_api.cpp (include/dxtlt_pixels.h, "the auto transform")
constexpr PixelCandidate kOrder[kCandidates] = {{1, 2}, {1, 1}, {1, 0}, {0, 2}, {0, 1}, {0, 0}};

thread_local uint64_t t_last[4] = {0, 0, 0, 0};   // dxtlt_debug_pixels_batch_auto_last
thread_local std::vector<uint64_t> t_totals;      // dxtlt_debug_pixels_batch_auto_last_totals: six per item
thread_local std::vector<uint8_t> t_total_counts;
thread_local bool t_time_phases = false;
thread_local double t_phase_ms[3] = {0, 0, 0};

// the first smallest total: from the first candidate with best = UINT64_MAX, replaced on strict `<`
int pick_of(const uint64_t* totals)
{
    int pick = 0;
    uint64_t best = UINT64_MAX;
    for (int i = 0; i < kCandidates; ++i)
        if (totals[i] < best) {
            best = totals[i];
            pick = i;
        }
    return pick;
}

// the bench hook's events: three per chunk -- in front of its candidate launches, between them and its estimator launch, behind
// it -- and two around the winners; read once everything has been waited for
struct PhaseEvents {
    std::vector<hipEvent_t> ev;
    ~PhaseEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    bool begin(size_t chunks)
    {
        ev.assign(chunks * 3 + 2, nullptr);
        for (hipEvent_t& e : ev)
            if (hipEventCreate(&e) != hipSuccess)
                return false;
        return true;
    }
    void mark(size_t k, hipStream_t st)
    {
        if (!ev.empty()) (void)hipEventRecord(ev[k], st);
    }
    double between(size_t a, size_t b) const
    {
        float ms = 0;
        return hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess ? (double)ms : 0.0;
    }
};

}  // namespace

extern "C" int32_t dxtlt_transform_pixels_batch_auto_device(DxtltPixelBatchAutoItem* items, size_t count, void* hip_stream)
{
    std::memset(t_last, 0, sizeof t_last);
    t_totals.clear();
    t_total_counts.clear();
    t_phase_ms[0] = t_phase_ms[1] = t_phase_ms[2] = 0;
    auto_begin_device_call();
    if (count == 0)
        return kOk;
    pb::AutoPlan plan;
    if (pb::Defect d = pb::plan_auto_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    bool any = false;
    for (size_t i = 0; i < count && !any; ++i)
        any = items[i].len != 0;
    auto report = [&](size_t i, int pick) {
        items[i].decorrelate = kOrder[pick].decorrelate;
        items[i].layout = kOrder[pick].layout;
    };
    if (!any) {   // every estimate of an empty buffer is 0: the first candidate stays; no device needed
        for (size_t i = 0; i < count; ++i)
            report(i, 0);
        return kOk;
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    int devices = 0;
    hipError_t e = hipGetDeviceCount(&devices);
    if (e != hipSuccess || devices <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument, "the auto transforms read their estimates back and wait for the stream: not capturable");

    uint8_t* arena = static_cast<uint8_t*>(auto_thread_arena((size_t)plan.arena_bytes));
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    BatchAutoBuffers& buffers = batch_auto_thread_buffers();
    HIP_TRY(buffers.reserve(plan.table_bytes, (size_t)plan.counters), "pixel batch auto tables / counters");
    pb::fill_auto_tables(plan, items, arena, static_cast<uint8_t*>(buffers.table_host));
    const uint8_t* dev = static_cast<const uint8_t*>(buffers.table_dev);

    PhaseEvents phases;
    if (t_time_phases && !phases.begin(plan.chunks.size()))
        return fail(kDevice, "pixel batch auto: hipEventCreate", hipErrorOutOfMemory);

    // every failure exit below drains the stream: the arena, the tables and the counters belong to this thread's next call
    e = hipMemsetAsync(buffers.counters_dev, 0, (size_t)plan.counters * sizeof(uint64_t), st);
    const char* what = "pixel batch auto: counter clear";
    if (e == hipSuccess) {
        e = dxtlt::launch_table_upload(buffers.table_mapped, buffers.table_dev, (plan.table_bytes + 15) & ~size_t(15), st);
        what = "pixel batch auto: table upload";
    }
    for (size_t c = 0; c < plan.chunks.size() && e == hipSuccess; ++c) {
        const pb::AutoChunk& ch = plan.chunks[c];
        phases.mark(c * 3, st);
        for (int b = 0; b < 2 && e == hipSuccess; ++b) {
            if (ch.entries[b] == 0)
                continue;
            const uint8_t* d = dev + ch.at[b];
            e = dxtlt::pixels::launch_pixel_batch_candidates(b == 0 ? 4 : 3, reinterpret_cast<const dxtlt::pixels::PixelBatchEntry*>(d),
                                                             d + ch.entry_bytes[b], ch.entries[b], ch.wgs[b], ch.wide[b], st);
            what = "pixel batch auto: candidate kernel launch";
            if (e == hipSuccess)
                t_last[2]++;
        }
        phases.mark(c * 3 + 1, st);
        if (e == hipSuccess && ch.estimator_entries != 0) {
            e = dxtlt::launch_entropy_table(reinterpret_cast<const dxtlt::EstimateTableEntry*>(dev + ch.sections_at), ch.estimator_entries,
                                            (uint32_t)ch.estimator_wgs, buffers.counters_dev, st);
            what = "pixel batch auto: estimator launch";
            if (e == hipSuccess)
                t_last[3]++;
        }
        phases.mark(c * 3 + 2, st);
        t_last[1]++;
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(buffers.counters_host, buffers.counters_dev, (size_t)plan.counters * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        what = "pixel batch auto: D2H estimates";
    }
    const hipError_t waited = hipStreamSynchronize(st);   // the one wait of the call
    t_last[0]++;
    if (e != hipSuccess)
        return fail(kDevice, what, e);
    if (waited != hipSuccess)
        return fail(kDevice, "stream synchronize", waited);

    // the counters hold sums of q: rounded up to bytes here, as the finishing launch of the single call rounds them
    std::vector<DxtltPixelBatchItem> winners(count);
    std::vector<uint64_t> totals(count * kCandidates, 0);
    std::vector<int> picks(count, 0);
    for (size_t i = 0; i < count; ++i) {
        const pb::AutoItem& p = plan.items[i];
        if (p.len != 0) {
            for (int k = 0; k < kCandidates; ++k)
                totals[i * kCandidates + (size_t)k] =
                    (buffers.counters_host[p.first_counter + (uint64_t)k] + ((1ull << dxtlt::kEntropyShift) - 1)) >> dxtlt::kEntropyShift;
            picks[i] = pick_of(&totals[i * kCandidates]);
        }
        DxtltPixelBatchItem& w = winners[i];
        std::memset(&w, 0, sizeof w);
        w.d_input = items[i].d_input;
        w.d_output = items[i].d_output;
        w.len = items[i].len;
        w.pixel_bytes = items[i].pixel_bytes;
        w.decorrelate = kOrder[picks[i]].decorrelate;
        w.layout = kOrder[picks[i]].layout;
    }
    pb::Plan winners_plan;
    int32_t rc = kOk;
    if (pb::Defect d = pb::plan_call(winners.data(), count, winners_plan); d.code != kOk)
        rc = fail(d.code, d.what);   // (not reached: the batch passed the same checks and the per-pixel_bytes limit above)
    phases.mark(plan.chunks.size() * 3, st);
    if (rc == kOk)
        rc = pixel_batch_enqueue(winners_plan, st);
    phases.mark(plan.chunks.size() * 3 + 1, st);
    if (rc != kOk) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    if (!phases.ev.empty() && hipStreamSynchronize(st) == hipSuccess) {
        for (size_t c = 0; c < plan.chunks.size(); ++c) {
            t_phase_ms[0] += phases.between(c * 3, c * 3 + 1);
            t_phase_ms[1] += phases.between(c * 3 + 1, c * 3 + 2);
        }
        t_phase_ms[2] = phases.between(plan.chunks.size() * 3, plan.chunks.size() * 3 + 1);
    }
    for (size_t i = 0; i < count; ++i)
        report(i, picks[i]);
    t_totals.swap(totals);
    t_total_counts.resize(count);
    for (size_t i = 0; i < count; ++i)
        t_total_counts[i] = plan.items[i].len != 0 ? kCandidates : 0;
    return kOk;
}

extern "C" int32_t dxtlt_debug_plan_pixels_batch_auto(const DxtltPixelBatchAutoItem* items, size_t count,
                                                      DxtltDebugPixelBatchAutoPlanItem* items_out,
                                                      DxtltDebugPixelBatchAutoPlanChunk* chunks_out, size_t chunk_capacity, size_t* out_chunks)
{
    if (out_chunks)
        *out_chunks = 0;
    if (count == 0)
        return kOk;
    pb::AutoPlan plan;
    if (pb::Defect d = pb::plan_auto_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    if (items_out == nullptr)
        return fail(kInvalidArgument, "NULL items_out with count > 0");
    for (size_t i = 0; i < count; ++i) {
        const pb::AutoItem& p = plan.items[i];
        DxtltDebugPixelBatchAutoPlanItem& o = items_out[i];
        std::memset(&o, 0, sizeof o);
        o.chunk = p.chunk;
        o.arena_offset = p.slice_off;
        o.arena_bytes = p.slice_bytes;
        for (int k = 0; k < kCandidates; ++k) {
            const bool in_arena = k < kCandidates - 1;
            o.sections[k] = DxtltDebugPixelBatchAutoSection{in_arena ? p.slice_off + (uint64_t)k * p.len : 0, p.len,
                                                            (uint32_t)(p.first_counter + (uint64_t)k), in_arena ? 1u : 0u};
        }
    }
    for (size_t c = 0; c < plan.chunks.size() && chunks_out != nullptr && c < chunk_capacity; ++c) {
        const pb::AutoChunk& ch = plan.chunks[c];
        chunks_out[c] = DxtltDebugPixelBatchAutoPlanChunk{ch.first, ch.count, ch.arena_bytes, ch.candidate_launches(), (uint32_t)ch.estimator_wgs};
    }
    if (out_chunks)
        *out_chunks = plan.chunks.size();
    return kOk;
}

extern "C" void dxtlt_debug_pixels_batch_auto_last(uint64_t out[4])
{
    if (out)
        std::memcpy(out, t_last, sizeof t_last);
}

extern "C" int32_t dxtlt_debug_pixels_batch_auto_last_totals(size_t item, uint64_t* out, int32_t cap)
{
    if (item >= t_total_counts.size())
        return 0;
    const int32_t n = t_total_counts[item];
    for (int32_t i = 0; out != nullptr && i < n && i < cap; ++i)
        out[i] = t_totals[item * kCandidates + (size_t)i];
    return n;
}

extern "C" void dxtlt_debug_pixels_batch_auto_time_phases(int32_t on) { t_time_phases = on != 0; }

extern "C" void dxtlt_debug_pixels_batch_auto_last_phase_ms(double out[3])
{
    if (out)
        std::memcpy(out, t_phase_ms, sizeof t_phase_ms);
}
