// pixel_batch_auto_api.cpp -- dxtlt_transform_pixels_batch_auto_device (include/dxtlt_pixels.h; docs/PIXEL_FORMAT.md, "Many buffers
// in one call"): the best of the six pixel settings for every buffer of a batch, and all of them transformed, with ONE stream wait
// and a launch count that does not grow with the number of buffers.  The pixel twin of batch_auto_api.cpp:
//   plan      (pixel_batch_plan.h) every item gets a 16-byte aligned slice of 5 x len bytes of this thread's candidate arena and
//             six counters; items are cut into chunks whose slices fit the arena cap (a larger item is a chunk by itself)
//   upload    ONE table for the whole call: per chunk the candidate launches' entries and indices and the estimator's sections
//   per chunk one candidate launch per pixel_bytes present (pixel_batch_kernels.hip) and ONE table-driven entropy launch over all
//             six sections of all items (entropy_kernels.hip; the sixth section is the item's d_input); the stream orders the
//             reuse of the arena between chunks (batch_auto_common.h: run_auto_chunks)
//   readback  all counters -- sums of q -- in one copy, ONE wait; rounded up to bytes and compared on the host, in the candidate
//             order of pixel_launch.h with strict `<` from UINT64_MAX
//   winners   the planner and kernels of dxtlt_transform_pixels_batch_device with the chosen per-item settings: enqueued, not waited for
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "../../include/dxtlt_pixels.h"
#include "entropy_launch.h"
#include "auto_call.h"
#include "pixel_batch_api.h"
#include "pixel_batch_launch.h"
#include "pixel_batch_plan.h"

namespace {

using namespace dxtlt_host;
namespace pb = dxtlt_host::pixel_batch;
using dxtlt::pixels::kAutoOrder;
using pb::kCandidates;

// the dxtlt_debug_pixels_batch_auto_* hooks: six totals per item, three phase figures (the third: the winners)
thread_local BatchAutoDebug t_debug(kCandidates);

// the candidate launches of one chunk, one per pixel_bytes present, from the call's table at `dev` (fill_auto_tables)
hipError_t launch_chunk_candidates(const pb::AutoChunk& ch, const uint8_t* dev, hipStream_t st, uint64_t& launched)
{
    for (int b = 0; b < 2; ++b) {
        if (ch.entries[b] == 0)
            continue;
        const uint8_t* d = dev + ch.at[b];
        if (hipError_t e = dxtlt::pixels::launch_pixel_batch_candidates(b == 0 ? 4 : 3, reinterpret_cast<const dxtlt::pixels::PixelBatchEntry*>(d),
                                                                        d + ch.entry_bytes[b], ch.entries[b], ch.wgs[b], ch.wide[b], st);
            e != hipSuccess)
            return e;
        launched++;
    }
    return hipSuccess;
}

}  // namespace

extern "C" int32_t dxtlt_transform_pixels_batch_auto_device(DxtltPixelBatchAutoItem* items, size_t count, void* hip_stream)
{
    t_debug.begin_call();
    t_debug.clear_phase_ms();
    auto_state().begin_call();
    if (count == 0)
        return kOk;
    pb::AutoPlan plan;
    if (Defect d = pb::plan_auto_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    auto report = [&](size_t i, int pick) {
        items[i].decorrelate = kAutoOrder[pick].decorrelate;
        items[i].layout = kAutoOrder[pick].layout;
    };
    if (!plan.any) {   // every estimate of an empty buffer is 0: the first candidate stays; no device needed
        for (size_t i = 0; i < count; ++i)
            report(i, 0);
        return kOk;
    }
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int32_t rc = auto_call_device_check(st))
        return rc;

    uint8_t* arena = static_cast<uint8_t*>(auto_state().arena.get((size_t)plan.arena_bytes));
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    BatchAutoBuffers& buffers = batch_auto_thread_buffers();
    HIP_TRY(buffers.reserve(plan.table_bytes, (size_t)plan.counters), "pixel batch auto tables / counters");
    pb::fill_auto_tables(plan, items, arena, static_cast<uint8_t*>(buffers.table_host));
    const uint8_t* dev = static_cast<const uint8_t*>(buffers.table_dev);

    PhaseEvents phases;   // and two marks around the winners
    if (t_debug.time_phases && !phases.begin(plan.chunks.size(), 2))
        return fail(kDevice, "pixel batch auto: hipEventCreate", hipErrorOutOfMemory);
    auto candidates = [&](size_t c, uint64_t& launched) { return launch_chunk_candidates(plan.chunks[c], dev, st, launched); };
    auto estimator = [&](size_t c, uint64_t& launched) {
        const pb::AutoChunk& ch = plan.chunks[c];
        if (ch.estimator_entries == 0)
            return hipSuccess;
        const hipError_t e = dxtlt::launch_entropy_table(reinterpret_cast<const dxtlt::EstimateTableEntry*>(dev + ch.sections_at),
                                                         ch.estimator_entries, (uint32_t)ch.estimator_wgs, buffers.counters_dev, st);
        launched += e == hipSuccess;
        return e;
    };
    if (int32_t rc = run_auto_chunks("pixel batch auto", buffers, plan.table_bytes, plan.counters, plan.chunks.size(), st, phases, t_debug,
                                     candidates, estimator))
        return rc;

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
            picks[i] = dxtlt::pixels::auto_pick_of(&totals[i * kCandidates]);
        }
        DxtltPixelBatchItem& w = winners[i];
        std::memset(&w, 0, sizeof w);
        w.d_input = items[i].d_input;
        w.d_output = items[i].d_output;
        w.len = items[i].len;
        w.pixel_bytes = items[i].pixel_bytes;
        w.decorrelate = kAutoOrder[picks[i]].decorrelate;
        w.layout = kAutoOrder[picks[i]].layout;
    }
    pb::Plan winners_plan;
    int32_t rc = kOk;
    if (Defect d = pb::plan_call(winners.data(), count, winners_plan); d.code != kOk)
        rc = fail(d.code, d.what);   // (not reached: the batch passed the same checks and the per-pixel_bytes limit above)
    const size_t around = plan.chunks.size() * 3;
    phases.mark(around, st);
    if (rc == kOk)
        rc = pixel_batch_enqueue(winners_plan, st);
    phases.mark(around + 1, st);
    if (rc != kOk) {
        (void)hipStreamSynchronize(st);
        t_debug.clear_phase_ms();
        return rc;
    }
    if (phases.on() && hipStreamSynchronize(st) == hipSuccess)
        t_debug.phase_ms[2] = phases.between(around, around + 1);
    for (size_t i = 0; i < count; ++i)
        report(i, picks[i]);
    t_debug.totals.swap(totals);
    t_debug.total_counts.resize(count);
    for (size_t i = 0; i < count; ++i)
        t_debug.total_counts[i] = plan.items[i].len != 0 ? kCandidates : 0;
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
    if (Defect d = pb::plan_auto_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
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

extern "C" int32_t dxtlt_debug_pixels_batch_candidates_device(const DxtltPixelBatchAutoItem* items, size_t count, size_t chunk, void* d_arena,
                                                              uint64_t arena_bytes, void* hip_stream)
{
    pb::AutoPlan plan;
    if (Defect d = pb::plan_auto_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    if (chunk >= plan.chunks.size())
        return fail(kInvalidArgument, "pixel batch candidates: no such chunk");
    const pb::AutoChunk& ch = plan.chunks[chunk];
    if (d_arena == nullptr || arena_bytes < ch.arena_bytes)
        return fail(kInvalidArgument, "pixel batch candidates: an arena smaller than the chunk's arena_bytes");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int32_t rc = auto_call_device_check(st))
        return rc;
    if (ch.candidate_launches() == 0)
        return kOk;
    BatchAutoBuffers& buffers = batch_auto_thread_buffers();
    HIP_TRY(buffers.reserve(plan.table_bytes, 0), "pixel batch candidates: tables");
    pb::fill_auto_tables(plan, items, static_cast<uint8_t*>(d_arena), static_cast<uint8_t*>(buffers.table_host));
    // every exit below drains the stream: the tables belong to this thread's next call
    hipError_t e = dxtlt::launch_table_upload(buffers.table_mapped, buffers.table_dev, (plan.table_bytes + 15) & ~size_t(15), st);
    const char* step = "pixel batch candidates: table upload";
    if (e == hipSuccess) {
        uint64_t launched = 0;
        e = launch_chunk_candidates(plan.chunks[chunk], static_cast<const uint8_t*>(buffers.table_dev), st, launched);
        step = "pixel batch candidates: candidate kernel launch";
    }
    const hipError_t waited = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return fail(kDevice, step, e);
    if (waited != hipSuccess)
        return fail(kDevice, "stream synchronize", waited);
    return kOk;
}

extern "C" void dxtlt_debug_pixels_batch_auto_last(uint64_t out[4]) { t_debug.copy_last(out); }

extern "C" int32_t dxtlt_debug_pixels_batch_auto_last_totals(size_t item, uint64_t* out, int32_t cap)
{
    return t_debug.copy_totals(item, out, cap);
}

extern "C" void dxtlt_debug_pixels_batch_auto_time_phases(int32_t on) { t_debug.time_phases = on != 0; }

extern "C" void dxtlt_debug_pixels_batch_auto_last_phase_ms(double out[3]) { t_debug.copy_phase_ms(out, 3); }
