// batch_auto_api.cpp -- dxtlt_transform_batch_auto_device (include/dxtlt_estimator.h): the best settings for every buffer of a
// batch, and all of them transformed, with ONE stream wait and a launch count that does not grow with the number of buffers.
//
// A loop of dxtlt_transform_bcN_auto_device waits for the stream once per buffer and launches a candidate kernel, an estimator and
// a transform over each buffer alone -- textures of a few MiB that cannot fill the chip.  Here:
//   plan      (batch_auto_plan.h) every item gets a 16-byte aligned slice of this thread's candidate arena and up to 10 counters;
//             items are cut into chunks whose slices fit the arena cap (an item larger than the cap is a chunk by itself)
//   upload    ONE table for the whole call: per chunk the candidate launches' entry tables and the estimator's section table
//   per chunk one candidate launch per (format, use_all) present (batch_auto_kernels.hip) and one table-driven estimator launch
//             (estimate_kernels.hip); the stream orders the reuse of the arena between chunks (batch_auto_common.h: run_auto_chunks)
//   readback  all counters of the batch in one copy, ONE wait; the pick per item on the host (auto_pick: candidates_of's order, strict `<`)
//   winners   dxtlt_transform_batch_device with the chosen per-item settings: enqueued, not waited for
#include <cstring>
#include <vector>

#include "../../include/dxtlt_estimator.h"
#include "../../include/dxtlt_gfx950.h"
#include "batch_auto_plan.h"
#include "estimate_launch.h"
#include "auto_call.h"

namespace {

using namespace dxtlt_host;
namespace ba = dxtlt_host::batch_auto;

thread_local uint64_t t_arena_cap = 0;        // dxtlt_debug_batch_auto_arena_cap; 0 = DXTLT_BATCH_AUTO_ARENA_CAP
thread_local BatchAutoDebug t_debug(16);      // the dxtlt_debug_batch_auto_* hooks: 16 totals per item, two phase figures

// this thread's table staging and counters (batch_auto_common.h), shared with the batched pixel auto call
thread_local BatchAutoBuffers g_buffers;

// the candidate launches of one chunk, one per (format, use_all) present, from the call's table at `dev` (fill_tables) into `arena`
hipError_t launch_chunk_candidates(const ba::PlannedChunk& ch, const uint8_t* dev, uint8_t* arena, hipStream_t st, uint64_t& launched)
{
    for (int g = 0; g < ba::kGroups; ++g) {
        if (ch.entries[g] == 0)
            continue;
        if (hipError_t e = dxtlt::launch_batch_auto_candidates((dxtlt::Format)(g / 2 + 1), (g & 1) != 0,
                                                               reinterpret_cast<const dxtlt::BatchAutoEntry*>(dev + ch.at[g]),
                                                               ch.entries[g], ch.wgs[g], arena, st);
            e != hipSuccess)
            return e;
        launched++;
    }
    return hipSuccess;
}

}  // namespace

void dxtlt_host::release_batch_auto_thread_buffers() { g_buffers.release(); }

dxtlt_host::BatchAutoBuffers& dxtlt_host::batch_auto_thread_buffers() { return g_buffers; }

uint64_t dxtlt_host::batch_auto_arena_cap() { return t_arena_cap ? t_arena_cap : DXTLT_BATCH_AUTO_ARENA_CAP; }

extern "C" int32_t dxtlt_transform_batch_auto_device(DxtltBatchAutoItem* items, size_t count, void* hip_stream)
{
    t_debug.begin_call();
    auto_state().begin_call();
    if (count == 0)
        return kOk;
    ba::Plan plan;
    if (Defect d = ba::plan_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (plan.any)
        if (int32_t rc = auto_call_device_check(st))
            return rc;

    std::vector<AutoChoice> orders(count * 16);
    std::vector<uint8_t> order_counts(count);
    for (size_t i = 0; i < count; ++i)
        order_counts[i] = (uint8_t)auto_candidate_order(items[i].format, ba::use_all_of(items[i]), &orders[i * 16]);
    auto report = [&](size_t i, int pick) {
        const AutoChoice& c = orders[i * 16 + (size_t)pick];
        items[i].decorrelation_mode = c.mode;
        items[i].split_alpha_endpoints = c.split_alpha ? 1 : 0;
        items[i].split_colour_endpoints = c.split_colour ? 1 : 0;
    };
    if (!plan.any) {   // every estimate of an empty buffer is 0: the first candidate stays
        for (size_t i = 0; i < count; ++i)
            report(i, 0);
        return kOk;
    }

    uint8_t* arena = static_cast<uint8_t*>(auto_state().arena.get((size_t)plan.arena_bytes));
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    HIP_TRY(g_buffers.reserve(plan.table_bytes, (size_t)plan.counters), "batch auto tables / counters");
    ba::fill_tables(plan, items, arena, static_cast<uint8_t*>(g_buffers.table_host));
    const uint8_t* dev = static_cast<const uint8_t*>(g_buffers.table_dev);

    PhaseEvents phases;
    if (t_debug.time_phases && !phases.begin(plan.chunks.size(), 0))
        return fail(kDevice, "batch auto: hipEventCreate", hipErrorOutOfMemory);
    auto candidates = [&](size_t c, uint64_t& launched) { return launch_chunk_candidates(plan.chunks[c], dev, arena, st, launched); };
    auto estimator = [&](size_t c, uint64_t& launched) {
        const ba::PlannedChunk& ch = plan.chunks[c];
        if (ch.estimator_entries == 0)
            return hipSuccess;
        const hipError_t e = dxtlt::launch_estimate_table(reinterpret_cast<const dxtlt::EstimateTableEntry*>(dev + ch.sections_at),
                                                          ch.estimator_entries, (uint32_t)ch.estimator_wgs, g_buffers.counters_dev, st);
        launched += e == hipSuccess;
        return e;
    };
    if (int32_t rc = run_auto_chunks("batch auto", g_buffers, plan.table_bytes, plan.counters, plan.chunks.size(), st, phases, t_debug,
                                     candidates, estimator))
        return rc;

    std::vector<DxtltBatchItem> winners(count);
    std::vector<uint64_t> totals(count * 16, 0);
    for (size_t i = 0; i < count; ++i) {
        const ba::PlannedItem& p = plan.items[i];
        int pick = 0;
        if (p.blocks != 0)
            pick = auto_pick(items[i].format, ba::use_all_of(items[i]), false, g_buffers.counters_host + p.first_counter, &totals[i * 16]);
        report(i, pick);
        DxtltBatchItem& w = winners[i];
        std::memset(&w, 0, sizeof w);
        w.d_input = items[i].d_input;
        w.d_output = items[i].d_output;
        w.len = items[i].len;
        w.format = items[i].format;
        w.decorrelation_mode = items[i].decorrelation_mode;
        w.split_alpha_endpoints = items[i].split_alpha_endpoints;
        w.split_colour_endpoints = items[i].split_colour_endpoints;
    }
    if (int32_t rc = dxtlt_transform_batch_device(winners.data(), count, hip_stream)) {
        (void)hipStreamSynchronize(st);
        return rc;
    }
    t_debug.totals.swap(totals);
    t_debug.total_counts.resize(count);
    for (size_t i = 0; i < count; ++i)
        t_debug.total_counts[i] = plan.items[i].blocks != 0 ? order_counts[i] : 0;
    return kOk;
}

extern "C" int32_t dxtlt_debug_plan_batch_auto(const DxtltBatchAutoItem* items, size_t count, DxtltDebugBatchAutoPlanItem* items_out,
                                               DxtltDebugBatchAutoPlanChunk* chunks_out, size_t chunk_capacity, size_t* out_chunks)
{
    if (out_chunks)
        *out_chunks = 0;
    if (count == 0)
        return kOk;
    ba::Plan plan;
    if (Defect d = ba::plan_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    if (items_out == nullptr)
        return fail(kInvalidArgument, "NULL items_out with count > 0");
    for (size_t i = 0; i < count; ++i) {
        const ba::PlannedItem& p = plan.items[i];
        DxtltDebugBatchAutoPlanItem& o = items_out[i];
        std::memset(&o, 0, sizeof o);
        o.chunk = p.chunk;
        o.section_count = (uint32_t)p.sections;
        o.arena_offset = p.slice_off;
        o.arena_bytes = p.slice_bytes;
        for (int k = 0; k < p.sections; ++k)
            o.sections[k] = DxtltDebugBatchAutoSection{p.slice_off + p.sec_off[k], p.sec_len[k], (uint32_t)(p.first_counter + (uint64_t)k), 0};
    }
    for (size_t c = 0; c < plan.chunks.size() && chunks_out != nullptr && c < chunk_capacity; ++c) {
        const ba::PlannedChunk& ch = plan.chunks[c];
        chunks_out[c] = DxtltDebugBatchAutoPlanChunk{ch.first, ch.count, ch.arena_bytes, ch.candidate_launches(), (uint32_t)ch.estimator_wgs};
    }
    if (out_chunks)
        *out_chunks = plan.chunks.size();
    return kOk;
}

extern "C" int32_t dxtlt_debug_batch_auto_candidates_device(const DxtltBatchAutoItem* items, size_t count, size_t chunk, void* d_arena,
                                                            uint64_t arena_bytes, void* hip_stream)
{
    ba::Plan plan;
    if (Defect d = ba::plan_call(items, count, batch_auto_arena_cap(), plan); d.code != kOk)
        return fail(d.code, d.what);
    if (chunk >= plan.chunks.size())
        return fail(kInvalidArgument, "batch auto candidates: no such chunk");
    const ba::PlannedChunk& ch = plan.chunks[chunk];
    if (d_arena == nullptr || (reinterpret_cast<uintptr_t>(d_arena) & 15) != 0 || arena_bytes < ch.arena_bytes)
        return fail(kInvalidArgument, "batch auto candidates: an arena off a 16-byte boundary or smaller than the chunk's arena_bytes");
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (int32_t rc = auto_call_device_check(st))
        return rc;
    if (ch.candidate_launches() == 0)
        return kOk;
    HIP_TRY(g_buffers.reserve(plan.table_bytes, 0), "batch auto candidates: tables");
    ba::fill_tables(plan, items, static_cast<uint8_t*>(d_arena), static_cast<uint8_t*>(g_buffers.table_host));
    // every exit below drains the stream: the tables belong to this thread's next call
    hipError_t e = dxtlt::launch_table_upload(g_buffers.table_mapped, g_buffers.table_dev, (plan.table_bytes + 15) & ~size_t(15), st);
    const char* step = "batch auto candidates: table upload";
    if (e == hipSuccess) {
        uint64_t launched = 0;
        e = launch_chunk_candidates(ch, static_cast<const uint8_t*>(g_buffers.table_dev), static_cast<uint8_t*>(d_arena), st, launched);
        step = "batch auto candidates: candidate kernel launch";
    }
    const hipError_t waited = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return fail(kDevice, step, e);
    if (waited != hipSuccess)
        return fail(kDevice, "stream synchronize", waited);
    return kOk;
}

extern "C" int32_t dxtlt_debug_auto_pick(int32_t route, int32_t format, bool use_all, const uint64_t* section_sizes, int32_t n_sizes,
                                         uint64_t* totals_out, int32_t cap, uint8_t* mode, bool* split_alpha, bool* split_colour)
{
    if (format < 1 || format > 5 || route < 0 || route > 2 || section_sizes == nullptr)
        return fail(kInvalidArgument, "auto pick: route 0..2, format 1..5, section sizes");
    use_all = use_all && format <= 3;
    AutoChoice order[16];
    const int n = auto_candidate_order(format, use_all, order);
    const bool per_candidate = route == 2 || (route == 0 && format >= 4);
    const int want = per_candidate ? 2 * n : dxtlt::auto_sections((dxtlt::Format)format, use_all, 0).count;
    if (n_sizes != want)
        return fail(kInvalidArgument, "auto pick: another number of section sizes than the route reads back");
    uint64_t total[16];
    const int pick = auto_pick(format, use_all, per_candidate, section_sizes, total);
    for (int i = 0; totals_out != nullptr && i < n && i < cap; ++i)
        totals_out[i] = total[i];
    if (mode) *mode = order[pick].mode;
    if (split_alpha) *split_alpha = order[pick].split_alpha;
    if (split_colour) *split_colour = order[pick].split_colour;
    return kOk;
}

extern "C" void dxtlt_debug_batch_auto_last(uint64_t out[4]) { t_debug.copy_last(out); }

extern "C" int32_t dxtlt_debug_batch_auto_last_totals(size_t item, uint64_t* out, int32_t cap) { return t_debug.copy_totals(item, out, cap); }

extern "C" void dxtlt_debug_batch_auto_arena_cap(uint64_t bytes) { t_arena_cap = bytes; }

extern "C" void dxtlt_debug_batch_auto_time_phases(int32_t on) { t_debug.time_phases = on != 0; }

extern "C" void dxtlt_debug_batch_auto_last_phase_ms(double out[2]) { t_debug.copy_phase_ms(out, 2); }
