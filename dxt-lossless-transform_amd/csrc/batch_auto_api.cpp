// batch_auto_api.cpp -- dxtlt_transform_batch_auto_device (include/dxtlt_estimator.h): the best settings for every buffer of a
// batch, and all of them transformed, with ONE stream wait and a launch count that does not grow with the number of buffers.
//
// A loop of dxtlt_transform_bcN_auto_device waits for the stream once per buffer and launches a candidate kernel, an estimator and
// a transform over each buffer alone -- textures of a few MiB that cannot fill the chip.  Here:
//   plan      every item gets a 16-byte aligned slice of this thread's candidate arena and up to 10 counters; items are cut into
//             chunks whose slices fit the arena cap (an item larger than the cap is a chunk by itself)
//   upload    ONE table for the whole call: per chunk the candidate launches' entry tables and the estimator's section table
//   per chunk one candidate launch per (format, use_all) present (batch_auto_kernels.hip) and one table-driven estimator launch
//             (estimate_kernels.hip); the stream orders the reuse of the arena between chunks
//   readback  all counters of the batch in one copy, ONE wait; the pick per item on the host (auto_pick: candidates_of's order, strict `<`)
//   winners   dxtlt_transform_batch_device with the chosen per-item settings: enqueued, not waited for
#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_estimator.h"
#include "../../include/dxtlt_gfx950.h"
#include "auto_launch.h"
#include "batch_auto_buffers.h"
#include "bcn_launch.h"
#include "estimate_launch.h"
#include "host_common.h"

namespace {

using namespace dxtlt_host;

constexpr int kMaxSections = 10;   // counters per item: BC3 with every mode, 2 alpha + 8 colour sections

thread_local uint64_t t_arena_cap = 0;        // dxtlt_debug_batch_auto_arena_cap; 0 = DXTLT_BATCH_AUTO_ARENA_CAP
thread_local uint64_t t_last[4] = {0, 0, 0, 0};   // dxtlt_debug_batch_auto_last
thread_local std::vector<uint64_t> t_totals;  // dxtlt_debug_batch_auto_last_totals: 16 per item
thread_local std::vector<uint8_t> t_total_counts;
thread_local bool t_time_phases = false;      // dxtlt_debug_batch_auto_time_phases
thread_local double t_phase_ms[2] = {0, 0};   // candidate launches, estimator launches of the last timed call

inline uint32_t block_bytes_of(uint8_t format) { return format == 1 || format == 4 ? 8u : 16u; }
inline bool use_all_of(const DxtltBatchAutoItem& it) { return it.use_all_decorrelation_modes != 0 && it.format <= 3; }

struct PlannedItem {
    uint32_t chunk = 0;
    int sections = 0;
    uint64_t blocks = 0;
    uint64_t slice_off = 0, slice_bytes = 0;   // inside the arena
    uint64_t sec_off[kMaxSections], sec_len[kMaxSections];   // sec_off: from the slice's first byte
    uint64_t first_counter = 0;
};

struct PlannedChunk {
    size_t first = 0, count = 0;
    uint64_t arena_bytes = 0;
    uint32_t groups = 0;          // bit (format - 1) * 2 + use_all: a candidate launch
    uint64_t estimator_wgs = 0;
    uint32_t estimator_entries = 0;
};

struct Plan {
    std::vector<PlannedItem> items;
    std::vector<PlannedChunk> chunks;
    uint64_t counters = 0;
    uint64_t arena_bytes = 0;   // the largest chunk
};

int32_t validate(const DxtltBatchAutoItem* items, size_t count)
{
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    struct Span {
        uintptr_t begin, end;
        bool output;
    };
    std::vector<Span> spans;
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchAutoItem& it = items[i];
        if (it.format < 1 || it.format > 5)
            return fail(kInvalidArgument, "batch auto item: format must be 1..5 (BC1..BC5)");
        if (it.len % block_bytes_of(it.format) != 0)
            return fail(kInvalidLength, "batch auto item: len is not a multiple of the block size");
        if (it.len > 0 && (it.d_input == nullptr || it.d_output == nullptr))
            return fail(kInvalidArgument, "batch auto item: NULL device buffer with len > 0");
        if (it.len >= (uint64_t(64) << 30))
            return fail(kInvalidArgument, "batch auto item of 64 GiB or more: use the single-buffer entry point");
        if (it.len > 0) {
            const uintptr_t in = reinterpret_cast<uintptr_t>(it.d_input), out = reinterpret_cast<uintptr_t>(it.d_output);
            spans.push_back({in, in + (uintptr_t)it.len, false});
            spans.push_back({out, out + (uintptr_t)it.len, true});
        }
    }
    // the winners go out through dxtlt_transform_batch_device, one launch per (format, settings) of fewer than 2^24 workgroups: a
    // whole tile per 256 blocks and at most two edge tiles per item.  Which settings win is not known yet, so a format's items are
    // held to the limit together -- refused here, not after the choices have been written.
    uint64_t winner_wgs[5] = {0, 0, 0, 0, 0};
    for (size_t i = 0; i < count; ++i)
        if (items[i].len > 0)
            winner_wgs[items[i].format - 1] += items[i].len / block_bytes_of(items[i].format) / 256 + 2;
    for (uint64_t w : winner_wgs)
        if (w > 0xFFFFFFull)
            return fail(kInvalidArgument, "batch auto: too large for one launch (about 32 GiB of BC1 / BC4 or 64 GiB of BC2 / BC3 / BC5 items)");
    // an output may overlap nothing: in order of their first bytes, a span overlaps an earlier one when it begins before that one ends
    std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
    uintptr_t end_any = 0, end_output = 0;
    for (const Span& s : spans) {
        if (s.begin < (s.output ? end_any : end_output))
            return fail(kInvalidArgument, "batch auto item: a d_output overlaps another buffer of the batch");
        end_any = std::max(end_any, s.end);
        if (s.output)
            end_output = std::max(end_output, s.end);
    }
    return kOk;
}

// arena slices, counters and chunks; the items are valid
void make_plan(const DxtltBatchAutoItem* items, size_t count, Plan& plan)
{
    const uint64_t cap = batch_auto_arena_cap();
    plan.items.assign(count, PlannedItem{});
    PlannedChunk cur;
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchAutoItem& it = items[i];
        PlannedItem& p = plan.items[i];
        const dxtlt::Format fmt = (dxtlt::Format)it.format;
        const bool all = use_all_of(it);
        p.blocks = it.len / block_bytes_of(it.format);
        const dxtlt::AutoSections secs = dxtlt::auto_sections(fmt, all, p.blocks);
        p.slice_bytes = secs.bytes;
        p.sections = secs.count;
        std::copy(secs.off, secs.off + secs.count, p.sec_off);
        std::copy(secs.len, secs.len + secs.count, p.sec_len);
        const uint64_t padded = (p.slice_bytes + 15) & ~uint64_t(15);
        // a chunk is closed BEFORE the item that would push it past the cap: it holds at most the cap, or one larger item
        if (cur.count > 0 && cur.arena_bytes + padded > cap) {
            plan.chunks.push_back(cur);
            cur = PlannedChunk{};
            cur.first = i;
        }
        p.chunk = (uint32_t)plan.chunks.size();
        p.slice_off = cur.arena_bytes;
        p.first_counter = plan.counters;
        plan.counters += (uint64_t)p.sections;
        cur.arena_bytes += padded;
        cur.count++;
        if (p.blocks != 0) {
            cur.groups |= 1u << ((it.format - 1) * 2 + (all ? 1 : 0));
            for (int k = 0; k < p.sections; ++k)
                cur.estimator_wgs += (p.sec_len[k] + dxtlt::kEstimatorWindow - 1) / dxtlt::kEstimatorWindow;
            cur.estimator_entries += (uint32_t)p.sections;
        }
    }
    plan.chunks.push_back(cur);
    for (const PlannedChunk& c : plan.chunks)
        plan.arena_bytes = std::max(plan.arena_bytes, c.arena_bytes);
}

// this thread's table staging and counters (batch_auto_buffers.h), shared with the batched pixel auto call
thread_local BatchAutoBuffers g_buffers;

}  // namespace

void dxtlt_host::release_batch_auto_thread_buffers() { g_buffers.release(); }

dxtlt_host::BatchAutoBuffers& dxtlt_host::batch_auto_thread_buffers() { return g_buffers; }

uint64_t dxtlt_host::batch_auto_arena_cap() { return t_arena_cap ? t_arena_cap : DXTLT_BATCH_AUTO_ARENA_CAP; }

extern "C" int32_t dxtlt_transform_batch_auto_device(DxtltBatchAutoItem* items, size_t count, void* hip_stream)
{
    std::memset(t_last, 0, sizeof t_last);
    t_totals.clear();
    t_total_counts.clear();
    auto_begin_device_call();
    if (count == 0)
        return kOk;
    if (int32_t rc = validate(items, count))
        return rc;
    bool any = false;
    for (size_t i = 0; i < count && !any; ++i)
        any = items[i].len != 0;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (any) {
        int devices = 0;
        hipError_t e = hipGetDeviceCount(&devices);
        if (e != hipSuccess || devices <= 0)
            return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
        if (stream_is_capturing(st))
            return fail(kInvalidArgument, "the auto transforms read their estimates back and wait for the stream: not capturable");
    }

    Plan plan;
    make_plan(items, count, plan);
    std::vector<AutoChoice> orders(count * 16);
    std::vector<uint8_t> order_counts(count);
    for (size_t i = 0; i < count; ++i)
        order_counts[i] = (uint8_t)auto_candidate_order(items[i].format, use_all_of(items[i]), &orders[i * 16]);
    auto report = [&](size_t i, int pick) {
        const AutoChoice& c = orders[i * 16 + (size_t)pick];
        items[i].decorrelation_mode = c.mode;
        items[i].split_alpha_endpoints = c.split_alpha ? 1 : 0;
        items[i].split_colour_endpoints = c.split_colour ? 1 : 0;
    };
    if (!any) {   // every estimate of an empty buffer is 0: the first candidate stays
        for (size_t i = 0; i < count; ++i)
            report(i, 0);
        return kOk;
    }

    // the table of the whole call: per chunk, per candidate launch its entries, then the estimator's sections
    struct Launch {
        int format;
        bool all;
        size_t at;   // bytes into the table
        uint32_t entries, wgs;
    };
    struct ChunkTables {
        std::vector<Launch> launches;
        size_t sections_at = 0;
    };
    std::vector<ChunkTables> tables(plan.chunks.size());
    size_t table_bytes = 0;
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const PlannedChunk& ch = plan.chunks[c];
        if (ch.estimator_wgs > 0x7FFFFFFFull)
            return fail(kInvalidArgument, "batch auto: a chunk of more than 2^31 - 1 estimator windows");
        for (int g = 0; g < 10; ++g) {
            if (!(ch.groups & (1u << g)))
                continue;
            Launch l{g / 2 + 1, (g & 1) != 0, table_bytes, 0, 0};
            for (size_t i = ch.first; i < ch.first + ch.count; ++i)
                if (plan.items[i].blocks != 0 && items[i].format == l.format && use_all_of(items[i]) == l.all)
                    l.entries++;
            table_bytes += (size_t)l.entries * sizeof(dxtlt::BatchAutoEntry);
            tables[c].launches.push_back(l);
        }
        tables[c].sections_at = table_bytes;
        table_bytes += ((size_t)ch.estimator_entries * sizeof(dxtlt::EstimateTableEntry) + 15) & ~size_t(15);
    }
    if (table_bytes > (size_t(1) << 31))
        return fail(kInvalidArgument, "batch auto: too many items for one call (a table of more than 2 GiB)");

    uint8_t* arena = static_cast<uint8_t*>(auto_thread_arena((size_t)plan.arena_bytes));
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    HIP_TRY(g_buffers.reserve(table_bytes, (size_t)plan.counters), "batch auto tables / counters");
    uint8_t* host = static_cast<uint8_t*>(g_buffers.table_host);
    const uint8_t* dev = static_cast<const uint8_t*>(g_buffers.table_dev);
    for (size_t c = 0; c < plan.chunks.size(); ++c) {
        const PlannedChunk& ch = plan.chunks[c];
        for (Launch& l : tables[c].launches) {
            dxtlt::BatchAutoEntry* e = reinterpret_cast<dxtlt::BatchAutoEntry*>(host + l.at);
            for (size_t i = ch.first; i < ch.first + ch.count; ++i) {
                const PlannedItem& p = plan.items[i];
                if (p.blocks == 0 || items[i].format != l.format || use_all_of(items[i]) != l.all)
                    continue;
                *e++ = dxtlt::BatchAutoEntry{static_cast<const uint8_t*>(items[i].d_input), p.slice_off, p.blocks, l.wgs, 0};
                l.wgs += dxtlt::batch_auto_workgroups((dxtlt::Format)l.format, p.blocks);
            }
        }
        dxtlt::EstimateTableEntry* s = reinterpret_cast<dxtlt::EstimateTableEntry*>(host + tables[c].sections_at);
        uint32_t wgs = 0;
        for (size_t i = ch.first; i < ch.first + ch.count; ++i) {
            const PlannedItem& p = plan.items[i];
            for (int k = 0; k < p.sections && p.blocks != 0; ++k) {
                wgs += (uint32_t)((p.sec_len[k] + dxtlt::kEstimatorWindow - 1) / dxtlt::kEstimatorWindow);
                *s++ = dxtlt::EstimateTableEntry{arena + p.slice_off + p.sec_off[k], p.sec_len[k], wgs, (uint32_t)(p.first_counter + (uint64_t)k)};
            }
        }
    }

    // dxtlt_debug_batch_auto_time_phases: three events per chunk -- in front of its candidate launches, between them and its
    // estimator launch, behind it -- read after the call's one wait
    std::vector<hipEvent_t> events;
    if (t_time_phases) {
        events.assign(plan.chunks.size() * 3, nullptr);
        for (hipEvent_t& ev : events)
            if (hipEventCreate(&ev) != hipSuccess) {
                for (hipEvent_t made : events)
                    if (made) (void)hipEventDestroy(made);
                return fail(kDevice, "batch auto: hipEventCreate", hipErrorOutOfMemory);
            }
    }
    auto mark = [&](size_t c, int k) { return events.empty() ? hipSuccess : hipEventRecord(events[c * 3 + (size_t)k], st); };
    t_phase_ms[0] = t_phase_ms[1] = 0;

    // every failure exit below drains the stream: the arena, the tables and the counters belong to this thread's next call
    hipError_t e = hipMemsetAsync(g_buffers.counters_dev, 0, (size_t)plan.counters * sizeof(uint64_t), st);
    const char* what = "batch auto: counter clear";
    if (e == hipSuccess) {
        e = dxtlt::launch_table_upload(g_buffers.table_mapped, g_buffers.table_dev, (table_bytes + 15) & ~size_t(15), st);
        what = "batch auto: table upload";
    }
    for (size_t c = 0; c < plan.chunks.size() && e == hipSuccess; ++c) {
        const PlannedChunk& ch = plan.chunks[c];
        (void)mark(c, 0);
        for (const Launch& l : tables[c].launches) {
            e = dxtlt::launch_batch_auto_candidates((dxtlt::Format)l.format, l.all, reinterpret_cast<const dxtlt::BatchAutoEntry*>(dev + l.at),
                                                    l.entries, l.wgs, arena, st);
            what = "batch auto: candidate kernel launch";
            if (e != hipSuccess)
                break;
            t_last[2]++;
        }
        (void)mark(c, 1);
        if (e == hipSuccess && ch.estimator_entries != 0) {
            e = dxtlt::launch_estimate_table(reinterpret_cast<const dxtlt::EstimateTableEntry*>(dev + tables[c].sections_at),
                                             ch.estimator_entries, (uint32_t)ch.estimator_wgs, g_buffers.counters_dev, st);
            what = "batch auto: estimator launch";
            if (e == hipSuccess)
                t_last[3]++;
        }
        (void)mark(c, 2);
        t_last[1]++;
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(g_buffers.counters_host, g_buffers.counters_dev, (size_t)plan.counters * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        what = "batch auto: D2H estimates";
    }
    const hipError_t waited = hipStreamSynchronize(st);   // the one wait of the call
    t_last[0]++;
    for (size_t c = 0; c * 3 < events.size(); ++c) {
        float ms = 0;
        if (e == hipSuccess && waited == hipSuccess && hipEventElapsedTime(&ms, events[c * 3], events[c * 3 + 1]) == hipSuccess)
            t_phase_ms[0] += ms;
        if (e == hipSuccess && waited == hipSuccess && hipEventElapsedTime(&ms, events[c * 3 + 1], events[c * 3 + 2]) == hipSuccess)
            t_phase_ms[1] += ms;
        for (int k = 0; k < 3; ++k)
            (void)hipEventDestroy(events[c * 3 + (size_t)k]);
    }
    if (e != hipSuccess)
        return fail(kDevice, what, e);
    if (waited != hipSuccess)
        return fail(kDevice, "stream synchronize", waited);

    std::vector<DxtltBatchItem> winners(count);
    std::vector<uint64_t> totals(count * 16, 0);
    for (size_t i = 0; i < count; ++i) {
        const PlannedItem& p = plan.items[i];
        int pick = 0;
        if (p.blocks != 0)
            pick = auto_pick(items[i].format, use_all_of(items[i]), false, g_buffers.counters_host + p.first_counter, &totals[i * 16]);
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
    t_totals.swap(totals);
    t_total_counts.resize(count);
    for (size_t i = 0; i < count; ++i)
        t_total_counts[i] = plan.items[i].blocks != 0 ? order_counts[i] : 0;
    return kOk;
}

extern "C" int32_t dxtlt_debug_plan_batch_auto(const DxtltBatchAutoItem* items, size_t count, DxtltDebugBatchAutoPlanItem* items_out,
                                               DxtltDebugBatchAutoPlanChunk* chunks_out, size_t chunk_capacity, size_t* out_chunks)
{
    if (out_chunks)
        *out_chunks = 0;
    if (count == 0)
        return kOk;
    if (int32_t rc = validate(items, count))
        return rc;
    if (items_out == nullptr)
        return fail(kInvalidArgument, "NULL items_out with count > 0");
    Plan plan;
    make_plan(items, count, plan);
    for (size_t i = 0; i < count; ++i) {
        const PlannedItem& p = plan.items[i];
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
        const PlannedChunk& ch = plan.chunks[c];
        uint32_t launches = 0;
        for (uint32_t g = ch.groups; g != 0; g &= g - 1)
            ++launches;
        chunks_out[c] = DxtltDebugBatchAutoPlanChunk{ch.first, ch.count, ch.arena_bytes, launches, (uint32_t)ch.estimator_wgs};
    }
    if (out_chunks)
        *out_chunks = plan.chunks.size();
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

extern "C" void dxtlt_debug_batch_auto_last(uint64_t out[4])
{
    if (out)
        std::memcpy(out, t_last, sizeof t_last);
}

extern "C" int32_t dxtlt_debug_batch_auto_last_totals(size_t item, uint64_t* out, int32_t cap)
{
    if (item >= t_total_counts.size())
        return 0;
    const int32_t n = t_total_counts[item];
    for (int32_t i = 0; out != nullptr && i < n && i < cap; ++i)
        out[i] = t_totals[item * 16 + (size_t)i];
    return n;
}

extern "C" void dxtlt_debug_batch_auto_arena_cap(uint64_t bytes) { t_arena_cap = bytes; }

extern "C" void dxtlt_debug_batch_auto_time_phases(int32_t on) { t_time_phases = on != 0; }

extern "C" void dxtlt_debug_batch_auto_last_phase_ms(double out[2])
{
    if (out)
        std::memcpy(out, t_phase_ms, sizeof t_phase_ms);
}
