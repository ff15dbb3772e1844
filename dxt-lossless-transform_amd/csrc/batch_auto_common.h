// batch_auto_common.h -- what the two batched auto calls (batch_auto_api.cpp: dxtlt_transform_batch_auto_device, BC1 - BC5;
// pixel_batch_auto_api.cpp: dxtlt_transform_pixels_batch_auto_device) are made of, written once.  Pure host arithmetic for their
// planners (batch_auto_plan.h, pixel_batch_plan.h; it also runs stand-alone under the host sanitizers, tests/cpp/*_plan_main.cpp):
// the overlap rule, the chunk packer and the estimator's section table.  And the call itself: this thread's table staging and
// counters, the bench hooks' events and figures, and the stream driver.  Host only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "bcn_launch.h"
#include "estimate_launch.h"
#include "host_common.h"
#include "host_pipeline.h"

namespace dxtlt_host {

// why a batch is refused: the status and the text for dxtlt_last_error() (code kOk: not refused)
struct Defect {
    int32_t code = kOk;
    const char* what = nullptr;
};

// The rule that a d_output overlaps no other output and no input of its batch (inputs may overlap one another), over the
// non-empty items: in order of their first bytes, a span overlaps an earlier one when it begins before that one ends.
struct OverlapCheck {
    struct Span {
        uintptr_t begin, end;
        bool output;
    };
    std::vector<Span> spans;
    void add(const void* in, const void* out, uint64_t len)
    {
        if (len == 0)
            return;
        const uintptr_t i = reinterpret_cast<uintptr_t>(in), o = reinterpret_cast<uintptr_t>(out);
        spans.push_back({i, i + (uintptr_t)len, false});
        spans.push_back({o, o + (uintptr_t)len, true});
    }
    bool an_output_overlaps()
    {
        std::sort(spans.begin(), spans.end(), [](const Span& a, const Span& b) { return a.begin < b.begin; });
        uintptr_t end_any = 0, end_output = 0;
        for (const Span& s : spans) {
            if (s.begin < (s.output ? end_any : end_output))
                return true;
            end_any = std::max(end_any, s.end);
            if (s.output)
                end_output = std::max(end_output, s.end);
        }
        return false;
    }
};

inline uint64_t estimator_windows(uint64_t len) { return (len + dxtlt::kEstimatorWindow - 1) / dxtlt::kEstimatorWindow; }

// Where the packer puts an item, and a chunk of consecutive items whose slices share the arena.  A family's planner derives its
// own item and chunk from these.
struct PackedItem {
    uint32_t chunk = 0;
    uint64_t slice_off = 0;       // inside the arena, a multiple of 16
    uint64_t first_counter = 0;   // of the item's run of counters; dense over the call, whatever the cap
};
struct PackedChunk {
    size_t first = 0, count = 0;
    uint64_t arena_bytes = 0;
    uint64_t estimator_wgs = 0;   // of the chunk's one estimator launch: a workgroup per 32 KiB window of every section
    uint32_t estimator_entries = 0;
    size_t sections_at = 0;       // in the call's table: the estimator's section table
    void count_section(uint64_t len)
    {
        estimator_wgs += estimator_windows(len);
        estimator_entries++;
    }
    // places the section table at `table_bytes` of the call's table; returns the bytes behind it (padded to 16)
    size_t place_sections(size_t table_bytes)
    {
        sections_at = table_bytes;
        return table_bytes + (((size_t)estimator_entries * sizeof(dxtlt::EstimateTableEntry) + 15) & ~size_t(15));
    }
};

// Cuts the items of a call, in their order, into chunks at `cap` arena bytes: every item -- an empty one too -- gets a 16-byte
// aligned slice and its counters.
template <class Chunk>   // a PackedChunk, with whatever the family keeps per chunk
struct ChunkPacker {
    std::vector<Chunk>& chunks;
    uint64_t cap;
    size_t items = 0;
    uint64_t counters = 0;
    uint64_t arena_bytes = 0;   // the largest chunk
    Chunk& add(uint64_t slice_bytes, uint32_t item_counters, PackedItem& item)
    {
        const uint64_t padded = (slice_bytes + 15) & ~uint64_t(15);
        // a chunk is closed BEFORE the item that would push it past the cap: it holds at most the cap, or one larger item
        if (chunks.empty() || (chunks.back().count > 0 && chunks.back().arena_bytes + padded > cap)) {
            chunks.emplace_back();
            chunks.back().first = items;
        }
        Chunk& cur = chunks.back();
        item.chunk = (uint32_t)(chunks.size() - 1);
        item.slice_off = cur.arena_bytes;
        item.first_counter = counters;
        counters += item_counters;
        cur.arena_bytes += padded;
        cur.count++;
        items++;
        arena_bytes = std::max(arena_bytes, cur.arena_bytes);
        return cur;
    }
};

// Writes a chunk's section table: fed the non-empty sections in order, it gives each the cumulative end workgroup that
// PackedChunk::count_section counted.
struct SectionWriter {
    dxtlt::EstimateTableEntry* at;
    uint32_t wgs = 0;
    void add(const uint8_t* base, uint64_t len, uint64_t counter)
    {
        wgs += (uint32_t)estimator_windows(len);
        *at++ = dxtlt::EstimateTableEntry{base, len, wgs, (uint32_t)counter};
    }
};

// ---- the call ---------------------------------------------------------------------------------------------------------------------
// this thread's table staging (mapped pinned host memory and its device twin) and counters (device and pinned host): grow-only.
// A batched auto call waits for its stream before it returns -- the winners it leaves enqueued read the table ring's slots, not
// these -- so one of each is enough for both calls.
struct BatchAutoBuffers {
    void *table_host = nullptr, *table_mapped = nullptr, *table_dev = nullptr;
    size_t table_cap = 0;
    uint64_t *counters_dev = nullptr, *counters_host = nullptr;
    size_t counters_cap = 0;
    int device = -1;
    ~BatchAutoBuffers() { release(); }
    void release()
    {
        if (table_host) (void)hipHostFree(table_host);
        if (table_dev) (void)hipFree(table_dev);
        if (counters_dev) (void)hipFree(counters_dev);
        if (counters_host) (void)hipHostFree(counters_host);
        table_host = table_mapped = table_dev = nullptr;
        counters_dev = counters_host = nullptr;
        table_cap = counters_cap = 0;
        device = -1;
    }
    hipError_t reserve(size_t table_bytes, size_t counters)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess)
            return e;
        if (dev != device) {
            release();
            device = dev;
        }
        if (table_bytes > table_cap) {
            if (table_host) (void)hipHostFree(table_host);
            if (table_dev) (void)hipFree(table_dev);
            table_host = table_mapped = table_dev = nullptr;
            table_cap = 0;
            const size_t want = (table_bytes + table_bytes / 2 + 4095) & ~size_t(4095);
            e = hipHostMalloc(&table_host, want, hipHostMallocMapped);
            if (e == hipSuccess)
                e = hipHostGetDevicePointer(&table_mapped, table_host, 0);
            if (e == hipSuccess)
                e = hipMalloc(&table_dev, want);
            if (e != hipSuccess)
                return e;
            table_cap = want;
        }
        if (counters > counters_cap) {
            if (counters_dev) (void)hipFree(counters_dev);
            if (counters_host) (void)hipHostFree(counters_host);
            counters_dev = counters_host = nullptr;
            counters_cap = 0;
            const size_t want = counters + counters / 2 + 64;
            e = hipMalloc(reinterpret_cast<void**>(&counters_dev), want * sizeof(uint64_t));
            if (e == hipSuccess)
                e = hipHostMalloc(reinterpret_cast<void**>(&counters_host), want * sizeof(uint64_t), hipHostMallocDefault);
            if (e != hipSuccess)
                return e;
            counters_cap = want;
        }
        return hipSuccess;
    }
};

// the calling thread's buffers (batch_auto_api.cpp owns them; freed by release_batch_auto_thread_buffers)
BatchAutoBuffers& batch_auto_thread_buffers();
// the chunk cap in force on the calling thread: dxtlt_debug_batch_auto_arena_cap's value, or DXTLT_BATCH_AUTO_ARENA_CAP
uint64_t batch_auto_arena_cap();

// a call with a non-empty item needs a device and a stream that is not capturing
inline int32_t auto_call_device_check(hipStream_t st)
{
    int devices = 0;
    hipError_t e = hipGetDeviceCount(&devices);
    if (e != hipSuccess || devices <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument, "the auto transforms read their estimates back and wait for the stream: not capturable");
    return kOk;
}

// What a call leaves for its debug hooks (dxtlt_debug_*batch_auto_last, _last_totals, _time_phases, _last_phase_ms): one
// thread-local instance per call.
struct BatchAutoDebug {
    explicit BatchAutoDebug(size_t totals_per_item) : stride(totals_per_item) {}
    size_t stride;
    uint64_t last[4] = {0, 0, 0, 0};     // stream waits, chunks, candidate launches, estimator launches
    std::vector<uint64_t> totals;
    std::vector<uint8_t> total_counts;   // totals the item really has: 0 for an empty one
    bool time_phases = false;
    double phase_ms[3] = {0, 0, 0};      // of the last timed call: candidate launches, estimator launches, (pixels) the winners
    void begin_call()
    {
        std::memset(last, 0, sizeof last);
        totals.clear();
        total_counts.clear();
    }
    void clear_phase_ms() { phase_ms[0] = phase_ms[1] = phase_ms[2] = 0; }
    void copy_last(uint64_t out[4]) const
    {
        if (out) std::memcpy(out, last, sizeof last);
    }
    int32_t copy_totals(size_t item, uint64_t* out, int32_t cap) const
    {
        if (item >= total_counts.size())
            return 0;
        const int32_t n = total_counts[item];
        for (int32_t i = 0; out != nullptr && i < n && i < cap; ++i)
            out[i] = totals[item * stride + (size_t)i];
        return n;
    }
    void copy_phase_ms(double* out, int n) const
    {
        if (out) std::memcpy(out, phase_ms, (size_t)n * sizeof(double));
    }
};

// the bench hooks' events: three per chunk -- in front of its candidate launches, between them and its estimator launch, behind
// it -- and `extra` more behind those for the call's own marks; read once what they mark has been waited for
struct PhaseEvents {
    EventList ev;
    bool begin(size_t chunks, size_t extra) { return ev.create(chunks * 3 + extra, hipEventDefault) == hipSuccess; }
    bool on() const { return !ev.empty(); }
    void mark(size_t k, hipStream_t st)
    {
        if (on()) (void)hipEventRecord(ev[k], st);
    }
    double between(size_t a, size_t b) const
    {
        float ms = 0;
        return hipEventElapsedTime(&ms, ev[a], ev[b]) == hipSuccess ? (double)ms : 0.0;
    }
};

// The stream work of a call up to its readback: counter clear, table upload, per chunk `candidates(c, launched)` and
// `estimator(c, launched)` -- each enqueues chunk c's launches, adds how many to `launched` and returns the first error -- then all
// counters in one copy and the ONE wait.  Fills debug.last and, with `phases` begun, debug.phase_ms[0..1].  A failure is recorded
// with `prefix` in front of the step's name.
template <class Candidates, class Estimator>
int32_t run_auto_chunks(const char* prefix, BatchAutoBuffers& buffers, size_t table_bytes, uint64_t counters, size_t chunks, hipStream_t st,
                        PhaseEvents& phases, BatchAutoDebug& debug, Candidates&& candidates, Estimator&& estimator)
{
    debug.clear_phase_ms();
    // every failure exit below drains the stream: the arena, the tables and the counters belong to this thread's next call
    hipError_t e = hipMemsetAsync(buffers.counters_dev, 0, (size_t)counters * sizeof(uint64_t), st);
    const char* step = ": counter clear";
    if (e == hipSuccess) {
        e = dxtlt::launch_table_upload(buffers.table_mapped, buffers.table_dev, (table_bytes + 15) & ~size_t(15), st);
        step = ": table upload";
    }
    for (size_t c = 0; c < chunks && e == hipSuccess; ++c) {
        phases.mark(c * 3, st);
        e = candidates(c, debug.last[2]);
        step = ": candidate kernel launch";
        phases.mark(c * 3 + 1, st);
        if (e == hipSuccess) {
            e = estimator(c, debug.last[3]);
            step = ": estimator launch";
        }
        phases.mark(c * 3 + 2, st);
        debug.last[1]++;
    }
    if (e == hipSuccess) {
        e = hipMemcpyAsync(buffers.counters_host, buffers.counters_dev, (size_t)counters * sizeof(uint64_t), hipMemcpyDeviceToHost, st);
        step = ": D2H estimates";
    }
    const hipError_t waited = hipStreamSynchronize(st);   // the one wait of the call
    debug.last[0]++;
    for (size_t c = 0; c < chunks && phases.on() && e == hipSuccess && waited == hipSuccess; ++c) {
        debug.phase_ms[0] += phases.between(c * 3, c * 3 + 1);
        debug.phase_ms[1] += phases.between(c * 3 + 1, c * 3 + 2);
    }
    if (e != hipSuccess)
        return fail(kDevice, (std::string(prefix) + step).c_str(), e);
    if (waited != hipSuccess)
        return fail(kDevice, "stream synchronize", waited);
    return kOk;
}

}  // namespace dxtlt_host
