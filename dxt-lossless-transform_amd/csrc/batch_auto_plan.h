// batch_auto_plan.h -- the planner of dxtlt_transform_batch_auto_device (batch_auto_api.cpp), pure host arithmetic: it checks a
// whole batch and says what the call enqueues without touching a device or dereferencing an address.  The call and the test hook
// (dxtlt_debug_plan_batch_auto) run these very functions; being pure, they also run stand-alone under the host sanitizers
// (tests/cpp/batch_auto_plan_main.cpp).  The twin of pixel_batch_plan.h's auto half; what the two share is batch_auto_common.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/dxtlt_estimator.h"
#include "auto_launch.h"
#include "batch_auto_common.h"

namespace dxtlt_host {
namespace batch_auto {

constexpr int kMaxSections = 10;   // counters per item: BC3 with every mode, 2 alpha + 8 colour sections
constexpr int kGroups = 10;        // candidate launches a chunk can have: group (format - 1) * 2 + use_all

inline uint32_t block_bytes_of(uint8_t format) { return format == 1 || format == 4 ? 8u : 16u; }
inline bool use_all_of(const DxtltBatchAutoItem& it) { return it.use_all_decorrelation_modes != 0 && it.format <= 3; }
inline int group_of(const DxtltBatchAutoItem& it) { return (it.format - 1) * 2 + (use_all_of(it) ? 1 : 0); }

struct PlannedItem : PackedItem {
    int sections = 0;
    uint64_t blocks = 0;
    uint64_t slice_bytes = 0;                                 // dxtlt::auto_sections of the item, end to end
    uint64_t sec_off[kMaxSections], sec_len[kMaxSections];   // sec_off: from the slice's first byte
};

struct PlannedChunk : PackedChunk {
    uint32_t entries[kGroups] = {}, wgs[kGroups] = {};   // the candidate launch of group g: its non-empty items, in item order
    size_t at[kGroups] = {};                             // in the call's table: the launch's entries
    uint32_t candidate_launches() const { return (uint32_t)(kGroups - std::count(entries, entries + kGroups, 0u)); }
};

struct Plan {
    std::vector<PlannedItem> items;
    std::vector<PlannedChunk> chunks;
    bool any = false;           // a non-empty item
    uint64_t counters = 0;
    uint64_t arena_bytes = 0;   // the largest chunk
    size_t table_bytes = 0;     // ONE table for the whole call
};

// The whole batch before anything else happens.  Per item, in this order: format, block multiple, NULL buffers, the 64 GiB limit;
// then the winners' limit and the overlap rule.  Then arena slices, counters, chunks (closed at `cap` bytes; a larger item is a
// chunk by itself) and every table's place.
inline Defect plan_call(const DxtltBatchAutoItem* items, size_t count, uint64_t cap, Plan& plan)
{
    plan = Plan{};
    if (count == 0)
        return {};
    if (items == nullptr)
        return {kInvalidArgument, "NULL item array with count > 0"};
    OverlapCheck spans;
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchAutoItem& it = items[i];
        if (it.format < 1 || it.format > 5)
            return {kInvalidArgument, "batch auto item: format must be 1..5 (BC1..BC5)"};
        if (it.len % block_bytes_of(it.format) != 0)
            return {kInvalidLength, "batch auto item: len is not a multiple of the block size"};
        if (it.len > 0 && (it.d_input == nullptr || it.d_output == nullptr))
            return {kInvalidArgument, "batch auto item: NULL device buffer with len > 0"};
        if (it.len >= (uint64_t(64) << 30))
            return {kInvalidArgument, "batch auto item of 64 GiB or more: use the single-buffer entry point"};
        spans.add(it.d_input, it.d_output, it.len);
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
            return {kInvalidArgument, "batch auto: too large for one launch (about 32 GiB of BC1 / BC4 or 64 GiB of BC2 / BC3 / BC5 items)"};
    if (spans.an_output_overlaps())
        return {kInvalidArgument, "batch auto item: a d_output overlaps another buffer of the batch"};

    plan.items.assign(count, PlannedItem{});
    ChunkPacker<PlannedChunk> pack{plan.chunks, cap};
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchAutoItem& it = items[i];
        PlannedItem& p = plan.items[i];
        p.blocks = it.len / block_bytes_of(it.format);
        const dxtlt::AutoSections secs = dxtlt::auto_sections((dxtlt::Format)it.format, use_all_of(it), p.blocks);
        p.slice_bytes = secs.bytes;
        p.sections = secs.count;
        std::copy(secs.off, secs.off + secs.count, p.sec_off);
        std::copy(secs.len, secs.len + secs.count, p.sec_len);
        PlannedChunk& cur = pack.add(p.slice_bytes, (uint32_t)p.sections, p);
        if (p.blocks != 0) {
            plan.any = true;
            cur.entries[group_of(it)]++;
            cur.wgs[group_of(it)] += dxtlt::batch_auto_workgroups((dxtlt::Format)it.format, p.blocks);
            for (int k = 0; k < p.sections; ++k)
                cur.count_section(p.sec_len[k]);
        }
    }
    plan.counters = pack.counters;
    plan.arena_bytes = pack.arena_bytes;
    for (PlannedChunk& c : plan.chunks) {
        if (c.estimator_wgs > 0x7FFFFFFFull)
            return {kInvalidArgument, "batch auto: a chunk of more than 2^31 - 1 estimator windows"};
        for (int g = 0; g < kGroups; ++g) {
            c.at[g] = plan.table_bytes;
            plan.table_bytes += (size_t)c.entries[g] * sizeof(dxtlt::BatchAutoEntry);
        }
        plan.table_bytes = c.place_sections(plan.table_bytes);
    }
    if (plan.table_bytes > (size_t(1) << 31))
        return {kInvalidArgument, "batch auto: too many items for one call (a table of more than 2 GiB)"};
    return {};
}

// Writes the call's table (plan.table_bytes bytes at `host`, 16-byte aligned) for an arena at `arena`: per chunk the candidate
// launches' entries in ascending group order, then the estimator's sections where they lie in the items' slices.
inline void fill_tables(const Plan& plan, const DxtltBatchAutoItem* items, uint8_t* arena, uint8_t* host)
{
    for (const PlannedChunk& c : plan.chunks) {
        dxtlt::BatchAutoEntry* entry[kGroups];
        uint32_t first_wg[kGroups] = {};
        for (int g = 0; g < kGroups; ++g)
            entry[g] = reinterpret_cast<dxtlt::BatchAutoEntry*>(host + c.at[g]);
        SectionWriter sections{reinterpret_cast<dxtlt::EstimateTableEntry*>(host + c.sections_at)};
        for (size_t i = c.first; i < c.first + c.count; ++i) {
            const PlannedItem& p = plan.items[i];
            if (p.blocks == 0)
                continue;   // an empty item owns no workgroup and has no entry
            const int g = group_of(items[i]);
            *entry[g]++ = dxtlt::BatchAutoEntry{static_cast<const uint8_t*>(items[i].d_input), p.slice_off, p.blocks, first_wg[g], 0};
            first_wg[g] += dxtlt::batch_auto_workgroups((dxtlt::Format)items[i].format, p.blocks);
            for (int k = 0; k < p.sections; ++k)
                sections.add(arena + p.slice_off + p.sec_off[k], p.sec_len[k], p.first_counter + (uint64_t)k);
        }
    }
}

}  // namespace batch_auto
}  // namespace dxtlt_host
