// pixel_batch_plan.h -- the planners of the two batched uncompressed-pixel calls (pixel_batch_api.cpp:
// dxtlt_transform_pixels_batch_device; pixel_batch_auto_api.cpp: dxtlt_transform_pixels_batch_auto_device), pure host arithmetic:
// they check a whole batch and say what the call enqueues without touching a device or dereferencing an address.  The calls and
// the test hooks (dxtlt_debug_plan_pixels_batch, dxtlt_debug_plan_pixels_batch_auto) run these very functions; being pure, they
// also run stand-alone under the host sanitizers (tests/cpp/pixel_batch_plan_main.cpp).  What the auto planner shares with the block
// formats' (batch_auto_plan.h) -- the overlap rule, the chunk packer, the estimator's section table -- is batch_auto_common.h.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_pixels.h"
#include "batch_auto_common.h"
#include "bcn_launch.h"
#include "entropy_launch.h"
#include "host_common.h"
#include "pixel_batch_launch.h"
#include "pixel_launch.h"

namespace dxtlt_host {
namespace pixel_batch {

using dxtlt::pixels::PixelBatchEntry;

// a buffer as both calls' checks see it
struct Buffer {
    const void* in;
    const void* out;
    uint64_t len;
    uint8_t pixel_bytes;
    uint8_t layout;
};

inline uint64_t tiles_of(uint64_t pixels) { return (pixels + dxtlt::pixels::kTile - 1) / dxtlt::pixels::kTile; }

// The checks of both calls, the whole batch before anything else happens: per item, in this order, pixel_bytes, layout, NULL
// buffers, the length, the 64 GiB limit; then the rule that a d_output overlaps no other output and no input (OverlapCheck).
inline Defect check_buffers(const Buffer* b, size_t count)
{
    OverlapCheck spans;
    for (size_t i = 0; i < count; ++i) {
        if (b[i].pixel_bytes != 3 && b[i].pixel_bytes != 4)
            return {kInvalidArgument, "pixel batch item: pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)"};
        if (b[i].layout > 2)
            return {kInvalidArgument, "pixel batch item: layout must be 0 (INTERLEAVED), 1 (PLANAR) or 2 (PLANAR_DELTA)"};
        if (b[i].len > 0 && (b[i].in == nullptr || b[i].out == nullptr))
            return {kInvalidArgument, "pixel batch item: NULL device buffer with len > 0"};
        if (b[i].len % b[i].pixel_bytes != 0)
            return {kInvalidLength, "pixel batch item: len is not a multiple of pixel_bytes"};
        if (b[i].len >= (uint64_t(64) << 30))
            return {kInvalidArgument, "pixel batch item of 64 GiB or more: use the single-buffer entry point"};
        spans.add(b[i].in, b[i].out, b[i].len);
    }
    if (spans.an_output_overlaps())
        return {kInvalidArgument, "pixel batch item: a d_output overlaps another buffer of the batch"};
    return {};
}

// ---- dxtlt_transform_pixels_batch_device ----------------------------------------------------------------------------------------
// One launch of pixel_batch_tiles: the non-empty items of one (pixel_bytes, direction, decorrelate, layout) class, in item order.
struct ClassLaunch {
    int key = 0;   // (pixel_bytes == 3) * 12 + inverse * 6 + decorrelate * 3 + layout: launches go out in ascending key
    std::vector<PixelBatchEntry> entries;
    uint32_t wgs = 0;
    bool wide = false;               // the form of its workgroup index
    size_t at = 0, entry_bytes = 0;  // in the staged buffer: the entries, then the workgroup index

    int pixel_bytes() const { return key >= 12 ? 3 : 4; }
    bool inverse() const { return (key % 12) >= 6; }
    bool decorrelate() const { return (key % 6) >= 3; }
    int layout() const { return key % 3; }
};
inline int class_key(int pixel_bytes, bool inverse, bool decorrelate, int layout)
{
    return (pixel_bytes == 3 ? 12 : 0) + (inverse ? 6 : 0) + (decorrelate ? 3 : 0) + layout;
}

struct Plan {
    std::vector<ClassLaunch> launches;   // present classes only, in ascending key: at most 24
    std::vector<uint8_t> tables;         // every launch's tables at 16-byte aligned offsets of ONE staged buffer, as the device reads them
};

// The whole call: checks, class grouping, entries, workgroup indices, and the bytes of the one staged buffer.
inline Defect plan_call(const DxtltPixelBatchItem* items, size_t count, Plan& plan)
{
    plan = Plan{};
    if (count == 0)
        return {};
    if (items == nullptr)
        return {kInvalidArgument, "NULL item array with count > 0"};
    {
        std::vector<Buffer> buffers(count);
        for (size_t i = 0; i < count; ++i)
            buffers[i] = {items[i].d_input, items[i].d_output, items[i].len, items[i].pixel_bytes, items[i].layout};
        if (Defect d = check_buffers(buffers.data(), count); d.code != kOk)
            return d;
    }
    int launch_of_key[24];
    for (int& l : launch_of_key)
        l = -1;
    for (size_t i = 0; i < count; ++i) {
        const DxtltPixelBatchItem& it = items[i];
        if (it.len == 0)
            continue;   // an empty item owns no workgroup and has no entry
        const int key = class_key(it.pixel_bytes, it.inverse != 0, it.decorrelate != 0, it.layout);
        if (launch_of_key[key] < 0) {
            launch_of_key[key] = (int)plan.launches.size();
            plan.launches.emplace_back();
            plan.launches.back().key = key;
        }
        ClassLaunch& l = plan.launches[(size_t)launch_of_key[key]];
        const uint64_t pixels = it.len / it.pixel_bytes, wgs = tiles_of(pixels);
        // one launch holds fewer than 2^24 workgroups, which is also what build_batch_index's 32-bit spans take with room to spare
        if ((uint64_t)l.wgs + wgs > dxtlt::pixels::kPixelBatchMaxWorkgroups)
            return {kInvalidArgument, "pixel batch too large for one launch (2^24 tiles or more -- 256 GiB of 4-byte pixels -- in one class)"};
        l.entries.push_back({static_cast<const uint8_t*>(it.d_input), static_cast<uint8_t*>(it.d_output), pixels, l.wgs, l.wgs + (uint32_t)wgs});
        l.wgs += (uint32_t)wgs;
    }
    std::sort(plan.launches.begin(), plan.launches.end(), [](const ClassLaunch& a, const ClassLaunch& b) { return a.key < b.key; });
    size_t bytes = 0;
    for (ClassLaunch& l : plan.launches) {
        l.entry_bytes = (l.entries.size() * sizeof(PixelBatchEntry) + 15) & ~size_t(15);
        l.at = bytes;
        bytes += l.entry_bytes + dxtlt::batch_index_bytes(l.wgs);
    }
    plan.tables.assign(bytes, 0);
    std::vector<dxtlt::BatchEntry> spans;   // first_wg / end_wg of a launch's entries, for build_batch_index
    for (ClassLaunch& l : plan.launches) {
        std::memcpy(plan.tables.data() + l.at, l.entries.data(), l.entries.size() * sizeof(PixelBatchEntry));
        spans.assign(l.entries.size(), dxtlt::BatchEntry{});
        for (size_t k = 0; k < l.entries.size(); ++k) {
            spans[k].first_wg = l.entries[k].first_wg;
            spans[k].end_wg = l.entries[k].end_wg;
        }
        l.wide = dxtlt::build_batch_index(spans.data(), spans.size(), l.wgs, plan.tables.data() + l.at + l.entry_bytes);
    }
    return {};
}

// ---- dxtlt_transform_pixels_batch_auto_device -----------------------------------------------------------------------------------
constexpr int kCandidates = dxtlt::pixels::kAutoCandidates;   // in kAutoOrder (pixel_launch.h); the sixth is the input itself
static_assert(dxtlt::kEntropyWindow == dxtlt::kEstimatorWindow, "the shared section table counts the gram estimator's windows");

struct AutoItem : PackedItem {   // slice_off: candidate i < 5 at slice_off + i * len; first_counter: 6 * item, counter i is candidate i's
    uint64_t pixels = 0, len = 0;
    uint64_t slice_bytes = 0;    // inside the arena: 5 * len
};

struct AutoChunk : PackedChunk {
    uint32_t entries[2] = {0, 0}, wgs[2] = {0, 0};   // the candidate launch of 4-byte ([0]) and of 3-byte ([1]) pixels
    bool wide[2] = {false, false};
    size_t at[2] = {0, 0}, entry_bytes[2] = {0, 0};  // in the call's table: entries, then the workgroup index
    uint32_t candidate_launches() const { return (entries[0] != 0) + (entries[1] != 0); }
};

struct AutoPlan {
    std::vector<AutoItem> items;
    std::vector<AutoChunk> chunks;
    bool any = false;           // a non-empty item
    uint64_t counters = 0;
    uint64_t arena_bytes = 0;   // the largest chunk
    size_t table_bytes = 0;     // ONE table for the whole call
};

// Checks, arena slices, counters, chunks (closed at `cap` bytes; a larger item is a chunk by itself) and every table's place.
inline Defect plan_auto_call(const DxtltPixelBatchAutoItem* items, size_t count, uint64_t cap, AutoPlan& plan)
{
    plan = AutoPlan{};
    if (count == 0)
        return {};
    if (items == nullptr)
        return {kInvalidArgument, "NULL item array with count > 0"};
    {
        std::vector<Buffer> buffers(count);
        for (size_t i = 0; i < count; ++i)
            buffers[i] = {items[i].d_input, items[i].d_output, items[i].len, items[i].pixel_bytes, 0};
        if (Defect d = check_buffers(buffers.data(), count); d.code != kOk)
            return d;
    }
    // the winners go out through the planner above, one launch per class.  Which class wins is not known yet, so the items of one
    // pixel_bytes are held to a launch's limit together -- refused here, not after the choices have been written.
    uint64_t winner_wgs[2] = {0, 0};
    for (size_t i = 0; i < count; ++i)
        winner_wgs[items[i].pixel_bytes == 4 ? 0 : 1] += tiles_of(items[i].len / items[i].pixel_bytes);
    for (uint64_t w : winner_wgs)
        if (w > dxtlt::pixels::kPixelBatchMaxWorkgroups)
            return {kInvalidArgument, "pixel batch auto: too large for one launch (2^24 tiles or more of one pixel_bytes)"};

    plan.items.assign(count, AutoItem{});
    ChunkPacker<AutoChunk> pack{plan.chunks, cap};
    for (size_t i = 0; i < count; ++i) {
        AutoItem& p = plan.items[i];
        p.len = items[i].len;
        p.pixels = p.len / items[i].pixel_bytes;
        p.slice_bytes = 5 * p.len;
        AutoChunk& cur = pack.add(p.slice_bytes, kCandidates, p);
        if (p.len != 0) {
            const int b = items[i].pixel_bytes == 4 ? 0 : 1;
            plan.any = true;
            cur.entries[b]++;
            cur.wgs[b] += (uint32_t)tiles_of(p.pixels);   // (below a launch's limit: checked for the whole batch above)
            for (int k = 0; k < kCandidates; ++k)
                cur.count_section(p.len);
        }
    }
    plan.counters = pack.counters;
    plan.arena_bytes = pack.arena_bytes;
    for (AutoChunk& c : plan.chunks) {
        if (c.estimator_wgs > 0x7FFFFFFFull)
            return {kInvalidArgument, "pixel batch auto: a chunk of more than 2^31 - 1 estimator windows"};
        for (int b = 0; b < 2; ++b) {
            c.entry_bytes[b] = ((size_t)c.entries[b] * sizeof(PixelBatchEntry) + 15) & ~size_t(15);
            c.at[b] = plan.table_bytes;
            if (c.entries[b] != 0)
                plan.table_bytes += c.entry_bytes[b] + dxtlt::batch_index_bytes(c.wgs[b]);
        }
        plan.table_bytes = c.place_sections(plan.table_bytes);
    }
    if (plan.table_bytes > (size_t(1) << 31))
        return {kInvalidArgument, "pixel batch auto: too many items for one call (a table of more than 2 GiB)"};
    return {};
}

// Writes the call's table (plan.table_bytes bytes at `host`, 16-byte aligned) for an arena at `arena`: per chunk the candidate
// launches' entries and indices, then the estimator's sections -- candidates 0..4 where they lie in the item's slice, the sixth
// section the item's d_input itself.  Sets the chunks' `wide` flags.
inline void fill_auto_tables(AutoPlan& plan, const DxtltPixelBatchAutoItem* items, uint8_t* arena, uint8_t* host)
{
    std::memset(host, 0, plan.table_bytes);
    std::vector<dxtlt::BatchEntry> spans;
    for (AutoChunk& c : plan.chunks) {
        for (int b = 0; b < 2; ++b) {
            if (c.entries[b] == 0)
                continue;
            PixelBatchEntry* e = reinterpret_cast<PixelBatchEntry*>(host + c.at[b]);
            spans.clear();
            uint32_t wgs = 0;
            for (size_t i = c.first; i < c.first + c.count; ++i) {
                const AutoItem& p = plan.items[i];
                if (p.len == 0 || (items[i].pixel_bytes == 4 ? 0 : 1) != b)
                    continue;
                const uint32_t end = wgs + (uint32_t)tiles_of(p.pixels);
                *e++ = PixelBatchEntry{static_cast<const uint8_t*>(items[i].d_input), arena + p.slice_off, p.pixels, wgs, end};
                spans.emplace_back();
                spans.back().first_wg = wgs;
                spans.back().end_wg = end;
                wgs = end;
            }
            c.wide[b] = dxtlt::build_batch_index(spans.data(), spans.size(), c.wgs[b], host + c.at[b] + c.entry_bytes[b]);
        }
        SectionWriter sections{reinterpret_cast<dxtlt::EstimateTableEntry*>(host + c.sections_at)};
        for (size_t i = c.first; i < c.first + c.count; ++i) {
            const AutoItem& p = plan.items[i];
            for (int k = 0; k < kCandidates && p.len != 0; ++k) {
                const uint8_t* base = k == kCandidates - 1 ? static_cast<const uint8_t*>(items[i].d_input) : arena + p.slice_off + (uint64_t)k * p.len;
                sections.add(base, p.len, p.first_counter + (uint64_t)k);
            }
        }
    }
}

}  // namespace pixel_batch
}  // namespace dxtlt_host
