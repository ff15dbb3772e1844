// batch_api.cpp -- dxtlt_transform_batch_device: many device-resident buffers in one call.
//
// The reference transforms file after file (its CLI fans files out over rayon workers); a texture is typically
// 0.1-20 MiB.  On MI355X one such buffer cannot fill the chip (a 1 MiB BC1 texture is 256 workgroups for 256 CUs) and
// a launch costs the host ~5 us, longer than the kernel runs: measured 186 GiB/s for 1024 x 1 MiB through one call per
// buffer, even when spread over eight streams (profiles/r01_x).  So a batch becomes ONE launch per (format, direction
// and settings combination) present in it: the host lays the buffers' workgroups end to end in a table (96 bytes per buffer
// plus a two-level workgroup -> buffer index: bcn_launch.h), sends the tables of all its launches to the device in ONE upload on
// the caller's stream (a small kernel reads the mapped pinned slot: no copy-engine hand-over in front of the batch kernel) and
// launches batch_kernel (batch_kernels.hip), in which every workgroup looks its buffer up and runs one tile -- aligned, halo
// or shifted, as the single-buffer call would choose for that buffer -- or the buffer's edge tile.  Asynchronous and ordered
// like a single call on the caller's stream.  Uncompressed-pixel items (formats 8, 9: include/dxtlt_pixels.h) are taken by the
// host batch only (dxtlt_transform_batch_host, batch_host_api.cpp, which runs batch_device here on every chunk it has uploaded):
// checked with the rest there, they go out as one launch each, behind the batches of their chunk.
//
// Planning is pure host arithmetic: plan_batch checks the whole batch and says what the call enqueues -- the granule launches, the
// tile launches, the items that go out alone, every table's place in the staged buffer -- without touching a device or an address;
// fill_tables writes the tables.  The call (batch_device) and the test hooks (dxtlt_debug_plan_batch, dxtlt_debug_plan_batch_call)
// run the same two functions; the call stages through StagedTables (batch_tables.h), as the two image batch calls do.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_gfx950.h"
#include "batch_tables.h"
#include "batch_tile_plan.h"
#include "bcn_launch.h"
#include "granule_launch.h"
#include "host_common.h"

namespace {

using namespace dxtlt_host;
using dxtlt::BatchEntry;

// dxtlt_transform_batch_device takes 1..7, as before; dxtlt_transform_batch_host also 8 and 9
const char* const kDeviceFormatText = "batch item: format must be 1..5 (BC1..BC5), 6 (BC6H) or 7 (BC7; 6 and 7 are this build's own formats; "
                                      "pixel formats 8 and 9 go through dxtlt_transform_batch_host or the calls of dxtlt_pixels.h)";
const char* const kHostFormatText = "batch item: format must be 1..5 (BC1..BC5), 6 (BC6H), 7 (BC7), 8 (4-byte pixels) or 9 (3-byte pixels; "
                                    "6 to 9 are this build's own formats)";

// Pixel items (8, 9; include/dxtlt_pixels.h) are checked with the rest and go out as one launch each: their input and output
// must not overlap
inline bool pixel_item_overlaps(const DxtltBatchItem& it)
{
    if (!is_pixel_format(it.format) || it.len == 0)
        return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(it.d_input), b = reinterpret_cast<uintptr_t>(it.d_output);
    return a < b + it.len && b < a + it.len;
}

int32_t launch_pixel_item(const DxtltBatchItem& it, void* stream)
{
    const uint64_t pixels = it.len / item_block_bytes(it.format);
    return pixel_device_range(pixel_bytes_of(it.format), it.inverse != 0, it.d_input, it.d_output, pixels, 0, pixels,
                              pixel_decorrelate_of(it.decorrelation_mode),
                              pixel_layout_of(it.split_alpha_endpoints != 0, it.split_colour_endpoints != 0), stream);
}

// Table staging: table_ring.h, batch_tables.h (shared with the image batch calls)
thread_local dxtlt_host::TableRing g_ring;

}  // namespace

dxtlt_host::TableRing& dxtlt_host::thread_table_ring() { return g_ring; }

// By a kernel, not by the copy engine (the first version; the comparison is profiles/r02_m_batch_kernel.txt)
hipError_t dxtlt_host::upload_table(TableSlot* slot, size_t bytes, hipStream_t stream)
{
    return dxtlt::launch_table_upload(slot->host_mapped, slot->dev, bytes, stream);
}

void dxtlt_host::release_batch_thread_tables() { g_ring.release(); }

// The per-item checks of both batch calls, in the order in which defects are reported.  `host_call`: the texts of
// dxtlt_transform_batch_host, whose items also stay below 4 GiB.  kOk, or the failure as fail() recorded it.
int32_t dxtlt_host::batch_item_defect(const DxtltBatchItem& it, int max_format, bool host_call)
{
    if (it.format < 1 || it.format > max_format)
        return fail(kInvalidArgument, host_call ? kHostFormatText : kDeviceFormatText);
    if (it.len % item_block_bytes(it.format) != 0)
        return fail(kInvalidLength, "batch item: len is not a multiple of the block size");
    if (it.decorrelation_mode > 3 && dxtlt::format_has_colour(it.format))
        return fail(kInvalidArgument, "batch item: decorrelation_mode must be 0..3");
    if (it.len > 0 && (it.d_input == nullptr || it.d_output == nullptr))
        return fail(kInvalidArgument, host_call ? "batch item: NULL buffer with len > 0" : "batch item: NULL device buffer with len > 0");
    if (pixel_item_overlaps(it))
        return fail(kInvalidArgument, "batch item: pixel input and output overlap");
    if (host_call && it.len >= (size_t(4) << 30))
        return fail(kInvalidArgument, "batch item of 4 GiB or more: use the single-buffer entry point");
    return kOk;
}

namespace {

// the settings a BC1..BC5 item's kernels are instantiated with (BC4 / BC5: no variant, no colour split; BC1 / BC2: no alpha split)
inline dxtlt::Settings item_settings(const DxtltBatchItem& it)
{
    dxtlt::Settings s{};
    s.variant = it.decorrelation_mode;
    s.split_alpha = it.split_alpha_endpoints != 0;
    s.split_colour = it.split_colour_endpoints != 0;
    return dxtlt::effective_settings((dxtlt::Format)it.format, s);
}

// (TileLaunch, one launch of batch_kernel, and what is done with a plan's tile launches: batch_tile_plan.h)

// BC7 items (format 7; no settings): their granules in one launch per direction, their tail parts in a second one.  BC6H items
// (format 6) the same, in launches of their own.
using GranuleEntry = dxtlt::granule::BatchEntry;
struct GranuleLaunch {
    std::vector<GranuleEntry> entries, tails;
    std::vector<uint32_t> coarse;
    uint64_t wgs = 0;
    size_t items = 0;
    size_t at = 0, entry_bytes = 0, tail_bytes = 0, bytes = 0;   // in the staged buffer: entries, tails, coarse index
};

// What a call enqueues, in its order: granules[0..3] (BC7 forward, inverse; BC6H forward, inverse), the tile launches, the singles,
// the pixel items.
struct BatchPlan {
    GranuleLaunch granules[4];
    std::vector<TileLaunch> tiles;   // present groups only, in ascending key
    std::vector<size_t> singles;     // items the batch kernel does not take (plan_batch_entry): launched alone, behind the batches
    std::vector<size_t> pixels;      // non-empty items of formats 8, 9: one launch each, behind the rest
    size_t table_bytes = 0;          // every table above at a 16-byte aligned offset of ONE staged buffer
};
inline int granule_format(int q) { return q < 2 ? 7 : 6; }

// Validates the batch as a whole and plans it; nothing is enqueued, no device is touched, no address is dereferenced.
// `pixels_allowed`: items of formats 8 and 9 are taken too (the host batch's chunks: their buffers are this library's own staging,
// checked by the host call) -- the public device call keeps refusing them.
int32_t plan_batch(const DxtltBatchItem* items, size_t count, bool pixels_allowed, BatchPlan& plan)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    // validate everything first: a batch is enqueued whole or not at all
    for (size_t i = 0; i < count; ++i)
        if (int32_t rc = batch_item_defect(items[i], pixels_allowed ? 9 : 7, false); rc != kOk)
            return rc;
    // one launch holds fewer than 2^32 threads = 2^24 workgroups of 256 lanes: for BC7 (or BC6H) that is 256 GiB of granules
    // per direction
    for (const int format : {7, 6}) {
        uint64_t granules[2] = {0, 0};
        for (size_t i = 0; i < count; ++i)
            if (items[i].format == format)
                granules[items[i].inverse ? 1 : 0] += items[i].len / 16 / 1024;
        if (granules[0] > 0xFFFFFFull || granules[1] > 0xFFFFFFull)
            return fail(kInvalidArgument, dxtlt::granule::named(format, "batch too large for one launch (256 GiB or more of ", " in one direction)"));
    }

    int launch_of_key[5 * 2 * 16];   // format, direction, settings code
    for (int& l : launch_of_key)
        l = -1;
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchItem& it = items[i];
        if (it.len == 0 || dxtlt::granule::is_granule_format(it.format))
            continue;
        if (is_pixel_format(it.format)) {
            plan.pixels.push_back(i);
            continue;
        }
        if (it.len >= (size_t(64) << 30))
            return fail(kInvalidArgument, "batch item of 64 GiB or more: use the single-buffer entry point");
        const dxtlt::Settings s = item_settings(it);
        const int key = (((it.format - 1) * 2 + (it.inverse ? 1 : 0)) << 4) | settings_code(s);
        int li = launch_of_key[key];
        BatchEntry e{};
        e.src = static_cast<const uint8_t*>(it.d_input);
        e.dst = static_cast<uint8_t*>(it.d_output);
        e.blocks = it.len / item_block_bytes(it.format);
        e.first_wg = li >= 0 ? plan.tiles[(size_t)li].wgs : 0;
        const uint32_t wgs = dxtlt::plan_batch_entry((dxtlt::Format)it.format, it.inverse != 0, s, e);
        if (wgs == 0xFFFFFFFFu) {
            plan.singles.push_back(i);
            continue;
        }
        // one launch holds fewer than 2^32 threads = 2^24 workgroups of 256 (64 GiB of blocks per format, direction and settings)
        if (!add_tile_entry(plan.tiles, launch_of_key[key], key, 0, e, wgs))
            return fail(kInvalidArgument, "batch too large for one launch (64 GiB or more of one format, direction and settings)");
    }
    order_tile_launches(plan.tiles);

    for (int q = 0; q < 4; ++q) {
        GranuleLaunch& p = plan.granules[q];
        const int inverse = q & 1, format = granule_format(q);
        for (size_t i = 0; i < count; ++i) {
            const DxtltBatchItem& it = items[i];
            if (it.format != format || it.len == 0 || (it.inverse != 0) != (inverse != 0))
                continue;
            const uint64_t blocks = it.len / 16, tail = blocks % 1024, main = blocks - tail;
            const uint8_t* src = static_cast<const uint8_t*>(it.d_input);
            uint8_t* dst = static_cast<uint8_t*>(it.d_output);
            ++p.items;
            if (main != 0) {
                p.entries.push_back({src, dst, main, (uint32_t)p.wgs, 0});
                p.wgs += main / 1024;
            }
            if (tail != 0)
                p.tails.push_back({src + main * 16, dst + main * 16, 0, 0, (uint32_t)tail});
        }
        if (p.items == 0)
            continue;
        p.coarse.resize(coarse_index_count((uint32_t)p.wgs));
        build_coarse_index(p.entries.data(), p.entries.size(), (uint32_t)p.wgs, p.coarse.data());
        p.entry_bytes = p.entries.size() * sizeof(GranuleEntry);
        p.tail_bytes = p.tails.size() * sizeof(GranuleEntry);
        p.bytes = padded(p.entry_bytes + p.tail_bytes + p.coarse.size() * sizeof(uint32_t), 16);
        p.at = plan.table_bytes;
        plan.table_bytes += p.bytes;
    }
    // Every table of the call -- the granule tables above, then every tile launch's (entries, then the workgroup index) -- goes into
    // ONE staged buffer and ONE upload, at 16-byte aligned offsets: one ring slot per call.  (One slot per group made a call with many
    // settings combinations -- rare in a corpus, routine in the fuzz: up to 96 groups -- wait in hipEventSynchronize for kernels this
    // same call had enqueued: the "asynchronous" call then drained its own work, and would deadlock under a caller whose stream is
    // gated on an event recorded after the call returns.  Three slots per call -- BC7 forward, BC7 inverse, the groups -- still let
    // the NEXT mixed call wait for this one's kernels; see the ring's comment.)
    place_tile_tables(plan.tiles, plan.table_bytes);
    return kOk;
}

// Writes the plan's tables into `host` (plan.table_bytes bytes, 16-byte aligned) as the device reads them
void fill_tables(BatchPlan& plan, uint8_t* host)
{
    for (const GranuleLaunch& p : plan.granules) {
        uint8_t* h = host + p.at;
        if (p.entry_bytes) std::memcpy(h, p.entries.data(), p.entry_bytes);
        if (p.tail_bytes) std::memcpy(h + p.entry_bytes, p.tails.data(), p.tail_bytes);
        if (!p.coarse.empty()) std::memcpy(h + p.entry_bytes + p.tail_bytes, p.coarse.data(), p.coarse.size() * sizeof(uint32_t));
    }
    fill_tile_tables(plan.tiles, host);
}

}  // namespace

// The device batch: planned whole, its tables staged in one slot, then its launches in the plan's order on the caller's stream
int32_t dxtlt_host::batch_device(const DxtltBatchItem* items, size_t count, void* hip_stream, bool pixels_allowed)
{
    BatchPlan plan;
    if (int32_t rc = plan_batch(items, count, pixels_allowed, plan); rc != kOk)
        return rc;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);
    if (plan.table_bytes != 0) {
        StagedTables tables;
        hipError_t e = tables.acquire(plan.table_bytes);
        if (e != hipSuccess)
            return fail(kDevice, "batch table staging", e);
        fill_tables(plan, tables.host());
        e = tables.upload(user);
        const char* what = "batch table copy / launch";
        for (int q = 0; q < 4 && e == hipSuccess; ++q) {
            const GranuleLaunch& p = plan.granules[q];
            if (p.bytes == 0)
                continue;
            const uint8_t* d = tables.dev() + p.at;
            e = dxtlt::granule::launch_batch(granule_format(q), (q & 1) != 0, reinterpret_cast<const GranuleEntry*>(d),
                                             reinterpret_cast<const uint32_t*>(d + p.entry_bytes + p.tail_bytes), (uint32_t)p.entries.size(),
                                             (uint32_t)p.wgs, reinterpret_cast<const GranuleEntry*>(d + p.entry_bytes),
                                             (uint32_t)p.tails.size(), user);
            if (e != hipSuccess)
                what = granule_format(q) == 7 ? "BC7 batch table copy / launch" : "BC6H batch table copy / launch";
        }
        for (size_t k = 0; k < plan.tiles.size() && e == hipSuccess; ++k) {
            const TileLaunch& l = plan.tiles[k];
            const uint8_t* d = tables.dev() + l.at;
            e = dxtlt::launch_batch(l.format(), l.inverse(), settings_of_code(l.key & 15), reinterpret_cast<const BatchEntry*>(d),
                                    d + l.entry_bytes, (uint32_t)l.entries.size(), l.wgs, l.uniform_wgs, l.wide, user,
                                    l.strided ? &l.entries[0] : nullptr, l.src_stride, l.dst_stride);
        }
        if (int32_t rc = tables.finish(e, user, what, "batch event"); rc != kOk)
            return rc;
    }
    // buffers with a stream base off its element width: the single-buffer call, one launch each
    for (size_t i : plan.singles) {
        const DxtltBatchItem& it = items[i];
        const uint64_t blocks = it.len / item_block_bytes(it.format);
        HIP_TRY(dxtlt::launch_transform((dxtlt::Format)it.format, it.inverse != 0, item_settings(it), it.d_input, it.d_output,
                                        dxtlt::Range{blocks, 0, blocks}, user),
                "batch item launch");
    }
    for (size_t i : plan.pixels)
        if (int32_t rc = launch_pixel_item(items[i], user); rc != kOk)
            return rc;
    return kOk;
}

namespace {

void* address(uint64_t a) { return reinterpret_cast<void*>(static_cast<uintptr_t>(a)); }

}  // namespace

extern "C" int32_t dxtlt_transform_batch_device(const DxtltBatchItem* items, size_t count, void* hip_stream)
{
    return batch_device(items, count, hip_stream, false);
}

// Test hooks (no device needed, nothing is dereferenced; include/dxtlt_gfx950.h): they run the call's own plan_batch and
// fill_tables, into host memory, so that the host logic which ships can be checked on a machine without a GPU
// (tests/test_batch_plan.py, tests/test_batch_call_plan.py).
//
// dxtlt_debug_plan_batch: buffers of one format, direction and settings, as items of one call -- which then has one tile launch
// at the most.  Hands back every buffer's entry and the launch's workgroup -> entry index.
extern "C" uint32_t dxtlt_debug_plan_batch(int32_t format, int32_t inverse, int32_t variant, int32_t split_alpha, int32_t split_colour,
                                           const uint64_t* src_addresses, const uint64_t* dst_addresses, const uint64_t* blocks, size_t count,
                                           DxtltDebugPlannedEntry* entries_out, uint8_t* index_out, size_t index_capacity,
                                           uint32_t* index_is_wide_out)
{
    if (index_is_wide_out)
        *index_is_wide_out = 0;
    if (format < 1 || format > 5 || (count != 0 && (!src_addresses || !dst_addresses || !blocks || !entries_out)))
        return 0xFFFFFFFFu;
    std::vector<DxtltBatchItem> items(count);
    for (size_t i = 0; i < count; ++i) {
        if (blocks[i] >= (uint64_t(64) << 30) / item_block_bytes((uint8_t)format))
            return 0xFFFFFFFFu;
        items[i] = DxtltBatchItem{address(src_addresses[i]), address(dst_addresses[i]), blocks[i] * item_block_bytes((uint8_t)format),
                                  (uint8_t)format, (uint8_t)(inverse != 0), (uint8_t)std::min<uint32_t>((uint32_t)variant, 255),
                                  (uint8_t)(split_alpha != 0), (uint8_t)(split_colour != 0), {0, 0, 0}};
    }
    BatchPlan plan;
    if (plan_batch(items.data(), count, false, plan) != kOk || !plan.singles.empty())
        return 0xFFFFFFFFu;
    static const TileLaunch none;
    const TileLaunch& l = plan.tiles.empty() ? none : plan.tiles[0];
    if (l.wgs != 0 && (index_out == nullptr || index_capacity < dxtlt::batch_index_bytes(l.wgs)))
        return 0xFFFFFFFFu;
    size_t k = 0;
    for (size_t i = 0; i < count; ++i) {
        DxtltDebugPlannedEntry& o = entries_out[i];
        o = DxtltDebugPlannedEntry{};
        if (blocks[i] == 0) {   // owns no workgroup, has no entry
            o.first_wg = o.end_wg = k < l.entries.size() ? l.entries[k].first_wg : l.wgs;
            continue;
        }
        const BatchEntry& e = l.entries[k++];
        o.first_wg = e.first_wg;
        o.end_wg = e.end_wg;
        o.full_tiles = e.full_tiles;
        o.form = e.form;
        o.halo_vecs = e.halo_vecs;
        std::memcpy(o.shift, e.shift, sizeof o.shift);
        std::memcpy(o.gbase, e.gbase, sizeof o.gbase);
    }
    if (l.wgs != 0) {
        std::vector<uint8_t> tables(plan.table_bytes);
        fill_tables(plan, tables.data());
        std::memcpy(index_out, tables.data() + plan.tiles[0].at + plan.tiles[0].entry_bytes, dxtlt::batch_index_bytes(l.wgs));
        if (index_is_wide_out)
            *index_is_wide_out = plan.tiles[0].wide ? 1 : 0;
    }
    return l.wgs;
}

// dxtlt_debug_plan_batch_call: any batch; one record per launch, in the order in which the call enqueues them
extern "C" int32_t dxtlt_debug_plan_batch_call(const DxtltBatchItem* items, size_t count, int32_t pixels_allowed, DxtltDebugBatchLaunch* out,
                                               size_t cap, uint64_t* table_bytes_out)
{
    if (table_bytes_out)
        *table_bytes_out = 0;
    BatchPlan plan;
    if (plan_batch(items, count, pixels_allowed != 0, plan) != kOk)
        return -1;
    std::vector<uint8_t> tables(plan.table_bytes);
    fill_tables(plan, tables.data());
    if (table_bytes_out)
        *table_bytes_out = plan.table_bytes;
    size_t n = 0;
    auto put = [&](const DxtltDebugBatchLaunch& r) {
        if (out != nullptr && n < cap)
            out[n] = r;
        ++n;
    };
    for (int q = 0; q < 4; ++q) {
        const GranuleLaunch& p = plan.granules[q];
        if (p.bytes == 0)
            continue;
        DxtltDebugBatchLaunch r{};
        r.kind = 0, r.format = granule_format(q), r.inverse = q & 1;
        r.items = (uint32_t)p.items, r.entries = (uint32_t)p.entries.size(), r.tails = (uint32_t)p.tails.size(), r.workgroups = (uint32_t)p.wgs;
        r.table_offset = p.at, r.table_bytes = p.bytes;
        put(r);
    }
    for (const TileLaunch& l : plan.tiles)
        put(tile_launch_record(l));
    for (int kind = 2; kind <= 3; ++kind)
        for (size_t i : kind == 2 ? plan.singles : plan.pixels) {
            DxtltDebugBatchLaunch r{};
            r.kind = kind, r.format = items[i].format, r.inverse = items[i].inverse ? 1 : 0;
            r.settings_code = kind == 2 ? settings_code(item_settings(items[i])) : 0;
            r.items = r.entries = 1, r.first_item = i;
            put(r);
        }
    return (int32_t)n;
}

// the granule launch of `format` (7, 6) and direction in the same plan: its entries and its coarse index, read back from the
// tables as staged.  Returns the coarse index's elements (those beyond `coarse_cap`, and entries beyond `entry_cap`, are not
// written); -1 for a batch the call would refuse or a format without granules.
extern "C" int32_t dxtlt_debug_plan_batch_granules(const DxtltBatchItem* items, size_t count, int32_t format, int32_t inverse,
                                                   uint32_t* first_wg_out, uint64_t* main_blocks_out, size_t entry_cap, uint32_t* coarse_out,
                                                   size_t coarse_cap)
{
    BatchPlan plan;
    if (!dxtlt::granule::is_granule_format(format) || plan_batch(items, count, false, plan) != kOk)
        return -1;
    std::vector<uint8_t> tables(plan.table_bytes);
    fill_tables(plan, tables.data());
    const GranuleLaunch& p = plan.granules[(format == 7 ? 0 : 2) + (inverse != 0 ? 1 : 0)];
    if (p.bytes == 0)
        return 0;
    const GranuleEntry* entries = reinterpret_cast<const GranuleEntry*>(tables.data() + p.at);
    const uint32_t* coarse = reinterpret_cast<const uint32_t*>(tables.data() + p.at + p.entry_bytes + p.tail_bytes);
    for (size_t k = 0; k < p.entries.size() && k < entry_cap; ++k) {
        if (first_wg_out) first_wg_out[k] = entries[k].first_wg;
        if (main_blocks_out) main_blocks_out[k] = entries[k].main_blocks;
    }
    for (size_t k = 0; k < p.coarse.size() && k < coarse_cap && coarse_out != nullptr; ++k)
        coarse_out[k] = coarse[k];
    return (int32_t)p.coarse.size();
}
