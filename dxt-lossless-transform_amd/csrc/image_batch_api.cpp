// image_batch_api.cpp -- dxtlt_untransform_decode_images_batch_device (include/dxtlt_image.h; docs/IMAGE_DECODE.md, "Many buffers
// in one call"): the images of many transformed device buffers in one launch per (format, settings) present in the batch.
//
// Planning is pure host arithmetic (plan_image_batch; dxtlt_debug_plan_image_batch exposes it to the tests on a machine without a
// GPU): every item is checked as the single call checks it (image_regions_defect, image_host.h); its non-empty regions are cut
// into groups of at most sixteen, each group one entry -- the inverse transform's plan for the range from the group's first block to the end of its last region
// (plan_image_batch_entry) and the group's region table; entries of one format and settings share a launch.  The call then
// stages every table of the batch -- region tables, entries, workgroup indexes -- in ONE slot of the batch calls' ring
// (StagedTables, batch_tables.h) and uploads it on the caller's stream in front of the launches, as dxtlt_transform_batch_device does.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_gfx950.h"
#include "../../include/dxtlt_image.h"
#include "batch_tables.h"
#include "host_common.h"
#include "image_batch_launch.h"
#include "image_host.h"
#include "image_launch.h"

namespace {

using namespace dxtlt_host;
using dxtlt::ImageBatchEntry;
using dxtlt::ImageBatchRegion;


// One entry: a group of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH non-empty regions of an item
struct PlannedEntry {
    uint32_t item, first_region, region_count;
    int launch;           // index into ImageBatchPlan::launches; -1: alone, through the single call's kernels
    size_t regions_at;    // of its first region in ImageBatchPlan::regions
    ImageBatchEntry entry;
};

struct PlannedLaunch {
    int key;              // (format - 1) << 4 | mode << 2 | alpha split << 1 | colour split, the format's effective settings
    std::vector<size_t> entries;   // indices into ImageBatchPlan::entries, in item order
    uint32_t wgs = 0;
};

struct ImageBatchPlan {
    std::vector<PlannedEntry> entries;        // in list order
    std::vector<ImageBatchRegion> regions;    // of all entries, in list order
    std::vector<PlannedLaunch> launches;      // in the order in which their settings first appear
};

inline dxtlt::Format key_format(int key) { return (dxtlt::Format)((key >> 4) + 1); }

int32_t fail_item(size_t i, const char* why)
{
    char text[224];
    std::snprintf(text, sizeof text, "image batch item %zu: %s", i, why);
    return fail(kInvalidArgument, text);
}

// Validates the batch as a whole and plans it; nothing is enqueued, no device is touched, no address is dereferenced.
int32_t plan_image_batch(const DxtltImageBatchItem* items, size_t count, ImageBatchPlan& plan)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    static_assert(DXTLT_IMAGE_REGIONS_PER_LAUNCH == dxtlt::kImageRegionsPerLaunch, "the header's constant is the kernels'");
    int launch_of_key[5 * 16];
    for (int& l : launch_of_key)
        l = -1;
    for (size_t i = 0; i < count; ++i) {
        const DxtltImageBatchItem& it = items[i];
        bool nothing = true;
        if (const char* why = image_regions_defect(it.format, it.d_transformed, it.total_blocks, it.regions, it.region_count,
                                                   it.decorrelation_mode, &nothing))
            return fail_item(i, why);
        if (nothing)
            continue;
        const dxtlt::Format fmt = (dxtlt::Format)it.format;
        dxtlt::Settings s{};
        s.variant = it.decorrelation_mode;
        s.split_alpha = it.split_alpha_endpoints != 0;
        s.split_colour = it.split_colour_endpoints != 0;
        s = dxtlt::effective_settings(fmt, s);
        const int key = ((it.format - 1) << 4) | settings_code(s);
        const uint32_t bpp = pixel_rule(it.format).bpp;
        for (uint32_t r = 0; r < it.region_count;) {
            // the next group: up to sixteen non-empty regions from region r on
            PlannedEntry pe{};
            pe.item = (uint32_t)i;
            pe.regions_at = plan.regions.size();
            uint64_t end = 0;
            for (; r < it.region_count && pe.region_count < (uint32_t)dxtlt::kImageRegionsPerLaunch; ++r) {
                const DxtltImageRegion& reg = it.regions[r];
                if (empty_region(reg))
                    continue;
                if (pe.region_count == 0)
                    pe.first_region = r;
                const dxtlt::ImageSink img = dxtlt::make_image_sink(reg.pixels, reg.pitch, reg.width, reg.height, bpp);
                plan.regions.push_back(dxtlt::make_batch_region(img, reg.first_block));
                end = reg.first_block + dxtlt::image_blocks(img);
                ++pe.region_count;
            }
            if (pe.region_count == 0)
                break;   // only empty regions were left
            ImageBatchEntry& e = pe.entry;
            e.src = static_cast<const uint8_t*>(it.d_transformed);
            e.regions = nullptr;   // known once the tables have their place in device memory
            e.total_blocks = it.total_blocks;
            e.region_count = (uint8_t)pe.region_count;
            e.first_block = plan.regions[pe.regions_at].first;
            e.range_blocks = end - e.first_block;
            int li = launch_of_key[key];
            e.first_wg = li >= 0 ? plan.launches[(size_t)li].wgs : 0;
            const uint32_t wgs = dxtlt::plan_image_batch_entry(fmt, s, e);
            if (wgs == 0xFFFFFFFFu) {
                pe.launch = -1;
                e.first_wg = e.end_wg = 0;
                plan.entries.push_back(pe);
                continue;
            }
            if (li < 0) {
                li = launch_of_key[key] = (int)plan.launches.size();
                plan.launches.push_back(PlannedLaunch{key, {}, 0});
            }
            PlannedLaunch& l = plan.launches[(size_t)li];
            // one launch holds fewer than 2^32 threads = 2^24 workgroups of 256 lanes, one tile each
            if ((uint64_t)l.wgs + wgs > 0xFFFFFFull)
                return fail_item(i, "batch too large for one launch: one format and settings may take at most 16777215 tiles "
                                    "(a tile is 512 BC1 / BC4 blocks or 256 blocks of the other formats)");
            l.wgs += wgs;
            pe.launch = li;
            l.entries.push_back(plan.entries.size());
            plan.entries.push_back(pe);
        }
    }
    return kOk;
}

// the kernel-argument table of an entry that goes out alone
dxtlt::ImageRegionTable alone_table(const ImageBatchPlan& plan, const PlannedEntry& pe)
{
    dxtlt::ImageRegionTable tab;
    dxtlt::clear_regions(tab);
    for (uint32_t k = 0; k < pe.region_count; ++k) {
        const ImageBatchRegion& r = plan.regions[pe.regions_at + k];
        dxtlt::append_region(tab, dxtlt::ImageSink{reinterpret_cast<uint8_t*>(static_cast<uintptr_t>(r.pixels)), r.pitch, r.blocks_per_row,
                                                   r.width, r.height, r.bpp},
                             r.first);
    }
    return tab;
}

// The workgroup index of a launch (batch_index_bytes(l.wgs) bytes at `index`); true when it has the wide form.  `spans`: scratch,
// the first_wg / end_wg of the launch's entries for build_batch_index
bool build_launch_index(const ImageBatchPlan& plan, const PlannedLaunch& l, std::vector<dxtlt::BatchEntry>& spans, uint8_t* index)
{
    spans.assign(l.entries.size(), dxtlt::BatchEntry{});
    for (size_t j = 0; j < l.entries.size(); ++j) {
        spans[j].first_wg = plan.entries[l.entries[j]].entry.first_wg;
        spans[j].end_wg = plan.entries[l.entries[j]].entry.end_wg;
    }
    return dxtlt::build_batch_index(spans.data(), spans.size(), l.wgs, index);
}

}  // namespace

extern "C" int32_t dxtlt_untransform_decode_images_batch_device(const DxtltImageBatchItem* items, size_t count, void* hip_stream)
{
    ImageBatchPlan plan;
    if (int32_t rc = plan_image_batch(items, count, plan); rc != kOk)
        return rc;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);

    // One staged buffer, one upload: the region tables of every batched entry (64-byte records on 64-byte addresses), then
    // per launch its entries (on a 128-byte address: an entry is two lines) and its workgroup index.
    if (!plan.launches.empty()) {
        const size_t region_bytes = plan.regions.size() * sizeof(ImageBatchRegion);
        size_t table_bytes = padded(region_bytes, 128);
        struct Placed {
            size_t at, entry_bytes;
        };
        std::vector<Placed> placed;
        for (const PlannedLaunch& l : plan.launches) {
            const size_t entry_bytes = l.entries.size() * sizeof(ImageBatchEntry);
            placed.push_back({table_bytes, entry_bytes});
            table_bytes += padded(entry_bytes + dxtlt::batch_index_bytes(l.wgs), 128);
        }
        StagedTables tables;
        hipError_t e = tables.acquire(table_bytes);
        if (e != hipSuccess)
            return fail(kDevice, "image batch table staging", e);
        uint8_t* host = tables.host();
        const uint8_t* dev = tables.dev();
        std::memcpy(host, plan.regions.data(), region_bytes);
        std::vector<bool> wide(plan.launches.size());
        std::vector<dxtlt::BatchEntry> spans;
        for (size_t k = 0; k < plan.launches.size(); ++k) {
            const PlannedLaunch& l = plan.launches[k];
            ImageBatchEntry* out = reinterpret_cast<ImageBatchEntry*>(host + placed[k].at);
            for (size_t j = 0; j < l.entries.size(); ++j) {
                const PlannedEntry& pe = plan.entries[l.entries[j]];
                out[j] = pe.entry;
                out[j].regions = reinterpret_cast<const ImageBatchRegion*>(dev) + pe.regions_at;
            }
            wide[k] = build_launch_index(plan, l, spans, host + placed[k].at + placed[k].entry_bytes);
        }
        e = tables.upload(user);
        for (size_t k = 0; k < plan.launches.size() && e == hipSuccess; ++k) {
            const PlannedLaunch& l = plan.launches[k];
            const uint8_t* d = dev + placed[k].at;
            e = dxtlt::launch_image_batch(key_format(l.key), settings_of_code(l.key & 15), reinterpret_cast<const ImageBatchEntry*>(d),
                                          d + placed[k].entry_bytes, (uint32_t)l.entries.size(), l.wgs, wide[k], user);
        }
        if (int32_t rc = tables.finish(e, user, "image batch table upload / launch", "image batch event"); rc != kOk)
            return rc;
    }
    // entries the batch kernel does not take: the single call's kernels, one group each, behind the batch launches
    for (const PlannedEntry& pe : plan.entries) {
        if (pe.launch >= 0)
            continue;
        const DxtltImageBatchItem& it = items[pe.item];
        const dxtlt::Settings s{it.decorrelation_mode, it.split_alpha_endpoints != 0, it.split_colour_endpoints != 0};
        HIP_TRY(dxtlt::launch_untransform_decode_image_regions((dxtlt::Format)it.format, s, it.d_transformed, it.total_blocks,
                                                               alone_table(plan, pe), user),
                "image batch item launch");
    }
    return kOk;
}

extern "C" int32_t dxtlt_debug_plan_image_batch(const DxtltImageBatchItem* items, size_t count, DxtltDebugImageBatchEntry* out, size_t cap)
{
    ImageBatchPlan plan;
    if (plan_image_batch(items, count, plan) != kOk)
        return -1;
    // the form of every launch's index, as the call would build it
    std::vector<uint32_t> wide(plan.launches.size(), 0);
    std::vector<dxtlt::BatchEntry> spans;
    std::vector<uint8_t> index;
    for (size_t k = 0; k < plan.launches.size(); ++k) {
        const PlannedLaunch& l = plan.launches[k];
        index.assign(dxtlt::batch_index_bytes(l.wgs), 0);
        wide[k] = build_launch_index(plan, l, spans, index.data()) ? 1 : 0;
    }
    for (size_t k = 0; k < plan.entries.size() && k < cap && out != nullptr; ++k) {
        const PlannedEntry& pe = plan.entries[k];
        DxtltDebugImageBatchEntry& o = out[k];
        o.item = pe.item;
        o.first_region = pe.first_region;
        o.region_count = pe.region_count;
        o.launch = pe.launch;
        o.first_wg = pe.entry.first_wg;
        o.end_wg = pe.entry.end_wg;
        o.full_tiles = pe.entry.full_tiles;
        o.form = pe.entry.form;
        o.first_block = pe.entry.first_block;
        o.range_blocks = pe.entry.range_blocks;
        o.wide_index = pe.launch >= 0 ? wide[(size_t)pe.launch] : 0;
        o.launch_wgs = pe.launch >= 0 ? plan.launches[(size_t)pe.launch].wgs : 0;
    }
    return (int32_t)plan.entries.size();
}
