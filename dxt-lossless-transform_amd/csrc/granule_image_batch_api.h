// granule_image_batch_api.h -- the bodies of the batch image calls of the two granule-sorted formats
// (dxtlt_untransform_decode_bc7_images_batch_device, include/dxtlt_bc7_image.h; dxtlt_untransform_decode_bc6h_images_batch_device,
// include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "Many BC7 buffers in one call" and "Many BC6H buffers in one call"): the images
// of many transformed device buffers in at most two launches, written once over a host-side family H; bc7_image_batch_api.cpp and
// bc6h_image_batch_api.cpp name their family and forward their two entry points to the bodies here.  A family holds
//   * rule: the PixelRule of its images (image_host.h);
//   * kName: the format's word in the error texts ("bc7", "bc6h");
//   * Item, DebugEntry: the public item and debug record (the two formats' are field for field the same);
//   * launch: the launcher of its two kernels over the tables of granule_image_batch_launch.h.
//
// Planning is pure host arithmetic (plan_batch; the debug hooks expose it to the tests on a machine without a GPU): every item is
// checked as the family's single call checks it (image_regions_defect, image_host.h); its non-empty regions are cut into the single
// call's groups (for_each_region_group), each group one entry whose covering range is planned as the single call plans it
// (for_each_range_launch, granule_launch.h): the main part's granules it touches go into the granule launch, its tail part, if it
// reaches one, into the tail launch.  The call then stages every table of the batch -- region tables, granule entries, tail
// entries, the coarse index (build_coarse_index) -- in ONE slot of the batch calls' ring (StagedTables, batch_tables.h) and uploads
// it on the caller's stream in front of the launches, as image_batch_api.cpp does.  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "batch_tables.h"
#include "granule_image_batch_launch.h"
#include "granule_launch.h"   // for_each_range_launch
#include "host_common.h"
#include "image_host.h"       // image_regions_defect

namespace dxtlt_host {
namespace granule_image_batch {

using dxtlt::ImageBatchRegion;
using dxtlt::granule::ImageBatchEntry;
using dxtlt::granule::kMaxBatchWorkgroups;

// One entry: a group of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH non-empty regions of an item
struct PlannedEntry {
    uint32_t item, first_region, region_count;
    size_t regions_at;        // of its first region in Plan::regions
    uint64_t first_granule;
    uint32_t granules;        // workgroups in the granule launch, 0 if none
    uint32_t first_wg;
    int32_t tail_index;       // workgroup in the tail launch, or -1
};

struct Plan {
    std::vector<PlannedEntry> entries;       // in list order
    std::vector<ImageBatchRegion> regions;   // of all entries, in list order
    uint32_t granule_wgs = 0, tail_wgs = 0;
};

template <typename H>
int32_t fail_item(size_t i, const char* why)
{
    char text[224];
    std::snprintf(text, sizeof text, "%s image batch item %zu: %s", H::kName, i, why);
    return fail(kInvalidArgument, text);
}

// what went wrong on the device, with the family's name in front: "bc7 image batch table staging"
template <typename H>
int32_t fail_device(const char* what, hipError_t e)
{
    char text[96];
    std::snprintf(text, sizeof text, "%s image batch %s", H::kName, what);
    return fail(kDevice, text, e);
}

// Validates the batch as a whole and plans it; nothing is enqueued, no device is touched, no address is dereferenced.
template <typename H>
int32_t plan_batch(const typename H::Item* items, size_t count, Plan& plan)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    for (size_t i = 0; i < count; ++i) {
        const typename H::Item& it = items[i];
        bool nothing = true;
        if (const char* why = image_regions_defect(H::rule, it.d_transformed, it.total_blocks, it.regions, it.region_count, &nothing))
            return fail_item<H>(i, why);
        if (nothing)
            continue;
        // the single call's walk: the same groups, the same plan of each group's covering range, entries in the place of launches
        size_t group_first = 0;
        bool group_open = false;
        const char* too_large = nullptr;
        const hipError_t e = for_each_region_group(
            it.regions, it.region_count,
            [&](size_t r) {
                if (!group_open)
                    group_first = r, group_open = true;
                const DxtltImageRegion& reg = it.regions[r];
                return dxtlt::make_image_sink(reg.pixels, reg.pitch, reg.width, reg.height, H::rule.bpp);
            },
            [&](const dxtlt::ImageRegionTable& tab) {
                uint64_t first = 0, n = 0;
                if (!dxtlt::covering_range(tab, it.total_blocks, first, n))
                    return hipErrorInvalidValue;
                group_open = false;
                PlannedEntry pe{(uint32_t)i, (uint32_t)group_first, tab.count, plan.regions.size(), 0, 0, plan.granule_wgs, -1};
                for (uint32_t k = 0; k < tab.count; ++k)
                    plan.regions.push_back(dxtlt::make_batch_region(tab.img[k], tab.first[k]));
                uint64_t granules = 0;
                bool tail = false;
                (void)dxtlt::granule::for_each_range_launch(it.total_blocks, first, first + n, [&](uint64_t granule, uint64_t ng, bool is_tail) {
                    // (the single call's launches over the main part follow one another: one run of granules here)
                    if (is_tail)
                        tail = true;
                    else if (granules == 0)
                        pe.first_granule = granule, granules = ng;
                    else
                        granules += ng;
                    return hipSuccess;
                });
                // one launch holds fewer than 2^32 threads = 2^24 workgroups of 256 lanes
                if (plan.granule_wgs + granules > kMaxBatchWorkgroups || (tail && plan.tail_wgs + 1ull > kMaxBatchWorkgroups)) {
                    too_large = "batch too large for two launches: a call may take at most 16777215 granules (of 1024 blocks of a "
                                "main part) and at most 16777215 tail parts";
                    return hipErrorInvalidValue;
                }
                pe.granules = (uint32_t)granules;
                plan.granule_wgs += pe.granules;
                if (tail)
                    pe.tail_index = (int32_t)plan.tail_wgs++;
                plan.entries.push_back(pe);
                return hipSuccess;
            });
        if (e != hipSuccess)
            return fail_item<H>(i, too_large != nullptr ? too_large : "the regions are not a list the kernels take");
    }
    return kOk;
}

template <typename H>
int32_t untransform_decode_images_batch_device(const typename H::Item* items, size_t count, void* hip_stream)
{
    Plan plan;
    if (int32_t rc = plan_batch<H>(items, count, plan); rc != kOk)
        return rc;
    if (plan.entries.empty())
        return kOk;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);

    // One staged buffer, one upload: the region tables (64-byte records on 64-byte addresses), the granule entries in ascending
    // first_wg, the tail entries (64-byte records again) and the coarse index of the granule launch.
    size_t n_granule_entries = 0;
    for (const PlannedEntry& pe : plan.entries)
        n_granule_entries += pe.granules != 0 ? 1 : 0;
    const size_t region_bytes = plan.regions.size() * sizeof(ImageBatchRegion);
    const size_t entries_at = region_bytes, tails_at = entries_at + n_granule_entries * sizeof(ImageBatchEntry);
    const size_t coarse_at = tails_at + (size_t)plan.tail_wgs * sizeof(ImageBatchEntry);
    const size_t table_bytes = padded(coarse_at + coarse_index_count(plan.granule_wgs) * sizeof(uint32_t), 16);
    StagedTables tables;
    hipError_t e = tables.acquire(table_bytes);
    if (e != hipSuccess)
        return fail_device<H>("table staging", e);
    uint8_t* host = tables.host();
    const uint8_t* dev = tables.dev();
    std::memcpy(host, plan.regions.data(), region_bytes);
    ImageBatchEntry* granule_entries = reinterpret_cast<ImageBatchEntry*>(host + entries_at);
    ImageBatchEntry* tail_entries = reinterpret_cast<ImageBatchEntry*>(host + tails_at);
    size_t at = 0;
    for (const PlannedEntry& pe : plan.entries) {
        const typename H::Item& it = items[pe.item];
        const uint8_t* src = static_cast<const uint8_t*>(it.d_transformed);
        const uint64_t tail = it.total_blocks % 1024, main_blocks = it.total_blocks - tail;
        const ImageBatchRegion* regions = reinterpret_cast<const ImageBatchRegion*>(dev) + pe.regions_at;
        if (pe.granules != 0)
            granule_entries[at++] = ImageBatchEntry{src, regions, main_blocks, pe.first_granule, pe.first_wg, pe.region_count, 0, pe.granules, {0, 0}};
        if (pe.tail_index >= 0)
            tail_entries[pe.tail_index] = ImageBatchEntry{src + main_blocks * 16, regions, main_blocks, 0, 0, pe.region_count, (uint32_t)tail, 0, {0, 0}};
    }
    build_coarse_index(granule_entries, n_granule_entries, plan.granule_wgs, reinterpret_cast<uint32_t*>(host + coarse_at));
    e = tables.upload(user);
    if (e == hipSuccess)
        e = H::launch(reinterpret_cast<const ImageBatchEntry*>(dev + entries_at), reinterpret_cast<const uint32_t*>(dev + coarse_at),
                      (uint32_t)n_granule_entries, plan.granule_wgs, reinterpret_cast<const ImageBatchEntry*>(dev + tails_at), plan.tail_wgs,
                      user);
    char what_launch[96], what_event[96];
    std::snprintf(what_launch, sizeof what_launch, "%s image batch table upload / launch", H::kName);
    std::snprintf(what_event, sizeof what_event, "%s image batch event", H::kName);
    return tables.finish(e, user, what_launch, what_event);
}

// The entries the call would stage, in list order, as H::DebugEntry records; records beyond `cap` are counted, not written.
// Returns the number of entries, or -1 for a batch the call would refuse.
template <typename H>
int32_t debug_plan(const typename H::Item* items, size_t count, typename H::DebugEntry* out, size_t cap)
{
    Plan plan;
    if (plan_batch<H>(items, count, plan) != kOk)
        return -1;
    for (size_t k = 0; k < plan.entries.size() && k < cap && out != nullptr; ++k) {
        const PlannedEntry& pe = plan.entries[k];
        out[k] = typename H::DebugEntry{pe.item,     pe.first_region, pe.region_count,  pe.tail_index, pe.first_granule,
                                        pe.granules, pe.first_wg,     plan.granule_wgs, plan.tail_wgs};
    }
    return (int32_t)plan.entries.size();
}

}  // namespace granule_image_batch
}  // namespace dxtlt_host
