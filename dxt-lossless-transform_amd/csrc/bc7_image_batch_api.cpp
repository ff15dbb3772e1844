// bc7_image_batch_api.cpp -- dxtlt_untransform_decode_bc7_images_batch_device (include/dxtlt_bc7_image.h; docs/IMAGE_DECODE.md,
// "Many BC7 buffers in one call"): the images of many BC7 transformed device buffers in at most two launches.
//
// Planning is pure host arithmetic (plan_batch; dxtlt_debug_plan_bc7_image_batch exposes it to the tests on a machine without a
// GPU): every item is checked as dxtlt_untransform_decode_bc7_images_device checks it (image_regions_defect, image_host.h); its
// non-empty regions are cut into the single call's groups (for_each_region_group), each group one entry whose covering range is
// planned as the single call plans it (for_each_range_launch, granule_launch.h): the main part's granules it touches go into the
// granule launch, its tail part, if it reaches one, into the tail launch.  The call then stages every table of the batch -- region tables, granule
// entries, tail entries, the coarse index (build_coarse_index) -- in ONE slot of the batch calls' ring (StagedTables,
// batch_tables.h) and uploads it on the caller's stream in front of the launches, as image_batch_api.cpp does.
#include <hip/hip_runtime_api.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_bc7_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "batch_tables.h"
#include "bc7_image_batch_launch.h"
#include "granule_launch.h"   // for_each_range_launch
#include "host_common.h"
#include "image_host.h"       // image_regions_defect

namespace {

using namespace dxtlt_host;
using dxtlt::ImageBatchRegion;
using dxtlt::bc7::ImageBatchEntry;
using dxtlt::bc7::kMaxBatchWorkgroups;

// One entry: a group of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH non-empty regions of an item
struct PlannedEntry {
    uint32_t item, first_region, region_count;
    size_t regions_at;        // of its first region in Bc7ImageBatchPlan::regions
    uint64_t first_granule;
    uint32_t granules;        // workgroups in the granule launch, 0 if none
    uint32_t first_wg;
    int32_t tail_index;       // workgroup in the tail launch, or -1
};

struct Bc7ImageBatchPlan {
    std::vector<PlannedEntry> entries;       // in list order
    std::vector<ImageBatchRegion> regions;   // of all entries, in list order
    uint32_t granule_wgs = 0, tail_wgs = 0;
};

int32_t fail_item(size_t i, const char* why)
{
    char text[224];
    std::snprintf(text, sizeof text, "bc7 image batch item %zu: %s", i, why);
    return fail(kInvalidArgument, text);
}

// Validates the batch as a whole and plans it; nothing is enqueued, no device is touched, no address is dereferenced.
int32_t plan_batch(const DxtltBc7ImageBatchItem* items, size_t count, Bc7ImageBatchPlan& plan)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    for (size_t i = 0; i < count; ++i) {
        const DxtltBc7ImageBatchItem& it = items[i];
        bool nothing = true;
        if (const char* why = image_regions_defect(kRgba8888, it.d_transformed, it.total_blocks, it.regions, it.region_count, &nothing))
            return fail_item(i, why);
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
                return dxtlt::make_image_sink(reg.pixels, reg.pitch, reg.width, reg.height);
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
            return fail_item(i, too_large != nullptr ? too_large : "the regions are not a list the kernels take");
    }
    return kOk;
}

}  // namespace

extern "C" int32_t dxtlt_untransform_decode_bc7_images_batch_device(const DxtltBc7ImageBatchItem* items, size_t count, void* hip_stream)
{
    Bc7ImageBatchPlan plan;
    if (int32_t rc = plan_batch(items, count, plan); rc != kOk)
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
        return fail(kDevice, "bc7 image batch table staging", e);
    uint8_t* host = tables.host();
    const uint8_t* dev = tables.dev();
    std::memcpy(host, plan.regions.data(), region_bytes);
    ImageBatchEntry* granule_entries = reinterpret_cast<ImageBatchEntry*>(host + entries_at);
    ImageBatchEntry* tail_entries = reinterpret_cast<ImageBatchEntry*>(host + tails_at);
    size_t at = 0;
    for (const PlannedEntry& pe : plan.entries) {
        const DxtltBc7ImageBatchItem& it = items[pe.item];
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
        e = dxtlt::bc7::launch_image_batch(reinterpret_cast<const ImageBatchEntry*>(dev + entries_at),
                                           reinterpret_cast<const uint32_t*>(dev + coarse_at), (uint32_t)n_granule_entries, plan.granule_wgs,
                                           reinterpret_cast<const ImageBatchEntry*>(dev + tails_at), plan.tail_wgs, user);
    return tables.finish(e, user, "bc7 image batch table upload / launch", "bc7 image batch event");
}

extern "C" int32_t dxtlt_debug_plan_bc7_image_batch(const DxtltBc7ImageBatchItem* items, size_t count, DxtltDebugBc7ImageBatchEntry* out,
                                                    size_t cap)
{
    Bc7ImageBatchPlan plan;
    if (plan_batch(items, count, plan) != kOk)
        return -1;
    for (size_t k = 0; k < plan.entries.size() && k < cap && out != nullptr; ++k) {
        const PlannedEntry& pe = plan.entries[k];
        out[k] = DxtltDebugBc7ImageBatchEntry{pe.item,     pe.first_region, pe.region_count,  pe.tail_index, pe.first_granule,
                                              pe.granules, pe.first_wg,     plan.granule_wgs, plan.tail_wgs};
    }
    return (int32_t)plan.entries.size();
}
