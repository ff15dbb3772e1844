// image_region_groups.h -- how the image-region calls (image_api.cpp: BC1 - BC5; bc7_image_api.cpp: BC7; bc6h_image_api.cpp: BC6H;
// all through image_host.h, which also checks the list) walk their region list: host code beside image_regions.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/dxtlt_image.h"
#include "image_regions.h"

namespace dxtlt_host {

inline bool empty_region(const DxtltImageRegion& r) { return r.width == 0 || r.height == 0; }

// The non-empty regions in groups of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH consecutive ones: sink_of(i) is region i's image,
// launch(table) enqueues one group
template <typename SINK_OF, typename LAUNCH>
inline hipError_t for_each_region_group(const DxtltImageRegion* regions, size_t count, const SINK_OF& sink_of, const LAUNCH& launch)
{
    static_assert(DXTLT_IMAGE_REGIONS_PER_LAUNCH == dxtlt::kImageRegionsPerLaunch, "the header's constant is the kernels'");
    dxtlt::ImageRegionTable tab;
    dxtlt::clear_regions(tab);
    for (size_t i = 0; i < count; ++i) {
        if (empty_region(regions[i]))
            continue;
        dxtlt::append_region(tab, sink_of(i), regions[i].first_block);
        if (tab.count == (uint32_t)dxtlt::kImageRegionsPerLaunch) {
            if (hipError_t e = launch(tab); e != hipSuccess)
                return e;
            dxtlt::clear_regions(tab);
        }
    }
    return tab.count != 0 ? launch(tab) : hipSuccess;
}

}  // namespace dxtlt_host
