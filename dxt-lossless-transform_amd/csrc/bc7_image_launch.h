// bc7_image_launch.h -- internal launch interface of the BC7 decoders (bc7_image_kernels.hip, bc7_image_regions_kernels.hip) for
// bc7_image_api.cpp.  Every call enqueues on `stream` only, allocates nothing and does not synchronise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "bc7_fields.h"   // kGranule
#include "image_regions.h"
#include "image_sink.h"

namespace dxtlt {
namespace bc7 {

// blocks in block order, any alignment -> one 64-byte Decoded4x4Block per block
hipError_t launch_decode_blocks(const void* blocks, void* pixels, uint64_t num_blocks, hipStream_t stream);
// blocks: ceil(width / 4) * ceil(height / 4) blocks in block order, any alignment -> an RGBA8888 image
hipError_t launch_decode_image(const void* blocks, const ImageSink& img, hipStream_t stream);
// soa: byte 0 of a transformed buffer of `total_blocks`; the image is its blocks [first_block, first_block + image blocks), any
// first_block
hipError_t launch_untransform_decode_image(const void* soa, uint64_t total_blocks, uint64_t first_block, const ImageSink& img,
                                           hipStream_t stream);

// Several images of one buffer (bc7_image_regions_kernels.hip): `tab` holds 1 .. kImageRegionsPerLaunch non-empty RGBA8888 regions
// inside [0, total_blocks), ascending and disjoint (append_region).  `blocks` / `soa`: byte 0 of the whole block array /
// transformed buffer.  The fused call goes out as for_each_range_launch plans the range that covers the regions.
hipError_t launch_decode_image_regions(const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream);
hipError_t launch_untransform_decode_image_regions(const void* soa, uint64_t total_blocks, const ImageRegionTable& tab,
                                                   hipStream_t stream);

// The launches of the fused kernels over blocks [first, end), first < end <= total_blocks, of a transformed buffer, as
// launch_untransform_decode_image plans one image: one launch over the main part's granules first / 1024 ..
// (min(end, main_blocks) - 1) / 1024, split at 2^21 granules (granule_sort.h), then the tail part's launch if the range reaches
// it.  launch(first granule, granules, tail) enqueues one; the tail part is granule main_blocks / 1024.  Host arithmetic only.
template <typename LAUNCH>
hipError_t for_each_range_launch(uint64_t total_blocks, uint64_t first, uint64_t end, const LAUNCH& launch)
{
    constexpr uint64_t kT = kGranule, kMaxGranules = 1ull << 21;
    const uint64_t main_blocks = total_blocks - total_blocks % kT;
    if (first < main_blocks) {
        const uint64_t g0 = first / kT, g1 = ((end < main_blocks ? end : main_blocks) - 1) / kT;
        for (uint64_t g = g0; g <= g1; g += kMaxGranules) {
            const uint64_t ng = g1 + 1 - g < kMaxGranules ? g1 + 1 - g : kMaxGranules;
            if (hipError_t e = launch(g, ng, false); e != hipSuccess)
                return e;
        }
    }
    return end > main_blocks ? launch(main_blocks / kT, (uint64_t)1, true) : hipSuccess;
}

}  // namespace bc7
}  // namespace dxtlt
