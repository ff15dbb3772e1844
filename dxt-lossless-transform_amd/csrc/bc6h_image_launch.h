// bc6h_image_launch.h -- internal launch interface of the BC6H decoders (bc6h_image_kernels.hip, bc6h_image_regions_kernels.hip) for
// bc6h_image_api.cpp.  Every call enqueues on `stream` only, allocates nothing and does not synchronise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_regions.h"
#include "image_sink.h"

namespace dxtlt {
namespace bc6h {

// blocks in block order, any alignment -> one 128-byte record per block
hipError_t launch_decode_blocks(const void* blocks, void* pixels, uint64_t num_blocks, hipStream_t stream);
// blocks: ceil(width / 4) * ceil(height / 4) blocks in block order, any alignment -> an RGBA16F image (img.bpp == 8)
hipError_t launch_decode_image(const void* blocks, const ImageSink& img, hipStream_t stream);
// soa: byte 0 of a transformed buffer of `total_blocks`; the image is its blocks [first_block, first_block + image blocks), any
// first_block
hipError_t launch_untransform_decode_image(const void* soa, uint64_t total_blocks, uint64_t first_block, const ImageSink& img,
                                           hipStream_t stream);

// Several images of one buffer (bc6h_image_regions_kernels.hip): `tab` holds 1 .. kImageRegionsPerLaunch non-empty RGBA16F regions
// inside [0, total_blocks), ascending and disjoint (append_region).  `blocks` / `soa`: byte 0 of the whole block array /
// transformed buffer.  The fused call goes out as granule::for_each_range_launch (granule_launch.h) plans the range that covers the
// regions.
hipError_t launch_decode_image_regions(const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream);
hipError_t launch_untransform_decode_image_regions(const void* soa, uint64_t total_blocks, const ImageRegionTable& tab,
                                                   hipStream_t stream);

}  // namespace bc6h
}  // namespace dxtlt
