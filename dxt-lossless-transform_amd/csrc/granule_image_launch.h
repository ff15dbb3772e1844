// granule_image_launch.h -- internal launch interface of the image decoders of the two granule-sorted formats, BC7 -> RGBA8888 and
// BC6H -> RGBA16F, for bc7_image_api.cpp and bc6h_image_api.cpp (through granule_image_api.h).  The launchers are written once, over
// a format's image family F (granule_image.h); bc7_image_kernels.hip and bc6h_image_kernels.hip instantiate them for their family,
// named here so that a caller can say which.  Every call enqueues on `stream` only, allocates nothing and does not synchronise.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_regions.h"
#include "image_sink.h"

namespace dxtlt {

namespace bc7 {
struct Bc7Image;    // bc7_image_sinks.h: 64 bytes per decoded block, img.bpp == 4
// blocks in block order, any alignment -> one 64-byte Decoded4x4Block per block
hipError_t launch_decode_blocks(const void* blocks, void* pixels, uint64_t num_blocks, hipStream_t stream);
}  // namespace bc7
namespace bc6h {
struct Bc6hImage;   // bc6h_image_sinks.h: 128 bytes per decoded block, img.bpp == 8
// blocks in block order, any alignment -> one 128-byte record per block
hipError_t launch_decode_blocks(const void* blocks, void* pixels, uint64_t num_blocks, hipStream_t stream);
}  // namespace bc6h

// blocks: ceil(width / 4) * ceil(height / 4) blocks in block order, any alignment -> the family's image
template <typename F>
hipError_t launch_decode_image(const void* blocks, const ImageSink& img, hipStream_t stream);
// soa: byte 0 of a transformed buffer of `total_blocks`; the image is its blocks [first_block, first_block + image blocks), any
// first_block
template <typename F>
hipError_t launch_untransform_decode_image(const void* soa, uint64_t total_blocks, uint64_t first_block, const ImageSink& img,
                                           hipStream_t stream);

// Several images of one buffer: `tab` holds 1 .. kImageRegionsPerLaunch non-empty regions of the family's pixels inside
// [0, total_blocks), ascending and disjoint (append_region).  `blocks` / `soa`: byte 0 of the whole block array / transformed
// buffer.  The fused calls go out as granule::for_each_range_launch (granule_launch.h) plans the range that covers the image or
// the regions.
template <typename F>
hipError_t launch_decode_image_regions(const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream);
template <typename F>
hipError_t launch_untransform_decode_image_regions(const void* soa, uint64_t total_blocks, const ImageRegionTable& tab,
                                                   hipStream_t stream);

}  // namespace dxtlt
