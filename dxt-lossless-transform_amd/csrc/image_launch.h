// image_launch.h -- internal launch interface of the image decoders (image_kernels.hip, image_regions_kernels.hip) for image_api.cpp
// and image_batch_api.cpp: kernel launches only; the calls' argument checks are image_host.h's.
#pragma once
#include "bcn_launch.h"
#include "image_regions.h"
#include "image_sink.h"

namespace dxtlt {

// fmt = 1, 2, 3 and an RGBA8888 image.  Both enqueue on `stream` only, allocate nothing and do not synchronise.
// blocks: ceil(width / 4) * ceil(height / 4) blocks in block order, any alignment
hipError_t launch_decode_image(int fmt, const void* blocks, const ImageSink& img, hipStream_t stream);
// soa: byte 0 of a transformed buffer of `total_blocks`; the image is its blocks [first_block, first_block + image blocks)
hipError_t launch_untransform_decode_image(Format fmt, const Settings& s, const void* soa, uint64_t total_blocks,
                                           uint64_t first_block, const ImageSink& img, hipStream_t stream);

// The same for fmt = 4, 5 and an image of 1 / 2 bytes per pixel (img.bpp); one setting, split_endpoints
hipError_t launch_decode_channel_image(int fmt, const void* blocks, const ImageSink& img, hipStream_t stream);
hipError_t launch_untransform_decode_channel_image(Format fmt, bool split_endpoints, const void* soa, uint64_t total_blocks,
                                                   uint64_t first_block, const ImageSink& img, hipStream_t stream);

// Several images of one buffer (image_regions_kernels.hip), fmt = 1 .. 5 and images of 4, 4, 4, 1, 2 bytes per pixel: `tab` holds
// 1 .. kImageRegionsPerLaunch non-empty regions inside [0, total_blocks), ascending and disjoint (append_region); one plan over
// the range that covers them.  `blocks` / `soa`: byte 0 of the whole block array / transformed buffer.
hipError_t launch_decode_image_regions(int fmt, const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab,
                                       hipStream_t stream);
hipError_t launch_untransform_decode_image_regions(Format fmt, const Settings& s, const void* soa, uint64_t total_blocks,
                                                   const ImageRegionTable& tab, hipStream_t stream);

}  // namespace dxtlt
