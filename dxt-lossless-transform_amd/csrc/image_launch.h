// image_launch.h -- internal launch interface of the image decoders (image_kernels.hip) for image_api.cpp.
#pragma once
#include "bcn_launch.h"
#include "image_sink.h"

namespace dxtlt {

// fmt = 1, 2, 3.  Both enqueue on `stream` only, allocate nothing and do not synchronise.
// blocks: ceil(width / 4) * ceil(height / 4) blocks in block order, any alignment
hipError_t launch_decode_image(int fmt, const void* blocks, const ImageSink& img, hipStream_t stream);
// soa: byte 0 of a transformed buffer of `total_blocks`; the image is its blocks [first_block, first_block + image blocks)
hipError_t launch_untransform_decode_image(Format fmt, const Settings& s, const void* soa, uint64_t total_blocks,
                                           uint64_t first_block, const ImageSink& img, hipStream_t stream);

}  // namespace dxtlt
