// bc6h_image_batch_launch.h -- the launch interface of the BC6H batch image call (bc6h_image_batch_kernels.hip;
// include/dxtlt_bc6h_image.h, dxtlt_untransform_decode_bc6h_images_batch_device; docs/IMAGE_DECODE.md, "Many BC6H buffers in one
// call") for bc6h_image_batch_api.cpp.  The tables are granule_image_batch_launch.h's, which BC7 shares.  Host and device code.
#pragma once
#include "granule_image_batch_launch.h"

namespace dxtlt {
namespace bc6h {

using granule::ImageBatchEntry;
using granule::kMaxBatchWorkgroups;

// d_entries: n_entries granule entries, granule_wgs workgroups in all; d_coarse[k] = the entry that owns workgroup 64 k;
// d_tails: n_tails tail entries.  At most two launches on `stream`; a table without work is not launched.
hipError_t launch_image_batch(const ImageBatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries, uint32_t granule_wgs,
                              const ImageBatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);

}  // namespace bc6h
}  // namespace dxtlt
