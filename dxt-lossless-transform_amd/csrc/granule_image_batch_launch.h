// granule_image_batch_launch.h -- the tables of the batch image calls of the two granule-sorted formats
// (dxtlt_untransform_decode_bc7_images_batch_device, include/dxtlt_bc7_image.h; dxtlt_untransform_decode_bc6h_images_batch_device,
// include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "Many BC7 buffers in one call" and "Many BC6H buffers in one call"), shared by
// granule_image_batch_api.h, which fills them, and the two formats' kernels (bc7_image_batch_kernels.hip,
// bc6h_image_batch_kernels.hip), which read them.  Each format's launcher is declared in its own header
// (bc7_image_batch_launch.h, bc6h_image_batch_launch.h).  Host and device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_batch_launch.h"   // ImageBatchRegion: the region tables are the generic batch call's

namespace dxtlt {
namespace granule {

// One entry per group of at most kImageRegionsPerLaunch regions of an item, once in each table it has work in.
//   granule table   `granules` workgroups from first_wg on: workgroup b runs granule first_granule + b - first_wg of the main
//                   part (main_blocks blocks, src = byte 0 of the whole transformed buffer); ascending first_wg.
//   tail table      one workgroup: src = the tail part's byte 0, `tail` its blocks, main_blocks its first block.
// One 64-byte record on a 64-byte address, read with scalar loads only.
struct ImageBatchEntry {
    const uint8_t* src;
    const ImageBatchRegion* regions;   // device memory, on a 64-byte address: region_count records
    uint64_t main_blocks;
    uint64_t first_granule;            // granule table
    uint32_t first_wg;                 // granule table
    uint32_t region_count;             // 1 .. kImageRegionsPerLaunch
    uint32_t tail;                     // tail table: blocks of the tail part, 1 .. 1023
    uint32_t granules;                 // granule table: the entry's workgroups (the host's; the kernel does not read it)
    uint64_t reserved[2];
};
static_assert(sizeof(ImageBatchEntry) == 64, "ImageBatchEntry layout is shared between host and device: one cache line");

// Workgroups one launch may hold: fewer than 2^32 threads of 256-lane workgroups
constexpr uint64_t kMaxBatchWorkgroups = 0xFFFFFFull;

}  // namespace granule
}  // namespace dxtlt
