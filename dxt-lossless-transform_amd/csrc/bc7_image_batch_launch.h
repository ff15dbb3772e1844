// bc7_image_batch_launch.h -- the tables of the BC7 batch image call (bc7_image_batch_kernels.hip; include/dxtlt_bc7_image.h,
// dxtlt_untransform_decode_bc7_images_batch_device; docs/IMAGE_DECODE.md, "Many BC7 buffers in one call") and its launch
// interface for bc7_image_batch_api.cpp.  Host and device code.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "image_batch_launch.h"   // ImageBatchRegion: the region tables are the generic batch call's

namespace dxtlt {
namespace bc7 {

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

// d_entries: n_entries granule entries, granule_wgs workgroups in all; d_coarse[k] = the entry that owns workgroup 64 k;
// d_tails: n_tails tail entries.  At most two launches on `stream`; a table without work is not launched.
hipError_t launch_image_batch(const ImageBatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries, uint32_t granule_wgs,
                              const ImageBatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);

}  // namespace bc7
}  // namespace dxtlt
