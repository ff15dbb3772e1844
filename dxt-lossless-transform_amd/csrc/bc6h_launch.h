// bc6h_launch.h -- internal launch interface of the BC6H granule-sorted field split, layout version 1
// (docs/BC6H_FORMAT.md).  The same calls as bc7_launch.h: the two formats share the granule, the streams and the batch
// table, and differ only in the record inside a block.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "bc7_launch.h"

namespace dxtlt {
namespace bc6h {

using BatchEntry = bc7::BatchEntry;

hipError_t launch(bool inverse, const void* src, void* dst, uint64_t n_blocks, hipStream_t stream);
hipError_t launch_range(bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block,
                        uint64_t num_blocks, hipStream_t stream);
hipError_t launch_batch(bool inverse, const BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);

}  // namespace bc6h
}  // namespace dxtlt
