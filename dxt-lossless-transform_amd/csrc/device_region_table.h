// device_region_table.h -- the region table of a batch entry as it lies in DEVICE memory (image_batch_launch.h: one 64-byte
// ImageBatchRegion per region), for the lookups of image_regions.h.  Device code, shared by the batch image kernels of BC1 - BC5
// (image_batch_kernels.hip) and of BC7 (bc7_image_batch_kernels.hip).
//
// The table's address comes out of the entry in scalar registers, so the wave-first lookup (region_of_run) stays what it is in
// the single-buffer kernels: scalar loads and scalar comparisons.  The table is read through the constant address space -- global
// memory nothing writes while the kernel runs -- which is what lets the compiler keep every read of it whose address is uniform on
// the scalar unit, also behind a barrier; the loop counter is the only index (image_regions.h: no per-lane indexing, no unrolled
// walks, nothing in scratch memory).
#pragma once
#include <cstddef>

#include "bcn_device.h"
#include "image_batch_launch.h"

namespace dxtlt {
namespace {

typedef const __attribute__((address_space(4))) uint64_t* const_qwords;
typedef const __attribute__((address_space(4))) uint32_t* const_dwords;

// The table of an entry for the lookups of image_regions.h: `at` = the address of its first ImageBatchRegion, uniform
struct DeviceRegionTable {
    uint64_t at;
    uint32_t count;

    __device__ __forceinline__ const_qwords qwords(uint32_t i) const { return (const_qwords)(at + (uint64_t)i * sizeof(ImageBatchRegion)); }
    __device__ __forceinline__ uint32_t regions() const { return count; }
    __device__ __forceinline__ uint64_t first_of(uint32_t i) const { return qwords(i)[0]; }
    __device__ __forceinline__ uint64_t blocks_of(uint32_t i) const { return qwords(i)[1]; }
    __device__ __forceinline__ ImageSink image_of(uint32_t i) const
    {
        const const_qwords q = qwords(i);
        const const_dwords w = (const_dwords)q;
        // (the pixel pointer is tagged as global memory: a pointer that was loaded from memory is a generic one to the compiler)
        return ImageSink{(uint8_t*)(global_ptr)q[2], q[3], q[4], w[10], w[11], w[12]};
    }
};
static_assert(offsetof(ImageBatchRegion, first) == 0 && offsetof(ImageBatchRegion, blocks) == 8 && offsetof(ImageBatchRegion, pixels) == 16 &&
                  offsetof(ImageBatchRegion, pitch) == 24 && offsetof(ImageBatchRegion, blocks_per_row) == 32 &&
                  offsetof(ImageBatchRegion, width) == 40 && offsetof(ImageBatchRegion, height) == 44 && offsetof(ImageBatchRegion, bpp) == 48,
              "DeviceRegionTable reads ImageBatchRegion by qword and dword offsets");

}  // namespace
}  // namespace dxtlt
