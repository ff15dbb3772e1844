// bc6h_image_batch_kernels.hip -- the RGBA16F images of MANY BC6H transformed buffers in at most two launches on gfx950
// (dxtlt_untransform_decode_bc6h_images_batch_device, include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "Many BC6H buffers in one
// call").
//
// The shape of bc7_image_batch_kernels.hip: the lookup of the batch untransform in front of the fused kernels of one buffer
// (inverse_images, granule_image.h).  Workgroup b of the granule launch finds its entry -- a group of up to sixteen regions of one
// buffer -- through coarse[b / 64] and a short scan, and un-sorts and decodes ONE granule of that buffer's main part; the tail
// launch has one workgroup per entry whose range reaches its buffer's tail part.  Each block's pixels go to whichever region of
// the entry's table owns the block (Bc6hRegionPixelSinkOf, bc6h_image_sinks.h).  The table lies in device memory beside the
// entries (DeviceRegionTable, device_region_table.h); its address and everything else of the entry come out of scalar loads, so
// the table is walked exactly as the kernel-argument table of the single-buffer kernels is: by the two loops of image_regions.h,
// with the loop counter as the only index, on the scalar unit.
// Unlike BC7 the two launches have two sink types, <DeviceRegionTable, false> and <DeviceRegionTable, true>: in a full granule
// lane l stores halves of blocks l / 2 and 32 + l / 2 of its wave's run, in the tail part its own block.  The sink's rules hold as
// in the single-buffer kernels: the block numbers it gets are buffer-relative (`first` below counts from the buffer's block 0,
// the tail part's first block is main_blocks), all 64 lanes take part in both cross-lane moves before any lane skips a store, the
// ownership question is asked about the block a lane STORES, and no lane and no workgroup leaves before inverse_granule's barriers.
// The kernels are BC6H's own and not a body shared with BC7: with the bodies in a common header BC7's instructions moved
// (docs/IMAGE_DECODE.md, "Many BC6H buffers in one call", the kernels).
#include <cstddef>

#include "bc6h_image_batch_launch.h"
#include "bc6h_image_sinks.h"
#include "device_region_table.h"

namespace dxtlt {
namespace bc6h {
namespace {

using granule::inverse_granule;

template <bool TAIL>
using BatchRegionPixelSink = Bc6hRegionPixelSinkOf<DeviceRegionTable, TAIL>;

// An entry as the workgroup sees it: scalar loads (the entry's address is uniform), the buffer pointer tagged as global memory --
// a pointer that was loaded from memory is a generic one to the compiler
struct EntryView {
    const uint8_t* src;
    uint64_t regions_at, main_blocks, first_granule;
    uint32_t first_wg, region_count, tail;
};

__device__ __forceinline__ EntryView load_entry(const ImageBatchEntry* entry)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(entry);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(entry);
    EntryView v;
    v.src = (const uint8_t*)(global_cptr)q[0];
    v.regions_at = q[1];
    v.main_blocks = q[2];
    v.first_granule = q[3];
    v.first_wg = w[8];
    v.region_count = w[9];
    v.tail = w[10];
    // everything of the entry stays on the scalar unit: the granule kernel has 4 vector registers to spare under the 128 of its
    // fourth wave per SIMD
    uint64_t at = reinterpret_cast<uintptr_t>(v.src);
    asm("" : "+s"(at), "+s"(v.regions_at), "+s"(v.main_blocks), "+s"(v.first_granule));
    asm("" : "+s"(v.first_wg), "+s"(v.region_count), "+s"(v.tail));
    v.src = (const uint8_t*)(global_cptr)at;
    return v;
}
static_assert(offsetof(ImageBatchEntry, src) == 0 && offsetof(ImageBatchEntry, regions) == 8 && offsetof(ImageBatchEntry, main_blocks) == 16 &&
                  offsetof(ImageBatchEntry, first_granule) == 24 && offsetof(ImageBatchEntry, first_wg) == 32 &&
                  offsetof(ImageBatchEntry, region_count) == 36 && offsetof(ImageBatchEntry, tail) == 40,
              "load_entry reads ImageBatchEntry by qword and dword offsets");

// Workgroup b finds its entry -- `coarse[b / 64]` is the entry of workgroup 64 * (b / 64), a short scan from there, every load
// uniform -- and runs one granule of the entry's buffer.
__global__ void __launch_bounds__(256)
bc6h_batch_inverse_images(const ImageBatchEntry* __restrict__ entries, const uint32_t* __restrict__ coarse, uint32_t n_entries)
{
    const uint32_t b = blockIdx.x;
    uint32_t i = coarse[b >> 6];
    while (i + 1 < n_entries && entries[i + 1].first_wg <= b)
        ++i;
    const EntryView e = load_entry(entries + i);
    const BatchRegionPixelSink<false> sink{DeviceRegionTable{e.regions_at, e.region_count}};
    // the granule's first block of the BUFFER, pinned to scalar registers as in the BC7 kernel
    uint64_t first = (e.first_granule + (b - e.first_wg)) * kT;
    asm volatile("" : "+s"(first));
    inverse_granule<Bc6hCodec, 256, false, BatchRegionPixelSink<false>>(e.src, nullptr, e.main_blocks, first, 0, sink);
}

// One workgroup per tail entry, with the arguments inverse_images<Bc6hImage, 256, true> gets: the tail part's byte 0, its blocks,
// and main_blocks as its first block
__global__ void __launch_bounds__(256)
bc6h_batch_inverse_image_tails(const ImageBatchEntry* __restrict__ tails)
{
    const EntryView e = load_entry(tails + blockIdx.x);
    const BatchRegionPixelSink<true> sink{DeviceRegionTable{e.regions_at, e.region_count}};
    inverse_granule<Bc6hCodec, 256, true, BatchRegionPixelSink<true>>(e.src, nullptr, e.tail, e.main_blocks, (int)e.tail, sink);
}

}  // namespace

hipError_t launch_image_batch(const ImageBatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries, uint32_t granule_wgs,
                              const ImageBatchEntry* d_tails, uint32_t n_tails, hipStream_t stream)
{
    if (granule_wgs > kMaxBatchWorkgroups || n_tails > kMaxBatchWorkgroups)
        return hipErrorInvalidValue;
    if (granule_wgs > 0 && n_entries > 0) {
        hipLaunchKernelGGL(bc6h_batch_inverse_images, dim3(granule_wgs), dim3(256), 0, stream, d_entries, d_coarse, n_entries);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
    }
    if (n_tails > 0) {
        hipLaunchKernelGGL(bc6h_batch_inverse_image_tails, dim3(n_tails), dim3(256), 0, stream, d_tails);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace bc6h
}  // namespace dxtlt
