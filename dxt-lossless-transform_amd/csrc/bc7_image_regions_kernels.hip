// bc7_image_regions_kernels.hip -- several RGBA8888 images of one BC7 buffer in one call on gfx950 (include/dxtlt_bc7_image.h;
// docs/IMAGE_DECODE.md, "Several images of one BC7 buffer"): a mip chain, the faces of a cube map, the slices of an array.
//   * bc7_inverse_images: the inverse granule sort (granule_sort.h over Bc7Codec) with Bc7RegionPixelSink (bc7_image_sinks.h):
//     every granule that the group's covering range touches is un-sorted and decoded ONCE, in the sorted domain, and each block's
//     pixels go to whichever region of the table owns the block.  The per-level way decodes a granule again for every level
//     that has blocks in it: the seven small levels of a 256 x 256 chain all live in the tail part.
//   * decode_bc7_regions_image_kernel: the plain decoder for a block array in block order, one block per lane over the same
//     range, with the lookup and the stores of the BC1 - BC3 region decoders (RegionPixelSinkOf, image_region_sinks.h).
// The table travels in the kernel arguments and is walked only by the two loops of image_regions.h, which says why they stay
// loops: no scratch memory.
#include "bc7_image_launch.h"
#include "bc7_image_sinks.h"
#include "launch_grid.h"

namespace dxtlt {
namespace bc7 {
namespace {

using granule::inverse_granule;

constexpr int kThreads = 256;

// Full granules: workgroup g is granule first_granule_block / 1024 + g of the main part (part_blocks blocks, soa = its byte 0).
// TAIL: one workgroup, soa = the tail part's byte 0, first_granule_block = the tail part's first block, n_tail its blocks.
template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc7_inverse_images(const uint8_t* __restrict__ soa, Bc7RegionPixelSink sink, uint64_t part_blocks, uint64_t first_granule_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    inverse_granule<Bc7Codec, LANES, TAIL, Bc7RegionPixelSink>(soa, nullptr, part_blocks, first_granule_block + granule * kT, n_tail, sink);
}

// blocks [sink.block0, sink.block0 + num_blocks) of a block array in block order, one block per lane: decode_bc7_image_kernel's
// load, the region decoders' lookup (the last wave's run reaches past the last region: its lanes look for themselves)
using RegionPixelSink = RegionPixelSinkOf<ImageRegionTable>;

template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc7_regions_image_kernel(const uint8_t* __restrict__ in, RegionPixelSink sink, uint64_t num_blocks)
{
    const uint64_t i = workgroup_index() * kThreads + threadIdx.x;
    if (i >= num_blocks)
        return;
    const uint64_t b = sink.block0 + i;
    uint32_t px[16];
    decode_px(load_block<ALIGNED>(in, b), px);
    sink.put(wave_run(sink.tab, b - (threadIdx.x & 63), 64), b, px);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

}  // namespace

hipError_t launch_decode_image_regions(const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (!covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = grid_rows(n, kThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    hipLaunchKernelGGL(aligned16(blocks) ? decode_bc7_regions_image_kernel<true> : decode_bc7_regions_image_kernel<false>, grid,
                       dim3(kThreads), 0, stream, in, RegionPixelSink{tab, first}, n);
    return hipGetLastError();
}

hipError_t launch_untransform_decode_image_regions(const void* soa_arg, uint64_t total_blocks, const ImageRegionTable& tab,
                                                   hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (!covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    const auto* soa = static_cast<const uint8_t*>(soa_arg);
    const uint64_t main_blocks = total_blocks - total_blocks % kT;
    const Bc7RegionPixelSink sink{tab};
    return granule::for_each_range_launch(total_blocks, first, first + n, [&](uint64_t granule, uint64_t granules, bool tail) {
        if (tail) {
            const uint64_t n_tail = total_blocks - main_blocks;
            hipLaunchKernelGGL((bc7_inverse_images<256, true>), dim3(1), dim3(256), 0, stream, soa + main_blocks * 16, sink, n_tail,
                               main_blocks, (int)n_tail);
        } else {
            hipLaunchKernelGGL((bc7_inverse_images<256, false>), dim3((unsigned)granules), dim3(256), 0, stream, soa, sink, main_blocks,
                               granule * kT, 0);
        }
        return hipGetLastError();
    });
}

}  // namespace bc7
}  // namespace dxtlt
