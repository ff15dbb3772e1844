// bc6h_image_regions_kernels.hip -- several RGBA16F images of one BC6H buffer in one call on gfx950 (include/dxtlt_bc6h_image.h;
// docs/IMAGE_DECODE.md, "Several images of one BC6H buffer"): a mip chain, the faces of a cube map, the slices of an array.
//   * bc6h_inverse_images: the inverse granule sort (granule_sort.h over Bc6hCodec) with Bc6hRegionPixelSink (bc6h_image_sinks.h):
//     every granule that the group's covering range touches is un-sorted and prepared ONCE, in the sorted domain, and each block's
//     pixels go to whichever region of the table owns the block.  The per-level way decodes a granule again for every level
//     that has blocks in it: the seven small levels of a 256 x 256 chain all live in the tail part.
//   * decode_bc6h_regions_image_kernel: the plain decoder for a block array in block order, one block per lane over the same
//     range: decode_bc6h_image_kernel's load and stores (plain, never `sc1 nt`: store_block_row says why), the lookup of the
//     region decoders.
// The table travels in the kernel arguments and is walked only by the two loops of image_regions.h, which says why they stay
// loops: no scratch memory.
#include "bc6h_image_launch.h"
#include "bc6h_image_sinks.h"
#include "granule_launch.h"
#include "launch_grid.h"

namespace dxtlt {
namespace bc6h {
namespace {

using granule::inverse_granule;

constexpr int kThreads = 256;

// Full granules: workgroup g is granule first_granule_block / 1024 + g of the main part (part_blocks blocks, soa = its byte 0).
// TAIL: one workgroup, soa = the tail part's byte 0, first_granule_block = the tail part's first block, n_tail its blocks.
template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc6h_inverse_images(const uint8_t* __restrict__ soa, Bc6hRegionPixelSink<TAIL> sink, uint64_t part_blocks, uint64_t first_granule_block,
                    int n_tail)
{
    const uint64_t granule = blockIdx.x;
    inverse_granule<Bc6hCodec, LANES, TAIL, Bc6hRegionPixelSink<TAIL>>(soa, nullptr, part_blocks, first_granule_block + granule * kT, n_tail,
                                                                       sink);
}

// blocks [block0, block0 + num_blocks) of a block array in block order, one block per lane: the wave asks about its run of 64 (the
// last wave's run reaches past the last region: its lanes look for themselves), then every lane about its block
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc6h_regions_image_kernel(const uint8_t* __restrict__ in, ImageRegionTable tab, uint64_t block0, uint64_t num_blocks)
{
    const uint64_t i = workgroup_index() * kThreads + threadIdx.x;
    if (i >= num_blocks)
        return;
    const uint64_t b = block0 + i;
    const Interp s = prepare_q(load_block<ALIGNED>(in, b));
    const WaveRun run = wave_run(tab, b - (threadIdx.x & 63), 64);
    if (run.region >= 0) {
        store_block_pixels(run.img, run.local + (b - run.first), s);
    } else {
        ImageSink img{nullptr, 0, 1, 0, 0, 8};
        uint64_t local = 0;
        if (region_of_block(tab, b, img, local) >= 0)
            store_block_pixels(img, local, s);
    }
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
    hipLaunchKernelGGL(aligned16(blocks) ? decode_bc6h_regions_image_kernel<true> : decode_bc6h_regions_image_kernel<false>, grid,
                       dim3(kThreads), 0, stream, in, tab, first, n);
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
    return granule::for_each_range_launch(total_blocks, first, first + n, [&](uint64_t granule, uint64_t granules, bool tail) {
        if (tail) {
            const uint64_t n_tail = total_blocks - main_blocks;
            hipLaunchKernelGGL((bc6h_inverse_images<256, true>), dim3(1), dim3(256), 0, stream, soa + main_blocks * 16,
                               Bc6hRegionPixelSink<true>{tab}, n_tail, main_blocks, (int)n_tail);
        } else {
            hipLaunchKernelGGL((bc6h_inverse_images<256, false>), dim3((unsigned)granules), dim3(256), 0, stream, soa,
                               Bc6hRegionPixelSink<false>{tab}, main_blocks, granule * kT, 0);
        }
        return hipGetLastError();
    });
}

}  // namespace bc6h
}  // namespace dxtlt
