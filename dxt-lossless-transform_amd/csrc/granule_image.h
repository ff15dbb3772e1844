// granule_image.h -- the image kernels and launchers of the two granule-sorted formats, written once over a format's image family
// F (Bc7Image, bc7_image_sinks.h; Bc6hImage, bc6h_image_sinks.h).  docs/IMAGE_DECODE.md, "BC7", "BC6H blocks to a row-major RGBA16F
// image" and the two "Several images of one ... buffer".  A family names
//   * Codec: the granule codec of granule_sort.h;
//   * Sink<TAIL>, RegionSink<TABLE, TAIL>: the staging sinks of the inverse granule sort for one image and for the images of a
//     region table, each measured into its shape in its own header;
//   * kBpp, Decoded, decode(), store(): the bytes of a pixel and the block decode and store of the plain decoders.
// The kernels:
//   * decode_image_kernel, decode_regions_image_kernel: the plain decoders for a block array in BLOCK order, one block per lane.
//     The decoder's mode switch is per lane there (a wave runs the arm of every mode that occurs among its 64 blocks: on a buffer
//     of mixed modes they are bound by instruction issue, not by memory).
//   * inverse_image, inverse_images: the inverse granule sort with a staging sink in the place of its block store.  The blocks are
//     decoded in the sorted domain, where the mode is wave-uniform, and their pixels go through LDS to block order, so that the
//     untransformed blocks never touch memory.  For several images every granule that the covering range touches is un-sorted and
//     decoded ONCE, and each block's pixels go to whichever region of the table owns the block; the per-level way decodes a granule
//     again for every level that has blocks in it: the seven small levels of a 256 x 256 chain all live in the tail part.
// The region table travels in the kernel arguments and is walked only by the two loops of image_regions.h, which says why they
// stay loops: no scratch memory.
// A format's kernels file includes this behind its sinks and instantiates the four launchers (granule_image_launch.h).
#pragma once
#include "granule_image_launch.h"
#include "granule_launch.h"
#include "granule_sort.h"
#include "image_region_sinks.h"
#include "image_store.h"
#include "launch_grid.h"

namespace dxtlt {
namespace {

constexpr int kImageThreads = 256;

// ---- blocks in block order -> image, one block per lane ----------------------------------------------------------------
template <typename F, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_image_kernel(const uint8_t* __restrict__ in, ImageSink img, uint64_t num_blocks)
{
    const uint64_t b = workgroup_index() * kImageThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
    typename F::Decoded d;
    F::decode(load_block<ALIGNED>(in, b), d);
    F::store(img, b, d);
}

// blocks [block0, block0 + num_blocks) of the array: the wave asks about its run of 64 (the last wave's run reaches past the last
// region: its lanes look for themselves), then every lane about its block (put_in_region, image_region_sinks.h)
template <typename F, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_regions_image_kernel(const uint8_t* __restrict__ in, ImageRegionTable tab, uint64_t block0, uint64_t num_blocks)
{
    const uint64_t i = workgroup_index() * kImageThreads + threadIdx.x;
    if (i >= num_blocks)
        return;
    const uint64_t b = block0 + i;
    typename F::Decoded d;
    F::decode(load_block<ALIGNED>(in, b), d);
    put_in_region<F>(tab, wave_run(tab, b - (threadIdx.x & 63), 64), b, d);
}

// ---- the inverse granule sort with a pixel sink ------------------------------------------------------------------------
// Full granules: workgroup g is granule first_granule_block / 1024 + g of the main part (part_blocks blocks, soa = its byte 0).
// TAIL: one workgroup, soa = the tail part's byte 0, first_granule_block = the tail part's first block, n_tail its blocks.
template <typename F, bool TAIL>
using ImageSinkOf = typename F::template Sink<TAIL>;
template <typename F, bool TAIL>
using TableSinkOf = typename F::template RegionSink<ImageRegionTable, TAIL>;   // the table in the kernel arguments

template <typename F, int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
inverse_image(const uint8_t* __restrict__ soa, ImageSinkOf<F, TAIL> sink, uint64_t part_blocks, uint64_t first_granule_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    granule::inverse_granule<typename F::Codec, LANES, TAIL, ImageSinkOf<F, TAIL>>(soa, nullptr, part_blocks,
                                                                                  first_granule_block + granule * granule::kT, n_tail, sink);
}

template <typename F, int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
inverse_images(const uint8_t* __restrict__ soa, TableSinkOf<F, TAIL> sink, uint64_t part_blocks, uint64_t first_granule_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    granule::inverse_granule<typename F::Codec, LANES, TAIL, TableSinkOf<F, TAIL>>(soa, nullptr, part_blocks,
                                                                                  first_granule_block + granule * granule::kT, n_tail, sink);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// The launches of the range [first, end) of a transformed buffer, as granule::for_each_range_launch plans them: full_kernel over
// the main part's granules with the sink `full`, tail_kernel over the tail part with the sink `tail_sink`
template <typename FULL, typename TAIL_SINK>
hipError_t launch_inverse_range(void (*full_kernel)(const uint8_t*, FULL, uint64_t, uint64_t, int),
                                void (*tail_kernel)(const uint8_t*, TAIL_SINK, uint64_t, uint64_t, int), const void* soa_arg,
                                uint64_t total_blocks, uint64_t first, uint64_t end, const FULL& full, const TAIL_SINK& tail_sink,
                                hipStream_t stream)
{
    const auto* soa = static_cast<const uint8_t*>(soa_arg);
    const uint64_t main_blocks = total_blocks - total_blocks % granule::kT;
    return granule::for_each_range_launch(total_blocks, first, end, [&](uint64_t granule, uint64_t granules, bool tail) {
        if (!tail) {
            hipLaunchKernelGGL(full_kernel, dim3((unsigned)granules), dim3(256), 0, stream, soa, full, main_blocks, granule * granule::kT, 0);
        } else {
            const uint64_t n_tail = total_blocks - main_blocks;
            hipLaunchKernelGGL(tail_kernel, dim3(1), dim3(256), 0, stream, soa + main_blocks * 16, tail_sink, n_tail, main_blocks,
                               (int)n_tail);
        }
        return hipGetLastError();
    });
}

}  // namespace

template <typename F>
hipError_t launch_decode_image(const void* blocks, const ImageSink& img, hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_rows(n, kImageThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    hipLaunchKernelGGL((aligned16(blocks) ? decode_image_kernel<F, true> : decode_image_kernel<F, false>), grid, dim3(kImageThreads), 0,
                       stream, in, img, n);
    return hipGetLastError();
}

template <typename F>
hipError_t launch_untransform_decode_image(const void* soa, uint64_t total_blocks, uint64_t first_block, const ImageSink& img,
                                           hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    if (first_block > total_blocks || n > total_blocks - first_block)
        return hipErrorInvalidValue;
    return launch_inverse_range(inverse_image<F, 256, false>, inverse_image<F, 256, true>, soa, total_blocks, first_block, first_block + n,
                                ImageSinkOf<F, false>{img, first_block, n}, ImageSinkOf<F, true>{img, first_block, n}, stream);
}

template <typename F>
hipError_t launch_decode_image_regions(const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (!covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = grid_rows(n, kImageThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    hipLaunchKernelGGL((aligned16(blocks) ? decode_regions_image_kernel<F, true> : decode_regions_image_kernel<F, false>), grid,
                       dim3(kImageThreads), 0, stream, in, tab, first, n);
    return hipGetLastError();
}

template <typename F>
hipError_t launch_untransform_decode_image_regions(const void* soa, uint64_t total_blocks, const ImageRegionTable& tab, hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (!covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    return launch_inverse_range(inverse_images<F, 256, false>, inverse_images<F, 256, true>, soa, total_blocks, first, first + n,
                                TableSinkOf<F, false>{tab}, TableSinkOf<F, true>{tab}, stream);
}

}  // namespace dxtlt
