// image_regions_kernels.hip -- several images of one block buffer in one launch (include/dxtlt_image.h, "image regions";
// docs/IMAGE_DECODE.md, "Several images of one buffer"): a mip chain, the faces of a cube map, the slices of an array.
//   * inv_tiled_regions_image / inv_tiled_shift_regions_image and their channel twins: the inverse tiles of image_kernels.hip
//     (bcn_device.h) planned ONCE over the range that covers a group of up to sixteen regions, with a sink that finds every
//     block's image in a table that travels in the kernel arguments (image_regions.h);
//   * decode_regions_image_kernel / decode_regions_channel_image_kernel: the plain decoders over the same range.
// Decoding and the stores are image_store.h's, those of the single-image kernels; the sinks are image_region_sinks.h's.
//
// The lookup.  A wave holds 64 or 128 consecutive blocks of the buffer, and but for the few waves at a chain's tail all of them
// lie in one region.  So the wave first asks for the region of its whole run with its first block in scalar registers
// (region_of_run: scalar loads and comparisons, done at the first region that holds the run); the image it finds is uniform,
// and the stores are exactly the single-image kernels': the streaming-or-plain choice is uniform again.  Only a wave whose run
// straddles a boundary or touches a gap lets every lane search for itself (region_of_block: the same walk with per-lane
// selects); there the image is per lane and so is the store choice.  A block in no region is dropped.  Why both walks are loops
// and not unrolled is in image_regions.h: the table must not go to scratch memory.  The other form that was built -- every lane
// of every wave searches for itself -- and what both cost is in docs/IMAGE_DECODE.md.
#include "image_launch.h"
#include "image_planned_launch.h"
#include "image_region_sinks.h"
#include "image_regions.h"
#include "image_store.h"
#include "launch_grid.h"

namespace dxtlt {
namespace {

using RegionPixelSink = RegionPixelSinkOf<ImageRegionTable>;
using RegionChannelSink = RegionChannelSinkOf<ImageRegionTable>;

// ---- the fused kernels: inv_tiled_image / inv_tiled_shift_image (image_kernels.hip) with the region sinks ---------------
template <int FMT, int VARIANT, bool SA, bool SC, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_regions_image(const uint8_t* __restrict__ soa, RegionPixelSink sink, uint64_t total_blocks, uint64_t first_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[THREADS * 16];
    inv_aligned_tile<FMT, VARIANT, SA, SC, THREADS, RegionPixelSink>(soa, nullptr, total_blocks, first_block, blockIdx.x, lds, sink);
}

template <int FMT, int VARIANT, bool SA, bool SC, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_shift_regions_image(const uint8_t* __restrict__ soa_arg, RegionPixelSink sink, uint64_t total_blocks, uint64_t first_block,
                              Shifts sh_arg)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    const uint32_t wg = blockIdx.x;
    const Shifts sh = shifts_fetched_at_once(sh_arg);
    const uint8_t* __restrict__ soa = fetched_now(soa_arg);
    const bool whole = wg < sh.full_tiles;
    const uint64_t tile = whole ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)sh.full_tiles;
    if (!whole)
        inv_shift_edge_tile<FMT, VARIANT, SA, SC, THREADS, RegionPixelSink>(soa, nullptr, total_blocks, sh, tile, lds, sink);
    else
        inv_shift_tile<FMT, VARIANT, SA, SC, THREADS, RegionPixelSink>(soa, nullptr, total_blocks, first_block, sh, tile, lds, sink);
}

template <int FMT, bool SA, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_regions_channel_image(const uint8_t* __restrict__ soa, RegionChannelSink sink, uint64_t total_blocks, uint64_t first_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[THREADS * 16];
    inv_aligned_tile<FMT, kNone, SA, false, THREADS, RegionChannelSink>(soa, nullptr, total_blocks, first_block, blockIdx.x, lds, sink);
}

template <int FMT, bool SA, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_shift_regions_channel_image(const uint8_t* __restrict__ soa_arg, RegionChannelSink sink, uint64_t total_blocks,
                                      uint64_t first_block, Shifts sh_arg)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    const uint32_t wg = blockIdx.x;
    const Shifts sh = shifts_fetched_at_once(sh_arg);
    const uint8_t* __restrict__ soa = fetched_now(soa_arg);
    const bool whole = wg < sh.full_tiles;
    const uint64_t tile = whole ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)sh.full_tiles;
    if (!whole)
        inv_shift_edge_tile<FMT, kNone, SA, false, THREADS, RegionChannelSink>(soa, nullptr, total_blocks, sh, tile, lds, sink);
    else
        inv_shift_tile<FMT, kNone, SA, false, THREADS, RegionChannelSink>(soa, nullptr, total_blocks, first_block, sh, tile, lds, sink);
}

// ---- the plain decoders: blocks [sink.block0, sink.block0 + num_blocks) of a block array in block order ------------------
constexpr int kImageThreads = 256;

template <int FMT, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_regions_image_kernel(const uint8_t* __restrict__ in, RegionPixelSink sink, uint64_t num_blocks)
{
    constexpr int BS = FMT == kBc1 ? 8 : 16;
    const uint64_t i = workgroup_index() * kImageThreads + threadIdx.x;
    if (i >= num_blocks)
        return;
    const uint64_t b = sink.block0 + i;
    uint32_t q[4] = {0, 0, 0, 0};
    if constexpr (ALIGNED) {   // the block pointer is a multiple of the block size
        if constexpr (FMT == kBc1) {
            const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(in) + b);
            q[0] = v.x, q[1] = v.y;
        } else {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in) + b);
            q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        }
    } else {
        for (int k = 0; k < BS; ++k)
            q[k >> 2] |= (uint32_t)in[BS * b + k] << (8 * (k & 3));
    }
    // (the last wave's run reaches past the last region: its lanes look for themselves)
    sink.decode_and_put<FMT>(wave_run(sink.tab, b - (threadIdx.x & 63), 64), b, q[0], q[1], q[2], q[3]);
}

// BC4 / BC5: 16 bytes of blocks per lane, as in the tiles
template <int FMT, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_regions_channel_image_kernel(const uint8_t* __restrict__ in, RegionChannelSink sink, uint64_t num_blocks)
{
    constexpr int BS = fmt_block(FMT), PV = ChannelFormat<FMT>::per_vector;
    const uint64_t vec = workgroup_index() * kImageThreads + threadIdx.x, i = vec * PV;
    if (i >= num_blocks)
        return;
    const int have = num_blocks - i < (uint64_t)PV ? (int)(num_blocks - i) : PV;
    const uint64_t first = sink.block0 + i;
    uint32_t q[4] = {0, 0, 0, 0};
    if constexpr (ALIGNED) {   // the block pointer is a multiple of the block size
        if constexpr (FMT == kBc4) {
            if (have == 2) {   // two blocks: 16 bytes on an 8-byte address
                const u32x4_align8 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_align8*>(in + 8 * first));
                q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
            } else {
                const u32x2 v = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(in) + first);
                q[0] = v.x, q[1] = v.y;
            }
        } else {
            const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in) + first);
            q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
        }
    } else {
        for (int k = 0; k < BS * have; ++k)
            q[k >> 2] |= (uint32_t)in[BS * first + k] << (8 * (k & 3));
    }
    u32x2 w[4];
    decode_channel_vector<FMT>(u32x4{q[0], q[1], q[2], q[3]}, w);
    sink.put<FMT>(wave_run(sink.tab, first - (uint64_t)(PV * (threadIdx.x & 63)), 64 * PV), first, w, have);
}

template <typename SINK, typename KERNEL>
hipError_t launch_plain(KERNEL aligned, KERNEL unaligned, int block_size, int per_lane, const void* blocks, const SINK& sink,
                        uint64_t num_blocks, hipStream_t stream)
{
    dim3 grid;
    if (hipError_t e = grid_rows((num_blocks + per_lane - 1) / per_lane, kImageThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    if ((reinterpret_cast<uintptr_t>(blocks) & (uintptr_t)(block_size - 1)) == 0)
        hipLaunchKernelGGL(aligned, grid, dim3(kImageThreads), 0, stream, in, sink, num_blocks);
    else
        hipLaunchKernelGGL(unaligned, grid, dim3(kImageThreads), 0, stream, in, sink, num_blocks);
    return hipGetLastError();
}

template <int FMT>
hipError_t decode_regions_fmt(const void* blocks, const ImageRegionTable& tab, uint64_t first, uint64_t n, hipStream_t stream)
{
    if constexpr (FMT == kBc4 || FMT == kBc5)
        return launch_plain(decode_regions_channel_image_kernel<FMT, true>, decode_regions_channel_image_kernel<FMT, false>,
                            fmt_block(FMT), ChannelFormat<FMT>::per_vector, blocks, RegionChannelSink{tab, first}, n, stream);
    else
        return launch_plain(decode_regions_image_kernel<FMT, true>, decode_regions_image_kernel<FMT, false>, fmt_block(FMT), 1, blocks,
                            RegionPixelSink{tab, first}, n, stream);
}

// ---- host-side dispatch of the fused kernels, as in image_kernels.hip ------------------------------------------------------
using RegionKernels = ImageKernelsOf<RegionPixelSink>;

template <int FMT, int VARIANT, bool SA, bool SC>
RegionKernels region_kernels_for()
{
    return RegionKernels{inv_tiled_regions_image<FMT, VARIANT, SA, SC, default_tile_threads(FMT, true)>,
                         inv_tiled_shift_regions_image<FMT, VARIANT, SA, SC, shift_tile_threads(FMT)>};
}

template <int FMT, int VARIANT>
RegionKernels pick_region_splits(bool sa, bool sc)
{
    if constexpr (FMT == kBc3) {
        if (sa)
            return sc ? region_kernels_for<FMT, VARIANT, true, true>() : region_kernels_for<FMT, VARIANT, true, false>();
    }
    return sc ? region_kernels_for<FMT, VARIANT, false, true>() : region_kernels_for<FMT, VARIANT, false, false>();
}

template <int FMT>
RegionKernels pick_region_kernels(int variant, bool sa, bool sc)
{
    switch (variant) {
    case kNone: return pick_region_splits<FMT, kNone>(sa, sc);
    case kVar1: return pick_region_splits<FMT, kVar1>(sa, sc);
    case kVar2: return pick_region_splits<FMT, kVar2>(sa, sc);
    default: return pick_region_splits<FMT, kVar3>(sa, sc);
    }
}

template <int FMT>
ImageKernelsOf<RegionChannelSink> pick_region_channel_kernels(bool split_endpoints)
{
    constexpr int TH = default_tile_threads(FMT, true), SH = shift_tile_threads(FMT);
    if (split_endpoints)
        return {inv_tiled_regions_channel_image<FMT, true, TH>, inv_tiled_shift_regions_channel_image<FMT, true, SH>};
    return {inv_tiled_regions_channel_image<FMT, false, TH>, inv_tiled_shift_regions_channel_image<FMT, false, SH>};
}

}  // namespace

hipError_t launch_decode_image_regions(int fmt, const void* blocks, uint64_t total_blocks, const ImageRegionTable& tab,
                                       hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (!covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    switch (fmt) {
    case kBc1: return decode_regions_fmt<kBc1>(blocks, tab, first, n, stream);
    case kBc2: return decode_regions_fmt<kBc2>(blocks, tab, first, n, stream);
    case kBc3: return decode_regions_fmt<kBc3>(blocks, tab, first, n, stream);
    case kBc4: return decode_regions_fmt<kBc4>(blocks, tab, first, n, stream);
    case kBc5: return decode_regions_fmt<kBc5>(blocks, tab, first, n, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_untransform_decode_image_regions(Format fmt, const Settings& s_arg, const void* soa, uint64_t total_blocks,
                                                   const ImageRegionTable& tab, hipStream_t stream)
{
    uint64_t first = 0, n = 0;
    if (fmt < kBc1 || fmt > kBc5 || !covering_range(tab, total_blocks, first, n))
        return hipErrorInvalidValue;
    const Settings s = effective_settings(fmt, s_arg);
    if (s.variant < 0 || s.variant > 3)
        return hipErrorInvalidValue;
    if (fmt == kBc4 || fmt == kBc5) {
        const ImageKernelsOf<RegionChannelSink> ks =
            fmt == kBc4 ? pick_region_channel_kernels<kBc4>(s.split_alpha) : pick_region_channel_kernels<kBc5>(s.split_alpha);
        return launch_planned_image(fmt, s, ks, soa, total_blocks, first, n, stream,
                                    [&](uint64_t k) { return RegionChannelSink{tab, first + k}; });
    }
    const RegionKernels ks = fmt == kBc1   ? pick_region_kernels<kBc1>(s.variant, false, s.split_colour)
                             : fmt == kBc2 ? pick_region_kernels<kBc2>(s.variant, false, s.split_colour)
                                           : pick_region_kernels<kBc3>(s.variant, s.split_alpha, s.split_colour);
    return launch_planned_image(fmt, s, ks, soa, total_blocks, first, n, stream, [&](uint64_t k) { return RegionPixelSink{tab, first + k}; });
}

}  // namespace dxtlt
