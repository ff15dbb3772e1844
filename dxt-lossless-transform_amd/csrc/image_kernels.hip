// image_kernels.hip -- BC1 / BC2 / BC3 blocks -> a row-major RGBA8888 image, BC4 / BC5 blocks -> a row-major R8 / RG8 image
// (include/dxtlt_image.h; docs/IMAGE_DECODE.md; the one- and two-channel kernels have their notes at "BC4 / BC5" below):
//   * decode_image_kernel: a block array in block order -> the image, one block per lane;
//   * inv_tiled_image / inv_tiled_shift_image: the inverse transform's aligned and shifted / edge tiles (bcn_device.h) with the
//     block store replaced by "decode and store four pixel rows" (PixelSink), so that the untransformed blocks never touch
//     memory.  Which tiles a range takes is launch_transform's own plan (debug_plan_transform, bcn_kernels.hip).
//
// Store shape.  A block's pixel row is 16 bytes, and the blocks of one block row lie side by side: 64 lanes that hold 64
// consecutive blocks write 1 KiB of consecutive bytes per pixel row and store instruction -- the shape bcn_decode.hip found to
// run at 0.80 of peak, against 0.17 for a lane that stores its own 64 bytes.  BC2 / BC3 tiles have that shape as they are (one
// block per lane).  A BC1 lane holds blocks 2t and 2t + 1, whose rows together are 32 bytes with the next lane's 32 bytes behind
// them: the wave's 128 blocks are first dealt out again so that lane l holds blocks l and 64 + l of the wave (eight
// ds_bpermute_b32 on the 8-byte blocks -- cheaper than exchanging the 128 bytes of pixels, and no LDS is allocated: a
// bpermute uses the LDS crossbar only, so bank conflicts do not arise).  A wave that straddles a block row writes two runs.
// Stores: `sc1 nt` streaming stores (streaming_store.h) when the pixel pointer and the pitch are multiples of 16, plain
// 4-byte aligned vector stores otherwise; a block clipped by the image's right or bottom edge is written pixel by pixel.
#include "image_launch.h"
#include "image_planned_launch.h"
#include "image_store.h"
#include "launch_grid.h"

namespace dxtlt {
namespace {

// The sink of the inverse tiles (bcn_device.h, AosSink): the launch's first block is block `block0` of the image.
struct PixelSink {
    ImageSink img;
    uint64_t block0;

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store(uint8_t*, uint64_t tile, int t, u32x4 q) const
    {
        static_assert(FMT == kBc1 || FMT == kBc2 || FMT == kBc3, "decoders exist for BC1, BC2 and BC3");
        constexpr int T = tile_blocks(FMT, THREADS);
        if constexpr (FMT == kBc1) {
            // the wave's blocks dealt out again: lane l takes blocks l and 64 + l of the wave's 128 (all 64 lanes are here)
            const int lane = t & 63, half = lane >> 1;
            const bool second = (lane & 1) != 0;
            const uint32_t ax = from_lane(q.x, half), ay = from_lane(q.y, half), az = from_lane(q.z, half), aw = from_lane(q.w, half);
            const uint32_t bx = from_lane(q.x, 32 + half), by = from_lane(q.y, 32 + half), bz = from_lane(q.z, 32 + half),
                           bw = from_lane(q.w, 32 + half);
            const uint64_t first = block0 + tile * T + (uint64_t)(2 * (t - lane) + lane);
            decode_and_store<FMT>(img, first, second ? az : ax, second ? aw : ay, 0, 0);
            decode_and_store<FMT>(img, first + 64, second ? bz : bx, second ? bw : by, 0, 0);
        } else {
            decode_and_store<FMT>(img, block0 + tile * T + (uint64_t)t, q.x, q.y, q.z, q.w);
        }
    }

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store_edge(uint8_t*, uint64_t tile, int t, u32x4 q, int own) const
    {
        constexpr int T = tile_blocks(FMT, THREADS);
        if constexpr (FMT == kBc1) {   // one ragged tile per image: every lane writes its own blocks
            const uint64_t first = block0 + tile * T + (uint64_t)(2 * t);
            decode_and_store<FMT>(img, first, q.x, q.y, 0, 0);
            if (2 * t + 1 < own)
                decode_and_store<FMT>(img, first + 1, q.z, q.w, 0, 0);
        } else {
            decode_and_store<FMT>(img, block0 + tile * T + (uint64_t)t, q.x, q.y, q.z, q.w);
        }
    }
};

template <int FMT, int VARIANT, bool SA, bool SC, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_image(const uint8_t* __restrict__ soa, PixelSink sink, uint64_t total_blocks, uint64_t first_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[THREADS * 16];
    inv_aligned_tile<FMT, VARIANT, SA, SC, THREADS, PixelSink>(soa, nullptr, total_blocks, first_block, blockIdx.x, lds, sink);
}

// inv_tiled_shift with the sink: workgroups [0, sh.full_tiles) are whole tiles, one behind them the edge tile
template <int FMT, int VARIANT, bool SA, bool SC, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_shift_image(const uint8_t* __restrict__ soa_arg, PixelSink sink, uint64_t total_blocks, uint64_t first_block, Shifts sh_arg)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    const uint32_t wg = blockIdx.x;
    const Shifts sh = shifts_fetched_at_once(sh_arg);
    const uint8_t* __restrict__ soa = fetched_now(soa_arg);
    const bool whole = wg < sh.full_tiles;
    const uint64_t tile = whole ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)sh.full_tiles;
    if (!whole)
        inv_shift_edge_tile<FMT, VARIANT, SA, SC, THREADS, PixelSink>(soa, nullptr, total_blocks, sh, tile, lds, sink);
    else
        inv_shift_tile<FMT, VARIANT, SA, SC, THREADS, PixelSink>(soa, nullptr, total_blocks, first_block, sh, tile, lds, sink);
}

// ---- BC4 / BC5: R8 / RG8 images ------------------------------------------------------------------------------------------
// A lane's 16-byte vector is two BC4 blocks (2t, 2t + 1) or one BC5 block.  Decoded (decode_bc4_block_rows, bcn_decode.h) it is
// four pixel rows of 8 bytes -- BC4: the two blocks' 4-byte rows side by side when both lie in one block row; BC5: r g r g r g r g.
// Store shape.  Every lane stores its own 8 bytes of each of the four rows (four 8-byte `sc1 nt` stores, store_streaming8), so
// that a wave instruction writes 512 consecutive bytes of a pixel row in 8-byte pieces: 0.81 of peak on 16384 x 16384 for both
// formats, the rate of the BC3 image kernel's 1 KiB runs of 16-byte pieces.  The other form that was built -- lanes 2k and
// 2k + 1 exchange half of their rows with four DPP moves, the even lane then stores rows 0 and 1 and the odd lane rows 2 and 3
// in 16-byte pieces, two store instructions per lane -- was 1 to 4 % slower in every cell and is not here
// (profiles/channel_image_bench.json, "ab"; docs/IMAGE_DECODE.md).
// The 8-byte rows need the lane's blocks whole and in one block row, and the pixel pointer and the pitch multiples of 8
// (`sc1 nt` when they are multiples of 16, plain stores otherwise).  A lane that has not all of that writes every block for
// itself, a row as dwords, halfwords or bytes -- the alignment the pixel pointer and the pitch have -- and a block clipped by
// the right or bottom edge pixel by pixel.
// The sink of the inverse tiles for BC4 / BC5 (bcn_device.h, AosSink): the launch's first block is block `block0` of the image.
struct ChannelSink {
    ImageSink img;
    uint64_t block0;

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store(uint8_t*, uint64_t tile, int t, u32x4 q) const
    {
        constexpr int T = tile_blocks(FMT, THREADS), PV = ChannelFormat<FMT>::per_vector;
        u32x2 w[4];
        decode_channel_vector<FMT>(q, w);
        store_channel_lane<FMT>(img, block0 + tile * T + (uint64_t)(PV * t), w, PV);
    }

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store_edge(uint8_t*, uint64_t tile, int t, u32x4 q, int own) const
    {
        constexpr int T = tile_blocks(FMT, THREADS), PV = ChannelFormat<FMT>::per_vector;
        u32x2 w[4];
        decode_channel_vector<FMT>(q, w);
        store_channel_lane<FMT>(img, block0 + tile * T + (uint64_t)(PV * t), w, own - PV * t < PV ? own - PV * t : PV);
    }
};

template <int FMT, bool SA, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_channel_image(const uint8_t* __restrict__ soa, ChannelSink sink, uint64_t total_blocks, uint64_t first_block)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[THREADS * 16];
    inv_aligned_tile<FMT, kNone, SA, false, THREADS, ChannelSink>(soa, nullptr, total_blocks, first_block, blockIdx.x, lds, sink);
}

template <int FMT, bool SA, int THREADS>
__global__ void __launch_bounds__(THREADS)
inv_tiled_shift_channel_image(const uint8_t* __restrict__ soa_arg, ChannelSink sink, uint64_t total_blocks, uint64_t first_block,
                              Shifts sh_arg)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    const uint32_t wg = blockIdx.x;
    const Shifts sh = shifts_fetched_at_once(sh_arg);
    const uint8_t* __restrict__ soa = fetched_now(soa_arg);
    const bool whole = wg < sh.full_tiles;
    const uint64_t tile = whole ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)sh.full_tiles;
    if (!whole)
        inv_shift_edge_tile<FMT, kNone, SA, false, THREADS, ChannelSink>(soa, nullptr, total_blocks, sh, tile, lds, sink);
    else
        inv_shift_tile<FMT, kNone, SA, false, THREADS, ChannelSink>(soa, nullptr, total_blocks, first_block, sh, tile, lds, sink);
}

// ---- the plain decoder: blocks in block order, one per lane ------------------------------------------------------------
constexpr int kImageThreads = 256;

template <int FMT, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_image_kernel(const uint8_t* __restrict__ in, ImageSink img, uint64_t num_blocks)
{
    constexpr int BS = FMT == kBc1 ? 8 : 16;
    const uint64_t b = workgroup_index() * kImageThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
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
        for (int i = 0; i < BS; ++i)
            q[i >> 2] |= (uint32_t)in[BS * b + i] << (8 * (i & 3));
    }
    decode_and_store<FMT>(img, b, q[0], q[1], q[2], q[3]);
}

template <int FMT>
hipError_t decode_image_fmt(const void* blocks, const ImageSink& img, hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    dim3 grid;
    if (hipError_t e = grid_rows(n, kImageThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    if ((reinterpret_cast<uintptr_t>(blocks) & (uintptr_t)(fmt_block(FMT) - 1)) == 0)
        hipLaunchKernelGGL((decode_image_kernel<FMT, true>), grid, dim3(kImageThreads), 0, stream, in, img, n);
    else
        hipLaunchKernelGGL((decode_image_kernel<FMT, false>), grid, dim3(kImageThreads), 0, stream, in, img, n);
    return hipGetLastError();
}

// BC4 / BC5: 16 bytes of blocks per lane, as in the tiles, and the tiles' stores
template <int FMT, bool ALIGNED>
__global__ void __launch_bounds__(kImageThreads)
decode_channel_image_kernel(const uint8_t* __restrict__ in, ImageSink img, uint64_t num_blocks)
{
    constexpr int BS = fmt_block(FMT), PV = ChannelFormat<FMT>::per_vector;
    const uint64_t vec = workgroup_index() * kImageThreads + threadIdx.x, first = vec * PV;
    if (first >= num_blocks)
        return;
    const int have = num_blocks - first < (uint64_t)PV ? (int)(num_blocks - first) : PV;
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
        for (int i = 0; i < BS * have; ++i)
            q[i >> 2] |= (uint32_t)in[BS * first + i] << (8 * (i & 3));
    }
    u32x2 w[4];
    decode_channel_vector<FMT>(u32x4{q[0], q[1], q[2], q[3]}, w);
    store_channel_lane<FMT>(img, first, w, have);
}

template <int FMT>
hipError_t decode_channel_image_fmt(const void* blocks, const ImageSink& img, hipStream_t stream)
{
    constexpr int PV = ChannelFormat<FMT>::per_vector;
    const uint64_t n = image_blocks(img);
    dim3 grid;
    if (hipError_t e = grid_rows((n + PV - 1) / PV, kImageThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    if ((reinterpret_cast<uintptr_t>(blocks) & (uintptr_t)(fmt_block(FMT) - 1)) == 0)
        hipLaunchKernelGGL((decode_channel_image_kernel<FMT, true>), grid, dim3(kImageThreads), 0, stream, in, img, n);
    else
        hipLaunchKernelGGL((decode_channel_image_kernel<FMT, false>), grid, dim3(kImageThreads), 0, stream, in, img, n);
    return hipGetLastError();
}

// ---- host-side dispatch of the fused kernels (ImageKernelsOf, launch_planned_image: image_planned_launch.h) -------------
using ImageKernels = ImageKernelsOf<PixelSink>;

template <int FMT, int VARIANT, bool SA, bool SC>
ImageKernels image_kernels_for()
{
    return ImageKernels{inv_tiled_image<FMT, VARIANT, SA, SC, default_tile_threads(FMT, true)>,
                        inv_tiled_shift_image<FMT, VARIANT, SA, SC, shift_tile_threads(FMT)>};
}

template <int FMT, int VARIANT>
ImageKernels pick_image_splits(bool sa, bool sc)
{
    if constexpr (FMT == kBc3) {
        if (sa)
            return sc ? image_kernels_for<FMT, VARIANT, true, true>() : image_kernels_for<FMT, VARIANT, true, false>();
    }
    return sc ? image_kernels_for<FMT, VARIANT, false, true>() : image_kernels_for<FMT, VARIANT, false, false>();
}

template <int FMT>
ImageKernels pick_image_kernels(int variant, bool sa, bool sc)
{
    switch (variant) {
    case kNone: return pick_image_splits<FMT, kNone>(sa, sc);
    case kVar1: return pick_image_splits<FMT, kVar1>(sa, sc);
    case kVar2: return pick_image_splits<FMT, kVar2>(sa, sc);
    default: return pick_image_splits<FMT, kVar3>(sa, sc);
    }
}

// BC4 / BC5: no decorrelation and no colour split; the endpoint split picks the kernels (pick_bc45, bcn_kernels.hip)
template <int FMT>
ImageKernelsOf<ChannelSink> pick_channel_kernels(bool split_endpoints)
{
    constexpr int TH = default_tile_threads(FMT, true), SH = shift_tile_threads(FMT);
    if (split_endpoints)
        return {inv_tiled_channel_image<FMT, true, TH>, inv_tiled_shift_channel_image<FMT, true, SH>};
    return {inv_tiled_channel_image<FMT, false, TH>, inv_tiled_shift_channel_image<FMT, false, SH>};
}

}  // namespace

hipError_t launch_decode_image(int fmt, const void* blocks, const ImageSink& img, hipStream_t stream)
{
    if (image_blocks(img) == 0)
        return hipSuccess;
    switch (fmt) {
    case kBc1: return decode_image_fmt<kBc1>(blocks, img, stream);
    case kBc2: return decode_image_fmt<kBc2>(blocks, img, stream);
    case kBc3: return decode_image_fmt<kBc3>(blocks, img, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_untransform_decode_image(Format fmt, const Settings& s_arg, const void* soa, uint64_t total_blocks,
                                           uint64_t first_block, const ImageSink& img, hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    if (fmt != kBc1 && fmt != kBc2 && fmt != kBc3)
        return hipErrorInvalidValue;
    const Settings s = effective_settings(fmt, s_arg);
    if (s.variant < 0 || s.variant > 3 || first_block > total_blocks || n > total_blocks - first_block)
        return hipErrorInvalidValue;
    const ImageKernels ks = fmt == kBc1   ? pick_image_kernels<kBc1>(s.variant, false, s.split_colour)
                            : fmt == kBc2 ? pick_image_kernels<kBc2>(s.variant, false, s.split_colour)
                                          : pick_image_kernels<kBc3>(s.variant, s.split_alpha, s.split_colour);
    return launch_planned_image(fmt, s, ks, soa, total_blocks, first_block, n, stream, [&](uint64_t block0) { return PixelSink{img, block0}; });
}

hipError_t launch_decode_channel_image(int fmt, const void* blocks, const ImageSink& img, hipStream_t stream)
{
    if (image_blocks(img) == 0)
        return hipSuccess;
    switch (fmt) {
    case kBc4: return decode_channel_image_fmt<kBc4>(blocks, img, stream);
    case kBc5: return decode_channel_image_fmt<kBc5>(blocks, img, stream);
    default: return hipErrorInvalidValue;
    }
}

hipError_t launch_untransform_decode_channel_image(Format fmt, bool split_endpoints, const void* soa, uint64_t total_blocks,
                                                   uint64_t first_block, const ImageSink& img, hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    if ((fmt != kBc4 && fmt != kBc5) || first_block > total_blocks || n > total_blocks - first_block)
        return hipErrorInvalidValue;
    const Settings s = effective_settings(fmt, Settings{0, split_endpoints, false});
    const ImageKernelsOf<ChannelSink> ks = fmt == kBc4 ? pick_channel_kernels<kBc4>(split_endpoints) : pick_channel_kernels<kBc5>(split_endpoints);
    return launch_planned_image(fmt, s, ks, soa, total_blocks, first_block, n, stream, [&](uint64_t block0) { return ChannelSink{img, block0}; });
}

}  // namespace dxtlt
