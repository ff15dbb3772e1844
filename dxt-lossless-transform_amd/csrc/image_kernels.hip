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
#include "bcn_decode.h"
#include "bcn_device.h"
#include "image_launch.h"
#include "launch_grid.h"

namespace dxtlt {
namespace {

typedef uint32_t u32x4_align4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4_align8 __attribute__((ext_vector_type(4), aligned(8)));

// the sixteen pixels of block `b` of the image into their rows
__device__ __forceinline__ void store_block_pixels(const ImageSink& img, uint64_t b, const uint32_t (&px)[16])
{
    const BlockPlace p = place_block<4>(img, b);
    const bool aligned16 = ((reinterpret_cast<uintptr_t>(img.pixels) | img.pitch) & 15) == 0;   // uniform
    if (p.cols == 4 && p.rows == 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint8_t* row = block_row(img, p, r);
            const u32x4 v = u32x4{px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]};
            if (aligned16)
                store_streaming16(row, v);
            else
                *reinterpret_cast<u32x4_align4*>(row) = v;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint32_t* row = reinterpret_cast<uint32_t*>(block_row(img, p, r));
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((uint32_t)r < p.rows && (uint32_t)c < p.cols)
                    row[c] = px[4 * r + c];
        }
    }
}

template <int FMT>
__device__ __forceinline__ void decode_and_store(const ImageSink& img, uint64_t b, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3)
{
    const uint32_t q[4] = {q0, q1, q2, q3};
    uint32_t px[16];
    decode_block_px<FMT>(q, px);
    store_block_pixels(img, b, px);
}

__device__ __forceinline__ uint32_t from_lane(uint32_t v, int lane)
{
    return (uint32_t)__builtin_amdgcn_ds_bpermute(lane * 4, (int)v);
}

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
    const uint64_t tile = !whole ? (uint64_t)sh.full_tiles
                          : shifts_xcd_contiguous(sh, true) ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)wg;
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
template <int FMT>
struct ChannelFormat {
    static_assert(FMT == kBc4 || FMT == kBc5, "one- and two-channel decoders exist for BC4 and BC5");
    static constexpr int bpp = FMT == kBc4 ? 1 : 2;
    static constexpr int per_vector = FMT == kBc4 ? 2 : 1;   // blocks in a lane's 16 bytes
};

// w[r] = the 8 bytes of pixel row r of the lane's vector (BC4: .x block 2t, .y block 2t + 1)
template <int FMT>
__device__ __forceinline__ void decode_channel_vector(u32x4 q, u32x2 (&w)[4])
{
    if constexpr (FMT == kBc4) {
        uint32_t a[4], b[4];
        decode_bc4_block_rows(q.x, q.y, a);
        decode_bc4_block_rows(q.z, q.w, b);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            w[r] = u32x2{a[r], b[r]};
    } else {
        const uint32_t qq[4] = {q.x, q.y, q.z, q.w};
        uint32_t rows[4][2];
        decode_bc5_block_rows(qq, rows);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            w[r] = u32x2{rows[r][0], rows[r][1]};
    }
}

// One block for itself: its row r is the low 4 * BPP bytes of rows[r]
template <int BPP>
__device__ __forceinline__ void store_channel_block(const ImageSink& img, const BlockPlace& p, const uint64_t (&rows)[4])
{
    const uintptr_t al = reinterpret_cast<uintptr_t>(img.pixels) | img.pitch;   // uniform; a block's offset in its row is a multiple of 4
    if (p.cols == 4 && p.rows == 4) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint8_t* row = block_row(img, p, r);
            if ((al & 3) == 0) {
#pragma unroll
                for (int i = 0; i < BPP; ++i)
                    reinterpret_cast<uint32_t*>(row)[i] = (uint32_t)(rows[r] >> (32 * i));
            } else if ((al & 1) == 0) {
#pragma unroll
                for (int i = 0; i < 2 * BPP; ++i)
                    reinterpret_cast<uint16_t*>(row)[i] = (uint16_t)(rows[r] >> (16 * i));
            } else if constexpr (BPP == 1) {   // (a two-byte pixel never sits at an odd address: the C ABI's checks)
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    row[i] = (uint8_t)(rows[r] >> (8 * i));
            }
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint8_t* row = block_row(img, p, r);
#pragma unroll
            for (int c = 0; c < 4; ++c)
                if ((uint32_t)r < p.rows && (uint32_t)c < p.cols) {
                    if constexpr (BPP == 1)
                        row[c] = (uint8_t)(rows[r] >> (8 * c));
                    else
                        reinterpret_cast<uint16_t*>(row)[c] = (uint16_t)(rows[r] >> (16 * c));
                }
        }
    }
}

// A lane for itself: the first `have` (1 .. per_vector) blocks of its vector, whose first block is block `first` of the image
template <int FMT>
__device__ __forceinline__ void store_channel_lane(const ImageSink& img, uint64_t first, const u32x2 (&w)[4], int have)
{
    constexpr int BPP = ChannelFormat<FMT>::bpp, PV = ChannelFormat<FMT>::per_vector;
    const BlockPlace p = place_block<BPP>(img, first);
    const uintptr_t al = reinterpret_cast<uintptr_t>(img.pixels) | img.pitch;   // uniform
    // PV blocks from column p.bx on, whole, in this block row, their 8 bytes per pixel row on an 8-byte address
    const bool rows8 = have == PV && (al & 7) == 0 && (p.bx & (PV - 1)) == 0 && 4 * ((uint64_t)p.bx + PV) <= img.width && p.rows == 4;
    if (rows8) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            uint8_t* row = block_row(img, p, r);
            if ((al & 15) == 0)
                store_streaming8(row, w[r]);
            else
                *reinterpret_cast<u32x2*>(row) = w[r];
        }
        return;
    }
    if constexpr (FMT == kBc4) {
        const uint64_t a[4] = {w[0].x, w[1].x, w[2].x, w[3].x};
        store_channel_block<BPP>(img, p, a);
        if (have == 2) {
            const uint64_t b[4] = {w[0].y, w[1].y, w[2].y, w[3].y};
            store_channel_block<BPP>(img, place_block<BPP>(img, first + 1), b);
        }
    } else {
        uint64_t a[4];
#pragma unroll
        for (int r = 0; r < 4; ++r)
            a[r] = ((uint64_t)w[r].y << 32) | w[r].x;
        store_channel_block<BPP>(img, p, a);
    }
}

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
    const uint64_t tile = !whole ? (uint64_t)sh.full_tiles
                          : shifts_xcd_contiguous(sh, true) ? xcd_contiguous_tile(wg, sh.full_tiles) : (uint64_t)wg;
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

// ---- host-side dispatch of the fused kernels -------------------------------------------------------------------------
template <typename SINK>
struct ImageKernelsOf {
    void (*tiled)(const uint8_t*, SINK, uint64_t, uint64_t);             // default_tile_threads(fmt, true) lanes
    void (*shifted)(const uint8_t*, SINK, uint64_t, uint64_t, Shifts);   // shift_tile_threads(fmt) lanes
};
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

constexpr uint64_t kMaxBlocksPerImageLaunch = 1ull << 31;   // launch_transform's sub-ranges

// The launches of the inverse transform's own plan for blocks [first_block, first_block + n) -- `s` the format's effective
// settings -- with the kernels `ks`, whose sink is SINK{img, the launch's first block in the image}
template <typename SINK>
hipError_t launch_planned_image(Format fmt, const Settings& s, const ImageKernelsOf<SINK>& ks, const void* soa, uint64_t total_blocks,
                                uint64_t first_block, uint64_t n, const ImageSink& img, hipStream_t stream)
{
    const auto* soa8 = static_cast<const uint8_t*>(soa);
    for (uint64_t off = 0; off < n; off += kMaxBlocksPerImageLaunch) {
        const Range sub{total_blocks, first_block + off, std::min(kMaxBlocksPerImageLaunch, n - off)};
        // the inverse transform's own plan for the sub-range (the block side's address plays no part in it): aligned tiles
        // and an edge tile behind them, or shifted tiles with theirs
        constexpr int kCap = 8;
        DebugPlannedLaunch plan[kCap];
        const int launches = debug_plan_transform(fmt, true, s, reinterpret_cast<uintptr_t>(soa), 0, sub, nullptr, plan, kCap);
        if (launches < 0 || launches > kCap)
            return hipErrorInvalidValue;
        for (int i = 0; i < launches; ++i) {
            const DebugPlannedLaunch& l = plan[i];
            const SINK sink{img, off + l.aos_offset / (uint64_t)fmt_block(fmt)};
            if (l.kind == 0) {
                if (l.threads != default_tile_threads(fmt, true))
                    return hipErrorInvalidValue;
                hipLaunchKernelGGL(ks.tiled, dim3(l.workgroups), dim3(l.threads), 0, stream, soa8, sink, total_blocks, sub.first_block);
            } else {
                if (l.kind != 2 || l.threads != shift_tile_threads(fmt))
                    return hipErrorInvalidValue;
                Shifts sh{};
                for (int k = 0; k < 6; ++k) {
                    sh.d[k] = l.shift[k];
                    sh.gbase[k] = l.gbase[k];
                }
                sh.natural = l.natural;
                sh.halo_vecs = l.halo_vecs;
                sh.full_tiles = l.full_tiles;
                sh.range_blocks = l.range_blocks;
#ifdef DXTLT_EXPERIMENTS
                sh.xcd_remap = 1;
#endif
                hipLaunchKernelGGL(ks.shifted, dim3(l.workgroups), dim3(l.threads), 0, stream, soa8, sink, total_blocks, sub.first_block, sh);
            }
            if (hipError_t e = hipGetLastError(); e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
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
    return launch_planned_image(fmt, s, ks, soa, total_blocks, first_block, n, img, stream);
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
    return launch_planned_image(fmt, s, ks, soa, total_blocks, first_block, n, img, stream);
}

}  // namespace dxtlt
