// image_region_sinks.h -- the sinks of the inverse tiles (bcn_device.h, AosSink) that decode a block and write it into the image
// its region names: RegionPixelSinkOf (BC1 / BC2 / BC3 -> RGBA8888) and RegionChannelSinkOf (BC4 / BC5 -> R8 / RG8), over any
// table the lookups of image_regions.h take -- the one in the kernel arguments (image_regions_kernels.hip) and the one in device
// memory (image_batch_kernels.hip).  Device code; decoding and the stores are image_store.h's.
//
// The lookup.  A wave holds 64 or 128 consecutive blocks of the buffer, and but for the few waves at a chain's tail all of them
// lie in one region.  So the wave first asks for the region of its whole run with its first block in scalar registers
// (region_of_run: scalar loads and comparisons, done at the first region that holds the run); the image it finds is uniform,
// and the stores are exactly the single-image kernels': the streaming-or-plain choice is uniform again.  Only a wave whose run
// straddles a boundary or touches a gap lets every lane search for itself (region_of_block: the same walk with per-lane
// selects); there the image is per lane and so is the store choice.  A block in no region is dropped.
#pragma once
#include "bcn_device.h"
#include "image_regions.h"
#include "image_store.h"

namespace dxtlt {

// a value every lane of the wave holds alike, moved to scalar registers
__device__ __forceinline__ uint64_t wave_uniform(uint64_t v)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return ((uint64_t)hi << 32) | lo;
}

// What a wave knows about its run of consecutive blocks [first, first + n): region >= 0 -- all of them are blocks
// [local, local + n) of the image `img`, everything here in scalar registers; -1 -- every lane has to look for itself
struct WaveRun {
    int region;
    ImageSink img;
    uint64_t first, local;
};

template <typename TABLE>
__device__ __forceinline__ WaveRun wave_run(const TABLE& tab, uint64_t first, uint64_t n)
{
    WaveRun w{-1, ImageSink{nullptr, 0, 1, 0, 0, 0}, wave_uniform(first), 0};
    w.region = region_of_run(tab, w.first, n, w.img, w.local);
    return w;
}

__device__ __forceinline__ WaveRun no_wave_run() { return WaveRun{-1, ImageSink{nullptr, 0, 1, 0, 0, 0}, 0, 0}; }

// The wave has asked, now the lane asks: decoded block `b` of the buffer goes to STORE::store(its image, its number in that image,
// decoded) -- the image of the wave's run if the run found one, else the one the lane finds for itself (STORE::kBpp: its bytes per
// pixel); a block in no region is dropped.  STORE is Rgba8888Store below or the image family of BC7 or BC6H (granule_image.h).
template <typename STORE, typename TABLE, typename DECODED>
__device__ __forceinline__ void put_in_region(const TABLE& tab, const WaveRun& run, uint64_t b, const DECODED& decoded)
{
    if (run.region >= 0) {
        STORE::store(run.img, run.local + (b - run.first), decoded);
    } else {
        ImageSink img{nullptr, 0, 1, 0, 0, STORE::kBpp};
        uint64_t local = 0;
        if (region_of_block(tab, b, img, local) >= 0)
            STORE::store(img, local, decoded);
    }
}

struct Rgba8888Store {
    static constexpr uint32_t kBpp = 4;
    static __device__ __forceinline__ void store(const ImageSink& img, uint64_t b, const uint32_t (&px)[16]) { store_block_pixels(img, b, px); }
};

// The sink of the inverse tiles for BC1 / BC2 / BC3 (bcn_device.h, AosSink): the launch's first block is block `block0` of the
// BUFFER.
template <typename TABLE>
struct RegionPixelSinkOf {
    TABLE tab;
    uint64_t block0;

    // block `b` of the buffer, decoded
    __device__ __forceinline__ void put(const WaveRun& run, uint64_t b, const uint32_t (&px)[16]) const
    {
        put_in_region<Rgba8888Store>(tab, run, b, px);
    }

    template <int FMT>
    __device__ __forceinline__ void decode_and_put(const WaveRun& run, uint64_t b, uint32_t q0, uint32_t q1, uint32_t q2, uint32_t q3) const
    {
        const uint32_t q[4] = {q0, q1, q2, q3};
        uint32_t px[16];
        decode_block_px<FMT>(q, px);
        put(run, b, px);
    }

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store(uint8_t*, uint64_t tile, int t, u32x4 q) const
    {
        static_assert(FMT == kBc1 || FMT == kBc2 || FMT == kBc3, "decoders exist for BC1, BC2 and BC3");
        constexpr int T = tile_blocks(FMT, THREADS);
        const int lane = t & 63;
        if constexpr (FMT == kBc1) {
            // the wave's blocks dealt out again as in PixelSink, by all 64 lanes, before any lane finds that it has no image
            const int half = lane >> 1;
            const bool second = (lane & 1) != 0;
            const uint32_t ax = from_lane(q.x, half), ay = from_lane(q.y, half), az = from_lane(q.z, half), aw = from_lane(q.w, half);
            const uint32_t bx = from_lane(q.x, 32 + half), by = from_lane(q.y, 32 + half), bz = from_lane(q.z, 32 + half),
                           bw = from_lane(q.w, 32 + half);
            const WaveRun run = wave_run(tab, block0 + tile * T + (uint64_t)(2 * (t - lane)), 128);
            decode_and_put<FMT>(run, run.first + lane, second ? az : ax, second ? aw : ay, 0, 0);
            decode_and_put<FMT>(run, run.first + 64 + lane, second ? bz : bx, second ? bw : by, 0, 0);
        } else {
            const WaveRun run = wave_run(tab, block0 + tile * T + (uint64_t)(t - lane), 64);
            decode_and_put<FMT>(run, run.first + lane, q.x, q.y, q.z, q.w);
        }
    }

    // the one ragged tile of a launch: its lanes look for themselves
    template <int FMT, int THREADS>
    __device__ __forceinline__ void store_edge(uint8_t*, uint64_t tile, int t, u32x4 q, int own) const
    {
        constexpr int T = tile_blocks(FMT, THREADS);
        if constexpr (FMT == kBc1) {
            const uint64_t first = block0 + tile * T + (uint64_t)(2 * t);
            decode_and_put<FMT>(no_wave_run(), first, q.x, q.y, 0, 0);
            if (2 * t + 1 < own)
                decode_and_put<FMT>(no_wave_run(), first + 1, q.z, q.w, 0, 0);
        } else {
            decode_and_put<FMT>(no_wave_run(), block0 + tile * T + (uint64_t)t, q.x, q.y, q.z, q.w);
        }
    }
};

// The same for BC4 / BC5.  A BC4 lane's two blocks may lie in two regions, or one of them in none: the 8-byte rows
// (store_channel_lane, rows8) are for two blocks of one region, otherwise each block goes alone.
template <typename TABLE>
struct RegionChannelSinkOf {
    TABLE tab;
    uint64_t block0;

    // the first `have` blocks of the lane's decoded vector, whose first block is block `b` of the buffer
    template <int FMT>
    __device__ __forceinline__ void put(const WaveRun& run, uint64_t b, const u32x2 (&w)[4], int have) const
    {
        if (run.region >= 0) {
            store_channel_lane<FMT>(run.img, run.local + (b - run.first), w, have);
            return;
        }
        ImageSink img{nullptr, 0, 1, 0, 0, (uint32_t)ChannelFormat<FMT>::bpp};
        uint64_t local = 0;
        const int r0 = region_of_block(tab, b, img, local);
        if constexpr (FMT == kBc4) {
            ImageSink img1 = img;
            uint64_t local1 = 0;
            const int r1 = have == 2 ? region_of_block(tab, b + 1, img1, local1) : -1;
            const bool together = r0 >= 0 && r1 == r0;
            if (r0 >= 0)
                store_channel_lane<FMT>(img, local, w, together ? 2 : 1);
            if (r1 >= 0 && !together) {
                const u32x2 second[4] = {u32x2{w[0].y, 0}, u32x2{w[1].y, 0}, u32x2{w[2].y, 0}, u32x2{w[3].y, 0}};
                store_channel_lane<FMT>(img1, local1, second, 1);
            }
        } else {
            if (r0 >= 0)
                store_channel_lane<FMT>(img, local, w, 1);
        }
    }

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store(uint8_t*, uint64_t tile, int t, u32x4 q) const
    {
        constexpr int T = tile_blocks(FMT, THREADS), PV = ChannelFormat<FMT>::per_vector;
        const int lane = t & 63;
        u32x2 w[4];
        decode_channel_vector<FMT>(q, w);
        const WaveRun run = wave_run(tab, block0 + tile * T + (uint64_t)(PV * (t - lane)), 64 * PV);
        put<FMT>(run, run.first + (uint64_t)(PV * lane), w, PV);
    }

    template <int FMT, int THREADS>
    __device__ __forceinline__ void store_edge(uint8_t*, uint64_t tile, int t, u32x4 q, int own) const
    {
        constexpr int T = tile_blocks(FMT, THREADS), PV = ChannelFormat<FMT>::per_vector;
        u32x2 w[4];
        decode_channel_vector<FMT>(q, w);
        put<FMT>(no_wave_run(), block0 + tile * T + (uint64_t)(PV * t), w, own - PV * t < PV ? own - PV * t : PV);
    }
};

}  // namespace dxtlt
