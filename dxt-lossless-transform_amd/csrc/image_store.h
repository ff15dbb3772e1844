// image_store.h -- device helpers shared by the image kernels (image_kernels.hip: one image per call;
// image_regions_kernels.hip: several images of one buffer; the BC7 and BC6H image kernels): a decoded block's sixteen pixels into
// their rows of an ImageSink (image_sink.h), and the 16-byte block load of the plain BC7 and BC6H decoders.  The notes on the store
// shapes are at the head of image_kernels.hip and at its "BC4 / BC5" section.
#pragma once
#include "bcn_decode.h"
#include "bcn_device.h"
#include "image_sink.h"

namespace dxtlt {
namespace {

typedef uint32_t u32x4_align4 __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4_align8 __attribute__((ext_vector_type(4), aligned(8)));

// 16-byte block `b` of a block array (the plain BC7 and BC6H decoders): a 16-byte load when the block pointer is a multiple of 16,
// byte loads otherwise
template <bool ALIGNED>
__device__ __forceinline__ u32x4 load_block(const uint8_t* __restrict__ in, uint64_t b)
{
    if constexpr (ALIGNED) {
        return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in) + b);
    } else {
        uint32_t q[4] = {0, 0, 0, 0};
        for (int i = 0; i < 16; ++i)
            q[i >> 2] |= (uint32_t)in[16 * b + i] << (8 * (i & 3));
        return u32x4{q[0], q[1], q[2], q[3]};
    }
}

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

// ---- BC4 / BC5: a lane's 16-byte vector is two BC4 blocks (2t, 2t + 1) or one BC5 block (image_kernels.hip, "BC4 / BC5") ----
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

}  // namespace
}  // namespace dxtlt
