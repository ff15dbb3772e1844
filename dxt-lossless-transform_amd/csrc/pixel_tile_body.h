// pixel_tile_body.h -- what ONE workgroup of the uncompressed-pixel kernels does with ONE tile of 4096 pixels, written once: the
// tile of the transform (pixel_kernels.hip: one buffer per launch; pixel_batch_kernels.hip: many buffers per launch, the buffer
// looked up per workgroup) and the tile of the auto transform's five candidates (pixel_auto_kernels.hip; pixel_batch_kernels.hip).
// pixel_kernels.hip explains the tile -- LDS image, planes in registers, the alignment rule; device code only.
#pragma once
#include <hip/hip_runtime.h>

#include "pixel_device.h"
#include "pixel_launch.h"
#include "pixel_tile_io.h"

namespace dxtlt {
namespace pixels {
namespace {

// Inclusive prefix sum over the tile's 4096 bytes of every plane; lane t holds bytes [16 t, 16 t + 16) of each.
template <int B>
__device__ __forceinline__ void scan_planes(uint32_t (&pl)[B][4], uint32_t* wave_totals)
{
    // in the lane; the B lane totals share one dword, a byte each
    uint32_t totals = 0;
    for (int c = 0; c < B; ++c)
        totals |= scan16(pl[c]) << (8 * c);
    // across the wave: inclusive, then the lane in front's value is what this lane has to add
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t incl = totals;
    for (int d = 1; d < 64; d *= 2) {
        const uint32_t up = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d)
            incl = byte_add(incl, up);
    }
    uint32_t before = __shfl_up(incl, 1, 64);
    if (lane == 0)
        before = 0;
    // across the four waves
    if (lane == 63)
        wave_totals[wave] = incl;
    __syncthreads();
    for (uint32_t w = 0; w < wave; ++w)
        before = byte_add(before, wave_totals[w]);
    for (int c = 0; c < B; ++c)
        add_to_all16(pl[c], (before >> (8 * c)) & 0xFF);
}

// Tile `tile` of pixels [first, first + num) of a buffer of `total` pixels (launch_range's arguments; the caller has made sure that
// the tile exists: tile * kTile < num), as every lane of the workgroup runs it.  Expanded inside a kernel template with the
// parameters B, INVERSE, DECORRELATE and LAYOUT and with the kernel's LDS in scope: `lds`, B * kTile bytes on a 16-byte boundary,
// and `wave_totals`, kThreads / 64 dwords.  A macro, not a function (as DXTLT_ESTIMATE_WINDOW_OF, estimate_sections.h): the code of
// pixel_tiles is pinned, and through a __forceinline__ template -- LDS passed by pointer, by array reference or declared inside,
// with or without __restrict__ -- hipcc emitted other instructions for the inverse PLANAR_DELTA kernels and for pixel_candidates;
// expanded in place the statements compile to the code they always did.  The arguments are names, members or literals.
#define DXTLT_PIXEL_TILE(src, dst, total, first, num, tile) \
    do {                                                                                                                           \
        const uint64_t tile_first = (uint64_t)(tile) * kTile; /* inside the range */                                               \
        const uint32_t n = (uint32_t)(num - tile_first < kTile ? num - tile_first : kTile);                                        \
        const uint32_t p0 = 16 * threadIdx.x; /* the lane's first pixel inside the tile */                                         \
        const uint32_t valid = p0 >= n ? 0 : (n - p0 < 16 ? n - p0 : 16);                                                          \
        /* where the tile lies on the transformed side: layout 0 keeps the pixels in place, else plane c starts at c * total */    \
        const uint64_t at = first + tile_first;                                                                                    \
                                                                                                                                   \
        if constexpr (LAYOUT == kInterleaved) {                                                                                    \
            stage_in(lds, INVERSE ? src + at * B : src + tile_first * B, n * B);                                                   \
            if constexpr (DECORRELATE) {                                                                                           \
                __syncthreads();                                                                                                   \
                if (valid != 0) {                                                                                                  \
                    uint32_t w[4 * B], pl[B][4];                                                                                   \
                    lds_read_pixels<B>(lds, w);                                                                                    \
                    Pixels16<B>::deinterleave(w, pl);                                                                              \
                    decorrelate_planes<B, INVERSE>(pl);                                                                            \
                    Pixels16<B>::interleave(pl, w);                                                                                \
                    lds_write_pixels<B>(lds, w);                                                                                   \
                }                                                                                                                  \
            }                                                                                                                      \
            __syncthreads();                                                                                                       \
            stage_out(lds, INVERSE ? dst + tile_first * B : dst + at * B, n * B);                                                  \
        } else if constexpr (!INVERSE) {                                                                                           \
            stage_in(lds, src + tile_first * B, n * B);                                                                            \
            __syncthreads();                                                                                                       \
            if (valid != 0) {                                                                                                      \
                uint32_t w[4 * B], pl[B][4];                                                                                       \
                lds_read_pixels<B>(lds, w);                                                                                        \
                Pixels16<B>::deinterleave(w, pl);                                                                                  \
                if constexpr (DECORRELATE)                                                                                         \
                    decorrelate_planes<B, false>(pl);                                                                              \
                if constexpr (LAYOUT == kPlanarDelta) {                                                                            \
                    /* the pixel in front of the lane's first: the last of the lane in front; a segment's first byte stays */    \
                    uint32_t prev[B];                                                                                              \
                    for (int c = 0; c < B; ++c)                                                                                    \
                        prev[c] = p0 == 0 ? 0u : lds[(p0 - 1) * B + c];                                                            \
                    if constexpr (DECORRELATE) {                                                                                   \
                        prev[0] = (prev[0] - prev[1]) & 0xFF;                                                                      \
                        prev[2] = (prev[2] - prev[1]) & 0xFF;                                                                      \
                    }                                                                                                              \
                    for (int c = 0; c < B; ++c)                                                                                    \
                        delta16(pl[c], prev[c]);                                                                                   \
                }                                                                                                                  \
                for (int c = 0; c < B; ++c)                                                                                        \
                    plane_store(dst + (uint64_t)c * total + at + p0, pl[c], valid);                                                \
            }                                                                                                                      \
        } else {                                                                                                                   \
            uint32_t w[4 * B], pl[B][4];                                                                                           \
            for (int c = 0; c < B; ++c)                                                                                            \
                plane_load(src + (uint64_t)c * total + at + p0, pl[c], valid);                                                     \
            if constexpr (LAYOUT == kPlanarDelta)                                                                                  \
                scan_planes<B>(pl, wave_totals);                                                                                   \
            if constexpr (DECORRELATE)                                                                                             \
                decorrelate_planes<B, true>(pl);                                                                                   \
            Pixels16<B>::interleave(pl, w);                                                                                        \
            lds_write_pixels<B>(lds, w);                                                                                           \
            __syncthreads();                                                                                                       \
            stage_out(lds, dst + tile_first * B, n * B);                                                                           \
        }                                                                                                                          \
    } while (0)

// Tile `tile` of the five candidates of the auto transform (pixel_auto_kernels.hip has the order and the steps): from the `total`
// pixels at `src`, candidate i at arena + i * total * B.  tile * kTile < total; B and `lds` in scope as above.
#define DXTLT_PIXEL_CANDIDATES_TILE(src, arena, total, tile) \
    do {                                                                                                                   \
        const uint64_t tile_first = (uint64_t)(tile) * kTile;                                                              \
        const uint32_t n = (uint32_t)(total - tile_first < kTile ? total - tile_first : kTile);                            \
        const uint32_t p0 = 16 * threadIdx.x; /* the lane's first pixel inside the tile */                                 \
        const uint32_t valid = p0 >= n ? 0 : (n - p0 < 16 ? n - p0 : 16);                                                  \
        const uint64_t len = total * B;                                                                                    \
        auto planes_of = [&](int candidate) { return arena + (uint64_t)candidate * len + tile_first + p0; };               \
                                                                                                                           \
        stage_in(lds, src + tile_first * B, n * B);                                                                        \
        __syncthreads();                                                                                                   \
        uint32_t w[4 * B];                                                                                                 \
        if (valid != 0) {                                                                                                  \
            uint32_t pl[B][4], prev[B];                                                                                    \
            lds_read_pixels<B>(lds, w);                                                                                    \
            Pixels16<B>::deinterleave(w, pl);                                                                              \
            /* the pixel in front of the lane's first: the last of the lane in front; a segment's first byte stays */    \
            for (int c = 0; c < B; ++c)                                                                                    \
                prev[c] = p0 == 0 ? 0u : lds[(p0 - 1) * B + c];                                                            \
            for (int c = 0; c < B; ++c)                                                                                    \
                plane_store(planes_of(4) + (uint64_t)c * total, pl[c], valid);                                             \
            for (int c = 0; c < B; ++c) {                                                                                  \
                uint32_t d[4] = {pl[c][0], pl[c][1], pl[c][2], pl[c][3]};                                                  \
                delta16(d, prev[c]);                                                                                       \
                plane_store(planes_of(3) + (uint64_t)c * total, d, valid);                                                 \
            }                                                                                                              \
            decorrelate_planes<B, false>(pl);                                                                              \
            prev[0] = (prev[0] - prev[1]) & 0xFF;                                                                          \
            prev[2] = (prev[2] - prev[1]) & 0xFF;                                                                          \
            for (int c = 0; c < B; ++c)                                                                                    \
                plane_store(planes_of(1) + (uint64_t)c * total, pl[c], valid);                                             \
            Pixels16<B>::interleave(pl, w);                                                                                \
            for (int c = 0; c < B; ++c) {                                                                                  \
                delta16(pl[c], prev[c]);                                                                                   \
                plane_store(planes_of(0) + (uint64_t)c * total, pl[c], valid);                                             \
            }                                                                                                              \
        }                                                                                                                  \
        __syncthreads(); /* every lane has read its pixels and the one in front of them */                                 \
        if (valid != 0)                                                                                                    \
            lds_write_pixels<B>(lds, w);                                                                                   \
        __syncthreads();                                                                                                   \
        stage_out(lds, arena + 2 * len + tile_first * B, n * B);                                                           \
    } while (0)

}  // namespace
}  // namespace pixels
}  // namespace dxtlt
