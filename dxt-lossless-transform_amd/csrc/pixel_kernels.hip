// pixel_kernels.hip -- gfx950 kernels of the uncompressed-pixel transform, layout version 1 (docs/PIXEL_FORMAT.md): RGBA8888 and
// BGRA8888 (B = 4 bytes per pixel; byte 1 is G in both, so they are one transform) and BGR888 (B = 3).
//
// One workgroup of 256 lanes runs one tile of 4096 pixels: 16 KiB (B = 4) or 12 KiB (B = 3) of interleaved bytes, 4096 bytes of every
// plane -- exactly one PLANAR_DELTA segment per plane, so nothing is carried between workgroups.
//
//   interleaved side   the tile's bytes travel as 16-byte vectors, lane after lane (coalesced), and pass through LDS, where lane t
//                      owns pixels [16 t, 16 t + 16): 16 B contiguous bytes, B ds_read_b128 / ds_write_b128.  (Lane stride 48 bytes
//                      for B = 3: the sixteen lanes of a pass start in sixteen different banks.  64 bytes for B = 4: a 4-way
//                      conflict, 512 clocks per tile next to the ~2500 the tile's 32 KiB take at a CU's share of HBM.)
//   in registers       the 16 pixels are de-interleaved with v_perm_b32 into B plane vectors of 16 bytes; subtract-green is a
//                      byte-wise vector subtract of plane 1 from planes 0 and 2; the delta needs the pixel in front of the lane's
//                      first one, which it takes from the LDS image (B bytes).
//   planar side        lane t moves bytes [16 t, 16 t + 16) of every plane of the tile as ONE 16-byte vector: a wave instruction
//                      covers 1 KiB of one plane, and no store reaches past the tile's 4096 bytes of its plane, so it cannot spill
//                      into the next plane, which follows it directly in memory.
//   PLANAR_DELTA back  an inclusive prefix sum modulo 256 over the 4096 bytes of every plane: sixteen bytes in the lane (byte-wise
//                      adds on dwords), the lane totals of all B planes in ONE dword across the wave (__shfl_up, six steps), the
//                      four wave totals through LDS.
//
// Alignment.  Plane c of a buffer of P pixels starts at byte c P: every residue occurs, and a mip chain makes P odd.  16-byte
// vector accesses at unaligned global addresses are exact on gfx950 under ROCm's default memory mode and cost a few hundredths of
// peak (bcn_kernels.hip; tools/unaligned_lab.hip), so the same tile body serves every alignment: when both pointers and P are
// multiples of 16 every access is aligned (the fast form), otherwise the very same vectors are issued at the addresses they fall
// on (the general form).  What is not a whole vector -- only in the last, short tile of a range -- moves byte by byte, bounds
// checked: no access touches a byte outside the range's own.
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

template <int B, bool INVERSE, bool DECORRELATE, int LAYOUT>
__global__ void __launch_bounds__(kThreads)
pixel_tiles(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t total, uint64_t first, uint64_t num)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[B * kTile];
    __shared__ uint32_t wave_totals[kThreads / 64];
    const uint64_t tile_first = (uint64_t)blockIdx.x * kTile;   // inside the range
    const uint32_t n = (uint32_t)(num - tile_first < kTile ? num - tile_first : kTile);
    const uint32_t p0 = 16 * threadIdx.x;                       // the lane's first pixel inside the tile
    const uint32_t valid = p0 >= n ? 0 : (n - p0 < 16 ? n - p0 : 16);
    // where the tile lies on the transformed side: layout 0 keeps the pixels in place, else plane c starts at c * total
    const uint64_t at = first + tile_first;

    if constexpr (LAYOUT == kInterleaved) {
        stage_in(lds, INVERSE ? src + at * B : src + tile_first * B, n * B);
        if constexpr (DECORRELATE) {
            __syncthreads();
            if (valid != 0) {
                uint32_t w[4 * B], pl[B][4];
                lds_read_pixels<B>(lds, w);
                Pixels16<B>::deinterleave(w, pl);
                decorrelate_planes<B, INVERSE>(pl);
                Pixels16<B>::interleave(pl, w);
                lds_write_pixels<B>(lds, w);
            }
        }
        __syncthreads();
        stage_out(lds, INVERSE ? dst + tile_first * B : dst + at * B, n * B);
    } else if constexpr (!INVERSE) {
        stage_in(lds, src + tile_first * B, n * B);
        __syncthreads();
        if (valid != 0) {
            uint32_t w[4 * B], pl[B][4];
            lds_read_pixels<B>(lds, w);
            Pixels16<B>::deinterleave(w, pl);
            if constexpr (DECORRELATE)
                decorrelate_planes<B, false>(pl);
            if constexpr (LAYOUT == kPlanarDelta) {
                // the pixel in front of the lane's first: the last one of the lane in front; the segment's first byte stays
                uint32_t prev[B];
                for (int c = 0; c < B; ++c)
                    prev[c] = p0 == 0 ? 0u : lds[(p0 - 1) * B + c];
                if constexpr (DECORRELATE) {
                    prev[0] = (prev[0] - prev[1]) & 0xFF;
                    prev[2] = (prev[2] - prev[1]) & 0xFF;
                }
                for (int c = 0; c < B; ++c)
                    delta16(pl[c], prev[c]);
            }
            for (int c = 0; c < B; ++c)
                plane_store(dst + (uint64_t)c * total + at + p0, pl[c], valid);
        }
    } else {
        uint32_t w[4 * B], pl[B][4];
        for (int c = 0; c < B; ++c)
            plane_load(src + (uint64_t)c * total + at + p0, pl[c], valid);
        if constexpr (LAYOUT == kPlanarDelta)
            scan_planes<B>(pl, wave_totals);
        if constexpr (DECORRELATE)
            decorrelate_planes<B, true>(pl);
        Pixels16<B>::interleave(pl, w);
        lds_write_pixels<B>(lds, w);
        __syncthreads();
        stage_out(lds, dst + tile_first * B, n * B);
    }
}

template <int B, bool INVERSE, bool DECORRELATE>
hipError_t launch_layout(int layout, const uint8_t* src, uint8_t* dst, uint64_t total, uint64_t first, uint64_t num, hipStream_t stream)
{
    const dim3 grid((uint32_t)((num + kTile - 1) / kTile)), block(kThreads);
    switch (layout) {
    case kInterleaved:
        hipLaunchKernelGGL((pixel_tiles<B, INVERSE, DECORRELATE, kInterleaved>), grid, block, 0, stream, src, dst, total, first, num);
        break;
    case kPlanar:
        hipLaunchKernelGGL((pixel_tiles<B, INVERSE, DECORRELATE, kPlanar>), grid, block, 0, stream, src, dst, total, first, num);
        break;
    case kPlanarDelta:
        hipLaunchKernelGGL((pixel_tiles<B, INVERSE, DECORRELATE, kPlanarDelta>), grid, block, 0, stream, src, dst, total, first, num);
        break;
    default:
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

template <int B>
hipError_t launch_bytes(bool inverse, bool decorrelate, int layout, const uint8_t* src, uint8_t* dst, uint64_t total, uint64_t first,
                        uint64_t num, hipStream_t stream)
{
    if (inverse)
        return decorrelate ? launch_layout<B, true, true>(layout, src, dst, total, first, num, stream)
                           : launch_layout<B, true, false>(layout, src, dst, total, first, num, stream);
    return decorrelate ? launch_layout<B, false, true>(layout, src, dst, total, first, num, stream)
                       : launch_layout<B, false, false>(layout, src, dst, total, first, num, stream);
}

}  // namespace

hipError_t launch_range(int pixel_bytes, bool inverse, bool decorrelate, int layout, const void* src, void* dst, uint64_t total,
                        uint64_t first, uint64_t num, hipStream_t stream)
{
    if (num == 0)
        return hipSuccess;
    // one workgroup per tile in grid.x: fewer than 2^31 tiles (32 TiB of 4-byte pixels)
    if ((pixel_bytes != 3 && pixel_bytes != 4) || layout < 0 || layout > 2 || src == nullptr || dst == nullptr || first % kTile != 0 ||
        first > total || num > total - first || (num + kTile - 1) / kTile > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* d = static_cast<uint8_t*>(dst);
    return pixel_bytes == 4 ? launch_bytes<4>(inverse, decorrelate, layout, s, d, total, first, num, stream)
                            : launch_bytes<3>(inverse, decorrelate, layout, s, d, total, first, num, stream);
}

}  // namespace pixels
}  // namespace dxtlt
