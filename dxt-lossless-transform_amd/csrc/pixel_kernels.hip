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

#include "pixel_launch.h"
#include "pixel_tile_body.h"

namespace dxtlt {
namespace pixels {
namespace {

// one tile per workgroup: pixel_tile (pixel_tile_body.h), which the batch kernels of pixel_batch_kernels.hip run too
template <int B, bool INVERSE, bool DECORRELATE, int LAYOUT>
__global__ void __launch_bounds__(kThreads)
pixel_tiles(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, uint64_t total, uint64_t first, uint64_t num)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[B * kTile];
    __shared__ uint32_t wave_totals[kThreads / 64];
    DXTLT_PIXEL_TILE(src, dst, total, first, num, blockIdx.x);
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
