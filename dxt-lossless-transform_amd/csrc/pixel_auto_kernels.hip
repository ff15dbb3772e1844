// pixel_auto_kernels.hip -- the fused candidate kernel of the pixel auto transform (pixel_auto_api.cpp; docs/PIXEL_FORMAT.md "The
// auto transform"): ONE read of the input writes the five candidates that are not the input itself side by side into the arena,
// candidate i of the order at arena + i * len:
//     0 (decorrelate, PLANAR_DELTA)   1 (decorrelate, PLANAR)   2 (decorrelate, INTERLEAVED)   3 (plain, PLANAR_DELTA)   4 (plain, PLANAR)
// byte for byte what dxtlt_transform_pixels_device writes for those settings.  (plain, INTERLEAVED) is the input.
//
// The tile of pixel_kernels.hip's forward kernels: one workgroup of 256 lanes per 4096 pixels -- one PLANAR_DELTA segment of every
// plane, so nothing is carried between workgroups -- staged through LDS, where lane t owns pixels [16 t, 16 t + 16) and takes the
// pixel in front of its first one for the deltas.  In registers the sixteen pixels become planes once (pixel_device.h); the planes
// are stored (4), their deltas (3), then subtract-green and the same two stores (1, 0); the decorrelated pixels, interleaved
// again, go back into the lane's place in the LDS image once every lane has read it, and leave as the tile's vectors (2).
// The input must be on a 16-byte boundary for the staging vectors to be aligned loads (the caller's route condition); the arena
// slices start wherever i * len falls: the stores are the same vectors at those addresses, single bytes in the last, short tile.
#include <hip/hip_runtime.h>

#include "pixel_launch.h"
#include "pixel_tile_body.h"

namespace dxtlt {
namespace pixels {
namespace {

// one tile per workgroup: pixel_candidates_tile (pixel_tile_body.h), which pixel_batch_candidates (pixel_batch_kernels.hip) runs too
template <int B>
__global__ void __launch_bounds__(kThreads) pixel_candidates(const uint8_t* __restrict__ src, uint8_t* __restrict__ arena, uint64_t total)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[B * kTile];
    DXTLT_PIXEL_CANDIDATES_TILE(src, arena, total, blockIdx.x);
}

}  // namespace

hipError_t launch_auto_candidates(int pixel_bytes, const void* src, void* arena, uint64_t total, hipStream_t stream)
{
    if (total == 0)
        return hipSuccess;
    if ((pixel_bytes != 3 && pixel_bytes != 4) || src == nullptr || arena == nullptr || (total + kTile - 1) / kTile > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((total + kTile - 1) / kTile)), block(kThreads);
    const uint8_t* s = static_cast<const uint8_t*>(src);
    uint8_t* a = static_cast<uint8_t*>(arena);
    if (pixel_bytes == 4)
        hipLaunchKernelGGL(pixel_candidates<4>, grid, block, 0, stream, s, a, total);
    else
        hipLaunchKernelGGL(pixel_candidates<3>, grid, block, 0, stream, s, a, total);
    return hipGetLastError();
}

}  // namespace pixels
}  // namespace dxtlt
