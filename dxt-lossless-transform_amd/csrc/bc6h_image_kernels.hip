// bc6h_image_kernels.hip -- BC6H blocks -> RGBA16F pixels on gfx950 (include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "BC6H blocks
// to a row-major RGBA16F image" and "Several images of one BC6H buffer").  The image kernels and their launchers are
// granule_image.h's, instantiated here for Bc6hImage (bc6h_image_sinks.h); what is BC6H's own is the decoder of a block array:
//   * decode_bc6h_blocks_kernel: a block array -> one 128-byte record per block, one block per lane.
// The decoder is bc6h_decode.h; its mode switch is per lane here, as in the plain image decoders.
#include "bc6h_image_sinks.h"
#include "granule_image.h"

namespace dxtlt {
namespace bc6h {
namespace {

constexpr int kThreads = 256;

// ---- blocks -> 128-byte records ----------------------------------------------------------------------------------------------
// A record is the block's own 4 x 4 image at a pitch of 32 bytes.  VECTOR: `out` is a multiple of 8 -- plain 16-byte stores (a lane
// fills its record's 128-byte line over eight instructions: no `sc1 nt`, see store_block_row); otherwise byte stores.
template <bool ALIGNED, bool VECTOR>
__global__ void __launch_bounds__(kThreads)
decode_bc6h_blocks_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t num_blocks)
{
    const uint64_t b = workgroup_index() * kThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
    const Interp s = prepare_q(load_block<ALIGNED>(in, b));
    uint8_t* o = out + 128 * b;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        uint32_t px[8];
        row_pixels(s, r, px);
        if constexpr (VECTOR) {
            *reinterpret_cast<u32x4_align8*>(o + 32 * r) = u32x4{px[0], px[1], px[2], px[3]};
            *reinterpret_cast<u32x4_align8*>(o + 32 * r + 16) = u32x4{px[4], px[5], px[6], px[7]};
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k)
                for (int c = 0; c < 4; ++c)
                    o[32 * r + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
        }
    }
}

inline unsigned alignment_of(const void* p) { return (unsigned)(reinterpret_cast<uintptr_t>(p) & 15); }

}  // namespace

hipError_t launch_decode_blocks(const void* blocks, void* pixels, uint64_t num_blocks, hipStream_t stream)
{
    if (num_blocks == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_rows(num_blocks, kThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    auto* out = static_cast<uint8_t*>(pixels);
    const bool a = alignment_of(blocks) == 0;
    const unsigned o = alignment_of(pixels);
    void (*kernel)(const uint8_t*, uint8_t*, uint64_t) =
        o % 8 == 0 ? (a ? decode_bc6h_blocks_kernel<true, true> : decode_bc6h_blocks_kernel<false, true>)
                   : (a ? decode_bc6h_blocks_kernel<true, false> : decode_bc6h_blocks_kernel<false, false>);
    hipLaunchKernelGGL(kernel, grid, dim3(kThreads), 0, stream, in, out, num_blocks);
    return hipGetLastError();
}

}  // namespace bc6h

template hipError_t launch_decode_image<bc6h::Bc6hImage>(const void*, const ImageSink&, hipStream_t);
template hipError_t launch_untransform_decode_image<bc6h::Bc6hImage>(const void*, uint64_t, uint64_t, const ImageSink&, hipStream_t);
template hipError_t launch_decode_image_regions<bc6h::Bc6hImage>(const void*, uint64_t, const ImageRegionTable&, hipStream_t);
template hipError_t launch_untransform_decode_image_regions<bc6h::Bc6hImage>(const void*, uint64_t, const ImageRegionTable&, hipStream_t);

}  // namespace dxtlt
