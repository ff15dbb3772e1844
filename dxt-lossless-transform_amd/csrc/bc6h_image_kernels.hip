// bc6h_image_kernels.hip -- BC6H blocks -> RGBA16F pixels on gfx950 (include/dxtlt_bc6h_image.h; docs/IMAGE_DECODE.md, "BC6H blocks
// to a row-major RGBA16F image"):
//   * decode_bc6h_blocks_kernel: a block array -> one 128-byte record per block, one block per lane;
//   * decode_bc6h_image_kernel: a block array in block order -> a row-major image, one block per lane, the clipping of the BC2 / BC3
//     plain decoder with 8 bytes per pixel and plain stores (store_block_pixels, bc6h_image_sinks.h);
//   * bc6h_inverse_image: the inverse granule sort (granule_sort.h over Bc6hCodec) with a staging sink (Bc6hPixelSink,
//     bc6h_image_sinks.h) in the place of its block store: the blocks are prepared in the sorted domain, where the class is
//     wave-uniform, and their pixels go through LDS to block order, so that the untransformed blocks never touch memory.
// The decoder is bc6h_decode.h.  Its mode switch is per lane in the first two kernels, which decode in BLOCK order (a wave runs the
// arm of every class that occurs among its 64 blocks), and wave-uniform in the third.
#include "bc6h_decode.h"
#include "bc6h_granule_codec.h"
#include "bc6h_image_launch.h"
#include "bc6h_image_sinks.h"
#include "image_store.h"
#include "launch_grid.h"

namespace dxtlt {
namespace bc6h {
namespace {

using granule::inverse_granule;
using granule::kT;

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

// ---- blocks in block order -> image, one block per lane ----------------------------------------------------------------
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc6h_image_kernel(const uint8_t* __restrict__ in, ImageSink img, uint64_t num_blocks)
{
    const uint64_t b = workgroup_index() * kThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
    store_block_pixels(img, b, prepare_q(load_block<ALIGNED>(in, b)));
}

// ---- the inverse granule sort with a pixel sink (Bc6hPixelSink, bc6h_image_sinks.h) ------------------------------------------
// Full granules: workgroup g is granule first_granule_block / 1024 + g of the main part (part_blocks blocks, soa = its byte 0).
// TAIL: one workgroup, soa = the tail part's byte 0, first_granule_block = the tail part's first block, n_tail its blocks.
template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc6h_inverse_image(const uint8_t* __restrict__ soa, Bc6hPixelSink<TAIL> sink, uint64_t part_blocks, uint64_t first_granule_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    inverse_granule<Bc6hCodec, LANES, TAIL, Bc6hPixelSink<TAIL>>(soa, nullptr, part_blocks, first_granule_block + granule * kT, n_tail, sink);
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

hipError_t launch_decode_image(const void* blocks, const ImageSink& img, hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_rows(n, kThreads, grid); e != hipSuccess)
        return e;
    const auto* in = static_cast<const uint8_t*>(blocks);
    hipLaunchKernelGGL(alignment_of(blocks) == 0 ? decode_bc6h_image_kernel<true> : decode_bc6h_image_kernel<false>, grid, dim3(kThreads), 0,
                       stream, in, img, n);
    return hipGetLastError();
}

hipError_t launch_untransform_decode_image(const void* soa_arg, uint64_t total_blocks, uint64_t first_block, const ImageSink& img,
                                           hipStream_t stream)
{
    const uint64_t n = image_blocks(img);
    if (n == 0)
        return hipSuccess;
    if (first_block > total_blocks || n > total_blocks - first_block)
        return hipErrorInvalidValue;
    const auto* soa = static_cast<const uint8_t*>(soa_arg);
    const uint64_t main_blocks = total_blocks - total_blocks % kT;
    const Bc6hPixelSink<false> sink{img, first_block, n};
    const Bc6hPixelSink<true> tail_sink{img, first_block, n};
    return granule::for_each_range_launch(total_blocks, first_block, first_block + n, [&](uint64_t granule, uint64_t granules, bool tail) {
        if (!tail) {
            hipLaunchKernelGGL((bc6h_inverse_image<256, false>), dim3((unsigned)granules), dim3(256), 0, stream, soa, sink, main_blocks,
                               granule * kT, 0);
        } else {
            const uint64_t n_tail = total_blocks - main_blocks;
            hipLaunchKernelGGL((bc6h_inverse_image<256, true>), dim3(1), dim3(256), 0, stream, soa + main_blocks * 16, tail_sink, n_tail,
                               main_blocks, (int)n_tail);
        }
        return hipGetLastError();
    });
}

}  // namespace bc6h
}  // namespace dxtlt
