// bc7_image_kernels.hip -- BC7 blocks -> RGBA8888 pixels on gfx950 (include/dxtlt_bc7_image.h; docs/IMAGE_DECODE.md, "BC7"):
//   * decode_bc7_blocks_kernel: a block array -> one 64-byte Decoded4x4Block per block, in the store shape of bcn_decode.hip (the
//     wave's 4 KiB of pixels through LDS, every store instruction 1 KiB of consecutive bytes);
//   * decode_bc7_image_kernel: a block array in block order -> a row-major image, one block per lane, the stores of the BC2 / BC3
//     plain decoder (store_block_pixels, image_store.h);
//   * bc7_inverse_image: the inverse granule sort (granule_sort.h over Bc7Codec) with a staging sink (Bc7PixelSink,
//     bc7_image_sinks.h) in the place of its block store: the blocks are decoded in the sorted domain, where the mode is
//     wave-uniform, and their pixels go through LDS to block order, so that the untransformed blocks never touch memory.
// The decoder is bc7_decode.h.  Its mode switch is per lane in the first two kernels, which decode in BLOCK order (a wave runs the
// arm of every mode that occurs among its 64 blocks: on a buffer of mixed modes they are bound by instruction issue, not by
// memory), and wave-uniform in the third.
#include "bc7_decode.h"
#include "bc7_granule_codec.h"
#include "bc7_image_launch.h"
#include "bc7_image_sinks.h"
#include "image_store.h"
#include "launch_grid.h"

namespace dxtlt {
namespace bc7 {
namespace {

using granule::inverse_granule;
using granule::kT;

constexpr int kThreads = 256;
constexpr int kRowStride = 64 + 4;            // u32x4 units: 64 lanes + 64 bytes of padding (bcn_decode.hip)
constexpr int kWaveStage = 4 * kRowStride;    // four pixel rows per wave

// ---- blocks -> Decoded4x4Block -----------------------------------------------------------------------------------------
// `out` is a multiple of 16
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc7_blocks_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t num_blocks)
{
    __shared__ u32x4 stage[(kThreads / 64) * kWaveStage];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t wave_first = workgroup_index() * kThreads + 64 * wave;
    const uint64_t b = wave_first + lane;
    u32x4* mine = stage + wave * kWaveStage;
    if (b < num_blocks) {
        uint32_t px[16];
        decode_px(load_block<ALIGNED>(in, b), px);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            mine[r * kRowStride + lane] = u32x4{px[4 * r], px[4 * r + 1], px[4 * r + 2], px[4 * r + 3]};
    }
    __syncthreads();
    u32x4* dst = reinterpret_cast<u32x4*>(out) + 4 * wave_first;   // 16-byte chunk j of the wave = block j / 4, row j % 4
    const uint64_t chunks = num_blocks > wave_first ? 4 * (num_blocks - wave_first) : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int j = 64 * k + lane;
        if ((uint64_t)j < chunks)
            store_streaming16(dst + j, mine[(j & 3) * kRowStride + (j >> 2)]);
    }
}

// any alignment of `out`: byte stores; one block per lane
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc7_blocks_bytes_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ out, uint64_t num_blocks)
{
    const uint64_t b = workgroup_index() * kThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
    uint32_t px[16];
    decode_px(load_block<ALIGNED>(in, b), px);
    uint8_t* o = out + 64 * b;
#pragma unroll
    for (int i = 0; i < 16; ++i)
        for (int c = 0; c < 4; ++c)
            o[4 * i + c] = (uint8_t)(px[i] >> (8 * c));
}

// ---- blocks in block order -> image, one block per lane ----------------------------------------------------------------
template <bool ALIGNED>
__global__ void __launch_bounds__(kThreads)
decode_bc7_image_kernel(const uint8_t* __restrict__ in, ImageSink img, uint64_t num_blocks)
{
    const uint64_t b = workgroup_index() * kThreads + threadIdx.x;
    if (b >= num_blocks)
        return;
    uint32_t px[16];
    decode_px(load_block<ALIGNED>(in, b), px);
    store_block_pixels(img, b, px);
}

// ---- the inverse granule sort with a pixel sink (Bc7PixelSink, bc7_image_sinks.h) -------------------------------------------
// Full granules: workgroup g is granule first_granule_block / 1024 + g of the main part (part_blocks blocks, soa = its byte 0).
// TAIL: one workgroup, soa = the tail part's byte 0, first_granule_block = the tail part's first block, n_tail its blocks.
template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc7_inverse_image(const uint8_t* __restrict__ soa, Bc7PixelSink sink, uint64_t part_blocks, uint64_t first_granule_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    inverse_granule<Bc7Codec, LANES, TAIL, Bc7PixelSink>(soa, nullptr, part_blocks, first_granule_block + granule * kT, n_tail, sink);
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

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
    const bool a = aligned16(blocks);
    if (aligned16(pixels)) {
        // six workgroups per CU, as the BC2 / BC3 block decoders (bcn_decode.hip, decode_fmt): the same 16 bytes in, 64 out
        const unsigned pad = lds_pad_for_wgs_per_cu(wgs_per_cu_or(6), kThreads, (unsigned)((kThreads / 64) * kWaveStage * 16));
        hipLaunchKernelGGL(a ? decode_bc7_blocks_kernel<true> : decode_bc7_blocks_kernel<false>, grid, dim3(kThreads), pad, stream, in, out,
                           num_blocks);
    } else {
        hipLaunchKernelGGL(a ? decode_bc7_blocks_bytes_kernel<true> : decode_bc7_blocks_bytes_kernel<false>, grid, dim3(kThreads), 0,
                           stream, in, out, num_blocks);
    }
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
    hipLaunchKernelGGL(aligned16(blocks) ? decode_bc7_image_kernel<true> : decode_bc7_image_kernel<false>, grid, dim3(kThreads), 0, stream,
                       in, img, n);
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
    const Bc7PixelSink sink{img, first_block, n};
    return granule::for_each_range_launch(total_blocks, first_block, first_block + n, [&](uint64_t granule, uint64_t granules, bool tail) {
        if (!tail) {
            hipLaunchKernelGGL((bc7_inverse_image<256, false>), dim3((unsigned)granules), dim3(256), 0, stream, soa, sink, main_blocks,
                               granule * kT, 0);
        } else {
            const uint64_t n_tail = total_blocks - main_blocks;
            hipLaunchKernelGGL((bc7_inverse_image<256, true>), dim3(1), dim3(256), 0, stream, soa + main_blocks * 16, sink, n_tail,
                               main_blocks, (int)n_tail);
        }
        return hipGetLastError();
    });
}

}  // namespace bc7
}  // namespace dxtlt
