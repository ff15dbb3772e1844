// bc7_image_kernels.hip -- BC7 blocks -> RGBA8888 pixels on gfx950 (include/dxtlt_bc7_image.h; docs/IMAGE_DECODE.md, "BC7").  The
// image kernels and their launchers are granule_image.h's, instantiated for Bc7Image (bc7_image_sinks.h): the ones of a single image
// here, the ones of several images in bc7_image_regions_kernels.hip.  What is BC7's own is the decoder of a block array:
//   * decode_bc7_blocks_kernel: a block array -> one 64-byte Decoded4x4Block per block, in the store shape of bcn_decode.hip (the
//     wave's 4 KiB of pixels through LDS, every store instruction 1 KiB of consecutive bytes);
//   * decode_bc7_blocks_bytes_kernel: the same for pixels of any alignment, byte stores.
// The decoder is bc7_decode.h; its mode switch is per lane here, as in the plain image decoders.
#include "bc7_image_sinks.h"
#include "granule_image.h"

namespace dxtlt {
namespace bc7 {
namespace {

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
        const unsigned pad = lds_pad_for_wgs_per_cu(6, kThreads, (unsigned)((kThreads / 64) * kWaveStage * 16));
        hipLaunchKernelGGL(a ? decode_bc7_blocks_kernel<true> : decode_bc7_blocks_kernel<false>, grid, dim3(kThreads), pad, stream, in, out,
                           num_blocks);
    } else {
        hipLaunchKernelGGL(a ? decode_bc7_blocks_bytes_kernel<true> : decode_bc7_blocks_bytes_kernel<false>, grid, dim3(kThreads), 0,
                           stream, in, out, num_blocks);
    }
    return hipGetLastError();
}

}  // namespace bc7

template hipError_t launch_decode_image<bc7::Bc7Image>(const void*, const ImageSink&, hipStream_t);
template hipError_t launch_untransform_decode_image<bc7::Bc7Image>(const void*, uint64_t, uint64_t, const ImageSink&, hipStream_t);

}  // namespace dxtlt
