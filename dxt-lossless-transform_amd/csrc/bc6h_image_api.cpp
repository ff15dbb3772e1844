// bc6h_image_api.cpp -- C ABI of the BC6H decoders (include/dxtlt_bc6h_image.h); kernels in bc6h_image_kernels.hip, the decoder
// itself in bc6h_decode.h.  Every argument is checked before a device is touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/dxtlt_bc6h_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc6h_decode.h"
#include "bc6h_image_launch.h"
#include "host_common.h"

using dxtlt_host::fail;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kInvalidLength;
using dxtlt_host::kOk;

namespace {

constexpr size_t kDecodedBlockBytes = 128;   // sixteen pixels of four halves
constexpr uint32_t kBpp = 8;

inline uint64_t blocks_of(uint32_t width, uint32_t height) { return (((uint64_t)width + 3) / 4) * (((uint64_t)height + 3) / 4); }

// as dxtlt_decode_bc7_blocks* (bc7_image_api.cpp)
int32_t check_decode(const void* in, size_t len, const void* out, size_t out_len)
{
    if (len % 16 != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");
    const size_t n = len / 16;
    if (n > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    if (out_len / kDecodedBlockBytes < n)
        return fail(kInvalidArgument, "pixels_len is smaller than 128 bytes per block");
    return kOk;
}

// the checks of a non-empty image, in the documented order (the BC7 image calls', bc7_image_api.cpp, with 8 bytes per pixel)
int32_t check_image(const void* blocks, const void* pixels, uint32_t width, uint64_t pitch)
{
    if (blocks == nullptr || pixels == nullptr)
        return fail(kInvalidArgument, "NULL pointer with a non-empty image");
    if (pitch < kBpp * (uint64_t)width)
        return fail(kInvalidArgument, "pitch is smaller than 8 * width");
    if ((pitch & 7) != 0 || (reinterpret_cast<uintptr_t>(pixels) & 7) != 0)
        return fail(kInvalidArgument, "pitch and the pixel pointer must be multiples of 8");
    return kOk;
}

int32_t check_range(uint64_t total_blocks, uint64_t first_block, uint64_t blocks)
{
    if (first_block > total_blocks || blocks > total_blocks - first_block)
        return fail(kInvalidArgument, "first_block + blocks of the image exceeds total_blocks");
    return kOk;
}

}  // namespace

extern "C" {

int32_t dxtlt_decode_bc6h_blocks(const uint8_t* blocks, size_t len, uint8_t* pixels, size_t pixels_len)
{
    if (int32_t rc = check_decode(blocks, len, pixels, pixels_len); rc != kOk)
        return rc;
    // on the CPU, with the decoder the kernels run (bc6h_decode.h): a record per block needs no device
    for (size_t i = 0; i < len / 16; ++i) {
        dxtlt::bc7::B128 b;
        std::memcpy(b.d, blocks + 16 * i, 16);
        uint32_t px[32];
        dxtlt::bc6h::decode_bc6h_block(b, px);
        for (int k = 0; k < 32; ++k)
            for (int c = 0; c < 4; ++c)
                pixels[kDecodedBlockBytes * i + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
    }
    return kOk;
}

int32_t dxtlt_decode_bc6h_blocks_device(const void* d_blocks, size_t len, void* d_pixels, size_t pixels_len, void* hip_stream)
{
    if (int32_t rc = check_decode(d_blocks, len, d_pixels, pixels_len); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc6h::launch_decode_blocks(d_blocks, d_pixels, len / 16, static_cast<hipStream_t>(hip_stream)), "kernel launch");
    return kOk;
}

int32_t dxtlt_decode_bc6h_image_device(const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels, uint64_t pitch,
                                       void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc6h::launch_decode_image(d_blocks, dxtlt::make_image_sink(d_pixels, pitch, width, height, kBpp),
                                             static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc6h_image_device(const void* d_transformed, uint64_t total_blocks, uint64_t first_block, uint32_t width,
                                                   uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc6h::launch_untransform_decode_image(d_transformed, total_blocks, first_block,
                                                         dxtlt::make_image_sink(d_pixels, pitch, width, height, kBpp),
                                                         static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc6h_image(const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width, uint32_t height,
                                            uint8_t* pixels, uint64_t pitch)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(transformed, pixels, width, pitch); rc != kOk)
        return rc;
    const uint64_t total_blocks = len / 16;
    if (int32_t rc = check_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    if (len % 16 != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");

    // as dxtlt_untransform_decode_bc7_image: one upload, the device call into rows a multiple of 16 bytes apart, one download of the
    // rows
    const uint64_t row_bytes = kBpp * (uint64_t)width, d_pitch = (row_bytes + 15) & ~(uint64_t)15;
    const uint64_t need = std::max<uint64_t>(len, d_pitch * height);
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)need, &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    HIP_TRY(dxtlt::bc6h::launch_untransform_decode_image(d_in, total_blocks, first_block,
                                                         dxtlt::make_image_sink(d_out, d_pitch, width, height, kBpp), st),
            "kernel launch");
    HIP_TRY(hipMemcpy2DAsync(pixels, pitch, d_out, d_pitch, row_bytes, height, hipMemcpyDeviceToHost, st), "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

}  // extern "C"
