// granule_image_api.h -- the bodies of the C ABI of the BC7 and BC6H image decoders (include/dxtlt_bc7_image.h,
// include/dxtlt_bc6h_image.h), written once over a host-side family H; bc7_image_api.cpp and bc6h_image_api.cpp name their family
// and forward every entry point to its body here.  A family holds
//   * rule: the PixelRule of its images (image_host.h);
//   * kDecodedBlockBytes, kTooSmall: the bytes of a decoded block and the error text that names them;
//   * decode_block(b, px): the CPU block decoder, kDecodedBlockBytes / 4 words;
//   * launch_decode_blocks, Launch: the block decoder's launcher and the image family of granule_image_launch.h.
// Every argument is checked before a device is touched, in the documented order (docs/IMAGE_DECODE.md, the public headers); the
// checks, the defects of a region list, the plan of the debug call and the host-pointer paths are image_host.h's.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>

#include "bc7_fields.h"   // B128
#include "granule_image_launch.h"
#include "host_common.h"
#include "image_host.h"

namespace dxtlt_host {
namespace granule_image {

template <typename H>
int32_t check_decode(const void* in, size_t len, const void* out, size_t out_len)
{
    return dxtlt_host::check_decode(in, len, 16, out, out_len, H::kDecodedBlockBytes, H::kTooSmall);
}

// on the CPU, with the decoder the kernels run: a record per block needs no device
template <typename H>
int32_t decode_blocks(const uint8_t* blocks, size_t len, uint8_t* pixels, size_t pixels_len)
{
    if (int32_t rc = check_decode<H>(blocks, len, pixels, pixels_len); rc != kOk)
        return rc;
    constexpr int kWords = (int)(H::kDecodedBlockBytes / 4);
    for (size_t i = 0; i < len / 16; ++i) {
        dxtlt::bc7::B128 b;
        std::memcpy(b.d, blocks + 16 * i, 16);
        uint32_t px[kWords];
        H::decode_block(b, px);
        for (int k = 0; k < kWords; ++k)
            for (int c = 0; c < 4; ++c)
                pixels[H::kDecodedBlockBytes * i + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
    }
    return kOk;
}

template <typename H>
int32_t decode_blocks_device(const void* d_blocks, size_t len, void* d_pixels, size_t pixels_len, void* hip_stream)
{
    if (int32_t rc = check_decode<H>(d_blocks, len, d_pixels, pixels_len); rc != kOk)
        return rc;
    HIP_TRY(H::launch_decode_blocks(d_blocks, d_pixels, len / 16, static_cast<hipStream_t>(hip_stream)), "kernel launch");
    return kOk;
}

template <typename H>
int32_t decode_image_device(const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(H::rule, d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_decode_image<typename H::Launch>(d_blocks, dxtlt::make_image_sink(d_pixels, pitch, width, height, H::rule.bpp),
                                                           static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

template <typename H>
int32_t untransform_decode_image_device(const void* d_transformed, uint64_t total_blocks, uint64_t first_block, uint32_t width,
                                        uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(H::rule, d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_block_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_untransform_decode_image<typename H::Launch>(d_transformed, total_blocks, first_block,
                                                                       dxtlt::make_image_sink(d_pixels, pitch, width, height, H::rule.bpp),
                                                                       static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

template <typename H>
int32_t untransform_decode_image(const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width, uint32_t height,
                                 uint8_t* pixels, uint64_t pitch)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(H::rule, transformed, pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_host_range(len, 16, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    return untransform_decode_host_image(
        transformed, len, H::rule.bpp, width, height, pixels, pitch, [&](const void* d_in, const dxtlt::ImageSink& staged, hipStream_t st) {
            return dxtlt::launch_untransform_decode_image<typename H::Launch>(d_in, len / 16, first_block, staged, st);
        });
}

// ---- several images of one buffer --------------------------------------------------------------------------------------
// the checks of the region calls, in the documented order; *nothing = there is no non-empty region (DXTLT_OK, nothing to do)
template <typename H>
int32_t check_regions(const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count, bool* nothing)
{
    if (const char* defect = image_regions_defect(H::rule, buffer, total_blocks, regions, count, nothing))
        return fail(kInvalidArgument, defect);
    return kOk;
}

// launch: launch_untransform_decode_image_regions for a transformed buffer, launch_decode_image_regions for a block array in block
// order
template <typename H>
int32_t decode_images_device(hipError_t (*launch)(const void*, uint64_t, const dxtlt::ImageRegionTable&, hipStream_t), const void* d_buffer,
                             uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count, void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions<H>(d_buffer, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count,
                [&](size_t i) {
                    return dxtlt::make_image_sink(regions[i].pixels, regions[i].pitch, regions[i].width, regions[i].height, H::rule.bpp);
                },
                [&](const dxtlt::ImageRegionTable& tab) { return launch(d_buffer, total_blocks, tab, static_cast<hipStream_t>(hip_stream)); }),
            "kernel launch");
    return kOk;
}

template <typename H>
int32_t untransform_decode_images(const uint8_t* transformed, size_t len, const DxtltImageRegion* regions, size_t region_count)
{
    const uint64_t total_blocks = len / 16;
    bool nothing = true;
    if (int32_t rc = check_regions<H>(transformed, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    if (int32_t rc = check_len(len, 16); rc != kOk)
        return rc;
    return untransform_decode_host_regions(
        transformed, len, regions, region_count, H::rule.bpp, [&](const void* d_in, const dxtlt::ImageRegionTable& tab, hipStream_t st) {
            return dxtlt::launch_untransform_decode_image_regions<typename H::Launch>(d_in, total_blocks, tab, st);
        });
}

}  // namespace granule_image
}  // namespace dxtlt_host
