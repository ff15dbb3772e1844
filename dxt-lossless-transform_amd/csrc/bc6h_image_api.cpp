// bc6h_image_api.cpp -- C ABI of the BC6H decoders (include/dxtlt_bc6h_image.h); kernels in bc6h_image_kernels.hip and, for several
// images of one buffer, bc6h_image_regions_kernels.hip; the decoder itself in bc6h_decode.h.  Every argument is checked before a
// device is touched.  The checks (an RGBA16F image, no format, no settings), the defects of a region list, the plan of the debug
// call and the host-pointer paths are image_host.h's.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/dxtlt_bc6h_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc6h_decode.h"
#include "bc6h_image_launch.h"
#include "host_common.h"
#include "image_host.h"

using dxtlt_host::blocks_of;
using dxtlt_host::check_block_range;
using dxtlt_host::check_image;
using dxtlt_host::fail;
using dxtlt_host::for_each_region_group;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kOk;
using dxtlt_host::kRgba16f;

namespace {

constexpr size_t kDecodedBlockBytes = 128;   // sixteen pixels of four halves

int32_t check_decode(const void* in, size_t len, const void* out, size_t out_len)
{
    return dxtlt_host::check_decode(in, len, 16, out, out_len, kDecodedBlockBytes, "pixels_len is smaller than 128 bytes per block");
}

// ---- several images of one buffer --------------------------------------------------------------------------------------
// the checks of the region calls, in the documented order; *nothing = there is no non-empty region (DXTLT_OK, nothing to do)
int32_t check_regions(const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count, bool* nothing)
{
    if (const char* defect = dxtlt_host::image_regions_defect(kRgba16f, buffer, total_blocks, regions, count, nothing))
        return fail(kInvalidArgument, defect);
    return kOk;
}

inline dxtlt::ImageSink sink_of(const DxtltImageRegion& r)
{
    return dxtlt::make_image_sink(r.pixels, r.pitch, r.width, r.height, kRgba16f.bpp);
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
    if (int32_t rc = check_image(kRgba16f, d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc6h::launch_decode_image(d_blocks, dxtlt::make_image_sink(d_pixels, pitch, width, height, kRgba16f.bpp),
                                             static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc6h_image_device(const void* d_transformed, uint64_t total_blocks, uint64_t first_block, uint32_t width,
                                                   uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(kRgba16f, d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_block_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc6h::launch_untransform_decode_image(d_transformed, total_blocks, first_block,
                                                         dxtlt::make_image_sink(d_pixels, pitch, width, height, kRgba16f.bpp),
                                                         static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc6h_image(const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width, uint32_t height,
                                            uint8_t* pixels, uint64_t pitch)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(kRgba16f, transformed, pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = dxtlt_host::check_host_range(len, 16, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    return dxtlt_host::untransform_decode_host_image(
        transformed, len, kRgba16f.bpp, width, height, pixels, pitch, [&](const void* d_in, const dxtlt::ImageSink& staged, hipStream_t st) {
            return dxtlt::bc6h::launch_untransform_decode_image(d_in, len / 16, first_block, staged, st);
        });
}

int32_t dxtlt_untransform_decode_bc6h_images_device(const void* d_transformed, uint64_t total_blocks, const DxtltImageRegion* regions,
                                                    size_t region_count, void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(d_transformed, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i]); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::bc6h::launch_untransform_decode_image_regions(d_transformed, total_blocks, tab,
                                                                                static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_decode_bc6h_images_device(const void* d_blocks, uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                        void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(d_blocks, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i]); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::bc6h::launch_decode_image_regions(d_blocks, total_blocks, tab, static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc6h_images(const uint8_t* transformed, size_t len, const DxtltImageRegion* regions, size_t region_count)
{
    const uint64_t total_blocks = len / 16;
    bool nothing = true;
    if (int32_t rc = check_regions(transformed, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    if (int32_t rc = dxtlt_host::check_len(len, 16); rc != kOk)
        return rc;
    return dxtlt_host::untransform_decode_host_regions(
        transformed, len, regions, region_count, kRgba16f.bpp, [&](const void* d_in, const dxtlt::ImageRegionTable& tab, hipStream_t st) {
            return dxtlt::bc6h::launch_untransform_decode_image_regions(d_in, total_blocks, tab, st);
        });
}

int32_t dxtlt_debug_plan_bc6h_images(uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                     DxtltBc6hImagesLaunch* out, size_t cap)
{
    // the arithmetic is the BC7 debug call's too (image_host.h)
    return dxtlt_host::plan_granule_region_launches(kRgba16f, total_blocks, regions, region_count, out, cap);
}

}  // extern "C"
