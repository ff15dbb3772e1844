// image_api.cpp -- C ABI of the image decoders (include/dxtlt_image.h): BC1 / BC2 / BC3 -> RGBA8888, BC4 / BC5 -> R8 / RG8; kernels
// in image_kernels.hip and, for several images of one buffer, image_regions_kernels.hip.  Every argument is checked before a device is
// touched.  The checks, the defects of a region list and the host-pointer paths are image_host.h's, which the BC7 and BC6H calls
// share; what is written here is a call's own checks (format, decorrelation mode) and its launcher.
#include <hip/hip_runtime.h>

#include "../../include/dxtlt_gfx950.h"
#include "../../include/dxtlt_image.h"
#include "host_common.h"
#include "image_host.h"
#include "image_launch.h"

using dxtlt_host::blocks_of;
using dxtlt_host::check_block_range;
using dxtlt_host::check_host_range;
using dxtlt_host::check_image;
using dxtlt_host::fail;
using dxtlt_host::for_each_region_group;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kOk;
using dxtlt_host::kRgba8888;
using dxtlt_host::pixel_rule;

namespace {

inline uint64_t block_bytes_of(int32_t fmt) { return fmt == 1 || fmt == 4 ? 8 : 16; }
// side `v` of a texture at mip level k
inline uint32_t mip_dim(uint32_t v, uint32_t k) { return k < 32 && (v >> k) > 0 ? v >> k : 1u; }

int32_t check_format(int32_t fmt)
{
    if (fmt < 1 || fmt > 3)
        return fail(kInvalidArgument, "format must be 1 (BC1), 2 (BC2) or 3 (BC3)");
    return kOk;
}

// (in front of the range check)
int32_t check_mode(uint8_t mode)
{
    if (mode > 3)
        return fail(kInvalidArgument, "decorrelation_mode must be 0..3");
    return kOk;
}

// ---- BC4 / BC5 -> R8 / RG8 ---------------------------------------------------------------------------------------------
int32_t check_channel_format(int32_t fmt)
{
    if (fmt != 4 && fmt != 5)
        return fail(kInvalidArgument, "format must be 4 (BC4) or 5 (BC5)");
    return kOk;
}

// ---- several images of one buffer --------------------------------------------------------------------------------------
// The checks of the image-region calls, in the documented order: the format first, the decorrelation mode (0 for the call that has
// none) last; *nothing = there is no non-empty region (DXTLT_OK, nothing to do)
int32_t check_regions(int32_t fmt, const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count,
                      uint8_t mode, bool* nothing)
{
    if (const char* defect = dxtlt_host::image_regions_defect(fmt, buffer, total_blocks, regions, count, mode, nothing))
        return fail(kInvalidArgument, defect);
    return kOk;
}

// the image of region i where the caller put it
inline dxtlt::ImageSink sink_of(const DxtltImageRegion& r, uint32_t bpp) { return dxtlt::make_image_sink(r.pixels, r.pitch, r.width, r.height, bpp); }

}  // namespace

extern "C" {

int32_t dxtlt_decode_image_device(int32_t format, const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels,
                                  uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(kRgba8888, d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_decode_image(format, d_blocks, dxtlt::make_image_sink(d_pixels, pitch, width, height),
                                       static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_image_device(int32_t format, const void* d_transformed, uint64_t total_blocks, uint64_t first_block,
                                              uint32_t width, uint32_t height, uint8_t decorrelation_mode,
                                              bool split_alpha_endpoints, bool split_colour_endpoints, void* d_pixels,
                                              uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(kRgba8888, d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_mode(decorrelation_mode); rc != kOk)
        return rc;
    if (int32_t rc = check_block_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    HIP_TRY(dxtlt::launch_untransform_decode_image(static_cast<dxtlt::Format>(format), s, d_transformed, total_blocks, first_block,
                                                   dxtlt::make_image_sink(d_pixels, pitch, width, height),
                                                   static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_image(int32_t format, const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width,
                                       uint32_t height, uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                       bool split_colour_endpoints, uint8_t* pixels, uint64_t pitch)
{
    if (int32_t rc = check_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(kRgba8888, transformed, pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_mode(decorrelation_mode); rc != kOk)
        return rc;
    const uint64_t bs = block_bytes_of(format);
    if (int32_t rc = check_host_range(len, bs, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    return dxtlt_host::untransform_decode_host_image(
        transformed, len, kRgba8888.bpp, width, height, pixels, pitch, [&](const void* d_in, const dxtlt::ImageSink& staged, hipStream_t st) {
            return dxtlt::launch_untransform_decode_image(static_cast<dxtlt::Format>(format), s, d_in, len / bs, first_block, staged, st);
        });
}

int32_t dxtlt_decode_channel_image_device(int32_t format, const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels,
                                          uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_channel_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(pixel_rule(format), d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_decode_channel_image(format, d_blocks,
                                               dxtlt::make_image_sink(d_pixels, pitch, width, height, pixel_rule(format).bpp),
                                               static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_channel_image_device(int32_t format, const void* d_transformed, uint64_t total_blocks,
                                                      uint64_t first_block, uint32_t width, uint32_t height, bool split_endpoints,
                                                      void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_channel_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(pixel_rule(format), d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_block_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_untransform_decode_channel_image(
                static_cast<dxtlt::Format>(format), split_endpoints, d_transformed, total_blocks, first_block,
                dxtlt::make_image_sink(d_pixels, pitch, width, height, pixel_rule(format).bpp), static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_channel_image(int32_t format, const uint8_t* transformed, size_t len, uint64_t first_block,
                                               uint32_t width, uint32_t height, bool split_endpoints, uint8_t* pixels, uint64_t pitch)
{
    if (int32_t rc = check_channel_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(pixel_rule(format), transformed, pixels, width, pitch); rc != kOk)
        return rc;
    const uint64_t bs = block_bytes_of(format);
    if (int32_t rc = check_host_range(len, bs, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    return dxtlt_host::untransform_decode_host_image(
        transformed, len, pixel_rule(format).bpp, width, height, pixels, pitch,
        [&](const void* d_in, const dxtlt::ImageSink& staged, hipStream_t st) {
            return dxtlt::launch_untransform_decode_channel_image(static_cast<dxtlt::Format>(format), split_endpoints, d_in, len / bs,
                                                                  first_block, staged, st);
        });
}

int32_t dxtlt_image_mip_level(uint32_t width, uint32_t height, uint32_t mip_count, uint32_t level, uint32_t* level_width,
                              uint32_t* level_height, uint64_t* first_block, uint64_t* num_blocks, uint64_t* total_blocks)
{
    if (width == 0 || height == 0 || mip_count == 0 || level >= mip_count)
        return fail(kInvalidArgument, "mip level: zero width, height or mip_count, or level >= mip_count");
    const auto dim = mip_dim;
    uint64_t before = 0, total = 0;
    // levels 32 and up are 1 x 1 = one block each, whatever the size
    const uint32_t walked = mip_count < 32 ? mip_count : 32;
    for (uint32_t k = 0; k < walked; ++k) {
        const uint64_t n = blocks_of(dim(width, k), dim(height, k));
        if (k < level)
            before += n;
        total += n;
    }
    total += mip_count - walked;
    if (level > walked)
        before += level - walked;
    if (level_width)
        *level_width = dim(width, level);
    if (level_height)
        *level_height = dim(height, level);
    if (first_block)
        *first_block = before;
    if (num_blocks)
        *num_blocks = blocks_of(dim(width, level), dim(height, level));
    if (total_blocks)
        *total_blocks = total;
    return kOk;
}

int32_t dxtlt_untransform_decode_images_device(int32_t format, const void* d_transformed, uint64_t total_blocks,
                                               const DxtltImageRegion* regions, size_t region_count, uint8_t decorrelation_mode,
                                               bool split_alpha_endpoints, bool split_colour_endpoints, void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(format, d_transformed, total_blocks, regions, region_count, decorrelation_mode, &nothing);
        rc != kOk || nothing)
        return rc;
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i], pixel_rule(format).bpp); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::launch_untransform_decode_image_regions(static_cast<dxtlt::Format>(format), s, d_transformed,
                                                                          total_blocks, tab, static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_decode_images_device(int32_t format, const void* d_blocks, uint64_t total_blocks, const DxtltImageRegion* regions,
                                   size_t region_count, void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(format, d_blocks, total_blocks, regions, region_count, 0, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i], pixel_rule(format).bpp); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::launch_decode_image_regions(format, d_blocks, total_blocks, tab, static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_images(int32_t format, const uint8_t* transformed, size_t len, const DxtltImageRegion* regions,
                                        size_t region_count, uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                        bool split_colour_endpoints)
{
    const uint64_t bs = block_bytes_of(format), total_blocks = len / bs;
    bool nothing = true;
    if (int32_t rc = check_regions(format, transformed, total_blocks, regions, region_count, decorrelation_mode, &nothing);
        rc != kOk || nothing)
        return rc;
    if (int32_t rc = dxtlt_host::check_len(len, bs); rc != kOk)
        return rc;
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    return dxtlt_host::untransform_decode_host_regions(
        transformed, len, regions, region_count, pixel_rule(format).bpp,
        [&](const void* d_in, const dxtlt::ImageRegionTable& tab, hipStream_t st) {
            return dxtlt::launch_untransform_decode_image_regions(static_cast<dxtlt::Format>(format), s, d_in, total_blocks, tab, st);
        });
}

int32_t dxtlt_image_mip_chain(uint32_t width, uint32_t height, uint32_t mip_count, uint64_t first_block, DxtltImageRegion* regions,
                              uint64_t* total_blocks)
{
    if (width == 0 || height == 0 || mip_count == 0 || regions == nullptr)
        return fail(kInvalidArgument, "mip chain: zero width, height or mip_count, or NULL regions");
    uint64_t at = first_block;
    for (uint32_t k = 0; k < mip_count; ++k) {
        regions[k].first_block = at;
        regions[k].width = mip_dim(width, k);
        regions[k].height = mip_dim(height, k);
        at += blocks_of(regions[k].width, regions[k].height);
    }
    if (total_blocks)
        *total_blocks = at;
    return kOk;
}

}  // extern "C"
