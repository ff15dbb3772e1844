// image_api.cpp -- C ABI of the image decoders (include/dxtlt_image.h): BC1 / BC2 / BC3 -> RGBA8888, BC4 / BC5 -> R8 / RG8; kernels
// in image_kernels.hip and, for several images of one buffer, image_regions_kernels.hip.  Every argument is checked before a device is touched.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dxtlt_gfx950.h"
#include "../../include/dxtlt_image.h"
#include "host_common.h"
#include "image_launch.h"
#include "image_region_groups.h"

using dxtlt_host::empty_region;
using dxtlt_host::fail;
using dxtlt_host::for_each_region_group;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kInvalidLength;
using dxtlt_host::kOk;

// The first defect of an image-region call's arguments in the documented order -- all of them DXTLT_E_INVALID_ARGUMENT -- or
// nullptr; *nothing = there is no non-empty region.  (image_launch.h: the batch call runs the same checks per item; the BC7
// region calls, which have no format argument and no settings, pass bc7.)
const char* dxtlt_host::image_regions_defect(int32_t fmt, const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions,
                                             size_t count, uint8_t mode, bool* nothing, bool bc7)
{
    *nothing = true;
    if (!bc7 && (fmt < 1 || fmt > 5))
        return "format must be 1 (BC1) .. 5 (BC5)";
    if (count == 0)
        return nullptr;
    if (regions == nullptr)
        return "NULL regions pointer";
    for (size_t i = 0; i < count && *nothing; ++i)
        *nothing = regions[i].width == 0 || regions[i].height == 0;
    if (*nothing)
        return nullptr;
    if (buffer == nullptr)
        return "NULL buffer with a non-empty region";
    const uint64_t bpp = bc7 || fmt <= 3 ? 4 : fmt == 4 ? 1 : 2, multiple = bc7 || fmt <= 3 ? 4 : bpp;
    auto blocks_of = [](uint32_t width, uint32_t height) { return (((uint64_t)width + 3) / 4) * (((uint64_t)height + 3) / 4); };
    uint64_t end = 0;   // of the previous non-empty region
    for (size_t i = 0; i < count; ++i) {
        const DxtltImageRegion& r = regions[i];
        if (r.width == 0 || r.height == 0)
            continue;
        if (r.pixels == nullptr)
            return "NULL pixels pointer of a non-empty region";
        if (r.pitch < bpp * (uint64_t)r.width)
            return "a region's pitch is smaller than the bytes of a pixel row";
        if (r.pitch % multiple != 0 || reinterpret_cast<uintptr_t>(r.pixels) % multiple != 0)
            return "a region's pitch and pixel pointer must be multiples of 4 (BC1 - BC3) or of the bytes per pixel";
        if (r.first_block > total_blocks || blocks_of(r.width, r.height) > total_blocks - r.first_block)
            return "first_block + blocks of a region exceeds total_blocks";
        if (r.first_block < end)
            return "regions must come in ascending block order and must not overlap";
        end = r.first_block + blocks_of(r.width, r.height);
    }
    if (!bc7 && fmt <= 3 && mode > 3)
        return "decorrelation_mode must be 0..3";
    return nullptr;
}

namespace {

inline uint64_t block_bytes_of(int32_t fmt) { return fmt == 1 ? 8 : 16; }
inline uint64_t blocks_of(uint32_t width, uint32_t height) { return (((uint64_t)width + 3) / 4) * (((uint64_t)height + 3) / 4); }
// side `v` of a texture at mip level k
inline uint32_t mip_dim(uint32_t v, uint32_t k) { return k < 32 && (v >> k) > 0 ? v >> k : 1u; }

int32_t check_format(int32_t fmt)
{
    if (fmt < 1 || fmt > 3)
        return fail(kInvalidArgument, "format must be 1 (BC1), 2 (BC2) or 3 (BC3)");
    return kOk;
}

// the checks every call shares, for a non-empty image, in the documented order
int32_t check_image(const void* blocks, const void* pixels, uint32_t width, uint64_t pitch)
{
    if (blocks == nullptr || pixels == nullptr)
        return fail(kInvalidArgument, "NULL pointer with a non-empty image");
    if (pitch < 4 * (uint64_t)width)
        return fail(kInvalidArgument, "pitch is smaller than 4 * width");
    if ((pitch & 3) != 0 || (reinterpret_cast<uintptr_t>(pixels) & 3) != 0)
        return fail(kInvalidArgument, "pitch and the pixel pointer must be multiples of 4");
    return kOk;
}

int32_t check_range(uint8_t mode, uint64_t total_blocks, uint64_t first_block, uint64_t blocks)
{
    if (mode > 3)
        return fail(kInvalidArgument, "decorrelation_mode must be 0..3");
    if (first_block > total_blocks || blocks > total_blocks - first_block)
        return fail(kInvalidArgument, "first_block + blocks of the image exceeds total_blocks");
    return kOk;
}

// ---- BC4 / BC5 -> R8 / RG8 ---------------------------------------------------------------------------------------------
inline uint64_t channel_bpp(int32_t fmt) { return fmt == 4 ? 1 : 2; }

int32_t check_channel_format(int32_t fmt)
{
    if (fmt != 4 && fmt != 5)
        return fail(kInvalidArgument, "format must be 4 (BC4) or 5 (BC5)");
    return kOk;
}

int32_t check_channel_image(int32_t fmt, const void* blocks, const void* pixels, uint32_t width, uint64_t pitch)
{
    const uint64_t bpp = channel_bpp(fmt);
    if (blocks == nullptr || pixels == nullptr)
        return fail(kInvalidArgument, "NULL pointer with a non-empty image");
    if (pitch < bpp * (uint64_t)width)
        return fail(kInvalidArgument, "pitch is smaller than the bytes of a pixel row");
    if (pitch % bpp != 0 || reinterpret_cast<uintptr_t>(pixels) % bpp != 0)
        return fail(kInvalidArgument, "pitch and the pixel pointer must be multiples of the bytes per pixel");
    return kOk;
}


// ---- several images of one buffer --------------------------------------------------------------------------------------
inline uint64_t bpp_of(int32_t fmt) { return fmt <= 3 ? 4 : channel_bpp(fmt); }

int32_t check_any_format(int32_t fmt)
{
    if (fmt < 1 || fmt > 5)
        return fail(kInvalidArgument, "format must be 1 (BC1) .. 5 (BC5)");
    return kOk;
}

// The checks of the image-region calls behind the format, in the documented order; *nothing = there is no non-empty region
// (DXTLT_OK, nothing to do).  `mode`: the decorrelation mode, 0 for the call that has none.
int32_t check_regions(int32_t fmt, const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count,
                      uint8_t mode, bool* nothing)
{
    if (const char* defect = dxtlt_host::image_regions_defect(fmt, buffer, total_blocks, regions, count, mode, nothing))
        return fail(kInvalidArgument, defect);
    return kOk;
}

}  // namespace

extern "C" {

int32_t dxtlt_decode_image_device(int32_t format, const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels,
                                  uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(d_blocks, d_pixels, width, pitch); rc != kOk)
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
    if (int32_t rc = check_image(d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_range(decorrelation_mode, total_blocks, first_block, blocks_of(width, height)); rc != kOk)
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
    if (int32_t rc = check_image(transformed, pixels, width, pitch); rc != kOk)
        return rc;
    const uint64_t bs = block_bytes_of(format), total_blocks = len / bs;
    if (int32_t rc = check_range(decorrelation_mode, total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    if (len % bs != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");

    // one upload of the transformed buffer, the device call into tightly packed rows, one download of the rows
    const uint64_t row_bytes = 4 * (uint64_t)width, d_pitch = (row_bytes + 15) & ~(uint64_t)15;
    const uint64_t need = std::max<uint64_t>(len, d_pitch * height);
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)need, &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    HIP_TRY(dxtlt::launch_untransform_decode_image(static_cast<dxtlt::Format>(format), s, d_in, total_blocks, first_block,
                                                   dxtlt::make_image_sink(d_out, d_pitch, width, height), st),
            "kernel launch");
    HIP_TRY(hipMemcpy2DAsync(pixels, pitch, d_out, d_pitch, row_bytes, height, hipMemcpyDeviceToHost, st), "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

int32_t dxtlt_decode_channel_image_device(int32_t format, const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels,
                                          uint64_t pitch, void* hip_stream)
{
    if (int32_t rc = check_channel_format(format); rc != kOk)
        return rc;
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_channel_image(format, d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_decode_channel_image(format, d_blocks,
                                               dxtlt::make_image_sink(d_pixels, pitch, width, height, (uint32_t)channel_bpp(format)),
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
    if (int32_t rc = check_channel_image(format, d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_range(0, total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::launch_untransform_decode_channel_image(
                static_cast<dxtlt::Format>(format), split_endpoints, d_transformed, total_blocks, first_block,
                dxtlt::make_image_sink(d_pixels, pitch, width, height, (uint32_t)channel_bpp(format)), static_cast<hipStream_t>(hip_stream)),
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
    if (int32_t rc = check_channel_image(format, transformed, pixels, width, pitch); rc != kOk)
        return rc;
    const uint64_t bs = format == 4 ? 8 : 16, total_blocks = len / bs;
    if (int32_t rc = check_range(0, total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    if (len % bs != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");

    // as dxtlt_untransform_decode_image: one upload, the device call into rows a multiple of 16 bytes apart, one download of the rows
    const uint64_t bpp = channel_bpp(format), row_bytes = bpp * (uint64_t)width, d_pitch = (row_bytes + 15) & ~(uint64_t)15;
    const uint64_t need = std::max<uint64_t>(len, d_pitch * height);
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)need, &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    HIP_TRY(dxtlt::launch_untransform_decode_channel_image(static_cast<dxtlt::Format>(format), split_endpoints, d_in, total_blocks,
                                                           first_block,
                                                           dxtlt::make_image_sink(d_out, d_pitch, width, height, (uint32_t)bpp), st),
            "kernel launch");
    HIP_TRY(hipMemcpy2DAsync(pixels, pitch, d_out, d_pitch, row_bytes, height, hipMemcpyDeviceToHost, st), "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
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
    if (int32_t rc = check_any_format(format); rc != kOk)
        return rc;
    bool nothing = true;
    if (int32_t rc = check_regions(format, d_transformed, total_blocks, regions, region_count, decorrelation_mode, &nothing);
        rc != kOk || nothing)
        return rc;
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    const uint32_t bpp = (uint32_t)bpp_of(format);
    HIP_TRY(for_each_region_group(
                regions, region_count,
                [&](size_t i) { return dxtlt::make_image_sink(regions[i].pixels, regions[i].pitch, regions[i].width, regions[i].height, bpp); },
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
    if (int32_t rc = check_any_format(format); rc != kOk)
        return rc;
    bool nothing = true;
    if (int32_t rc = check_regions(format, d_blocks, total_blocks, regions, region_count, 0, &nothing); rc != kOk || nothing)
        return rc;
    const uint32_t bpp = (uint32_t)bpp_of(format);
    HIP_TRY(for_each_region_group(
                regions, region_count,
                [&](size_t i) { return dxtlt::make_image_sink(regions[i].pixels, regions[i].pitch, regions[i].width, regions[i].height, bpp); },
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
    if (int32_t rc = check_any_format(format); rc != kOk)
        return rc;
    const uint64_t bs = format == 1 || format == 4 ? 8 : 16, total_blocks = len / bs;
    bool nothing = true;
    if (int32_t rc = check_regions(format, transformed, total_blocks, regions, region_count, decorrelation_mode, &nothing);
        rc != kOk || nothing)
        return rc;
    if (len % bs != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");

    // one upload of the transformed buffer, the device call into staging -- region after region, every base a multiple of 16
    // and its rows a multiple of 16 bytes apart -- and one download of the rows per region
    const uint64_t bpp = bpp_of(format);
    auto staged_pitch = [&](const DxtltImageRegion& r) { return (bpp * (uint64_t)r.width + 15) & ~(uint64_t)15; };
    uint64_t out_bytes = 0;
    for (size_t i = 0; i < region_count; ++i)
        if (!empty_region(regions[i]))
            out_bytes += staged_pitch(regions[i]) * regions[i].height;
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)std::max<uint64_t>(len, out_bytes), &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    const dxtlt::Settings s{decorrelation_mode, split_alpha_endpoints, split_colour_endpoints};
    uint64_t at = 0;   // the regions are visited in list order, here and in the download below
    HIP_TRY(for_each_region_group(
                regions, region_count,
                [&](size_t i) {
                    const dxtlt::ImageSink img = dxtlt::make_image_sink(static_cast<uint8_t*>(d_out) + at, staged_pitch(regions[i]),
                                                                        regions[i].width, regions[i].height, (uint32_t)bpp);
                    at += staged_pitch(regions[i]) * regions[i].height;
                    return img;
                },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::launch_untransform_decode_image_regions(static_cast<dxtlt::Format>(format), s, d_in, total_blocks, tab, st);
                }),
            "kernel launch");
    at = 0;
    for (size_t i = 0; i < region_count; ++i) {
        const DxtltImageRegion& r = regions[i];
        if (empty_region(r))
            continue;
        HIP_TRY(hipMemcpy2DAsync(r.pixels, r.pitch, static_cast<uint8_t*>(d_out) + at, staged_pitch(r), bpp * (uint64_t)r.width, r.height,
                                 hipMemcpyDeviceToHost, st),
                "D2H copy");
        at += staged_pitch(r) * r.height;
    }
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
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
