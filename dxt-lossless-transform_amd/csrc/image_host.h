// image_host.h -- the host side of the image-decode entry points, stated once for every family: image_api.cpp (BC1 - BC3 ->
// RGBA8888, BC4 / BC5 -> R8 / RG8), granule_image_api.h (BC7, BC6H) and the batch calls (image_batch_api.cpp,
// granule_image_batch_api.h).  A family is a PixelRule; an entry point keeps the checks that are its own (format, decorrelation
// mode) and a lambda that names its launcher.  The order of the checks is the documented one (docs/IMAGE_DECODE.md, the public
// headers).  The launch plan the two granule formats' debug calls report is here too.  Not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "../../include/dxtlt_image.h"
#include "granule_launch.h"   // for_each_range_launch
#include "host_common.h"
#include "image_region_groups.h"
#include "image_sink.h"

namespace dxtlt_host {

inline uint64_t blocks_of(uint32_t width, uint32_t height) { return (((uint64_t)width + 3) / 4) * (((uint64_t)height + 3) / 4); }

// What a family asks of an image: the bytes of a pixel, the multiple required of pitch and pixel pointer, and its two error texts
struct PixelRule {
    uint32_t bpp, multiple;
    const char *small_pitch, *not_multiple;
};
constexpr PixelRule kRgba8888{4, 4, "pitch is smaller than 4 * width", "pitch and the pixel pointer must be multiples of 4"};   // BC1 - BC3, BC7
constexpr PixelRule kR8{1, 1, "pitch is smaller than the bytes of a pixel row",
                        "pitch and the pixel pointer must be multiples of the bytes per pixel"};                               // BC4
constexpr PixelRule kRg8{2, 2, kR8.small_pitch, kR8.not_multiple};                                                             // BC5
constexpr PixelRule kRgba16f{8, 8, "pitch is smaller than 8 * width", "pitch and the pixel pointer must be multiples of 8"};   // BC6H
// format 1 .. 5
inline const PixelRule& pixel_rule(int32_t fmt) { return fmt <= 3 ? kRgba8888 : fmt == 4 ? kR8 : kRg8; }

// the checks every call shares, for a non-empty image
inline int32_t check_image(const PixelRule& rule, const void* blocks, const void* pixels, uint32_t width, uint64_t pitch)
{
    if (blocks == nullptr || pixels == nullptr)
        return fail(kInvalidArgument, "NULL pointer with a non-empty image");
    if (pitch < rule.bpp * (uint64_t)width)
        return fail(kInvalidArgument, rule.small_pitch);
    if (pitch % rule.multiple != 0 || reinterpret_cast<uintptr_t>(pixels) % rule.multiple != 0)
        return fail(kInvalidArgument, rule.not_multiple);
    return kOk;
}

inline int32_t check_block_range(uint64_t total_blocks, uint64_t first_block, uint64_t blocks)
{
    if (first_block > total_blocks || blocks > total_blocks - first_block)
        return fail(kInvalidArgument, "first_block + blocks of the image exceeds total_blocks");
    return kOk;
}

// a buffer of len / block_bytes blocks.  In the host-pointer image calls this is the LAST check, behind the range or the regions
inline int32_t check_len(size_t len, uint64_t block_bytes)
{
    if (len % block_bytes != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");
    return kOk;
}

inline int32_t check_host_range(size_t len, uint64_t block_bytes, uint64_t first_block, uint64_t blocks)
{
    if (int32_t rc = check_block_range(len / block_bytes, first_block, blocks); rc != kOk)
        return rc;
    return check_len(len, block_bytes);
}

// the block decoders: `len` bytes of blocks -> decoded_bytes per block in a buffer of out_len; too_small names decoded_bytes
inline int32_t check_decode(const void* in, size_t len, size_t block_bytes, const void* out, size_t out_len, size_t decoded_bytes,
                            const char* too_small)
{
    if (int32_t rc = check_len(len, block_bytes); rc != kOk)
        return rc;
    const size_t n = len / block_bytes;
    if (n > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    if (out_len / decoded_bytes < n)
        return fail(kInvalidArgument, too_small);
    return kOk;
}

// The first defect of a region list in the documented order -- all of them DXTLT_E_INVALID_ARGUMENT -- or nullptr;
// *nothing = there is no non-empty region.  The batch calls check every item with it.
inline const char* image_regions_defect(const PixelRule& rule, const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions,
                                        size_t count, bool* nothing)
{
    *nothing = true;
    if (count == 0)
        return nullptr;
    if (regions == nullptr)
        return "NULL regions pointer";
    for (size_t i = 0; i < count && *nothing; ++i)
        *nothing = empty_region(regions[i]);
    if (*nothing)
        return nullptr;
    if (buffer == nullptr)
        return "NULL buffer with a non-empty region";
    uint64_t end = 0;   // of the previous non-empty region
    for (size_t i = 0; i < count; ++i) {
        const DxtltImageRegion& r = regions[i];
        if (empty_region(r))
            continue;
        if (r.pixels == nullptr)
            return "NULL pixels pointer of a non-empty region";
        if (r.pitch < rule.bpp * (uint64_t)r.width)
            return "a region's pitch is smaller than the bytes of a pixel row";
        if (r.pitch % rule.multiple != 0 || reinterpret_cast<uintptr_t>(r.pixels) % rule.multiple != 0)
            return "a region's pitch and pixel pointer must be multiples of 4 (BC1 - BC3) or of the bytes per pixel";
        if (r.first_block > total_blocks || blocks_of(r.width, r.height) > total_blocks - r.first_block)
            return "first_block + blocks of a region exceeds total_blocks";
        if (r.first_block < end)
            return "regions must come in ascending block order and must not overlap";
        end = r.first_block + blocks_of(r.width, r.height);
    }
    return nullptr;
}

// The same for the calls that take a format 1 .. 5 and a decorrelation mode (0 for a call that has none): the format is the first
// check, the mode of BC1 - BC3 the last
inline const char* image_regions_defect(int32_t fmt, const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions,
                                        size_t count, uint8_t mode, bool* nothing)
{
    *nothing = true;
    if (fmt < 1 || fmt > 5)
        return "format must be 1 (BC1) .. 5 (BC5)";
    if (const char* defect = image_regions_defect(pixel_rule(fmt), buffer, total_blocks, regions, count, nothing))
        return defect;
    return !*nothing && fmt <= 3 && mode > 3 ? "decorrelation_mode must be 0..3" : nullptr;
}

// The launches a fused region call of a granule format (BC7, BC6H) enqueues, as records in the place of launches -- the body of
// dxtlt_debug_plan_bc7_images and dxtlt_debug_plan_bc6h_images.  The device call's checks but for the buffer pointer, which a plan
// does not have, then the device call's walk: the same groups (for_each_region_group), the same plan of each group's covering
// range (granule::for_each_range_launch).  RECORD is {first region, region count, first granule, granule count, tail, reserved};
// records beyond `cap` are counted, not written.  Returns the number of launches, or -1 for a list the call would refuse.
template <typename RECORD>
int32_t plan_granule_region_launches(const PixelRule& rule, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count,
                                     RECORD* out, size_t cap)
{
    bool nothing = true;
    // any non-NULL address stands in for the buffer
    if (const char* defect = image_regions_defect(rule, &nothing, total_blocks, regions, count, &nothing)) {
        fail(kInvalidArgument, defect);
        return -1;
    }
    if (nothing)
        return 0;
    size_t launches = 0, group_first = 0;
    bool group_open = false;
    const hipError_t e = for_each_region_group(
        regions, count,
        [&](size_t i) {
            if (!group_open)
                group_first = i, group_open = true;
            return dxtlt::make_image_sink(regions[i].pixels, regions[i].pitch, regions[i].width, regions[i].height, rule.bpp);
        },
        [&](const dxtlt::ImageRegionTable& tab) {
            uint64_t first = 0, n = 0;
            if (!dxtlt::covering_range(tab, total_blocks, first, n))
                return hipErrorInvalidValue;
            group_open = false;
            return dxtlt::granule::for_each_range_launch(total_blocks, first, first + n, [&](uint64_t granule, uint64_t granules, bool tail) {
                if (out != nullptr && launches < cap)
                    out[launches] = RECORD{(uint32_t)group_first, tab.count, granule, granules, tail ? 1u : 0u, 0u};
                ++launches;
                return hipSuccess;
            });
        });
    return e == hipSuccess ? (int32_t)launches : -1;
}

// The host-pointer path of one image, its arguments checked: one upload of the transformed buffer, launch(d_in, staged image,
// stream) into rows a multiple of 16 bytes apart, one download of the rows, and the wait for them
template <typename LAUNCH>
int32_t untransform_decode_host_image(const uint8_t* transformed, size_t len, uint32_t bpp, uint32_t width, uint32_t height,
                                      uint8_t* pixels, uint64_t pitch, const LAUNCH& launch)
{
    const uint64_t row_bytes = bpp * (uint64_t)width, d_pitch = (row_bytes + 15) & ~(uint64_t)15;
    const uint64_t need = std::max<uint64_t>(len, d_pitch * height);
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = acquire_staging((size_t)need, &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    HIP_TRY(launch(d_in, dxtlt::make_image_sink(d_out, d_pitch, width, height, bpp), st), "kernel launch");
    HIP_TRY(hipMemcpy2DAsync(pixels, pitch, d_out, d_pitch, row_bytes, height, hipMemcpyDeviceToHost, st), "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

// The host-pointer path of several regions, their list checked: one upload of the transformed buffer, launch(d_in, table, stream)
// per group into staging -- region after region, every base a multiple of 16 and its rows a multiple of 16 bytes apart -- and one
// download of the rows per region
template <typename LAUNCH>
int32_t untransform_decode_host_regions(const uint8_t* transformed, size_t len, const DxtltImageRegion* regions, size_t count,
                                        uint32_t bpp, const LAUNCH& launch)
{
    auto staged_pitch = [&](const DxtltImageRegion& r) { return (bpp * (uint64_t)r.width + 15) & ~(uint64_t)15; };
    uint64_t out_bytes = 0;
    for (size_t i = 0; i < count; ++i)
        if (!empty_region(regions[i]))
            out_bytes += staged_pitch(regions[i]) * regions[i].height;
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = acquire_staging((size_t)std::max<uint64_t>(len, out_bytes), &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    uint64_t at = 0;   // the regions are visited in list order, here and in the download below
    HIP_TRY(for_each_region_group(
                regions, count,
                [&](size_t i) {
                    const dxtlt::ImageSink img = dxtlt::make_image_sink(static_cast<uint8_t*>(d_out) + at, staged_pitch(regions[i]),
                                                                        regions[i].width, regions[i].height, bpp);
                    at += staged_pitch(regions[i]) * regions[i].height;
                    return img;
                },
                [&](const dxtlt::ImageRegionTable& tab) { return launch(d_in, tab, st); }),
            "kernel launch");
    at = 0;
    for (size_t i = 0; i < count; ++i) {
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

}  // namespace dxtlt_host
