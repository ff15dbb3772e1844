// bc7_image_api.cpp -- C ABI of the BC7 decoders (include/dxtlt_bc7_image.h); kernels in bc7_image_kernels.hip and, for several
// images of one buffer, bc7_image_regions_kernels.hip; the decoder itself in bc7_decode.h.  Every argument is checked before a
// device is touched.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "../../include/dxtlt_bc7_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc7_decode.h"
#include "bc7_image_launch.h"
#include "host_common.h"
#include "image_launch.h"   // image_regions_defect
#include "image_region_groups.h"

using dxtlt_host::empty_region;
using dxtlt_host::fail;
using dxtlt_host::for_each_region_group;
using dxtlt_host::kInvalidArgument;
using dxtlt_host::kInvalidLength;
using dxtlt_host::kOk;

namespace {

constexpr size_t kDecodedBlockBytes = 64;

inline uint64_t blocks_of(uint32_t width, uint32_t height) { return (((uint64_t)width + 3) / 4) * (((uint64_t)height + 3) / 4); }

// as dxtlt_decode_bc3_blocks* (decode_api.cpp)
int32_t check_decode(const void* in, size_t len, const void* out, size_t out_len)
{
    if (len % 16 != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");
    const size_t n = len / 16;
    if (n > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    if (out_len / kDecodedBlockBytes < n)
        return fail(kInvalidArgument, "pixels_len is smaller than 64 bytes per block");
    return kOk;
}

// the checks of a non-empty image, in the documented order (the RGBA image calls', image_api.cpp, minus format and settings)
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

int32_t check_range(uint64_t total_blocks, uint64_t first_block, uint64_t blocks)
{
    if (first_block > total_blocks || blocks > total_blocks - first_block)
        return fail(kInvalidArgument, "first_block + blocks of the image exceeds total_blocks");
    return kOk;
}

// ---- several images of one buffer --------------------------------------------------------------------------------------
// the checks of the region calls, in the documented order: those of dxtlt_untransform_decode_images_device minus format and
// settings; *nothing = there is no non-empty region (DXTLT_OK, nothing to do)
int32_t check_regions(const void* buffer, uint64_t total_blocks, const DxtltImageRegion* regions, size_t count, bool* nothing)
{
    if (const char* defect = dxtlt_host::image_regions_defect(0, buffer, total_blocks, regions, count, 0, nothing, true))
        return fail(kInvalidArgument, defect);
    return kOk;
}

inline dxtlt::ImageSink sink_of(const DxtltImageRegion& r) { return dxtlt::make_image_sink(r.pixels, r.pitch, r.width, r.height); }

}  // namespace

extern "C" {

int32_t dxtlt_decode_bc7_blocks(const uint8_t* blocks, size_t len, uint8_t* pixels, size_t pixels_len)
{
    if (int32_t rc = check_decode(blocks, len, pixels, pixels_len); rc != kOk)
        return rc;
    // on the CPU, with the decoder the kernels run (bc7_decode.h): a Decoded4x4Block per block needs no device
    for (size_t i = 0; i < len / 16; ++i) {
        dxtlt::bc7::B128 b;
        std::memcpy(b.d, blocks + 16 * i, 16);
        uint32_t px[16];
        dxtlt::bc7::decode_bc7_block(b, px);
        for (int k = 0; k < 16; ++k)
            for (int c = 0; c < 4; ++c)
                pixels[kDecodedBlockBytes * i + 4 * k + c] = (uint8_t)(px[k] >> (8 * c));
    }
    return kOk;
}

int32_t dxtlt_decode_bc7_blocks_device(const void* d_blocks, size_t len, void* d_pixels, size_t pixels_len, void* hip_stream)
{
    if (int32_t rc = check_decode(d_blocks, len, d_pixels, pixels_len); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc7::launch_decode_blocks(d_blocks, d_pixels, len / 16, static_cast<hipStream_t>(hip_stream)), "kernel launch");
    return kOk;
}

int32_t dxtlt_decode_bc7_image_device(const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels, uint64_t pitch,
                                      void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(d_blocks, d_pixels, width, pitch); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc7::launch_decode_image(d_blocks, dxtlt::make_image_sink(d_pixels, pitch, width, height),
                                            static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc7_image_device(const void* d_transformed, uint64_t total_blocks, uint64_t first_block, uint32_t width,
                                                  uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    if (width == 0 || height == 0)
        return kOk;
    if (int32_t rc = check_image(d_transformed, d_pixels, width, pitch); rc != kOk)
        return rc;
    if (int32_t rc = check_range(total_blocks, first_block, blocks_of(width, height)); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::bc7::launch_untransform_decode_image(d_transformed, total_blocks, first_block,
                                                        dxtlt::make_image_sink(d_pixels, pitch, width, height),
                                                        static_cast<hipStream_t>(hip_stream)),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc7_image(const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width, uint32_t height,
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

    // as dxtlt_untransform_decode_image: one upload, the device call into rows a multiple of 16 bytes apart, one download of the rows
    const uint64_t row_bytes = 4 * (uint64_t)width, d_pitch = (row_bytes + 15) & ~(uint64_t)15;
    const uint64_t need = std::max<uint64_t>(len, d_pitch * height);
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)need, &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    HIP_TRY(dxtlt::bc7::launch_untransform_decode_image(d_in, total_blocks, first_block, dxtlt::make_image_sink(d_out, d_pitch, width, height),
                                                        st),
            "kernel launch");
    HIP_TRY(hipMemcpy2DAsync(pixels, pitch, d_out, d_pitch, row_bytes, height, hipMemcpyDeviceToHost, st), "D2H copy");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc7_images_device(const void* d_transformed, uint64_t total_blocks, const DxtltImageRegion* regions,
                                                   size_t region_count, void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(d_transformed, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i]); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::bc7::launch_untransform_decode_image_regions(d_transformed, total_blocks, tab,
                                                                               static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_decode_bc7_images_device(const void* d_blocks, uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                       void* hip_stream)
{
    bool nothing = true;
    if (int32_t rc = check_regions(d_blocks, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    HIP_TRY(for_each_region_group(
                regions, region_count, [&](size_t i) { return sink_of(regions[i]); },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::bc7::launch_decode_image_regions(d_blocks, total_blocks, tab, static_cast<hipStream_t>(hip_stream));
                }),
            "kernel launch");
    return kOk;
}

int32_t dxtlt_untransform_decode_bc7_images(const uint8_t* transformed, size_t len, const DxtltImageRegion* regions, size_t region_count)
{
    const uint64_t total_blocks = len / 16;
    bool nothing = true;
    if (int32_t rc = check_regions(transformed, total_blocks, regions, region_count, &nothing); rc != kOk || nothing)
        return rc;
    if (len % 16 != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");

    // as dxtlt_untransform_decode_images: one upload of the transformed buffer, the device path into staging -- region after
    // region, every base a multiple of 16 and its rows a multiple of 16 bytes apart -- and one download of the rows per region
    auto staged_pitch = [](const DxtltImageRegion& r) { return (4 * (uint64_t)r.width + 15) & ~(uint64_t)15; };
    uint64_t out_bytes = 0;
    for (size_t i = 0; i < region_count; ++i)
        if (!empty_region(regions[i]))
            out_bytes += staged_pitch(regions[i]) * regions[i].height;
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = dxtlt_host::acquire_staging((size_t)std::max<uint64_t>(len, out_bytes), &d_in, &d_out, &st); rc != kOk)
        return rc;
    HIP_TRY(hipMemcpyAsync(d_in, transformed, len, hipMemcpyHostToDevice, st), "H2D copy");
    uint64_t at = 0;   // the regions are visited in list order, here and in the download below
    HIP_TRY(for_each_region_group(
                regions, region_count,
                [&](size_t i) {
                    const dxtlt::ImageSink img = dxtlt::make_image_sink(static_cast<uint8_t*>(d_out) + at, staged_pitch(regions[i]),
                                                                        regions[i].width, regions[i].height);
                    at += staged_pitch(regions[i]) * regions[i].height;
                    return img;
                },
                [&](const dxtlt::ImageRegionTable& tab) {
                    return dxtlt::bc7::launch_untransform_decode_image_regions(d_in, total_blocks, tab, st);
                }),
            "kernel launch");
    at = 0;
    for (size_t i = 0; i < region_count; ++i) {
        const DxtltImageRegion& r = regions[i];
        if (empty_region(r))
            continue;
        HIP_TRY(hipMemcpy2DAsync(r.pixels, r.pitch, static_cast<uint8_t*>(d_out) + at, staged_pitch(r), 4 * (uint64_t)r.width, r.height,
                                 hipMemcpyDeviceToHost, st),
                "D2H copy");
        at += staged_pitch(r) * r.height;
    }
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

int32_t dxtlt_debug_plan_bc7_images(uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                    DxtltBc7ImagesLaunch* out, size_t cap)
{
    // the device call's checks but for the buffer pointer, which this call does not have: any non-NULL address stands in
    bool nothing = true;
    if (check_regions(&nothing, total_blocks, regions, region_count, &nothing) != kOk)
        return -1;
    if (nothing)
        return 0;
    // the device call's walk: the same groups, the same plan of each group's covering range, records in the place of launches
    size_t launches = 0, group_first = 0;
    bool group_open = false;
    const hipError_t e = for_each_region_group(
        regions, region_count,
        [&](size_t i) {
            if (!group_open)
                group_first = i, group_open = true;
            return sink_of(regions[i]);
        },
        [&](const dxtlt::ImageRegionTable& tab) {
            uint64_t first = 0, n = 0;
            if (!dxtlt::covering_range(tab, total_blocks, first, n))
                return hipErrorInvalidValue;
            group_open = false;
            return dxtlt::bc7::for_each_range_launch(total_blocks, first, first + n, [&](uint64_t granule, uint64_t granules, bool tail) {
                if (out != nullptr && launches < cap)
                    out[launches] = DxtltBc7ImagesLaunch{(uint32_t)group_first, tab.count, granule, granules, tail ? 1u : 0u, 0u};
                ++launches;
                return hipSuccess;
            });
        });
    return e == hipSuccess ? (int32_t)launches : -1;
}

}  // extern "C"
