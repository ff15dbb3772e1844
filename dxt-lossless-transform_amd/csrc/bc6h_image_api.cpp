// bc6h_image_api.cpp -- C ABI of the BC6H decoders (include/dxtlt_bc6h_image.h): BC6H as a family of granule_image_api.h, which has the
// bodies, and one forward per entry point.  The kernels are granule_image.h's, instantiated in bc6h_image_kernels.hip (which has the
// block-array decoder too); the decoder itself is bc6h_decode.h.
#include "../../include/dxtlt_bc6h_image.h"
#include "../../include/dxtlt_gfx950.h"
#include "bc6h_decode.h"
#include "granule_image_api.h"

namespace {

namespace api = dxtlt_host::granule_image;

struct Bc6h {
    static constexpr dxtlt_host::PixelRule rule = dxtlt_host::kRgba16f;   // RGBA16F
    static constexpr size_t kDecodedBlockBytes = 128;   // sixteen pixels of four halves
    static constexpr const char* kTooSmall = "pixels_len is smaller than 128 bytes per block";
    static void decode_block(const dxtlt::bc7::B128& b, uint32_t (&px)[32]) { dxtlt::bc6h::decode_bc6h_block(b, px); }
    static constexpr auto& launch_decode_blocks = dxtlt::bc6h::launch_decode_blocks;
    using Launch = dxtlt::bc6h::Bc6hImage;
};

}  // namespace

extern "C" {

int32_t dxtlt_decode_bc6h_blocks(const uint8_t* blocks, size_t len, uint8_t* pixels, size_t pixels_len)
{
    return api::decode_blocks<Bc6h>(blocks, len, pixels, pixels_len);
}

int32_t dxtlt_decode_bc6h_blocks_device(const void* d_blocks, size_t len, void* d_pixels, size_t pixels_len, void* hip_stream)
{
    return api::decode_blocks_device<Bc6h>(d_blocks, len, d_pixels, pixels_len, hip_stream);
}

int32_t dxtlt_decode_bc6h_image_device(const void* d_blocks, uint32_t width, uint32_t height, void* d_pixels, uint64_t pitch,
                                       void* hip_stream)
{
    return api::decode_image_device<Bc6h>(d_blocks, width, height, d_pixels, pitch, hip_stream);
}

int32_t dxtlt_untransform_decode_bc6h_image_device(const void* d_transformed, uint64_t total_blocks, uint64_t first_block, uint32_t width,
                                                   uint32_t height, void* d_pixels, uint64_t pitch, void* hip_stream)
{
    return api::untransform_decode_image_device<Bc6h>(d_transformed, total_blocks, first_block, width, height, d_pixels, pitch, hip_stream);
}

int32_t dxtlt_untransform_decode_bc6h_image(const uint8_t* transformed, size_t len, uint64_t first_block, uint32_t width, uint32_t height,
                                            uint8_t* pixels, uint64_t pitch)
{
    return api::untransform_decode_image<Bc6h>(transformed, len, first_block, width, height, pixels, pitch);
}

int32_t dxtlt_untransform_decode_bc6h_images_device(const void* d_transformed, uint64_t total_blocks, const DxtltImageRegion* regions,
                                                    size_t region_count, void* hip_stream)
{
    return api::decode_images_device<Bc6h>(dxtlt::launch_untransform_decode_image_regions<Bc6h::Launch>, d_transformed, total_blocks, regions,
                                           region_count, hip_stream);
}

int32_t dxtlt_decode_bc6h_images_device(const void* d_blocks, uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                        void* hip_stream)
{
    return api::decode_images_device<Bc6h>(dxtlt::launch_decode_image_regions<Bc6h::Launch>, d_blocks, total_blocks, regions, region_count,
                                           hip_stream);
}

int32_t dxtlt_untransform_decode_bc6h_images(const uint8_t* transformed, size_t len, const DxtltImageRegion* regions, size_t region_count)
{
    return api::untransform_decode_images<Bc6h>(transformed, len, regions, region_count);
}

int32_t dxtlt_debug_plan_bc6h_images(uint64_t total_blocks, const DxtltImageRegion* regions, size_t region_count,
                                     DxtltBc6hImagesLaunch* out, size_t cap)
{
    // the arithmetic is the BC7 debug call's too (image_host.h)
    return dxtlt_host::plan_granule_region_launches(Bc6h::rule, total_blocks, regions, region_count, out, cap);
}

}  // extern "C"
