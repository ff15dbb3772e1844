// C++ host API of the BC6H region calls (include/dxt_lossless_transform.hpp: api::untransform_decode_bc6h_images_device,
// api::decode_bc6h_images_device, api::untransform_decode_bc6h_images), built and run by tests/test_bc6h_image_regions_layout.py:
// the three wrappers compile, link and pass their arguments on -- every call here ends in the library's checks, before a device
// is touched.
#include <cstdio>
#include <cstdint>

#include "../../include/dxt_lossless_transform.hpp"

using namespace dxt_lossless_transform;

static int failures = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #cond);     \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

template <typename F>
static int thrown_code(F&& f)
{
    try {
        f();
    } catch (const DeviceError& e) {
        return e.code;
    }
    return 0;
}

int main()
{
    alignas(16) static uint8_t src[64 * 16], dst[16 * 16 * 8];
    // a 16 x 16 chain of three levels: 16 + 4 + 1 blocks; rows of 128 bytes
    DxtltImageRegion chain[3] = {};
    CHECK(api::image_mip_chain(16, 16, 3, 0, chain) == 21);
    for (int k = 0; k < 3; ++k)
        chain[k].pixels = dst, chain[k].pitch = 128;
    // nothing to do: no regions, or only empty ones -- NULL pointers and all
    DxtltImageRegion empty[2] = {{5, 0, 8, nullptr, 0}, {1ull << 63, 8, 0, nullptr, 1}};
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_device(nullptr, 0, nullptr, 0, nullptr); }) == 0);
    CHECK(thrown_code([&] { api::decode_bc6h_images_device(nullptr, 0, empty, 2, nullptr); }) == 0);
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images(nullptr, 7, empty, 2); }) == 0);
    // the chain does not fit in 20 blocks; a NULL buffer; regions out of order
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_device(src, 20, chain, 3, nullptr); }) == 2);
    CHECK(thrown_code([&] { api::decode_bc6h_images_device(src, 20, chain, 3, nullptr); }) == 2);
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images(src, 20 * 16, chain, 3); }) == 2);
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_device(nullptr, 21, chain, 3, nullptr); }) == 2);
    DxtltImageRegion swapped[2] = {chain[1], chain[0]};
    CHECK(thrown_code([&] { api::decode_bc6h_images_device(src, 21, swapped, 2, nullptr); }) == 2);
    // eight bytes a pixel: level 0's 64-byte pitch, right for RGBA8888, is too small; 132 and a pointer + 4 are no multiples of 8
    chain[0].pitch = 64;
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images(src, 21 * 16, chain, 3); }) == 2);
    chain[0].pitch = 132;
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_device(src, 21, chain, 3, nullptr); }) == 2);
    chain[0].pitch = 128;
    chain[2].pixels = dst + 4;
    CHECK(thrown_code([&] { api::decode_bc6h_images_device(src, 21, chain, 3, nullptr); }) == 2);
    chain[2].pixels = dst;
    // the host call's length comes last
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images(src, 21 * 16 + 5, chain, 3); }) == 1);
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
