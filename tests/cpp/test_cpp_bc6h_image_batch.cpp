// C++ host API of the BC6H batch image call (include/dxt_lossless_transform.hpp: api::untransform_decode_bc6h_images_batch_device),
// built and run by tests/test_bc6h_image_batch_layout.py: the wrapper compiles, links and passes its arguments on -- every call
// here ends in the library's checks, before a device is touched.
#include <cstdio>
#include <cstdint>
#include <cstring>

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
    // a 16 x 16 chain of three levels: 16 + 4 + 1 blocks, eight bytes a pixel
    DxtltImageRegion chain[3] = {};
    CHECK(api::image_mip_chain(16, 16, 3, 0, chain) == 21);
    for (int k = 0; k < 3; ++k)
        chain[k].pixels = dst, chain[k].pitch = 128;
    DxtltImageRegion empty[2] = {{5, 0, 8, nullptr, 0}, {1ull << 63, 8, 0, nullptr, 1}};
    // nothing to do: no items, or only items without a non-empty region -- NULL buffers and all
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_batch_device(nullptr, 0, nullptr); }) == 0);
    DxtltBc6hImageBatchItem nothing[2] = {{nullptr, 0, empty, 2, 0}, {nullptr, 0, nullptr, 0, 0}};
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_batch_device(nothing, 2, nullptr); }) == 0);
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_batch_device(nullptr, 2, nullptr); }) == 2);
    // the second item's chain does not fit in 20 blocks: the error names the item
    DxtltBc6hImageBatchItem items[2] = {{nullptr, 0, empty, 2, 0}, {src, 20, chain, 3, 0}};
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_batch_device(items, 2, nullptr); }) == 2);
    CHECK(std::strstr(dxtlt_last_error(), "bc6h image batch item 1:") != nullptr);
    CHECK(dxtlt_debug_plan_bc6h_image_batch(items, 2, nullptr, 0) == -1);
    // ... and in 21 it plans: one entry, the tail part alone
    items[1].total_blocks = 21;
    DxtltDebugBc6hImageBatchEntry e = {};
    CHECK(dxtlt_debug_plan_bc6h_image_batch(items, 2, &e, 1) == 1);
    CHECK(e.item == 1 && e.region_count == 3 && e.granule_count == 0 && e.tail_index == 0 && e.granule_wgs == 0 && e.tail_wgs == 1);
    // a pitch of 64 holds a 16-pixel row of RGBA8888, not of RGBA16F: the 8-byte pixel's rule is the one applied
    chain[0].pitch = 64;
    CHECK(thrown_code([&] { api::untransform_decode_bc6h_images_batch_device(items, 2, nullptr); }) == 2);
    CHECK(std::strstr(dxtlt_last_error(), "pitch is smaller") != nullptr);
    std::printf("%d failure(s)\n", failures);
    return failures ? 1 : 0;
}
