// C++ host API of the BC4 / BC5 image decoders (include/dxt_lossless_transform.hpp: api::decode_channel_image_device,
// api::untransform_decode_channel_image_device, api::untransform_decode_channel_image), driven by tests/test_cpp_channel_image.py.
//   test_cpp_channel_image cpu   -- every wrapper throws DeviceError for a bad argument and returns for an empty image (no device)
//   test_cpp_channel_image gpu   -- an 8 x 8 image through the three wrappers, against values worked out by hand
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/dxt_lossless_transform.hpp"

using namespace dxt_lossless_transform;

// the four HIP runtime calls the device-pointer wrappers need around them (libamdhip64)
extern "C" {
int hipMalloc(void** ptr, size_t size);
int hipFree(void* ptr);
int hipMemcpy(void* dst, const void* src, size_t size, int kind);
int hipDeviceSynchronize(void);
}

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

static void cpu_tests()
{
    uint8_t src[64] = {0}, dst[64] = {0};
    for (int32_t fmt : {0, 1, 3, 6, -1}) {
        CHECK(thrown_code([&] { api::decode_channel_image_device(fmt, src, 8, 8, dst, 16, nullptr); }) == 2);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image_device(fmt, src, 4, 0, 8, 8, true, dst, 16, nullptr); }) == 2);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image(fmt, src, 64, 0, 8, 8, true, dst, 16); }) == 2);
    }
    for (int32_t fmt : {4, 5}) {
        const uint64_t row = fmt == 4 ? 8 : 16;
        CHECK(thrown_code([&] { api::decode_channel_image_device(fmt, nullptr, 0, 8, nullptr, 0, nullptr); }) == 0);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image_device(fmt, nullptr, 0, 0, 8, 0, true, nullptr, 0, nullptr); }) == 0);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image(fmt, nullptr, 0, 0, 0, 0, true, nullptr, 0); }) == 0);
        CHECK(thrown_code([&] { api::decode_channel_image_device(fmt, src, 8, 8, nullptr, row, nullptr); }) == 2);
        CHECK(thrown_code([&] { api::decode_channel_image_device(fmt, src, 8, 8, dst, row - 1, nullptr); }) == 2);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image_device(fmt, src, 3, 0, 8, 8, true, dst, row, nullptr); }) == 2);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image(fmt, src, 3 * (fmt == 4 ? 8 : 16), 0, 8, 8, true, dst, row); }) == 2);
        CHECK(thrown_code([&] { api::untransform_decode_channel_image(fmt, src, 4 * (fmt == 4 ? 8 : 16) + 1, 0, 8, 8, true, dst, row); }) == 1);
    }
    CHECK(thrown_code([&] { api::untransform_decode_channel_image(5, src, 64, 0, 8, 8, true, dst + 1, 16); }) == 2);
    const api::MipLevel m = api::image_mip_level(40, 24, 6, 2);   // block counts do not depend on the format
    CHECK(m.width == 10 && m.height == 6 && m.first_block == 75 && m.num_blocks == 6 && m.total_blocks == 85);
}

// Half k (an 8-byte BC4 block): endpoints a0 = 10 + k <= a1 = 200 (the six-value table), every index 0 (-> a0) for even k and
// 7 (-> 255) for odd k
static void half(uint8_t* p, int k)
{
    p[0] = (uint8_t)(10 + k), p[1] = 200;
    std::memset(p + 2, k & 1 ? 0xFF : 0x00, 6);
}
static uint8_t half_value(int k) { return k & 1 ? 255 : (uint8_t)(10 + k); }

// the transformed buffer of `n` blocks, split_endpoints = false (docs/BC45_FORMAT.md): per half h the endpoint pairs of all
// blocks, then their index records
static std::vector<uint8_t> transformed_of(const std::vector<uint8_t>& blocks, int halves)
{
    const size_t n = blocks.size() / (8 * halves);
    std::vector<uint8_t> t(blocks.size());
    for (int h = 0; h < halves; ++h)
        for (size_t b = 0; b < n; ++b) {
            const uint8_t* s = blocks.data() + (b * halves + h) * 8;
            std::memcpy(t.data() + (8 * h) * n + 2 * b, s, 2);
            std::memcpy(t.data() + (8 * h + 2) * n + 6 * b, s + 2, 6);
        }
    return t;
}

static void gpu_tests()
{
    for (int32_t fmt : {4, 5}) {
        const int halves = fmt == 4 ? 1 : 2, bpp = halves;
        const uint32_t width = 8, height = 8;
        const uint64_t pitch = bpp * width + 6;
        std::vector<uint8_t> blocks(4 * 8 * halves);
        for (int k = 0; k < 4 * halves; ++k)
            half(blocks.data() + 8 * k, k);
        const std::vector<uint8_t> t = transformed_of(blocks, halves);
        std::vector<uint8_t> want(pitch * height, 0xA5);
        for (uint32_t y = 0; y < height; ++y)
            for (uint32_t x = 0; x < width; ++x)
                for (int c = 0; c < bpp; ++c)
                    want[y * pitch + bpp * x + c] = half_value((int)((y / 4) * 2 + x / 4) * halves + c);
        // host pointers
        std::vector<uint8_t> got(pitch * height, 0xA5);
        api::untransform_decode_channel_image(fmt, t.data(), t.size(), 0, width, height, false, got.data(), pitch);
        CHECK(got == want);
        // device pointers: fused and plain
        void *d_t = nullptr, *d_blocks = nullptr, *d_px = nullptr;
        CHECK(hipMalloc(&d_t, t.size()) == 0 && hipMalloc(&d_blocks, blocks.size()) == 0 && hipMalloc(&d_px, want.size()) == 0);
        CHECK(hipMemcpy(d_t, t.data(), t.size(), 1) == 0 && hipMemcpy(d_blocks, blocks.data(), blocks.size(), 1) == 0);
        for (int plain = 0; plain < 2; ++plain) {
            std::vector<uint8_t> fill(want.size(), 0xA5), back(want.size());
            CHECK(hipMemcpy(d_px, fill.data(), fill.size(), 1) == 0);
            if (plain)
                api::decode_channel_image_device(fmt, d_blocks, width, height, d_px, pitch, nullptr);
            else
                api::untransform_decode_channel_image_device(fmt, d_t, 4, 0, width, height, false, d_px, pitch, nullptr);
            CHECK(hipDeviceSynchronize() == 0);
            CHECK(hipMemcpy(back.data(), d_px, back.size(), 2) == 0);
            CHECK(back == want);
        }
        hipFree(d_t), hipFree(d_blocks), hipFree(d_px);
    }
}

int main(int argc, char** argv)
{
    const bool gpu = argc > 1 && std::strcmp(argv[1], "gpu") == 0;
    try {
        cpu_tests();
        if (gpu) gpu_tests();
    } catch (const DeviceError& e) {
        std::printf("DeviceError %d: %s\n", e.code, e.what());
        return 2;
    }
    std::printf("%s: %d failure(s)\n", gpu ? "gpu" : "cpu", failures);
    return failures ? 1 : 0;
}
