// C++ mirror of the fused BC2 / BC3 normalise + transform calls (include/dxt_lossless_transform.hpp:
// core::experimental::bc2::transform_bc2_with_normalize_blocks, core::experimental::bc3::transform_bc3_with_normalize_blocks),
// driven by tests/test_normalize_fused_bc23_gpu.py.
//   test_cpp_normalize_fused_bc23 bc2|bc3 IN OUT alpha_mode color_mode decorrelation_mode split_alpha split_colour
// reads the blocks of file IN, transforms them through the wrapper (host pointers) and writes the result to file OUT; before
// that it checks that a bad argument comes back as a DeviceError with code 2 (no device needed for those).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dxt_lossless_transform.hpp"

using namespace dxt_lossless_transform;
namespace ex = core::experimental;

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

int main(int argc, char** argv)
{
    if (argc != 9) {
        std::printf("usage: %s bc2|bc3 IN OUT alpha_mode color_mode decorrelation_mode split_alpha split_colour\n", argv[0]);
        return 2;
    }
    const bool bc3 = std::strcmp(argv[1], "bc3") == 0;
    const int alpha = std::atoi(argv[4]), colour = std::atoi(argv[5]), variant = std::atoi(argv[6]);
    const bool sa = std::atoi(argv[7]) != 0, sc = std::atoi(argv[8]) != 0;

    uint8_t a[32] = {0}, b[32] = {0};
    int bad = 0;
    bad += thrown_code([&] { ex::bc2::transform_bc2_with_normalize_blocks(a, b, 24, ex::bc2::ColorNormalizationMode::Color0Only); }) != 2;
    bad += thrown_code([&] { ex::bc2::transform_bc2_with_normalize_blocks(a, b, 16, static_cast<ex::bc2::ColorNormalizationMode>(3)); }) != 2;
    bad += thrown_code([&] {
        ex::bc3::transform_bc3_with_normalize_blocks(a, b, 16, static_cast<ex::bc3::AlphaNormalizationMode>(4),
                                                     ex::bc3::ColorNormalizationMode::Color0Only);
    }) != 2;
    bad += thrown_code([&] {
        ex::bc3::transform_bc3_with_normalize_blocks(nullptr, b, 16, ex::bc3::AlphaNormalizationMode::OpaqueFillAll,
                                                     ex::bc3::ColorNormalizationMode::ReplicateColor);
    }) != 2;
    bad += thrown_code([&] {
        ex::bc3::transform_bc3_with_normalize_blocks(nullptr, nullptr, 0, ex::bc3::AlphaNormalizationMode::OpaqueFillAll,
                                                     ex::bc3::ColorNormalizationMode::ReplicateColor);
    }) != 0;
    if (bad) {
        std::printf("FAIL: %d argument checks\n", bad);
        return 1;
    }

    std::FILE* in = std::fopen(argv[2], "rb");
    if (!in)
        return 2;
    std::vector<uint8_t> x;
    uint8_t buf[4096];
    for (size_t n; (n = std::fread(buf, 1, sizeof buf, in)) > 0;)
        x.insert(x.end(), buf, buf + n);
    std::fclose(in);
    std::vector<uint8_t> y(x.size());
    try {
        if (bc3) {
            core::Bc3TransformSettings s;
            s.decorrelation_mode = static_cast<core::YCoCgVariant>(variant);
            s.split_alpha_endpoints = sa;
            s.split_colour_endpoints = sc;
            ex::bc3::transform_bc3_with_normalize_blocks(x.data(), y.data(), x.size(), static_cast<ex::bc3::AlphaNormalizationMode>(alpha),
                                                         static_cast<ex::bc3::ColorNormalizationMode>(colour), s);
        } else {
            core::Bc2TransformSettings s;
            s.decorrelation_mode = static_cast<core::YCoCgVariant>(variant);
            s.split_colour_endpoints = sc;
            ex::bc2::transform_bc2_with_normalize_blocks(x.data(), y.data(), x.size(), static_cast<ex::bc2::ColorNormalizationMode>(colour), s);
        }
    } catch (const DeviceError& e) {
        std::printf("FAIL: DeviceError %d: %s\n", e.code, e.what());
        return 1;
    }
    std::FILE* out = std::fopen(argv[3], "wb");
    if (!out || std::fwrite(y.data(), 1, y.size(), out) != y.size())
        return 2;
    std::fclose(out);
    return 0;
}
