// C++ mirror of the normalising batch calls (include/dxt_lossless_transform.hpp: core::transform_batch_with_normalize_blocks_device,
// batch_any_normalizable_device), driven by tests/test_batch_normalize_gpu.py.
//   test_cpp_batch_normalize { 1|2|3 IN OUT alpha_mode color_mode decorrelation_mode split_alpha split_colour } ...
// One batch item per group of eight arguments: the blocks of file IN (format BC1 / BC2 / BC3) go to the device, ONE call transforms
// all items, every result is written to its file OUT, and "flags f0 f1 ..." -- batch_any_normalizable_device's answer for the same
// items -- goes to standard output.  Before that a bad item must come back as a DeviceError with code 2 (no device needed).
#include <cstdio>
#include <cstdlib>
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
    if (argc < 9 || (argc - 1) % 8 != 0) {
        std::printf("usage: %s { 1|2|3 IN OUT alpha_mode color_mode decorrelation_mode split_alpha split_colour } ...\n", argv[0]);
        return 2;
    }
    int dummy = 0;
    DxtltBatchNormalizeItem bad{&dummy, &dummy, 16, 3, 4, 0, 0, 0, 0, {0, 0}};   // alpha mode 4
    if (thrown_code([&] { core::transform_batch_with_normalize_blocks_device(&bad, 1, nullptr); }) != 2 ||
        thrown_code([&] { core::transform_batch_with_normalize_blocks_device(nullptr, 0, nullptr); }) != 0 ||
        thrown_code([&] { core::batch_any_normalizable_device(&bad, 1, nullptr, nullptr); }) != 2) {
        std::printf("FAIL: argument checks\n");
        return 1;
    }
    const size_t count = (size_t)(argc - 1) / 8;
    std::vector<std::vector<uint8_t>> data(count);
    std::vector<DxtltBatchNormalizeItem> items(count);
    for (size_t k = 0; k < count; ++k) {
        char** a = argv + 1 + 8 * k;
        std::FILE* in = std::fopen(a[1], "rb");
        if (!in)
            return 2;
        uint8_t buf[4096];
        for (size_t n; (n = std::fread(buf, 1, sizeof buf, in)) > 0;)
            data[k].insert(data[k].end(), buf, buf + n);
        std::fclose(in);
        void *d_in = nullptr, *d_out = nullptr;
        if (hipMalloc(&d_in, data[k].size()) != 0 || hipMalloc(&d_out, data[k].size()) != 0 ||
            hipMemcpy(d_in, data[k].data(), data[k].size(), 1 /* host to device */) != 0)
            return 2;
        items[k] = DxtltBatchNormalizeItem{d_in, d_out, data[k].size(), (uint8_t)std::atoi(a[0]), (uint8_t)std::atoi(a[3]),
                                           (uint8_t)std::atoi(a[4]), (uint8_t)std::atoi(a[5]), (uint8_t)std::atoi(a[6]), (uint8_t)std::atoi(a[7]), {0, 0}};
    }
    std::vector<uint32_t> flags(count, 7);
    void* d_flags = nullptr;
    if (hipMalloc(&d_flags, count * sizeof(uint32_t)) != 0 || hipMemcpy(d_flags, flags.data(), count * sizeof(uint32_t), 1) != 0)
        return 2;
    try {
        core::transform_batch_with_normalize_blocks_device(items.data(), count, nullptr);
        core::batch_any_normalizable_device(items.data(), count, static_cast<uint32_t*>(d_flags), nullptr);
    } catch (const DeviceError& e) {
        std::printf("FAIL: DeviceError %d: %s\n", e.code, e.what());
        return 1;
    }
    if (hipDeviceSynchronize() != 0 || hipMemcpy(flags.data(), d_flags, count * sizeof(uint32_t), 2 /* device to host */) != 0)
        return 2;
    for (size_t k = 0; k < count; ++k) {
        std::vector<uint8_t> y(data[k].size());
        if (hipMemcpy(y.data(), items[k].d_output, y.size(), 2) != 0)
            return 2;
        std::FILE* out = std::fopen(argv[1 + 8 * k + 2], "wb");
        if (!out || std::fwrite(y.data(), 1, y.size(), out) != y.size())
            return 2;
        std::fclose(out);
        hipFree(const_cast<void*>(items[k].d_input));
        hipFree(items[k].d_output);
    }
    hipFree(d_flags);
    std::printf("flags");
    for (uint32_t f : flags)
        std::printf(" %u", f);
    std::printf("\n");
    return 0;
}
