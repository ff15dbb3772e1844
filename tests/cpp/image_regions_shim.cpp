// Host build of csrc/image_regions.h for tests/test_image_regions_layout.py: the region table a launch carries and both lookups,
// for every block index the test asks about.  Addresses are numbers: nothing is dereferenced.
#include <cstddef>
#include <cstdint>
#define __host__
#define __device__
#include "../../dxt-lossless-transform_amd/csrc/image_regions.h"

namespace {

dxtlt::ImageRegionTable table_of(size_t count, const uint64_t* first, const uint32_t* width, const uint32_t* height, const uint64_t* base,
                                 const uint64_t* pitch, uint32_t bpp)
{
    dxtlt::ImageRegionTable t;
    dxtlt::clear_regions(t);
    for (size_t i = 0; i < count; ++i)
        dxtlt::append_region(t, dxtlt::make_image_sink(reinterpret_cast<void*>(static_cast<uintptr_t>(base[i])), pitch[i], width[i], height[i], bpp),
                             first[i]);
    return t;
}

}  // namespace

extern "C" {

int shim_regions_per_launch() { return dxtlt::kImageRegionsPerLaunch; }
size_t shim_region_table_bytes() { return sizeof(dxtlt::ImageRegionTable); }

// For blocks [b0, b0 + n) of the buffer: region[k] = the region of block b0 + k or -1, local[k] its number in the region, and
// place[6 k ..] = bx, by, cols, rows, offset from the region's pixel pointer (two words: low, high) of its BlockPlace; address[k]
// = the address of its pixel (0, 0).  `count` <= kImageRegionsPerLaunch regions.
void shim_region_of_block(size_t count, const uint64_t* first, const uint32_t* width, const uint32_t* height, const uint64_t* base,
                          const uint64_t* pitch, uint32_t bpp, uint64_t b0, size_t n, int32_t* region, uint64_t* local,
                          uint32_t* place, uint64_t* address)
{
    const dxtlt::ImageRegionTable t = table_of(count, first, width, height, base, pitch, bpp);
    for (size_t k = 0; k < n; ++k) {
        dxtlt::ImageSink img{nullptr, 0, 1, 0, 0, bpp};
        uint64_t l = 0;
        region[k] = dxtlt::region_of_block(t, b0 + k, img, l);
        local[k] = 0, address[k] = 0;
        for (int j = 0; j < 6; ++j)
            place[6 * k + j] = 0;
        if (region[k] < 0)
            continue;
        local[k] = l;
        const dxtlt::BlockPlace p = dxtlt::place_block(img, l);
        place[6 * k] = p.bx, place[6 * k + 1] = p.by, place[6 * k + 2] = p.cols, place[6 * k + 3] = p.rows;
        place[6 * k + 4] = (uint32_t)p.offset, place[6 * k + 5] = (uint32_t)(p.offset >> 32);
        address[k] = static_cast<uint64_t>(reinterpret_cast<uintptr_t>(dxtlt::block_row(img, p, 0)));
    }
}

// For runs [b0 + k, b0 + k + run) of the buffer, k < n: region[k] = the region that holds the whole run or -1, local[k] the
// number of the run's first block in it, address[k] the region's pixel pointer
void shim_region_of_run(size_t count, const uint64_t* first, const uint32_t* width, const uint32_t* height, const uint64_t* base,
                        const uint64_t* pitch, uint32_t bpp, uint64_t b0, size_t n, uint64_t run, int32_t* region, uint64_t* local,
                        uint64_t* address)
{
    const dxtlt::ImageRegionTable t = table_of(count, first, width, height, base, pitch, bpp);
    for (size_t k = 0; k < n; ++k) {
        dxtlt::ImageSink img{nullptr, 0, 1, 0, 0, bpp};
        uint64_t l = 0;
        region[k] = dxtlt::region_of_run(t, b0 + k, run, img, l);
        local[k] = region[k] < 0 ? 0 : l;
        address[k] = region[k] < 0 ? 0 : static_cast<uint64_t>(reinterpret_cast<uintptr_t>(img.pixels));
    }
}

}  // extern "C"
