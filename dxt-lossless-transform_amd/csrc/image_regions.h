// image_regions.h -- several images of one block buffer (include/dxtlt_image.h, "image regions"; docs/IMAGE_DECODE.md, "Several
// images of one buffer"): the table one launch carries in its kernel arguments and the lookup from a block of the buffer to its
// image.  Host and device code, beside image_sink.h; the tests build it for the host.
//
// Region i is the image img[i] and the blocks [first[i], first[i] + blocks[i]) of the buffer, blocks[i] = image_blocks(img[i]),
// numbered inside the region as image_sink.h numbers an image's blocks.  The regions ascend and do not overlap; a block may lie
// in none (a gap).  Entries [count, kImageRegionsPerLaunch) are cleared (blocks == 0: no block is ever found in them).
#pragma once
#include "image_sink.h"

// The lookups are written once for every kind of table: a TABLE answers regions(), first_of(i), blocks_of(i) and image_of(i).
//
// Both lookups below are loops that stay loops.  Unrolled over the sixteen entries, the walks of one kernel read the table in
// many hundreds of places, and from a few hundred on the compiler no longer reads a by-value kernel argument in place: it
// copies the whole table to scratch memory first (seen in the BC1 and BC4 shifted kernels, whose two blocks per lane double the
// walks).  As a loop over `count` entries a walk reads the table in a dozen places with the loop counter -- the same number in
// every lane -- as the index: scalar loads from the kernel arguments, no scratch, and it ends at the last region in use.
#ifdef __HIPCC__
#define DXTLT_REGIONS_LOOP _Pragma("nounroll")
#else
#define DXTLT_REGIONS_LOOP
#endif

namespace dxtlt {

constexpr int kImageRegionsPerLaunch = 16;   // DXTLT_IMAGE_REGIONS_PER_LAUNCH: a full mip chain up to 32768 x 32768

struct ImageRegionTable {
    ImageSink img[kImageRegionsPerLaunch];
    uint64_t first[kImageRegionsPerLaunch];
    uint64_t blocks[kImageRegionsPerLaunch];
    uint32_t count;

    // what the lookups below ask of a table (image_batch_kernels.hip has the one that lives in device memory); the index keeps
    // the type the lookup has it in
    __host__ __device__ uint32_t regions() const { return count; }
    template <typename I> __host__ __device__ uint64_t first_of(I i) const { return first[i]; }
    template <typename I> __host__ __device__ uint64_t blocks_of(I i) const { return blocks[i]; }
    template <typename I> __host__ __device__ const ImageSink& image_of(I i) const { return img[i]; }
};
static_assert(sizeof(ImageRegionTable) <= 1024, "the table travels in the kernel arguments");

inline void clear_regions(ImageRegionTable& t)
{
    t.count = 0;
    for (int i = 0; i < kImageRegionsPerLaunch; ++i) {
        t.img[i] = ImageSink{nullptr, 0, 0, 0, 0, 0};
        t.first[i] = t.blocks[i] = 0;
    }
}

// appends a non-empty region behind the ones the table has (count < kImageRegionsPerLaunch)
inline void append_region(ImageRegionTable& t, const ImageSink& img, uint64_t first_block)
{
    t.img[t.count] = img;
    t.first[t.count] = first_block;
    t.blocks[t.count] = image_blocks(img);
    ++t.count;
}

// the range that covers the table's regions; false when the table is not one the kernels take
inline bool covering_range(const ImageRegionTable& tab, uint64_t total_blocks, uint64_t& first, uint64_t& n)
{
    if (tab.count == 0 || tab.count > (uint32_t)kImageRegionsPerLaunch)
        return false;
    uint64_t end = 0;
    for (uint32_t i = 0; i < tab.count; ++i) {
        if (tab.blocks[i] == 0 || tab.blocks[i] != image_blocks(tab.img[i]) || tab.first[i] < end || tab.first[i] > total_blocks ||
            tab.blocks[i] > total_blocks - tab.first[i])
            return false;
        end = tab.first[i] + tab.blocks[i];
    }
    for (int i = (int)tab.count; i < kImageRegionsPerLaunch; ++i)
        if (tab.blocks[i] != 0)
            return false;
    first = tab.first[0];
    n = end - first;
    return true;
}

// Is block `b` of the buffer in region i?  `local` = its number inside the region.  (b < first[i] wraps to a number that no
// region has blocks for: one comparison.)
template <typename TABLE>
__host__ __device__ inline bool in_region(const TABLE& t, int i, uint64_t b, uint64_t& local)
{
    local = b - t.first_of(i);
    return local < t.blocks_of(i);
}

// The region that holds all of the blocks [b, b + n), n >= 1, or -1: these blocks straddle a boundary, or some lie in a gap.
// `img` and `local` are then the region's image and the number of block `b` in it.  This is the question a wave asks about its
// 64 or 128 consecutive blocks with `b` in scalar registers: every condition below is the same in all lanes, so what is found
// stays in scalar registers and serves every lane.
template <typename TABLE>
__host__ __device__ inline int region_of_run(const TABLE& t, uint64_t b, uint64_t n, ImageSink& img, uint64_t& local)
{
    DXTLT_REGIONS_LOOP
    for (uint32_t i = 0; i < t.regions(); ++i) {
        uint64_t d;
        if (in_region(t, (int)i, b, d) && n <= t.blocks_of(i) - d) {
            local = d;
            img = t.image_of(i);
            return (int)i;
        }
    }
    return -1;
}

// The region of ONE block, each lane with a `b` of its own: -1 = the block lies in no region; otherwise `img` and `local` are
// the region's image and the block's number in it.  The walk over the regions is uniform -- every lane compares with region i at
// the same time and keeps what matches, field by field -- so the table is never indexed with a per-lane number.
template <typename TABLE>
__host__ __device__ inline int region_of_block(const TABLE& t, uint64_t b, ImageSink& img, uint64_t& local)
{
    int found = -1;
    DXTLT_REGIONS_LOOP
    for (uint32_t i = 0; i < t.regions(); ++i) {
        uint64_t d;
        if (in_region(t, (int)i, b, d)) {
            found = (int)i;
            local = d;
            img = t.image_of(i);
        }
    }
    return found;
}

}  // namespace dxtlt
