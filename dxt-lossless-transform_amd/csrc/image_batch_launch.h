// image_batch_launch.h -- the tables of a batch image launch (image_batch_kernels.hip; include/dxtlt_image.h,
// dxtlt_untransform_decode_images_batch_device; docs/IMAGE_DECODE.md, "Many buffers in one call") and its launch interface for
// image_batch_api.cpp.  Host and device code.
#pragma once
#include "bcn_launch.h"
#include "image_sink.h"

namespace dxtlt {

// One region of an entry as it lies in DEVICE memory: the block range and the image side by side in one 64-byte record on a
// 64-byte address, so that a wave whose run lies in the entry's first region -- level 0 of a chain: three blocks of four --
// touches ONE line of the scalar cache for its lookup (what a lookup costs is its scalar-cache misses: bcn_launch.h), and a
// small item's workgroup, which sees its table for the first time, fetches nothing it does not read.  Only the regions an
// entry has are stored.
struct ImageBatchRegion {
    uint64_t first, blocks;   // blocks [first, first + blocks) of the buffer; blocks = image_blocks of the image
    uint64_t pixels;          // ImageSink, field by field
    uint64_t pitch;
    uint64_t blocks_per_row;
    uint32_t width, height;
    uint32_t bpp;
    uint32_t reserved[3];
};
static_assert(sizeof(ImageBatchRegion) == 64, "one region, one cache line");

inline ImageBatchRegion make_batch_region(const ImageSink& img, uint64_t first_block)
{
    return ImageBatchRegion{first_block, image_blocks(img), reinterpret_cast<uintptr_t>(img.pixels), img.pitch, img.blocks_per_row,
                            img.width, img.height, img.bpp, {0, 0, 0}};
}

// One entry per group of at most kImageRegionsPerLaunch regions of an item, in workgroup order: the inverse transform's plan
// for the range [first_block, first_block + range_blocks) of the item's buffer -- from the group's first block to the end of
// its last region -- with tiles of batch_tile_threads(fmt, split_colour, true) lanes.  The first 96 bytes are a BatchEntry
// (bcn_launch.h) in which the region table stands where the destination does and `blocks` is the WHOLE buffer's count: the
// workgroup lookup (batch_lookup.h) is the batch transform's.
struct ImageBatchEntry {
    const uint8_t* src;                 // byte 0 of the whole transformed buffer
    const ImageBatchRegion* regions;    // device memory, on a 64-byte address
    uint64_t total_blocks;
    uint32_t first_wg;
    uint32_t end_wg;
    uint32_t full_tiles;
    uint8_t form;           // 1: every stream base of the range on a 128-byte line (aligned tiles); 0: shifted tiles
    uint8_t region_count;   // 1 .. kImageRegionsPerLaunch
    uint8_t natural;        // always 1 (plan_image_batch_entry hands other ranges back)
    uint8_t reserved;
    uint8_t shift[6];       // stream base of the range modulo 16
    uint8_t reserved2[2];
    uint64_t gbase[6];      // Shifts::gbase of the range
    uint64_t first_block;   // of the range
    uint64_t range_blocks;
    uint64_t reserved3[2];
};
static_assert(sizeof(ImageBatchEntry) == 128, "ImageBatchEntry layout is shared between host and device");

// Fills the planning fields of `e` (src, total_blocks, first_block, range_blocks and first_wg set by the caller) for settings
// `s` and returns the workgroups the range needs, or 0xFFFFFFFF when the batch kernel cannot take it (stream shifts that are
// not multiples of the element widths: the caller launches the group alone).  The range form of plan_batch_entry.
uint32_t plan_image_batch_entry(Format fmt, const Settings& s, ImageBatchEntry& e);

// d_entries / d_index as in launch_batch (build_batch_index over the entries' end_wg); every tile of the launch has
// batch_tile_threads(fmt, split_colour, true) lanes.
hipError_t launch_image_batch(Format fmt, const Settings& s, const ImageBatchEntry* d_entries, const uint8_t* d_index,
                              uint32_t n_entries, uint32_t total_wgs, bool wide_index, hipStream_t stream);

}  // namespace dxtlt
