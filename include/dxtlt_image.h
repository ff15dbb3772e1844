/*
 * dxtlt_image.h -- C ABI of the image decoders of libdxtlt_gfx950.so: BC1 / BC2 / BC3 blocks -> a row-major RGBA8888
 * image (BC4 / BC5 -> R8 / RG8: the last paragraph), from a plain block array or straight from a TRANSFORMED buffer (the inverse transform and the decoder in one
 * kernel: the untransformed blocks are never written to memory).  docs/IMAGE_DECODE.md has the definition in byte terms.
 *
 *   format    1, 2, 3 = BC1, BC2, BC3; anything else is DXTLT_E_INVALID_ARGUMENT.
 *   image     width x height pixels.  Its blocks are numbered row-major over ceil(width / 4) columns and ceil(height / 4)
 *             rows; block (bx, by) holds pixels (4 bx .. 4 bx + 3, 4 by .. 4 by + 3).
 *   pixels    pixel (x, y) is the four bytes r, g, b, a at pixels + y * pitch + 4 * x, exactly what the block decoders of
 *             dxtlt_decode.h produce (BC1's three-colour mode and the documented rounding included).  Pixels of the last
 *             block column / row that fall outside the image are not written, and neither is anything else: only bytes
 *             [y * pitch, y * pitch + 4 * width) of rows 0 .. height - 1 change.
 *   checks    in this order, before any device is touched: a NULL pointer with a non-empty image, pitch < 4 * width, pitch
 *             or the pixel pointer not a multiple of 4, decorrelation_mode > 3, first_block + blocks > total_blocks -- all
 *             DXTLT_E_INVALID_ARGUMENT -- and, host call only, len not a multiple of the block size: DXTLT_E_INVALID_LENGTH.
 *             width == 0 or height == 0 is DXTLT_OK and does nothing.
 *   alignment the block-side pointers may have any alignment; a pixel pointer and pitch that are multiples of 16 are the
 *             fast case.
 *   device    the *_device calls enqueue on `hip_stream` only, use no scratch memory and do not synchronise: they can be
 *             captured into a HIP graph.
 *   settings  as in dxtlt_transform_range_device (core numbering of the decorrelation mode); BC1 and BC2 ignore
 *             split_alpha_endpoints.
 *
 * BC4 / BC5 (single- and two-channel maps, UNORM) have calls of their own, the *_channel_image ones at the end: format 4, 5
 * = BC4, BC5, anything else is DXTLT_E_INVALID_ARGUMENT there (and 4, 5 stay invalid in the RGBA calls).
 *   pixels    bpp = 1 (BC4) or 2 (BC5) bytes: pixel (x, y) is r, or r, g, at pixels + y * pitch + bpp * x.  r (and g) is the
 *             alpha byte that the BC3 decoder of dxtlt_decode.h produces for the block's 8-byte (red / green) half; only bytes
 *             [y * pitch, y * pitch + bpp * width) of rows 0 .. height - 1 change.  Blocks, partial blocks and the block
 *             range are as above; a block is 8 (BC4) or 16 (BC5) bytes.
 *   checks    in this order, before any device is touched: the format; width == 0 or height == 0 is DXTLT_OK and does
 *             nothing; a NULL pointer; pitch < bpp * width; pitch or the pixel pointer not a multiple of bpp (a BC4 image may
 *             sit at any byte address with any pitch); first_block + blocks > total_blocks -- all DXTLT_E_INVALID_ARGUMENT --
 *             and, host call only, len not a multiple of the block size: DXTLT_E_INVALID_LENGTH.
 *   settings  split_endpoints, as in dxtlt_transform_range_device with format 4 / 5 (docs/BC45_FORMAT.md).
 *
 * Status codes and dxtlt_last_error() as in dxtlt_gfx950.h.
 */
#ifndef DXTLT_IMAGE_H
#define DXTLT_IMAGE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* blocks in block order (row-major over ceil(w/4) x ceil(h/4) blocks) -> RGBA8888 rows */
int32_t dxtlt_decode_image_device(int32_t format, const void *d_blocks, uint32_t width, uint32_t height,
                                  void *d_pixels, uint64_t pitch, void *hip_stream);

/* blocks [first_block, first_block + ceil(w/4)*ceil(h/4)) of a TRANSFORMED buffer of total_blocks -> the same image;
 * d_transformed is byte 0 of the whole transformed buffer, as in dxtlt_transform_range_device */
int32_t dxtlt_untransform_decode_image_device(int32_t format, const void *d_transformed, uint64_t total_blocks,
                                              uint64_t first_block, uint32_t width, uint32_t height,
                                              uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                              bool split_colour_endpoints, void *d_pixels, uint64_t pitch,
                                              void *hip_stream);

/* host pointers: one upload, the same kernel, one download of the rows (no pipelining); `transformed` is the whole
 * transformed buffer of len bytes (total_blocks = len / block size) */
int32_t dxtlt_untransform_decode_image(int32_t format, const uint8_t *transformed, size_t len, uint64_t first_block,
                                       uint32_t width, uint32_t height, uint8_t decorrelation_mode,
                                       bool split_alpha_endpoints, bool split_colour_endpoints,
                                       uint8_t *pixels, uint64_t pitch);

/* pure host arithmetic, no device: level `level` of a width x height texture with mip_count levels stored largest first.
 * Level k is max(1, width >> k) x max(1, height >> k) pixels = ceil(w_k / 4) * ceil(h_k / 4) blocks; first_block is the
 * sum of the levels in front of it, total_blocks the sum of all levels.  level >= mip_count, mip_count == 0 or a zero
 * width or height is DXTLT_E_INVALID_ARGUMENT.  An output pointer may be NULL.  Block counts do not depend on the format:
 * the answer serves BC4 / BC5 chains and the *_channel_image calls as it serves BC1 - BC3.
 * 256 x 256, 9 levels: total_blocks 5463; level 1 = 128 x 128, first_block 4096, 1024 blocks; level 3 = 32 x 32, 5376, 64;
 * level 7 = 2 x 2, 5461, 1; level 8 = 1 x 1, 5462, 1. */
int32_t dxtlt_image_mip_level(uint32_t width, uint32_t height, uint32_t mip_count, uint32_t level,
                              uint32_t *level_width, uint32_t *level_height,
                              uint64_t *first_block, uint64_t *num_blocks, uint64_t *total_blocks);

/* ---- BC4 / BC5 -> R8 / RG8 (format 4, 5; bpp = 1, 2) ---- */

/* blocks in block order -> rows of bpp-byte pixels */
int32_t dxtlt_decode_channel_image_device(int32_t format, const void *d_blocks, uint32_t width, uint32_t height,
                                          void *d_pixels, uint64_t pitch, void *hip_stream);

/* blocks [first_block, first_block + ceil(w/4)*ceil(h/4)) of a TRANSFORMED BC4 / BC5 buffer of total_blocks -> the same
 * image; d_transformed is byte 0 of the whole transformed buffer */
int32_t dxtlt_untransform_decode_channel_image_device(int32_t format, const void *d_transformed, uint64_t total_blocks,
                                                      uint64_t first_block, uint32_t width, uint32_t height,
                                                      bool split_endpoints, void *d_pixels, uint64_t pitch, void *hip_stream);

/* host pointers: one upload, the same kernel, one download of the rows; total_blocks = len / block size */
int32_t dxtlt_untransform_decode_channel_image(int32_t format, const uint8_t *transformed, size_t len, uint64_t first_block,
                                               uint32_t width, uint32_t height, bool split_endpoints,
                                               uint8_t *pixels, uint64_t pitch);

/* ---- several images of one buffer (format 1 .. 5; bpp = 4, 4, 4, 1, 2): docs/IMAGE_DECODE.md, "Several images of one buffer" ----
 *
 * An image region is one image and the block range it comes from: blocks [first_block, first_block + ceil(w/4)*ceil(h/4)) of
 * the buffer, numbered inside the region as an image's blocks are.  One call writes every region's image -- a mip chain, the
 * faces of a cube map -- with the pixel values, the partial blocks and the "nothing else is written" rule of the single-image
 * call for the format.
 *   regions   a HOST array, read during the call and never afterwards.  A region of zero width or height is skipped.  The
 *             others must come in ascending block order and must not overlap; gaps between them are legal, and a block that
 *             lies in no region is written nowhere.  The images must not overlap in memory (not checked).
 *   settings  as in dxtlt_transform_range_device: formats 4 / 5 take split_endpoints in split_alpha_endpoints and ignore the
 *             decorrelation mode and the colour split.
 *   checks    in this order, before any device is touched: the format; region_count == 0 or every region empty is DXTLT_OK
 *             and does nothing; a NULL buffer or `regions` pointer; for every non-empty region in list order a NULL `pixels`,
 *             pitch < bpp * width, pitch or `pixels` not a multiple of 4 (formats 1 - 3) or of bpp (formats 4, 5),
 *             first_block + blocks > total_blocks, a region that starts before the previous non-empty one ends; then
 *             decorrelation_mode > 3 for formats 1 - 3 -- all DXTLT_E_INVALID_ARGUMENT -- and, host call only, len not a
 *             multiple of the block size: DXTLT_E_INVALID_LENGTH.
 *   launches  the non-empty regions are taken in groups of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH consecutive ones; a group is
 *             one plan of the inverse transform over the range from its first block to the end of its last region (one or
 *             two launches), its table in the kernel arguments.  Blocks in gaps are loaded and dropped: a caller with a large
 *             gap makes two calls.
 *   device    the *_device calls enqueue on `hip_stream` only, allocate nothing, copy nothing to the device but kernel
 *             arguments and do not synchronise: they can be captured into a HIP graph, the table frozen at capture.
 */
#define DXTLT_IMAGE_REGIONS_PER_LAUNCH 16

typedef struct DxtltImageRegion {
    uint64_t first_block;     /* index into the buffer's blocks */
    uint32_t width, height;   /* pixels; a zero width or height: the region is skipped */
    void    *pixels;          /* device (or, in the host call, host) pointer */
    uint64_t pitch;
} DxtltImageRegion;

/* a TRANSFORMED device buffer of total_blocks, any alignment -> every region's device image */
int32_t dxtlt_untransform_decode_images_device(int32_t format, const void *d_transformed, uint64_t total_blocks,
                                               const DxtltImageRegion *regions, size_t region_count,
                                               uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                               bool split_colour_endpoints, void *hip_stream);

/* a device block array of total_blocks in block order, any alignment -> the same */
int32_t dxtlt_decode_images_device(int32_t format, const void *d_blocks, uint64_t total_blocks,
                                   const DxtltImageRegion *regions, size_t region_count, void *hip_stream);

/* host pointers: one upload of the whole transformed buffer of len bytes, the same kernels into staging (every region's
 * base a multiple of 16, its rows a multiple of 16 bytes apart), one strided download per region */
int32_t dxtlt_untransform_decode_images(int32_t format, const uint8_t *transformed, size_t len,
                                        const DxtltImageRegion *regions, size_t region_count,
                                        uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                        bool split_colour_endpoints);

/* pure host arithmetic, no device: first_block, width and height of regions[0 .. mip_count) for a width x height chain of
 * mip_count levels whose level 0 starts at block first_block -- level k exactly as dxtlt_image_mip_level has it, first_block
 * added.  `pixels` and `pitch` are left alone.  *total_blocks (may be NULL) = the block just behind the chain.  A zero width,
 * height or mip_count, or a NULL `regions`, is DXTLT_E_INVALID_ARGUMENT. */
int32_t dxtlt_image_mip_chain(uint32_t width, uint32_t height, uint32_t mip_count, uint64_t first_block,
                              DxtltImageRegion *regions, uint64_t *total_blocks);

/* ---- many buffers in one call (docs/IMAGE_DECODE.md, "Many buffers in one call") ----
 *
 * One item is one dxtlt_untransform_decode_images_device call: a transformed device buffer, its regions and its settings.  For
 * every item the call writes exactly the bytes that call writes for the item alone -- pixel values, partial blocks, "nothing
 * else is written", gaps, empty regions -- but a whole batch goes out as ONE launch per (format, decorrelation mode, alpha
 * split, colour split) present in it, whatever the number of items: thousands of small mip chains cost one launch, not one
 * each.
 *   items     a HOST array, and every item's `regions` a host array, read during the call and never afterwards.  Items may mix
 *             formats, settings, sizes and alignments; two items may name the same buffer (buffers are only read).  The
 *             images of a batch must not overlap one another (not checked).
 *   checks    the whole batch before anything is enqueued: it goes out whole or not at all.  count == 0 is DXTLT_OK; a NULL
 *             `items` with count > 0 is DXTLT_E_INVALID_ARGUMENT; then the items in list order, each with the checks of
 *             dxtlt_untransform_decode_images_device in that call's order.  The first failure is the answer, and
 *             dxtlt_last_error() names the item's index.  An item without a non-empty region is skipped, its buffer pointer
 *             unchecked, as in the single call.
 *   launches  an item's non-empty regions are taken in groups of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH, each group one range
 *             of the inverse transform -- from its first block to the end of its last region -- planned for its address as the
 *             single call plans it.  The groups of one format and settings share a launch, launches in the order in which
 *             their settings first appear in the list.  A group of a buffer whose stream shifts are not multiples of the
 *             stream element widths (a buffer address that is not a multiple of 8, say) goes out alone through the single
 *             call's kernels, behind the batch launches.
 *   limit     one launch holds at most 16777215 (2^24 - 1) tiles -- a tile is 256 lanes' worth of blocks: 512 BC1 / BC4
 *             blocks, 256 of the others; every group takes ceil(range blocks / tile) of them.  A batch that needs more for
 *             one format and settings is DXTLT_E_INVALID_ARGUMENT, and nothing is enqueued.
 *   device    asynchronous on `hip_stream`, ordered like a single call.  The call stages its tables (entries, workgroup index,
 *             region tables) in one of four pinned slots of the calling thread and uploads them on the stream, as
 *             dxtlt_transform_batch_device does; it blocks the host only when four earlier batch calls of the thread are all
 *             still in flight.  Capture into a HIP graph is NOT promised (the tables are staged per call), as for
 *             dxtlt_transform_batch_device.
 */
typedef struct DxtltImageBatchItem {
    const void *d_transformed;        /* byte 0 of the item's WHOLE transformed device buffer, any alignment */
    uint64_t total_blocks;
    const DxtltImageRegion *regions;  /* host array; pixels = device pointers; the rules of the *_images calls */
    uint32_t region_count;
    uint8_t format;                   /* 1..5 */
    uint8_t decorrelation_mode;       /* as dxtlt_untransform_decode_images_device takes them */
    uint8_t split_alpha_endpoints;    /* formats 4 / 5: split_endpoints */
    uint8_t split_colour_endpoints;
} DxtltImageBatchItem;

int32_t dxtlt_untransform_decode_images_batch_device(const DxtltImageBatchItem *items, size_t count, void *hip_stream);

/* Test hook, no device needed: what dxtlt_untransform_decode_images_batch_device would enqueue for the batch.  Addresses are
 * numbers; nothing is dereferenced but `items` and the items' `regions`.  One record per entry -- a group of at most
 * DXTLT_IMAGE_REGIONS_PER_LAUNCH non-empty regions of an item -- in list order; records beyond `cap` are counted, not written.
 * Returns the number of entries, or -1 for a batch the call would refuse. */
typedef struct DxtltDebugImageBatchEntry {
    uint32_t item;            /* index of the entry's item */
    uint32_t first_region;    /* index in the item's list of the group's first region */
    uint32_t region_count;    /* non-empty regions of the group */
    int32_t  launch;          /* number of the batch launch that holds the entry; -1: launched alone, behind them */
    uint32_t first_wg, end_wg;/* its workgroups in that launch (both 0 for an entry launched alone) */
    uint32_t full_tiles;      /* whole tiles among them; one more workgroup, if there is one, is the edge tile */
    uint32_t form;            /* 1: every stream base of the range on a 128-byte line (aligned tiles); 0: shifted tiles */
    uint64_t first_block;     /* the range: from the group's first block ... */
    uint64_t range_blocks;    /* ... to the end of its last region */
    uint32_t wide_index;      /* 1: the launch's workgroup index has the wide (16-bit) form */
    uint32_t launch_wgs;      /* workgroups of the whole launch */
} DxtltDebugImageBatchEntry;

int32_t dxtlt_debug_plan_image_batch(const DxtltImageBatchItem *items, size_t count, DxtltDebugImageBatchEntry *out, size_t cap);

#ifdef __cplusplus
}
#endif
#endif
