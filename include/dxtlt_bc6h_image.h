/*
 * dxtlt_bc6h_image.h -- C ABI of the BC6H decoders of libdxtlt_gfx950.so: BC6H blocks -> RGBA16F pixels
 * (docs/IMAGE_DECODE.md, "BC6H blocks to a row-major RGBA16F image").
 *
 * The decoder is Direct3D 11's for the UNSIGNED format (UF16, DXGI BC6H_UF16): every mode with its partitions and deltas; the
 * four reserved mode values decode to r = g = b = 0.  A pixel is four little-endian half-float bit patterns r, g, b, a -- eight
 * bytes, DXGI R16G16B16A16_FLOAT -- and a is always 0x3C00 (1.0).  There is no signedness argument: signed (SF16) blocks are
 * not decoded by these calls (the document has the finding that decides it); a later decoder gets names of its own.
 *
 *   dxtlt_decode_bc6h_blocks*         `len / 16` blocks -> that many 128-byte records: sixteen pixels in row-major order, pixel
 *                                     4 r + c at (c, r).  The host-pointer call decodes on the CPU with the code the kernels
 *                                     use and needs no device.
 *   dxtlt_decode_bc6h_image_device    ceil(width / 4) * ceil(height / 4) blocks in block order -> a row-major image: pixel
 *                                     (x, y) at pixels + y * pitch + 8 * x.  Nothing else of the image's memory is written.
 *   dxtlt_untransform_decode_bc6h_image*
 *                                     the same from the blocks [first_block, first_block + image blocks) of a buffer
 *                                     TRANSFORMED by dxtlt_transform_bc6h (dxtlt_bc6h.h), of `total_blocks` (`len / 16`)
 *                                     blocks in all, in one pass: the untransformed blocks never touch memory.
 *                                     `first_block` may be any block.  At most two launches; nothing is allocated or copied
 *                                     by the device call, there is no synchronisation, and it can be captured into a graph.
 *
 * Checks, in this order, all before a device is touched (status codes and dxtlt_last_error() as in dxtlt_gfx950.h):
 *   1. width == 0 or height == 0: DXTLT_OK, nothing is done;
 *   2. a NULL pointer: DXTLT_E_INVALID_ARGUMENT (2);
 *   3. pitch < 8 * width: 2;
 *   4. pitch or the pixel pointer not a multiple of 8: 2;
 *   5. first_block + image blocks > total_blocks (wrap-safe): 2;
 *   6. host call only: len not a multiple of 16: DXTLT_E_INVALID_LENGTH (1).
 * The block calls: len not a multiple of 16: 1; a NULL pointer with len > 0, or pixels_len < 128 * blocks: 2.
 *
 * Several images of one BC6H buffer -- a mip chain, the faces of a cube map, the slices of an array -- in one call
 * (docs/IMAGE_DECODE.md, "Several images of one BC6H buffer"): the dxtlt_*_bc6h_images* calls take the DxtltImageRegion list of
 * dxtlt_image.h ("several images of one buffer") with that section's rules -- the non-empty regions ascend and do not overlap,
 * gaps are legal and a block in a gap is written nowhere, empty regions are skipped, a region's first_block may be any block --
 * and write, for every region, exactly the bytes the single-image call above writes for that region alone (for a block array:
 * dxtlt_decode_bc6h_image_device), clipped blocks and pitch padding included; nothing else is written.
 *   checks    in this order, before any device is touched: region_count == 0 or every region empty is DXTLT_OK and does
 *             nothing; a NULL buffer or `regions` pointer; for every non-empty region in list order a NULL `pixels`,
 *             pitch < 8 * width, pitch or `pixels` not a multiple of 8, first_block + blocks > total_blocks (wrap-safe), a
 *             region that starts before the previous non-empty one ends -- all DXTLT_E_INVALID_ARGUMENT -- and, host call
 *             only, len not a multiple of 16: DXTLT_E_INVALID_LENGTH.
 *   launches  the non-empty regions are taken in groups of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH consecutive ones.  The fused
 *             call covers a group's range, from its first block to the end of its last region, as the single-image call covers
 *             one image: one launch over the main part's granules that the range touches (split at 2^21 granules) and one over
 *             the tail part if the range reaches it.  Every granule is un-sorted and decoded once per group; blocks in gaps are
 *             decoded and dropped.  The block-array call is one launch per group.
 *   device    the *_device calls enqueue on `hip_stream` only, allocate nothing, copy nothing to the device but kernel
 *             arguments and do not synchronise: they can be captured into a HIP graph, the table frozen at capture.
 *
 * The images of MANY BC6H transformed buffers in one call (docs/IMAGE_DECODE.md, "Many BC6H buffers in one call"):
 * dxtlt_untransform_decode_bc6h_images_batch_device takes one DxtltBc6hImageBatchItem per buffer and writes, for every item,
 * exactly the bytes dxtlt_untransform_decode_bc6h_images_device writes for that item alone.  Items may differ in size, alignment
 * and region layout, and two items may name the same buffer; the images of a batch must not overlap (not checked).
 *   checks    the whole batch before anything is enqueued -- it goes out whole or not at all: count == 0 is DXTLT_OK; a NULL
 *             `items` with count > 0 is DXTLT_E_INVALID_ARGUMENT; then the items in list order, each with the checks of
 *             dxtlt_untransform_decode_bc6h_images_device in their order.  The first failure is the answer and
 *             dxtlt_last_error() names the item ("bc6h image batch item 7: ...").  An item without a non-empty region is
 *             skipped, its buffer pointer unchecked.  A batch that needs more than 16777215 granules (of 1024 blocks) or more
 *             than 16777215 tail parts is DXTLT_E_INVALID_ARGUMENT.
 *   launches  every group of at most DXTLT_IMAGE_REGIONS_PER_LAUNCH non-empty regions of an item is one entry, covered as the
 *             single call covers it; all entries' granules go out in ONE launch and all their tail parts in a second one: at
 *             most two launches, whatever the number of items.
 *   device    asynchronous on `hip_stream`, ordered like a single call.  The call stages its tables in pinned memory of the
 *             calling thread (dxtlt_release_thread_resources frees it) and uploads them on the stream in front of the
 *             launches; capture into a HIP graph is not promised.
 *
 * The RGBA image calls of dxtlt_image.h, their region and batch calls and the BC7 calls of dxtlt_bc7_image.h do not take BC6H.
 */
#ifndef DXTLT_BC6H_IMAGE_H
#define DXTLT_BC6H_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#include "dxtlt_image.h" /* DxtltImageRegion, DXTLT_IMAGE_REGIONS_PER_LAUNCH */

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host pointers ---------------------------------------------------------------------------------- */
int32_t dxtlt_decode_bc6h_blocks(const uint8_t *blocks, size_t len, uint8_t *pixels, size_t pixels_len);
int32_t dxtlt_untransform_decode_bc6h_image(const uint8_t *transformed, size_t len, uint64_t first_block, uint32_t width,
                                            uint32_t height, uint8_t *pixels, uint64_t pitch);

/* ---- device pointers, asynchronous on `hip_stream` --------------------------------------------------- */
int32_t dxtlt_decode_bc6h_blocks_device(const void *d_blocks, size_t len, void *d_pixels, size_t pixels_len, void *hip_stream);
int32_t dxtlt_decode_bc6h_image_device(const void *d_blocks, uint32_t width, uint32_t height, void *d_pixels, uint64_t pitch,
                                       void *hip_stream);
int32_t dxtlt_untransform_decode_bc6h_image_device(const void *d_transformed, uint64_t total_blocks, uint64_t first_block,
                                                   uint32_t width, uint32_t height, void *d_pixels, uint64_t pitch,
                                                   void *hip_stream);

/* ---- several images of one buffer ------------------------------------------------------------------------ */
/* a TRANSFORMED device buffer of total_blocks, any alignment -> every region's device image */
int32_t dxtlt_untransform_decode_bc6h_images_device(const void *d_transformed, uint64_t total_blocks,
                                                    const DxtltImageRegion *regions, size_t region_count, void *hip_stream);
/* a device block array of total_blocks in block order, any alignment -> the same */
int32_t dxtlt_decode_bc6h_images_device(const void *d_blocks, uint64_t total_blocks, const DxtltImageRegion *regions,
                                        size_t region_count, void *hip_stream);
/* host pointers: one upload of the whole transformed buffer of len bytes, the same kernels into staging (every region's
 * base a multiple of 16, its rows a multiple of 16 bytes apart), one strided download per region */
int32_t dxtlt_untransform_decode_bc6h_images(const uint8_t *transformed, size_t len, const DxtltImageRegion *regions,
                                             size_t region_count);

/* Test hook, no device needed: the launches dxtlt_untransform_decode_bc6h_images_device would enqueue, in order -- the
 * arithmetic of dxtlt_debug_plan_bc7_images (dxtlt_bc7_image.h) with the 8-byte pixel's checks.  Addresses are numbers; nothing
 * is dereferenced but `regions`, and a NULL buffer is not an error here.  Records beyond `cap` are counted, not written.  Returns
 * the number of launches (0 for a list without a non-empty region), or -1 for a list the call would refuse. */
typedef struct DxtltBc6hImagesLaunch {
    uint32_t first_region;   /* index in the list of the group's first non-empty region */
    uint32_t region_count;   /* non-empty regions of the group */
    uint64_t first_granule;  /* the launch's first 1024-block granule; the tail part counts as granule main_blocks / 1024 */
    uint64_t granule_count;  /* its workgroups: granules of the main part, 1 for the tail launch */
    uint32_t tail;           /* 1: the tail part's launch */
    uint32_t reserved;       /* 0 */
} DxtltBc6hImagesLaunch;

int32_t dxtlt_debug_plan_bc6h_images(uint64_t total_blocks, const DxtltImageRegion *regions, size_t region_count,
                                     DxtltBc6hImagesLaunch *out, size_t cap);

/* ---- many buffers in one call ------------------------------------------------------------------------------ */
typedef struct DxtltBc6hImageBatchItem {
    const void *d_transformed;        /* byte 0 of the item's WHOLE device buffer made by dxtlt_transform_bc6h, any alignment */
    uint64_t total_blocks;
    const DxtltImageRegion *regions;  /* host array; pixels = device pointers; the rules of the *_bc6h_images calls */
    uint32_t region_count;
    uint32_t reserved;                /* 0 */
} DxtltBc6hImageBatchItem;

int32_t dxtlt_untransform_decode_bc6h_images_batch_device(const DxtltBc6hImageBatchItem *items, size_t count, void *hip_stream);

/* Test hook, no device needed: the entries the batch call would stage, in list order -- the records of
 * dxtlt_debug_plan_bc7_image_batch (dxtlt_bc7_image.h), field for field.  Addresses are numbers; nothing is dereferenced but
 * `items` and their `regions`.  Records beyond `cap` are counted, not written.  Returns the number of entries, or -1 for a
 * batch the call would refuse. */
typedef struct DxtltDebugBc6hImageBatchEntry {
    uint32_t item;           /* index of the entry's item */
    uint32_t first_region;   /* index in the item's list of the group's first non-empty region */
    uint32_t region_count;   /* non-empty regions of the group */
    int32_t tail_index;      /* the entry's workgroup in the tail launch, or -1 */
    uint64_t first_granule;  /* of the buffer's main part (0 when granule_count is 0) */
    uint32_t granule_count;  /* the entry's workgroups in the granule launch, 0 if none */
    uint32_t first_wg;       /* its first workgroup there: the workgroups of all entries before it */
    uint32_t granule_wgs;    /* workgroups of the whole granule launch (0: not launched) */
    uint32_t tail_wgs;       /* workgroups of the whole tail launch (0: not launched) */
} DxtltDebugBc6hImageBatchEntry;

int32_t dxtlt_debug_plan_bc6h_image_batch(const DxtltBc6hImageBatchItem *items, size_t count, DxtltDebugBc6hImageBatchEntry *out,
                                          size_t cap);

#ifdef __cplusplus
}
#endif
#endif
