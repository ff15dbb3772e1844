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

#ifdef __cplusplus
}
#endif
#endif
