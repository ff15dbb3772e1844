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
 * The RGBA image calls of dxtlt_image.h, their region and batch calls and the BC7 calls of dxtlt_bc7_image.h do not take BC6H.
 */
#ifndef DXTLT_BC6H_IMAGE_H
#define DXTLT_BC6H_IMAGE_H

#include <stddef.h>
#include <stdint.h>

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

#ifdef __cplusplus
}
#endif
#endif
