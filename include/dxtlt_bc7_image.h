/*
 * dxtlt_bc7_image.h -- C ABI of the BC7 decoders of libdxtlt_gfx950.so: BC7 blocks -> RGBA8888 pixels
 * (docs/IMAGE_DECODE.md, "BC7").
 *
 * The decoder is Direct3D 11's: every mode 0..7 with its partitions, p-bits, rotation and index selector; the reserved
 * encoding (byte 0 == 0) decodes to sixteen pixels of four zero bytes.  A pixel is the bytes r, g, b, a.
 *
 *   dxtlt_decode_bc7_blocks*          `len / 16` blocks -> that many 64-byte Decoded4x4Block records (dxtlt_decode.h): sixteen
 *                                     pixels in row-major order.  The host-pointer call decodes on the CPU with the code the
 *                                     kernels use and needs no device.
 *   dxtlt_decode_bc7_image_device     ceil(width / 4) * ceil(height / 4) blocks in block order -> a row-major image: pixel
 *                                     (x, y) at pixels + y * pitch + 4 * x.  Nothing else of the image's memory is written.
 *   dxtlt_untransform_decode_bc7_image*
 *                                     the same from the blocks [first_block, first_block + image blocks) of a buffer
 *                                     TRANSFORMED by dxtlt_transform_bc7 (dxtlt_bc7.h), of `total_blocks` (`len / 16`)
 *                                     blocks in all, in one pass: the untransformed blocks never touch memory.
 *                                     `first_block` may be any block.  At most two launches; nothing is allocated or copied
 *                                     by the device call, there is no synchronisation, and it can be captured into a graph.
 *
 * Checks, in this order, all before a device is touched (status codes and dxtlt_last_error() as in dxtlt_gfx950.h):
 *   1. width == 0 or height == 0: DXTLT_OK, nothing is done;
 *   2. a NULL pointer: DXTLT_E_INVALID_ARGUMENT (2);
 *   3. pitch < 4 * width: 2;
 *   4. pitch or the pixel pointer not a multiple of 4: 2;
 *   5. first_block + image blocks > total_blocks (wrap-safe): 2;
 *   6. host call only: len not a multiple of 16: DXTLT_E_INVALID_LENGTH (1).
 * The block calls: len not a multiple of 16: 1; a NULL pointer with len > 0, or pixels_len < 64 * blocks: 2.
 *
 * The RGBA image calls of dxtlt_image.h (format 1..3) and its region and batch calls do not take BC7.
 */
#ifndef DXTLT_BC7_IMAGE_H
#define DXTLT_BC7_IMAGE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host pointers ---------------------------------------------------------------------------------- */
int32_t dxtlt_decode_bc7_blocks(const uint8_t *blocks, size_t len, uint8_t *pixels, size_t pixels_len);
int32_t dxtlt_untransform_decode_bc7_image(const uint8_t *transformed, size_t len, uint64_t first_block, uint32_t width,
                                           uint32_t height, uint8_t *pixels, uint64_t pitch);

/* ---- device pointers, asynchronous on `hip_stream` --------------------------------------------------- */
int32_t dxtlt_decode_bc7_blocks_device(const void *d_blocks, size_t len, void *d_pixels, size_t pixels_len, void *hip_stream);
int32_t dxtlt_decode_bc7_image_device(const void *d_blocks, uint32_t width, uint32_t height, void *d_pixels, uint64_t pitch,
                                      void *hip_stream);
int32_t dxtlt_untransform_decode_bc7_image_device(const void *d_transformed, uint64_t total_blocks, uint64_t first_block,
                                                  uint32_t width, uint32_t height, void *d_pixels, uint64_t pitch,
                                                  void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
