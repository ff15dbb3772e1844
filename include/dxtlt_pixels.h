/*
 * dxtlt_pixels.h -- uncompressed pixel transform (RGBA8888, BGRA8888, BGR888), layout version 1: C ABI (libdxtlt_gfx950.so).
 *
 * A FORMAT DEFINED BY THIS BUILD (docs/PIXEL_FORMAT.md).  Upstream parses these DDS payloads and reserves
 * TransformFormat::Rgba8888 = 5, Bgra8888 = 6 and Bgr888 = 7 with a placeholder settings struct of one flag, `decorrelation`
 * (embed/formats/rgba8888.rs, bgra8888.rs, bgr888.rs), but has no transform behind them.
 *
 * A buffer holds P = len / pixel_bytes pixels of pixel_bytes = 4 (RGBA8888, BGRA8888) or 3 (BGR888) bytes.  Byte 1 of a pixel
 * is G in all three formats, so RGBA and BGRA are the same byte transform.
 *   decorrelate   subtract-green modulo 256: byte0 -= byte1, byte2 -= byte1; byte 3 (alpha) is never changed
 *   layout        DXTLT_PIXEL_LAYOUT_INTERLEAVED   pixels stay in place
 *                 DXTLT_PIXEL_LAYOUT_PLANAR        byte c of pixel i goes to output byte c * P + i
 *                 DXTLT_PIXEL_LAYOUT_PLANAR_DELTA  PLANAR, then every plane in segments of DXTLT_PIXEL_SEGMENT bytes counted from
 *                                                  the plane's first byte: a segment's first byte as it is, every other byte
 *                                                  as p[i] - p[i - 1] modulo 256
 * Decorrelation comes first.  Parity: exact round trip and GPU == tests/pixels_ref.py.
 *
 * Contract: len is a multiple of pixel_bytes (else DXTLT_E_INVALID_LENGTH); pixel_bytes is 3 or 4, layout 0..2, no NULL
 * buffer with len > 0 (else DXTLT_E_INVALID_ARGUMENT); all checked before any device work; len == 0 is a no-op; output
 * length == input length; buffers must not overlap; returns the DXTLT_* status codes of dxtlt_gfx950.h.  Device-pointer
 * calls take any pointer alignment and any P (16-byte aligned buffers with P a multiple of 16 are the fast case); they
 * enqueue one kernel on the stream, use no scratch memory and do not synchronise, so they can be captured into a HIP graph.
 *
 * The generic entry points of dxtlt_gfx950.h know these buffers as format codes 8 (4-byte pixels) and 9 (3-byte pixels):
 * DxtltBatchItem.format of the host batch call (dxtlt_transform_batch_device keeps refusing them), and dxtlt_transform_sharded.  Their settings triple reads
 * decorrelation_mode != 0 as `decorrelate` and the two split flags as the layout: no colour split = INTERLEAVED, colour
 * split alone = PLANAR, colour and alpha split = PLANAR_DELTA (the alpha split alone is ignored).
 */
#ifndef DXTLT_PIXELS_H
#define DXTLT_PIXELS_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXTLT_PIXEL_LAYOUT_INTERLEAVED 0
#define DXTLT_PIXEL_LAYOUT_PLANAR 1
#define DXTLT_PIXEL_LAYOUT_PLANAR_DELTA 2
#define DXTLT_PIXEL_SEGMENT 4096

/* the generic entry points' format codes (dxtlt_gfx950.h) */
#define DXTLT_FORMAT_PIXELS4 8
#define DXTLT_FORMAT_PIXELS3 9

/* Host pointers: mapped staging, the chunked pipeline or one upload + launch + download, by size. */
int32_t dxtlt_transform_pixels(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, int32_t pixel_bytes, bool decorrelate,
                               uint8_t layout);
int32_t dxtlt_untransform_pixels(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, int32_t pixel_bytes, bool decorrelate,
                                 uint8_t layout);

int32_t dxtlt_transform_pixels_device(const void *d_input, void *d_output, size_t len, int32_t pixel_bytes, bool decorrelate,
                                      uint8_t layout, void *hip_stream);
int32_t dxtlt_untransform_pixels_device(const void *d_input, void *d_output, size_t len, int32_t pixel_bytes, bool decorrelate,
                                        uint8_t layout, void *hip_stream);

/* Pixels [first_pixel, first_pixel + num_pixels) of a buffer of total_pixels pixels, as dxtlt_transform_range_device: the
 * interleaved-side pointer is the range's first pixel, the transformed-side pointer byte 0 of the WHOLE transformed buffer;
 * forward reads the former and writes the latter, inverse the other way round.  first_pixel must be a multiple of
 * DXTLT_PIXEL_SEGMENT and the range must lie inside total_pixels (else DXTLT_E_INVALID_ARGUMENT, nothing enqueued). */
int32_t dxtlt_transform_pixels_range_device(int32_t pixel_bytes, bool inverse, const void *d_src, void *d_dst,
                                            uint64_t total_pixels, uint64_t first_pixel, uint64_t num_pixels, bool decorrelate,
                                            uint8_t layout, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_PIXELS_H */
