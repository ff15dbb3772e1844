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

#include "dlt_size_estimator.h"

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

/* ---- the auto transform: the best of the six settings, chosen on the device ---------------------------------------------------
 * Candidates, in this order: (decorrelate, PLANAR_DELTA), (decorrelate, PLANAR), (decorrelate, INTERLEAVED), (plain, PLANAR_DELTA),
 * (plain, PLANAR), (plain, INTERLEAVED).  The estimator is shown each candidate's whole output, len bytes, as ONE section; the
 * choice starts at the first candidate with best = UINT64_MAX and moves on strict `<`, so ties and empty buffers keep
 * (decorrelate, PLANAR_DELTA).  The choice is reported in out_* (each may be NULL) and output holds the data transformed with it.
 * Argument checks as the single calls above, before any device work.
 *
 * Device pointers: the entropy estimator (dxtlt_entropy_estimator.h), nothing but six counters leaves the device.  The contract of
 * dxtlt_transform_bc4_auto_device: any alignment; the call WAITS for `hip_stream` once, for the counters, and is NOT capturable --
 * on a capturing stream, or one whose capture state cannot be queried, it returns DXTLT_E_INVALID_ARGUMENT with nothing enqueued;
 * the winner's transform reads d_input only and is enqueued, not waited for.  A d_input on a 16-byte boundary is read once for all
 * candidates, into this thread's candidate arena (5 x len, grow-only, freed by dxtlt_release_thread_resources); off one -- or when
 * the arena cannot be allocated -- every candidate is one full transform into d_output, estimated there in stream order: the same
 * totals, choice and bytes.
 *
 * Host pointers: with dxtlt_builtin_entropy_estimator(), recognised by pointer identity and never called, one upload, the device
 * call, one download.  With any other estimator MaxCompressedSize is asked once for len, then per candidate, in order, its output
 * is downloaded and EstimateCompressedSize called on it (the last candidate is the input itself); a callback's failure is
 * DXTLT_E_ESTIMATOR.  A NULL estimator is DXTLT_E_INVALID_ARGUMENT. */
int32_t dxtlt_transform_pixels_auto_device(const void *d_input, void *d_output, size_t len, int32_t pixel_bytes, void *hip_stream,
                                           bool *out_decorrelate, uint8_t *out_layout);
int32_t dxtlt_transform_pixels_auto(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, int32_t pixel_bytes,
                                    const DltSizeEstimator *estimator, bool *out_decorrelate, uint8_t *out_layout);

/* Test hook: the six totals the last entropy-estimator pixel auto call of this thread compared, in candidate order; returns how
 * many there were (0 after a callback-route call, an empty buffer or a failed call); writes at most cap. */
int32_t dxtlt_debug_pixels_auto_last_totals(uint64_t *out, int32_t cap);

/* Bench hooks, per calling thread.  time_phases: anything but 0 = the entropy-estimator pixel auto calls record HIP events around
 * their phases and wait for the winner's transform before they return; last_phase_ms then reports the milliseconds of the last
 * such call: out[0] the candidate kernel, out[1] the estimator launch, out[2] the readback and the winner's transform (on the
 * route of one transform per candidate, where candidates and estimates alternate, out[0] is both and out[1] is 0).
 * candidates_device: the fused candidate kernel alone, from `len` bytes at d_input (on a 16-byte boundary, else
 * DXTLT_E_INVALID_ARGUMENT) into the calling thread's arena, enqueued on `hip_stream`. */
void dxtlt_debug_pixels_auto_time_phases(int32_t on);
void dxtlt_debug_pixels_auto_last_phase_ms(double out[3]);
int32_t dxtlt_debug_pixels_auto_candidates_device(const void *d_input, size_t len, int32_t pixel_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_PIXELS_H */
