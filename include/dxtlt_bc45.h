/*
 * dxtlt_bc45.h -- BC4 and BC5 block transforms of libdxtlt_gfx950.so (additive: upstream reserves TransformFormat::Bc4 = 8 and
 * Bc5 = 9 and a settings struct with one field, split_endpoints, but defines no transform for them).  The layout is this
 * build's own, written down in docs/BC45_FORMAT.md:
 *
 *   BC4  8-byte blocks  a0 a1 i0..i5                         split_endpoints = false: (a0 a1) x N, indices 6 x N
 *                                                            split_endpoints = true:  a0 x N, a1 x N, indices 6 x N
 *   BC5  16-byte blocks a red BC4 block, then a green one    the BC4 layout of the red halves at byte 0, of the green halves
 *                                                            at byte 8 N (N = blocks)
 *
 * BC4S / BC5S (DXGI 81 / 84) are the same bytes and take the same transform.  Output length == input length; index bytes are
 * copied verbatim.  `len` must be a multiple of 8 (BC4) or 16 (BC5); any pointer alignment; any block count including 0; input
 * and output must not overlap.  Status codes are the DXTLT_* codes of dxtlt_gfx950.h.
 *
 * The generic entry points of dxtlt_gfx950.h take the formats as codes 4 (BC4) and 5 (BC5): dxtlt_transform_range_device,
 * dxtlt_transform_sharded, DxtltBatchItem.format (device and host batches), dxtlt_debug_plan_transform and
 * dxtlt_debug_plan_batch.  Their split_alpha_endpoints argument carries split_endpoints; the decorrelation mode and the colour
 * split are ignored for these codes.
 */
#ifndef DXTLT_BC45_H
#define DXTLT_BC45_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "dlt_size_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- host pointers: H2D + kernel + D2H on the current device, staged like the BC1-3 host calls -------------------------- */
int32_t dxtlt_transform_bc4_with_settings(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, bool split_endpoints);
int32_t dxtlt_untransform_bc4_with_settings(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, bool split_endpoints);
int32_t dxtlt_transform_bc5_with_settings(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, bool split_endpoints);
int32_t dxtlt_untransform_bc5_with_settings(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, bool split_endpoints);

/* ---- device pointers, asynchronous on `hip_stream` (a hipStream_t; NULL = default): enqueue only, no scratch, capturable -- */
int32_t dxtlt_transform_bc4_with_settings_device(const void *d_input, void *d_output, size_t len, bool split_endpoints,
                                                 void *hip_stream);
int32_t dxtlt_untransform_bc4_with_settings_device(const void *d_input, void *d_output, size_t len, bool split_endpoints,
                                                   void *hip_stream);
int32_t dxtlt_transform_bc5_with_settings_device(const void *d_input, void *d_output, size_t len, bool split_endpoints,
                                                 void *hip_stream);
int32_t dxtlt_untransform_bc5_with_settings_device(const void *d_input, void *d_output, size_t len, bool split_endpoints,
                                                   void *hip_stream);

/* ---- host pointers: the auto transform ------------------------------------------------------------------------------------
 * Candidates split_endpoints = false, then true; strict `<` against the running best (the first best wins).  The estimator sees
 * the endpoint section(s) only: BC4 [0, 2N); BC5 [0, 2N) and [8N, 10N), estimated one after the other (red, then green) and
 * added; a failed estimate ends the call (DXTLT_E_ESTIMATOR; dxtlt_last_error() says so).  One
 * max_compressed_size query up front, for a 2N-byte section.  dxtlt_set_auto_estimator_threads applies as for BC1-3.  On
 * DXTLT_OK output_ptr holds the data transformed with *out_split_endpoints (may be NULL). */
int32_t dxtlt_transform_bc4_auto(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, const DltSizeEstimator *estimator,
                                 bool *out_split_endpoints);
int32_t dxtlt_transform_bc5_auto(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, const DltSizeEstimator *estimator,
                                 bool *out_split_endpoints);

#ifdef __cplusplus
}
#endif
#endif
