/*
 * dxtlt_entropy_estimator.h -- the entropy estimator of libdxtlt_gfx950.so: a second built-in, device-resident size estimator
 * beside the gram estimator of dxtlt_estimator.h (additive; that one is unchanged).
 *
 * Written down in byte terms in docs/ESTIMATOR.md, "The entropy estimator, version 1": a section of L bytes is cut into windows
 * of 32768 bytes counted from its first byte (the last may be shorter); a window of n bytes with byte counts c[0..255] costs
 * q = max(0, n T[n] - sum c[v] T[c[v]]) in 1/65536 bit, T[k] = floor(2^16 log2 k), T[0] = 0; the estimate is
 * (sum of q over the windows + 2^19 - 1) >> 19 bytes.  An exact integer that no schedule can change.  It is what the pixel auto
 * transform (dxtlt_pixels.h) ranks its candidates with: on planes, deltas and interleaved pixels an order-0 cost follows what
 * zlib and zstd do with them, where 4-byte grams rank them the wrong way round (docs/PIXEL_FORMAT.md).  Device only, like the gram
 * estimator: without a device the calls that need one return DXTLT_E_NO_DEVICE.
 *
 * Pointer, stream and status conventions are those of dxtlt_gfx950.h.
 */
#ifndef DXTLT_ENTROPY_ESTIMATOR_H
#define DXTLT_ENTROPY_ESTIMATOR_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "dlt_size_estimator.h"
#include "dxtlt_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the definition in docs/ESTIMATOR.md.  A change of the definition changes the number. */
uint32_t dxtlt_entropy_estimator_version(void);

/* d_out[i] = entropy estimate of sections[i] for i < count (NULL or empty sections: 0); `sections` is host memory (read before the
 * call returns), d_out device memory of count * 8 bytes, 8-byte aligned.  Enqueues on `hip_stream` only -- a clear of d_out, one
 * launch per 16 sections and one finishing launch -- and does not synchronise: capturable.  Sections may overlap one another;
 * none may overlap d_out. */
int32_t dxtlt_estimate_entropy_sizes_device(const DxtltEstimateSection *sections, size_t count, void *hip_stream, uint64_t *d_out);

/* Test and bench hooks: the same estimates through the table-driven launch the batched pixel auto transform uses
 * (dxtlt_transform_pixels_batch_auto_device, dxtlt_pixels.h; docs/ESTIMATOR.md, "The table launch").  table_device: the section
 * table of all `count` sections is built on the host, staged in one of the calling thread's four table slots and uploaded on
 * `hip_stream`; then a clear of d_out, ONE estimator launch for any count, and one finishing launch.  d_out[i] equals what
 * dxtlt_estimate_entropy_sizes_device writes.  table_counters_device: section i adds into d_out[counters[i]] (counters NULL: i),
 * d_out holding counter_count numbers -- sections that share a counter are rounded up to bytes as ONE sum of q.  Both enqueue only,
 * but are not capturable (the slot is rewritten by later calls): DXTLT_E_INVALID_ARGUMENT on a capturing stream, for a counter
 * out of range, or for more than 2^31 - 1 windows in all. */
int32_t dxtlt_debug_estimate_entropy_table_device(const DxtltEstimateSection *sections, size_t count, void *hip_stream, uint64_t *d_out);
int32_t dxtlt_debug_estimate_entropy_table_counters_device(const DxtltEstimateSection *sections, const uint32_t *counters, size_t count,
                                                           size_t counter_count, void *hip_stream, uint64_t *d_out);

/* One section of device memory; waits for `hip_stream` and returns the number in *out. */
int32_t dxtlt_estimate_entropy_size_device(const void *d_ptr, size_t len, void *hip_stream, uint64_t *out);

/* One section of HOST memory: uploaded into a per-thread device buffer and stream of this call's own (those of
 * dxtlt_estimate_size: grow-only, freed by dxtlt_release_thread_resources; not the staging of the host-pointer transforms, so
 * it may be called from an estimator callback inside an auto transform of the same thread) and estimated on the current device. */
int32_t dxtlt_estimate_entropy_size(const uint8_t *host_ptr, size_t len, uint64_t *out);

/* The estimator as a DltSizeEstimator, valid for the life of the process: MaxCompressedSize reports 0, EstimateCompressedSize is
 * dxtlt_estimate_entropy_size (its return value is the DXTLT_* status), Context is NULL.  dxtlt_transform_pixels_auto recognises
 * this pointer and then never calls it: everything stays on the device. */
const DltSizeEstimator *dxtlt_builtin_entropy_estimator(void);

/* Test hook, on the host, no device needed: T[k] as the kernels read it; 0 for k > 32768. */
uint32_t dxtlt_debug_entropy_table(uint32_t k);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_ENTROPY_ESTIMATOR_H */
