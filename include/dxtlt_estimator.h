/*
 * dxtlt_estimator.h -- the built-in, device-resident size estimator of libdxtlt_gfx950.so and the auto transforms that keep
 * every byte on the device (additive: upstream's estimators are CPU crates behind the DltSizeEstimator vtable).
 *
 * The estimator is this build's own, written down in byte terms in docs/ESTIMATOR.md (version 1): a section of L bytes is cut
 * into windows of 32768 bytes; inside a window a position is a match when its 4-byte gram equals the gram at the smallest
 * position of the same hash slot; estimate = L - matches.  An exact integer that no schedule can change.  Like upstream's fast
 * estimator (len - estimated LZ matches) only the relative order of its results means anything.  It runs on the device only:
 * there is no CPU implementation in the library, and without a device the calls return DXTLT_E_NO_DEVICE.
 *
 * Pointer, stream and status conventions are those of dxtlt_gfx950.h: any alignment, `hip_stream` is a hipStream_t (NULL = the
 * default stream), 0 = DXTLT_OK, dxtlt_last_error() has the text of a failure.
 */
#ifndef DXTLT_ESTIMATOR_H
#define DXTLT_ESTIMATOR_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "dlt_size_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* 1: the definition in docs/ESTIMATOR.md.  A change of the definition changes the number. */
uint32_t dxtlt_estimator_version(void);

/* One section of device memory: `len` bytes at `d_ptr` (any alignment).  NULL, or fewer than 4 bytes, estimates as `len`. */
typedef struct DxtltEstimateSection {
    const void *d_ptr;
    uint64_t len;
} DxtltEstimateSection;

/* d_out[i] = estimate of sections[i] for i < count; `sections` is host memory (read before the call returns), d_out device memory
 * of count * 8 bytes, 8-byte aligned.  Enqueues on `hip_stream` only -- a clear of d_out and one launch per 16 sections -- and
 * does not synchronise: capturable.  Sections may overlap one another; none may overlap d_out. */
int32_t dxtlt_estimate_sizes_device(const DxtltEstimateSection *sections, size_t count, void *hip_stream, uint64_t *d_out);

/* One section of device memory; waits for `hip_stream` and returns the number in *out. */
int32_t dxtlt_estimate_size_device(const void *d_ptr, size_t len, void *hip_stream, uint64_t *out);

/* One section of HOST memory: uploaded into a per-thread device buffer and stream of this call's own (grow-only, freed by
 * dxtlt_release_thread_resources) -- not the staging of the host-pointer transforms, so it may be called from an estimator
 * callback inside an auto transform of the same thread -- and estimated on the current device.  DXTLT_E_NO_DEVICE without one. */
int32_t dxtlt_estimate_size(const uint8_t *host_ptr, size_t len, uint64_t *out);

/* The estimator as a DltSizeEstimator, valid for the life of the process and for any caller of that vtable (upstream's CPU code
 * included): MaxCompressedSize reports 0 (no scratch buffer is needed), EstimateCompressedSize is dxtlt_estimate_size (its return
 * value is the DXTLT_* status), Context is NULL.
 *
 * The auto transforms of this library (dxtlt_transform_bc{1,2,3,4,5}_auto, and through them the dltbcN auto builders and
 * dxtlt_dds_transform_auto) recognise it by the identity of its two function pointers and then never call it: every distinct
 * section a candidate can show the estimator is estimated where the candidate kernel left it, with one launch; 6 / 10 eight-byte
 * counters come back instead of the sections; candidate order, the additions for BC3 / BC5 and the strict `<` are unchanged. */
const DltSizeEstimator *dxtlt_builtin_size_estimator(void);

/* ---- the auto transforms on device pointers, with the built-in estimator ----------------------------------------------------
 * d_input stays untouched, d_output (len bytes, not overlapping d_input) receives the data transformed with the settings
 * reported in out_* (each may be NULL); same candidates, order and tie-break as the host-pointer auto calls given
 * dxtlt_builtin_size_estimator().  The candidate sections live in a per-thread device arena (2-4 x len, grow-only, freed by
 * dxtlt_release_thread_resources).  The choice is made on the host from one readback of at most 32 counters, so these calls WAIT
 * for `hip_stream` once and are NOT capturable into a HIP graph: on a capturing stream they return DXTLT_E_INVALID_ARGUMENT
 * without enqueueing or synchronising anything (so does a stream whose capture state cannot be queried).  The winning transform
 * reads d_input only and is enqueued, not waited for.
 *
 * d_input and d_output may have any alignment.  BC1 / BC2 / BC3 read a d_input on a 16-byte boundary once for all candidates;
 * a d_input off a 16-byte boundary costs one full transform per candidate (4 / 8, BC3 8 / 16) into d_output, each estimated
 * there in stream order -- the same choice and bytes, and still nothing downloaded.  BC4 / BC5 run both transforms either way. */
int32_t dxtlt_transform_bc1_auto_device(const void *d_input, void *d_output, size_t len, bool use_all_decorrelation_modes,
                                        void *hip_stream, uint8_t *out_decorrelation_mode, bool *out_split_colour_endpoints);
int32_t dxtlt_transform_bc2_auto_device(const void *d_input, void *d_output, size_t len, bool use_all_decorrelation_modes,
                                        void *hip_stream, uint8_t *out_decorrelation_mode, bool *out_split_colour_endpoints);
int32_t dxtlt_transform_bc3_auto_device(const void *d_input, void *d_output, size_t len, bool use_all_decorrelation_modes,
                                        void *hip_stream, uint8_t *out_decorrelation_mode, bool *out_split_alpha_endpoints,
                                        bool *out_split_colour_endpoints);
/* BC4 / BC5 (dxtlt_bc45.h) have two candidates and no decorrelation: use_all_decorrelation_modes is ignored. */
int32_t dxtlt_transform_bc4_auto_device(const void *d_input, void *d_output, size_t len, bool use_all_decorrelation_modes,
                                        void *hip_stream, bool *out_split_endpoints);
int32_t dxtlt_transform_bc5_auto_device(const void *d_input, void *d_output, size_t len, bool use_all_decorrelation_modes,
                                        void *hip_stream, bool *out_split_endpoints);

/* Test hook: what the last auto transform called from this thread (host or device pointers, any format) moved and called for
 * its estimates: bytes of candidate sections copied to the host, and calls made through the estimator's vtable
 * (MaxCompressedSize and EstimateCompressedSize).  Both are 0 with the built-in estimator.  Either pointer may be NULL. */
void dxtlt_debug_auto_last_estimation(uint64_t *out_section_bytes_downloaded, uint64_t *out_estimator_callbacks);

/* Test hook: the totals the last built-in-estimator auto transform of this thread compared, in candidate order;
 * returns how many there were (0 after a callback-route call, an empty buffer or a failed call); writes at most cap. */
int32_t dxtlt_debug_auto_last_totals(uint64_t *out_totals, int32_t cap);

/* Test hook, per calling thread: 0 = the built-in path of the auto transforms behaves as if its candidate arena could not be
 * allocated (one full transform per candidate into the output buffer, estimated there); anything else = normal. */
void dxtlt_debug_auto_use_arena(int32_t on);

/* Test / bench hook, stateless: dxtlt_estimate_sizes_device with `lanes` per workgroup (256, 512 or 1024) and another
 * (window, bits) pair of the definition -- (32768, 14) is the estimator, whose result does not depend on `lanes`; (32768, 13),
 * (16384, 13) and (8192, 12) are compiled for the shape sweep of tools/estimator_bench.py and define other numbers.  Anything
 * else: DXTLT_E_INVALID_ARGUMENT. */
int32_t dxtlt_debug_estimate_sizes_shape(const DxtltEstimateSection *sections, size_t count, void *hip_stream, uint64_t *d_out,
                                         int32_t lanes, uint32_t window, uint32_t bits);

/* Bench hook: the fused candidate kernel of the auto transforms alone -- every candidate section of format 1..3 from the `len`
 * bytes at d_input into the calling thread's arena, enqueued on `hip_stream`.  Unlike the auto transforms it takes the kernel as
 * it is: d_input must be 16-byte aligned (DXTLT_E_DEVICE otherwise). */
int32_t dxtlt_debug_auto_candidates_device(int32_t format, bool use_all_decorrelation_modes, const void *d_input, size_t len,
                                           void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
