/*
 * dxtlt_auto_normalize.h -- transform_bcN_auto_with_normalization on the device, BC1 and BC2: which colour normalisation mode
 * and which transform settings make the colour section compress best, chosen by the built-in size estimator
 * (dxtlt_estimator.h, docs/ESTIMATOR.md) without a section leaving the device.
 *
 * Definition (docs/ESTIMATOR.md, "Auto transform with block normalisation").  With est = the built-in estimator:
 *
 *   BC1   the reference's experimental::normalize_blocks::transform_bc1_auto_with_normalization (transform.rs:222).
 *         any = some block is fully transparent or a normalisable solid colour.  any == 0: the call IS
 *         dxtlt_transform_bc1_auto_device and the colour mode reported is None.  Otherwise, for norm in (None, Color0Only,
 *         ReplicateColor), for (variant, split) in BC1's test order (fast: 4, all modes: 8 entries), est sees the first len / 2
 *         bytes of transform(normalized[norm], variant, split), where normalized[None] still has its transparent blocks rewritten
 *         to 0xFF.  Strict `<` against a best that starts at (None, Variant1, split) with the maximum size.  The output is
 *         dxtlt_transform_bc1_with_normalize_blocks(input, winner): a None winner is written without the transparent rewrite.
 *   BC2   this build's own extension, the same shape.  any = some block whose colour half is a normalisable solid.  any == 0:
 *         dxtlt_transform_bc2_auto_device, mode None.  Otherwise the same loops over BC2's test order; est sees the colour
 *         section, bytes [len / 2, 3 * len / 4), of transform_bc2(normalize_bc2_blocks(input, norm), variant, split);
 *         normalized[None] is the input itself.  The output is dxtlt_transform_bc2_with_normalize_blocks(input, winner).
 *
 * Candidate numbering: candidate index = norm * order_len + position in the test order (order_len 4 or 8): 12 or 24 candidates.
 * Section numbering (what one candidate kernel writes from one read of the input, dxtlt_debug_auto_normalization_sections):
 * section index = norm * (2 * variants) + 2 * variant + split, variants = 2 (None, Variant1) or 4; every candidate is one section.
 *
 * Cost: a read-only classification pass and a wait for its flag (wait 1); then one candidate kernel into a per-thread arena of
 * 6 x len (BC1, fast search), 12 x len (BC1, all modes), 3 x len or 6 x len (BC2), the estimator over its 12 / 24 sections and
 * one readback of 12 / 24 counters (wait 2); then the winner's fused normalise + transform launch, which is NOT waited for.
 * The arena is grow-only and freed by dxtlt_release_thread_resources().
 */
#ifndef DXTLT_AUTO_NORMALIZE_H
#define DXTLT_AUTO_NORMALIZE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#include "dlt_size_estimator.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- device pointers, the built-in estimator; everything on `hip_stream` (a hipStream_t; NULL = default stream) ----
 * len % 8 (BC1) / len % 16 (BC2) != 0: DXTLT_E_INVALID_LENGTH.  A NULL buffer with len > 0: DXTLT_E_INVALID_ARGUMENT.  len == 0:
 * as dxtlt_transform_bcN_auto_device, colour mode None.  A capturing stream, or one whose capture state cannot be queried:
 * DXTLT_E_INVALID_ARGUMENT, nothing enqueued (the call waits twice).  d_input off a 16-byte boundary, dxtlt_debug_auto_use_arena(0)
 * or a failed arena allocation: one fused normalise + transform per candidate into d_output, each estimated there in stream
 * order -- the same choice and bytes, nothing downloaded.  The out-parameters may be NULL; they are written on DXTLT_OK only. */
int32_t dxtlt_transform_bc1_auto_with_normalization_device(const void *d_input, void *d_output, size_t len,
                                                           bool use_all_decorrelation_modes, void *hip_stream,
                                                           uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                           bool *out_split_colour_endpoints);
int32_t dxtlt_transform_bc2_auto_with_normalization_device(const void *d_input, void *d_output, size_t len,
                                                           bool use_all_decorrelation_modes, void *hip_stream,
                                                           uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                           bool *out_split_colour_endpoints);

/* ---- host pointers ----
 * BC2's twin of dxtlt_transform_bc1_auto_with_normalization (dxtlt_bc1_normalize.h).  Both recognise
 * dxtlt_builtin_size_estimator() by the identity of its two function pointers: one upload, the device flow above, one download of
 * `len` bytes, no callback.  With any other estimator: max_compressed_size(len / 2 [BC1], len / 4 [BC2]) once, the classification,
 * then one fused launch per candidate whose colour section is downloaded and shown to the estimator; a failing estimate skips its
 * candidate; DXTLT_E_ESTIMATOR only when max_compressed_size fails (or from the plain auto path). */
int32_t dxtlt_transform_bc2_auto_with_normalization(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len,
                                                    const DltSizeEstimator *estimator, bool use_all_decorrelation_modes,
                                                    uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                    bool *out_split_colour_endpoints, uint32_t *out_estimator_error);

/* ---- test hooks ---- */
/* The arena layout for `blocks` blocks of format 1 or 2: offsets and lengths of the 12 / 24 sections, end to end, 48 / 96 bytes
 * per block in all.  Returns the section count, -1 for another format.  Needs no device. */
int32_t dxtlt_debug_auto_normalization_sections(int32_t format, bool use_all_decorrelation_modes, uint64_t blocks,
                                                uint64_t out_off[24], uint64_t out_len[24]);
/* The pick every route runs after its readback.  sizes[n]: the estimates in SECTION order, n == 12 or 24 as the depth says (else
 * DXTLT_E_INVALID_ARGUMENT).  out_totals (optional, `cap` entries): the same sizes in CANDIDATE order.  Strict `<` in candidate
 * order against (None, Variant1, split) with UINT64_MAX.  Needs no device. */
int32_t dxtlt_debug_auto_normalization_pick(int32_t format, bool use_all_decorrelation_modes, const uint64_t *sizes, int32_t n,
                                            uint64_t *out_totals, int32_t cap, uint8_t *out_color_mode,
                                            uint8_t *out_decorrelation_mode, bool *out_split_colour_endpoints);
/* The candidate kernel alone, into caller memory: format 1 or 2, a whole number of blocks, d_input and d_arena on 16-byte
 * boundaries, arena_bytes at least the layout's size; anything else: DXTLT_E_INVALID_ARGUMENT.  len == 0: nothing to do. */
int32_t dxtlt_debug_auto_normalization_candidates_into_device(int32_t format, bool use_all_decorrelation_modes,
                                                              const void *d_input, size_t len, void *d_arena,
                                                              uint64_t arena_bytes, void *hip_stream);
/* Of this thread's last call above (device or host, built-in estimator): out[0] waits for the stream inside the device flow,
 * out[1] candidate-kernel launches (fallback route: fused transforms of candidates), out[2] estimator launches, out[3] the flag.
 * With the flag 0 the plain auto path does the rest: out = {2, 0, 0, 0}. */
void dxtlt_debug_auto_normalization_last(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
