/*
 * dxtlt_auto_normalize.h -- transform_bcN_auto_with_normalization on the device, BC1, BC2 and BC3: which normalisation mode(s)
 * and which transform settings make the endpoint section(s) compress best, chosen by the built-in size estimator
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
 *   BC3   this build's own extension, BC2's shape with an alpha part (N = blocks).  any = some block whose alpha half is uniform
 *         (all sixteen decoded alpha values equal) or whose colour half is a normalisable solid; a block already in normal form
 *         counts.  any == 0: the call IS dxtlt_transform_bc3_auto_device, both modes None, its 8 / 16 totals.  Otherwise
 *         alpha_mode over 0..3, inside it colour_mode over 0..2, inside it (variant, split_alpha, split_colour) over BC3's test
 *         order (fast: 8, all modes: 16 entries): candidate index = (alpha_mode * 3 + colour_mode) * order_len + position, 96 or
 *         192 candidates.  A candidate's total is est(T[0, 2N)) + est(T[len / 2, len / 2 + 4N)), the `+` wrapping as the plain BC3
 *         call's does, with T = transform_bc3(normalize_bc3_blocks(input, alpha_mode, colour_mode), variant, split_alpha,
 *         split_colour); mode None leaves that half's bytes alone.  Strict `<` in candidate order against a best that starts at
 *         (None, None, Variant1, split alpha, split colour) with UINT64_MAX.  The output is
 *         dxtlt_transform_bc3_with_normalize_blocks(input, winner).
 *         The halves of a block are normalised independently, so the alpha endpoint section depends on (alpha_mode, split_alpha)
 *         alone and the colour endpoint section on (colour_mode, variant, split_colour) alone: the 96 / 192 totals are sums over
 *         20 / 32 distinct sections, and those are all that is ever produced and estimated.
 *
 * Candidate numbering: candidate index = norm * order_len + position in the test order (order_len 4 or 8): 12 or 24 candidates.
 * Section numbering (what one candidate kernel writes from one read of the input, dxtlt_debug_auto_normalization_sections):
 * section index = norm * (2 * variants) + 2 * variant + split, variants = 2 (None, Variant1) or 4; every candidate is one section.
 * BC3 (dxtlt_debug_bc3_auto_normalization_sections): 8 alpha sections of 2N bytes, [alpha pairs 2N][alpha split: first endpoints N,
 * second endpoints N] per alpha mode, section index = 2 * alpha_mode + split_alpha; behind them, from 16N on, BC2's arena byte for
 * byte, section index = 8 + colour_mode * (2 * variants) + 2 * variant + split_colour.  A section's index is its estimate counter.
 *
 * Cost: a read-only classification pass and a wait for its flag (wait 1); then one candidate kernel into a per-thread arena of
 * 6 x len (BC1, fast search), 12 x len (BC1, all modes), 3 x len or 6 x len (BC2), 4 x len or 7 x len (BC3: 64 / 112 bytes per
 * block), the estimator over its 12 / 24 (BC3: 20 / 32) sections in two launches and one readback of as many counters (wait 2);
 * then the pick on the host (BC3: the literal 96 / 192-entry walk over sums) and the winner's fused normalise + transform launch,
 * which is NOT waited for.  The arena is grow-only and freed by dxtlt_release_thread_resources().
 * Speed (BC3; profiles/auto_normalize_bc3_bench.json, one MI355X, 10 % normalisable alpha halves and 10 % normalisable colour
 * halves, 20 % of blocks, fast / all modes): 2 GiB 13.5 / 22.9 ms
 * against 18.7 / 34.0 ms for the 12 / 24 fused launches with an estimate per shown section; the estimator is 75 % / 78 % of the call.
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
 * len % 8 (BC1) / len % 16 (BC2, BC3) != 0: DXTLT_E_INVALID_LENGTH.  A NULL buffer with len > 0: DXTLT_E_INVALID_ARGUMENT.  len == 0:
 * as dxtlt_transform_bcN_auto_device, colour mode None.  A capturing stream, or one whose capture state cannot be queried:
 * DXTLT_E_INVALID_ARGUMENT, nothing enqueued (the call waits twice).  d_input off a 16-byte boundary, dxtlt_debug_auto_use_arena(0)
 * or a failed arena allocation: one fused normalise + transform per candidate into d_output, each estimated there in stream
 * order -- the same choice and bytes, nothing downloaded.  BC3 makes 12 / 24 such launches, one per colour section k: the first
 * eight carry alpha section k as well (alpha_mode = k / 2, split_alpha = k % 2), the others alpha mode None, unsplit; each launch's
 * colour section, and for k < 8 its alpha section, is estimated in place into its own counter: 20 / 32 estimator launches.
 * The out-parameters may be NULL; they are written on DXTLT_OK only. */
int32_t dxtlt_transform_bc1_auto_with_normalization_device(const void *d_input, void *d_output, size_t len,
                                                           bool use_all_decorrelation_modes, void *hip_stream,
                                                           uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                           bool *out_split_colour_endpoints);
int32_t dxtlt_transform_bc2_auto_with_normalization_device(const void *d_input, void *d_output, size_t len,
                                                           bool use_all_decorrelation_modes, void *hip_stream,
                                                           uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                           bool *out_split_colour_endpoints);

int32_t dxtlt_transform_bc3_auto_with_normalization_device(const void *d_input, void *d_output, size_t len,
                                                           bool use_all_decorrelation_modes, void *hip_stream,
                                                           uint8_t *out_alpha_mode, uint8_t *out_color_mode,
                                                           uint8_t *out_decorrelation_mode, bool *out_split_alpha_endpoints,
                                                           bool *out_split_colour_endpoints);

/* ---- host pointers ----
 * BC2's twin of dxtlt_transform_bc1_auto_with_normalization (dxtlt_bc1_normalize.h).  Both recognise
 * dxtlt_builtin_size_estimator() by the identity of its two function pointers: one upload, the device flow above, one download of
 * `len` bytes, no callback.  With any other estimator: max_compressed_size(len / 2 [BC1], len / 4 [BC2]) once, the classification,
 * then one fused launch per candidate whose colour section is downloaded and shown to the estimator; a failing estimate skips its
 * candidate; DXTLT_E_ESTIMATOR only when max_compressed_size fails (or from the plain auto path).
 * BC3 with any other estimator: max_compressed_size(len / 8), then max_compressed_size(len / 4), each once up front (either
 * failing: DXTLT_E_ESTIMATOR, nothing written); the classification; the 12 / 24 fused launches above on the resident copy, of which
 * only the 20 / 32 shown sections are downloaded; each is estimated once (a launch's alpha section before its colour section); a
 * failing estimate skips every candidate that uses its section. */
int32_t dxtlt_transform_bc2_auto_with_normalization(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len,
                                                    const DltSizeEstimator *estimator, bool use_all_decorrelation_modes,
                                                    uint8_t *out_color_mode, uint8_t *out_decorrelation_mode,
                                                    bool *out_split_colour_endpoints, uint32_t *out_estimator_error);

int32_t dxtlt_transform_bc3_auto_with_normalization(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len,
                                                    const DltSizeEstimator *estimator, bool use_all_decorrelation_modes,
                                                    uint8_t *out_alpha_mode, uint8_t *out_color_mode,
                                                    uint8_t *out_decorrelation_mode, bool *out_split_alpha_endpoints,
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
/* BC3's twins of the three hooks above (which keep refusing format 3).  Sections: the 20 / 32 offsets and lengths, 64 / 112 bytes
 * per block in all; returns the section count.  Pick: sizes[n] in SECTION order, n == 20 or 32 as the depth says (else
 * DXTLT_E_INVALID_ARGUMENT); out_totals (optional, `cap` entries): the 96 / 192 sums in CANDIDATE order.  Candidates: d_input and
 * d_arena on 16-byte boundaries, a whole number of blocks, arena_bytes at least the layout's size. */
int32_t dxtlt_debug_bc3_auto_normalization_sections(bool use_all_decorrelation_modes, uint64_t blocks, uint64_t out_off[32],
                                                    uint64_t out_len[32]);
int32_t dxtlt_debug_bc3_auto_normalization_pick(bool use_all_decorrelation_modes, const uint64_t *sizes, int32_t n,
                                                uint64_t *out_totals, int32_t cap, uint8_t *out_alpha_mode, uint8_t *out_color_mode,
                                                uint8_t *out_decorrelation_mode, bool *out_split_alpha_endpoints,
                                                bool *out_split_colour_endpoints);
int32_t dxtlt_debug_bc3_auto_normalization_candidates_into_device(bool use_all_decorrelation_modes, const void *d_input, size_t len,
                                                                  void *d_arena, uint64_t arena_bytes, void *hip_stream);
/* Of this thread's last call above (device or host, built-in estimator): out[0] waits for the stream inside the device flow,
 * out[1] candidate-kernel launches (fallback route: fused transforms), out[2] estimator launches, out[3] the flag.  All formats.
 * With the flag 0 the plain auto path does the rest: out = {2, 0, 0, 0}. */
void dxtlt_debug_auto_normalization_last(uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif
