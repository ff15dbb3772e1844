/*
 * dxtlt_batch_normalize.h -- C ABI of the batched block-normalisation entry points of libdxtlt_gfx950.so: block normalisation
 * fused into the forward transform for MANY device buffers per call, and the batched "does this buffer hold a block that
 * normalisation would touch" classification.  Additive, like dxtlt_transform_batch_device (dxtlt_gfx950.h): upstream transforms
 * one buffer per call.  Status codes and dxtlt_last_error() as in dxtlt_gfx950.h.
 *
 * A corpus of mip-chained textures through one fused single-buffer call per texture (dxtlt_bc1_normalize.h,
 * dxtlt_bc23_normalize.h) is bound by the ~5 us a launch costs the host; here a batch is a handful of launches.
 */
#ifndef DXTLT_BATCH_NORMALIZE_H
#define DXTLT_BATCH_NORMALIZE_H

#include <stddef.h>
#include <stdint.h>

#include "dxtlt_gfx950.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct DxtltBatchNormalizeItem {
    const void *d_input;
    void *d_output;
    uint64_t len;                   /* a multiple of the block size; 0 allowed */
    uint8_t format;                 /* 1, 2, 3 = BC1, BC2, BC3 */
    uint8_t alpha_mode;             /* BC3: 0..3 (DXTLT_ALPHA_NORMALIZE_*); ignored for BC1 / BC2 */
    uint8_t color_mode;             /* 0..2: None, Color0Only, ReplicateColor */
    uint8_t decorrelation_mode;     /* core numbering, 0..3 */
    uint8_t split_alpha_endpoints;  /* BC3 only */
    uint8_t split_colour_endpoints;
    uint8_t reserved[2];            /* ignored */
} DxtltBatchNormalizeItem;

/* ---- normalise + transform, many buffers in one call ------------------------------------------------------------------
 * For every item, d_output[0, len) receives exactly what the single call
 *     dxtlt_transform_bcN_with_normalize_blocks_device(d_input, d_output, len, modes, settings, hip_stream)
 * writes: transform_bcN_with_settings(normalize_blocks(input, modes), settings), byte for byte.  No byte outside d_output[0, len)
 * is written and no input byte changes.  Forward only (the inverse of the result is dxtlt_transform_batch_device's).  Items must
 * not overlap one another.  Any block counts and pointer alignments.
 *
 * Asynchronous on `hip_stream` and ordered like a single call; the tables of the call's launches are staged in one of the calling
 * thread's four slots and sent in one upload, exactly as dxtlt_transform_batch_device does (the same ring: its rule about more
 * than four calls behind a later event applies).  The whole batch is validated before anything is enqueued; per item, in this
 * order: format outside 1..3 (DXTLT_E_INVALID_ARGUMENT), len no multiple of the block size (DXTLT_E_INVALID_LENGTH), and with
 * DXTLT_E_INVALID_ARGUMENT decorrelation_mode > 3, color_mode > 2, alpha_mode > 3 on a BC3 item, a NULL buffer with len > 0; then
 * an item of 64 GiB or more and a launch of 2^24 - 1 workgroups or more.  count == 0 is DXTLT_OK.
 *
 * Launches, in ascending (format, settings code, plain before normalising, BC1 colour mode):
 *   - items whose modes are all None (BC1 / BC2: color_mode 0; BC3: both 0): dxtlt_transform_batch_device's own launches, one
 *     per (format, settings), with all its shortcuts for regular batches -- its kernels, its bytes;
 *   - BC2 / BC3 items with a mode set: ONE launch per (format, settings) whatever mixture of modes they carry; the modes travel
 *     in every item's table entry and are uniform over a workgroup;
 *   - BC1 items with a mode set: one launch per (settings, colour mode) -- BC1's mode is compiled into its tile code;
 *   - an item whose d_output is off an 8-byte boundary in a way the tile kernels do not take goes out alone, through the
 *     single-buffer fused kernels, behind the batch launches (one launch each, no wait).
 * The normalising launches always read their table (no regular-array shortcut); the division for batches of one size stays.
 *
 * Resources on gfx950 (compiler's resource report; plain batch kernel of the same settings in parentheses; default settings;
 * scratch is 0 in all 40 new kernels and LDS equals the plain kernel's; all 40: profiles/batch_norm_isa.txt):
 *
 *   kernel                              lanes   VGPRs        LDS bytes      waves / SIMD
 *   BC1, colour mode 1 | 2              256     21 (22)      4992 (4992)    8 (8)
 *   BC1 without the colour split        128     21 (21)      2944 (2944)    8 (8)
 *   BC2, modes per entry                256     21 (18)      5504 (5504)    8 (8)
 *   BC3, modes per entry                256     35 (23)      5504 (5504)    8 (8)
 *
 * No new kernel falls below the plain kernel's occupancy (64 VGPRs would still give 8 waves per SIMD); what the kernels add is
 * instructions, as the single-buffer fused kernels do (dxtlt_bc23_normalize.h).  Timings: profiles/normalize_batch_bench.json.
 */
int32_t dxtlt_transform_batch_with_normalize_blocks_device(const DxtltBatchNormalizeItem *items, size_t count, void *hip_stream);

/* ---- which items hold a normalisable block -----------------------------------------------------------------------------
 * d_flags: `count` device uint32.  d_flags[i] becomes 1 when item i holds a block the single-buffer classification flags, else 0:
 *   BC1  a fully transparent block, or a solid colour that normalisation would rewrite;
 *   BC2  a colour half that is one normalisable solid colour;
 *   BC3  a uniform alpha half or such a colour half -- a block already in normal form counts.
 * The call writes all `count` flags itself (zeroed first, in stream order) and nothing else.  Only d_input, len and format of an
 * item are read; they are validated as above (d_flags == NULL with count > 0: DXTLT_E_INVALID_ARGUMENT).  Any input alignment.
 * One launch for the whole batch, all formats mixed, one block per lane; empty items own no workgroup and their flag is 0.
 * Asynchronous on `hip_stream`; its table is staged like the other batch tables. */
int32_t dxtlt_batch_any_normalizable_device(const DxtltBatchNormalizeItem *items, size_t count, uint32_t *d_flags, void *hip_stream);

/* Test hook, no device needed, nothing is dereferenced: what dxtlt_transform_batch_with_normalize_blocks_device would enqueue for
 * these items -- the call's own planner.  One record per launch, in stream order: kind 1 = a plain tile launch
 * (dxtlt_debug_plan_batch_call's record of it, field for field), kind 4 = a normalising tile launch (settings_code: the settings
 * code, for BC1 | color_mode << 8; strided is 0), kind 2 = an item that goes out alone.  Returns the number of launches (records
 * beyond `cap` are counted, not written); 0 for count == 0; for a batch the call refuses, minus the status the call returns.
 * *table_bytes_out: the bytes of the one staged buffer. */
int32_t dxtlt_debug_plan_batch_normalize_call(const DxtltBatchNormalizeItem *items, size_t count, DxtltDebugBatchLaunch *out,
                                              size_t cap, uint64_t *table_bytes_out);

#ifdef __cplusplus
}
#endif
#endif
