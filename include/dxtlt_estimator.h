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

/* ---- the batched auto transform: many device-resident buffers, the best settings chosen for each, in one call ----------------
 * For every item the choice (written into the item's result fields before the call returns) and the bytes in d_output are exactly
 * what dxtlt_transform_bcN_auto_device(d_input, d_output, len, use_all_decorrelation_modes, ...) gives for that item alone: the
 * same candidates in the same order, the same sections shown to the estimator, the same additions and strict `<`.  An empty item
 * keeps the first candidate of its order and nothing is written for it.
 *
 * The whole batch is validated before anything is enqueued: NULL items with count > 0, a format outside 1..5 and a NULL buffer
 * with len > 0 are DXTLT_E_INVALID_ARGUMENT, a len that is not a multiple of the block size DXTLT_E_INVALID_LENGTH, an item of
 * 64 GiB or more and a d_output that overlaps any other d_output or any d_input of the batch DXTLT_E_INVALID_ARGUMENT (inputs
 * may overlap one another).  On a capturing stream, or one whose capture state cannot be queried, the call returns
 * DXTLT_E_INVALID_ARGUMENT and enqueues nothing.
 *
 * A batch whose winning transforms could not go out in one launch per (format, settings) is refused with the rest, before the
 * choices are known: per format the items together may hold at most 2^24 - 1 tiles, counted as len / block size / 256 + 2 per
 * item (about 32 GiB of BC1 / BC4 or 64 GiB of BC2 / BC3 / BC5 items): DXTLT_E_INVALID_ARGUMENT.
 *
 * The call WAITS for `hip_stream` exactly once, to read the counters back (at most 10 eight-byte counters per item), whatever
 * the number of items; the number of launches does not grow with it either: per chunk one candidate launch per (format,
 * use_all_decorrelation_modes) present and ONE estimator launch, then the winning transforms through the path of
 * dxtlt_transform_batch_device, enqueued and not waited for.  They read the d_inputs only: when the call returns nothing in
 * flight touches this thread's arena or counters.  Formats and use_all values may be mixed; d_input and d_output may have any
 * alignment (a d_input off a 16-byte boundary is read with narrower loads: the same choice and bytes, no further wait).
 * What the winners inherit from dxtlt_transform_batch_device: an item whose d_output is off an 8-byte boundary is transformed by
 * a launch of its own (one more launch per such item, no wait), and that call's ring of four table slots makes the HOST wait for
 * an earlier batch call of this thread when four of them are still in flight -- a wait for earlier work, not for this call's
 * stream.  dxtlt_debug_batch_auto_last counts the waits and launches this call makes itself, not those.
 *
 * Chunks: every item owns a 16-byte aligned slice of the per-thread candidate arena -- 16 / 32 bytes per block for BC1 and BC2
 * (fast / all modes), 20 / 36 for BC3, 4 for BC4, 8 for BC5.  A chunk is closed before the item that would push its slices past
 * DXTLT_BATCH_AUTO_ARENA_CAP bytes; an item whose slice alone is larger is a chunk by itself.  The stream orders the reuse of
 * the arena from chunk to chunk. */
#define DXTLT_BATCH_AUTO_ARENA_CAP (256ull << 20)

typedef struct DxtltBatchAutoItem {
    const void *d_input;
    void *d_output;                      /* len bytes, overlapping no input or output of the batch */
    uint64_t len;                        /* a multiple of the block size; 0 is allowed */
    uint8_t format;                      /* 1..5 = BC1..BC5 */
    uint8_t use_all_decorrelation_modes; /* ignored for 4, 5 */
    /* results, written before the call returns */
    uint8_t decorrelation_mode;          /* core numbering; 0 for BC4 / BC5 */
    uint8_t split_alpha_endpoints;       /* BC3; BC4 / BC5: split_endpoints */
    uint8_t split_colour_endpoints;
    uint8_t reserved[3];
} DxtltBatchAutoItem;

int32_t dxtlt_transform_batch_auto_device(DxtltBatchAutoItem *items, size_t count, void *hip_stream);

/* Test hook, no device needed (addresses are numbers, nothing is dereferenced): the plan dxtlt_transform_batch_auto_device
 * makes for `items` -- after the same validation, whose status it returns.  items_out: `count` records; chunks_out: up to
 * chunk_capacity records (chunks beyond it are counted, not written); *out_chunks: the number of chunks.  A section's
 * arena_offset counts from the arena's first byte; sections are listed in slice order: BC3's alpha pairs and alpha split, then
 * per variant colour pairs and colour split; BC4 pairs, split; BC5 red pairs, red split, green pairs, green split.  A total is
 * BC3: alpha + colour, BC5: red + green of the same kind, else one section. */
typedef struct DxtltDebugBatchAutoSection {
    uint64_t arena_offset;
    uint64_t len;
    uint32_t counter; /* index into the batch's counter buffer */
    uint32_t reserved;
} DxtltDebugBatchAutoSection;
typedef struct DxtltDebugBatchAutoPlanItem {
    uint32_t chunk;
    uint32_t section_count;
    uint64_t arena_offset; /* of the item's slice */
    uint64_t arena_bytes;  /* of the item's slice, before it is padded to 16 */
    DxtltDebugBatchAutoSection sections[10];
} DxtltDebugBatchAutoPlanItem;
typedef struct DxtltDebugBatchAutoPlanChunk {
    uint64_t first_item;
    uint64_t item_count;
    uint64_t arena_bytes;
    uint32_t candidate_launches;
    uint32_t estimator_workgroups;
} DxtltDebugBatchAutoPlanChunk;
int32_t dxtlt_debug_plan_batch_auto(const DxtltBatchAutoItem *items, size_t count, DxtltDebugBatchAutoPlanItem *items_out,
                                    DxtltDebugBatchAutoPlanChunk *chunks_out, size_t chunk_capacity, size_t *out_chunks);

/* Test hook: of the last dxtlt_transform_batch_auto_device call of this thread: stream waits, chunks, candidate launches,
 * estimator launches. */
void dxtlt_debug_batch_auto_last(uint64_t out[4]);

/* Test hook: the totals that call compared for item `item`, in candidate order; returns how many there were (0 for an item
 * index out of range, a failed call or an empty item); writes at most cap. */
int32_t dxtlt_debug_batch_auto_last_totals(size_t item, uint64_t *out, int32_t cap);

/* Test hook, per calling thread: the chunk cap in bytes in place of DXTLT_BATCH_AUTO_ARENA_CAP; 0 restores the default. */
void dxtlt_debug_batch_auto_arena_cap(uint64_t bytes);

/* Bench hook, per calling thread: anything but 0 = dxtlt_transform_batch_auto_device records HIP events around the candidate
 * launches and the estimator launch of every chunk (three events per chunk, created and destroyed by the call).
 * dxtlt_debug_batch_auto_last_phase_ms then reports, for the last such call of this thread, the milliseconds between them summed
 * over the chunks: out[0] candidate launches, out[1] estimator launches ({0, 0} after a call without the switch). */
void dxtlt_debug_batch_auto_time_phases(int32_t on);
void dxtlt_debug_batch_auto_last_phase_ms(double out[2]);

/* Test hook: what the last auto transform called from this thread (host or device pointers, any format) moved and called for
 * its estimates: bytes of candidate sections copied to the host, and calls made through the estimator's vtable
 * (MaxCompressedSize and EstimateCompressedSize).  Both are 0 with the built-in estimator and after the batched call.  Either pointer may be NULL. */
void dxtlt_debug_auto_last_estimation(uint64_t *out_section_bytes_downloaded, uint64_t *out_estimator_callbacks);

/* Test hook: the totals the last built-in-estimator auto transform of this thread compared, in candidate order;
 * returns how many there were (0 after a callback-route call, an empty buffer or a failed call); writes at most cap. */
int32_t dxtlt_debug_auto_last_totals(uint64_t *out_totals, int32_t cap);

/* Test hook, per calling thread: 0 = the auto transforms, with the built-in estimator or a caller's, behave as if their candidate
 * arena could not be allocated (one full transform per candidate into the output buffer, estimated there or downloaded from
 * there); anything else = normal. */
void dxtlt_debug_auto_use_arena(int32_t on);

/* Test hook: the code the estimator's callback returned in the last dxtlt_transform_bc{1..5}_auto call of this thread, 0 when none
 * failed.  The BC4 / BC5 calls have no out parameter for it. */
uint32_t dxtlt_debug_auto_last_estimator_error(void);

/* Test hook, no device needed: the host-side pick of the device routes, on section sizes given by the caller instead of read back.
 * It runs the function the routes run after their readback.  route 0: dxtlt_transform_bcN_auto_device -- BC1-3 the distinct
 * sections as route 1 takes them, BC4 / BC5 two slots per candidate (BC4 reads the first of each).  route 1:
 * dxtlt_transform_batch_auto_device, the counters of one item -- the distinct sections in the order they lie in memory (BC3 alpha
 * pairs, alpha split, then per variant colour pairs, colour split; BC4 pairs, split; BC5 red pairs, red split, green pairs,
 * green split).  route 2: route 0 without its arena, two slots per candidate for every format (BC1, BC2 and BC4 read the first of
 * each).  n_sizes must be what the route reads back (DXTLT_E_INVALID_ARGUMENT otherwise).  Writes at most cap candidate totals,
 * in candidate order, and the settings of the pick (split_alpha = split_endpoints for BC4 / BC5); any output pointer may be NULL. */
int32_t dxtlt_debug_auto_pick(int32_t route, int32_t format, bool use_all_decorrelation_modes, const uint64_t *section_sizes,
                              int32_t n_sizes, uint64_t *totals_out, int32_t cap, uint8_t *mode, bool *split_alpha,
                              bool *split_colour);

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

/* Test hook: the same launch or launches -- launch_auto_candidates of the fused route: auto_candidates_kernel<format, fast | all>
 * over the whole 16-byte vectors and, for an odd BC1 block count, auto_candidates_bc1_last_block -- into memory of the caller's:
 * every section of format 1..3, laid out as the batched call's note on sections says (BC3's alpha pairs and alpha split, then per
 * variant colour pairs and colour split), end to end from d_arena; 16 / 32 bytes per block for BC1 and BC2 (fast / all modes),
 * 20 / 36 for BC3, and no other byte.  Only enqueues on `hip_stream`.  DXTLT_E_INVALID_ARGUMENT with nothing enqueued: another
 * format, a len that is not a multiple of the block size, d_input or d_arena off a 16-byte boundary (the kernel's own
 * requirement) or NULL with len != 0, arena_bytes below the sections' bytes.  len == 0: DXTLT_OK, nothing enqueued. */
int32_t dxtlt_debug_auto_candidates_into_device(int32_t format, bool use_all_decorrelation_modes, const void *d_input, size_t len,
                                                void *d_arena, uint64_t arena_bytes, void *hip_stream);

/* Test hook: the candidate launches of ONE chunk of dxtlt_transform_batch_auto_device over `items`, into memory of the caller's.
 * Plans as the call does, at the arena cap in force on the thread (dxtlt_debug_batch_auto_arena_cap), fills the call's tables for
 * an arena whose first byte is d_arena, uploads them, runs chunk `chunk`'s candidate launches -- one per (format,
 * use_all_decorrelation_modes) present, through the function the call runs them through -- and waits for `hip_stream`.  Item k of
 * the chunk then has its slice at d_arena + arena_offset (dxtlt_debug_plan_batch_auto; offsets restart in every chunk), its sections
 * where that hook lists them; no other byte of the arena, no d_output and no result field is written and no estimator runs.
 * With nothing enqueued: whatever the call refuses, with the call's status; DXTLT_E_INVALID_ARGUMENT for a chunk the plan does not
 * have (count == 0 has none), a NULL d_arena or one off a 16-byte boundary, arena_bytes below that chunk's arena_bytes, and a
 * capturing stream. */
int32_t dxtlt_debug_batch_auto_candidates_device(const DxtltBatchAutoItem *items, size_t count, size_t chunk, void *d_arena,
                                                 uint64_t arena_bytes, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
