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
/* Test hook: the same kernel with the same checks, into 5 * len bytes of the CALLER's at d_arena (any alignment: in the thread's
 * arena candidate i starts i * len past a 256-byte boundary, which reaches every residue) -- candidate i < 5 at d_arena + i * len,
 * byte for byte what dxtlt_transform_pixels_device writes for that setting, and no other byte.  Enqueues only. */
int32_t dxtlt_debug_pixels_auto_candidates_into_device(const void *d_input, size_t len, int32_t pixel_bytes, void *d_arena,
                                                       void *hip_stream);

/* ---- many buffers in one call (docs/PIXEL_FORMAT.md, "Many buffers in one call") -------------------------------------------------
 * dxtlt_transform_pixels_batch_device: for every item the bytes in d_output are exactly what dxtlt_transform_pixels_device
 * (inverse = 0) or dxtlt_untransform_pixels_device (inverse = 1) writes for that item alone, and no byte outside an item's own len
 * output bytes is written -- with ONE kernel launch per (pixel_bytes, inverse, decorrelate, layout) class present in the batch (at
 * most 24) and one small table upload, however many items there are.  Any pointer alignment and any pixel count per item.
 * Asynchronous: enqueues on `hip_stream` and does not wait for it; ordered like a single call.  count == 0 is a no-op; an item with
 * len == 0 needs no pointers and owns no workgroup.
 *
 * The whole batch is checked before anything is enqueued.  DXTLT_E_INVALID_ARGUMENT: NULL `items` with count > 0; pixel_bytes not
 * 3 or 4; layout > 2; a NULL buffer with len > 0; an item of 64 GiB or more; a d_output that overlaps any other d_output or any
 * d_input of the batch (inputs may overlap one another); a class of 2^24 tiles of 4096 pixels or more -- 256 GiB of 4-byte,
 * 192 GiB of 3-byte pixels: the limit of one launch of dxtlt_transform_batch_device; a capturing stream.  DXTLT_E_INVALID_LENGTH:
 * len not a multiple of pixel_bytes.
 *
 * Not capturable.  Like dxtlt_transform_batch_device the call stages its tables in ONE of four per-thread slots of pinned host
 * memory, which a small kernel copies to the device on `hip_stream`; taking a slot may wait (on the host) for the event of the
 * call that used it last -- so do not enqueue more than four batch calls of one thread behind an event that is recorded later --
 * and a replayed graph would copy whatever a later call has put into the slot.  So a capturing stream, or one whose capture state
 * cannot be queried, is refused with nothing enqueued, as the auto calls refuse it. */
typedef struct DxtltPixelBatchItem {
    const void *d_input;
    void *d_output;        /* len bytes */
    uint64_t len;          /* a multiple of pixel_bytes; 0 is allowed */
    uint8_t pixel_bytes;   /* 4 or 3 */
    uint8_t inverse;       /* 0 = transform, 1 = untransform */
    uint8_t decorrelate;   /* 0 / not 0 */
    uint8_t layout;        /* DXTLT_PIXEL_LAYOUT_* */
    uint8_t reserved[4];
} DxtltPixelBatchItem;
int32_t dxtlt_transform_pixels_batch_device(const DxtltPixelBatchItem *items, size_t count, void *hip_stream);

/* Test hook, no device needed: what dxtlt_transform_pixels_batch_device would enqueue for these items -- the call's own planner,
 * addresses are numbers, nothing is dereferenced.  One record per launch in stream order (4-byte pixels first; then forward before
 * inverse, plain before decorrelate, layout 0, 1, 2).  Returns the number of launches (records beyond `cap` are counted, not
 * written); 0 for count == 0; -1 for a batch the call refuses (dxtlt_last_error() says why).  *table_bytes_out: the bytes of the
 * ONE staged buffer that holds every launch's entries (32 bytes per non-empty item) and workgroup index. */
typedef struct DxtltDebugPixelBatchLaunch {
    uint8_t pixel_bytes, inverse, decorrelate, layout;
    uint32_t items;          /* non-empty items of the class = table entries */
    uint32_t workgroups;     /* tiles of 4096 pixels */
    uint32_t wide;           /* 1 = 16-bit deltas in the workgroup index (dxtlt_debug_plan_batch, dxtlt_gfx950.h) */
    uint64_t table_offset;   /* where the launch's tables start in the staged buffer (a multiple of 16) ... */
    uint64_t table_bytes;    /* ... and their bytes */
} DxtltDebugPixelBatchLaunch;
int32_t dxtlt_debug_plan_pixels_batch(const DxtltPixelBatchItem *items, size_t count, DxtltDebugPixelBatchLaunch *launches_out, size_t cap,
                                      uint64_t *table_bytes_out);

/* dxtlt_transform_pixels_batch_auto_device: dxtlt_transform_pixels_auto_device for every item of a batch -- the same six candidates
 * in the same order, each candidate's whole output one section of the entropy estimator, strict `<` from UINT64_MAX; the same
 * choice, totals and output bytes per item -- with ONE wait for `hip_stream` and a launch count that does not grow with the number
 * of items.  Per chunk of the batch one candidate launch per pixel_bytes present (at most two; a d_input at any alignment is read
 * once for its five candidates, into this thread's candidate arena) and ONE estimator launch over all six sections of all its
 * items; all counters come back in one copy; the pick is made on the host and written into the items' result fields before the call
 * returns; the winners go out through dxtlt_transform_pixels_batch_device's planner and kernels (at most 12 launches), enqueued
 * and not waited for: they read the d_inputs only, so when the call returns nothing in flight touches the arena or the counters.
 * An empty item keeps (decorrelate, PLANAR_DELTA) and nothing is written for it.
 *
 * Every item owns a 16-byte aligned slice of 5 * len bytes of the arena; a chunk is closed before the item that would push its
 * slices past DXTLT_BATCH_AUTO_ARENA_CAP (dxtlt_estimator.h; the test hook dxtlt_debug_batch_auto_arena_cap governs this call
 * too), and an item whose slice alone is larger is a chunk by itself.  The stream orders the reuse of the arena between chunks.
 *
 * Refused before anything is enqueued and with the result fields untouched: everything dxtlt_transform_pixels_batch_device
 * refuses (a d_output may overlap no input or output of the batch); a capturing stream (DXTLT_E_INVALID_ARGUMENT: the call reads
 * its estimates back and waits); a batch with 2^24 tiles or more of one pixel_bytes, whichever settings would win.  On every
 * failure exit the stream is drained before the arena can be reused. */
typedef struct DxtltPixelBatchAutoItem {
    const void *d_input;
    void *d_output;        /* len bytes, overlapping no input or output of the batch */
    uint64_t len;
    uint8_t pixel_bytes;
    /* results, written before the call returns */
    uint8_t decorrelate;
    uint8_t layout;
    uint8_t reserved[5];
} DxtltPixelBatchAutoItem;
int32_t dxtlt_transform_pixels_batch_auto_device(DxtltPixelBatchAutoItem *items, size_t count, void *hip_stream);

/* Test hook, no device needed: the plan of dxtlt_transform_pixels_batch_auto_device for these items (nothing is dereferenced).
 * items_out[i]: the item's chunk, its slice of the arena and its six sections in candidate order -- sections 0..4 at
 * arena_offset + i * len of the arena (in_arena = 1), section 5 the item's d_input itself (in_arena = 0, offset 0); counter =
 * 6 * item + section.  chunks_out[c] (at most chunk_capacity are written; *out_chunks receives how many there are).  Returns
 * DXTLT_OK or the status the call would return before any device work. */
typedef struct DxtltDebugPixelBatchAutoSection {
    uint64_t offset;
    uint64_t len;
    uint32_t counter;
    uint32_t in_arena;
} DxtltDebugPixelBatchAutoSection;
typedef struct DxtltDebugPixelBatchAutoPlanItem {
    uint32_t chunk;
    uint32_t reserved;
    uint64_t arena_offset;   /* a multiple of 16 */
    uint64_t arena_bytes;    /* 5 * len */
    DxtltDebugPixelBatchAutoSection sections[6];
} DxtltDebugPixelBatchAutoPlanItem;
typedef struct DxtltDebugPixelBatchAutoPlanChunk {
    uint64_t first_item, item_count;
    uint64_t arena_bytes;
    uint32_t candidate_launches;     /* 0..2: one per pixel_bytes with a non-empty item */
    uint32_t estimator_workgroups;   /* 32 KiB windows of all six sections of all items */
} DxtltDebugPixelBatchAutoPlanChunk;
int32_t dxtlt_debug_plan_pixels_batch_auto(const DxtltPixelBatchAutoItem *items, size_t count, DxtltDebugPixelBatchAutoPlanItem *items_out,
                                           DxtltDebugPixelBatchAutoPlanChunk *chunks_out, size_t chunk_capacity, size_t *out_chunks);

/* Test hook: the candidate launches of ONE chunk of dxtlt_transform_pixels_batch_auto_device into memory of the caller's.  Plans
 * as the call does (at the arena cap in force on the thread), writes the call's tables for an arena at d_arena, uploads them, runs
 * chunk `chunk`'s candidate launches -- one per pixel_bytes present -- and WAITS for `hip_stream`: item k of the chunk has its five
 * candidates at d_arena + arena_offset (dxtlt_debug_plan_pixels_batch_auto) + i * len and no other byte of the arena is written.
 * No d_output is touched (the items must still pass the call's checks) and no estimator is launched.  Refused with nothing
 * enqueued: what the call refuses, with its status; DXTLT_E_INVALID_ARGUMENT for a chunk that does not exist, a NULL d_arena, an
 * arena_bytes below that chunk's arena_bytes and a capturing stream. */
int32_t dxtlt_debug_pixels_batch_candidates_device(const DxtltPixelBatchAutoItem *items, size_t count, size_t chunk, void *d_arena,
                                                   uint64_t arena_bytes, void *hip_stream);

/* Test hooks, per calling thread, read-only.  last: of this thread's last dxtlt_transform_pixels_batch_auto_device, out[0] the
 * stream waits, out[1] the chunks, out[2] the candidate launches, out[3] the estimator launches (all 0 after a refused or an
 * all-empty batch; the winners' launches are not counted).  last_totals: the six totals that call compared for `item`, in candidate
 * order; returns how many there were (0 for an empty item, an item out of range or a failed call); writes at most cap. */
void dxtlt_debug_pixels_batch_auto_last(uint64_t out[4]);
int32_t dxtlt_debug_pixels_batch_auto_last_totals(size_t item, uint64_t *out, int32_t cap);
/* Bench hooks, per calling thread.  time_phases: anything but 0 = the batched pixel auto calls record HIP events around the
 * phases of every chunk and around the winners and wait for the winners before they return; last_phase_ms then reports, for the
 * last such call, the milliseconds summed over its chunks: out[0] the candidate launches, out[1] the estimator launches, and
 * out[2] the winners' launches. */
void dxtlt_debug_pixels_batch_auto_time_phases(int32_t on);
void dxtlt_debug_pixels_batch_auto_last_phase_ms(double out[3]);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_PIXELS_H */
