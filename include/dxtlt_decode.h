/*
 * dxtlt_decode.h -- C ABI of the block decoders of libdxtlt_gfx950.so: the MI355X implementation of the reference's
 * util modules as array operations
 *
 *   decode_bc1_block   core/dxt-lossless-transform-bc1/src/util/bc1_decode.rs:42   (+ _from_slice :109)
 *   decode_bc2_block   core/dxt-lossless-transform-bc2/src/util/bc2_decode.rs:44   (+ _from_slice :130)
 *   decode_bc3_block   core/dxt-lossless-transform-bc3/src/util/bc3_decode.rs:43   (+ _from_slice :181)
 *   Decoded4x4Block    core/dxt-lossless-transform-common/src/decoded_4x4_block.rs:56
 *
 * The reference decodes one block per call; here one call decodes `len / block_size` blocks into that many
 * Decoded4x4Block records: 64 bytes each, sixteen pixels in row-major order, every pixel the bytes r, g, b, a
 * (Color8888, color_8888.rs:30).  BC1 uses the three-colour + transparent mode when c0 <= c1; BC2 / BC3 colours are
 * always four-colour; interpolation is the "ideal" DX9 rounding the reference documents (integer / 3, / 2, / 7, / 5
 * on the 8-bit expansions).
 *
 * dxtlt_count_pixel_differences_*: the number of blocks whose sixteen decoded pixels differ between two block arrays
 * of equal length -- what the reference's normalisation tests assert to be zero ("decode before == decode after").
 *
 * Status codes and dxtlt_last_error() as in dxtlt_gfx950.h: 1 = len not a multiple of the block size, 2 = NULL
 * pointer, bad format or pixels_len < 64 * blocks.
 */
#ifndef DXTLT_DECODE_H
#define DXTLT_DECODE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXTLT_DECODED_BLOCK_BYTES 64

/* ---- host pointers ---------------------------------------------------------------------------------- */
int32_t dxtlt_decode_bc1_blocks(const uint8_t *blocks, size_t len, uint8_t *pixels, size_t pixels_len);
int32_t dxtlt_decode_bc2_blocks(const uint8_t *blocks, size_t len, uint8_t *pixels, size_t pixels_len);
int32_t dxtlt_decode_bc3_blocks(const uint8_t *blocks, size_t len, uint8_t *pixels, size_t pixels_len);
/* format = 1, 2, 3 */
int32_t dxtlt_count_pixel_differences(int32_t format, const uint8_t *blocks_a, const uint8_t *blocks_b, size_t len,
                                      uint64_t *out_count);

/* ---- device pointers, asynchronous on `hip_stream` --------------------------------------------------- */
int32_t dxtlt_decode_bc1_blocks_device(const void *d_blocks, size_t len, void *d_pixels, size_t pixels_len, void *hip_stream);
int32_t dxtlt_decode_bc2_blocks_device(const void *d_blocks, size_t len, void *d_pixels, size_t pixels_len, void *hip_stream);
int32_t dxtlt_decode_bc3_blocks_device(const void *d_blocks, size_t len, void *d_pixels, size_t pixels_len, void *hip_stream);
/* d_count = one uint64_t in device memory; zeroed, then accumulated, on the stream */
int32_t dxtlt_count_pixel_differences_device(int32_t format, const void *d_blocks_a, const void *d_blocks_b, size_t len,
                                             uint64_t *d_count, void *hip_stream);

/* ---- test hooks, no device needed ---------------------------------------------------------------------
 * The host-pointer calls above stage through device buffers in slices: dxtlt_decode_bcN_blocks takes 2^22 blocks (256 MiB of
 * pixels) per slice, dxtlt_count_pixel_differences 256 MiB of each array per slice and adds the slices' counts.
 * dxtlt_debug_array_op_slices returns those two sizes (either pointer may be NULL). */
void dxtlt_debug_array_op_slices(uint64_t *decode_slice_blocks, uint64_t *difference_slice_bytes);

/* What one `_device` call of this header or of dxtlt_color565.h would launch for these addresses -- the launch functions' own
 * plan; addresses are numbers here, nothing is dereferenced.  `count` is what the operation counts in:
 *   DXTLT_ARRAY_OP_YCOCG              addr0 = src, addr1 = dst; colours (variants 1..3: variant 0 is a copy and launches nothing)
 *   DXTLT_ARRAY_OP_RECORRELATE_SPLIT  addr0 = src_0, addr1 = src_1, addr2 = dst; colour pairs (num_items / 2)
 *   DXTLT_ARRAY_OP_SPLIT_ENDPOINTS    addr0 = colors, addr1 = colors_out; colour pairs (colors_len_bytes / 4)
 *   DXTLT_ARRAY_OP_DECODE + format    addr0 = blocks, addr1 = pixels; blocks
 *   DXTLT_ARRAY_OP_DIFFERENCE + format  addr0 = blocks_a, addr1 = blocks_b; blocks
 * Returns 0, or -1 for an unknown op or a NULL `out`.  count == 0 launches nothing: every field but `threads` is 0. */
#define DXTLT_ARRAY_OP_YCOCG 0
#define DXTLT_ARRAY_OP_RECORRELATE_SPLIT 1
#define DXTLT_ARRAY_OP_SPLIT_ENDPOINTS 2
#define DXTLT_ARRAY_OP_DECODE 10     /* + format 1, 2, 3 */
#define DXTLT_ARRAY_OP_DIFFERENCE 20 /* + format 1, 2, 3 */
typedef struct DxtltDebugArrayOpPlan {
    int32_t vector;        /* 1 = the vector route: colour arrays 16 bytes per lane; decode: vector loads, stores staged through LDS;
                              difference: vector loads.  0 = the route for any alignment: byte loads and stores */
    int32_t threads;       /* lanes per workgroup */
    uint64_t vector_lanes; /* colour arrays: lanes that write one 16-byte vector (8 colours / 4 pairs / 8 pairs); decode and
                              difference: the blocks, on the vector route */
    uint64_t single_lanes; /* colour arrays: lanes behind them that take one colour (ycocg) or one pair; decode and difference: the
                              blocks, on the byte route */
    uint64_t workgroups;
    uint64_t steps;        /* difference: steps the busiest workgroup takes through the array (the grid is capped at 4096
                              workgroups of 512 blocks per step); every other launch: 1 */
} DxtltDebugArrayOpPlan;
int32_t dxtlt_debug_plan_array_op(int32_t op, uint64_t addr0, uint64_t addr1, uint64_t addr2, uint64_t count,
                                  DxtltDebugArrayOpPlan *out);

#ifdef __cplusplus
}
#endif
#endif
