/*
 * dxtlt_bc6h.h -- BC6H granule-sorted field split, layout version 1: C ABI (libdxtlt_gfx950.so).
 *
 * A FORMAT DEFINED BY THIS BUILD (docs/BC6H_FORMAT.md).  Upstream parses BC6H DDS files and reserves
 * TransformFormat::Bc6H = 4, but has no BC6H transform.  The layout is BC7's (dxtlt_bc7.h): granules of 1024 blocks
 * sorted by mode, eight byte streams, a main part and a tail part; only the record inside a block differs.  UF16, SF16
 * and typeless payloads are the same bits and take the same transform.  Parity: exact round trip and GPU ==
 * tests/bc6h_ref.py.
 *
 * Contract: len is a multiple of 16; output length == input length; buffers must not overlap; returns DXTLT_* status
 * codes of dxtlt_gfx950.h.  Device-pointer calls take any pointer alignment (16-byte aligned buffers are the fast case);
 * they enqueue one kernel (two when the block count is not a multiple of 1024) on the stream, use no scratch memory and
 * do not synchronise, so they can be captured into a HIP graph.
 */
#ifndef DXTLT_BC6H_H
#define DXTLT_BC6H_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int32_t dxtlt_transform_bc6h(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len);
int32_t dxtlt_untransform_bc6h(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len);

int32_t dxtlt_transform_bc6h_device(const void *d_input, void *d_output, size_t len, void *hip_stream);
int32_t dxtlt_untransform_bc6h_device(const void *d_input, void *d_output, size_t len, void *hip_stream);

/* One block range of an array of total_blocks blocks, as dxtlt_transform_bc7_range_device: the AoS-side pointer is the
 * range's first block, the SoA-side pointer byte 0 of the WHOLE transformed buffer.  first_block must be a multiple of
 * dxtlt_bc6h_sort_granule() and the range must end on one or at the end of the array. */
int32_t dxtlt_transform_bc6h_range_device(bool inverse, const void *d_src, void *d_dst, uint64_t total_blocks,
                                          uint64_t first_block, uint64_t num_blocks, void *hip_stream);
uint32_t dxtlt_bc6h_sort_granule(void); /* 1024 */

/* Single-process multi-GPU, as dxtlt_transform_bc7_sharded: contiguous granule-aligned block ranges over the node's GPUs,
 * no collective.  num_shards <= 0: one shard per visible device.  At most 64 shards.  Same result as the unsharded call. */
int32_t dxtlt_transform_bc6h_sharded(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, int32_t num_shards);
int32_t dxtlt_untransform_bc6h_sharded(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, int32_t num_shards);

/* The placement of one shard (host code, no device), as dxtlt_bc7_shard_pieces: p = 0..7 its slice of main stream p
 * (Q8, Q2, B0..B4, F), p = 8 the tail part.  Arrays of 9. */
int32_t dxtlt_bc6h_shard_pieces(uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks, uint64_t *global_off,
                                uint64_t *local_off, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif /* DXTLT_BC6H_H */
