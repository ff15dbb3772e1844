/*
 * dxtlt_bc23_normalize.h -- C ABI of the BC2 / BC3 block-normalisation entry points of libdxtlt_gfx950.so: the MI355X
 * implementation of the reference's experimental modules
 *   /root/reference/src/core/dxt-lossless-transform-bc2/src/experimental/normalize_blocks/normalize.rs
 *   /root/reference/src/core/dxt-lossless-transform-bc3/src/experimental/normalize_blocks/normalize.rs
 * (Rust-only upstream, like the BC1 module: see dxtlt_bc1_normalize.h and INTEGRATION.md section 6).
 *
 *   normalize_blocks                    bc2 normalize.rs:35     bc3 normalize.rs:36
 *   normalize_blocks_all_modes          bc2 normalize.rs:193    bc3 normalize.rs:419
 *   normalize_split_blocks_in_place     bc2 normalize.rs:382    bc3 normalize.rs:539
 *
 * ColorNormalizationMode: None = 0, Color0Only = 1, ReplicateColor = 2 (bc2 normalize.rs:339-352).  The colour half of a
 * block (bytes 8..15; always decoded in four-colour mode, alpha ignored) whose 16 pixels are one colour that survives
 * RGBA8888 -> RGB565 -> RGBA8888 becomes (colour, 0, indices 0) or (colour, colour, indices 0).  BC2's explicit alpha
 * (bytes 0..7) is never changed.
 * AlphaNormalizationMode (BC3, bc3 normalize.rs:117-139): None = 0, UniformAlphaZeroIndices = 1, OpaqueFillAll = 2,
 * OpaqueZeroAlphaMaxIndices = 3.  An alpha half (bytes 0..7) whose 16 decoded alpha values are equal becomes
 * (alpha, 0, indices 0); for alpha == 255, mode 2 writes eight 0xFF bytes and mode 3 writes (0, 0, indices 0xFF).
 *
 * `len` in bytes, a multiple of 16; any pointer alignment; any block count including 0; input == output is allowed for
 * normalize_blocks.  Status codes and dxtlt_last_error() as in dxtlt_gfx950.h.
 */
#ifndef DXTLT_BC23_NORMALIZE_H
#define DXTLT_BC23_NORMALIZE_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DXTLT_ALPHA_NORMALIZE_NONE 0
#define DXTLT_ALPHA_NORMALIZE_UNIFORM_ALPHA_ZERO_INDICES 1
#define DXTLT_ALPHA_NORMALIZE_OPAQUE_FILL_ALL 2
#define DXTLT_ALPHA_NORMALIZE_OPAQUE_ZERO_ALPHA_MAX_INDICES 3

/* ---- host pointers ---------------------------------------------------------------------------------- */
int32_t dxtlt_bc2_normalize_blocks(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, uint8_t color_mode);
/* alpha_ptr (8 bytes per block) is part of the reference signature; the decision does not depend on it: may be NULL */
int32_t dxtlt_bc2_normalize_split_blocks_in_place(const uint8_t *alpha_ptr, uint8_t *colors_ptr, uint8_t *indices_ptr,
                                                  size_t num_blocks, uint8_t color_mode);
/* output_ptrs[color_mode] */
int32_t dxtlt_bc2_normalize_blocks_all_modes(const uint8_t *input_ptr, uint8_t *const output_ptrs[3], size_t len);

int32_t dxtlt_bc3_normalize_blocks(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len, uint8_t alpha_mode,
                                   uint8_t color_mode);
/* the four sections of the unsplit-endpoint BC3 layout: 2, 6, 4 and 4 bytes per block */
int32_t dxtlt_bc3_normalize_split_blocks_in_place(uint8_t *alpha_endpoints_ptr, uint8_t *alpha_indices_ptr,
                                                  uint8_t *color_endpoints_ptr, uint8_t *color_indices_ptr,
                                                  size_t num_blocks, uint8_t alpha_mode, uint8_t color_mode);
/* output_ptrs[alpha_mode * 3 + color_mode] (the reference's [alpha_mode][color_mode] array, flattened) */
int32_t dxtlt_bc3_normalize_blocks_all_modes(const uint8_t *input_ptr, uint8_t *const output_ptrs[12], size_t len);

/* ---- device pointers, asynchronous on `hip_stream` --------------------------------------------------- */
int32_t dxtlt_bc2_normalize_blocks_device(const void *d_input, void *d_output, size_t len, uint8_t color_mode,
                                          void *hip_stream);
int32_t dxtlt_bc2_normalize_split_blocks_in_place_device(void *d_colors, void *d_indices, size_t num_blocks,
                                                         uint8_t color_mode, void *hip_stream);
int32_t dxtlt_bc2_normalize_blocks_all_modes_device(const void *d_input, void *const d_outputs[3], size_t len,
                                                    void *hip_stream);
int32_t dxtlt_bc3_normalize_blocks_device(const void *d_input, void *d_output, size_t len, uint8_t alpha_mode,
                                          uint8_t color_mode, void *hip_stream);
int32_t dxtlt_bc3_normalize_split_blocks_in_place_device(void *d_alpha_endpoints, void *d_alpha_indices,
                                                         void *d_color_endpoints, void *d_color_indices,
                                                         size_t num_blocks, uint8_t alpha_mode, uint8_t color_mode,
                                                         void *hip_stream);
int32_t dxtlt_bc3_normalize_blocks_all_modes_device(const void *d_input, void *const d_outputs[12], size_t len,
                                                    void *hip_stream);

/* ---- normalise + transform in one pass ------------------------------------------------------------------
 * The BC2 / BC3 counterpart of dxtlt_transform_bc1_with_normalize_blocks (dxtlt_bc1_normalize.h): block normalisation fused
 * into the forward transform kernels.  Upstream has no such function for BC2 / BC3; the contract is the composition
 *
 *   output == transform_bcN_with_settings(normalize_blocks(input, modes), settings)           byte for byte
 *   untransform_bcN_with_settings(output, settings) == normalize_blocks(input, modes)
 *
 * Modes: color_mode 0..2 (ColorNormalizationMode), alpha_mode 0..3 (AlphaNormalizationMode, BC3 only; BC2's explicit alpha
 * is never touched).  With every mode None the call IS the plain transform: same kernels, same launches, same bytes.
 * Settings: decorrelation_mode 0..3 and the endpoint splits, as in dxtlt_transform_bcN_with_settings.
 * `len` a multiple of 16; any pointer alignment; any block count, 0 included.  A mode or decorrelation mode out of range, a
 * NULL pointer with len > 0 and -- unlike the plain transforms, which answer DXTLT_E_INVALID_LENGTH -- a len that is no
 * multiple of 16 are all answered with DXTLT_E_INVALID_ARGUMENT and a dxtlt_last_error() text, before any device work.
 *
 * A lane normalises its 16-byte block in registers between the load and the LDS scatter, so the call moves the plain
 * transform's 2 * len bytes (normalize_blocks into a scratch buffer followed by the transform: 4 * len, and two launches).
 * The modes are a wave-uniform kernel argument, one extra kernel set per (format, decorrelation mode, splits): 8 for BC2,
 * 16 for BC3.  The device calls are asynchronous on `hip_stream`, use no scratch memory and can be captured into a HIP graph
 * (one kernel node, or two when aligned tiles are followed by an edge tile; a single branch).  The host calls take the
 * library's common host paths: mapped staging up to 1 MiB, one upload / launch / download above, the chunked pipeline from
 * 96 MiB.
 *
 * Resources on gfx950 (compiler's resource report; plain forward kernel of the same settings in parentheses; default
 * settings, 256 lanes; scratch is 0 everywhere; the full table for all 24 sets: profiles/normalize_fused_bc23_isa.txt):
 *
 *   kernel                         VGPRs        LDS bytes      waves / SIMD    scratch
 *   BC2 aligned tile               17 (13)      4096 (4096)    8 (8)           0 (0)
 *   BC2 halo tile, natural         21 (18)      5504 (5504)    8 (8)           0 (0)
 *   BC2 halo tile, generic         21 (16)      5504 (5504)    8 (8)           0 (0)
 *   BC3 aligned tile               31 (17)      4096 (4096)    8 (8)           0 (0)
 *   BC3 halo tile, natural         36 (24)      5504 (5504)    8 (8)           0 (0)
 *   BC3 halo tile, generic         36 (16)      5504 (5504)    8 (8)           0 (0)
 *
 * The occupancy is that of the plain kernels in all 72 new kernels (64 VGPRs would still give 8 waves per SIMD); what the
 * kernels add is instructions: the classification of the colour half (a few compares; a 565 round trip for blocks whose
 * indices are all 2 or all 3) and, BC3, of the alpha half, whose one long path is the sixteen-index walk for neighbouring
 * alpha endpoints (uniform_alpha_bc3, bc23_normalize.h).
 * Measured (4 GiB, three processes per cell, profiles/normalize_fused_bc23_bench.json; fraction of the 8 TB/s peak on
 * 2 * len): BC2 0.84 aligned and 0.82-0.83 at 2^k + 1 blocks, the plain transform's rate; BC3 0.69-0.75 and 0.54-0.60 against
 * the plain transform's 0.82-0.84 and 0.81-0.82 -- a larger gap than BC1's (0.84 against 0.84-0.86), and its cause is in the
 * instruction column, not the occupancy column: the BC3 kernels are 2.0-3.2 x the plain kernels' instructions, and in the
 * halo tiles the first wave normalises a second vector, the halo.  normalize_blocks + transform reaches 0.37-0.42 per cell.
 *
 * transform_bc2_auto_with_normalization and transform_bc3_auto_with_normalization, host and device: dxtlt_auto_normalize.h
 * (upstream has no BC3 one; its 12 x 16 candidates are sums over 8 alpha and 24 colour sections, so no brute force is made).
 * Many device buffers per call: dxtlt_transform_batch_with_normalize_blocks_device (dxtlt_batch_normalize.h).  Out of scope:
 * normalisation in the sharded, host-batch and DDS calls; the stand-alone normalisers above and the inverse kernels are unchanged.
 */
int32_t dxtlt_transform_bc2_with_normalize_blocks(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len,
                                                  uint8_t color_mode, uint8_t decorrelation_mode,
                                                  bool split_colour_endpoints);
int32_t dxtlt_transform_bc2_with_normalize_blocks_device(const void *d_input, void *d_output, size_t len,
                                                         uint8_t color_mode, uint8_t decorrelation_mode,
                                                         bool split_colour_endpoints, void *hip_stream);
int32_t dxtlt_transform_bc3_with_normalize_blocks(const uint8_t *input_ptr, uint8_t *output_ptr, size_t len,
                                                  uint8_t alpha_mode, uint8_t color_mode, uint8_t decorrelation_mode,
                                                  bool split_alpha_endpoints, bool split_colour_endpoints);
int32_t dxtlt_transform_bc3_with_normalize_blocks_device(const void *d_input, void *d_output, size_t len,
                                                         uint8_t alpha_mode, uint8_t color_mode,
                                                         uint8_t decorrelation_mode, bool split_alpha_endpoints,
                                                         bool split_colour_endpoints, void *hip_stream);

#ifdef __cplusplus
}
#endif
#endif
