// auto_launch.h -- internal interface of the fused candidate kernel of transform_bcN_auto (auto_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bcn_launch.h"

namespace dxtlt {

// Bytes of the candidate arena for `blocks` blocks: BC3's two alpha-endpoint sections (2 bytes per block each), then per
// YCoCg-R variant (None, Variant1; with all_variants also Variant2, Variant3) the colour section as pairs and split
// (4 bytes per block each).
uint64_t auto_arena_bytes(Format fmt, bool all_variants, uint64_t blocks);
// byte offset of a section inside the arena
uint64_t auto_section_offset(Format fmt, uint64_t blocks, int variant, bool split_colour);
uint64_t auto_alpha_section_offset(uint64_t blocks, bool split_alpha);   // BC3
// One read of d_in (the AoS blocks, 16-byte aligned) -> every section.  Enqueues on `stream`.
hipError_t launch_auto_candidates(Format fmt, bool all_variants, const void* d_in, void* d_arena, uint64_t blocks,
                                  hipStream_t stream);

// ---- the batched candidate kernel of dxtlt_transform_batch_auto_device (batch_auto_kernels.hip) -------------------------------
// One entry per non-empty buffer of a launch, in workgroup order: entry e owns workgroups [first_wg, next entry's first_wg).
struct BatchAutoEntry {
    const uint8_t* src;   // the AoS blocks, any alignment
    uint64_t arena_off;   // of the buffer's slice inside the arena, a multiple of 16
    uint64_t blocks;
    uint32_t first_wg;
    uint32_t reserved;
};
static_assert(sizeof(BatchAutoEntry) == 32, "BatchAutoEntry layout is shared between host and device");

// Bytes of one buffer's slice -- BC1-3: auto_arena_bytes; BC4: 4 per block, BC5: 8 per block (pairs and split endpoint sections) --
// and its distinct sections in slice order (at most 10; returns how many): BC3's alpha pairs and alpha split, then per variant
// colour pairs and colour split; BC4 pairs, split; BC5 red pairs, red split, green pairs, green split.
uint64_t batch_auto_slice_bytes(Format fmt, bool all_variants, uint64_t blocks);
int batch_auto_sections(Format fmt, bool all_variants, uint64_t blocks, uint64_t* offsets, uint64_t* lengths);
// workgroups a buffer owns in the launch: one lane per 16-byte vector, the odd last block of BC1 / BC4 included
uint32_t batch_auto_workgroups(Format fmt, uint64_t blocks);
// One read of every buffer of the table (device memory, `entries` entries, total_wgs = workgroups of all of them) -> every
// section, at d_arena + arena_off.  fmt 1..5; all_variants is ignored for BC4 / BC5.  Enqueues on `stream`.
hipError_t launch_batch_auto_candidates(Format fmt, bool all_variants, const BatchAutoEntry* d_table, uint32_t entries,
                                        uint32_t total_wgs, void* d_arena, hipStream_t stream);

}  // namespace dxtlt
