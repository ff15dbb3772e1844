// auto_launch.h -- internal interface of the candidate kernels of transform_bcN_auto (auto_kernels.hip, batch_auto_kernels.hip):
// the layout they write and their launches.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "bcn_launch.h"

namespace dxtlt {

// ONE layout for what a candidate kernel writes for a buffer of N blocks -- the single-buffer arena and a batch item's slice
// alike -- and ONE list of it: the distinct sections the candidates of (fmt, all_variants) show the estimator, in memory order
//     BC3         [alpha pairs 2N][alpha split 2N], then the colour sections
//     BC1 - BC3   per YCoCg-R variant (None, Variant1; with all_variants also Variant2, Variant3): [colour pairs 4N][colour split 4N]
//     BC4         [endpoint pairs 2N][endpoints split 2N]
//     BC5         [red pairs 2N][red split 2N][green pairs 2N][green split 2N]
// The sections lie end to end: `bytes` is the arena / slice size.  all_variants is ignored for BC4 / BC5.  (auto_transform.cpp)
struct AutoSections {
    int count;   // at most 10
    uint64_t bytes;
    uint64_t off[10], len[10];
};
// (this and batch_auto_workgroups are defined here, inline and pure: the planner that calls them also runs stand-alone under the
// host sanitizers)
inline AutoSections auto_sections(Format fmt, bool all_variants, uint64_t blocks)
{
    AutoSections s{};
    auto add = [&](int sections, uint64_t bytes_per_block) {
        for (int k = 0; k < sections; ++k) {
            s.off[s.count] = s.bytes;
            s.len[s.count++] = bytes_per_block * blocks;
            s.bytes += bytes_per_block * blocks;
        }
    };
    if (fmt == kBc4 || fmt == kBc5)
        add(fmt == kBc5 ? 4 : 2, 2);
    else {
        if (fmt == kBc3)
            add(2, 2);
        add(all_variants ? 8 : 4, 4);
    }
    return s;
}
// One read of d_in (the AoS blocks, 16-byte aligned) -> every section of BC1 - BC3, at d_arena.  Enqueues on `stream`.
hipError_t launch_auto_candidates(Format fmt, bool all_variants, const void* d_in, void* d_arena, uint64_t blocks,
                                  hipStream_t stream);

// ---- the candidate kernel of transform_bcN_auto_with_normalization, BC1 - BC3 (auto_normalize_kernels.hip) --------------------
// One section list for the three formats: BC1 / BC2 fill 12 or 24 entries, BC3 20 or 32.
struct AutoNormalizeSections {
    int count;
    uint64_t bytes;
    uint64_t off[32], len[32];
};
// BC1 / BC2.
// Three copies of the colour part of auto_sections, one per colour normalisation the candidates are estimated on:
//     for norm in (None*, Color0Only, ReplicateColor):
//         for variant in (None, Variant1[, Variant2, Variant3]):  [colour pairs 4N][colour split 4N]
// None*: BC1 with its fully transparent blocks rewritten to 0xFF (kNormTransparentOnly), BC2 the input's own colours.  12 or 24
// sections end to end, 48 or 96 bytes per block; section (norm, variant, split) has index norm * (count / 3) + 2 * variant + split.
inline AutoNormalizeSections auto_normalize_sections(bool all_variants, uint64_t blocks)
{
    AutoNormalizeSections s{};
    s.count = all_variants ? 24 : 12;
    for (int k = 0; k < s.count; ++k) {
        s.off[k] = s.bytes;
        s.len[k] = 4 * blocks;
        s.bytes += 4 * blocks;
    }
    return s;
}
// BC3 (dxtlt_transform_bc3_auto_with_normalization): the alpha half and the colour half of a block are normalised independently,
// so a candidate's two shown sections come from two small families --
//     for alpha_mode in 0..3:            [alpha pairs 2N][alpha split: first endpoints N, second endpoints N]
//     for colour_mode in 0..2:
//         for variant in (None, Variant1[, Variant2, Variant3]):  [colour pairs 4N][colour split 4N]
// 8 alpha sections of 2N bytes, index 2 * alpha_mode + split_alpha, then 12 or 24 colour sections of 4N bytes, index
// 8 + colour_mode * 2 * variants + 2 * variant + split_colour: 20 or 32 sections end to end, 64 or 112 bytes per block.  The colour
// part starts at 16N and is auto_normalize_sections' arena byte for byte.  The section index is also the estimate counter.
constexpr int kBc3AlphaSections = 8;
inline AutoNormalizeSections auto_normalize_bc3_sections(bool all_variants, uint64_t blocks)
{
    AutoNormalizeSections s{};
    s.count = kBc3AlphaSections + (all_variants ? 24 : 12);
    for (int k = 0; k < s.count; ++k) {
        s.off[k] = s.bytes;
        s.len[k] = (k < kBc3AlphaSections ? 2 : 4) * blocks;
        s.bytes += s.len[k];
    }
    return s;
}
// One read of d_in (the AoS blocks of BC1, BC2 or BC3, 16-byte aligned) -> every section, at d_arena (16-byte aligned).  Enqueues on
// `stream`; *launches (optional) receives the number of kernels enqueued: BC1's odd last block is a launch of its own.
hipError_t launch_auto_normalize_candidates(Format fmt, bool all_variants, const void* d_in, void* d_arena, uint64_t blocks,
                                            hipStream_t stream, int* launches);
// Read-only: *d_any (a device uint32 the caller has zeroed) = 1 when the colour half of any BC2 block is a normalisable solid
// (solid_colour_4c); the twin of launch_bc1_any_normalizable.  Any alignment of `in`.
hipError_t launch_bc2_any_normalizable(const void* in, uint64_t num_blocks, uint32_t* d_any, hipStream_t stream);
// The same for BC3: 1 when the alpha half of any block is uniform (uniform_alpha_bc3) or its colour half a normalisable solid
// (solid_colour_4c); the twin of launch_bc2_any_normalizable.  Any alignment of `in`.
hipError_t launch_bc3_any_normalizable(const void* in, uint64_t num_blocks, uint32_t* d_any, hipStream_t stream);

// ---- the batched candidate kernel of dxtlt_transform_batch_auto_device (batch_auto_kernels.hip) -------------------------------
// One entry per non-empty buffer of a launch, in workgroup order: entry e owns workgroups [first_wg, next entry's first_wg).
struct BatchAutoEntry {
    const uint8_t* src;   // the AoS blocks, any alignment
    uint64_t arena_off;   // of the buffer's slice (auto_sections) inside the arena, a multiple of 16
    uint64_t blocks;
    uint32_t first_wg;
    uint32_t reserved;
};
static_assert(sizeof(BatchAutoEntry) == 32, "BatchAutoEntry layout is shared between host and device");

// workgroups a buffer owns in the launch: one lane per 16-byte vector, the odd last block of BC1 / BC4 included
inline uint32_t batch_auto_workgroups(Format fmt, uint64_t blocks)
{
    const uint64_t lanes = fmt == kBc1 || fmt == kBc4 ? (blocks + 1) / 2 : blocks;
    return (uint32_t)((lanes + 255) / 256);
}
// One read of every buffer of the table (device memory, `entries` entries, total_wgs = workgroups of all of them) -> every
// section, at d_arena + arena_off.  fmt 1..5; all_variants is ignored for BC4 / BC5.  Enqueues on `stream`.
hipError_t launch_batch_auto_candidates(Format fmt, bool all_variants, const BatchAutoEntry* d_table, uint32_t entries,
                                        uint32_t total_wgs, void* d_arena, hipStream_t stream);

}  // namespace dxtlt
