// granule_launch.h -- internal launch interface of the granule-sorted field splits: BC7, version 2 (docs/BC7_FORMAT.md),
// and BC6H, layout version 1 (docs/BC6H_FORMAT.md).  The two formats share the granule, the streams and the batch table,
// and differ only in the record inside a block; `format` picks the kernels: 7 = BC7, 6 = BC6H.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include "bc7_fields.h"   // kGranule

namespace dxtlt {

namespace granule {

constexpr int kT = bc7::kGranule;     // blocks per granule

inline bool is_granule_format(int format) { return format == 7 || format == 6; }
const char* format_name(int format);     // "BC7" / "BC6H": the format in error texts
const char* format_symbol(int format);   // "bc7" / "bc6h": the format in the C ABI's function names
// `before` + format_name(format) + `after`: an error text, in a buffer of the calling thread (valid until its next call)
const char* named(int format, const char* before, const char* after);

// The eight streams of a transformed buffer's main part (its whole granules, N blocks): stream s starts at byte
// kStreamOff[s] * N and holds kStreamWidth[s] bytes per block (Q8, Q2, B0..B4, F; docs/BC7_FORMAT.md).  The tail part
// (N blocks onwards) is a buffer of its own behind them.  Host-side placement only: the kernels have their own constants.
constexpr int kStreams = 8;
constexpr uint64_t kStreamOff[kStreams] = {0, 8, 10, 11, 12, 13, 14, 15};
constexpr uint64_t kStreamWidth[kStreams] = {8, 2, 1, 1, 1, 1, 1, 1};

// Whole buffer.  Forward: src = blocks, dst = transformed; inverse: the other way round.  Device pointers of any alignment
// (16-byte aligned ones are the fast case).  One or two kernels on `stream`, no workspace, no synchronisation.
hipError_t launch(int format, bool inverse, const void* src, void* dst, uint64_t n_blocks, hipStream_t stream);

// One block range of an array of `total_blocks` blocks.  The AoS-side pointer is the range's first block, the SoA-side
// pointer byte 0 of the WHOLE transformed buffer.  first_block must be a multiple of the sort granule (1024) and the
// range must end on one or at the end of the array (hipErrorInvalidValue otherwise).
hipError_t launch_range(int format, bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block,
                        uint64_t num_blocks, hipStream_t stream);

// The plan of ANY block range [first, end), first < end <= total_blocks, of a transformed buffer -- what the fused image decoders
// of both formats launch and what their batch and debug plans record: one launch over the main part's granules first / 1024 ..
// (min(end, main_blocks) - 1) / 1024, split at 2^21 granules (a launch of 2^32 or more threads is refused), then the tail part's
// launch if the range reaches it.  launch(first granule, granules, tail) enqueues one; the tail part is granule
// main_blocks / 1024.  Host arithmetic only.
template <typename LAUNCH>
hipError_t for_each_range_launch(uint64_t total_blocks, uint64_t first, uint64_t end, const LAUNCH& launch)
{
    constexpr uint64_t kMaxGranules = 1ull << 21;
    const uint64_t main_blocks = total_blocks - total_blocks % kT;
    if (first < main_blocks) {
        const uint64_t g0 = first / kT, g1 = ((end < main_blocks ? end : main_blocks) - 1) / kT;
        for (uint64_t g = g0; g <= g1; g += kMaxGranules) {
            const uint64_t ng = g1 + 1 - g < kMaxGranules ? g1 + 1 - g : kMaxGranules;
            if (hipError_t e = launch(g, ng, false); e != hipSuccess)
                return e;
        }
    }
    return end > main_blocks ? launch(main_blocks / kT, (uint64_t)1, true) : hipSuccess;
}

// Many buffers per launch.  One entry per buffer with full granules (src / dst: the buffer's first byte on both sides;
// first_wg: its first workgroup in the granule launch, entries in ascending order) and one per buffer with a tail part
// (src / dst: the tail part's first byte on both sides).  `d_coarse[k]` = the entry that owns workgroup 64 k.
struct BatchEntry {
    const uint8_t* src;
    uint8_t* dst;
    uint64_t main_blocks;   // blocks of the main part (a multiple of 1024)
    uint32_t first_wg;
    uint32_t tail;          // blocks of the tail part (tail entries)
};
hipError_t launch_batch(int format, bool inverse, const BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);

}  // namespace granule

// What the calls above dispatch to: each format's kernels file (bc7_kernels.hip, bc6h_kernels.hip) defines these two.
namespace bc7 {
hipError_t launch_range(bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks,
                        hipStream_t stream);
hipError_t launch_batch(bool inverse, const granule::BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const granule::BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);
}  // namespace bc7
namespace bc6h {
hipError_t launch_range(bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks,
                        hipStream_t stream);
hipError_t launch_batch(bool inverse, const granule::BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const granule::BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream);
}  // namespace bc6h

}  // namespace dxtlt
