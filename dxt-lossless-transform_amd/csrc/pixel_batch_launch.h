// pixel_batch_launch.h -- internal launch interface of the batched uncompressed-pixel kernels (pixel_batch_kernels.hip): many
// buffers of one (pixel_bytes, direction, decorrelate, layout) class in ONE launch, and the candidates of the batched pixel auto
// transform for many buffers of one pixel_bytes in ONE launch.  docs/PIXEL_FORMAT.md, "Many buffers in one call".
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace dxtlt {
namespace pixels {

// One buffer of a launch, in workgroup order: workgroups [first_wg, end_wg) run its tiles of 4096 pixels in order, the last one
// the short tile when `total` is no multiple of 4096.  end_wg is dword 7, as batch_lookup.h reads it.  For a candidate launch
// `dst` is the buffer's slice of the arena (candidate i at dst + i * total * pixel_bytes).  No empty buffers: end_wg > first_wg.
struct PixelBatchEntry {
    const uint8_t* src;
    uint8_t* dst;
    uint64_t total;      // pixels
    uint32_t first_wg;
    uint32_t end_wg;     // first_wg + ceil(total / 4096) = the next buffer's first_wg
};
static_assert(sizeof(PixelBatchEntry) == 32 && offsetof(PixelBatchEntry, end_wg) == 28, "PixelBatchEntry layout is shared between host and device");

// One launch holds fewer than 2^24 workgroups, the limit of the BC1-BC5 batch launch (launch_batch, bcn_launch.h): 256 GiB of
// 4-byte pixels, 192 GiB of 3-byte pixels per class.
constexpr uint32_t kPixelBatchMaxWorkgroups = 0xFFFFFFu;

// d_entries / d_index: device copies of the entries and of their workgroup index (build_batch_index over the entries' end_wg:
// base[] then delta[]; wide_index = its return value); total_wgs = the last entry's end_wg.  Every buffer takes any alignment of
// both pointers and any `total`, exactly as launch_range.  Enqueues on `stream`; hipErrorInvalidValue for a class the kernels do
// not have or more than kPixelBatchMaxWorkgroups workgroups.
hipError_t launch_pixel_batch(int pixel_bytes, bool inverse, bool decorrelate, int layout, const PixelBatchEntry* d_entries,
                              const uint8_t* d_index, uint32_t n_entries, uint32_t total_wgs, bool wide_index, hipStream_t stream);

// The five candidates of launch_auto_candidates (pixel_launch.h) for every buffer of the table, each into its own `dst`; `src` at
// any alignment.
hipError_t launch_pixel_batch_candidates(int pixel_bytes, const PixelBatchEntry* d_entries, const uint8_t* d_index, uint32_t n_entries,
                                         uint32_t total_wgs, bool wide_index, hipStream_t stream);

}  // namespace pixels
}  // namespace dxtlt
