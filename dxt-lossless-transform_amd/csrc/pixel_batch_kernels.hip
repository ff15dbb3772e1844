// pixel_batch_kernels.hip -- the uncompressed-pixel kernels for MANY buffers in one launch (dxtlt_transform_pixels_batch_device,
// dxtlt_transform_pixels_batch_auto_device; docs/PIXEL_FORMAT.md, "Many buffers in one call").
//
// A 256 x 256 mip chain is 22 tiles; a launch of its own puts 22 workgroups on 256 CUs and costs the host more than the kernel
// runs.  Here the buffers of one class lie end to end in one grid: one workgroup of 256 lanes still runs one tile of 4096 pixels of
// one buffer, finds that buffer through the batch transform's lookup (batch_lookup.h: two-level index, wide form, bisection over
// end_wg) in a table of 32-byte entries in device memory, and then runs the tile of the single-buffer kernels
// (pixel_tile_body.h) with first = 0, num = total.  Tiles keep launch order inside a buffer (no rotation over the XCDs: a short
// tile is less work than a whole one here, not more).  Any alignment of either pointer and any pixel count, as in the single
// kernels: the 16-byte vectors fall where they fall, only a buffer's last, short tile moves bytes one at a time, and no byte
// outside a buffer's own is touched.
#include <hip/hip_runtime.h>

#include "batch_lookup.h"
#include "bcn_launch.h"
#include "pixel_batch_launch.h"
#include "pixel_tile_body.h"

namespace dxtlt {
namespace pixels {

// An entry as the workgroup sees it (BatchView, batch_kernels.hip): scalar dword loads, and the buffer pointers tagged as global
// memory again -- a pointer loaded from memory is a generic one to the compiler, which would make every access of the tile flat_*.
typedef const __attribute__((address_space(1))) uint8_t* global_cptr;
typedef __attribute__((address_space(1))) uint8_t* global_ptr;

struct PixelBatchView {
    const uint8_t* src;
    uint8_t* dst;
    uint64_t total;
    uint32_t first_wg, end_wg;
};

__device__ __forceinline__ PixelBatchView load_batch_entry(const PixelBatchEntry* entry)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(entry);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(entry);
    PixelBatchView v;
    v.src = (const uint8_t*)(global_cptr)q[0];
    v.dst = (uint8_t*)(global_ptr)q[1];
    v.total = q[2];
    v.first_wg = w[6];
    v.end_wg = w[7];
    return v;
}
__device__ __forceinline__ void pin_batch_view(PixelBatchView& v)
{
    uint64_t s = reinterpret_cast<uintptr_t>(v.src), d = reinterpret_cast<uintptr_t>(v.dst);
    asm("" : "+s"(s), "+s"(d), "+s"(v.total), "+s"(v.first_wg), "+s"(v.end_wg));
    v.src = (const uint8_t*)(global_cptr)s;
    v.dst = (uint8_t*)(global_ptr)d;
}
static_assert(offsetof(PixelBatchEntry, dst) == 8 && offsetof(PixelBatchEntry, total) == 16 && offsetof(PixelBatchEntry, first_wg) == 24 &&
                  offsetof(PixelBatchEntry, end_wg) == 28,
              "load_batch_entry reads PixelBatchEntry by dword offsets");

namespace {

// the entry of workgroup blockIdx.x; both table pointers in the first scalar round trip, through integers (batch_kernel)
__device__ __forceinline__ PixelBatchView entry_of_this_workgroup(const PixelBatchEntry* entries_arg, const uint8_t* index_arg, uint32_t n_base,
                                                                  uint32_t n_entries)
{
    uint64_t entries_at = reinterpret_cast<uintptr_t>(entries_arg), index_at = reinterpret_cast<uintptr_t>(index_arg);
    asm("" : "+s"(entries_at), "+s"(index_at), "+s"(n_base), "+s"(n_entries));
    const PixelBatchEntry* entries = (const PixelBatchEntry*)(const __attribute__((address_space(1))) PixelBatchEntry*)entries_at;
    const uint8_t* index = (const uint8_t*)(global_cptr)index_at;
    PixelBatchView en;
    (void)batch_entry_of_workgroup(entries, index, n_base, n_entries, blockIdx.x, en);
    return en;
}

template <int B, bool INVERSE, bool DECORRELATE, int LAYOUT>
__global__ void __launch_bounds__(kThreads)
pixel_batch_tiles(const PixelBatchEntry* __restrict__ entries, const uint8_t* __restrict__ index, uint32_t n_base, uint32_t n_entries)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[B * kTile];
    __shared__ uint32_t wave_totals[kThreads / 64];
    const PixelBatchView en = entry_of_this_workgroup(entries, index, n_base, n_entries);
    const uint32_t tile = blockIdx.x - en.first_wg;   // < end_wg - first_wg = ceil(total / kTile): the tile exists
    DXTLT_PIXEL_TILE(en.src, en.dst, en.total, 0, en.total, tile);
}

template <int B>
__global__ void __launch_bounds__(kThreads)
pixel_batch_candidates(const PixelBatchEntry* __restrict__ entries, const uint8_t* __restrict__ index, uint32_t n_base, uint32_t n_entries)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[B * kTile];
    const PixelBatchView en = entry_of_this_workgroup(entries, index, n_base, n_entries);
    const uint32_t tile = blockIdx.x - en.first_wg;
    DXTLT_PIXEL_CANDIDATES_TILE(en.src, en.dst, en.total, tile);
}

using BatchFn = void (*)(const PixelBatchEntry*, const uint8_t*, uint32_t, uint32_t);

template <int B, bool INVERSE, bool DECORRELATE>
BatchFn batch_layout(int layout)
{
    switch (layout) {
    case kInterleaved: return pixel_batch_tiles<B, INVERSE, DECORRELATE, kInterleaved>;
    case kPlanar: return pixel_batch_tiles<B, INVERSE, DECORRELATE, kPlanar>;
    case kPlanarDelta: return pixel_batch_tiles<B, INVERSE, DECORRELATE, kPlanarDelta>;
    default: return nullptr;
    }
}

template <int B>
BatchFn batch_bytes(bool inverse, bool decorrelate, int layout)
{
    if (inverse)
        return decorrelate ? batch_layout<B, true, true>(layout) : batch_layout<B, true, false>(layout);
    return decorrelate ? batch_layout<B, false, true>(layout) : batch_layout<B, false, false>(layout);
}

hipError_t launch(BatchFn k, const PixelBatchEntry* d_entries, const uint8_t* d_index, uint32_t n_entries, uint32_t total_wgs, bool wide_index,
                  hipStream_t stream)
{
    if (k == nullptr || d_entries == nullptr || d_index == nullptr || total_wgs > kPixelBatchMaxWorkgroups)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k, dim3(total_wgs), dim3(kThreads), 0, stream, d_entries, d_index,
                       (uint32_t)batch_index_base_count(total_wgs) | (wide_index ? 0x80000000u : 0u), n_entries);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_pixel_batch(int pixel_bytes, bool inverse, bool decorrelate, int layout, const PixelBatchEntry* d_entries,
                              const uint8_t* d_index, uint32_t n_entries, uint32_t total_wgs, bool wide_index, hipStream_t stream)
{
    if (n_entries == 0 || total_wgs == 0)
        return hipSuccess;
    if (pixel_bytes != 3 && pixel_bytes != 4)
        return hipErrorInvalidValue;
    return launch(pixel_bytes == 4 ? batch_bytes<4>(inverse, decorrelate, layout) : batch_bytes<3>(inverse, decorrelate, layout), d_entries,
                  d_index, n_entries, total_wgs, wide_index, stream);
}

hipError_t launch_pixel_batch_candidates(int pixel_bytes, const PixelBatchEntry* d_entries, const uint8_t* d_index, uint32_t n_entries,
                                         uint32_t total_wgs, bool wide_index, hipStream_t stream)
{
    if (n_entries == 0 || total_wgs == 0)
        return hipSuccess;
    if (pixel_bytes != 3 && pixel_bytes != 4)
        return hipErrorInvalidValue;
    return launch(pixel_bytes == 4 ? (BatchFn)pixel_batch_candidates<4> : (BatchFn)pixel_batch_candidates<3>, d_entries, d_index, n_entries,
                  total_wgs, wide_index, stream);
}

}  // namespace pixels
}  // namespace dxtlt
