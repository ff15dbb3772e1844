// image_batch_kernels.hip -- the images of MANY transformed buffers of one format and settings in ONE launch
// (dxtlt_untransform_decode_images_batch_device; docs/IMAGE_DECODE.md, "Many buffers in one call").
//
// The inverse half of batch_kernel (batch_kernels.hip) with the region sinks of the image-region kernels
// (image_region_sinks.h) in the place of the block store: every workgroup finds its entry -- a group of up to sixteen regions
// of one buffer, planned as ONE range of the inverse transform -- through the batch transform's own lookup (batch_lookup.h:
// two-level index, wide form, bisection, tiles rotated over the XCDs) and runs one tile of the range: aligned, shifted or the
// edge tile.  A whole 256 x 256 mip chain is 43 KiB, 5-6 us through a launch of its own, and that is the price of the launch:
// here 8000 of them are one launch.
//
// The region table of an entry lives in device memory beside the entries (image_batch_launch.h: one 64-byte record per
// region), not in the kernel arguments; DeviceRegionTable (device_region_table.h) reads it for the lookups of image_regions.h
// with scalar loads only.
#include <cstring>

#include "bcn_device.h"

#include "batch_lookup.h"
#include "device_region_table.h"
#include "image_batch_launch.h"
#include "image_region_sinks.h"

namespace dxtlt {
namespace {

using BatchPixelSink = RegionPixelSinkOf<DeviceRegionTable>;
using BatchChannelSink = RegionChannelSinkOf<DeviceRegionTable>;

}  // namespace

// An entry as the workgroup sees it, as BatchView (batch_kernels.hip): scalar loads, the buffer pointer tagged as global memory
struct ImageBatchView {
    const uint8_t* src;
    uint64_t regions_at;
    uint64_t total_blocks;
    uint32_t first_wg, end_wg, full_tiles;
    uint32_t flags;       // form | region_count << 8 | natural << 16
    uint32_t shifts[2];   // shift[0..3], shift[4..5]
    uint64_t gbase[6];
    uint64_t first_block, range_blocks;
};

__device__ __forceinline__ ImageBatchView load_batch_entry(const ImageBatchEntry* entry)
{
    const uint64_t* q = reinterpret_cast<const uint64_t*>(entry);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(entry);
    ImageBatchView v;
    v.src = (const uint8_t*)(global_cptr)q[0];
    v.regions_at = q[1];
    v.total_blocks = q[2];
    v.first_wg = w[6];
    v.end_wg = w[7];
    v.full_tiles = w[8];
    v.flags = w[9];
    v.shifts[0] = w[10];
    v.shifts[1] = w[11];
#pragma unroll
    for (int i = 0; i < 6; ++i)
        v.gbase[i] = q[6 + i];
    v.first_block = q[12];
    v.range_blocks = q[13];
    return v;
}
__device__ __forceinline__ void pin_batch_view(ImageBatchView& v)
{
    uint64_t s = reinterpret_cast<uintptr_t>(v.src);
    asm("" : "+s"(s), "+s"(v.regions_at), "+s"(v.total_blocks));
    v.src = (const uint8_t*)(global_cptr)s;
    asm("" : "+s"(v.first_wg), "+s"(v.end_wg), "+s"(v.full_tiles), "+s"(v.flags), "+s"(v.shifts[0]), "+s"(v.shifts[1]));
#pragma unroll
    for (int i = 0; i < 6; ++i)
        asm("" : "+s"(v.gbase[i]));
    asm("" : "+s"(v.first_block), "+s"(v.range_blocks));
}
static_assert(offsetof(ImageBatchEntry, first_wg) == 24 && offsetof(ImageBatchEntry, end_wg) == 28 && offsetof(ImageBatchEntry, full_tiles) == 32 &&
                  offsetof(ImageBatchEntry, form) == 36 && offsetof(ImageBatchEntry, shift) == 40 && offsetof(ImageBatchEntry, gbase) == 48 &&
                  offsetof(ImageBatchEntry, first_block) == 96 && offsetof(ImageBatchEntry, range_blocks) == 104,
              "load_batch_entry reads ImageBatchEntry by dword offsets");

namespace {

// One tile of the workgroup's entry with the sink SINK (BatchPixelSink / BatchChannelSink); `lds`: shift_lds_bytes(1, THREADS)
template <int FMT, int VARIANT, bool SA, bool SC, int THREADS, typename SINK>
__device__ __forceinline__ void batch_image_tile(const ImageBatchEntry* entries_arg, const uint8_t* index_arg, uint32_t n_base,
                                                 uint32_t n_entries, uint8_t* lds)
{
    const uint32_t wg = blockIdx.x;
    // both table pointers in the first scalar round trip, through integers (batch_kernel)
    uint64_t entries_at = reinterpret_cast<uintptr_t>(entries_arg), index_at = reinterpret_cast<uintptr_t>(index_arg);
    asm("" : "+s"(entries_at), "+s"(index_at), "+s"(n_base), "+s"(n_entries));
    const ImageBatchEntry* entries = (const ImageBatchEntry*)(const __attribute__((address_space(1))) ImageBatchEntry*)entries_at;
    const uint8_t* index = (const uint8_t*)(global_cptr)index_at;
    ImageBatchView en;
    const uint32_t e = batch_entry_of_workgroup(entries, index, n_base, n_entries, wg, en);
    const uint32_t local = batch_rotated_tile(en.first_wg, en.end_wg, e, wg);
    // the launch's first block is block first_block of the buffer (image_region_sinks.h)
    const SINK sink{DeviceRegionTable{en.regions_at, (en.flags >> 8) & 0xFFu}, en.first_block};
    const bool aligned = (en.flags & 0xFF) == 1;
    if (aligned && local < en.full_tiles) {
        // every stream base of the range on a 128-byte line: the aligned tile, tiles in launch order
        inv_aligned_tile<FMT, VARIANT, SA, SC, THREADS, SINK>(en.src, nullptr, en.total_blocks, en.first_block, local, lds, sink);
        return;
    }
    Shifts sh;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        sh.d[i] = (int)((en.shifts[i >> 2] >> (8 * (i & 3))) & 127u);
        sh.gbase[i] = en.gbase[i];
    }
    sh.natural = 1;   // plan_image_batch_entry hands ranges with other shifts back to the host
    sh.halo_vecs = 0;
    sh.full_tiles = en.full_tiles;
    sh.range_blocks = en.range_blocks;
    // the whole tile first, with a return behind it (batch_kernel has the reason)
    if (local < en.full_tiles) {
        // neighbouring tiles share 128-byte lines: consecutive tiles stay on one XCD
        const uint64_t tile = xcd_contiguous_tile(local, en.full_tiles);
        inv_shift_tile<FMT, VARIANT, SA, SC, THREADS, SINK>(en.src, nullptr, en.total_blocks, en.first_block, sh, tile, lds, sink);
        return;
    }
    inv_shift_edge_tile<FMT, VARIANT, SA, SC, THREADS, SINK>(en.src, nullptr, en.total_blocks, sh, en.full_tiles, lds, sink);
}

template <int FMT, int VARIANT, bool SA, bool SC, int THREADS = batch_tile_threads(FMT, SC, true)>
__global__ void __launch_bounds__(THREADS)
batch_image_kernel(const ImageBatchEntry* __restrict__ entries, const uint8_t* __restrict__ index, uint32_t n_base, uint32_t n_entries)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    batch_image_tile<FMT, VARIANT, SA, SC, THREADS, BatchPixelSink>(entries, index, n_base, n_entries, lds);
}

template <int FMT, bool SA, int THREADS = batch_tile_threads(FMT, false, true)>
__global__ void __launch_bounds__(THREADS)
batch_channel_image_kernel(const ImageBatchEntry* __restrict__ entries, const uint8_t* __restrict__ index, uint32_t n_base,
                           uint32_t n_entries)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[shift_lds_bytes(1, THREADS)];
    batch_image_tile<FMT, kNone, SA, false, THREADS, BatchChannelSink>(entries, index, n_base, n_entries, lds);
}

using ImageBatchFn = void (*)(const ImageBatchEntry*, const uint8_t*, uint32_t, uint32_t);

template <int FMT, int VARIANT>
ImageBatchFn image_batch_splits(bool sa, bool sc)
{
    if constexpr (FMT == kBc3) {
        if (sa)
            return sc ? batch_image_kernel<FMT, VARIANT, true, true> : batch_image_kernel<FMT, VARIANT, true, false>;
    }
    return sc ? batch_image_kernel<FMT, VARIANT, false, true> : batch_image_kernel<FMT, VARIANT, false, false>;
}

template <int FMT>
ImageBatchFn image_batch_variant(int variant, bool sa, bool sc)
{
    switch (variant) {
    case kNone: return image_batch_splits<FMT, kNone>(sa, sc);
    case kVar1: return image_batch_splits<FMT, kVar1>(sa, sc);
    case kVar2: return image_batch_splits<FMT, kVar2>(sa, sc);
    default: return image_batch_splits<FMT, kVar3>(sa, sc);
    }
}

template <int FMT>
ImageBatchFn image_batch_channel(bool split_endpoints)
{
    return split_endpoints ? batch_channel_image_kernel<FMT, true> : batch_channel_image_kernel<FMT, false>;
}

}  // namespace

uint32_t plan_image_batch_entry(Format fmt, const Settings& s, ImageBatchEntry& e)
{
    const Settings es = effective_settings(fmt, s);
    const Streams S = make_streams(fmt, es.split_alpha, es.split_colour);
    const uint64_t T = (uint64_t)tile_blocks(fmt, batch_tile_threads(fmt, es.split_colour, true));
    const uint64_t tiles = e.range_blocks / T, rest = e.range_blocks % T;
    // The tile forms of launch_transform for the range: aligned tiles when every stream base of the range is on a 128-byte
    // line, otherwise shifted tiles (slices displaced by the base modulo 16); the edge tile takes what is left behind them.
    bool on_lines = true;
    int d[6] = {0, 0, 0, 0, 0, 0};
    for (int i = 0; i < S.n; ++i) {
        const uint64_t base = reinterpret_cast<uintptr_t>(e.src) + (uint64_t)S.off[i] * e.total_blocks + (uint64_t)S.width[i] * e.first_block;
        d[i] = (int)(base & 15);
        on_lines = on_lines && (base & 127) == 0;
    }
    if (!shifts_are_natural(S, d))
        return 0xFFFFFFFFu;
    e.form = on_lines ? 1 : 0;
    e.natural = 1;
    e.reserved = 0;
    e.reserved2[0] = e.reserved2[1] = 0;
    e.reserved3[0] = e.reserved3[1] = 0;
    for (int i = 0; i < 6; ++i) {
        e.shift[i] = (uint8_t)d[i];
        e.gbase[i] = i < S.n ? (uint64_t)S.off[i] * e.total_blocks + (uint64_t)S.width[i] * e.first_block - (uint64_t)d[i] : 0;
    }
    e.full_tiles = (uint32_t)tiles;
    const uint32_t wgs = (uint32_t)tiles + (rest != 0 ? 1u : 0u);
    e.end_wg = e.first_wg + wgs;
    return wgs;
}

hipError_t launch_image_batch(Format fmt, const Settings& s, const ImageBatchEntry* d_entries, const uint8_t* d_index,
                              uint32_t n_entries, uint32_t total_wgs, bool wide_index, hipStream_t stream)
{
    if (n_entries == 0 || total_wgs == 0)
        return hipSuccess;
    const Settings es = effective_settings(fmt, s);
    if (es.variant < 0 || es.variant > 3 || total_wgs > 0xFFFFFFu)
        return hipErrorInvalidValue;
    const bool sa = es.split_alpha, sc = es.split_colour;
    ImageBatchFn k = nullptr;
    switch (fmt) {
    case kBc1: k = image_batch_variant<kBc1>(es.variant, false, sc); break;
    case kBc2: k = image_batch_variant<kBc2>(es.variant, false, sc); break;
    case kBc3: k = image_batch_variant<kBc3>(es.variant, sa, sc); break;
    case kBc4: k = image_batch_channel<kBc4>(sa); break;
    case kBc5: k = image_batch_channel<kBc5>(sa); break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3(total_wgs), dim3(batch_tile_threads(fmt, sc, true)), 0, stream, d_entries, d_index,
                       (uint32_t)batch_index_base_count(total_wgs) | (wide_index ? 0x80000000u : 0u), n_entries);
    return hipGetLastError();
}

}  // namespace dxtlt
