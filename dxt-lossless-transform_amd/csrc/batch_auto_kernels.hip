// batch_auto_kernels.hip -- dxtlt_transform_batch_auto_device, candidate phase: every endpoint section the size estimator will be
// shown, for MANY buffers of one format and search depth in one launch.
//
// auto_kernels.hip does this for one buffer per launch; a texture of a few MiB is a few hundred workgroups for 256 CUs and the
// launch costs the host longer than the kernel runs.  Here the buffers' workgroups lie end to end: a workgroup finds its buffer
// in a table in device memory (input pointer, offset of the buffer's slice of the arena, block count, first workgroup) by a
// uniform bisection over first_wg -- scalar loads and compares -- and then runs the lane body auto_candidates_kernel runs
// (auto_candidate_lanes.h): one 16-byte vector per lane (two BC1 / BC4 blocks or one BC2 / BC3 / BC5 block), SWAR YCoCg-R, no LDS,
// every section written with wave-contiguous stores.  Per buffer the slice is laid out as the single-buffer arena is (auto_launch.h,
// auto_sections); BC4 and BC5, for which the single-buffer call runs two full transforms instead, get BC3's alpha-endpoint code:
//     BC4         [endpoint pairs 2N][endpoints split 2N]
//     BC5         [red pairs 2N][red split 2N][green pairs 2N][green split 2N]
// What the single-buffer path leaves to other launches is handled here, per workgroup and uniformly:
//   * the odd last block of a BC1 / BC4 buffer (half a vector) belongs to the lane behind the last whole vector;
//   * a buffer whose input is off a 16-byte boundary is read with dword loads (off a 4-byte boundary: byte loads) of the two
//     dwords of a vector that hold endpoints -- slower, the same bytes out.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "auto_candidate_lanes.h"
#include "auto_launch.h"
#include "bcn_launch.h"
#include "launch_grid.h"

namespace dxtlt {

namespace {

// (a pointer out of a table in memory is generic to the compiler: the address space is restored for global_load)
typedef const uint8_t __attribute__((address_space(1))) * GlobalBytes;
typedef const uint32_t __attribute__((address_space(1))) * GlobalDword;
typedef const u32x4 __attribute__((address_space(1))) * GlobalVec;

// one dword at p, whose address is `misalign` (mod 4, uniform) off a dword boundary
__device__ __forceinline__ uint32_t load_dword_any(GlobalBytes p, uint32_t misalign)
{
    if (misalign == 0)
        return *reinterpret_cast<GlobalDword>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

template <int FMT, bool ALL>
__global__ void __launch_bounds__(256)
batch_auto_candidates_kernel(const BatchAutoEntry* __restrict__ tab, uint32_t entries, uint32_t total_wgs, uint8_t* __restrict__ arena_base)
{
    const uint64_t wg64 = workgroup_index();
    if (wg64 >= total_wgs)
        return;
    const uint32_t wg = (uint32_t)wg64;
    uint32_t lo = 0, hi = entries - 1;   // the last entry whose first_wg is not above wg
    while (lo < hi) {
        const uint32_t mid = (lo + hi + 1) >> 1;
        if (tab[mid].first_wg <= wg)
            lo = mid;
        else
            hi = mid - 1;
    }
    const GlobalBytes in = reinterpret_cast<GlobalBytes>(reinterpret_cast<uintptr_t>(tab[lo].src));
    const uint64_t n = tab[lo].blocks;
    uint8_t* __restrict__ arena = arena_base + tab[lo].arena_off;
    const uint64_t v = uint64_t(wg - tab[lo].first_wg) * 256 + threadIdx.x;

    constexpr bool kTwoBlocks = FMT == kBc1 || FMT == kBc4;   // blocks per 16-byte vector
    const uint64_t vectors = kTwoBlocks ? n / 2 : n;
    const bool half = kTwoBlocks && (n & 1) != 0 && v == vectors;   // the odd last block: the first half of a vector
    if (v >= vectors && !half)
        return;

    // the two dwords of the vector that hold endpoints: x (bytes 0-3) and z (bytes 8-11)
    const uint32_t misalign = uint32_t(reinterpret_cast<uintptr_t>(in) & 15);
    const GlobalBytes p = in + 16 * v;
    uint32_t x, z = 0;
    if (misalign == 0 && !half) {
        const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<GlobalVec>(p));
        x = q.x;
        z = q.z;
    } else {
        x = load_dword_any(p, misalign & 3);
        if (!half)
            z = load_dword_any(p + 8, misalign & 3);
    }

    candidate_lane<FMT, ALL, true>(arena, n, v, x, z, half);
}

}  // namespace

hipError_t launch_batch_auto_candidates(Format fmt, bool all_variants, const BatchAutoEntry* d_table, uint32_t entries,
                                        uint32_t total_wgs, void* d_arena, hipStream_t stream)
{
    if (entries == 0 || total_wgs == 0)
        return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(d_arena) & 15) != 0)
        return hipErrorInvalidValue;
    dim3 grid;
    if (hipError_t e = grid_rows((uint64_t)total_wgs * 256, 256, grid); e != hipSuccess)
        return e;
    uint8_t* arena = static_cast<uint8_t*>(d_arena);
#define DXTLT_BATCH_AUTO_LAUNCH(F, A) \
    hipLaunchKernelGGL((batch_auto_candidates_kernel<F, A>), grid, dim3(256), 0, stream, d_table, entries, total_wgs, arena)
    switch (fmt) {
    case kBc1: if (all_variants) DXTLT_BATCH_AUTO_LAUNCH(kBc1, true); else DXTLT_BATCH_AUTO_LAUNCH(kBc1, false); break;
    case kBc2: if (all_variants) DXTLT_BATCH_AUTO_LAUNCH(kBc2, true); else DXTLT_BATCH_AUTO_LAUNCH(kBc2, false); break;
    case kBc3: if (all_variants) DXTLT_BATCH_AUTO_LAUNCH(kBc3, true); else DXTLT_BATCH_AUTO_LAUNCH(kBc3, false); break;
    case kBc4: DXTLT_BATCH_AUTO_LAUNCH(kBc4, false); break;
    default: DXTLT_BATCH_AUTO_LAUNCH(kBc5, false); break;
    }
#undef DXTLT_BATCH_AUTO_LAUNCH
    return hipGetLastError();
}

}  // namespace dxtlt
