// batch_auto_kernels.hip -- dxtlt_transform_batch_auto_device, candidate phase: every endpoint section the size estimator will be
// shown, for MANY buffers of one format and search depth in one launch.
//
// auto_kernels.hip does this for one buffer per launch; a texture of a few MiB is a few hundred workgroups for 256 CUs and the
// launch costs the host longer than the kernel runs.  Here the buffers' workgroups lie end to end: a workgroup finds its buffer
// in a table in device memory (input pointer, offset of the buffer's slice of the arena, block count, first workgroup) by a
// uniform bisection over first_wg -- scalar loads and compares -- and then does what auto_candidates_kernel does: one 16-byte
// vector per lane (two BC1 / BC4 blocks or one BC2 / BC3 / BC5 block), SWAR YCoCg-R, no LDS, every section written with
// wave-contiguous stores.  Per buffer the slice is laid out as the single-buffer arena is (auto_section_offset /
// auto_alpha_section_offset):
//     BC1 / BC2   per variant (None, Variant1[, Variant2, Variant3]):  [colour pairs 4N][colour split 4N]
//     BC3         [alpha pairs 2N][alpha split 2N], then the colour sections
//     BC4         [endpoint pairs 2N][endpoints split 2N]                  -- BC3's alpha-endpoint code; the single-buffer call
//     BC5         [red pairs 2N][red split 2N][green pairs 2N][green split 2N]    runs two full transforms instead
// What the single-buffer path leaves to other launches is handled here, per workgroup and uniformly:
//   * the odd last block of a BC1 / BC4 buffer (half a vector) belongs to the lane behind the last whole vector;
//   * a buffer whose input is off a 16-byte boundary is read with dword loads (off a 4-byte boundary: byte loads) of the two
//     dwords of a vector that hold endpoints -- slower, the same bytes out.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "auto_launch.h"
#include "bcn_launch.h"
#include "launch_grid.h"
#include "ycocg_swar.h"

namespace dxtlt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

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

// BC1: blocks 2v (ca) and, unless `half`, 2v + 1 (cb); BC2 / BC3: block v (ca)
template <int FMT, int VARIANT>
__device__ __forceinline__ void colour_sections(uint8_t* __restrict__ pairs, uint64_t n, uint64_t v, uint32_t ca, uint32_t cb, bool half)
{
    // pairs: [c0 c1] dwords at 4 * block; split: c0 at 2 * block, c1 at 2 * n + 2 * block (behind the pairs section)
    uint8_t* split = pairs + 4 * n;
    const uint32_t da = decorrelate2<VARIANT>(ca);
    if constexpr (FMT == kBc1) {
        if (half) {
            *reinterpret_cast<uint32_t*>(pairs + 8 * v) = da;
            *reinterpret_cast<uint16_t*>(split + 4 * v) = (uint16_t)da;
            *reinterpret_cast<uint16_t*>(split + 2 * n + 4 * v) = (uint16_t)(da >> 16);
            return;
        }
        const uint32_t db = decorrelate2<VARIANT>(cb);
        *reinterpret_cast<u32x2*>(pairs + 8 * v) = u32x2{da, db};
        *reinterpret_cast<uint32_t*>(split + 4 * v) = (da & 0xFFFFu) | (db << 16);
        *reinterpret_cast<uint32_t*>(split + 2 * n + 4 * v) = (da >> 16) | (db & 0xFFFF0000u);
    } else {
        *reinterpret_cast<uint32_t*>(pairs + 4 * v) = da;
        *reinterpret_cast<uint16_t*>(split + 2 * v) = (uint16_t)da;
        *reinterpret_cast<uint16_t*>(split + 2 * n + 2 * v) = (uint16_t)(da >> 16);
    }
}

// the endpoint pair `e` (low 16 bits) of block b: [pairs 2N][split: first endpoints N, second endpoints N] at `sec`
__device__ __forceinline__ void endpoint_sections(uint8_t* __restrict__ sec, uint64_t n, uint64_t b, uint32_t e)
{
    *reinterpret_cast<uint16_t*>(sec + 2 * b) = (uint16_t)e;
    sec[2 * n + b] = (uint8_t)e;
    sec[3 * n + b] = (uint8_t)(e >> 8);
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

    if constexpr (FMT == kBc4) {
        // [pairs 2N][split 2N]; this lane: blocks 2v and 2v + 1
        endpoint_sections(arena, n, 2 * v, x);
        if (!half)
            endpoint_sections(arena, n, 2 * v + 1, z);
    } else if constexpr (FMT == kBc5) {
        endpoint_sections(arena, n, v, x);            // red
        endpoint_sections(arena + 4 * n, n, v, z);    // green
    } else {
        uint8_t* colour0 = arena;
        uint32_t ca, cb = 0;
        if constexpr (FMT == kBc1) {
            ca = x;
            cb = z;
        } else {
            ca = z;
            if constexpr (FMT == kBc3) {
                endpoint_sections(arena, n, v, x);    // alpha endpoints
                colour0 = arena + 4 * n;
            }
        }
        colour_sections<FMT, kNone>(colour0, n, v, ca, cb, half);
        colour_sections<FMT, kVar1>(colour0 + 8 * n, n, v, ca, cb, half);
        if constexpr (ALL) {
            colour_sections<FMT, kVar2>(colour0 + 16 * n, n, v, ca, cb, half);
            colour_sections<FMT, kVar3>(colour0 + 24 * n, n, v, ca, cb, half);
        }
    }
}

}  // namespace

uint64_t batch_auto_slice_bytes(Format fmt, bool all_variants, uint64_t blocks)
{
    if (fmt == kBc4)
        return 4 * blocks;
    if (fmt == kBc5)
        return 8 * blocks;
    return auto_arena_bytes(fmt, all_variants, blocks);
}

int batch_auto_sections(Format fmt, bool all_variants, uint64_t blocks, uint64_t* offsets, uint64_t* lengths)
{
    int n = 0;
    if (fmt == kBc4 || fmt == kBc5) {
        for (int k = 0; k < (fmt == kBc5 ? 4 : 2); ++k) {
            offsets[n] = 2 * blocks * (uint64_t)k;
            lengths[n++] = 2 * blocks;
        }
        return n;
    }
    if (fmt == kBc3)
        for (int sp = 0; sp < 2; ++sp) {
            offsets[n] = auto_alpha_section_offset(blocks, sp != 0);
            lengths[n++] = 2 * blocks;
        }
    for (int m = 0; m < (all_variants ? 4 : 2); ++m)
        for (int sp = 0; sp < 2; ++sp) {
            offsets[n] = auto_section_offset(fmt, blocks, m, sp != 0);
            lengths[n++] = 4 * blocks;
        }
    return n;
}

uint32_t batch_auto_workgroups(Format fmt, uint64_t blocks)
{
    const uint64_t lanes = fmt == kBc1 || fmt == kBc4 ? (blocks + 1) / 2 : blocks;
    return (uint32_t)((lanes + 255) / 256);
}

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
