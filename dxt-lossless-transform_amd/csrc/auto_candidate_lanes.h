// auto_candidate_lanes.h -- the lane work of the candidate kernels of transform_bcN_auto (auto_kernels.hip, batch_auto_kernels.hip):
// from the two endpoint dwords of a lane's 16-byte vector to its piece of every section of a slice (auto_launch.h: the layout).
// One body for the three kernels that differ in how a lane finds and loads its vector.  Device code only.
#pragma once
#include <cstdint>

#include "bcn_launch.h"
#include "ycocg_swar.h"

namespace dxtlt {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// One variant's colour sections at `pairs`.  BC1: blocks 2v (ca) and, unless `half`, 2v + 1 (cb); BC2 / BC3: block v (ca).
// HALF_LANES: whether the kernel has half lanes at all; `half` is read only then (see candidate_lane).
template <int FMT, int VARIANT, bool HALF_LANES>
__device__ __forceinline__ void colour_sections(uint8_t* __restrict__ pairs, uint64_t n, uint64_t v, uint32_t ca, uint32_t cb, bool half)
{
    // pairs: [c0 c1] dwords at 4 * block; split: c0 at 2 * block, c1 at 2 * n + 2 * block (behind the pairs section)
    uint8_t* split = pairs + 4 * n;
    const uint32_t da = decorrelate2<VARIANT>(ca);
    if constexpr (FMT == kBc1) {
        if constexpr (HALF_LANES) {
            if (half) {
                *reinterpret_cast<uint32_t*>(pairs + 8 * v) = da;
                *reinterpret_cast<uint16_t*>(split + 4 * v) = (uint16_t)da;
                *reinterpret_cast<uint16_t*>(split + 2 * n + 4 * v) = (uint16_t)(da >> 16);
                return;
            }
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

// Vector v of a buffer of n blocks, its endpoint dwords x (bytes 0-3) and z (bytes 8-11) -> every section of the slice at `slice`.
// `half`: the vector is the odd last block of a BC1 / BC4 buffer and z does not exist.  A kernel whose lanes all hold whole vectors
// says so at compile time (HALF_LANES = false): its colour sections are then compiled without the branch, not with a folded one --
// the compiler simplifies colour_sections before it inlines it, and does so differently when the branch is there (DESIGN section 4,
// lesson 13; profiles/auto_candidates_refactor_isa.txt).
template <int FMT, bool ALL, bool HALF_LANES>
__device__ __forceinline__ void candidate_lane(uint8_t* slice, uint64_t n, uint64_t v, uint32_t x, uint32_t z, bool half)
{
    if constexpr (FMT == kBc4) {
        endpoint_sections(slice, n, 2 * v, x);
        if (!(HALF_LANES && half))
            endpoint_sections(slice, n, 2 * v + 1, z);
    } else if constexpr (FMT == kBc5) {
        endpoint_sections(slice, n, v, x);            // red
        endpoint_sections(slice + 4 * n, n, v, z);    // green
    } else {
        uint8_t* colour0 = slice;
        uint32_t ca, cb = 0;
        if constexpr (FMT == kBc1) {
            ca = x;
            cb = z;
        } else {
            ca = z;
            if constexpr (FMT == kBc3) {
                endpoint_sections(slice, n, v, x);    // alpha endpoints
                colour0 = slice + 4 * n;
            }
        }
        colour_sections<FMT, kNone, HALF_LANES>(colour0, n, v, ca, cb, half);
        colour_sections<FMT, kVar1, HALF_LANES>(colour0 + 8 * n, n, v, ca, cb, half);
        if constexpr (ALL) {
            colour_sections<FMT, kVar2, HALF_LANES>(colour0 + 16 * n, n, v, ca, cb, half);
            colour_sections<FMT, kVar3, HALF_LANES>(colour0 + 24 * n, n, v, ca, cb, half);
        }
    }
}

}  // namespace dxtlt
