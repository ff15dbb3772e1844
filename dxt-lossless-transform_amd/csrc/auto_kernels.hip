// auto_kernels.hip -- transform_bcN_auto, candidate phase: every endpoint section the size estimator will be shown,
// from ONE read of the input.
//
// The reference tries its candidates one full transform at a time and estimates the endpoint section(s) only -- the
// index sections are the same for every candidate and are left out (core/dxt-lossless-transform-bc1/src/transform/
// transform_auto.rs:245-256; BC2 / BC3 twins).  What differs between candidates is
//     the colour section   (4 bytes per block): YCoCg-R variant x {c0/c1 pairs, all c0 then all c1}
//     BC3's alpha endpoints (2 bytes per block): {a0/a1 pairs, all a0 then all a1}
// so 4 (fast search: variants None, Variant1) or 8 colour sections and, for BC3, 2 alpha sections cover all 4 / 8
// (BC1, BC2) or 8 / 16 (BC3) candidates.  This kernel writes them all into an arena:
//     [alpha pairs 2N][alpha split 2N]                         BC3 only
//     for variant in (None, Variant1[, Variant2, Variant3]):  [colour pairs 4N][colour split 4N]
// (auto_launch.h: auto_sections lists it).  One 16-byte vector per lane (two BC1 blocks or one BC2 / BC3 block), no LDS: a lane's
// piece of every section is 2-8 contiguous bytes and a wave instruction writes 128-512 contiguous bytes of one section.  What a
// lane does with its vector is auto_candidate_lanes.h, shared with the batched kernel.  Traffic: len read once,
// (sections x 4 + 4 [BC3]) bytes per block written -- BC1, fast search: 3 x len against 8 x len for four full
// transforms.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "auto_candidate_lanes.h"
#include "auto_launch.h"
#include "bcn_launch.h"
#include "launch_grid.h"

namespace dxtlt {

namespace {

// n = blocks; the kernel covers the first `vectors` 16-byte vectors (BC1: an odd last block is handled by the caller's
// tail launch with vectors = 0 semantics -- see launch_auto_candidates)
template <int FMT, bool ALL>
__global__ void __launch_bounds__(256)
auto_candidates_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ arena, uint64_t n, uint64_t vectors)
{
    const uint64_t v = workgroup_index() * 256 + threadIdx.x;
    if (v >= vectors)
        return;
    const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + 16 * v));
    candidate_lane<FMT, ALL, false>(arena, n, v, q.x, q.z, false);
}

// the odd last block of a BC1 buffer (half a vector): one lane, scalar accesses
template <bool ALL>
__global__ void auto_candidates_bc1_last_block(const uint8_t* __restrict__ in, uint8_t* __restrict__ arena, uint64_t n)
{
    const uint64_t b = n - 1;
    candidate_lane<kBc1, ALL, true>(arena, n, b / 2, *reinterpret_cast<const uint32_t*>(in + 8 * b), 0, true);
}

}  // namespace

hipError_t launch_auto_candidates(Format fmt, bool all_variants, const void* d_in, void* d_arena, uint64_t blocks,
                                  hipStream_t stream)
{
    if (blocks == 0)
        return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(d_in) & 15) != 0 || (reinterpret_cast<uintptr_t>(d_arena) & 15) != 0)
        return hipErrorInvalidValue;
    const uint8_t* in = static_cast<const uint8_t*>(d_in);
    uint8_t* arena = static_cast<uint8_t*>(d_arena);
    const uint64_t vectors = fmt == kBc1 ? blocks / 2 : blocks;
    if (vectors > 0) {
        dim3 grid;
        if (hipError_t e = grid_rows(vectors, 256, grid); e != hipSuccess)
            return e;
#define DXTLT_AUTO_LAUNCH(F, A) \
        hipLaunchKernelGGL((auto_candidates_kernel<F, A>), grid, dim3(256), 0, stream, in, arena, blocks, vectors)
        if (fmt == kBc1) { if (all_variants) DXTLT_AUTO_LAUNCH(kBc1, true); else DXTLT_AUTO_LAUNCH(kBc1, false); }
        else if (fmt == kBc2) { if (all_variants) DXTLT_AUTO_LAUNCH(kBc2, true); else DXTLT_AUTO_LAUNCH(kBc2, false); }
        else { if (all_variants) DXTLT_AUTO_LAUNCH(kBc3, true); else DXTLT_AUTO_LAUNCH(kBc3, false); }
#undef DXTLT_AUTO_LAUNCH
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
    }
    if (fmt == kBc1 && (blocks & 1)) {
        if (all_variants)
            hipLaunchKernelGGL(auto_candidates_bc1_last_block<true>, dim3(1), dim3(1), 0, stream, in, arena, blocks);
        else
            hipLaunchKernelGGL(auto_candidates_bc1_last_block<false>, dim3(1), dim3(1), 0, stream, in, arena, blocks);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace dxtlt
