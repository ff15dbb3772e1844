// auto_normalize_kernels.hip -- transform_bcN_auto_with_normalization (BC1, BC2, BC3), candidate phase: the colour section of every
// (normalisation mode, YCoCg-R variant, split) candidate -- and, BC3, the alpha endpoint section of every (alpha mode, split) --
// from ONE read of the input.
//
// The reference normalises the input three times (normalize_blocks_all_modes), transforms each copy once per settings candidate and
// estimates the colour section only (bc1 experimental/normalize_blocks/transform.rs:222-333).  Normalisation changes a block's
// colour dword and its index dword; the index section is never shown to the estimator, so it is not produced here.  A lane
// classifies its block(s) once (classify_bc1_block / solid_colour_4c, in registers), derives the block's colour dword under each of
// the three modes and hands each to colour_sections of auto_candidate_lanes.h -- the body the plain candidate kernels run.  Layout:
// auto_launch.h, auto_normalize_sections.  One 16-byte vector per lane, no LDS; traffic: len read once, 48 / 96 bytes per block
// written.
//
// BC3 (this build's extension): the alpha half and the colour half of a block are normalised independently (bc23_normalize.h), so
// the 96 / 192 candidates are sums over 8 alpha endpoint sections and BC2's 12 / 24 colour sections.  A lane classifies its alpha
// half once (uniform_alpha_bc3), derives the endpoint pair under the four alpha modes and writes four endpoint_sections; its colour
// half goes the BC2 way behind them.  Layout: auto_normalize_bc3_sections; 64 / 112 bytes per block written.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "auto_candidate_lanes.h"
#include "auto_launch.h"
#include "bc1_normalize.h"
#include "bc23_normalize.h"
#include "bcn_launch.h"
#include "launch_grid.h"

namespace dxtlt {

namespace {

// the colour dword of one block under None* / Color0Only / ReplicateColor
struct NormColours {
    uint32_t none, color0, replicate;
};

// BC1: None* = transparent blocks rewritten (kNormTransparentOnly), as in every buffer of normalize_blocks_all_modes
__device__ __forceinline__ NormColours bc1_colours(uint32_t colours, uint32_t indices)
{
    uint32_t solid = 0;
    const int cls = classify_bc1_block(colours, indices, solid);
    NormColours c{colours, colours, colours};
    if (cls == kBlockTransparent)
        c.none = c.color0 = c.replicate = 0xFFFFFFFFu;
    else if (cls == kBlockSolid) {
        c.color0 = solid;
        c.replicate = solid | (solid << 16);
    }
    return c;
}

// BC2: None = the input's colours
__device__ __forceinline__ NormColours bc2_colours(uint32_t colours, uint32_t indices)
{
    uint32_t solid = 0;
    NormColours c{colours, colours, colours};
    if (solid_colour_4c(colours, indices, solid)) {
        c.color0 = solid;
        c.replicate = solid | (solid << 16);
    }
    return c;
}

// BC3: the alpha endpoint pair (a0 | a1 << 8) of one block under the four alpha modes (normalize_alpha_half_bc3's bytes 0-1)
struct NormAlphaPairs {
    uint32_t none, uniform, fill, zero;
};

__device__ __forceinline__ NormAlphaPairs bc3_alpha_pairs(uint32_t w0, uint32_t w1)
{
    const uint32_t pair = w0 & 0xFFFFu;
    uint32_t alpha = 0;
    NormAlphaPairs a{pair, pair, pair, pair};
    if (uniform_alpha_bc3(w0, w1, alpha)) {
        a.uniform = alpha;                               // (alpha, 0)
        a.fill = alpha == 255 ? 0xFFFFu : alpha;         // opaque: eight 0xFF bytes
        a.zero = alpha == 255 ? 0u : alpha;              // opaque: (0, 0), indices 0xFF
    }
    return a;
}

// every variant's sections of one normalisation mode, at `colour0`
template <int FMT, bool ALL, bool HALF_LANES>
__device__ __forceinline__ void variant_sections(uint8_t* colour0, uint64_t n, uint64_t v, uint32_t ca, uint32_t cb, bool half)
{
    colour_sections<FMT, kNone, HALF_LANES>(colour0, n, v, ca, cb, half);
    colour_sections<FMT, kVar1, HALF_LANES>(colour0 + 8 * n, n, v, ca, cb, half);
    if constexpr (ALL) {
        colour_sections<FMT, kVar2, HALF_LANES>(colour0 + 16 * n, n, v, ca, cb, half);
        colour_sections<FMT, kVar3, HALF_LANES>(colour0 + 24 * n, n, v, ca, cb, half);
    }
}

// a: block 2v (BC1) or v (BC2); b: block 2v + 1 of BC1 unless `half`
template <int FMT, bool ALL, bool HALF_LANES>
__device__ __forceinline__ void normalize_candidate_lane(uint8_t* arena, uint64_t n, uint64_t v, const NormColours& a,
                                                         const NormColours& b, bool half)
{
    const uint64_t per_norm = (ALL ? 32 : 16) * n;
    variant_sections<FMT, ALL, HALF_LANES>(arena, n, v, a.none, b.none, half);
    variant_sections<FMT, ALL, HALF_LANES>(arena + per_norm, n, v, a.color0, b.color0, half);
    variant_sections<FMT, ALL, HALF_LANES>(arena + 2 * per_norm, n, v, a.replicate, b.replicate, half);
}

// n = blocks; the kernel covers the first `vectors` 16-byte vectors (BC1: n / 2, an odd last block has a launch of its own)
template <int FMT, bool ALL>
__global__ void __launch_bounds__(256)
auto_normalize_candidates_kernel(const uint8_t* __restrict__ in, uint8_t* __restrict__ arena, uint64_t n, uint64_t vectors)
{
    const uint64_t v = workgroup_index() * 256 + threadIdx.x;
    if (v >= vectors)
        return;
    const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + 16 * v));
    if constexpr (FMT == kBc1)
        normalize_candidate_lane<kBc1, ALL, false>(arena, n, v, bc1_colours(q.x, q.y), bc1_colours(q.z, q.w), false);
    else if constexpr (FMT == kBc2)
        normalize_candidate_lane<kBc2, ALL, false>(arena, n, v, bc2_colours(q.z, q.w), NormColours{0, 0, 0}, false);
    else {
        const NormAlphaPairs a = bc3_alpha_pairs(q.x, q.y);
        endpoint_sections(arena, n, v, a.none);
        endpoint_sections(arena + 4 * n, n, v, a.uniform);
        endpoint_sections(arena + 8 * n, n, v, a.fill);
        endpoint_sections(arena + 12 * n, n, v, a.zero);
        normalize_candidate_lane<kBc3, ALL, false>(arena + 16 * n, n, v, bc2_colours(q.z, q.w), NormColours{0, 0, 0}, false);
    }
}

// the odd last block of a BC1 buffer (half a vector): one lane
template <bool ALL>
__global__ void auto_normalize_candidates_bc1_last_block(const uint8_t* __restrict__ in, uint8_t* __restrict__ arena, uint64_t n)
{
    const uint64_t b = n - 1;
    const u32x2 q = *reinterpret_cast<const u32x2*>(in + 8 * b);
    normalize_candidate_lane<kBc1, ALL, true>(arena, n, b / 2, bc1_colours(q.x, q.y), NormColours{0, 0, 0}, true);
}

// BC2: only the "would anything change" flag; one block per lane, its colour half alone is read
__global__ void __launch_bounds__(256)
bc2_any_normalizable_kernel(const uint8_t* in, uint64_t n, uint32_t* d_any)
{
    const uint64_t i = workgroup_index() * 256 + threadIdx.x;
    bool changed = false;
    if (i < n) {
        const uint8_t* p = in + 16 * i + 8;
        uint32_t c, x;
        if ((reinterpret_cast<uintptr_t>(in) & 7) == 0) {
            const u32x2 q = __builtin_nontemporal_load(reinterpret_cast<const u32x2*>(p));
            c = q.x, x = q.y;
        } else {
            c = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
            x = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
        }
        uint32_t solid = 0;
        changed = solid_colour_4c(c, x, solid);
    }
    // one store per wave at most; every writer stores the same value
    if (__ballot(changed) != 0 && (threadIdx.x & 63) == 0)
        *d_any = 1u;
}

// BC3: the same flag for a block whose alpha half is uniform or whose colour half is a normalisable solid; one block per lane
__global__ void __launch_bounds__(256)
bc3_any_normalizable_kernel(const uint8_t* in, uint64_t n, uint32_t* d_any)
{
    const uint64_t i = workgroup_index() * 256 + threadIdx.x;
    bool changed = false;
    if (i < n) {
        const uint8_t* p = in + 16 * i;
        uint32_t w[4];
        if ((reinterpret_cast<uintptr_t>(in) & 15) == 0) {
            const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
            w[0] = q.x, w[1] = q.y, w[2] = q.z, w[3] = q.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
        }
        uint32_t alpha = 0, solid = 0;
        changed = uniform_alpha_bc3(w[0], w[1], alpha) || solid_colour_4c(w[2], w[3], solid);
    }
    // one store per wave at most; every writer stores the same value
    if (__ballot(changed) != 0 && (threadIdx.x & 63) == 0)
        *d_any = 1u;
}

}  // namespace

hipError_t launch_auto_normalize_candidates(Format fmt, bool all_variants, const void* d_in, void* d_arena, uint64_t blocks,
                                            hipStream_t stream, int* launches)
{
    if (launches)
        *launches = 0;
    if (fmt != kBc1 && fmt != kBc2 && fmt != kBc3)
        return hipErrorInvalidValue;
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
#define DXTLT_AUTO_NORM_LAUNCH(F, A) \
        hipLaunchKernelGGL((auto_normalize_candidates_kernel<F, A>), grid, dim3(256), 0, stream, in, arena, blocks, vectors)
        if (fmt == kBc1) { if (all_variants) DXTLT_AUTO_NORM_LAUNCH(kBc1, true); else DXTLT_AUTO_NORM_LAUNCH(kBc1, false); }
        else if (fmt == kBc2) { if (all_variants) DXTLT_AUTO_NORM_LAUNCH(kBc2, true); else DXTLT_AUTO_NORM_LAUNCH(kBc2, false); }
        else { if (all_variants) DXTLT_AUTO_NORM_LAUNCH(kBc3, true); else DXTLT_AUTO_NORM_LAUNCH(kBc3, false); }
#undef DXTLT_AUTO_NORM_LAUNCH
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
        if (launches)
            ++*launches;
    }
    if (fmt == kBc1 && (blocks & 1)) {
        if (all_variants)
            hipLaunchKernelGGL(auto_normalize_candidates_bc1_last_block<true>, dim3(1), dim3(1), 0, stream, in, arena, blocks);
        else
            hipLaunchKernelGGL(auto_normalize_candidates_bc1_last_block<false>, dim3(1), dim3(1), 0, stream, in, arena, blocks);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
        if (launches)
            ++*launches;
    }
    return hipSuccess;
}

hipError_t launch_bc2_any_normalizable(const void* in, uint64_t num_blocks, uint32_t* d_any, hipStream_t stream)
{
    if (num_blocks == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_rows(num_blocks, 256, grid); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(bc2_any_normalizable_kernel, grid, dim3(256), 0, stream, static_cast<const uint8_t*>(in), num_blocks, d_any);
    return hipGetLastError();
}

hipError_t launch_bc3_any_normalizable(const void* in, uint64_t num_blocks, uint32_t* d_any, hipStream_t stream)
{
    if (num_blocks == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_rows(num_blocks, 256, grid); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(bc3_any_normalizable_kernel, grid, dim3(256), 0, stream, static_cast<const uint8_t*>(in), num_blocks, d_any);
    return hipGetLastError();
}

}  // namespace dxtlt
