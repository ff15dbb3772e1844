// normalize_kernels.hip -- gfx950 kernels for BC1 / BC2 / BC3 block normalisation as stand-alone operations (the versions fused
// into the forward transform live in bcn_kernels.hip and bcn_norm23_kernels.hip; the per-block rules are bc1_normalize.h and
// bc23_normalize.h).
//
// Reference (experimental modules, /root/reference/src/core/dxt-lossless-transform-bc{1,2,3}/src/experimental/
// normalize_blocks/normalize.rs): normalize_blocks (bc1 :38-96, bc2 :35, bc3 :36), normalize_split_blocks_in_place (bc1 :286-386,
// bc2 :382, bc3 :539), normalize_blocks_all_modes (bc1 :417-481, bc2 :193, bc3 :419).  Element-wise, one-shot grid (the structure
// that measured best for the transform kernels): HBM bound, 2*len per output buffer.  One 16-byte vector per lane -- two BC1
// blocks, one BC2 / BC3 block --; pointers that are not 16-byte aligned, and BC1's odd blocks at the end, take a lane-per-block
// path with natural-width or byte accesses.
#include <hip/hip_runtime.h>

#include "bc1_normalize.h"
#include "bc23_normalize.h"
#include "bcn_launch.h"
#include "launch_grid.h"
#include "streaming_store.h"

namespace dxtlt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int kNormThreads = 256;

__device__ __forceinline__ bool is_aligned(const void* p, int a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p, bool aligned4)
{
    if (aligned4)
        return *reinterpret_cast<const uint32_t*>(p);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

__device__ __forceinline__ void store_u32(uint8_t* p, uint32_t v, bool aligned4)
{
    if (aligned4) {
        *reinterpret_cast<uint32_t*>(p) = v;
    } else {
        p[0] = (uint8_t)v;
        p[1] = (uint8_t)(v >> 8);
        p[2] = (uint8_t)(v >> 16);
        p[3] = (uint8_t)(v >> 24);
    }
}

__device__ __forceinline__ void flag_if_any(bool changed, uint32_t* d_any)
{
    // one store per wave at most; every writer stores the same value
    if (d_any != nullptr && __ballot(changed) != 0 && (threadIdx.x & 63) == 0)
        *d_any = 1u;
}

// ---- BC1, AoS blocks -------------------------------------------------------------------------------------
// lanes [0, pairs) take two blocks as one 16-byte vector (pointers 16-byte aligned); lanes [pairs, pairs + singles)
// take one block each with 4-byte or byte accesses
__global__ void __launch_bounds__(kNormThreads)
normalize_blocks_kernel(const uint8_t* in, uint8_t* out, uint64_t pairs, uint64_t singles, int mode)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i < pairs) {
        const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + 16 * i));
        uint32_t ca = q.x, xa = q.y, cb = q.z, xb = q.w;
        normalize_bc1_block_rt(mode, ca, xa);
        normalize_bc1_block_rt(mode, cb, xb);
        store_streaming16(out + 16 * i, u32x4{ca, xa, cb, xb});
    } else if (i < pairs + singles) {
        const uint64_t b = 2 * pairs + (i - pairs);
        const bool a4 = is_aligned(in, 4) && is_aligned(out, 4);
        uint32_t c = load_u32(in + 8 * b, a4), x = load_u32(in + 8 * b + 4, a4);
        normalize_bc1_block_rt(mode, c, x);
        store_u32(out + 8 * b, c, a4);
        store_u32(out + 8 * b + 4, x, a4);
    }
}

// in -> three outputs (None, Color0Only, ReplicateColor), classification done once per block
__global__ void __launch_bounds__(kNormThreads)
normalize_all_modes_kernel(const uint8_t* in, uint8_t* out0, uint8_t* out1, uint8_t* out2, uint64_t pairs, uint64_t singles,
                           uint32_t* d_any)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    bool changed = false;
    if (i < pairs) {
        const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + 16 * i));
        // the transparent rewrite goes to every output, the `None` one included (normalize.rs:447-454)
        u32x4 z = q, a = q, b = q;
        uint32_t sa = 0, sb = 0;
        const int ca = classify_bc1_block(q.x, q.y, sa), cb = classify_bc1_block(q.z, q.w, sb);
        if (ca == kBlockTransparent) { z.x = z.y = a.x = a.y = b.x = b.y = 0xFFFFFFFFu; }
        if (ca == kBlockSolid) { a.x = sa; a.y = 0; b.x = sa | (sa << 16); b.y = 0; }
        if (cb == kBlockTransparent) { z.z = z.w = a.z = a.w = b.z = b.w = 0xFFFFFFFFu; }
        if (cb == kBlockSolid) { a.z = sb; a.w = 0; b.z = sb | (sb << 16); b.w = 0; }
        changed = ca != kBlockUnchanged || cb != kBlockUnchanged;
        __builtin_nontemporal_store(z, reinterpret_cast<u32x4*>(out0 + 16 * i));
        __builtin_nontemporal_store(a, reinterpret_cast<u32x4*>(out1 + 16 * i));
        __builtin_nontemporal_store(b, reinterpret_cast<u32x4*>(out2 + 16 * i));
    } else if (i < pairs + singles) {
        const uint64_t blk = 2 * pairs + (i - pairs);
        const bool a4 = is_aligned(in, 4) && is_aligned(out0, 4) && is_aligned(out1, 4) && is_aligned(out2, 4);
        const uint32_t c = load_u32(in + 8 * blk, a4), x = load_u32(in + 8 * blk + 4, a4);
        uint32_t s = 0;
        const int cls = classify_bc1_block(c, x, s);
        uint32_t c0 = c, x0 = x, c1 = c, x1 = x, c2 = c, x2 = x;
        if (cls == kBlockTransparent) { c0 = x0 = c1 = x1 = c2 = x2 = 0xFFFFFFFFu; }
        if (cls == kBlockSolid) { c1 = s; c2 = s | (s << 16); x1 = x2 = 0; }
        changed = cls != kBlockUnchanged;
        store_u32(out0 + 8 * blk, c0, a4);
        store_u32(out0 + 8 * blk + 4, x0, a4);
        store_u32(out1 + 8 * blk, c1, a4);
        store_u32(out1 + 8 * blk + 4, x1, a4);
        store_u32(out2 + 8 * blk, c2, a4);
        store_u32(out2 + 8 * blk + 4, x2, a4);
    }
    flag_if_any(changed, d_any);
}

// only the "would anything change" flag (the auto transform uses it to skip the normalisation candidates)
__global__ void __launch_bounds__(kNormThreads)
any_normalizable_kernel(const uint8_t* in, uint64_t pairs, uint64_t singles, uint32_t* d_any)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    bool changed = false;
    uint32_t s = 0;
    if (i < pairs) {
        const u32x4 q = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(in + 16 * i));
        changed = classify_bc1_block(q.x, q.y, s) != kBlockUnchanged || classify_bc1_block(q.z, q.w, s) != kBlockUnchanged;
    } else if (i < pairs + singles) {
        const uint64_t blk = 2 * pairs + (i - pairs);
        const bool a4 = is_aligned(in, 4);
        changed = classify_bc1_block(load_u32(in + 8 * blk, a4), load_u32(in + 8 * blk + 4, a4), s) != kBlockUnchanged;
    }
    flag_if_any(changed, d_any);
}

// ---- BC1, split blocks: colours[4 * n] and indices[4 * n], in place ------------------------------------------
// lanes [0, quads) take four blocks (one 16-byte vector of each array); the rest one block each
__global__ void __launch_bounds__(kNormThreads)
normalize_split_kernel(uint8_t* colours, uint8_t* indices, uint64_t quads, uint64_t singles, int mode)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i < quads) {
        const u32x4 cv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(colours + 16 * i));
        const u32x4 xv = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(indices + 16 * i));
        uint32_t c[4] = {cv.x, cv.y, cv.z, cv.w}, x[4] = {xv.x, xv.y, xv.z, xv.w};
        int any = kBlockUnchanged;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            any |= normalize_bc1_block_rt(mode, c[k], x[k]);
        if (any != kBlockUnchanged) {   // in place: untouched vectors need no write
            *reinterpret_cast<u32x4*>(colours + 16 * i) = u32x4{c[0], c[1], c[2], c[3]};
            *reinterpret_cast<u32x4*>(indices + 16 * i) = u32x4{x[0], x[1], x[2], x[3]};
        }
    } else if (i < quads + singles) {
        const uint64_t b = 4 * quads + (i - quads);
        const bool a4 = is_aligned(colours, 4) && is_aligned(indices, 4);
        uint32_t c = load_u32(colours + 4 * b, a4), x = load_u32(indices + 4 * b, a4);
        if (normalize_bc1_block_rt(mode, c, x) != kBlockUnchanged) {
            store_u32(colours + 4 * b, c, a4);
            store_u32(indices + 4 * b, x, a4);
        }
    }
}

// ---- BC2 / BC3: one 16-byte block per lane -----------------------------------------------------------------
__device__ __forceinline__ void load_block(const uint8_t* p, bool vec, uint32_t (&q)[4])
{
    if (vec) {
        const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p));
        q[0] = v.x, q[1] = v.y, q[2] = v.z, q[3] = v.w;
    } else {
        const bool a4 = (reinterpret_cast<uintptr_t>(p) & 3) == 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            q[i] = load_u32(p + 4 * i, a4);
    }
}

__device__ __forceinline__ void store_block16(uint8_t* p, bool vec, const uint32_t (&q)[4])
{
    if (vec) {
        store_streaming16(p, u32x4{q[0], q[1], q[2], q[3]});
    } else {
        const bool a4 = (reinterpret_cast<uintptr_t>(p) & 3) == 0;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            store_u32(p + 4 * i, q[i], a4);
    }
}

template <int FMT>
__global__ void __launch_bounds__(kNormThreads)
normalize23_kernel(const uint8_t* in, uint8_t* out, uint64_t n, int alpha_mode, int color_mode, int vec)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i >= n)
        return;
    uint32_t q[4];
    load_block(in + 16 * i, vec != 0, q);
    normalize_block_bc23<FMT>(alpha_mode, color_mode, q);
    store_block16(out + 16 * i, vec != 0, q);
}

struct OutPtrs {
    uint8_t* p[12];
};

// BC2: outputs 0..2 = colour modes; BC3: outputs [alpha_mode * 3 + colour_mode].  The block is classified once.
template <int FMT>
__global__ void __launch_bounds__(kNormThreads)
normalize23_all_modes_kernel(const uint8_t* in, OutPtrs outs, uint64_t n, int vec)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i >= n)
        return;
    uint32_t q[4];
    load_block(in + 16 * i, vec != 0, q);
    uint32_t solid = 0, alpha = 0;
    const bool is_solid = solid_colour_4c(q[2], q[3], solid);
    const bool is_uniform = FMT == 3 && uniform_alpha_bc3(q[0], q[1], alpha);
    constexpr int kAlphaModes = FMT == 3 ? 4 : 1;
#pragma unroll
    for (int a = 0; a < kAlphaModes; ++a) {
        uint32_t w0 = q[0], w1 = q[1];
        if (is_uniform && a != kAlphaNone) {
            if (alpha == 255 && a == kAlphaOpaqueFillAll) {
                w0 = w1 = 0xFFFFFFFFu;
            } else if (alpha == 255 && a == kAlphaOpaqueZeroAlphaMaxIndices) {
                w0 = 0xFFFF0000u, w1 = 0xFFFFFFFFu;
            } else {
                w0 = alpha, w1 = 0;
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            uint32_t o[4] = {w0, w1, q[2], q[3]};
            if (is_solid && c != kNormNone) {
                o[2] = c == kNormReplicateColor ? solid | (solid << 16) : solid;
                o[3] = 0;
            }
            store_block16(outs.p[a * 3 + c] + 16 * i, vec != 0, o);
        }
    }
}

// BC2, colours (4 bytes per block) and indices (4 bytes per block) in place; the alpha array is not needed
__global__ void __launch_bounds__(kNormThreads)
normalize2_split_kernel(uint8_t* colours, uint8_t* indices, uint64_t n, int color_mode)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i >= n)
        return;
    const bool a4 = ((reinterpret_cast<uintptr_t>(colours) | reinterpret_cast<uintptr_t>(indices)) & 3) == 0;
    uint32_t c = load_u32(colours + 4 * i, a4), x = load_u32(indices + 4 * i, a4);
    if (normalize_colour_half_4c(color_mode, c, x)) {
        store_u32(colours + 4 * i, c, a4);
        store_u32(indices + 4 * i, x, a4);
    }
}

// BC3, four arrays in place: alpha endpoints (2 bytes per block), alpha indices (6), colour endpoints (4), colour indices (4)
__global__ void __launch_bounds__(kNormThreads)
normalize3_split_kernel(uint8_t* aep, uint8_t* aidx, uint8_t* cep, uint8_t* cidx, uint64_t n, int alpha_mode, int color_mode)
{
    const uint64_t i = workgroup_index() * kNormThreads + threadIdx.x;
    if (i >= n)
        return;
    const bool c4 = ((reinterpret_cast<uintptr_t>(cep) | reinterpret_cast<uintptr_t>(cidx)) & 3) == 0;
    uint8_t* pe = aep + 2 * i;
    uint8_t* pi = aidx + 6 * i;
    uint32_t w0 = (uint32_t)pe[0] | ((uint32_t)pe[1] << 8) | ((uint32_t)pi[0] << 16) | ((uint32_t)pi[1] << 24);
    uint32_t w1 = (uint32_t)pi[2] | ((uint32_t)pi[3] << 8) | ((uint32_t)pi[4] << 16) | ((uint32_t)pi[5] << 24);
    if (normalize_alpha_half_bc3(alpha_mode, w0, w1)) {
        pe[0] = (uint8_t)w0;
        pe[1] = (uint8_t)(w0 >> 8);
        pi[0] = (uint8_t)(w0 >> 16);
        pi[1] = (uint8_t)(w0 >> 24);
        pi[2] = (uint8_t)w1;
        pi[3] = (uint8_t)(w1 >> 8);
        pi[4] = (uint8_t)(w1 >> 16);
        pi[5] = (uint8_t)(w1 >> 24);
    }
    uint32_t c = load_u32(cep + 4 * i, c4), x = load_u32(cidx + 4 * i, c4);
    if (normalize_colour_half_4c(color_mode, c, x)) {
        store_u32(cep + 4 * i, c, c4);
        store_u32(cidx + 4 * i, x, c4);
    }
}

// ---- launches ---------------------------------------------------------------------------------------------------
template <class... P>
inline bool all_aligned16(const P*... p) { return (((reinterpret_cast<uintptr_t>(p) & 15) == 0) && ...); }

// Grid of `lanes` lanes, then the launch; `lds_pad`: launch_grid.h, lds_pad_for_wgs_per_cu
template <class K, class... A>
hipError_t launch_lanes(K kernel, uint64_t lanes, size_t lds_pad, hipStream_t stream, A... args)
{
    dim3 grid;
    if (hipError_t e = grid_rows(lanes, kNormThreads, grid); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kernel, grid, dim3(kNormThreads), lds_pad, stream, args...);
    return hipGetLastError();
}

// BC1: `per_vector` blocks per 16-byte vector lane when every pointer is 16-byte aligned, the rest -- all blocks otherwise -- one
// block per lane
struct Bc1Lanes {
    uint64_t vectors, singles;
    Bc1Lanes(bool vec, uint64_t num_blocks, uint64_t per_vector)
        : vectors(vec ? num_blocks / per_vector : 0), singles(num_blocks - per_vector * vectors) {}
};

}  // namespace

hipError_t launch_normalize_bc1_blocks(const void* in, void* out, uint64_t num_blocks, int mode, hipStream_t stream)
{
    if (!norm_modes_in_range(kBc1, kAlphaNone, mode))
        return hipErrorInvalidValue;
    if (num_blocks == 0)
        return hipSuccess;
    if (mode == kNormNone)   // normalize.rs:53-64: a copy, or nothing when in place
        return in == out ? hipSuccess : hipMemcpyAsync(out, in, num_blocks * 8, hipMemcpyDeviceToDevice, stream);
    const Bc1Lanes l(all_aligned16(in, out), num_blocks, 2);
    return launch_lanes(normalize_blocks_kernel, l.vectors + l.singles, 0, stream, static_cast<const uint8_t*>(in),
                        static_cast<uint8_t*>(out), l.vectors, l.singles, mode);
}

hipError_t launch_normalize_bc1_split(void* colours, void* indices, uint64_t num_blocks, int mode, hipStream_t stream)
{
    if (!norm_modes_in_range(kBc1, kAlphaNone, mode))
        return hipErrorInvalidValue;
    if (num_blocks == 0 || mode == kNormNone)   // normalize.rs:293-295
        return hipSuccess;
    const Bc1Lanes l(all_aligned16(colours, indices), num_blocks, 4);
    return launch_lanes(normalize_split_kernel, l.vectors + l.singles, 0, stream, static_cast<uint8_t*>(colours),
                        static_cast<uint8_t*>(indices), l.vectors, l.singles, mode);
}

hipError_t launch_normalize_bc1_all_modes(const void* in, void* const out[3], uint64_t num_blocks, uint32_t* d_any,
                                          hipStream_t stream)
{
    if (num_blocks == 0)
        return hipSuccess;
    const Bc1Lanes l(all_aligned16(in, out[0], out[1], out[2]), num_blocks, 2);
    // 16 bytes read and 48 written per lane: six workgroups per CU instead of eight (1 GiB of blocks: 782 -> 696 us;
    // five 731, four 688, three 1011; profiles/r02_o_wgs_per_cu.txt)
    return launch_lanes(normalize_all_modes_kernel, l.vectors + l.singles, lds_pad_for_wgs_per_cu(6, kNormThreads, 0),
                        stream, static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out[0]), static_cast<uint8_t*>(out[1]),
                        static_cast<uint8_t*>(out[2]), l.vectors, l.singles, d_any);
}

hipError_t launch_bc1_any_normalizable(const void* in, uint64_t num_blocks, uint32_t* d_any, hipStream_t stream)
{
    if (num_blocks == 0)
        return hipSuccess;
    const Bc1Lanes l(all_aligned16(in), num_blocks, 2);
    return launch_lanes(any_normalizable_kernel, l.vectors + l.singles, 0, stream, static_cast<const uint8_t*>(in), l.vectors,
                        l.singles, d_any);
}

hipError_t launch_normalize_bc23_blocks(int fmt, const void* in, void* out, uint64_t num_blocks, int alpha_mode, int color_mode,
                                        hipStream_t stream)
{
    if ((fmt != 2 && fmt != 3) || !norm_modes_in_range(fmt, alpha_mode, color_mode))
        return hipErrorInvalidValue;
    if (num_blocks == 0)
        return hipSuccess;
    if (alpha_mode == kAlphaNone && color_mode == kNormNone)   // bc2 normalize.rs:50-61, bc3 normalize.rs:52-62
        return in == out ? hipSuccess : hipMemcpyAsync(out, in, num_blocks * 16, hipMemcpyDeviceToDevice, stream);
    const int vec = all_aligned16(in, out);
    return launch_lanes(fmt == 2 ? normalize23_kernel<2> : normalize23_kernel<3>, num_blocks, 0, stream,
                        static_cast<const uint8_t*>(in), static_cast<uint8_t*>(out), num_blocks, alpha_mode, color_mode, vec);
}

hipError_t launch_normalize_bc23_all_modes(int fmt, const void* in, void* const* outs, uint64_t num_blocks, hipStream_t stream)
{
    if (fmt != 2 && fmt != 3)
        return hipErrorInvalidValue;
    if (num_blocks == 0)
        return hipSuccess;
    const int count = fmt == 2 ? 3 : 12;
    OutPtrs o{};
    int vec = all_aligned16(in);
    for (int i = 0; i < count; ++i) {
        o.p[i] = static_cast<uint8_t*>(outs[i]);
        vec = vec && all_aligned16(outs[i]);
    }
    // one read, 3 (BC2) or 12 (BC3) copies written per lane: fewer resident workgroups per CU move more (launch_grid.h).
    // BC2, 1 GiB of blocks: 764 us at eight, 658 at six, 681 / 672 at five / four, 908 at three; BC3, 256 MiB: 700 at eight,
    // 664 / 680 / 616 at six / five / four, 584 at three (profiles/r02_o_wgs_per_cu.txt)
    return launch_lanes(fmt == 2 ? normalize23_all_modes_kernel<2> : normalize23_all_modes_kernel<3>, num_blocks,
                        lds_pad_for_wgs_per_cu(fmt == 2 ? 6 : 3, kNormThreads, 0), stream,
                        static_cast<const uint8_t*>(in), o, num_blocks, vec);
}

hipError_t launch_normalize_bc2_split(void* colours, void* indices, uint64_t num_blocks, int color_mode, hipStream_t stream)
{
    if (!norm_modes_in_range(kBc2, kAlphaNone, color_mode))
        return hipErrorInvalidValue;
    if (num_blocks == 0 || color_mode == kNormNone)
        return hipSuccess;
    return launch_lanes(normalize2_split_kernel, num_blocks, 0, stream, static_cast<uint8_t*>(colours),
                        static_cast<uint8_t*>(indices), num_blocks, color_mode);
}

hipError_t launch_normalize_bc3_split(void* alpha_endpoints, void* alpha_indices, void* color_endpoints, void* color_indices,
                                      uint64_t num_blocks, int alpha_mode, int color_mode, hipStream_t stream)
{
    if (!norm_modes_in_range(kBc3, alpha_mode, color_mode))
        return hipErrorInvalidValue;
    if (num_blocks == 0 || (alpha_mode == kAlphaNone && color_mode == kNormNone))
        return hipSuccess;
    return launch_lanes(normalize3_split_kernel, num_blocks, 0, stream, static_cast<uint8_t*>(alpha_endpoints),
                        static_cast<uint8_t*>(alpha_indices), static_cast<uint8_t*>(color_endpoints),
                        static_cast<uint8_t*>(color_indices), num_blocks, alpha_mode, color_mode);
}

}  // namespace dxtlt
