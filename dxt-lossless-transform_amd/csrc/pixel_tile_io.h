// pixel_tile_io.h -- how the uncompressed-pixel kernels (pixel_kernels.hip, pixel_auto_kernels.hip) move a tile of 4096 pixels
// between global memory, the LDS image and a lane's registers: 16-byte vectors at whatever address they fall on, single bytes for
// what is not a whole vector, bounds checked (the alignment note of pixel_kernels.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace dxtlt {
namespace pixels {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
constexpr int kThreads = 256;

__device__ __forceinline__ u32x4 gload16(const uint8_t* p) { return __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(p)); }
__device__ __forceinline__ void gstore16(uint8_t* p, u32x4 v) { __builtin_nontemporal_store(v, reinterpret_cast<u32x4*>(p)); }

// `bytes` bytes between global memory and the LDS image, lane after lane: whole 16-byte vectors, then single bytes
__device__ __forceinline__ void stage_in(uint8_t* lds, const uint8_t* g, uint32_t bytes)
{
    const uint32_t vecs = bytes / 16;
    for (uint32_t v = threadIdx.x; v < vecs; v += kThreads)
        reinterpret_cast<u32x4*>(lds)[v] = gload16(g + 16 * (uint64_t)v);
    for (uint32_t i = 16 * vecs + threadIdx.x; i < bytes; i += kThreads)
        lds[i] = g[i];
}
__device__ __forceinline__ void stage_out(const uint8_t* lds, uint8_t* g, uint32_t bytes)
{
    const uint32_t vecs = bytes / 16;
    for (uint32_t v = threadIdx.x; v < vecs; v += kThreads)
        gstore16(g + 16 * (uint64_t)v, reinterpret_cast<const u32x4*>(lds)[v]);
    for (uint32_t i = 16 * vecs + threadIdx.x; i < bytes; i += kThreads)
        g[i] = lds[i];
}

// the lane's 16 B bytes of the LDS image
template <int B>
__device__ __forceinline__ void lds_read_pixels(const uint8_t* lds, uint32_t (&w)[4 * B])
{
    const u32x4* p = reinterpret_cast<const u32x4*>(lds) + B * threadIdx.x;
    for (int j = 0; j < B; ++j) {
        const u32x4 v = p[j];
        w[4 * j] = v.x, w[4 * j + 1] = v.y, w[4 * j + 2] = v.z, w[4 * j + 3] = v.w;
    }
}
template <int B>
__device__ __forceinline__ void lds_write_pixels(uint8_t* lds, const uint32_t (&w)[4 * B])
{
    u32x4* p = reinterpret_cast<u32x4*>(lds) + B * threadIdx.x;
    for (int j = 0; j < B; ++j)
        p[j] = u32x4{w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]};
}

// bytes [16 t, 16 t + 16) of one plane of the tile, of which the first `valid` (0..16) exist
__device__ __forceinline__ void plane_store(uint8_t* g, const uint32_t (&p)[4], uint32_t valid)
{
    if (valid >= 16) {
        gstore16(g, u32x4{p[0], p[1], p[2], p[3]});
    } else {
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i)   // (constant register indices)
            if (i < valid)
                g[i] = (uint8_t)(p[i / 4] >> (8 * (i % 4)));
    }
}
__device__ __forceinline__ void plane_load(const uint8_t* g, uint32_t (&p)[4], uint32_t valid)
{
    if (valid >= 16) {
        const u32x4 v = gload16(g);
        p[0] = v.x, p[1] = v.y, p[2] = v.z, p[3] = v.w;
    } else {
        p[0] = p[1] = p[2] = p[3] = 0;
#pragma unroll
        for (uint32_t i = 0; i < 16; ++i)
            if (i < valid)
                p[i / 4] |= (uint32_t)g[i] << (8 * (i % 4));
    }
}

}  // namespace
}  // namespace pixels
}  // namespace dxtlt
