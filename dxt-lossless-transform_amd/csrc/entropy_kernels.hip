// entropy_kernels.hip -- the entropy estimator, "The entropy estimator, version 1" of docs/ESTIMATOR.md.
//
//   q(window) = max(0, n T[n] - sum over byte values v of c[v] T[c[v]])     n bytes, byte counts c[], T[k] = floor(2^16 log2 k)
//   estimate(section) = (sum of q over its 32 KiB windows + 2^19 - 1) >> 19
//
// One workgroup of 256 lanes per (section, window), found through the section table walk the gram estimator uses
// (estimate_sections.h).  The window is read once: the bytes in front of its first 16-byte boundary and behind its last one by
// one lane each, everything between as aligned 16-byte `nt` vectors, at most eight per lane, all issued before the first is
// counted -- no byte outside the section is touched, whatever its base.  The histogram lives in LDS, privatised sixteen ways by
// lane: hist[v * 16 + (lane & 15)], so the sixteen copies of a value lie in sixteen banks and a constant window -- the alpha
// plane of an opaque texture: the common case -- sends a wave to sixteen addresses, not to one.  A dword of four equal bytes adds
// 4 once.  Then lane v sums the copies of value v, looks c T[c] up in the table (128 KiB, read-only, resident in L2), a wave
// reduction and four LDS words give the window's sum, and one 64-bit global atomic adds q to the section's counter, which the
// launch zeroed on the same stream.  A finishing launch rounds the counters up to bytes in place.  Integer sums: any schedule
// gives the same number.
//
// LDS 16 KiB + 32 bytes; no scratch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "entropy_launch.h"
#include "estimate_sections.h"

namespace dxtlt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLanes = 256, kCopies = 16;
constexpr uint32_t kVectorsPerLane = kEntropyWindow / 16 / kLanes;   // 8
static_assert(kVectorsPerLane * kLanes * 16 == kEntropyWindow, "a window is a whole number of vectors per lane");

__device__ const uint32_t d_entropy_table[kEntropyWindow + 1] = {
#include "entropy_table.h"
};
const uint32_t h_entropy_table[kEntropyWindow + 1] = {
#include "entropy_table.h"
};

// One window -- `w` > 0 bytes at byte `off` of the section at `base` -- counted by the workgroup, its q added to *(out): the steps of
// both kernels below, expanded in place with `hist`, `wave_sum` and `tid` in scope.  A macro, not a function, for the reason
// DXTLT_ESTIMATE_WINDOW_OF (estimate_sections.h) gives: entropy_kernel's code is pinned.
#define DXTLT_ENTROPY_WINDOW(base, off, w, out) \
    do {                                                                                                                                   \
        const uintptr_t a = reinterpret_cast<uintptr_t>(base) + off;                                                                       \
        const uint32_t to_line = uint32_t(-a) & 15;                                                                                        \
        const uint32_t head = to_line < w ? to_line : w; /* bytes in front of the first 16-byte boundary */                                \
        const uint32_t nvec = (w - head) >> 4; /* <= 2048 whole lines inside the window */                                                 \
        const uint32_t tail = w - head - 16 * nvec; /* < 16 bytes behind the last of them */                                               \
        /* (a pointer out of a by-value table is generic to the compiler: the address space is restored for global_load) */                \
        typedef const u32x4 __attribute__((address_space(1))) * GlobalVec;                                                                 \
        typedef const uint8_t __attribute__((address_space(1))) * GlobalByte;                                                              \
        const GlobalVec src = reinterpret_cast<GlobalVec>(a + head);                                                                       \
        const GlobalByte bytes = reinterpret_cast<GlobalByte>(a);                                                                          \
                                                                                                                                           \
        /* every load first.  A lane without a k-th vector loads the window's last one again (inside the section, never counted): no */    \
        /* branch around a load, so all eight are in flight together. */                                                                   \
        u32x4 v[kVectorsPerLane];                                                                                                          \
        if (nvec != 0) {                                                                                                                   \
        _Pragma("unroll")                                                                                                                  \
            for (uint32_t k = 0; k < kVectorsPerLane; ++k) {                                                                               \
                const uint32_t i = tid + k * kLanes;                                                                                       \
                v[k] = __builtin_nontemporal_load(src + (i < nvec ? i : nvec - 1));                                                        \
            }                                                                                                                              \
        }                                                                                                                                  \
        uint32_t edge = 0; /* lanes [0, head): a head byte; lanes [16, 16 + tail): a tail byte */                                          \
        if (tid < head)                                                                                                                    \
            edge = bytes[tid];                                                                                                             \
        else if (tid >= 16 && tid - 16 < tail)                                                                                             \
            edge = bytes[head + 16 * nvec + (tid - 16)];                                                                                   \
                                                                                                                                           \
        _Pragma("unroll")                                                                                                                  \
        for (uint32_t k = 0; k < 256 * kCopies / 4 / kLanes; ++k)                                                                          \
            reinterpret_cast<u32x4*>(hist)[tid + k * kLanes] = u32x4{0, 0, 0, 0};                                                          \
        __syncthreads();                                                                                                                   \
                                                                                                                                           \
        uint32_t* mine = hist + (tid & (kCopies - 1));                                                                                     \
        auto count_dword = [&](uint32_t x) {                                                                                               \
            const uint32_t b0 = x & 0xFF;                                                                                                  \
            if (x == b0 * 0x01010101u) {                                                                                                   \
                atomicAdd(mine + b0 * kCopies, 4u);                                                                                        \
            } else {                                                                                                                       \
                atomicAdd(mine + b0 * kCopies, 1u);                                                                                        \
                atomicAdd(mine + ((x >> 8) & 0xFF) * kCopies, 1u);                                                                         \
                atomicAdd(mine + ((x >> 16) & 0xFF) * kCopies, 1u);                                                                        \
                atomicAdd(mine + (x >> 24) * kCopies, 1u);                                                                                 \
            }                                                                                                                              \
        };                                                                                                                                 \
        if (nvec != 0) {                                                                                                                   \
        _Pragma("unroll")                                                                                                                  \
            for (uint32_t k = 0; k < kVectorsPerLane; ++k)                                                                                 \
                if (tid + k * kLanes < nvec) {                                                                                             \
                    count_dword(v[k].x);                                                                                                   \
                    count_dword(v[k].y);                                                                                                   \
                    count_dword(v[k].z);                                                                                                   \
                    count_dword(v[k].w);                                                                                                   \
                }                                                                                                                          \
        }                                                                                                                                  \
        if (tid < head || (tid >= 16 && tid - 16 < tail))                                                                                  \
            atomicAdd(mine + edge * kCopies, 1u);                                                                                          \
        __syncthreads();                                                                                                                   \
                                                                                                                                           \
        /* lane v: c[v] from its sixteen copies, then c T[c] (c <= 32768, T < 2^20: the product needs 64 bits) */                          \
        uint32_t c = 0;                                                                                                                    \
        _Pragma("unroll")                                                                                                                  \
        for (uint32_t k = 0; k < kCopies / 4; ++k) {                                                                                       \
            const u32x4 part = reinterpret_cast<const u32x4*>(hist)[tid * (kCopies / 4) + k];                                              \
            c += part.x + part.y + part.z + part.w;                                                                                        \
        }                                                                                                                                  \
        unsigned long long sum = (unsigned long long)c * d_entropy_table[c];                                                               \
        for (int o = 32; o > 0; o >>= 1)                                                                                                   \
            sum += __shfl_down(sum, o);                                                                                                    \
        if ((tid & 63) == 0)                                                                                                               \
            wave_sum[tid >> 6] = sum;                                                                                                      \
        __syncthreads();                                                                                                                   \
        if (tid == 0) {                                                                                                                    \
            unsigned long long all = 0;                                                                                                    \
        _Pragma("unroll")                                                                                                                  \
            for (uint32_t k = 0; k < kLanes / 64; ++k)                                                                                     \
                all += wave_sum[k];                                                                                                        \
            const unsigned long long whole = (unsigned long long)w * d_entropy_table[w];                                                   \
            if (whole > all)                                                                                                               \
                atomicAdd(out, whole - all);                                                                                               \
        }                                                                                                                                  \
    } while (0)

__global__ void __launch_bounds__(kLanes) entropy_kernel(const EstimateTable tab)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[256 * kCopies];
    __shared__ unsigned long long wave_sum[kLanes / 64];

    const uint32_t wg = blockIdx.x, tid = threadIdx.x;
    DXTLT_ESTIMATE_WINDOW_OF(kEntropyWindow, tab, wg);   // s, base, off, w
    if (base == nullptr || w == 0)   // (uniform) nothing to count: the section's counter stays as it is
        return;
    DXTLT_ENTROPY_WINDOW(base, off, w, tab.out + s);
}

// The same windows from a section table in DEVICE memory with any number of entries (the batched pixel auto transform: six
// sections per buffer, thousands of buffers, one launch): the entry by the bisection of estimate_table_kernel
// (DXTLT_ESTIMATE_TABLE_WINDOW_OF), then the window as above, q added to counters[entry.counter].  Sums only: the caller rounds
// (launch_entropy_finish, or on the host).
__global__ void __launch_bounds__(kLanes)
entropy_table_kernel(const EstimateTableEntry* __restrict__ tab, uint32_t entries, unsigned long long* __restrict__ counters)
{
    __shared__ __attribute__((aligned(16))) uint32_t hist[256 * kCopies];
    __shared__ unsigned long long wave_sum[kLanes / 64];

    const uint32_t wg = blockIdx.x, tid = threadIdx.x;
    DXTLT_ESTIMATE_TABLE_WINDOW_OF(kEntropyWindow, tab, entries, counters, wg);   // base, off, w, out
    if (base == nullptr || w == 0)
        return;
    DXTLT_ENTROPY_WINDOW(base, off, w, out);
}

__global__ void __launch_bounds__(64) entropy_finish_kernel(unsigned long long* __restrict__ sums, uint32_t count)
{
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i < count)
        sums[i] = (sums[i] + ((1ull << kEntropyShift) - 1)) >> kEntropyShift;
}

}  // namespace

hipError_t launch_entropy(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    if (count > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    hipError_t e = launch_per_section_table<kEntropyWindow>(sections, count, d_out, stream, [&](dim3 grid, const EstimateTable& tab) {
        hipLaunchKernelGGL(entropy_kernel, grid, dim3(kLanes), 0, stream, tab);
    });
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(entropy_finish_kernel, dim3(uint32_t((count + 63) / 64)), dim3(64), 0, stream,
                       reinterpret_cast<unsigned long long*>(d_out), uint32_t(count));
    return hipGetLastError();
}

hipError_t launch_entropy_table(const EstimateTableEntry* d_table, uint32_t entries, uint32_t workgroups, uint64_t* d_counters,
                                hipStream_t stream)
{
    if (entries == 0 || workgroups == 0)
        return hipSuccess;
    if (workgroups > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(entropy_table_kernel, dim3(workgroups), dim3(kLanes), 0, stream, d_table, entries,
                       reinterpret_cast<unsigned long long*>(d_counters));
    return hipGetLastError();
}

hipError_t launch_entropy_finish(uint64_t* d_counters, size_t count, hipStream_t stream)
{
    if (count == 0)
        return hipSuccess;
    if (count > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(entropy_finish_kernel, dim3(uint32_t((count + 63) / 64)), dim3(64), 0, stream,
                       reinterpret_cast<unsigned long long*>(d_counters), uint32_t(count));
    return hipGetLastError();
}

uint32_t entropy_table_host(uint32_t k) { return k <= kEntropyWindow ? h_entropy_table[k] : 0u; }

}  // namespace dxtlt
