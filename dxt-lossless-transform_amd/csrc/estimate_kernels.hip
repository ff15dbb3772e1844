// estimate_kernels.hip -- the device-resident size estimator, version 1 of docs/ESTIMATOR.md.
//
//   estimate(section) = L - sum over its 32 KiB windows of the positions i whose 4-byte gram g(i) equals the gram at
//   first[h(g(i))] < i, first[s] = the smallest position of the window whose gram hashes to slot s.
//
// One workgroup per (section, window).  The window is fetched with aligned 16-byte `nt` loads from the 16-byte line its
// first byte lies in (the section base may have any alignment; the up to 15 bytes in front and behind belong to the same
// lines and are never part of a gram) and staged in LDS as it arrives, so position i of the window is LDS byte head + i.
// Grams are built from two aligned LDS dwords with a byte-align shift -- never an unaligned 4-byte DS read (DESIGN §4
// lesson 8).  Pass 1 fills first[] with ds_min_u32 (a minimum: the order in which lanes arrive cannot change it), pass 2
// compares every position's gram with the gram at its slot's first position, a wave reduction and one LDS add per wave
// give the window's matches, and one 64-bit global atomic adds (window bytes - matches) to the section's counter, which
// the launch zeroed on the same stream.  Integer sums: any schedule gives the same number.
//
// LDS at W = 32 KiB, BITS = 14: 32 KiB + 32 bytes of window, 64 KiB of table: one workgroup per CU.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "estimate_launch.h"
#include "estimate_sections.h"

namespace dxtlt {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// T lanes per workgroup; W, BITS: the definition's constants.  The product's estimator is <*, kEstimatorWindow, kEstimatorBits>;
// the other instances exist for the shape sweep of tools/estimator_bench.py (launch_estimate_shape) and define other numbers.
template <int T, uint32_t W, uint32_t BITS>
__global__ void __launch_bounds__(T) estimate_kernel(const EstimateTable tab)
{
    constexpr uint32_t kSlots = 1u << BITS;
    constexpr uint32_t kWindowDwords = W / 4 + 8;   // 15 bytes of head, the window, the rest of its last line, one dword beyond
    auto slot_of = [](uint32_t gram) { return (gram * 2654435761u) >> (32 - BITS); };
    __shared__ __attribute__((aligned(16))) uint32_t win[kWindowDwords];
    __shared__ __attribute__((aligned(16))) uint32_t first[kSlots];
    __shared__ uint32_t wg_matches;

    const uint32_t wg = blockIdx.x, tid = threadIdx.x;
    DXTLT_ESTIMATE_WINDOW_OF(W, tab, wg);   // s, base, off, w: the section table walk of estimate_sections.h

    if (base == nullptr || w < 4) {   // no gram: every byte counts
        if (tid == 0)
            atomicAdd(tab.out + s, (unsigned long long)w);
        return;
    }

    const uintptr_t a = reinterpret_cast<uintptr_t>(base) + off;
    const uint32_t head = uint32_t(a & 15);
    // (a pointer out of a by-value table is generic to the compiler: the address space is restored for global_load)
    typedef const u32x4 __attribute__((address_space(1))) * GlobalVec;
    const GlobalVec src = reinterpret_cast<GlobalVec>(a - head);
    const uint32_t nvec = (head + w + 15) >> 4;   // <= 2049 lines, each holding at least one byte of the window
    for (uint32_t v = tid; v < nvec; v += T)
        reinterpret_cast<u32x4*>(win)[v] = __builtin_nontemporal_load(src + v);
    for (uint32_t i = tid; i < kSlots / 4; i += T)
        reinterpret_cast<u32x4*>(first)[i] = u32x4{~0u, ~0u, ~0u, ~0u};
    if (tid == 0)
        wg_matches = 0;
    __syncthreads();

    // gram positions as LDS byte offsets q = head + i, i in [0, w - 3)
    const uint32_t lo = head, hi = head + w - 3;
    const uint32_t ndw = (hi + 3) >> 2;   // dwords in which a gram starts; win[ndw] is inside the array
    for (uint32_t d = tid; d < ndw; d += T) {
        const uint32_t x = win[d], y = win[d + 1];
        const uint32_t g[4] = {x, __builtin_amdgcn_alignbyte(y, x, 1), __builtin_amdgcn_alignbyte(y, x, 2),
                               __builtin_amdgcn_alignbyte(y, x, 3)};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t q = 4 * d + k;
            if (q >= lo && q < hi)
                atomicMin(&first[slot_of(g[k])], q);
        }
    }
    __syncthreads();

    uint32_t matches = 0;
    for (uint32_t d = tid; d < ndw; d += T) {
        const uint32_t x = win[d], y = win[d + 1];
        const uint32_t g[4] = {x, __builtin_amdgcn_alignbyte(y, x, 1), __builtin_amdgcn_alignbyte(y, x, 2),
                               __builtin_amdgcn_alignbyte(y, x, 3)};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t q = 4 * d + k;
            if (q >= lo && q < hi) {
                const uint32_t f = first[slot_of(g[k])];   // <= q: q itself took part in the minimum
                if (f < q) {
                    const uint32_t fd = f >> 2;
                    matches += __builtin_amdgcn_alignbyte(win[fd + 1], win[fd], f & 3) == g[k];
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        matches += __shfl_down(matches, o);
    if ((tid & 63) == 0 && matches != 0)
        atomicAdd(&wg_matches, matches);
    __syncthreads();
    if (tid == 0)
        atomicAdd(tab.out + s, (unsigned long long)(w - wg_matches));
}

// The same windows from a section table in DEVICE memory with any number of entries (the batched auto transform: thousands of
// sections in one launch).  Entries are in workgroup order; entry e owns workgroups [end_wg of entry e - 1, end_wg) and adds into
// counters[counter].  A workgroup finds its entry by bisection over end_wg (DXTLT_ESTIMATE_TABLE_WINDOW_OF, estimate_sections.h) and then runs
// estimate_kernel's steps on its window, statement for statement.  (A copy, not a shared function: moving the steps into one
// changes the block placement and scalar registers of estimate_kernel's own code, and that kernel's code is pinned.)
template <int T, uint32_t W, uint32_t BITS>
__global__ void __launch_bounds__(T)
estimate_table_kernel(const EstimateTableEntry* __restrict__ tab, uint32_t entries, unsigned long long* __restrict__ counters)
{
    constexpr uint32_t kSlots = 1u << BITS;
    constexpr uint32_t kWindowDwords = W / 4 + 8;
    auto slot_of = [](uint32_t gram) { return (gram * 2654435761u) >> (32 - BITS); };
    __shared__ __attribute__((aligned(16))) uint32_t win[kWindowDwords];
    __shared__ __attribute__((aligned(16))) uint32_t first[kSlots];
    __shared__ uint32_t wg_matches;

    const uint32_t wg = blockIdx.x, tid = threadIdx.x;
    DXTLT_ESTIMATE_TABLE_WINDOW_OF(W, tab, entries, counters, wg);   // base, off, w, out

    if (base == nullptr || w < 4) {   // no gram: every byte counts
        if (tid == 0)
            atomicAdd(out, (unsigned long long)w);
        return;
    }

    const uintptr_t a = reinterpret_cast<uintptr_t>(base) + off;
    const uint32_t head = uint32_t(a & 15);
    typedef const u32x4 __attribute__((address_space(1))) * GlobalVec;
    const GlobalVec src = reinterpret_cast<GlobalVec>(a - head);
    const uint32_t nvec = (head + w + 15) >> 4;
    for (uint32_t v = tid; v < nvec; v += T)
        reinterpret_cast<u32x4*>(win)[v] = __builtin_nontemporal_load(src + v);
    for (uint32_t i = tid; i < kSlots / 4; i += T)
        reinterpret_cast<u32x4*>(first)[i] = u32x4{~0u, ~0u, ~0u, ~0u};
    if (tid == 0)
        wg_matches = 0;
    __syncthreads();

    const uint32_t lo_q = head, hi_q = head + w - 3;
    const uint32_t ndw = (hi_q + 3) >> 2;
    for (uint32_t d = tid; d < ndw; d += T) {
        const uint32_t x = win[d], y = win[d + 1];
        const uint32_t g[4] = {x, __builtin_amdgcn_alignbyte(y, x, 1), __builtin_amdgcn_alignbyte(y, x, 2),
                               __builtin_amdgcn_alignbyte(y, x, 3)};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t q = 4 * d + k;
            if (q >= lo_q && q < hi_q)
                atomicMin(&first[slot_of(g[k])], q);
        }
    }
    __syncthreads();

    uint32_t matches = 0;
    for (uint32_t d = tid; d < ndw; d += T) {
        const uint32_t x = win[d], y = win[d + 1];
        const uint32_t g[4] = {x, __builtin_amdgcn_alignbyte(y, x, 1), __builtin_amdgcn_alignbyte(y, x, 2),
                               __builtin_amdgcn_alignbyte(y, x, 3)};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t q = 4 * d + k;
            if (q >= lo_q && q < hi_q) {
                const uint32_t f = first[slot_of(g[k])];
                if (f < q) {
                    const uint32_t fd = f >> 2;
                    matches += __builtin_amdgcn_alignbyte(win[fd + 1], win[fd], f & 3) == g[k];
                }
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1)
        matches += __shfl_down(matches, o);
    if ((tid & 63) == 0 && matches != 0)
        atomicAdd(&wg_matches, matches);
    __syncthreads();
    if (tid == 0)
        atomicAdd(out, (unsigned long long)(w - wg_matches));
}

template <uint32_t W, uint32_t BITS>
hipError_t launch_shape(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream, int lanes)
{
    return launch_per_section_table<W>(sections, count, d_out, stream, [&](dim3 grid, const EstimateTable& tab) {
        if (lanes == 256)
            hipLaunchKernelGGL((estimate_kernel<256, W, BITS>), grid, dim3(256), 0, stream, tab);
        else if (lanes == 512)
            hipLaunchKernelGGL((estimate_kernel<512, W, BITS>), grid, dim3(512), 0, stream, tab);
        else
            hipLaunchKernelGGL((estimate_kernel<1024, W, BITS>), grid, dim3(1024), 0, stream, tab);
    });
}

}  // namespace

hipError_t launch_estimate(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream)
{
    return launch_shape<kEstimatorWindow, kEstimatorBits>(sections, count, d_out, stream, 1024);
}

hipError_t launch_estimate_table(const EstimateTableEntry* d_table, uint32_t entries, uint32_t workgroups, uint64_t* d_counters,
                                 hipStream_t stream)
{
    if (entries == 0 || workgroups == 0)
        return hipSuccess;
    if (workgroups > 0x7FFFFFFFu)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL((estimate_table_kernel<1024, kEstimatorWindow, kEstimatorBits>), dim3(workgroups), dim3(1024), 0, stream, d_table,
                       entries, reinterpret_cast<unsigned long long*>(d_counters));
    return hipGetLastError();
}

hipError_t launch_estimate_shape(const EstimateSection* sections, size_t count, uint64_t* d_out, hipStream_t stream, int lanes,
                                 uint32_t window, uint32_t bits)
{
    if (lanes != 256 && lanes != 512 && lanes != 1024)
        return hipErrorInvalidValue;
    if (window == 32768 && bits == 14)
        return launch_shape<32768, 14>(sections, count, d_out, stream, lanes);
    if (window == 32768 && bits == 13)
        return launch_shape<32768, 13>(sections, count, d_out, stream, lanes);
    if (window == 16384 && bits == 13)
        return launch_shape<16384, 13>(sections, count, d_out, stream, lanes);
    if (window == 8192 && bits == 12)
        return launch_shape<8192, 12>(sections, count, d_out, stream, lanes);
    return hipErrorInvalidValue;
}

}  // namespace dxtlt
