// batch_norm_kernels.hip -- the tile batch launch with block normalisation fused in (include/dxtlt_batch_normalize.h,
// dxtlt_transform_batch_with_normalize_blocks_device) and the batched "is anything normalisable" classification
// (dxtlt_batch_any_normalizable_device).
//
// batch_norm_kernel is the forward half of batch_kernel (batch_kernels.hip): a workgroup finds its entry through batch_lookup.h
// or, when every buffer owns the same number of workgroups, by the uniform division, rotates the entry's tiles over the XCDs and
// runs the aligned, halo or edge tile of bcn_device.h -- instantiated with NORM, so that a lane normalises its vector in registers
// between the load and the LDS scatter, as the single-buffer fused kernels do (bcn_kernels.hip, bcn_norm23_kernels.hip).
//   BC2 / BC3: NORM == kNormFromArgument.  The modes travel PER ENTRY -- BatchEntry::reserved = pack_norm_modes(alpha_mode,
//              color_mode), bits 24..31 of the `flags` dword load_batch_entry fetches anyway -- so one launch serves any mixture
//              of modes of one (format, settings); they are wave-uniform.  8 + 16 kernels.
//   BC1:       the colour mode (1, 2) is a template parameter of the tile bodies, as in the single-buffer kernels: 16 kernels,
//              one launch per (settings, mode).
// The strided and tiled-array shortcuts of batch_kernel are left out: the table is always read.
//
// A translation unit of its own, as bcn_norm23_kernels.hip is: compiled together with other kernel sets the plain batch kernels'
// schedules change (bcn_kernels.hip).  Resources (compiler's resource report, gfx950): profiles/batch_norm_isa.txt and
// include/dxtlt_batch_normalize.h -- scratch 0 everywhere, LDS the plain batch kernel's, 8 waves / SIMD in all 40 kernels.
#include "bcn_device.h"

#include "batch_lookup.h"
#include "batch_view.h"
#include "launch_grid.h"

namespace dxtlt {

template <int FMT, int VARIANT, bool SA, bool SC, int NORM, int THREADS = batch_tile_threads(FMT, SC, false)>
__global__ void __launch_bounds__(THREADS)
batch_norm_kernel(const BatchEntry* __restrict__ entries_arg, const uint8_t* __restrict__ index_arg, uint32_t n_base, uint32_t uniform_wgs,
                  uint32_t magic)
{
    __shared__ __attribute__((aligned(16))) uint8_t lds[halo_lds_bytes<FMT, THREADS>()];
    const uint32_t wg = blockIdx.x;
    BatchView en;
    uint32_t e;   // index of the buffer in its launch
    // both table pointers in the first scalar round trip, as in batch_kernel
    uint64_t entries_at = reinterpret_cast<uintptr_t>(entries_arg), index_at = reinterpret_cast<uintptr_t>(index_arg);
    asm("" : "+s"(entries_at), "+s"(index_at), "+s"(n_base), "+s"(uniform_wgs), "+s"(magic));
    const BatchEntry* entries = (const BatchEntry*)(const __attribute__((address_space(1))) BatchEntry*)entries_at;
    const uint8_t* index = (const uint8_t*)(global_cptr)index_at;
    if (uniform_wgs != 0) {
        // every buffer owns uniform_wgs workgroups: magic = floor(2^32 / uniform_wgs), exact or one short (launch_batch)
        e = __umulhi(wg, magic);
        if ((e + 1) * uniform_wgs <= wg)
            ++e;
        en = load_batch_entry(entries + e);
    } else {
        e = batch_entry_of_workgroup(entries, index, n_base, magic, wg, en);   // (`magic` carries the entry count in this mode)
    }
    const uint32_t local = batch_rotated_tile(en.first_wg, en.end_wg, e, wg);
    // BC2 / BC3: this entry's modes (pack_norm_modes), uniform over the workgroup; BC1: NORM says it all
    const int norm_modes = NORM == kNormFromArgument ? (int)(en.flags >> 24) : 0;
    const bool aligned = (en.flags & 0xFF) == kBatchAligned;
    if (aligned && local < en.full_tiles) {
        fwd_aligned_tile<FMT, VARIANT, SA, SC, THREADS, NORM>(en.src, en.dst, en.blocks, 0, local, lds, norm_modes);
        return;
    }
    Shifts sh;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        sh.d[i] = (int)((en.shifts[i >> 2] >> (8 * (i & 3))) & 127u);
        sh.gbase[i] = en.gbase[i];
    }
    sh.natural = 1;             // plan_batch_entry hands buffers with other shifts back to the host
    sh.halo_vecs = (int)(en.flags >> 8) & 0xFF;
    sh.full_tiles = en.full_tiles;
    sh.range_blocks = en.blocks;
    // the whole tile first, with a return behind it (batch_kernel has the reason)
    if (local != 0 && local < en.full_tiles) {
        fwd_halo_tile<FMT, VARIANT, SA, SC, NORM, true, THREADS>(en.src, en.dst, en.blocks, 0, sh, local, lds, norm_modes);
        return;
    }
    fwd_halo_edge_tile<FMT, VARIANT, SA, SC, NORM, true, THREADS>(en.src, en.dst, sh, local, lds, norm_modes);
}

namespace {

using BatchNormFn = void (*)(const BatchEntry*, const uint8_t*, uint32_t, uint32_t, uint32_t);

template <int FMT, int VARIANT, bool SA, bool SC>
BatchNormFn norm_fn(int norm)
{
    if constexpr (FMT == kBc1)
        return norm == kNormColor0Only ? batch_norm_kernel<FMT, VARIANT, SA, SC, kNormColor0Only> : batch_norm_kernel<FMT, VARIANT, SA, SC, kNormReplicateColor>;
    else
        return batch_norm_kernel<FMT, VARIANT, SA, SC, kNormFromArgument>;
}

template <int FMT, int VARIANT>
BatchNormFn norm_splits(bool sa, bool sc, int norm)
{
    if constexpr (FMT == kBc3) {
        if (sa)
            return sc ? norm_fn<FMT, VARIANT, true, true>(norm) : norm_fn<FMT, VARIANT, true, false>(norm);
    }
    return sc ? norm_fn<FMT, VARIANT, false, true>(norm) : norm_fn<FMT, VARIANT, false, false>(norm);
}

template <int FMT>
BatchNormFn norm_variant(int variant, bool sa, bool sc, int norm)
{
    switch (variant) {
    case kNone: return norm_splits<FMT, kNone>(sa, sc, norm);
    case kVar1: return norm_splits<FMT, kVar1>(sa, sc, norm);
    case kVar2: return norm_splits<FMT, kVar2>(sa, sc, norm);
    default: return norm_splits<FMT, kVar3>(sa, sc, norm);
    }
}

}  // namespace

uint8_t batch_norm_entry_modes(int alpha_mode, int color_mode) { return (uint8_t)pack_norm_modes(alpha_mode, color_mode); }

hipError_t launch_batch_norm(Format fmt, const Settings& s, const BatchEntry* d_entries, const uint8_t* d_index, uint32_t n_entries,
                             uint32_t total_wgs, uint32_t uniform_wgs, bool wide_index, hipStream_t stream)
{
    if (n_entries == 0 || total_wgs == 0)
        return hipSuccess;
    if (s.variant < 0 || s.variant > 3 || total_wgs > 0xFFFFFFu)
        return hipErrorInvalidValue;
    if (fmt == kBc1 && s.normalize != kNormColor0Only && s.normalize != kNormReplicateColor)
        return hipErrorInvalidValue;
    if (uniform_wgs != 0 && (uint64_t)uniform_wgs * n_entries != total_wgs)
        return hipErrorInvalidValue;
    // as launch_batch: the multiply-high's factor, 2^32 - 1 for one workgroup per buffer, else the bisection's bound
    const uint32_t magic = uniform_wgs > 1 ? (uint32_t)((1ull << 32) / uniform_wgs) : uniform_wgs == 1 ? 0xFFFFFFFFu : n_entries;
    const Settings es = effective_settings(fmt, s);
    BatchNormFn k = nullptr;
    switch (fmt) {
    case kBc1: k = norm_variant<kBc1>(es.variant, false, es.split_colour, s.normalize); break;
    case kBc2: k = norm_variant<kBc2>(es.variant, false, es.split_colour, 0); break;
    case kBc3: k = norm_variant<kBc3>(es.variant, es.split_alpha, es.split_colour, 0); break;
    default: return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(k, dim3(total_wgs), dim3(batch_tile_threads(fmt, es.split_colour, false)), 0, stream, d_entries, d_index,
                       (uint32_t)batch_index_base_count(total_wgs) | (wide_index ? 0x80000000u : 0u), uniform_wgs, magic);
    return hipGetLastError();
}

// ---- dxtlt_batch_any_normalizable_device ------------------------------------------------------------------------------------
// The batched twin of launch_bc{1,2,3}_any_normalizable (normalize_kernels.hip, auto_normalize_kernels.hip): the items' workgroups
// lie end to end, all three formats mixed; a workgroup finds its item by the uniform bisection over first_wg that
// batch_auto_candidates_kernel uses, and every lane classifies one block with the predicates of bc1_normalize.h / bc23_normalize.h.
namespace {

typedef const uint8_t __attribute__((address_space(1))) * GlobalBytes;

// N dwords at p: one vector load when the ITEM's base is on the vector's boundary (uniform), else dword loads, else byte loads
template <int N>
__device__ __forceinline__ void load_dwords(GlobalBytes p, uint32_t base_misalign, uint32_t (&w)[N])
{
    typedef uint32_t vec __attribute__((ext_vector_type(N)));
    if ((base_misalign & (4 * N - 1)) == 0) {
        const vec q = __builtin_nontemporal_load(reinterpret_cast<const vec __attribute__((address_space(1)))*>(p));
#pragma unroll
        for (int k = 0; k < N; ++k)
            w[k] = q[k];
    } else if ((base_misalign & 3) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k)
            w[k] = reinterpret_cast<const uint32_t __attribute__((address_space(1)))*>(p)[k];
    } else {
#pragma unroll
        for (int k = 0; k < N; ++k)
            w[k] = (uint32_t)p[4 * k] | ((uint32_t)p[4 * k + 1] << 8) | ((uint32_t)p[4 * k + 2] << 16) | ((uint32_t)p[4 * k + 3] << 24);
    }
}

__global__ void __launch_bounds__(256)
batch_any_normalizable_kernel(const BatchAnyEntry* __restrict__ tab, uint32_t entries, uint32_t total_wgs, uint32_t* __restrict__ d_flags)
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
    const uint32_t format = tab[lo].format;
    const uint64_t i = uint64_t(wg - tab[lo].first_wg) * 256 + threadIdx.x;   // one block per lane
    const uint32_t misalign = uint32_t(reinterpret_cast<uintptr_t>(in) & 15);
    bool changed = false;
    if (i < n) {
        if (format == kBc1) {
            uint32_t w[2], solid = 0;
            load_dwords<2>(in + 8 * i, misalign, w);
            changed = classify_bc1_block(w[0], w[1], solid) != kBlockUnchanged;
        } else if (format == kBc2) {   // the colour half alone is read
            uint32_t w[2], solid = 0;
            load_dwords<2>(in + 16 * i + 8, misalign, w);
            changed = solid_colour_4c(w[0], w[1], solid);
        } else {
            uint32_t w[4], alpha = 0, solid = 0;
            load_dwords<4>(in + 16 * i, misalign, w);
            changed = uniform_alpha_bc3(w[0], w[1], alpha) || solid_colour_4c(w[2], w[3], solid);
        }
    }
    // one store per wave at most; every writer stores the same value
    if (__ballot(changed) != 0 && (threadIdx.x & 63) == 0)
        d_flags[tab[lo].item] = 1u;
}

}  // namespace

hipError_t launch_batch_any_normalizable(const BatchAnyEntry* d_table, uint32_t entries, uint32_t total_wgs, uint32_t* d_flags,
                                         hipStream_t stream)
{
    if (entries == 0 || total_wgs == 0)
        return hipSuccess;
    dim3 grid;
    if (hipError_t e = grid_of_workgroups(total_wgs, grid); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(batch_any_normalizable_kernel, grid, dim3(256), 0, stream, d_table, entries, total_wgs, d_flags);
    return hipGetLastError();
}

}  // namespace dxtlt
