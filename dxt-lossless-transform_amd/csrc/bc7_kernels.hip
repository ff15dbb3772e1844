// bc7_kernels.hip -- gfx950 kernels of the BC7 granule-sorted field split, version 2 (docs/BC7_FORMAT.md).
//
// A format of this build's own: the reference has no BC7 transform (core/dxt-lossless-transform-bc7/src/lib.rs:1-13);
// it documents the modes' bit fields (assets/research/dds-bc7-blocks.hexpat:286-654), which bc7_fields.h follows.
//
// The granule sort of granule_sort.h (whose header comment says what is computed and how it maps to the machine) over
// BC7's record codec (Bc7Codec, bc7_granule_codec.h).
#include <cstdlib>

#include "bc7_granule_codec.h"

namespace dxtlt {
namespace bc7 {

using granule::BatchEntry;
using granule::forward_granule;
using granule::inverse_granule;
using granule::kT;

// Forward and inverse over a range of full granules (gridDim.x of them from first_block on, aos = the range's first
// block) or, TAIL, over a tail part in one workgroup; the arguments are forward_granule's (granule_sort.h).
template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc7_forward(const uint8_t* __restrict__ aos, uint8_t* __restrict__ soa, uint64_t part_blocks, uint64_t first_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    forward_granule<Bc7Codec, LANES, TAIL>(aos + granule * (kT * 16), soa, part_blocks, first_block + granule * kT, n_tail);
}

template <int LANES, bool TAIL>
__global__ void __launch_bounds__(LANES)
bc7_inverse(const uint8_t* __restrict__ soa, uint8_t* __restrict__ aos, uint64_t part_blocks, uint64_t first_block, int n_tail)
{
    const uint64_t granule = blockIdx.x;
    inverse_granule<Bc7Codec, LANES, TAIL>(soa, aos + granule * (kT * 16), part_blocks, first_block + granule * kT, n_tail);
}

// Many buffers per launch (dxtlt_transform_batch_device / _host with format 7): workgroup b finds its buffer in the
// table -- `coarse[b / 64]` is the entry of workgroup 64 * (b / 64), a short scan from there -- and runs one of its
// granules; the tail parts of all buffers (one workgroup each) go in a second launch over `tails`.
template <bool INVERSE>
__global__ void __launch_bounds__(256)
bc7_batch_granules(const BatchEntry* __restrict__ entries, const uint32_t* __restrict__ coarse, uint32_t n_entries)
{
    const uint32_t b = blockIdx.x;
    uint32_t i = coarse[b >> 6];
    while (i + 1 < n_entries && entries[i + 1].first_wg <= b)
        ++i;
    const BatchEntry e = entries[i];
    const uint64_t granule = b - e.first_wg;
    if constexpr (INVERSE)
        inverse_granule<Bc7Codec, 256, false>(e.src, e.dst + granule * (kT * 16), e.main_blocks, granule * kT, 0);
    else
        forward_granule<Bc7Codec, 256, false>(e.src + granule * (kT * 16), e.dst, e.main_blocks, granule * kT, 0);
}

template <bool INVERSE>
__global__ void __launch_bounds__(256)
bc7_batch_tails(const BatchEntry* __restrict__ tails)
{
    const BatchEntry e = tails[blockIdx.x];   // src / dst: the tail part's first byte on both sides
    if constexpr (INVERSE)
        inverse_granule<Bc7Codec, 256, true>(e.src, e.dst, e.tail, 0, (int)e.tail);
    else
        forward_granule<Bc7Codec, 256, true>(e.src, e.dst, e.tail, 0, (int)e.tail);
}

// Workgroup size: 256 lanes x 4 blocks per lane (DESIGN.md section 8 has the measurements against 512 and 1024 lanes).
hipError_t launch_range(bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block,
                        uint64_t num_blocks, hipStream_t stream)
{
    constexpr int lanes = 256;
    const granule::RangeKernel fwd = bc7_forward<256, false>, inv = bc7_inverse<256, false>;
    return granule::launch_range(lanes, fwd, inv, bc7_forward<256, true>, bc7_inverse<256, true>, inverse, src, dst, total_blocks,
                                 first_block, num_blocks, stream);
}

hipError_t launch_batch(bool inverse, const BatchEntry* d_entries, const uint32_t* d_coarse, uint32_t n_entries,
                        uint32_t granule_wgs, const BatchEntry* d_tails, uint32_t n_tails, hipStream_t stream)
{
    return granule::launch_batch(inverse ? bc7_batch_granules<true> : bc7_batch_granules<false>,
                                 inverse ? bc7_batch_tails<true> : bc7_batch_tails<false>, d_entries, d_coarse, n_entries,
                                 granule_wgs, d_tails, n_tails, stream);
}

}  // namespace bc7
}  // namespace dxtlt
