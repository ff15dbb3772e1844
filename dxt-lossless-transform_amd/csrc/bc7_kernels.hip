// bc7_kernels.hip -- gfx950 kernels of the BC7 granule-sorted field split, version 2 (docs/BC7_FORMAT.md).
//
// A format of this build's own: the reference has no BC7 transform (core/dxt-lossless-transform-bc7/src/lib.rs:1-13);
// it documents the modes' bit fields (assets/research/dds-bc7-blocks.hexpat:286-654), which bc7_fields.h follows.
//
// The granule sort of granule_sort.h (whose header comment says what is computed and how it maps to the machine) over
// BC7's record codec (bc7_fields.h): nine classes -- mode 0..7 by trailing zeros of byte 0, then the reserved
// byte-0 == 0 encoding, which is rare, so the ranks of a segment without it come from two wave scans instead of ballots.
#include <cstdlib>

#include "bc7_fields.h"
#include "granule_sort.h"

namespace dxtlt {
namespace bc7 {

using granule::BatchEntry;
using granule::forward_granule;
using granule::inverse_granule;
using granule::kLdsCounts;
using granule::kSegments;
using granule::kT;
using granule::lds_at;

constexpr int kClasses = 9;   // mode 0..7, then the reserved byte-0 == 0 encoding

// Rank of this lane's block among the blocks of its class in its 64-block segment (= wave instruction), and the class's
// count in the segment: lanes with the same class = AND over the class bits of (bit set ? ballot : ~ballot).
// cls: 0..8, or 9 for lanes beyond a tail part's blocks.  Classes 8 and 9 are rare: the fourth class bit is only
// matched when some lane of the wave has it set (a scalar branch).
__device__ __forceinline__ void rank_in_segment(int cls, int& rank, int& count)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0xFFFFFFFFu;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int sext = __builtin_amdgcn_sbfe(cls, k, 1);   // -1 when bit k is set, else 0
        const uint64_t b = __ballot(sext != 0);
        lo &= ~((uint32_t)b ^ (uint32_t)sext);               // bit set: b, else ~b
        hi &= ~((uint32_t)(b >> 32) ^ (uint32_t)sext);
    }
    const uint64_t high = __ballot(cls >= 8);
    if (high != 0) {
        const uint32_t m = cls >= 8 ? 0xFFFFFFFFu : 0u;
        lo &= ~((uint32_t)high ^ m);
        hi &= ~((uint32_t)(high >> 32) ^ m);
    }
    rank = (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0));
    count = __popc(lo) + __popc(hi);
}

// The same, and the counts into the table, for a segment whose 64 blocks are all of classes 0..7 (the caller checks), with
// a quarter fewer vector instructions: a lane's class as a one-hot byte counter -- classes 0..3 in one dword, 4..7 in a
// second; at most 64 per byte, no carry -- and one inclusive wave scan per dword (four row shifts and two row broadcasts,
// each fused into its add).  The rank is the lane's own byte of its scan value minus one; lane 63's scan value holds every
// class's count, which lanes 0..7 write to the counts table (so no class's "last lane" has to be found).
__device__ __forceinline__ uint32_t wave_scan_add(uint32_t x)
{
    x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, true);    // row_shr:1
    x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, true);    // row_shr:2
    x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, true);    // row_shr:4
    x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, true);    // row_shr:8
    x += __builtin_amdgcn_update_dpp(0, x, 0x142, 0xA, 0xF, false);   // row_bcast:15 into rows 1 and 3
    x += __builtin_amdgcn_update_dpp(0, x, 0x143, 0xC, 0xF, false);   // row_bcast:31 into rows 2 and 3
    return x;
}

__device__ __forceinline__ void rank_by_scan(uint8_t* lds, int cls, int lane, int segment, int& rank)
{
    const uint64_t one = 1ull << (8 * cls);
    const uint32_t a = wave_scan_add((uint32_t)one), b = wave_scan_add((uint32_t)(one >> 32));
    rank = (int)__builtin_amdgcn_ubfe(cls < 4 ? a : b, 8 * cls, 8) - 1;   // the offset operand is taken modulo 32
    const uint32_t ta = __builtin_amdgcn_readlane(a, 63), tb = __builtin_amdgcn_readlane(b, 63);
    if (lane < kClasses)   // lanes 0..7: the segment's count of class `lane`; lane 8: class 8 is absent here (the caller checked)
        lds_at<uint16_t>(lds, kLdsCounts + lane * (kSegments * 2) + segment * 2) =
            lane < 8 ? (uint16_t)__builtin_amdgcn_ubfe(lane < 4 ? ta : tb, 8 * lane, 8) : (uint16_t)0;
}

// (references to the field functions, not wrappers around them: one more call level changes the order of the instructions
// the compiler emits for the record permutations)
struct Bc7Codec {
    static constexpr int kClasses = bc7::kClasses;
    static constexpr int kCountsSpare = 32;   // nothing reads them; they keep the LDS offsets behind the table where they were
    static constexpr auto& block_class = bc7::block_class;
    static constexpr auto& byte0 = record_byte0;
    static constexpr auto& record = record_of_block_any;
    static constexpr auto& block = block_of_record_any;
    // Rank of the lane's block inside its class in this segment, and the segment's class counts into the table.
    template <bool TAIL>
    static __device__ __forceinline__ void rank_and_count(uint8_t* lds, int cls, int lane, int segment, int& rank)
    {
        if (!TAIL && __ballot(cls >= 8) == 0) {
            rank_by_scan(lds, cls, lane, segment, rank);
        } else {
            // the segment's column of the table is written whole by this wave -- zeros first, then the counts that exist (LDS
            // operations of one wave complete in order) -- so the table needs no zero fill and no barrier in front of the ranks
            if (lane < kClasses)
                lds_at<uint16_t>(lds, kLdsCounts + lane * (kSegments * 2) + segment * 2) = 0;
            int count;
            rank_in_segment(cls, rank, count);
            if (rank == count - 1 && cls < kClasses)   // the class's last lane in the segment reports its count
                lds_at<uint16_t>(lds, kLdsCounts + cls * (kSegments * 2) + segment * 2) = (uint16_t)count;
        }
    }
};

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

// Workgroup size: 256 lanes x 4 blocks per lane (DESIGN.md section 8 has the measurements; the experiments side build,
// -DDXTLT_EXPERIMENTS, also carries the 512- and 1024-lane kernels behind DXTLT_BC7_LANES).
hipError_t launch_range(bool inverse, const void* src, void* dst, uint64_t total_blocks, uint64_t first_block,
                        uint64_t num_blocks, hipStream_t stream)
{
#ifdef DXTLT_EXPERIMENTS
    static const int lanes = [] { const char* v = std::getenv("DXTLT_BC7_LANES"); const int x = v ? std::atoi(v) : 0; return x == 512 || x == 1024 ? x : 256; }();
    const granule::RangeKernel fwd = lanes == 1024 ? bc7_forward<1024, false> : lanes == 512 ? bc7_forward<512, false> : bc7_forward<256, false>;
    const granule::RangeKernel inv = lanes == 1024 ? bc7_inverse<1024, false> : lanes == 512 ? bc7_inverse<512, false> : bc7_inverse<256, false>;
#else
    constexpr int lanes = 256;
    const granule::RangeKernel fwd = bc7_forward<256, false>, inv = bc7_inverse<256, false>;
#endif
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
