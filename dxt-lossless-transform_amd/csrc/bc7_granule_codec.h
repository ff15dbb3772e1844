// bc7_granule_codec.h -- BC7's codec for the granule sort of granule_sort.h: the record codec of bc7_fields.h over nine classes
// -- mode 0..7 by trailing zeros of byte 0, then the reserved byte-0 == 0 encoding, which is rare, so the ranks of a segment
// without it come from two wave scans instead of ballots.  Included by bc7_kernels.hip (the transform) and, through bc7_image_sinks.h,
// by the image kernels (the inverse with a pixel sink).
#pragma once
#include "bc7_fields.h"
#include "granule_sort.h"

namespace dxtlt {
namespace bc7 {

using granule::kLdsCounts;
using granule::kSegments;
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

}  // namespace bc7
}  // namespace dxtlt
