// array_op_plan.h -- which route a stand-alone array operation takes, decided in ONE place: the colour-array kernels of
// color565_ops.hip and the block decode / pixel-difference kernels of bcn_decode.hip.  Pure host arithmetic on addresses and a
// count: nothing is dereferenced and no device is needed, so the CPU tests ask the same function through
// dxtlt_debug_plan_array_op (include/dxtlt_decode.h) that the launch functions ask.  The two host slice sizes of decode_api.cpp
// are named here as well, for the loops and for dxtlt_debug_array_op_slices.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace dxtlt {

constexpr int kArrayOpThreads = 256;                 // lanes per workgroup of every kernel planned here
constexpr uint64_t kDifferenceGrid = 256 * 16;       // workgroups of the difference count at the most: 16 per CU
// two blocks per lane and step: four loads in flight per lane.  Four blocks (eight loads) were slower on the sparse
// case -- BC2 0.673 against 0.697 of peak, BC3 0.626 against 0.666 -- and one block no better (0.667 / 0.652): more bytes
// in flight per CU than the memory system likes lower the rate (launch_grid.h)
constexpr int kDifferenceBlocksPerLane = 2;

constexpr size_t kDecodeSliceBlocks = size_t(4) << 20;        // decode_host: 256 MiB of pixels per slice
constexpr size_t kDifferenceSliceBytes = size_t(256) << 20;   // dxtlt_count_pixel_differences: a multiple of both block sizes

// the values of `op` (DXTLT_ARRAY_OP_* of include/dxtlt_decode.h)
enum ArrayOp : int {
    kOpYcocg = 0,             // addr0 = in, addr1 = out; count = colours
    kOpRecorrelateSplit = 1,  // addr0 = src0, addr1 = src1, addr2 = dst; count = colour PAIRS
    kOpSplitEndpoints = 2,    // addr0 = in, addr1 = out; count = colour PAIRS
    kOpDecodeBc1 = 11,        // 11..13: addr0 = blocks, addr1 = pixels; count = blocks
    kOpDecodeBc2 = 12,
    kOpDecodeBc3 = 13,
    kOpDifferenceBc1 = 21,    // 21..23: addr0 = a, addr1 = b; count = blocks
    kOpDifferenceBc2 = 22,
    kOpDifferenceBc3 = 23,
};

struct ArrayOpPlan {
    int32_t vector;         // 1: the vector route (colour arrays: 16-byte lanes; decode: staged through LDS; difference: vector loads)
    int32_t threads;        // lanes per workgroup
    uint64_t vector_lanes;  // colour arrays: lanes that take one 16-byte vector of output; decode / difference: blocks, when vector
    uint64_t single_lanes;  // colour arrays: lanes that take one colour (ycocg) or one pair; decode / difference: blocks, when not
    uint64_t workgroups;
    uint64_t steps;         // difference: grid steps of the busiest workgroup (workgroup 0); every other launch: 1
};

inline bool plan_aligned(uint64_t address, uint64_t a) { return (address & (a - 1)) == 0; }

// false: `op` is none of ArrayOp.  count == 0 plans no launch (all zero).
inline bool plan_array_op(int op, uint64_t addr0, uint64_t addr1, uint64_t addr2, uint64_t count, ArrayOpPlan& p)
{
    p = ArrayOpPlan{0, kArrayOpThreads, 0, 0, 0, 0};
    uint64_t per_vector = 0;   // elements of `count` per vector lane; 0: one lane per element on either route
    switch (op) {
    case kOpYcocg:
        p.vector = plan_aligned(addr0, 16) && plan_aligned(addr1, 16);
        per_vector = 8;
        break;
    case kOpRecorrelateSplit:
        p.vector = plan_aligned(addr0, 8) && plan_aligned(addr1, 8) && plan_aligned(addr2, 16);
        per_vector = 4;
        break;
    case kOpSplitEndpoints:
        // both halves of the output must be 16-byte aligned for the vector path: out and out + 2 * pairs
        p.vector = plan_aligned(addr0, 16) && plan_aligned(addr1, 16) && count % 8 == 0;
        per_vector = 8;
        break;
    case kOpDecodeBc1:
    case kOpDecodeBc2:
    case kOpDecodeBc3:
        p.vector = plan_aligned(addr0, op == kOpDecodeBc1 ? 8 : 16) && plan_aligned(addr1, 16);
        break;
    case kOpDifferenceBc1:
    case kOpDifferenceBc2:
    case kOpDifferenceBc3: {
        const uint64_t al = op == kOpDifferenceBc1 ? 8 : 16;
        p.vector = plan_aligned(addr0, al) && plan_aligned(addr1, al);
        break;
    }
    default:
        return false;
    }
    if (count == 0) {
        p.vector = 0;
        return true;
    }
    if (per_vector != 0) {
        p.vector_lanes = p.vector ? count / per_vector : 0;
        p.single_lanes = count - per_vector * p.vector_lanes;
    } else {
        (p.vector ? p.vector_lanes : p.single_lanes) = count;
    }
    p.steps = 1;
    if (op >= kOpDifferenceBc1) {
        const uint64_t per_wg = (uint64_t)kArrayOpThreads * kDifferenceBlocksPerLane;
        const uint64_t wgs = (count + per_wg - 1) / per_wg;
        p.workgroups = wgs > kDifferenceGrid ? kDifferenceGrid : wgs;
        const uint64_t stride = p.workgroups * per_wg;
        p.steps = (count + stride - 1) / stride;
    } else {
        p.workgroups = (p.vector_lanes + p.single_lanes + kArrayOpThreads - 1) / kArrayOpThreads;
    }
    return true;
}

}  // namespace dxtlt
