// image_planned_launch.h -- the host side that the fused image kernels share (image_kernels.hip: one image per call;
// image_regions_kernels.hip: several images of one buffer): the inverse transform's own plan for a block range, enqueued with
// kernels whose block store is a sink that writes pixels.
#pragma once
#include <algorithm>

#include "bcn_device.h"
#include "bcn_launch.h"

namespace dxtlt {

template <typename SINK>
struct ImageKernelsOf {
    void (*tiled)(const uint8_t*, SINK, uint64_t, uint64_t);             // default_tile_threads(fmt, true) lanes
    void (*shifted)(const uint8_t*, SINK, uint64_t, uint64_t, Shifts);   // shift_tile_threads(fmt) lanes
};

constexpr uint64_t kMaxBlocksPerImageLaunch = 1ull << 31;   // launch_transform's sub-ranges

// The launches of the inverse transform's own plan for blocks [first_block, first_block + n) -- `s` the format's effective
// settings -- with the kernels `ks`, whose sink is make_sink(k) for a launch whose first block is block first_block + k
template <typename SINK, typename MAKE_SINK>
hipError_t launch_planned_image(Format fmt, const Settings& s, const ImageKernelsOf<SINK>& ks, const void* soa, uint64_t total_blocks,
                                uint64_t first_block, uint64_t n, hipStream_t stream, const MAKE_SINK& make_sink)
{
    const auto* soa8 = static_cast<const uint8_t*>(soa);
    for (uint64_t off = 0; off < n; off += kMaxBlocksPerImageLaunch) {
        const Range sub{total_blocks, first_block + off, std::min(kMaxBlocksPerImageLaunch, n - off)};
        // the inverse transform's own plan for the sub-range (the block side's address plays no part in it): aligned tiles
        // and an edge tile behind them, or shifted tiles with theirs
        constexpr int kCap = 8;
        DebugPlannedLaunch plan[kCap];
        const int launches = debug_plan_transform(fmt, true, s, reinterpret_cast<uintptr_t>(soa), 0, sub, nullptr, plan, kCap);
        if (launches < 0 || launches > kCap)
            return hipErrorInvalidValue;
        for (int i = 0; i < launches; ++i) {
            const DebugPlannedLaunch& l = plan[i];
            const SINK sink = make_sink(off + l.aos_offset / (uint64_t)fmt_block(fmt));
            if (l.kind == 0) {
                if (l.threads != default_tile_threads(fmt, true))
                    return hipErrorInvalidValue;
                hipLaunchKernelGGL(ks.tiled, dim3(l.workgroups), dim3(l.threads), 0, stream, soa8, sink, total_blocks, sub.first_block);
            } else {
                if (l.kind != 2 || l.threads != shift_tile_threads(fmt))
                    return hipErrorInvalidValue;
                Shifts sh{};
                for (int k = 0; k < 6; ++k) {
                    sh.d[k] = l.shift[k];
                    sh.gbase[k] = l.gbase[k];
                }
                sh.natural = l.natural;
                sh.halo_vecs = l.halo_vecs;
                sh.full_tiles = l.full_tiles;
                sh.range_blocks = l.range_blocks;
                hipLaunchKernelGGL(ks.shifted, dim3(l.workgroups), dim3(l.threads), 0, stream, soa8, sink, total_blocks, sub.first_block, sh);
            }
            if (hipError_t e = hipGetLastError(); e != hipSuccess)
                return e;
        }
    }
    return hipSuccess;
}

}  // namespace dxtlt
