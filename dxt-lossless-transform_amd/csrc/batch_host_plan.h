// batch_host_plan.h -- the planner of dxtlt_transform_batch_host (batch_host_api.cpp): which items go out alone, how the rest is cut
// into chunks, and every item's slot inside its chunk.  Arithmetic over the item lengths and the chunk cap: no HIP, no address.  The
// call and its test hook (dxtlt_debug_plan_batch_host, tests/test_batch_host_plan.py) run this very function; being pure, it also
// runs stand-alone under the host sanitizers (tests/cpp/batch_host_plan_main.cpp).
//
// Not ChunkPacker (batch_auto_common.h), although both close a chunk BEFORE the item that would push it past the cap: that packer
// closes a chunk that holds items (count > 0), this one a chunk that holds bytes (in_chunk > 0) -- a chunk of empty items alone cuts
// differently -- and it pads slices to 16 bytes where the slots here are padded to 256.  One shared rule would move one caller's
// chunk boundaries.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace dxtlt_host {

constexpr uint32_t kHostBatchAlone = 0xFFFFFFFFu;   // HostBatchPlan::chunk_of_item of an item that goes out alone

struct HostBatchChunk {
    size_t first = 0, count = 0;   // in HostBatchPlan::packed
    uint64_t bytes = 0;            // the padded lengths of its items: what one upload and one download move
};

struct HostBatchPlan {
    std::vector<uint32_t> chunk_of_item;   // per item of the call: its chunk, or kHostBatchAlone
    std::vector<uint64_t> slot;            // per item: where it starts in its chunk, a multiple of 256 -- the same offset in the
                                           // pinned arenas and in the device slots (0 for an item that goes out alone)
    std::vector<size_t> packed;            // the items that travel in chunks, in the call's order
    std::vector<HostBatchChunk> chunks;
    uint64_t arena_bytes = 0;              // the largest chunk
};

inline uint64_t host_batch_padded(uint64_t len) { return (len + 255) & ~uint64_t(255); }

// Items of two chunks or more do not belong in a chunk: the arenas (four pinned ones and two device slots per direction, all of the
// largest chunk's size) would grow to the item's size and the item would move as one unpipelined upload, kernel, download.  They go
// out alone, through the single-buffer host entry points, which run their own chunked pipeline from 96 MiB up.  The rest keeps its
// order.  A chunk is closed BEFORE the item that would push it past the cap, and only when it already holds bytes: so a chunk holds
// at most the cap, or one item of less than two chunks (and empty items, whose slots are 0 bytes long), and arena_bytes stays below
// 3 x the cap whatever the item sizes.  Without an item left to pack there is no chunk; otherwise there is at least one, which
// holds no byte when every packed item is empty.
inline HostBatchPlan plan_host_batch(const uint64_t* len, size_t count, uint64_t chunk_cap_bytes)
{
    HostBatchPlan plan;
    plan.chunk_of_item.assign(count, kHostBatchAlone);
    plan.slot.assign(count, 0);
    const uint64_t alone_from = 2 * chunk_cap_bytes;
    for (size_t i = 0; i < count; ++i)
        if (len[i] < alone_from)
            plan.packed.push_back(i);
    if (plan.packed.empty())
        return plan;
    plan.chunks.emplace_back();
    for (size_t k = 0; k < plan.packed.size(); ++k) {
        const size_t i = plan.packed[k];
        const uint64_t padded = host_batch_padded(len[i]);
        if (plan.chunks.back().bytes > 0 && plan.chunks.back().bytes + padded > chunk_cap_bytes) {
            plan.chunks.emplace_back();
            plan.chunks.back().first = k;
        }
        HostBatchChunk& cur = plan.chunks.back();
        plan.chunk_of_item[i] = (uint32_t)(plan.chunks.size() - 1);
        plan.slot[i] = cur.bytes;
        cur.bytes += padded;
        cur.count++;
        plan.arena_bytes = std::max(plan.arena_bytes, cur.bytes);
    }
    return plan;
}

}  // namespace dxtlt_host
