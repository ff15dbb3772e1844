// batch_tile_plan.h -- the tile launches of a batch plan (host only, pure arithmetic): what plan_batch (batch_api.cpp,
// dxtlt_transform_batch_device) and plan_batch_normalize (batch_normalize_api.cpp, dxtlt_transform_batch_with_normalize_blocks_device)
// share -- one launch per key, its entries laid end to end, the regular-array test and the launch's place in the staged buffer.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "batch_tables.h"
#include "bcn_launch.h"

namespace dxtlt_host {

// One launch of batch_kernel (or batch_norm_kernel): the BC1..BC5 items of one format, direction and settings code that the kernel
// takes.  The kernel is instantiated per settings combination (no run-time switch in front of every tile): a corpus usually has one or two.
struct TileLaunch {
    int key = 0;                     // ((format - 1) * 2 + inverse) << 4 | settings_code
    int norm = 0;                    // the normalising batch call only: 0 = plain launch (batch_kernel); kNormFromArgument (4) = BC2 / BC3
                                     // with the modes in every entry; 1, 2 = BC1 with that colour mode (batch_norm_kernel)
    std::vector<dxtlt::BatchEntry> entries;
    uint32_t wgs = 0;
    uint32_t uniform_wgs = 0;        // workgroups per buffer when all buffers own the same number (the kernel then divides instead
                                     // of looking the entry up), else 0
    bool strided = false;            // a regular array of buffers: one size and tile form, pointers a constant stride apart
    int64_t src_stride = 0, dst_stride = 0;
    bool wide = false;               // the form of its workgroup index, known once fill_tile_tables has built it
    size_t at = 0, entry_bytes = 0;  // in the staged buffer: the entries, then the workgroup index

    dxtlt::Format format() const { return (dxtlt::Format)((key >> 5) + 1); }
    bool inverse() const { return ((key >> 4) & 1) != 0; }
};

// Entry `e` of `wgs` workgroups (plan_batch_entry's answer; e.first_wg = the launch's workgroups so far) joins launch `li` of
// `tiles`, a new launch of `key` and `norm` when li < 0.  false: the launch would reach 2^24 workgroups (fewer than 2^32 threads).
inline bool add_tile_entry(std::vector<TileLaunch>& tiles, int& li, int key, int norm, const dxtlt::BatchEntry& e, uint32_t wgs)
{
    if (li < 0) {
        li = (int)tiles.size();
        tiles.emplace_back();
        tiles.back().key = key;
        tiles.back().norm = norm;
        tiles.back().uniform_wgs = wgs;
    }
    TileLaunch& l = tiles[(size_t)li];
    if ((uint64_t)l.wgs + wgs > 0xFFFFFFull)
        return false;
    l.wgs += wgs;
    l.entries.push_back(e);
    if (wgs != l.uniform_wgs)
        l.uniform_wgs = 0;   // (stays 0: no buffer owns 0 workgroups)
    return true;
}

// The launches in ascending (key, norm), and which of them are regular arrays
inline void order_tile_launches(std::vector<TileLaunch>& tiles)
{
    std::sort(tiles.begin(), tiles.end(), [](const TileLaunch& a, const TileLaunch& b) { return a.key != b.key ? a.key < b.key : a.norm < b.norm; });
    for (TileLaunch& l : tiles) {
        const size_t n = l.entries.size();
        l.strided = l.uniform_wgs != 0;   // (one buffer is a regular array too)
        l.src_stride = n >= 2 ? (int64_t)(l.entries[1].src - l.entries[0].src) : 0;
        l.dst_stride = n >= 2 ? (int64_t)(l.entries[1].dst - l.entries[0].dst) : 0;
        for (size_t i = 1; i < n && l.strided; ++i) {
            const dxtlt::BatchEntry &a = l.entries[0], &b = l.entries[i];
            l.strided = b.blocks == a.blocks && b.full_tiles == a.full_tiles && b.form == a.form && b.halo_vecs == a.halo_vecs &&
                        std::memcmp(b.shift, a.shift, sizeof a.shift) == 0 && std::memcmp(b.gbase, a.gbase, sizeof a.gbase) == 0 &&
                        b.src == a.src + (int64_t)i * l.src_stride && b.dst == a.dst + (int64_t)i * l.dst_stride;
        }
    }
}

// Every launch's tables (entries, then the workgroup index) at 16-byte aligned offsets of the call's ONE staged buffer, from
// table_bytes on
inline void place_tile_tables(std::vector<TileLaunch>& tiles, size_t& table_bytes)
{
    for (TileLaunch& l : tiles) {
        l.entry_bytes = padded(l.entries.size() * sizeof(dxtlt::BatchEntry), 16);
        l.at = table_bytes;
        table_bytes += l.entry_bytes + dxtlt::batch_index_bytes(l.wgs);
    }
}

inline void fill_tile_tables(std::vector<TileLaunch>& tiles, uint8_t* host)
{
    for (TileLaunch& l : tiles) {
        std::memcpy(host + l.at, l.entries.data(), l.entries.size() * sizeof(dxtlt::BatchEntry));
        l.wide = dxtlt::build_batch_index(l.entries.data(), l.entries.size(), l.wgs, host + l.at + l.entry_bytes);
    }
}

// a tile launch as a record of the plan hooks (dxtlt_debug_plan_batch_call, dxtlt_debug_plan_batch_normalize_call)
inline DxtltDebugBatchLaunch tile_launch_record(const TileLaunch& l)
{
    DxtltDebugBatchLaunch r{};
    r.kind = 1, r.format = l.format(), r.inverse = l.inverse() ? 1 : 0, r.settings_code = l.key & 15;
    r.items = r.entries = (uint32_t)l.entries.size(), r.workgroups = l.wgs;
    r.uniform_wgs = l.uniform_wgs, r.strided = l.strided ? 1 : 0, r.wide = l.wide ? 1 : 0;
    r.src_stride = l.src_stride, r.dst_stride = l.dst_stride;
    r.table_offset = l.at, r.table_bytes = l.entry_bytes + dxtlt::batch_index_bytes(l.wgs);
    return r;
}

}  // namespace dxtlt_host
