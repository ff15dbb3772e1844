// batch_normalize_api.cpp -- include/dxtlt_batch_normalize.h: dxtlt_transform_batch_with_normalize_blocks_device (block
// normalisation fused into the forward transform, many buffers per call) and dxtlt_batch_any_normalizable_device (which of many
// buffers hold a block that normalisation would touch).
//
// The transform call is dxtlt_transform_batch_device's forward half with per-item modes: planned whole by one pure function
// (plan_batch_normalize), its tables staged in ONE slot of the thread's ring (StagedTables, batch_tables.h) and uploaded once, then
//   * items whose modes are all None through the plain launch_batch, grouped as the plain call groups them: the plain call's bytes
//     from the plain call's kernels;
//   * BC2 / BC3 items with a mode set in ONE launch_batch_norm per (format, settings code), the modes in every entry;
//   * BC1 items with a mode set in one launch_batch_norm per (settings code, colour mode);
//   * items plan_batch_entry hands back (a transformed-side pointer off its element width) alone through launch_transform with
//     Settings::normalize / normalize_alpha, behind the batch launches.
// The tile launches go out in ascending (format, settings code, plain before normalising, BC1 colour mode).
#include <hip/hip_runtime_api.h>

#include <cstring>
#include <vector>

#include "../../include/dxtlt_batch_normalize.h"
#include "batch_tables.h"
#include "batch_tile_plan.h"
#include "bcn_launch.h"
#include "host_common.h"

namespace {

using namespace dxtlt_host;
using dxtlt::BatchEntry;

constexpr int kNormPerEntry = 4;   // TileLaunch::norm of a BC2 / BC3 normalising launch (bcn_device.h: kNormFromArgument)

// What both calls read of an item: format, len and the input pointer, in batch_item_defect's order and style
int32_t source_defect(const DxtltBatchNormalizeItem& it)
{
    if (it.format < 1 || it.format > 3)
        return fail(kInvalidArgument, "batch normalize item: format must be 1, 2 or 3 (BC1, BC2, BC3)");
    if (it.len % item_block_bytes(it.format) != 0)
        return fail(kInvalidLength, "batch normalize item: len is not a multiple of the block size");
    return kOk;
}

int32_t item_defect(const DxtltBatchNormalizeItem& it)
{
    if (int32_t rc = source_defect(it); rc != kOk)
        return rc;
    if (it.decorrelation_mode > 3)
        return fail(kInvalidArgument, "batch normalize item: decorrelation_mode must be 0..3");
    if (it.color_mode > dxtlt::norm_limits(it.format).colour)
        return fail(kInvalidArgument, "batch normalize item: color_mode must be 0..2");
    if (it.format == 3 && it.alpha_mode > dxtlt::norm_limits(3).alpha)
        return fail(kInvalidArgument, "batch normalize item: alpha_mode must be 0..3");
    if (it.len > 0 && (it.d_input == nullptr || it.d_output == nullptr))
        return fail(kInvalidArgument, "batch normalize item: NULL device buffer with len > 0");
    return kOk;
}

// the settings an item's kernels are instantiated with, its modes included (alpha_mode: BC3 only)
dxtlt::Settings item_settings(const DxtltBatchNormalizeItem& it)
{
    dxtlt::Settings s{};
    s.variant = it.decorrelation_mode;
    s.split_alpha = it.split_alpha_endpoints != 0;
    s.split_colour = it.split_colour_endpoints != 0;
    s = dxtlt::effective_settings((dxtlt::Format)it.format, s);
    s.normalize = it.color_mode;
    s.normalize_alpha = it.format == 3 ? it.alpha_mode : 0;
    return s;
}

struct NormalizePlan {
    std::vector<TileLaunch> tiles;   // present launches only, ascending (key, norm)
    std::vector<size_t> singles;     // items the batch kernels do not take: launched alone, behind the batches
    size_t table_bytes = 0;
};

// Validates the batch as a whole and plans it; nothing is enqueued, no device is touched, no address is dereferenced
int32_t plan_batch_normalize(const DxtltBatchNormalizeItem* items, size_t count, NormalizePlan& plan)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    for (size_t i = 0; i < count; ++i)
        if (int32_t rc = item_defect(items[i]); rc != kOk)
            return rc;
    int launch_of[3 * 16][kNormPerEntry + 1];   // format and settings code; TileLaunch::norm
    for (auto& row : launch_of)
        for (int& l : row)
            l = -1;
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchNormalizeItem& it = items[i];
        if (it.len == 0)
            continue;
        if (it.len >= (size_t(64) << 30))
            return fail(kInvalidArgument, "batch normalize item of 64 GiB or more: use the single-buffer entry point");
        const dxtlt::Settings s = item_settings(it);
        const int code = settings_code(s);
        const int norm = s.normalize == 0 && s.normalize_alpha == 0 ? 0 : it.format == 1 ? s.normalize : kNormPerEntry;
        int& li = launch_of[(it.format - 1) * 16 + code][norm];
        BatchEntry e{};
        e.src = static_cast<const uint8_t*>(it.d_input);
        e.dst = static_cast<uint8_t*>(it.d_output);
        e.blocks = it.len / item_block_bytes(it.format);
        e.first_wg = li >= 0 ? plan.tiles[(size_t)li].wgs : 0;
        const uint32_t wgs = dxtlt::plan_batch_entry((dxtlt::Format)it.format, false, s, e);
        if (wgs == 0xFFFFFFFFu) {
            plan.singles.push_back(i);
            continue;
        }
        if (norm == kNormPerEntry)
            e.reserved = dxtlt::batch_norm_entry_modes(s.normalize_alpha, s.normalize);
        if (!add_tile_entry(plan.tiles, li, ((it.format - 1) * 2) << 4 | code, norm, e, wgs))
            return fail(kInvalidArgument, "batch too large for one launch (64 GiB or more of one format, settings and kind of launch)");
    }
    order_tile_launches(plan.tiles);
    place_tile_tables(plan.tiles, plan.table_bytes);
    return kOk;
}

// ---- dxtlt_batch_any_normalizable_device: one entry per non-empty item, ceil(blocks / 256) workgroups each ----
struct AnyPlan {
    std::vector<dxtlt::BatchAnyEntry> entries;
    uint32_t wgs = 0;
};

int32_t plan_any(const DxtltBatchNormalizeItem* items, size_t count, AnyPlan& plan)
{
    for (size_t i = 0; i < count; ++i) {
        if (int32_t rc = source_defect(items[i]); rc != kOk)
            return rc;
        if (items[i].len > 0 && items[i].d_input == nullptr)
            return fail(kInvalidArgument, "batch normalize item: NULL device buffer with len > 0");
    }
    for (size_t i = 0; i < count; ++i) {
        const DxtltBatchNormalizeItem& it = items[i];
        if (it.len == 0)
            continue;
        if (it.len >= (size_t(64) << 30))
            return fail(kInvalidArgument, "batch normalize item of 64 GiB or more: use the single-buffer entry point");
        const uint64_t blocks = it.len / item_block_bytes(it.format), wgs = (blocks + 255) / 256;
        if (plan.wgs + wgs > 0xFFFFFFull)
            return fail(kInvalidArgument, "batch too large for one launch (2^24 workgroups of 256 blocks or more)");
        plan.entries.push_back({static_cast<const uint8_t*>(it.d_input), blocks, plan.wgs, it.format, (uint32_t)i, 0});
        plan.wgs += (uint32_t)wgs;
    }
    return kOk;
}

}  // namespace

extern "C" int32_t dxtlt_transform_batch_with_normalize_blocks_device(const DxtltBatchNormalizeItem* items, size_t count, void* hip_stream)
{
    NormalizePlan plan;
    if (int32_t rc = plan_batch_normalize(items, count, plan); rc != kOk)
        return rc;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);
    if (plan.table_bytes != 0) {
        StagedTables tables;
        hipError_t e = tables.acquire(plan.table_bytes);
        if (e != hipSuccess)
            return fail(kDevice, "batch normalize table staging", e);
        fill_tile_tables(plan.tiles, tables.host());
        e = tables.upload(user);
        for (size_t k = 0; k < plan.tiles.size() && e == hipSuccess; ++k) {
            const TileLaunch& l = plan.tiles[k];
            const uint8_t* d = tables.dev() + l.at;
            dxtlt::Settings s = settings_of_code(l.key & 15);
            if (l.norm == 0) {
                e = dxtlt::launch_batch(l.format(), false, s, reinterpret_cast<const BatchEntry*>(d), d + l.entry_bytes, (uint32_t)l.entries.size(),
                                        l.wgs, l.uniform_wgs, l.wide, user, l.strided ? &l.entries[0] : nullptr, l.src_stride, l.dst_stride);
            } else {
                s.normalize = l.norm == kNormPerEntry ? 0 : l.norm;   // BC1: the launch's mode; BC2 / BC3: in the entries
                e = dxtlt::launch_batch_norm(l.format(), s, reinterpret_cast<const BatchEntry*>(d), d + l.entry_bytes, (uint32_t)l.entries.size(),
                                             l.wgs, l.uniform_wgs, l.wide, user);
            }
        }
        if (int32_t rc = tables.finish(e, user, "batch normalize table copy / launch", "batch normalize event"); rc != kOk)
            return rc;
    }
    for (size_t i : plan.singles) {
        const DxtltBatchNormalizeItem& it = items[i];
        const uint64_t blocks = it.len / item_block_bytes(it.format);
        HIP_TRY(dxtlt::launch_transform((dxtlt::Format)it.format, false, item_settings(it), it.d_input, it.d_output,
                                        dxtlt::Range{blocks, 0, blocks}, user),
                "batch normalize item launch");
    }
    return kOk;
}

extern "C" int32_t dxtlt_batch_any_normalizable_device(const DxtltBatchNormalizeItem* items, size_t count, uint32_t* d_flags, void* hip_stream)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    if (d_flags == nullptr)
        return fail(kInvalidArgument, "NULL flag array with count > 0");
    AnyPlan plan;
    if (int32_t rc = plan_any(items, count, plan); rc != kOk)
        return rc;
    hipStream_t user = static_cast<hipStream_t>(hip_stream);
    HIP_TRY(hipMemsetAsync(d_flags, 0, count * sizeof(uint32_t), user), "batch any-normalizable flag reset");
    if (plan.entries.empty())
        return kOk;
    StagedTables tables;
    const size_t bytes = plan.entries.size() * sizeof(dxtlt::BatchAnyEntry);   // (32 bytes each: a multiple of 16)
    hipError_t e = tables.acquire(bytes);
    if (e != hipSuccess)
        return fail(kDevice, "batch any-normalizable table staging", e);
    std::memcpy(tables.host(), plan.entries.data(), bytes);
    e = tables.upload(user);
    if (e == hipSuccess)
        e = dxtlt::launch_batch_any_normalizable(reinterpret_cast<const dxtlt::BatchAnyEntry*>(tables.dev()), (uint32_t)plan.entries.size(), plan.wgs,
                                                 d_flags, user);
    return tables.finish(e, user, "batch any-normalizable table copy / launch", "batch any-normalizable event");
}

// Test hook (no device needed, nothing is dereferenced): the transform call's own planner and table writer, one record per launch
// in the order in which the call enqueues them.  The number of launches (records beyond `cap` are counted, not written); 0 for
// count == 0; for a batch the call refuses, minus the status the call returns (dxtlt_last_error() has the text).
extern "C" int32_t dxtlt_debug_plan_batch_normalize_call(const DxtltBatchNormalizeItem* items, size_t count, DxtltDebugBatchLaunch* out,
                                                         size_t cap, uint64_t* table_bytes_out)
{
    if (table_bytes_out)
        *table_bytes_out = 0;
    NormalizePlan plan;
    if (int32_t rc = plan_batch_normalize(items, count, plan); rc != kOk)
        return -rc;
    std::vector<uint8_t> tables(plan.table_bytes);
    fill_tile_tables(plan.tiles, tables.data());
    if (table_bytes_out)
        *table_bytes_out = plan.table_bytes;
    size_t n = 0;
    auto put = [&](const DxtltDebugBatchLaunch& r) {
        if (out != nullptr && n < cap)
            out[n] = r;
        ++n;
    };
    for (const TileLaunch& l : plan.tiles) {
        DxtltDebugBatchLaunch r = tile_launch_record(l);
        if (l.norm != 0) {
            r.kind = 4;
            r.strided = 0;   // (the normalising kernel always reads its table)
            if (l.norm != kNormPerEntry)
                r.settings_code |= l.norm << 8;
        }
        put(r);
    }
    for (size_t i : plan.singles) {
        DxtltDebugBatchLaunch r{};
        r.kind = 2, r.format = items[i].format;
        r.settings_code = settings_code(item_settings(items[i]));
        r.items = r.entries = 1, r.first_item = i;
        put(r);
    }
    return (int32_t)n;
}
