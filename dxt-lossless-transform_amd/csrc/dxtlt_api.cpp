// dxtlt_api.cpp -- C ABI of libdxtlt_gfx950.so (include/dxtlt_gfx950.h) for formats 1-5: argument validation, the
// launch and stream layout these formats hand to the host-pointer and sharded paths (host_staging.cpp,
// host_sharded.cpp), the device-pointer entry points, and tuning / version / release.
// All arithmetic lives in bcn_kernels.hip; nothing here touches block bytes on the CPU.
#include "../../include/dxtlt_gfx950.h"
#include "../../include/dxtlt_bc45.h"

#include <hip/hip_runtime_api.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "bcn_launch.h"
#include "host_common.h"

namespace {

using dxtlt::Format;
using dxtlt::Range;
using dxtlt::Settings;

thread_local std::string g_last_error;
thread_local std::vector<DxtltShardStat> g_shard_stats;   // of this thread's last dxtlt_transform_sharded call
std::atomic<int> g_tile_threads{0};
std::atomic<int> g_force_generic{0};

}  // namespace

int32_t dxtlt_host::fail(int32_t code, const char* what, hipError_t e)
{
    char buf[256];
    if (e != hipSuccess)
        std::snprintf(buf, sizeof buf, "dxtlt: %s: %s (%d)", what, hipGetErrorString(e), (int)e);
    else
        std::snprintf(buf, sizeof buf, "dxtlt: %s", what);
    g_last_error = buf;
    return code;
}

int32_t dxtlt_host::fail_verbatim(int32_t code, const char* text)
{
    g_last_error = text;
    return code;
}

namespace {
using dxtlt_host::fail;

dxtlt::LaunchTuning current_tuning()
{
    dxtlt::LaunchTuning t;
    t.tile_threads = g_tile_threads.load(std::memory_order_relaxed);
    t.force_generic = g_force_generic.load(std::memory_order_relaxed);
    return t;
}

// BC4 / BC5 (formats 4, 5; include/dxtlt_bc45.h) have no colour endpoints: their decorrelation mode and colour split are ignored
inline bool ignores_colour_settings(int32_t format) { return !dxtlt::format_has_colour(format); }

int32_t check_common(int32_t format, size_t len, int mode, const void* a, const void* b)
{
    if (format < 1 || format > 5)
        return fail(DXTLT_E_INVALID_ARGUMENT, "format must be 1 (BC1), 2 (BC2), 3 (BC3), 4 (BC4) or 5 (BC5)");
    if (len % (size_t)dxtlt::block_bytes((Format)format) != 0)
        return fail(DXTLT_E_INVALID_LENGTH, "len is not a multiple of the block size");
    if (mode > 3 && !ignores_colour_settings(format))
        return fail(DXTLT_E_INVALID_ARGUMENT, "decorrelation_mode must be 0..3");
    if (len > 0 && (a == nullptr || b == nullptr))
        return fail(DXTLT_E_INVALID_ARGUMENT, "NULL buffer with len > 0");
    return DXTLT_OK;
}

// Block normalisation fused into a transform: BC1 / BC2 / BC3 forward only, in the modes of dxtlt::norm_limits (bcn_launch.h).
// BC1's colour mode 3 = transparent blocks only is internal, used by the auto transform (bc1_normalize.h): the public entry points
// (normalize_api.cpp) check color_mode <= 2 before they get here.
int32_t check_normalization(int32_t format, bool inverse, int normalize, int normalize_alpha)
{
    const dxtlt::NormLimits limits = dxtlt::norm_limits(format);
    if ((normalize != 0 || normalize_alpha != 0) &&
        (inverse || normalize > limits.colour_internal || normalize_alpha > limits.alpha))
        return fail(DXTLT_E_INVALID_ARGUMENT,
                    "block normalisation: BC1 / BC2 / BC3 forward only, color_mode 0..2, alpha_mode 0..3 for BC3 and 0 otherwise");
    return DXTLT_OK;
}

int32_t device_range(int32_t format, bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                     uint64_t num, Settings s, hipStream_t stream)
{
    if (format < 1 || format > 5)
        return fail(DXTLT_E_INVALID_ARGUMENT, "format must be 1 (BC1), 2 (BC2), 3 (BC3), 4 (BC4) or 5 (BC5)");
    if (ignores_colour_settings(format))
        s.variant = 0, s.split_colour = false;
    if (s.variant > 3)
        return fail(DXTLT_E_INVALID_ARGUMENT, "decorrelation_mode must be 0..3");
    if (first > total || num > total - first)
        return fail(DXTLT_E_INVALID_ARGUMENT, "block range exceeds total_blocks");
    if (num == 0)
        return DXTLT_OK;
    if (d_src == nullptr || d_dst == nullptr)
        return fail(DXTLT_E_INVALID_ARGUMENT, "NULL device buffer with a non-empty range");
    if (int32_t rc = check_normalization(format, inverse, s.normalize, s.normalize_alpha); rc != DXTLT_OK)
        return rc;
    Range r{total, first, num};
    dxtlt::LaunchTuning t = current_tuning();
    HIP_TRY(dxtlt::launch_transform((Format)format, inverse, s, d_src, d_dst, r, stream, &t), "kernel launch");
    return DXTLT_OK;
}

dxtlt_host::Launch launch_of(int32_t format, const Settings& s)
{
    return [=](bool inverse, const void* src, void* dst, uint64_t total, uint64_t first, uint64_t count, hipStream_t stream) {
        return device_range(format, inverse, src, dst, total, first, count, s, stream);
    };
}

}  // namespace

// Formats 1-5: the stream table of bcn_launch.h under the settings that apply to the format; shards and chunks on 2048
// blocks (one BC1 tile = two BC2 / BC3 tiles; also a multiple of 16, so all slices stay 16-byte aligned); a shard per block
// at most
dxtlt_host::StreamLayout dxtlt_host::block_layout(int32_t format, bool sa, bool sc)
{
    const dxtlt::Streams bs = dxtlt::make_streams(format, dxtlt::format_has_alpha_split(format) && sa, dxtlt::format_has_colour(format) && sc);
    StreamLayout S{format, bs.n, {}, {}, (uint64_t)dxtlt::block_bytes((Format)format), 2048, 1};
    for (int s = 0; s < bs.n; ++s) {
        S.off[s] = (uint64_t)bs.off[s];
        S.width[s] = (uint64_t)bs.width[s];
    }
    return S;
}

int32_t dxtlt_host::enqueue(int32_t format, bool inverse, const void* d_src, void* d_dst, uint64_t blocks, const Settings& s,
                            hipStream_t stream)
{
    return device_range(format, inverse, d_src, d_dst, blocks, 0, blocks, s, stream);
}

int32_t dxtlt_host::transform(int32_t format, bool inverse, const uint8_t* in, uint8_t* out, size_t len, const Settings& s)
{
    int32_t rc = check_common(format, len, s.variant, in, out);
    if (rc != DXTLT_OK)
        return rc;
    if (len == 0)
        return DXTLT_OK;  // zero blocks: nothing to do, no device needed
    const StreamLayout S = block_layout(format, s.split_alpha, s.split_colour);
    return host_round_trip(S, launch_of(format, s), inverse, in, out, len / S.block_bytes);
}

extern "C" {

// ---- host pointers ------------------------------------------------------------------------------
static int32_t host_call(int32_t format, bool inverse, const uint8_t* in, uint8_t* out, size_t len, uint8_t mode, bool sa, bool sc)
{
    return dxtlt_host::transform(format, inverse, in, out, len, Settings{mode, sa, sc});
}

int32_t dxtlt_transform_bc1_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sc)
{
    return host_call(1, false, i, o, len, mode, false, sc);
}
int32_t dxtlt_untransform_bc1_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sc)
{
    return host_call(1, true, i, o, len, mode, false, sc);
}
int32_t dxtlt_transform_bc2_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sc)
{
    return host_call(2, false, i, o, len, mode, false, sc);
}
int32_t dxtlt_untransform_bc2_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sc)
{
    return host_call(2, true, i, o, len, mode, false, sc);
}
int32_t dxtlt_transform_bc3_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sa, bool sc)
{
    return host_call(3, false, i, o, len, mode, sa, sc);
}
int32_t dxtlt_untransform_bc3_with_settings(const uint8_t* i, uint8_t* o, size_t len, uint8_t mode, bool sa, bool sc)
{
    return host_call(3, true, i, o, len, mode, sa, sc);
}

// ---- device pointers, whole buffer -------------------------------------------------------------------
static int32_t device_whole(int32_t format, bool inverse, const void* d_in, void* d_out, size_t len, uint8_t mode,
                            bool sa, bool sc, void* stream)
{
    int32_t rc = check_common(format, len, mode, d_in, d_out);
    if (rc != DXTLT_OK)
        return rc;
    const uint64_t blocks = len / (size_t)dxtlt::block_bytes((Format)format);
    return device_range(format, inverse, d_in, d_out, blocks, 0, blocks, Settings{mode, sa, sc}, (hipStream_t)stream);
}

int32_t dxtlt_transform_bc1_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sc, void* st)
{
    return device_whole(1, false, i, o, len, mode, false, sc, st);
}
int32_t dxtlt_untransform_bc1_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sc, void* st)
{
    return device_whole(1, true, i, o, len, mode, false, sc, st);
}
int32_t dxtlt_transform_bc2_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sc, void* st)
{
    return device_whole(2, false, i, o, len, mode, false, sc, st);
}
int32_t dxtlt_untransform_bc2_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sc, void* st)
{
    return device_whole(2, true, i, o, len, mode, false, sc, st);
}
int32_t dxtlt_transform_bc3_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sa, bool sc,
                                                 void* st)
{
    return device_whole(3, false, i, o, len, mode, sa, sc, st);
}
int32_t dxtlt_untransform_bc3_with_settings_device(const void* i, void* o, size_t len, uint8_t mode, bool sa, bool sc,
                                                   void* st)
{
    return device_whole(3, true, i, o, len, mode, sa, sc, st);
}

int32_t dxtlt_transform_range_device(int32_t format, bool inverse, const void* d_src, void* d_dst,
                                     uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks, uint8_t mode,
                                     bool sa, bool sc, void* stream)
{
    return device_range(format, inverse, d_src, d_dst, total_blocks, first_block, num_blocks, Settings{mode, sa, sc},
                        (hipStream_t)stream);
}

// ---- BC4 / BC5 (include/dxtlt_bc45.h): formats 4 and 5 of the same paths, split_endpoints in the alpha split ----------
int32_t dxtlt_transform_bc4_with_settings(const uint8_t* i, uint8_t* o, size_t len, bool split_endpoints)
{
    return host_call(4, false, i, o, len, 0, split_endpoints, false);
}
int32_t dxtlt_untransform_bc4_with_settings(const uint8_t* i, uint8_t* o, size_t len, bool split_endpoints)
{
    return host_call(4, true, i, o, len, 0, split_endpoints, false);
}
int32_t dxtlt_transform_bc5_with_settings(const uint8_t* i, uint8_t* o, size_t len, bool split_endpoints)
{
    return host_call(5, false, i, o, len, 0, split_endpoints, false);
}
int32_t dxtlt_untransform_bc5_with_settings(const uint8_t* i, uint8_t* o, size_t len, bool split_endpoints)
{
    return host_call(5, true, i, o, len, 0, split_endpoints, false);
}
int32_t dxtlt_transform_bc4_with_settings_device(const void* i, void* o, size_t len, bool split_endpoints, void* st)
{
    return device_whole(4, false, i, o, len, 0, split_endpoints, false, st);
}
int32_t dxtlt_untransform_bc4_with_settings_device(const void* i, void* o, size_t len, bool split_endpoints, void* st)
{
    return device_whole(4, true, i, o, len, 0, split_endpoints, false, st);
}
int32_t dxtlt_transform_bc5_with_settings_device(const void* i, void* o, size_t len, bool split_endpoints, void* st)
{
    return device_whole(5, false, i, o, len, 0, split_endpoints, false, st);
}
int32_t dxtlt_untransform_bc5_with_settings_device(const void* i, void* o, size_t len, bool split_endpoints, void* st)
{
    return device_whole(5, true, i, o, len, 0, split_endpoints, false, st);
}

// ---- single-process multi-GPU ---------------------------------------------------------------------------
int32_t dxtlt_transform_sharded(int32_t format, bool inverse, const uint8_t* in, uint8_t* out, size_t len,
                                uint8_t mode, bool sa, bool sc, int32_t num_devices)
{
    // 8 / 9: uncompressed pixels of 4 / 3 bytes (include/dxtlt_pixels.h), the settings triple read as pixel settings
    if (dxtlt_host::is_pixel_format(format))
        return dxtlt_host::pixel_sharded(dxtlt_host::pixel_bytes_of(format), inverse, in, out, len, dxtlt_host::pixel_decorrelate_of(mode),
                                         dxtlt_host::pixel_layout_of(sa, sc), num_devices, &g_shard_stats);
    int32_t rc = check_common(format, len, mode, in, out);
    if (rc != DXTLT_OK)
        return rc;
    if (len == 0)
        return DXTLT_OK;
    const dxtlt_host::StreamLayout S = dxtlt_host::block_layout(format, sa, sc);
    return dxtlt_host::run_sharded(S, launch_of(format, Settings{mode, sa, sc}), inverse, in, out, len / S.block_bytes, 0, num_devices,
                                   &g_shard_stats);
}

int32_t dxtlt_sharded_last_stats(DxtltShardStat* out, int32_t cap)
{
    const int32_t n = (int32_t)g_shard_stats.size();
    for (int32_t i = 0; out != nullptr && i < n && i < cap; ++i)
        out[i] = g_shard_stats[(size_t)i];
    return n;
}

// ---- plumbing -------------------------------------------------------------------------------------------
int32_t dxtlt_fill_splitmix64_device(void* d_dst, size_t len_bytes, uint64_t seed, uint64_t first_qword, void* stream)
{
    if (len_bytes > 0 && d_dst == nullptr)
        return fail(DXTLT_E_INVALID_ARGUMENT, "NULL device buffer");
    HIP_TRY(dxtlt::launch_fill_splitmix64(d_dst, len_bytes, seed, first_qword, (hipStream_t)stream), "fill launch");
    return DXTLT_OK;
}

const char* dxtlt_last_error(void) { return g_last_error.c_str(); }

int32_t dxtlt_device_count(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess)
        return 0;
    return count;
}

// The host-pointer crossover a size-routing caller should use (include/dxtlt_gfx950.h).  32 MiB: the size at which the
// chunked host pipeline (upload | kernel | download) overtakes one core of the reference's SIMD path on this class of host
// (profiles/r01_w_host_path_latency_vs_cpu.json, r01_j_host_pointer_pipeline_threshold.txt).
static std::atomic<size_t> g_host_route_threshold{size_t(32) << 20};

size_t dxtlt_host_route_threshold_bytes(void)
{
    if (const char* v = std::getenv("DXTLT_HOST_ROUTE_THRESHOLD_BYTES")) {
        char* end = nullptr;
        const unsigned long long x = std::strtoull(v, &end, 10);
        if (end != v)
            return (size_t)x;
    }
    return g_host_route_threshold.load();
}

void dxtlt_set_host_route_threshold_bytes(size_t bytes) { g_host_route_threshold.store(bytes); }

int32_t dxtlt_tuning_mask(void) { return dxtlt::launch_force_mask(); }

int32_t dxtlt_debug_check_normalization(int32_t format, int32_t inverse, uint8_t color_mode, uint8_t alpha_mode)
{
    return check_normalization(format, inverse != 0, color_mode, alpha_mode);
}

int32_t dxtlt_debug_plan_transform(int32_t format, int32_t inverse, int32_t variant, int32_t split_alpha, int32_t split_colour,
                                   uint64_t src_address, uint64_t dst_address, uint64_t total_blocks, uint64_t first_block,
                                   uint64_t num_blocks, DxtltDebugPlannedLaunch* out, int32_t cap)
{
    if (format < 1 || format > 5 || cap < 0 || (cap > 0 && out == nullptr) || first_block > total_blocks || num_blocks > total_blocks - first_block)
        return -1;
    std::vector<dxtlt::DebugPlannedLaunch> tmp((size_t)cap);
    const Settings s{variant, split_alpha != 0, split_colour != 0, 0};
    const dxtlt::LaunchTuning t = current_tuning();
    const int n = dxtlt::debug_plan_transform((Format)format, inverse != 0, s, src_address, dst_address, Range{total_blocks, first_block, num_blocks},
                                              &t, tmp.data(), cap);
    for (int i = 0; i < n && i < cap; ++i) {
        const dxtlt::DebugPlannedLaunch& l = tmp[(size_t)i];
        DxtltDebugPlannedLaunch& o = out[i];
        o.kind = l.kind;
        o.threads = l.threads;
        o.workgroups = l.workgroups;
        o.full_tiles = l.full_tiles;
        o.range_blocks = l.range_blocks;
        o.aos_offset = l.aos_offset;
        std::memcpy(o.shift, l.shift, sizeof o.shift);
        o.halo_vecs = l.halo_vecs;
        o.natural = l.natural;
        std::memcpy(o.gbase, l.gbase, sizeof o.gbase);
    }
    return n;
}

void dxtlt_set_tuning(int32_t tile_threads, int32_t force_path)
{
    g_tile_threads.store(tile_threads);
    // Only the bits the kernels know (bcn_kernels.hip, kForceMask): 2 and 0x20 -- test levers that select paths some address
    // pattern selects by itself, results exact -- and nothing else; in particular the library contains no switch that changes
    // results.
    g_force_generic.store(force_path & dxtlt::launch_force_mask());
}

const char* dxtlt_version(void) { return "dxtlt-gfx950 0.2.0"; }

void dxtlt_release_thread_resources(void)
{
    dxtlt_host::release_thread_staging();
    dxtlt_host::release_idle_shard_contexts();   // process-wide: the idle per-device contexts of the sharded calls
    dxtlt_host::release_normalize_thread_flag();
    dxtlt_host::release_batch_thread_tables();
    dxtlt_host::release_batch_host_thread_arenas();
    dxtlt_host::release_auto_thread_arena();
}

}  // extern "C"
