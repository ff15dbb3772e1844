// host_common.h -- internal interface between the host translation units: the C ABI files (dxtlt_api.cpp, bc7_api.cpp,
// bc6h_api.cpp, c_api_*.cpp, ...), the host-pointer staging paths (host_staging.cpp) and the sharded path
// (host_sharded.cpp).  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/dlt_size_estimator.h"
#include "../../include/dxtlt_gfx950.h"
#include "bcn_launch.h"
#include "estimate_launch.h"

namespace dxtlt_host {

// status codes == DXTLT_* in include/dxtlt_gfx950.h
enum : int32_t {
    kOk = 0,
    kInvalidLength = 1,
    kInvalidArgument = 2,
    kNoDevice = 3,
    kDevice = 4,
    kEstimator = 5,
    kAllocation = 6,
};

// Records the failure text for dxtlt_last_error() on this thread and returns `code`.
int32_t fail(int32_t code, const char* what, hipError_t e = hipSuccess);
// The same with a complete text, recorded as it is: a worker thread's dxtlt_last_error() carried to the caller's thread.
int32_t fail_verbatim(int32_t code, const char* text);

// A failed HIP call leaves the calling function with DXTLT_E_DEVICE and the call's name in the error text.
#define HIP_TRY(expr, what)                                             \
    do {                                                                \
        hipError_t e_ = (expr);                                         \
        if (e_ != hipSuccess)                                           \
            return dxtlt_host::fail(dxtlt_host::kDevice, what, e_);     \
    } while (0)

// ---------------------------------------------------------------------------------------------------
// What the host-pointer paths know about a format family: where a block range's bytes live on the transformed side,
// and how to launch its kernels.
// ---------------------------------------------------------------------------------------------------
// Stream s of a transformed array of N blocks starts at byte off[s] * N and holds width[s] bytes per block, so blocks
// [first, first + count) own bytes [off[s] * N + width[s] * first, ... + width[s] * count) of it.  Formats 1-5 fill this in
// from dxtlt::make_streams and their settings (block_layout, dxtlt_api.cpp), formats 6-7 from the granule formats' one
// table (granule_layout, granule_host.cpp), where N is the array's main part (whole granules): the tail part behind the
// streams is a buffer of its own and never passes through a layout.
struct StreamLayout {
    int format;              // 1..9: picks the pipeline's chunk-size rule
    int n;                   // streams
    uint64_t off[8], width[8];
    uint64_t block_bytes;
    uint64_t align_blocks;   // a shard and a pipeline chunk start on a multiple of this (2048 / the sort granule)
    uint64_t shard_unit;     // a call has at most one shard per `shard_unit` blocks (1 / the sort granule)
};
StreamLayout block_layout(int32_t format, bool split_alpha, bool split_colour);
StreamLayout granule_layout(int format);

// Enqueues the transform of blocks [first, first + count) of an array of `total` blocks (dxtlt_transform_range_device
// semantics: the AoS-side pointer is the range's first block, the SoA-side pointer the whole transformed array) and
// returns a status, the error text recorded.  The format and its settings are bound in.
using Launch = std::function<int32_t(bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                                     uint64_t count, hipStream_t stream)>;

// Host pointers in/out, whole buffer, synchronous (H2D + kernel + D2H on the current device).  `s` as the caller's arguments
// gave it (bcn_launch.h): its decorrelation mode and fused normalisation modes are checked here.
int32_t transform(int32_t format, bool inverse, const uint8_t* in, uint8_t* out, size_t len, const dxtlt::Settings& s);

// ---- host_staging.cpp -------------------------------------------------------------------------------
// This thread's staging context on the current device: two device buffers of at least `bytes` and a stream.
int32_t acquire_staging(size_t bytes, void** d_in, void** d_out, hipStream_t* stream);

// Small host buffers (up to 1 MiB, DXTLT_MAPPED_MAX_BYTES): the calling thread's pair of MAPPED pinned staging buffers
// (h_*: host addresses, d_*: the same memory as the device sees it) and its stream; usable == false above the limit.
// The caller copies its input to h_in, launches on d_in -> d_out, waits for the stream and copies h_out out.
struct MappedStaging {
    bool usable;
    void* h_in;
    void* h_out;
    void* d_in;
    void* d_out;
    hipStream_t stream;
};
int32_t acquire_mapped_staging(size_t bytes, MappedStaging* out);

// One whole array of `blocks` blocks from host memory to host memory on the current device: through the mapped pair,
// the chunked pipeline or one H2D + launch + D2H, by size.  The stream is drained on every exit.
int32_t host_round_trip(const StreamLayout& L, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out,
                        uint64_t blocks);
// Whether a transfer of `bytes` is large enough for the chunked pipeline (DXTLT_PIPELINE_MIN_BYTES).
bool pipeline_pays(uint64_t bytes);
// Blocks [first, first + count) of a host-resident array of `total` blocks through the chunked upload | kernel | download
// pipeline, on device `dev` with its stream `up` and two device buffers of count * block_bytes.
struct DeviceStaging {
    int dev;
    hipStream_t up;
    void* d_in;
    void* d_out;
};
int32_t pipelined_range(const StreamLayout& L, const Launch& launch, const DeviceStaging& d, bool inverse, const uint8_t* in,
                        uint8_t* out, uint64_t total, uint64_t first, uint64_t count);
void release_thread_staging();   // of dxtlt_release_thread_resources()

// The routes dxtlt_debug_host_route_counts reports, in its order: process-wide cumulative counters, bumped with relaxed
// atomic adds (shard workers and the pipeline's downloader run on threads of their own).  Counting changes no route.
enum HostRoute : int {
    kRouteMapped = 0,          // host_round_trip through the mapped pinned pair
    kRouteOneShot = 1,         // host_round_trip as one upload + launch + download
    kRoutePipelinedRange = 2,  // calls of pipelined_range (whole buffers and shards)
    kRoutePipelineChunk = 3,   // chunks pipelined_range has enqueued
    kRouteShardOneShot = 4,    // one_shot transfers of host_sharded.cpp
    kRouteCount = 5,
};
void count_route(HostRoute route);

// ---- host_sharded.cpp -------------------------------------------------------------------------------
// A host array of `total` blocks -- the last `tail` of them a part of its own behind the streams (granule formats; 0
// otherwise) -- in contiguous shards over the node's devices, one bound worker thread per shard.  The arguments are
// valid and the array is not empty.  `stats` (optional) receives one record per shard once the workers have joined.
int32_t run_sharded(const StreamLayout& L, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out, uint64_t total,
                    uint64_t tail, int32_t num_shards, std::vector<DxtltShardStat>* stats);
// Where a shard's transformed bytes live: slice s < L.n is its `in_main` blocks' share of stream s of an array whose
// streams hold `main_total` blocks, slice L.n its `tail` blocks of the part behind the streams.  host_off: in the whole
// transformed array; dev_off: in the shard transformed as a stand-alone buffer.
struct Slice {
    uint64_t host_off, dev_off, bytes;
};
void shard_slices(const StreamLayout& L, uint64_t main_total, uint64_t first, uint64_t in_main, uint64_t tail, Slice* out);
void release_idle_shard_contexts();   // process-wide; of dxtlt_release_thread_resources()

// ---- granule_host.cpp: the host, device and sharded calls of the granule formats, 7 = BC7, 6 = BC6H ----
int32_t granule_host_call(int format, bool inverse, const uint8_t* in, uint8_t* out, size_t len);
int32_t granule_device_call(int format, bool inverse, const void* d_in, void* d_out, size_t len, void* stream);
int32_t granule_device_range(int format, bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                             uint64_t num, void* stream);
int32_t granule_sharded(int format, bool inverse, const uint8_t* in, uint8_t* out, size_t len, int32_t num_shards);
int32_t granule_shard_pieces(int format, uint64_t total_blocks, uint64_t first_block, uint64_t num_blocks, uint64_t* global_off,
                             uint64_t* local_off, uint64_t* bytes);

// ---- pixels_api.cpp: uncompressed pixels (include/dxtlt_pixels.h); generic format codes 8 = 4-byte, 9 = 3-byte pixels ----
inline bool is_pixel_format(int format) { return format == 8 || format == 9; }
inline int pixel_bytes_of(int format) { return format == 8 ? 4 : 3; }
// the generic entry points' settings triple as pixel settings: any decorrelation mode = decorrelate; no colour split =
// INTERLEAVED, colour split = PLANAR, colour and alpha split = PLANAR_DELTA
inline bool pixel_decorrelate_of(uint8_t mode) { return mode != 0; }
inline uint8_t pixel_layout_of(bool split_alpha, bool split_colour) { return !split_colour ? 0 : split_alpha ? 2 : 1; }
StreamLayout pixel_layout(int pixel_bytes, uint8_t layout);
int32_t pixel_host_call(int pixel_bytes, bool inverse, const uint8_t* in, uint8_t* out, size_t len, bool decorrelate, uint8_t layout);
int32_t pixel_device_range(int pixel_bytes, bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                           uint64_t num, bool decorrelate, uint8_t layout, void* stream);
int32_t pixel_sharded(int pixel_bytes, bool inverse, const uint8_t* in, uint8_t* out, size_t len, bool decorrelate, uint8_t layout,
                      int32_t num_shards, std::vector<DxtltShardStat>* stats);

// ---- batch_api.cpp, for the host batch (batch_host_api.cpp) ----
// bytes per block (8, 9: per pixel) of a batch item's format (1..9)
inline uint32_t item_block_bytes(uint8_t format)
{
    return is_pixel_format(format) ? (uint32_t)pixel_bytes_of(format) : format == 1 || format == 4 ? 8u : 16u;
}
// The per-item checks of both batch calls, in the order in which defects are reported; `host_call`: the host batch's texts and its
// 4 GiB limit.  kOk, or the failure as fail() recorded it.
int32_t batch_item_defect(const DxtltBatchItem& it, int max_format, bool host_call);
// The device batch on `stream`; `pixels_allowed`: items of formats 8 and 9 are taken too (the host batch's chunks).
int32_t batch_device(const DxtltBatchItem* items, size_t count, void* stream, bool pixels_allowed);

// Binds the calling thread -- one this library created for `device` -- to the CPUs local to the device (numa_affinity.cpp).
// Returns the number of CPUs bound to, 0 when nothing was changed.
int bind_this_thread_near_device(int device);

// Enqueue one whole-buffer transform on device pointers.
int32_t enqueue(int32_t format, bool inverse, const void* d_src, void* d_dst, uint64_t blocks, const dxtlt::Settings& s,
                hipStream_t stream);

// Per-thread device resources of the other translation units, freed by dxtlt_release_thread_resources().
void release_normalize_thread_flag();   // normalize_api.cpp
void release_batch_thread_tables();     // batch_api.cpp
void release_batch_host_thread_arenas();   // batch_host_api.cpp
void release_auto_thread_arena();       // auto_transform.cpp

struct AutoChoice {
    uint8_t mode;  // core numbering
    bool split_alpha;
    bool split_colour;
    uint32_t estimator_error;  // the callback's non-zero return when the status is kEstimator
};

// transform_bcN_auto on host pointers, format 1..5 (see auto_transform.cpp).  BC4 / BC5: use_all_decorrelation_modes is ignored and
// choice->split_alpha = split_endpoints.
int32_t transform_auto(int32_t format, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* estimator,
                       bool use_all_decorrelation_modes, AutoChoice* choice);

// dxtlt_transform_bcN_auto_device (include/dxtlt_estimator.h), format 1..5: device pointers, the built-in estimator, one small
// readback; the winning transform is left enqueued on `stream`.
int32_t transform_auto_device(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all_decorrelation_modes,
                              hipStream_t stream, AutoChoice* choice);

// ---- auto_transform.cpp, shared with the batched call (batch_auto_api.cpp) ----
// The candidates of `format` (1..5) in the order they are compared, into out[0 .. 16); returns how many (candidates_of).
int auto_candidate_order(int32_t format, bool use_all_decorrelation_modes, AutoChoice* out);
// What every device route does with its counters after the readback: the candidates' totals in candidate order into total[0 .. 16)
// and the pick, the first minimum of the order (strict `<`).  sizes: the distinct sections in dxtlt::auto_sections' order (auto_launch.h)
// or, per_candidate, two slots per candidate (BC4 / BC5 on the single-buffer route, every format without the arena).
int auto_pick(int32_t format, bool use_all_decorrelation_modes, bool per_candidate, const uint64_t* sizes, uint64_t* total);
void release_batch_auto_thread_buffers();   // batch_auto_api.cpp; through release_auto_thread_arena()
// (the frame of the single-buffer auto calls and this thread's auto state: auto_call.h)

// ---- normalize_api.cpp, auto_normalize_api.cpp: block normalisation, alone, fused and in the auto transform ----
// What the calls need to know about a format; its legal modes are dxtlt::norm_limits (bcn_launch.h)
struct NormFormat {
    int fmt;
    size_t block_bytes;
    int all_modes_outputs;   // one per (alpha mode, colour mode), [alpha_mode * 3 + colour_mode]
    const char* bad_len;
};
inline constexpr NormFormat kNormBc1{1, 8, 3, "len is not a multiple of 8"}, kNormBc2{2, 16, 3, "len is not a multiple of 16"},
    kNormBc3{3, 16, 12, "len is not a multiple of 16"};
// normalize_api.cpp: this thread's flag word ("any block normalised") on the current device, zeroed on `stream`
int32_t normalize_thread_flag(uint32_t** d_flag, hipStream_t stream);

// ---- estimate_api.cpp: the built-in estimator (include/dxtlt_estimator.h) -----------------------------------------
bool is_builtin_estimator(const DltSizeEstimator* estimator);   // by the identity of its two function pointers
// This thread's counter block on the current device: kMaxCounters estimates (BC3 with every mode, one full transform per
// candidate: 16 x 2).  estimate_enqueue puts the estimates of `count` sections into counters [first_counter, + count) on
// `stream`; estimate_read_back copies counters [0, count) to `out` and waits for the stream.
constexpr size_t kMaxCounters = 32;   // also the sections of BC3's auto transform with normalisation (8 alpha + 24 colour)
int32_t estimate_enqueue(const dxtlt::EstimateSection* sections, size_t count, hipStream_t stream, size_t first_counter);
int32_t estimate_read_back(size_t count, hipStream_t stream, uint64_t* out);
// The entropy estimator (include/dxtlt_entropy_estimator.h) into the same counters; recognised by the identity of its pointer.
int32_t entropy_enqueue(const dxtlt::EstimateSection* sections, size_t count, hipStream_t stream, size_t first_counter);
bool is_builtin_entropy_estimator(const DltSizeEstimator* estimator);
bool stream_is_capturing(hipStream_t stream);
void release_estimate_thread_counters();   // of dxtlt_release_thread_resources(), through release_auto_thread_arena()

}  // namespace dxtlt_host
