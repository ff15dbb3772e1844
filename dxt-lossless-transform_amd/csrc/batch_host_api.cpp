// batch_host_api.cpp -- dxtlt_transform_batch_host: many HOST buffers in one call -- the reference's actual call pattern: one call
// per file, host pointers, textures of 0.1-20 MiB (tools/dxt-lossless-transform-cli/src/commands/transform/mod.rs:154-199).
// Through the single-buffer entry points every texture pays a PCIe round trip of its own (1 MiB: 149 us = 6.6 GiB/s,
// DESIGN.md section 5).  Here the batch is cut into chunks of about 64 MiB (batch_host_plan.h: pure arithmetic, checked without a
// device) and every chunk takes five steps:
//     pack      a few host threads copy the chunk's buffers side by side into a PINNED arena
//     upload    one asynchronous copy of the whole chunk
//     kernels   the device batch call on the chunk (batch_api.cpp: one launch per format, direction and settings present in it)
//     download  one asynchronous copy into a second pinned arena
//     unpack    host threads copy every result to its caller's buffer
// with two arenas per direction, so that packing chunk k + 1, moving chunk k and unpacking chunk k - 1 overlap and PCIe
// runs in both directions at once.  (A first version let several threads issue one small pageable copy per buffer
// straight from / to the callers' memory: 21 GiB/s at 1 MiB per buffer, 16 at 4 MiB -- the runtime pins pageable memory
// on the fly above 1 MiB; profiles/r02_d_batch_host.txt.)  Synchronous; every exit joins the threads and drains the streams
// before the arenas are released for reuse.  The stream, the events, the stage gate and the thread set are host_pipeline.h's.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/dxtlt_gfx950.h"
#include "batch_host_plan.h"
#include "bcn_launch.h"
#include "granule_launch.h"
#include "host_common.h"
#include "host_pipeline.h"

namespace {

using namespace dxtlt_host;

// chunk size and copy threads per direction; DXTLT_BATCH_CHUNK_MIB / DXTLT_BATCH_THREADS override them (experiments)
size_t env_number(const char* name, size_t fallback)
{
    const char* v = std::getenv(name);
    const unsigned long long x = v ? std::strtoull(v, nullptr, 10) : 0;
    return x ? (size_t)x : fallback;
}
const size_t kHostBatchChunkBytes = env_number("DXTLT_BATCH_CHUNK_MIB", 64) << 20;
const int kCopyThreads = (int)std::min<size_t>(64, env_number("DXTLT_BATCH_THREADS", 6));

// pinned arenas of the calling thread: two per direction, grow-only
struct PinnedArenas {
    void* in[2] = {nullptr, nullptr};
    void* out[2] = {nullptr, nullptr};
    size_t cap = 0;
    ~PinnedArenas() { release(); }
    void release()
    {
        for (int i = 0; i < 2; ++i) {
            if (in[i]) (void)hipHostFree(in[i]);
            if (out[i]) (void)hipHostFree(out[i]);
            in[i] = out[i] = nullptr;
        }
        cap = 0;
    }
    hipError_t reserve(size_t bytes)
    {
        if (bytes <= cap)
            return hipSuccess;
        release();
        for (int i = 0; i < 2; ++i) {
            hipError_t e = hipHostMalloc(&in[i], bytes, hipHostMallocDefault);
            if (e == hipSuccess)
                e = hipHostMalloc(&out[i], bytes, hipHostMallocDefault);
            if (e != hipSuccess) {
                release();
                return e;
            }
        }
        cap = bytes;
        return hipSuccess;
    }
};
thread_local PinnedArenas g_pinned;

// What the stages of one call share.  Chunk c uses pinned arena c % 2 and device slot c % 2 of either direction, and owns three
// events: uploaded, kernels done, downloaded.  Item k of the plan's packed list belongs to copy thread (k - chunk.first) % kCopyThreads.
struct HostBatch {
    const DxtltBatchItem* items;
    const HostBatchPlan& plan;
    int nchunks;
    int dev = 0;
    uint8_t *d_in = nullptr, *d_out = nullptr;   // two chunk-sized slots each, inside this thread's staging buffers
    hipStream_t up = nullptr;                    // this thread's staging stream: uploads and kernels
    OwnedStream down;                            // downloads
    // worker threads do not see the calling thread's thread_local arenas: they are handed the pointers
    uint8_t *pinned_in[2] = {nullptr, nullptr}, *pinned_out[2] = {nullptr, nullptr};
    EventList ev;

    StageGate gate;
    std::vector<int> packed;     // per chunk: packer threads that have finished it
    std::vector<int> unpacked;   // per chunk: unpacker threads that have finished it
    int uploaded_recorded = 0;   // chunks whose upload event has been recorded
    int kernels_issued = 0;      // chunks whose upload and kernels have been enqueued (ev_kernels recorded)
    int enqueued = 0;            // chunks whose download has been enqueued too (ev_downloaded recorded)

    HostBatch(const DxtltBatchItem* items_, const HostBatchPlan& plan_)
        : items(items_), plan(plan_), nchunks((int)plan_.chunks.size()), packed(plan_.chunks.size(), 0), unpacked(plan_.chunks.size(), 0)
    {
    }
    const HostBatchChunk& chunk(int c) const { return plan.chunks[(size_t)c]; }
    const DxtltBatchItem& item(size_t k) const { return items[plan.packed[k]]; }
    uint64_t slot(size_t k) const { return plan.slot[plan.packed[k]]; }
    uint8_t* arena_in(int c) const { return pinned_in[c & 1]; }
    uint8_t* arena_out(int c) const { return pinned_out[c & 1]; }
    uint8_t* device_in(int c) const { return d_in + (size_t)(c & 1) * plan.arena_bytes; }
    uint8_t* device_out(int c) const { return d_out + (size_t)(c & 1) * plan.arena_bytes; }
    hipEvent_t ev_uploaded(int c) const { return ev[(size_t)c * 3]; }
    hipEvent_t ev_kernels(int c) const { return ev[(size_t)c * 3 + 1]; }
    hipEvent_t ev_downloaded(int c) const { return ev[(size_t)c * 3 + 2]; }
};

// An item that goes out alone (batch_host_plan.h): the single-buffer host entry point of its format
int32_t transform_alone(const DxtltBatchItem& it)
{
    const uint8_t* in = static_cast<const uint8_t*>(it.d_input);
    uint8_t* out = static_cast<uint8_t*>(it.d_output);
    if (is_pixel_format(it.format))
        return pixel_host_call(pixel_bytes_of(it.format), it.inverse != 0, in, out, it.len, pixel_decorrelate_of(it.decorrelation_mode),
                               pixel_layout_of(it.split_alpha_endpoints != 0, it.split_colour_endpoints != 0));
    if (dxtlt::granule::is_granule_format(it.format))
        return granule_host_call(it.format, it.inverse != 0, in, out, it.len);
    return transform(it.format, it.inverse != 0, in, out, it.len,
                     dxtlt::Settings{it.decorrelation_mode, dxtlt::format_has_alpha_split(it.format) && it.split_alpha_endpoints,
                                     it.split_colour_endpoints != 0});
}

// This thread's device slots, stream and pinned arenas, the download stream and the events of a call
int32_t acquire(HostBatch& b)
{
    void *d_in = nullptr, *d_out = nullptr;
    if (int32_t rc = acquire_staging((size_t)(2 * b.plan.arena_bytes), &d_in, &d_out, &b.up); rc != kOk)
        return rc;
    b.d_in = static_cast<uint8_t*>(d_in), b.d_out = static_cast<uint8_t*>(d_out);
    if (hipError_t e = g_pinned.reserve((size_t)b.plan.arena_bytes); e != hipSuccess)
        return fail(kDevice, "hipHostMalloc(batch arenas)", e);
    for (int i = 0; i < 2; ++i) {
        b.pinned_in[i] = static_cast<uint8_t*>(g_pinned.in[i]);
        b.pinned_out[i] = static_cast<uint8_t*>(g_pinned.out[i]);
    }
    (void)hipGetDevice(&b.dev);
    if (hipError_t e = b.down.create(); e != hipSuccess)
        return fail(kDevice, "hipStreamCreate(download)", e);
    if (hipError_t e = b.ev.create((size_t)b.nchunks * 3, hipEventDisableTiming); e != hipSuccess)
        return fail(kDevice, "hipEventCreate", e);
    return kOk;
}

void packer(HostBatch* batch, int tid)
{
    HostBatch& b = *batch;
    hipError_t e = hipSetDevice(b.dev);
    for (int c = 0; c < b.nchunks && e == hipSuccess; ++c) {
        // arena c % 2 is free once chunk c - 2 has left it (chunks 0 and 1 wait for nothing -- but not for a call that is already
        // being abandoned)
        if (!b.gate.wait([&] { return c < 2 || b.uploaded_recorded > c - 2; }))
            return;
        if (c >= 2) {
            e = hipEventSynchronize(b.ev_uploaded(c - 2));
            if (e != hipSuccess)
                break;
        }
        const HostBatchChunk& ch = b.chunk(c);
        for (size_t k = ch.first + (size_t)tid; k < ch.first + ch.count; k += kCopyThreads)
            if (b.item(k).len)
                std::memcpy(b.arena_in(c) + b.slot(k), b.item(k).d_input, b.item(k).len);
        b.gate.increment(b.packed[(size_t)c]);
    }
    if (e != hipSuccess)
        b.gate.fail(e);
}

void unpacker(HostBatch* batch, int tid)
{
    HostBatch& b = *batch;
    hipError_t e = hipSetDevice(b.dev);
    for (int c = 0; c < b.nchunks && e == hipSuccess; ++c) {
        // a download that was enqueued before the call was abandoned is still unpacked
        if (!b.gate.wait_reached([&] { return b.enqueued > c; }))
            return;
        e = hipEventSynchronize(b.ev_downloaded(c));
        if (e != hipSuccess)
            break;
        const HostBatchChunk& ch = b.chunk(c);
        for (size_t k = ch.first + (size_t)tid; k < ch.first + ch.count; k += kCopyThreads)
            if (b.item(k).len)
                std::memcpy(b.item(k).d_output, b.arena_out(c) + b.slot(k), b.item(k).len);
        b.gate.increment(b.unpacked[(size_t)c]);
    }
    if (e != hipSuccess)
        b.gate.fail(e);
}

// The downloads are issued by a thread of their own.  A chunk's download may only be enqueued once the unpackers have
// emptied its pinned output arena (chunk c - 2) -- a HOST-side condition -- and when the uploading thread waited for that before
// it issued the chunk's upload, only two chunks were ever between upload and unpack: the steady state was
// (upload + kernels + download + unpack) / 2 per chunk, 33 GiB/s, not the slowest stage.
void downloader(HostBatch* batch)
{
    HostBatch& b = *batch;
    hipError_t e = hipSetDevice(b.dev);
    for (int c = 0; c < b.nchunks && e == hipSuccess; ++c) {
        if (!b.gate.wait([&] { return b.kernels_issued > c && (c < 2 || b.unpacked[(size_t)c - 2] == kCopyThreads); }))
            return;
        e = hipStreamWaitEvent(b.down.stream, b.ev_kernels(c), 0);
        if (e == hipSuccess)
            e = hipMemcpyAsync(b.arena_out(c), b.device_out(c), (size_t)b.chunk(c).bytes, hipMemcpyDeviceToHost, b.down.stream);
        if (e == hipSuccess)
            e = hipEventRecord(b.ev_downloaded(c), b.down.stream);
        if (e != hipSuccess)
            break;
        b.gate.publish(b.enqueued, c + 1);
    }
    if (e != hipSuccess)
        b.gate.fail(e);
}

// The calling thread: upload and kernels of every chunk, as soon as it is packed and its device slots are free.  A status other
// than kOk is the device batch call's, its text recorded; a HIP error of this loop goes to the gate.
int32_t uploader(HostBatch& b)
{
    int32_t rc = kOk;
    hipError_t err = hipSuccess;
    std::vector<DxtltBatchItem> dev_items;
    for (int c = 0; c < b.nchunks && rc == kOk && err == hipSuccess; ++c) {
        // packed; and the download of chunk c - 2 has been ENQUEUED, so that its event exists to be waited for below
        if (!b.gate.wait([&] { return b.packed[(size_t)c] == kCopyThreads && (c < 2 || b.enqueued > c - 2); }))
            break;
        // device input slot c % 2 is rewritten here: wait for chunk c - 2's kernels (same stream: already ordered; kept
        // for clarity)
        if (c >= 2)
            err = hipStreamWaitEvent(b.up, b.ev_kernels(c - 2), 0);
        if (err == hipSuccess)
            err = hipMemcpyAsync(b.device_in(c), b.arena_in(c), (size_t)b.chunk(c).bytes, hipMemcpyHostToDevice, b.up);
        if (err == hipSuccess)
            err = hipEventRecord(b.ev_uploaded(c), b.up);
        if (err != hipSuccess)
            break;
        b.gate.publish(b.uploaded_recorded, c + 1);
        // the kernels write device output slot c % 2: chunk c - 2's download must have read it
        if (c >= 2)
            err = hipStreamWaitEvent(b.up, b.ev_downloaded(c - 2), 0);
        if (err != hipSuccess)
            break;
        const HostBatchChunk& ch = b.chunk(c);
        dev_items.clear();
        for (size_t k = ch.first; k < ch.first + ch.count; ++k) {
            DxtltBatchItem it = b.item(k);
            it.d_input = b.device_in(c) + b.slot(k);
            it.d_output = b.device_out(c) + b.slot(k);
            dev_items.push_back(it);
        }
        rc = batch_device(dev_items.data(), dev_items.size(), b.up, true);
        if (rc != kOk)
            break;
        err = hipEventRecord(b.ev_kernels(c), b.up);
        if (err != hipSuccess)
            break;
        b.gate.publish(b.kernels_issued, c + 1);
    }
    if (rc != kOk || err != hipSuccess)
        b.gate.fail(err);
    return rc;
}

}  // namespace

void dxtlt_host::release_batch_host_thread_arenas() { g_pinned.release(); }

extern "C" int32_t dxtlt_transform_batch_host(const DxtltBatchItem* items, size_t count)
{
    if (count == 0)
        return kOk;
    if (items == nullptr)
        return fail(kInvalidArgument, "NULL item array with count > 0");
    std::vector<uint64_t> len(count);
    uint64_t total = 0;
    for (size_t i = 0; i < count; ++i) {
        if (int32_t rc = batch_item_defect(items[i], 9, true); rc != kOk)
            return rc;
        len[i] = items[i].len;
        total += len[i];
    }
    if (total == 0)
        return kOk;
    const HostBatchPlan plan = plan_host_batch(len.data(), count, kHostBatchChunkBytes);
    for (size_t i = 0; i < count; ++i)
        if (plan.chunk_of_item[i] == kHostBatchAlone)
            if (int32_t rc = transform_alone(items[i]); rc != kOk)
                return rc;
    if (plan.chunks.empty())
        return kOk;

    HostBatch b(items, plan);
    if (int32_t rc = acquire(b); rc != kOk)
        return rc;
    // Every stage waits on counts that only the full set of threads reaches, so a partial set is told to leave (the gate fails),
    // joined and the streams drained like any other, and the call reports it.
    ThreadSet threads;
    for (int t = 0; t < kCopyThreads; ++t) threads.spawn(packer, &b, t);
    for (int t = 0; t < kCopyThreads; ++t) threads.spawn(unpacker, &b, t);
    threads.spawn(downloader, &b);
    int32_t rc = kOk;
    if (threads.spawn_failed)
        b.gate.fail(hipErrorOutOfMemory);
    else
        rc = uploader(b);
    // the one teardown: the events and the download stream go with `b`, behind the joins and the drains
    threads.join();
    (void)hipStreamSynchronize(b.up);
    (void)hipStreamSynchronize(b.down.stream);
    if (threads.spawn_failed)
        return fail(kAllocation, "could not start the batch copy threads");
    if (rc != kOk)
        return rc;
    if (b.gate.failed)
        return fail(kDevice, "host batch copy", b.gate.error);
    return kOk;
}

// Test hook (no device needed; include/dxtlt_gfx950.h): the call's own planner over lengths alone (tests/test_batch_host_plan.py)
extern "C" int32_t dxtlt_debug_plan_batch_host(const uint64_t* len, size_t count, uint64_t chunk_cap_bytes, uint32_t* chunk_of_item_out,
                                               uint64_t* slot_out, uint64_t* chunk_bytes_out, size_t chunk_cap, uint64_t* arena_bytes_out)
{
    if (count != 0 && len == nullptr)
        return -1;
    const HostBatchPlan plan = plan_host_batch(len, count, chunk_cap_bytes);
    for (size_t i = 0; i < count; ++i) {
        if (chunk_of_item_out) chunk_of_item_out[i] = plan.chunk_of_item[i];
        if (slot_out) slot_out[i] = plan.slot[i];
    }
    for (size_t c = 0; c < plan.chunks.size() && c < chunk_cap && chunk_bytes_out != nullptr; ++c)
        chunk_bytes_out[c] = plan.chunks[c].bytes;
    if (arena_bytes_out)
        *arena_bytes_out = plan.arena_bytes;
    return (int32_t)plan.chunks.size();
}
