// host_staging.cpp -- how a host-resident buffer gets to a device and back: the calling thread's staging context, its
// mapped pinned pair for small buffers, the chunked pipeline for large ones, and the one round trip that chooses between
// them (host_common.h).  Format families enter as a StreamLayout and a Launch; nothing here knows a format's kernels.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <thread>

#include "granule_launch.h"
#include "host_common.h"
#include "host_pipeline.h"

namespace {

using namespace dxtlt_host;

// ---------------------------------------------------------------------------------------------------
// Per thread and device: one stream and a grow-only pair of device buffers, so that repeated calls (the reference's
// callers transform file after file) pay allocation once.
// ---------------------------------------------------------------------------------------------------
struct HostCtx {
    int device = -1;
    hipStream_t stream = nullptr;
    void* d_in = nullptr;
    void* d_out = nullptr;
    size_t cap = 0;

    ~HostCtx() { release(); }

    void release()
    {
        if (device >= 0) {
            // best effort; the runtime may already be shutting down at thread exit
            if (d_in) (void)hipFree(d_in);
            if (d_out) (void)hipFree(d_out);
            if (stream) (void)hipStreamDestroy(stream);
        }
        d_in = d_out = nullptr;
        stream = nullptr;
        cap = 0;
        device = -1;
    }

    int32_t prepare(size_t bytes)
    {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
        int dev = 0;
        HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
        if (dev != device) {
            release();
            device = dev;
            HIP_TRY(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
        }
        if (bytes > cap) {
            if (d_in) (void)hipFree(d_in);
            if (d_out) (void)hipFree(d_out);
            d_in = d_out = nullptr;
            cap = 0;
            size_t want = bytes + bytes / 8;  // a little headroom for the next, slightly larger file
            if (hipMalloc(&d_in, want) != hipSuccess || hipMalloc(&d_out, want) != hipSuccess) {
                (void)hipGetLastError();
                if (d_in) (void)hipFree(d_in);
                d_in = d_out = nullptr;
                want = bytes;
                HIP_TRY(hipMalloc(&d_in, want), "hipMalloc(input staging)");
                HIP_TRY(hipMalloc(&d_out, want), "hipMalloc(output staging)");
            }
            cap = want;
        }
        return kOk;
    }
};

thread_local HostCtx g_host_ctx;

// Small host buffers: a pair of MAPPED pinned staging buffers per thread.  The caller's bytes are copied in by the CPU,
// the kernel reads them over PCIe and writes its result straight into the second buffer, the CPU copies that out: one
// launch and one wait, no copy-engine transfers (each of which is a queue hand-over of its own; a 64 KiB call through
// two hipMemcpyAsync is 37-39 us).  Used up to kMappedMaxBytes (DXTLT_MAPPED_MAX_BYTES; 1 turns it
// off: 0, like every value env_bytes cannot read, means the default).
struct MappedPair {
    int device = -1;
    void* h_in = nullptr;
    void* h_out = nullptr;
    void* d_in = nullptr;   // device-side addresses of the two host buffers
    void* d_out = nullptr;
    size_t cap = 0;

    ~MappedPair() { release(); }
    void release()
    {
        if (h_in) (void)hipHostFree(h_in);
        if (h_out) (void)hipHostFree(h_out);
        h_in = h_out = d_in = d_out = nullptr;
        cap = 0;
        device = -1;
    }
    hipError_t reserve(int dev, size_t bytes)
    {
        if (dev == device && bytes <= cap)
            return hipSuccess;
        release();
        const size_t want = std::max<size_t>(bytes, 64u << 10);
        hipError_t e = hipHostMalloc(&h_in, want, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostMalloc(&h_out, want, hipHostMallocMapped);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d_in, h_in, 0);
        if (e == hipSuccess) e = hipHostGetDevicePointer(&d_out, h_out, 0);
        if (e != hipSuccess) {
            release();
            return e;
        }
        device = dev;
        cap = want;
        return hipSuccess;
    }
};
thread_local MappedPair g_mapped;

// ---------------------------------------------------------------------------------------------------
// Thresholds; overridable once per process through the environment for experiments (DXTLT_PIPELINE_MIN_BYTES,
// DXTLT_PIPELINE_CHUNK_BYTES, DXTLT_MAPPED_MAX_BYTES).
// ---------------------------------------------------------------------------------------------------
size_t env_bytes(const char* name, size_t fallback)
{
    const char* v = std::getenv(name);
    if (v == nullptr || *v == 0)
        return fallback;
    const unsigned long long x = std::strtoull(v, nullptr, 10);
    return x ? (size_t)x : fallback;
}
// Measured (profiles/r01_j_*): one-shot H2D + kernel + D2H runs at ~25.5 GiB/s at every size; the pipeline costs
// ~150 us per chunk and only wins from ~100 MiB up (16 MiB chunks: 32 / 36 / 38 GiB/s at 128 / 256 / 512 MiB; 32 MiB
// chunks: 40-42 GiB/s from 512 MiB up).
const size_t kPipelineMinBytes = env_bytes("DXTLT_PIPELINE_MIN_BYTES", 96u << 20);
// Up to 1 MiB the mapped staging pair wins (tools/host_path_latency.py: 4 KiB 30 -> 17 us per call, 64 KiB 37 -> 20,
// 256 KiB 52 -> 34, 1 MiB 120 -> 101; at 4 MiB it loses, 347 against 194: lanes reading host memory reach ~12 GiB/s
// where the copy engines reach 25).
const size_t kMappedMaxBytes = env_bytes("DXTLT_MAPPED_MAX_BYTES", 1u << 20);
const uint64_t kPipelineChunkOverride = env_bytes("DXTLT_PIPELINE_CHUNK_BYTES", 0) & ~(uint64_t)0xFFFF;

// Chunk size, formats 1-5.  BC3's six streams include two of a sixteenth of the data each: with 16 MiB chunks their
// downloads are 1 MiB copies and the pipeline falls to 22-30 GiB/s between 256 MiB and 1 GiB; 32 MiB chunks give 35-40
// there (tools/host_chunk_sweep.py, round 2).  BC1 / BC2 keep 16 MiB chunks below 256 MiB (one more GiB/s at 128 MiB).
uint64_t block_chunk_bytes(uint64_t len, int format)
{
    return (format >= 3 || len >= (256ull << 20)) ? (32ull << 20) : (16ull << 20);   // (BC4 / BC5: streams of 1/8 of the data too)
}
// Chunk size, formats 6-7.  Eight downloads per chunk, five of them a sixteenth of it: larger chunks than BC1-3 (16 MiB
// chunks lose to the one-shot path below 1 GiB; 32 MiB: 30 / 34 / 37 GiB/s at 128 / 256 / 512 MiB; 64 MiB: 40-41 from
// 1 GiB up; tools/bc7_host_bench.py)
uint64_t granule_chunk_bytes(uint64_t len) { return len >= (1ull << 30) ? (64ull << 20) : (32ull << 20); }

uint64_t pipeline_chunk_bytes(const StreamLayout& L, uint64_t len)
{
    if (kPipelineChunkOverride)
        return kPipelineChunkOverride;
    return dxtlt::granule::is_granule_format(L.format) ? granule_chunk_bytes(len) : block_chunk_bytes(len, L.format);
}

// dxtlt_debug_host_route_counts: which arm every host round trip and shard transfer of this process took (HostRoute)
std::atomic<uint64_t> g_route_counts[kRouteCount];

}  // namespace

bool dxtlt_host::pipeline_pays(uint64_t bytes) { return bytes >= kPipelineMinBytes; }

void dxtlt_host::count_route(HostRoute route) { g_route_counts[route].fetch_add(1, std::memory_order_relaxed); }

extern "C" void dxtlt_debug_host_route_counts(uint64_t out[5])
{
    for (int r = 0; out != nullptr && r < kRouteCount; ++r)
        out[r] = g_route_counts[r].load(std::memory_order_relaxed);
}

// ---------------------------------------------------------------------------------------------------
// Chunked host path: H2D of chunk k+1, the kernel of chunk k and D2H of chunk k-1 overlap.
// Copies from/to pageable host memory block the calling thread while the runtime stages them, so the two
// directions are driven by two host threads: the caller uploads and launches (stream `up`), a helper thread
// downloads (stream `down`) as soon as the chunk's event has fired.  PCIe is full duplex; the kernel time is
// negligible next to either copy.  A chunk is a block range of the whole array (dxtlt_transform_range_device
// semantics), so on the SoA side every chunk moves one slice per stream.
//
// The device holds the range as a stand-alone array of `count` blocks (d_in / d_out of count * B bytes: AoS slice
// and compact SoA, which IS the range's slice of every stream, packed); host offsets are those of the whole array.
// With first = 0 and count = total this is the whole-buffer pipeline of the host-pointer entry points; with a proper
// sub-range it is one shard of a sharded call.
// ---------------------------------------------------------------------------------------------------
int32_t dxtlt_host::pipelined_range(const StreamLayout& S, const Launch& launch, const DeviceStaging& d, bool inverse,
                                    const uint8_t* in, uint8_t* out, uint64_t total, uint64_t base, uint64_t blocks)
{
    const uint64_t B = S.block_bytes;
    // a multiple of every tile size (and of the sort granule); 3-byte pixels do not divide a power of two: rounded down
    uint64_t chunk_blocks = pipeline_chunk_bytes(S, blocks * B) / B;
    chunk_blocks -= chunk_blocks % S.align_blocks;
    const int nchunks = (int)((blocks + chunk_blocks - 1) / chunk_blocks);
    const int dev = d.dev;
    count_route(kRoutePipelinedRange);

    // the download stream and one event per chunk; they go with this call, behind the drains at its end
    OwnedStream down_stream;
    HIP_TRY(down_stream.create(), "hipStreamCreate(download)");
    const hipStream_t down = down_stream.stream;
    EventList ev;
    HIP_TRY(ev.create((size_t)nchunks, hipEventDisableTiming), "hipEventCreate");

    StageGate gate;     // fails when the uploader gives up
    int launched = 0;   // chunks whose kernel (and event) have been enqueued
    hipError_t down_err = hipSuccess;
    std::thread downloader([&] {
        hipError_t e = hipSetDevice(dev);
        for (int k = 0; k < nchunks && e == hipSuccess; ++k) {
            if (!gate.wait_reached([&] { return launched > k; }))
                break;  // uploader failed before this chunk
            const uint64_t first = (uint64_t)k * chunk_blocks;
            const uint64_t count = std::min<uint64_t>(chunk_blocks, blocks - first);
            e = hipStreamWaitEvent(down, ev[(size_t)k], 0);
            if (!inverse) {
                for (int s = 0; s < S.n && e == hipSuccess; ++s) {
                    const uint64_t w = S.width[s], off = S.off[s];
                    e = hipMemcpyAsync(out + off * total + w * (base + first),
                                       (const uint8_t*)d.d_out + off * blocks + w * first, (size_t)(w * count),
                                       hipMemcpyDeviceToHost, down);
                }
            } else if (e == hipSuccess) {
                e = hipMemcpyAsync(out + (base + first) * B, (const uint8_t*)d.d_out + first * B, (size_t)(count * B),
                                   hipMemcpyDeviceToHost, down);
            }
        }
        // drain whatever was enqueued, also after a failure: the events and the stream die with this call
        hipError_t e2 = hipStreamSynchronize(down);
        down_err = e != hipSuccess ? e : e2;
    });

    hipError_t up_err = hipSuccess;
    int32_t rc = kOk;
    for (int k = 0; k < nchunks; ++k) {
        const uint64_t first = (uint64_t)k * chunk_blocks;
        const uint64_t count = std::min<uint64_t>(chunk_blocks, blocks - first);
        if (!inverse) {
            up_err = hipMemcpyAsync((uint8_t*)d.d_in + first * B, in + (base + first) * B, (size_t)(count * B),
                                    hipMemcpyHostToDevice, d.up);
            if (up_err == hipSuccess)
                rc = launch(false, (const uint8_t*)d.d_in + first * B, d.d_out, blocks, first, count, d.up);
        } else {
            for (int s = 0; s < S.n && up_err == hipSuccess; ++s) {
                const uint64_t w = S.width[s], off = S.off[s];
                up_err = hipMemcpyAsync((uint8_t*)d.d_in + off * blocks + w * first, in + off * total + w * (base + first),
                                        (size_t)(w * count), hipMemcpyHostToDevice, d.up);
            }
            if (up_err == hipSuccess)
                rc = launch(true, d.d_in, (uint8_t*)d.d_out + first * B, blocks, first, count, d.up);
        }
        if (up_err == hipSuccess && rc == kOk)
            up_err = hipEventRecord(ev[(size_t)k], d.up);
        if (up_err == hipSuccess && rc == kOk)
            count_route(kRoutePipelineChunk);
        if (up_err != hipSuccess || rc != kOk) {
            gate.fail(up_err);
            break;
        }
        gate.publish(launched, k + 1);
    }
    downloader.join();
    // every exit drains the upload stream before the events go away and the staging buffers can be reused
    // (a failed copy or launch leaves earlier chunks queued)
    const hipError_t drain = hipStreamSynchronize(d.up);
    if (up_err == hipSuccess && rc == kOk)
        up_err = drain;
    if (rc != kOk)
        return rc;
    if (up_err != hipSuccess)
        return fail(kDevice, "pipelined upload/launch", up_err);
    if (down_err != hipSuccess)
        return fail(kDevice, "pipelined download", down_err);
    return kOk;
}

int32_t dxtlt_host::acquire_staging(size_t bytes, void** d_in, void** d_out, hipStream_t* stream)
{
    HostCtx& c = g_host_ctx;
    int32_t rc = c.prepare(bytes);
    if (rc != kOk)
        return rc;
    *d_in = c.d_in;
    *d_out = c.d_out;
    *stream = c.stream;
    return kOk;
}

int32_t dxtlt_host::acquire_mapped_staging(size_t bytes, MappedStaging* out)
{
    out->usable = false;
    if (bytes > kMappedMaxBytes)
        return kOk;
    HostCtx& c = g_host_ctx;
    int32_t rc = c.prepare(0);   // device and stream only
    if (rc != kOk)
        return rc;
    MappedPair& m = g_mapped;
    HIP_TRY(m.reserve(c.device, bytes), "hipHostMalloc(mapped staging)");
    *out = MappedStaging{true, m.h_in, m.h_out, m.d_in, m.d_out, c.stream};
    return kOk;
}

// Mapped staging is asked first, the pipeline second.  With the shipped thresholds the order cannot matter: the mapped
// pair ends at 1 MiB and the pipeline starts at 96 MiB.  If the environment variables cross them, a buffer both would
// take goes through the mapped pair.
int32_t dxtlt_host::host_round_trip(const StreamLayout& L, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out,
                                    uint64_t blocks)
{
    const size_t len = (size_t)(blocks * L.block_bytes);
    MappedStaging m;
    int32_t rc = acquire_mapped_staging(len, &m);
    if (rc != kOk)
        return rc;
    if (m.usable) {
        // the kernel reads and writes mapped pinned staging itself (no copy-engine hand-overs)
        count_route(kRouteMapped);
        std::memcpy(m.h_in, in, len);
        rc = launch(inverse, m.d_in, m.d_out, blocks, 0, blocks, m.stream);
        const hipError_t drained = hipStreamSynchronize(m.stream);
        if (rc != kOk)
            return rc;
        HIP_TRY(drained, "stream synchronize");
        std::memcpy(out, m.h_out, len);
        return kOk;
    }
    HostCtx& c = g_host_ctx;
    rc = c.prepare(len);
    if (rc != kOk)
        return rc;
    if (pipeline_pays(len))
        return pipelined_range(L, launch, DeviceStaging{c.device, c.stream, c.d_in, c.d_out}, inverse, in, out, blocks, 0, blocks);
    // Every exit drains the stream first: the staging buffers belong to this thread's next call, which may free or
    // regrow them while an earlier copy or kernel of this one is still queued.
    count_route(kRouteOneShot);
    hipError_t e = hipMemcpyAsync(c.d_in, in, len, hipMemcpyHostToDevice, c.stream);
    const char* what = "H2D copy";
    if (e == hipSuccess) {
        rc = launch(inverse, c.d_in, c.d_out, blocks, 0, blocks, c.stream);
        if (rc == kOk) {
            e = hipMemcpyAsync(out, c.d_out, len, hipMemcpyDeviceToHost, c.stream);
            what = "D2H copy";
        }
    }
    const hipError_t drained = hipStreamSynchronize(c.stream);
    if (rc != kOk)
        return rc;
    if (e != hipSuccess)
        return fail(kDevice, what, e);
    HIP_TRY(drained, "stream synchronize");
    return kOk;
}

void dxtlt_host::release_thread_staging()
{
    g_host_ctx.release();
    g_mapped.release();
}
