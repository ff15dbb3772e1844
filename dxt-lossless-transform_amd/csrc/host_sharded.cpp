// host_sharded.cpp -- single-process multi-GPU shard path of every format family: contiguous block
// ranges, one host thread per shard, no collective.  A shard is transformed as a stand-alone buffer on its device (blocks
// are independent -- for the granule formats, sort granules are -- so its compact result holds exactly this shard's slice
// of every stream, packed); the "host concat" is one copy per stream slice straight to the slice's final place.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <chrono>
#include <exception>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "host_common.h"

namespace {

using namespace dxtlt_host;

struct ShardPlan {
    uint64_t first;
    uint64_t count;
};

std::vector<ShardPlan> plan_shards(uint64_t total_blocks, int shards, uint64_t align_blocks)
{
    // equal shares rounded down to a multiple of `align_blocks` (keeps every per-stream slice 16-byte aligned and
    // tile- or granule-sized); the last shard takes the remainder, a granule format's tail part included
    std::vector<ShardPlan> p((size_t)shards);
    uint64_t share = total_blocks / (uint64_t)shards;
    share -= share % align_blocks;
    uint64_t at = 0;
    for (int i = 0; i < shards; ++i) {
        uint64_t n = (i == shards - 1) ? total_blocks - at : share;
        p[(size_t)i] = {at, n};
        at += n;
    }
    return p;
}

// Per-device shard contexts (a stream and a grow-only pair of device buffers), kept across sharded calls: the shard
// threads are new on every call, so thread-local staging as in the host-pointer path would be allocated and freed each
// time -- two hipMalloc / hipFree of the shard's size per call cost a 4 GiB BC3 array 30 ms of its 130 (pinned host
// memory) and far more with pageable memory (13 against 41 GiB/s through the single-buffer entry point;
// tools/pinned_host_probe.py).  dxtlt_release_thread_resources() frees the idle ones.
struct ShardCtx {
    int dev = -1;
    hipStream_t st = nullptr;
    void* a = nullptr;
    void* b = nullptr;
    size_t cap = 0;
    bool busy = false;
};
std::mutex g_shard_pool_mutex;
std::vector<ShardCtx*> g_shard_pool;

ShardCtx* shard_ctx_acquire(int dev, size_t bytes, hipError_t* err)
{
    ShardCtx* c = nullptr;
    {
        std::lock_guard<std::mutex> lk(g_shard_pool_mutex);
        for (ShardCtx* x : g_shard_pool)
            if (!x->busy && x->dev == dev && (c == nullptr || x->cap > c->cap))
                c = x;
        if (c == nullptr) {
            c = new ShardCtx();
            c->dev = dev;
            g_shard_pool.push_back(c);
        }
        c->busy = true;
    }
    *err = hipSuccess;
    if (c->st == nullptr)
        *err = hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking);
    if (*err == hipSuccess && c->cap < bytes) {
        if (c->a) (void)hipFree(c->a);
        if (c->b) (void)hipFree(c->b);
        c->a = c->b = nullptr;
        c->cap = 0;
        *err = hipMalloc(&c->a, bytes);
        if (*err == hipSuccess)
            *err = hipMalloc(&c->b, bytes);
        if (*err == hipSuccess) {
            c->cap = bytes;
        } else {
            if (c->a) (void)hipFree(c->a);
            c->a = c->b = nullptr;
        }
    }
    if (*err != hipSuccess) {
        (void)hipGetLastError();
        std::lock_guard<std::mutex> lk(g_shard_pool_mutex);
        c->busy = false;
        return nullptr;
    }
    return c;
}

// At most kIdleShardCtxPerDevice idle contexts stay per device (the largest ones): a call with 64 round-robin shards on
// one device would otherwise leave 64 streams and 2 x the array size of HBM behind until someone calls
// dxtlt_release_thread_resources().  Retained memory per device is thus bounded by 2 buffers x the largest shard x 2.
constexpr int kIdleShardCtxPerDevice = 2;

// Handing a context back only marks it idle: hipFree synchronises the whole device, so nothing is freed on a shard's
// completion path while other shards of the call are still moving data.  The surplus is trimmed by the call itself, after
// its workers have joined (shard_pool_trim).
void shard_ctx_release(ShardCtx* c)
{
    std::lock_guard<std::mutex> lk(g_shard_pool_mutex);
    c->busy = false;
}

// Contexts already taken out of the pool: their buffers and streams freed on their devices, the caller's device restored
void shard_ctx_free(const std::vector<ShardCtx*>& gone)
{
    if (gone.empty())
        return;
    int prev = 0;
    (void)hipGetDevice(&prev);
    for (ShardCtx* x : gone) {
        if (hipSetDevice(x->dev) == hipSuccess) {
            if (x->a) (void)hipFree(x->a);
            if (x->b) (void)hipFree(x->b);
            if (x->st) (void)hipStreamDestroy(x->st);
        }
        delete x;
    }
    (void)hipSetDevice(prev);
}

void shard_pool_trim()
{
    std::vector<ShardCtx*> drop;
    {
        std::lock_guard<std::mutex> lk(g_shard_pool_mutex);
        std::vector<ShardCtx*> idle;
        for (ShardCtx* x : g_shard_pool)
            if (!x->busy)
                idle.push_back(x);
        // per device: keep the kIdleShardCtxPerDevice largest idle contexts
        std::sort(idle.begin(), idle.end(), [](const ShardCtx* l, const ShardCtx* r) { return l->dev != r->dev ? l->dev < r->dev : l->cap > r->cap; });
        int run = 0;
        for (size_t i = 0; i < idle.size(); ++i) {
            run = (i > 0 && idle[i]->dev == idle[i - 1]->dev) ? run + 1 : 0;
            if (run >= kIdleShardCtxPerDevice)
                drop.push_back(idle[i]);
        }
        for (ShardCtx* x : drop)
            g_shard_pool.erase(std::find(g_shard_pool.begin(), g_shard_pool.end(), x));
    }
    shard_ctx_free(drop);
}

// One stand-alone buffer of `count` blocks at AoS byte `aos_off`, one shot on the shard's stream: forward = AoS slice
// up, launch, one D2H per slice to its final host offset; inverse = one H2D per slice into a compact buffer, launch,
// AoS down.  The stream is drained on every exit.
int32_t one_shot(const ShardCtx& c, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out, uint64_t aos_off,
                 uint64_t count, uint64_t B, const Slice* sl, int n)
{
    const size_t bytes = (size_t)(count * B);
    hipError_t e = hipSuccess;
    int32_t rc = kOk;
    count_route(kRouteShardOneShot);
    if (!inverse) {
        e = hipMemcpyAsync(c.a, in + aos_off, bytes, hipMemcpyHostToDevice, c.st);
        if (e == hipSuccess)
            rc = launch(false, c.a, c.b, count, 0, count, c.st);
        for (int s = 0; s < n && e == hipSuccess && rc == kOk; ++s)
            if (sl[s].bytes)
                e = hipMemcpyAsync(out + sl[s].host_off, (const uint8_t*)c.b + sl[s].dev_off, (size_t)sl[s].bytes,
                                   hipMemcpyDeviceToHost, c.st);
    } else {
        for (int s = 0; s < n && e == hipSuccess; ++s)
            if (sl[s].bytes)
                e = hipMemcpyAsync((uint8_t*)c.a + sl[s].dev_off, in + sl[s].host_off, (size_t)sl[s].bytes,
                                   hipMemcpyHostToDevice, c.st);
        if (e == hipSuccess)
            rc = launch(true, c.a, c.b, count, 0, count, c.st);
        if (e == hipSuccess && rc == kOk)
            e = hipMemcpyAsync(out + aos_off, c.b, bytes, hipMemcpyDeviceToHost, c.st);
    }
    const hipError_t drained = hipStreamSynchronize(c.st);
    if (rc != kOk)
        return rc;
    if (e == hipSuccess)
        e = drained;
    return e == hipSuccess ? kOk : fail(kDevice, "shard copy/launch", e);
}

// Blocks [sp.first, sp.first + sp.count) of the array on device `dev`.  `main_total` blocks of the array lie in the
// streams; what a shard holds beyond them (the last shard of a granule format only) is the array's tail part.
int32_t shard_worker(int dev, const StreamLayout& L, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out,
                     uint64_t main_total, ShardPlan sp)
{
    if (sp.count == 0)
        return kOk;
    const uint64_t B = L.block_bytes;
    const uint64_t in_main = sp.first >= main_total ? 0 : std::min<uint64_t>(sp.first + sp.count, main_total) - sp.first;
    const uint64_t tail = sp.count - in_main;
    Slice sl[9];
    shard_slices(L, main_total, sp.first, in_main, tail, sl);
    HIP_TRY(hipSetDevice(dev), "hipSetDevice");
    hipError_t acquire_err = hipSuccess;
    ShardCtx* ctx = shard_ctx_acquire(dev, (size_t)(sp.count * B), &acquire_err);
    if (ctx == nullptr)
        return fail(kDevice, "shard stream / buffers", acquire_err);
    int32_t rc;
    if (in_main != 0 && pipeline_pays(in_main * B)) {
        // large shard: upload, kernel and the per-stream downloads of consecutive chunks overlap; its share of the tail
        // part afterwards, one shot
        rc = pipelined_range(L, launch, DeviceStaging{dev, ctx->st, ctx->a, ctx->b}, inverse, in, out, main_total, sp.first, in_main);
        if (rc == kOk && tail != 0) {
            const Slice whole{sl[L.n].host_off, 0, sl[L.n].bytes};
            rc = one_shot(*ctx, launch, inverse, in, out, main_total * B, tail, B, &whole, 1);
        }
    } else {
        rc = one_shot(*ctx, launch, inverse, in, out, sp.first * B, sp.count, B, sl, L.n + 1);
    }
    shard_ctx_release(ctx);   // both paths have drained the stream
    return rc;
}

}  // namespace

void dxtlt_host::shard_slices(const StreamLayout& L, uint64_t main_total, uint64_t first, uint64_t in_main, uint64_t tail, Slice* out)
{
    for (int s = 0; s < L.n; ++s)
        out[s] = {L.off[s] * main_total + L.width[s] * first, L.off[s] * in_main, L.width[s] * in_main};
    out[L.n] = {L.block_bytes * main_total, L.block_bytes * in_main, L.block_bytes * tail};
}

void dxtlt_host::release_idle_shard_contexts()
{
    std::vector<ShardCtx*> idle;
    {
        std::lock_guard<std::mutex> lk(g_shard_pool_mutex);
        std::vector<ShardCtx*> keep;
        for (ShardCtx* x : g_shard_pool)
            (x->busy ? keep : idle).push_back(x);
        g_shard_pool.swap(keep);
    }
    shard_ctx_free(idle);
}

int32_t dxtlt_host::run_sharded(const StreamLayout& L, const Launch& launch, bool inverse, const uint8_t* in, uint8_t* out,
                                uint64_t total, uint64_t tail, int32_t num_shards, std::vector<DxtltShardStat>* stats_out)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    // more shards than devices are dealt round robin (a 1-GPU box runs the multi-shard placement that way)
    int shards = num_shards <= 0 ? count : std::min(num_shards, 64);
    const uint64_t units = (total + L.shard_unit - 1) / L.shard_unit;
    if ((uint64_t)shards > units)
        shards = (int)units;
    int prev = 0;
    (void)hipGetDevice(&prev);

    const std::vector<ShardPlan> plan = plan_shards(total, shards, L.align_blocks);
    std::vector<int32_t> codes((size_t)shards, kOk);
    std::vector<std::string> msgs((size_t)shards);
    std::vector<DxtltShardStat> stats((size_t)shards);
    std::vector<std::thread> threads;
    // The workers narrow their own affinity before their first HIP call, and threads the HIP / ROCr runtime starts lazily
    // from a worker would inherit that mask for the life of the process.  So the runtime is brought up for every device
    // this call uses HERE, on the caller's unbound thread, before any worker exists (DXTLT_NUMA_BIND in the header).
    for (int d = 0; d < std::min(shards, count); ++d)
        if (hipSetDevice(d) == hipSuccess)
            (void)hipFree(nullptr);
    (void)hipSetDevice(prev);
    // thread creation can fail (EAGAIN under a process limit): whatever was started is joined before the error leaves
    bool spawn_failed = false;
    for (int d = 0; d < shards && !spawn_failed; ++d) {
        try {
            threads.emplace_back([&, d] {
                // this thread is the library's own: put it next to its device before it submits anything (the pipeline's
                // downloader thread is created from it and inherits the mask)
                const int bound = bind_this_thread_near_device(d % count);
                const auto t0 = std::chrono::steady_clock::now();
                codes[(size_t)d] = shard_worker(d % count, L, launch, inverse, in, out, total - tail, plan[(size_t)d]);
                const double dt = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                stats[(size_t)d] = DxtltShardStat{d % count, bound, plan[(size_t)d].first, plan[(size_t)d].count, dt};
                if (codes[(size_t)d] != kOk)
                    msgs[(size_t)d] = dxtlt_last_error();
            });
        } catch (const std::exception&) {
            spawn_failed = true;
        }
    }
    for (auto& t : threads)
        t.join();
    shard_pool_trim();   // idle contexts beyond the cap, now that no shard of this call is moving data
    (void)hipSetDevice(prev);
    if (stats_out != nullptr)
        *stats_out = stats;
    if (spawn_failed)
        return fail(kAllocation, "could not start a shard worker thread");   // a host resource ran out (batch_host, auto pool: the same code)
    for (int d = 0; d < shards; ++d)
        if (codes[(size_t)d] != kOk)
            return fail_verbatim(codes[(size_t)d], msgs[(size_t)d].c_str());
    return kOk;
}
