// batch_auto_buffers.h -- the per-thread table staging and counters of the batched auto calls (batch_auto_api.cpp:
// dxtlt_transform_batch_auto_device; pixel_batch_auto_api.cpp: dxtlt_transform_pixels_batch_auto_device), and the chunk cap both
// cut their batches at.  Host only.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace dxtlt_host {

// this thread's table staging (mapped pinned host memory and its device twin) and counters (device and pinned host): grow-only.
// A batched auto call (batch_auto_api.cpp, pixel_batch_auto_api.cpp) waits for its stream before it returns -- the winners it leaves
// enqueued read the table ring's slots, not these -- so one of each is enough for both calls.
struct BatchAutoBuffers {
    void *table_host = nullptr, *table_mapped = nullptr, *table_dev = nullptr;
    size_t table_cap = 0;
    uint64_t *counters_dev = nullptr, *counters_host = nullptr;
    size_t counters_cap = 0;
    int device = -1;
    ~BatchAutoBuffers() { release(); }
    void release()
    {
        if (table_host) (void)hipHostFree(table_host);
        if (table_dev) (void)hipFree(table_dev);
        if (counters_dev) (void)hipFree(counters_dev);
        if (counters_host) (void)hipHostFree(counters_host);
        table_host = table_mapped = table_dev = nullptr;
        counters_dev = counters_host = nullptr;
        table_cap = counters_cap = 0;
        device = -1;
    }
    hipError_t reserve(size_t table_bytes, size_t counters)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess)
            return e;
        if (dev != device) {
            release();
            device = dev;
        }
        if (table_bytes > table_cap) {
            if (table_host) (void)hipHostFree(table_host);
            if (table_dev) (void)hipFree(table_dev);
            table_host = table_mapped = table_dev = nullptr;
            table_cap = 0;
            const size_t want = (table_bytes + table_bytes / 2 + 4095) & ~size_t(4095);
            e = hipHostMalloc(&table_host, want, hipHostMallocMapped);
            if (e == hipSuccess)
                e = hipHostGetDevicePointer(&table_mapped, table_host, 0);
            if (e == hipSuccess)
                e = hipMalloc(&table_dev, want);
            if (e != hipSuccess)
                return e;
            table_cap = want;
        }
        if (counters > counters_cap) {
            if (counters_dev) (void)hipFree(counters_dev);
            if (counters_host) (void)hipHostFree(counters_host);
            counters_dev = counters_host = nullptr;
            counters_cap = 0;
            const size_t want = counters + counters / 2 + 64;
            e = hipMalloc(reinterpret_cast<void**>(&counters_dev), want * sizeof(uint64_t));
            if (e == hipSuccess)
                e = hipHostMalloc(reinterpret_cast<void**>(&counters_host), want * sizeof(uint64_t), hipHostMallocDefault);
            if (e != hipSuccess)
                return e;
            counters_cap = want;
        }
        return hipSuccess;
    }
};

// the calling thread's buffers (batch_auto_api.cpp owns them; freed by release_batch_auto_thread_buffers)
BatchAutoBuffers& batch_auto_thread_buffers();
// the chunk cap in force on the calling thread: dxtlt_debug_batch_auto_arena_cap's value, or DXTLT_BATCH_AUTO_ARENA_CAP
uint64_t batch_auto_arena_cap();

}  // namespace dxtlt_host
