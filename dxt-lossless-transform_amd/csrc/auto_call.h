// auto_call.h -- the host frame every single-buffer auto call is written in: auto_transform.cpp (BC1-BC5), auto_normalize_api.cpp
// (BC1 / BC2 with block normalisation) and pixel_auto_api.cpp (pixels).  What a family adds is its flow -- its candidates, its
// estimates and its pick --; the guards, the staging and the per-thread state around it are here.  Not installed; the non-template
// definitions are in auto_transform.cpp.
#pragma once
#include <algorithm>
#include <cstdlib>

#include "host_common.h"

namespace dxtlt_host {

// THE invariant of every auto route: no exit returns while work that reads or writes this thread's staging buffers, pinned stage,
// arena, flag word or estimate counters is in flight -- they belong to this thread's next call.  Armed once anything has been
// enqueued, the guard waits for the stream on every exit; the success path waits itself (it has to report a failure of the wait)
// and disarms it.
struct StreamDrain {
    hipStream_t stream = nullptr;
    bool armed = false;
    ~StreamDrain()
    {
        if (armed) (void)hipStreamSynchronize(stream);
    }
};

// Estimator scratch of one thread: 64-byte aligned, freed on every exit.
struct EstimatorScratch {
    uint8_t* ptr = nullptr;
    EstimatorScratch() = default;
    EstimatorScratch(const EstimatorScratch&) = delete;
    ~EstimatorScratch() { std::free(ptr); }
    bool allocate(size_t max_comp)   // nothing for max_comp == 0
    {
        if (max_comp != 0)
            ptr = static_cast<uint8_t*>(std::aligned_alloc(64, (max_comp + 63) / 64 * 64));
        return max_comp == 0 || ptr != nullptr;
    }
};

// A grow-only per-thread buffer, like the staging buffers: the candidate arena (device memory, of the device it was allocated on)
// and the pinned stage of the callback flow's section downloads.
struct AutoArena {
    void* ptr = nullptr;
    size_t cap = 0;
    int device = -1;
    ~AutoArena() { release(); }
    void release();
    void* get(size_t bytes);   // on the current device, at least `bytes`; nullptr when it cannot be allocated
};
struct AutoHostStage {
    void* ptr = nullptr;
    size_t cap = 0;
    ~AutoHostStage() { release(); }
    void release();
    void* get(size_t bytes);
};

// What the auto calls of a thread keep between and about their calls.
constexpr int kAutoTotalsCap = 192;  // the most candidates a single-buffer call compares (auto_normalize_api.cpp, BC3, all modes)
struct AutoThreadState {
    // dxtlt_debug_auto_last_estimation: what the last auto call of this thread downloaded and called for its estimates
    uint64_t section_bytes_downloaded = 0, estimator_callbacks = 0;
    // dxtlt_debug_auto_last_totals: the totals the last built-in-estimator call compared, in its candidate order
    uint64_t last_totals[kAutoTotalsCap] = {};
    int last_total_count = 0;
    bool no_arena = false;   // dxtlt_debug_auto_use_arena(0): every auto route as if the arena could not be allocated
    AutoArena arena;
    AutoHostStage stage;

    // a call begins: nothing downloaded, no callback made and no totals of an earlier call
    void begin_call()
    {
        last_total_count = 0;
        section_bytes_downloaded = estimator_callbacks = 0;
    }
    void set_last_totals(const uint64_t* totals, int count)
    {
        last_total_count = std::min(count, kAutoTotalsCap);
        std::copy(totals, totals + last_total_count, last_totals);
    }
};
AutoThreadState& auto_state();

// A C out-parameter that may be NULL.
template <class T, class V>
void store_if(T* ptr, V value)
{
    if (ptr) *ptr = static_cast<T>(value);
}

// What a call on the caller's device pointers and stream needs before it enqueues: a device (kNoDevice without one) and a stream
// that is not capturing -- every auto call reads its estimates back and waits.
int32_t auto_device_preconditions(hipStream_t stream);

// The device-pointer call of a family: the preconditions, then flow().  A failing flow is waited for before its code is returned:
// the arena and the counters belong to this thread's next call.
template <class Flow>
int32_t auto_device_call(hipStream_t stream, Flow flow)
{
    if (int32_t rc = auto_device_preconditions(stream))
        return rc;
    const int32_t rc = flow();
    if (rc != kOk)
        (void)hipStreamSynchronize(stream);
    return rc;
}

// The host-pointer call of a family with a built-in estimator, len > 0: one upload into this thread's staging buffers,
// flow(d_in, d_out, stream) -- the family's *_on_device, which leaves the winner's transform enqueued --, one download.  The
// stream is waited for on every exit; the first failure is the one reported.
template <class Flow>
int32_t auto_staged_call(const uint8_t* in, uint8_t* out, size_t len, Flow flow)
{
    void *d_in = nullptr, *d_out = nullptr;
    hipStream_t st = nullptr;
    if (int32_t rc = acquire_staging(len, &d_in, &d_out, &st))
        return rc;
    hipError_t e = hipMemcpyAsync(d_in, in, len, hipMemcpyHostToDevice, st);
    int32_t rc = e == hipSuccess ? flow(d_in, d_out, st) : fail(kDevice, "H2D copy", e);
    if (rc == kOk && (e = hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, st)) != hipSuccess)
        rc = fail(kDevice, "D2H result", e);
    e = hipStreamSynchronize(st);
    if (rc == kOk && e != hipSuccess)
        rc = fail(kDevice, "stream synchronize", e);
    return rc;
}

}  // namespace dxtlt_host
