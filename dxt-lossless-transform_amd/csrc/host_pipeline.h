// host_pipeline.h -- what the host-side pipelines are made of, written once: the owner of a non-blocking stream, the owner of a list
// of events, the gate their stages meet at, and the set of threads a call starts.  Users: the host batch (batch_host_api.cpp), the
// chunked single-buffer pipeline (host_staging.cpp: pipelined_range) and the bench hooks' events of the batched auto calls
// (batch_auto_common.h: PhaseEvents).  The two pipelines differ in what a chunk is; only their resources and their gate are shared.
// Host only.  Not installed.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

#include <condition_variable>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

namespace dxtlt_host {

// A non-blocking stream that dies with its scope.  Whoever enqueues on it drains it first.
struct OwnedStream {
    hipStream_t stream = nullptr;
    OwnedStream() = default;
    OwnedStream(const OwnedStream&) = delete;
    OwnedStream& operator=(const OwnedStream&) = delete;
    ~OwnedStream()
    {
        if (stream) (void)hipStreamDestroy(stream);
    }
    hipError_t create() { return hipStreamCreateWithFlags(&stream, hipStreamNonBlocking); }
};

// n events that die with their scope.  A failed create() leaves the list empty: it holds all n events or none.
struct EventList {
    std::vector<hipEvent_t> ev;
    EventList() = default;
    EventList(const EventList&) = delete;
    EventList& operator=(const EventList&) = delete;
    ~EventList() { clear(); }
    void clear()
    {
        for (hipEvent_t e : ev)
            (void)hipEventDestroy(e);
        ev.clear();
    }
    hipError_t create(size_t n, unsigned flags)
    {
        ev.reserve(n);
        for (size_t i = 0; i < n; ++i) {
            hipEvent_t e = nullptr;
            if (hipError_t err = hipEventCreateWithFlags(&e, flags); err != hipSuccess) {
                clear();
                return err;
            }
            ev.push_back(e);
        }
        return hipSuccess;
    }
    bool empty() const { return ev.empty(); }
    hipEvent_t operator[](size_t k) const { return ev[k]; }
};

// Where the stages of a pipeline meet: every counter a stage publishes and another waits for is written and read under the gate's
// mutex, and a stage that gives up says so here -- the first error is kept -- which ends every wait.
struct StageGate {
    std::mutex m;
    std::condition_variable cv;
    bool failed = false;
    hipError_t error = hipSuccess;   // of the first fail()

    template <class T>
    void publish(T& counter, T value)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            counter = value;
        }
        cv.notify_all();
    }
    template <class T>
    void increment(T& counter)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            ++counter;
        }
        cv.notify_all();
    }
    // Waits until `ready()` holds or the call is being abandoned; false when it is being abandoned, whatever `ready()` says.
    template <class Ready>
    bool wait(Ready&& ready)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return ready() || failed; });
        return !failed;
    }
    // The same wait for a stage that still serves what was published before the call was abandoned: false only when `ready()` does
    // not hold -- this chunk was never reached.
    template <class Ready>
    bool wait_reached(Ready&& ready)
    {
        std::unique_lock<std::mutex> lk(m);
        cv.wait(lk, [&] { return ready() || failed; });
        return ready();
    }
    void fail(hipError_t e)
    {
        {
            std::lock_guard<std::mutex> lk(m);
            if (!failed) {
                failed = true;
                error = e;
            }
        }
        cv.notify_all();
    }
};

// The threads a call starts.  Thread creation can fail (EAGAIN under a process limit): nothing more is started then, and the caller
// tells the partial set to leave before it joins it.
struct ThreadSet {
    std::vector<std::thread> threads;
    bool spawn_failed = false;
    template <class Fn, class... Args>
    void spawn(Fn&& fn, Args... args)
    {
        if (spawn_failed)
            return;
        try {
            threads.emplace_back(fn, args...);
        } catch (const std::exception&) {
            spawn_failed = true;
        }
    }
    void join()
    {
        for (std::thread& t : threads)
            t.join();
        threads.clear();
    }
};

}  // namespace dxtlt_host
