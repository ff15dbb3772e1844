// table_ring.h -- staging of the tables of the batch calls (batch_api.cpp: dxtlt_transform_batch_device; image_batch_api.cpp:
// dxtlt_untransform_decode_images_batch_device; bc7_image_batch_api.cpp: dxtlt_untransform_decode_bc7_images_batch_device): pinned
// host slots with device twins, one ring per calling thread.  The three calls take and give back their slot through StagedTables
// (batch_tables.h), which alone records a slot's event and sets `pending`.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>

namespace dxtlt_host {

// Table staging: a ring of pinned host buffers with device twins.  A slot is reused only after the copy and the kernels that last
// read it have finished (its event).  A call takes exactly ONE slot -- the tables of its two BC7 launches and of all its BC1-3
// groups share one staged buffer and one upload -- so it never waits for its own work, and its acquire blocks the host only when
// kTableSlots earlier calls of this thread are all still in flight.  (Until round 6 a call with BC7 forward, BC7 inverse and BC1-3
// items took three slots: the next such call's second acquire landed on a slot the previous call had left pending and waited in
// hipEventSynchronize for that call's kernels -- an "asynchronous" call that host-blocked with a single earlier call in flight,
// which dxtlt_transform_batch_host hit on every chunk.  Sixteen mixed calls back to back: enqueued in 0.66 ms instead of 1.0 ms, finished
// 20 % sooner: profiles/r06_batch_one_slot.txt.)
constexpr int kTableSlots = 4;

struct TableSlot {
    void* host = nullptr;
    void* host_mapped = nullptr;   // the device-side address of `host`
    void* dev = nullptr;
    size_t cap = 0;
    hipEvent_t done = nullptr;
    bool pending = false;
};

struct TableRing {
    int device = -1;
    TableSlot slots[kTableSlots];
    int next = 0;

    ~TableRing() { release(); }
    void release()
    {
        if (device < 0)
            return;
        for (auto& s : slots) {
            if (s.host) (void)hipHostFree(s.host);
            if (s.dev) (void)hipFree(s.dev);
            if (s.done) (void)hipEventDestroy(s.done);
            s = TableSlot{};
        }
        device = -1;
        next = 0;
    }
    hipError_t acquire(size_t bytes, TableSlot** out)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess)
            return e;
        if (dev != device) {
            release();
            device = dev;
        }
        TableSlot& s = slots[next];
        next = (next + 1) % kTableSlots;
        if (s.pending) {
            e = hipEventSynchronize(s.done);
            if (e != hipSuccess)
                return e;
            s.pending = false;
        }
        if (s.done == nullptr) {
            e = hipEventCreateWithFlags(&s.done, hipEventDisableTiming);
            if (e != hipSuccess)
                return e;
        }
        if (s.cap < bytes) {
            if (s.host) (void)hipHostFree(s.host);
            if (s.dev) (void)hipFree(s.dev);
            s.host = s.dev = nullptr;
            s.cap = 0;
            const size_t want = bytes + bytes / 2 + 4096;
            e = hipHostMalloc(&s.host, want, hipHostMallocMapped);
            if (e == hipSuccess)
                e = hipHostGetDevicePointer(&s.host_mapped, s.host, 0);
            if (e == hipSuccess)
                e = hipMalloc(&s.dev, want);
            if (e != hipSuccess)
                return e;
            s.cap = want;
        }
        *out = &s;
        return hipSuccess;
    }
};

// the calling thread's ring (released by release_batch_thread_tables)
TableRing& thread_table_ring();

// Sends the first `bytes` (a multiple of 16) of the slot's host side to its device side on `stream`: a small kernel that reads the
// mapped pinned slot (launch_table_upload), no copy-engine hand-over in front of the kernels that read the tables
hipError_t upload_table(TableSlot* slot, size_t bytes, hipStream_t stream);

}  // namespace dxtlt_host
