// batch_tables.h -- what the batch calls that stage tables share (host only): the settings code of a launch, the coarse index of
// a granule launch, and StagedTables, the one owner of the ring's slot protocol (table_ring.h).  Users: batch_api.cpp,
// image_batch_api.cpp, granule_image_batch_api.h (the BC7 and BC6H batch image calls), pixel_batch_api.cpp (the pixel batch call and
// the winners of the batched pixel auto call), estimate_api.cpp (the entropy table launch's test hook).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "bcn_launch.h"
#include "host_common.h"
#include "table_ring.h"

namespace dxtlt_host {

inline size_t padded(size_t bytes, size_t to) { return (bytes + to - 1) & ~(to - 1); }

// The settings a tile kernel is instantiated with, in 4 bits: variant << 2 | split_alpha << 1 | split_colour.  The callers pass
// a format's EFFECTIVE settings (dxtlt::effective_settings), so that items which differ only in what their format ignores share a launch.
inline int settings_code(const dxtlt::Settings& s) { return (s.variant << 2) | ((s.split_alpha ? 1 : 0) << 1) | (s.split_colour ? 1 : 0); }
inline dxtlt::Settings settings_of_code(int code)
{
    dxtlt::Settings s{};
    s.variant = (code >> 2) & 3;
    s.split_alpha = ((code >> 1) & 1) != 0;
    s.split_colour = (code & 1) != 0;
    return s;
}

// The coarse index of a granule launch of `wgs` workgroups: out[k] = the entry that owns workgroup 64 k, for the `n` entries in
// ascending first_wg; coarse_index_count(wgs) elements.  A workgroup finds its owner by walking on from there.
inline size_t coarse_index_count(uint32_t wgs) { return ((size_t)wgs + 63) / 64; }
template <class ENTRY>
void build_coarse_index(const ENTRY* entries, size_t n, uint32_t wgs, uint32_t* out)
{
    size_t cur = 0;
    for (size_t k = 0; k < coarse_index_count(wgs); ++k) {
        while (cur + 1 < n && entries[cur + 1].first_wg <= (uint32_t)(k * 64))
            ++cur;
        out[k] = (uint32_t)cur;
    }
}

// The tables of ONE call in ONE slot of the calling thread's ring -- the rule table_ring.h explains: acquire once, fill host(),
// upload, launch the kernels that read dev(), then finish, whether or not a launch failed.
struct StagedTables {
    TableSlot* slot = nullptr;
    size_t bytes = 0;

    hipError_t acquire(size_t table_bytes)
    {
        bytes = table_bytes;
        return thread_table_ring().acquire(bytes, &slot);
    }
    uint8_t* host() const { return static_cast<uint8_t*>(slot->host); }
    const uint8_t* dev() const { return static_cast<const uint8_t*>(slot->dev); }
    hipError_t upload(hipStream_t stream) { return upload_table(slot, bytes, stream); }
    // Records the slot's event behind the upload and the kernels that read the device tables (also behind a failed launch: what
    // was enqueued still reads the slot) and reports the call's launch error first, the event's second
    int32_t finish(hipError_t launch_error, hipStream_t stream, const char* what_launch, const char* what_event)
    {
        const hipError_t ev = hipEventRecord(slot->done, stream);
        slot->pending = ev == hipSuccess;
        if (launch_error != hipSuccess)
            return fail(kDevice, what_launch, launch_error);
        if (ev != hipSuccess)
            return fail(kDevice, what_event, ev);
        return kOk;
    }
};

}  // namespace dxtlt_host
