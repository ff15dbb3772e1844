// pixel_batch_api.cpp -- dxtlt_transform_pixels_batch_device (include/dxtlt_pixels.h; docs/PIXEL_FORMAT.md, "Many buffers in one
// call"): many uncompressed-pixel buffers, both directions, ONE launch per (pixel_bytes, direction, decorrelate, layout) class.
//
// The shape of dxtlt_transform_batch_device (batch_api.cpp): the planner (pixel_batch_plan.h, pure host arithmetic) checks the
// whole batch, groups the items by class, lays every class's tiles end to end and writes entries and workgroup indices of all
// launches into ONE buffer; the call stages that buffer in one slot of the calling thread's table ring (StagedTables), uploads
// it on the caller's stream and launches pixel_batch_tiles (pixel_batch_kernels.hip) once per class.  Asynchronous.
#include <hip/hip_runtime_api.h>

#include <cstring>

#include "../../include/dxtlt_pixels.h"
#include "batch_tables.h"
#include "host_common.h"
#include "pixel_batch_api.h"
#include "pixel_batch_plan.h"

namespace {

using namespace dxtlt_host;
namespace pb = dxtlt_host::pixel_batch;

}  // namespace

int32_t dxtlt_host::pixel_batch_enqueue(const pixel_batch::Plan& plan, hipStream_t stream)
{
    if (plan.tables.empty())
        return kOk;
    StagedTables tables;
    hipError_t e = tables.acquire(plan.tables.size());
    if (e != hipSuccess)
        return fail(kDevice, "pixel batch table staging", e);
    std::memcpy(tables.host(), plan.tables.data(), plan.tables.size());
    e = tables.upload(stream);
    for (size_t k = 0; k < plan.launches.size() && e == hipSuccess; ++k) {
        const pb::ClassLaunch& l = plan.launches[k];
        const uint8_t* d = tables.dev() + l.at;
        e = dxtlt::pixels::launch_pixel_batch(l.pixel_bytes(), l.inverse(), l.decorrelate(), l.layout(),
                                              reinterpret_cast<const dxtlt::pixels::PixelBatchEntry*>(d), d + l.entry_bytes,
                                              (uint32_t)l.entries.size(), l.wgs, l.wide, stream);
    }
    return tables.finish(e, stream, "pixel batch table copy / launch", "pixel batch event");
}

extern "C" int32_t dxtlt_transform_pixels_batch_device(const DxtltPixelBatchItem* items, size_t count, void* hip_stream)
{
    pb::Plan plan;
    if (Defect d = pb::plan_call(items, count, plan); d.code != kOk)
        return fail(d.code, d.what);
    if (plan.launches.empty())
        return kOk;   // no item, or empty items only: nothing to enqueue, no device needed
    int devices = 0;
    hipError_t e = hipGetDeviceCount(&devices);
    if (e != hipSuccess || devices <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument, "the pixel batch call stages its tables in a per-thread ring that later calls rewrite: not capturable");
    return pixel_batch_enqueue(plan, st);
}

extern "C" int32_t dxtlt_debug_plan_pixels_batch(const DxtltPixelBatchItem* items, size_t count, DxtltDebugPixelBatchLaunch* launches_out,
                                                 size_t cap, uint64_t* table_bytes_out)
{
    if (table_bytes_out)
        *table_bytes_out = 0;
    pb::Plan plan;
    if (Defect d = pb::plan_call(items, count, plan); d.code != kOk) {
        (void)fail(d.code, d.what);
        return -1;
    }
    if (table_bytes_out)
        *table_bytes_out = plan.tables.size();
    size_t n = 0;
    for (const pb::ClassLaunch& l : plan.launches) {
        if (launches_out != nullptr && n < cap) {
            DxtltDebugPixelBatchLaunch r{};
            r.pixel_bytes = (uint8_t)l.pixel_bytes(), r.inverse = l.inverse() ? 1 : 0, r.decorrelate = l.decorrelate() ? 1 : 0;
            r.layout = (uint8_t)l.layout();
            r.items = (uint32_t)l.entries.size(), r.workgroups = l.wgs, r.wide = l.wide ? 1 : 0;
            r.table_offset = l.at, r.table_bytes = l.entry_bytes + dxtlt::batch_index_bytes(l.wgs);
            launches_out[n] = r;
        }
        ++n;
    }
    return (int32_t)n;
}
