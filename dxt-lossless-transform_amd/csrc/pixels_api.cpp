// pixels_api.cpp -- C ABI of the uncompressed-pixel transform, layout version 1 (include/dxtlt_pixels.h,
// docs/PIXEL_FORMAT.md): argument checks, and the stream layout and launch these buffers hand to the common host paths
// (host_staging.cpp, host_sharded.cpp).  Plane c of a buffer of P pixels is a stream at c * P of one byte per pixel, so
// the chunked pipeline, the sharded path and buffers of 4 GiB and more need nothing of their own; a shard or chunk starts
// on a multiple of the 4096-pixel segment, so a PLANAR_DELTA range transformed as a stand-alone buffer yields its slice
// of every plane byte for byte.  The kernels are pixel_kernels.hip.
#include "../../include/dxtlt_pixels.h"

#include <hip/hip_runtime_api.h>

#include <atomic>

#include "host_common.h"
#include "pixel_launch.h"

namespace {

using namespace dxtlt_host;
constexpr uint64_t kT = dxtlt::pixels::kTile;

int32_t check_settings(int32_t pixel_bytes, uint8_t layout)
{
    if (pixel_bytes != 3 && pixel_bytes != 4)
        return fail(kInvalidArgument, "pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)");
    if (layout > 2)
        return fail(kInvalidArgument, "layout must be 0 (INTERLEAVED), 1 (PLANAR) or 2 (PLANAR_DELTA)");
    return kOk;
}

// `len` bytes of host or device memory as pixels: the checks every whole-buffer call starts with, in this order
int32_t check_buffers(int32_t pixel_bytes, uint8_t layout, const void* in, const void* out, size_t len)
{
    if (int32_t rc = check_settings(pixel_bytes, layout); rc != kOk)
        return rc;
    if (len % (size_t)pixel_bytes != 0)
        return fail(kInvalidLength, "len is not a multiple of pixel_bytes");
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    return kOk;
}

// A launch needs a device: said once, in the library's words, in front of the first launch of the process (the host paths
// say it when they look for their staging context)
int32_t require_device()
{
    static std::atomic<bool> seen{false};
    if (seen.load(std::memory_order_relaxed))
        return kOk;
    int count = 0;
    const hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    seen.store(true, std::memory_order_relaxed);
    return kOk;
}

Launch launch_of(int pixel_bytes, bool decorrelate, uint8_t layout)
{
    return [=](bool inverse, const void* src, void* dst, uint64_t total, uint64_t first, uint64_t count, hipStream_t stream) {
        return pixel_device_range(pixel_bytes, inverse, src, dst, total, first, count, decorrelate, layout, stream);
    };
}

}  // namespace

// INTERLEAVED: one stream, the pixels themselves.  PLANAR / PLANAR_DELTA: a stream of one byte per pixel per plane.  Shards
// and pipeline chunks start on a segment; a shard per segment at most.
dxtlt_host::StreamLayout dxtlt_host::pixel_layout(int pixel_bytes, uint8_t layout)
{
    StreamLayout L{pixel_bytes == 4 ? 8 : 9, 1, {}, {}, (uint64_t)pixel_bytes, kT, kT};
    if (layout == dxtlt::pixels::kInterleaved) {
        L.off[0] = 0;
        L.width[0] = (uint64_t)pixel_bytes;
        return L;
    }
    L.n = pixel_bytes;
    for (int c = 0; c < pixel_bytes; ++c) {
        L.off[c] = (uint64_t)c;
        L.width[c] = 1;
    }
    return L;
}

int32_t dxtlt_host::pixel_device_range(int pixel_bytes, bool inverse, const void* d_src, void* d_dst, uint64_t total, uint64_t first,
                                       uint64_t num, bool decorrelate, uint8_t layout, void* stream)
{
    if (int32_t rc = check_settings(pixel_bytes, layout); rc != kOk)
        return rc;
    if (first > total || num > total - first)
        return fail(kInvalidArgument, "pixel range exceeds total_pixels");
    if (first % kT != 0)
        return fail(kInvalidArgument, "first_pixel must be a multiple of 4096 (DXTLT_PIXEL_SEGMENT)");
    if (num == 0)
        return kOk;
    if (d_src == nullptr || d_dst == nullptr)
        return fail(kInvalidArgument, "NULL device buffer with a non-empty range");
    if ((num + kT - 1) / kT > 0x7FFFFFFFull)
        return fail(kInvalidArgument, "pixel range of 2^43 pixels or more: split it into ranges");
    if (int32_t rc = require_device(); rc != kOk)
        return rc;
    HIP_TRY(dxtlt::pixels::launch_range(pixel_bytes, inverse, decorrelate, layout, d_src, d_dst, total, first, num, (hipStream_t)stream),
            "pixel kernel launch");
    return kOk;
}

int32_t dxtlt_host::pixel_host_call(int pixel_bytes, bool inverse, const uint8_t* in, uint8_t* out, size_t len, bool decorrelate,
                                    uint8_t layout)
{
    if (int32_t rc = check_buffers(pixel_bytes, layout, in, out, len); rc != kOk || len == 0)
        return rc;   // zero pixels: nothing to do, no device needed
    return host_round_trip(pixel_layout(pixel_bytes, layout), launch_of(pixel_bytes, decorrelate, layout), inverse, in, out,
                           len / (size_t)pixel_bytes);
}

int32_t dxtlt_host::pixel_sharded(int pixel_bytes, bool inverse, const uint8_t* in, uint8_t* out, size_t len, bool decorrelate,
                                  uint8_t layout, int32_t num_shards, std::vector<DxtltShardStat>* stats)
{
    if (int32_t rc = check_buffers(pixel_bytes, layout, in, out, len); rc != kOk || len == 0)
        return rc;
    return run_sharded(pixel_layout(pixel_bytes, layout), launch_of(pixel_bytes, decorrelate, layout), inverse, in, out,
                       len / (size_t)pixel_bytes, 0, num_shards, stats);
}

extern "C" {

int32_t dxtlt_transform_pixels(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t pixel_bytes, bool decorrelate,
                               uint8_t layout)
{
    return dxtlt_host::pixel_host_call(pixel_bytes, false, input_ptr, output_ptr, len, decorrelate, layout);
}
int32_t dxtlt_untransform_pixels(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t pixel_bytes, bool decorrelate,
                                 uint8_t layout)
{
    return dxtlt_host::pixel_host_call(pixel_bytes, true, input_ptr, output_ptr, len, decorrelate, layout);
}

static int32_t device_whole(bool inverse, const void* d_in, void* d_out, size_t len, int32_t pixel_bytes, bool decorrelate,
                            uint8_t layout, void* stream)
{
    if (int32_t rc = check_buffers(pixel_bytes, layout, d_in, d_out, len); rc != kOk)
        return rc;
    const uint64_t pixels = len / (size_t)pixel_bytes;
    return dxtlt_host::pixel_device_range(pixel_bytes, inverse, d_in, d_out, pixels, 0, pixels, decorrelate, layout, stream);
}
int32_t dxtlt_transform_pixels_device(const void* d_input, void* d_output, size_t len, int32_t pixel_bytes, bool decorrelate,
                                      uint8_t layout, void* hip_stream)
{
    return device_whole(false, d_input, d_output, len, pixel_bytes, decorrelate, layout, hip_stream);
}
int32_t dxtlt_untransform_pixels_device(const void* d_input, void* d_output, size_t len, int32_t pixel_bytes, bool decorrelate,
                                        uint8_t layout, void* hip_stream)
{
    return device_whole(true, d_input, d_output, len, pixel_bytes, decorrelate, layout, hip_stream);
}
int32_t dxtlt_transform_pixels_range_device(int32_t pixel_bytes, bool inverse, const void* d_src, void* d_dst, uint64_t total_pixels,
                                            uint64_t first_pixel, uint64_t num_pixels, bool decorrelate, uint8_t layout,
                                            void* hip_stream)
{
    return dxtlt_host::pixel_device_range(pixel_bytes, inverse, d_src, d_dst, total_pixels, first_pixel, num_pixels, decorrelate,
                                          layout, hip_stream);
}

}  // extern "C"
