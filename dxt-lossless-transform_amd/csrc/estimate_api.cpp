// estimate_api.cpp -- C ABI of the built-in size estimator (include/dxtlt_estimator.h) over estimate_kernels.hip, and the
// per-thread counter block the auto transforms read their estimates back through (auto_transform.cpp).  The entropy estimator
// (include/dxtlt_entropy_estimator.h, entropy_kernels.hip) has the same four entry points over the same counters, upload buffer
// and stream.
#include "../../include/dxtlt_entropy_estimator.h"
#include "../../include/dxtlt_estimator.h"

#include <cstring>
#include <vector>

#include "batch_tables.h"
#include "entropy_launch.h"
#include "estimate_launch.h"
#include "host_common.h"

namespace {

// this thread's counters on the current device and their pinned host copy (grow-never: kMaxCounters of 8 bytes each)
struct Counters {
    uint64_t* d = nullptr;
    uint64_t* h = nullptr;
    int device = -1;
    ~Counters() { release(); }
    void release()
    {
        if (d) (void)hipFree(d);
        if (h) (void)hipHostFree(h);
        d = h = nullptr;
        device = -1;
    }
    bool get()
    {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess)
            return false;
        if (dev != device || d == nullptr) {
            release();
            if (hipMalloc(reinterpret_cast<void**>(&d), dxtlt_host::kMaxCounters * sizeof(uint64_t)) != hipSuccess ||
                hipHostMalloc(reinterpret_cast<void**>(&h), dxtlt_host::kMaxCounters * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
                (void)hipGetLastError();
                release();
                return false;
            }
            device = dev;
        }
        return true;
    }
};
thread_local Counters g_counters;

// dxtlt_estimate_size's own upload buffer and stream (grow-only, per thread and device).  NOT the staging of the host-pointer
// transforms: this call is what an estimator callback makes from INSIDE an auto transform of the same thread, which keeps its
// uploaded input in that staging for the whole call.
struct UploadStage {
    void* ptr = nullptr;
    size_t cap = 0;
    hipStream_t stream = nullptr;
    int device = -1;
    ~UploadStage() { release(); }
    void release()
    {
        if (ptr) (void)hipFree(ptr);
        if (stream) (void)hipStreamDestroy(stream);
        ptr = nullptr;
        stream = nullptr;
        cap = 0;
        device = -1;
    }
    hipError_t get(size_t bytes)
    {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess)
            return e;
        if (dev != device)
            release();
        if (stream == nullptr) {
            if ((e = hipStreamCreateWithFlags(&stream, hipStreamNonBlocking)) != hipSuccess) {
                stream = nullptr;
                return e;
            }
            device = dev;
        }
        if (bytes > cap) {
            if (ptr) (void)hipFree(ptr);
            ptr = nullptr;
            cap = 0;
            if ((e = hipMalloc(&ptr, bytes)) != hipSuccess) {
                ptr = nullptr;
                return e;
            }
            cap = bytes;
        }
        return hipSuccess;
    }
};
thread_local UploadStage g_upload;

int32_t need_device()
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return dxtlt_host::fail(dxtlt_host::kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    return dxtlt_host::kOk;
}

uint32_t builtin_max_compressed_size(void*, size_t, size_t* out_size)
{
    if (out_size)
        *out_size = 0;
    return 0;
}

uint32_t builtin_estimate_compressed_size(void*, const uint8_t* input_ptr, size_t len_bytes, uint8_t*, size_t, size_t* out_size)
{
    uint64_t v = 0;
    const int32_t rc = dxtlt_estimate_size(input_ptr, len_bytes, &v);
    if (rc == DXTLT_OK && out_size)
        *out_size = static_cast<size_t>(v);
    return static_cast<uint32_t>(rc);
}

const DltSizeEstimator kBuiltin = {nullptr, builtin_max_compressed_size, builtin_estimate_compressed_size};

uint32_t entropy_estimate_compressed_size(void*, const uint8_t* input_ptr, size_t len_bytes, uint8_t*, size_t, size_t* out_size)
{
    uint64_t v = 0;
    const int32_t rc = dxtlt_estimate_entropy_size(input_ptr, len_bytes, &v);
    if (rc == DXTLT_OK && out_size)
        *out_size = static_cast<size_t>(v);
    return static_cast<uint32_t>(rc);
}

const DltSizeEstimator kBuiltinEntropy = {nullptr, builtin_max_compressed_size, entropy_estimate_compressed_size};

}  // namespace

void dxtlt_host::release_estimate_thread_counters()
{
    g_counters.release();
    g_upload.release();
}

bool dxtlt_host::is_builtin_estimator(const DltSizeEstimator* est)
{
    return est != nullptr && est->MaxCompressedSize == builtin_max_compressed_size &&
           est->EstimateCompressedSize == builtin_estimate_compressed_size;
}

bool dxtlt_host::is_builtin_entropy_estimator(const DltSizeEstimator* est) { return est == &kBuiltinEntropy; }

int32_t dxtlt_host::estimate_enqueue(const dxtlt::EstimateSection* sections, size_t count, hipStream_t st, size_t first_counter)
{
    if (first_counter + count > kMaxCounters)
        return fail(kInvalidArgument, "more estimates than this thread's counter block holds");
    if (!g_counters.get())
        return fail(kDevice, "estimator counters: allocation failed", hipErrorOutOfMemory);
    hipError_t e = dxtlt::launch_estimate(sections, count, g_counters.d + first_counter, st);
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, "a section of more than 2^31 - 1 windows");
    HIP_TRY(e, "estimator launch");
    return kOk;
}

int32_t dxtlt_host::entropy_enqueue(const dxtlt::EstimateSection* sections, size_t count, hipStream_t st, size_t first_counter)
{
    if (first_counter + count > kMaxCounters)
        return fail(kInvalidArgument, "more estimates than this thread's counter block holds");
    if (!g_counters.get())
        return fail(kDevice, "estimator counters: allocation failed", hipErrorOutOfMemory);
    hipError_t e = dxtlt::launch_entropy(sections, count, g_counters.d + first_counter, st);
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, "a section of more than 2^31 - 1 windows");
    HIP_TRY(e, "entropy estimator launch");
    return kOk;
}

int32_t dxtlt_host::estimate_read_back(size_t count, hipStream_t st, uint64_t* out)
{
    if (count > kMaxCounters || !g_counters.get())
        return fail(kInvalidArgument, "estimator counters: nothing to read");
    HIP_TRY(hipMemcpyAsync(g_counters.h, g_counters.d, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st), "D2H estimates");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    for (size_t i = 0; i < count; ++i)
        out[i] = g_counters.h[i];
    return kOk;
}

bool dxtlt_host::stream_is_capturing(hipStream_t st)
{
    hipStreamCaptureStatus status = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(st, &status) != hipSuccess) {
        // e.g. the legacy default stream while another stream captures in global mode: not provably outside a capture
        (void)hipGetLastError();
        return true;
    }
    return status != hipStreamCaptureStatusNone;
}

extern "C" {

uint32_t dxtlt_estimator_version(void) { return dxtlt::kEstimatorVersion; }

const DltSizeEstimator* dxtlt_builtin_size_estimator(void) { return &kBuiltin; }

int32_t dxtlt_debug_estimate_sizes_shape(const DxtltEstimateSection* sections, size_t count, void* hip_stream, uint64_t* d_out,
                                         int32_t lanes, uint32_t window, uint32_t bits)
{
    using namespace dxtlt_host;
    if (count == 0)
        return kOk;
    if (sections == nullptr || d_out == nullptr || reinterpret_cast<uintptr_t>(d_out) % 8 != 0)
        return fail(kInvalidArgument, "NULL sections / d_out with count > 0, or d_out not 8-byte aligned");
    if (int32_t rc = need_device())
        return rc;
    hipError_t e = dxtlt::launch_estimate_shape(reinterpret_cast<const dxtlt::EstimateSection*>(sections), count, d_out,
                                                static_cast<hipStream_t>(hip_stream), lanes, window, bits);
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, "lanes / window / bits not compiled in, or a section of more than 2^31 - 1 windows");
    HIP_TRY(e, "estimator launch");
    return kOk;
}

int32_t dxtlt_estimate_sizes_device(const DxtltEstimateSection* sections, size_t count, void* hip_stream, uint64_t* d_out)
{
    using namespace dxtlt_host;
    if (count == 0)
        return kOk;
    if (sections == nullptr || d_out == nullptr)
        return fail(kInvalidArgument, "NULL sections / d_out with count > 0");
    if (reinterpret_cast<uintptr_t>(d_out) % 8 != 0)
        return fail(kInvalidArgument, "d_out is not 8-byte aligned");
    if (int32_t rc = need_device())
        return rc;
    static_assert(sizeof(DxtltEstimateSection) == sizeof(dxtlt::EstimateSection), "one layout");
    hipError_t e = dxtlt::launch_estimate(reinterpret_cast<const dxtlt::EstimateSection*>(sections), count, d_out,
                                          static_cast<hipStream_t>(hip_stream));
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, "a section of more than 2^31 - 1 windows");
    HIP_TRY(e, "estimator launch");
    return kOk;
}

int32_t dxtlt_estimate_size_device(const void* d_ptr, size_t len, void* hip_stream, uint64_t* out)
{
    using namespace dxtlt_host;
    if (out == nullptr)
        return fail(kInvalidArgument, "NULL out");
    if (d_ptr == nullptr || len < 4) {   // no gram (docs/ESTIMATOR.md): nothing to ask a device
        *out = len;
        return kOk;
    }
    if (int32_t rc = need_device())
        return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument, "dxtlt_estimate_size_device waits for its stream: not capturable (dxtlt_estimate_sizes_device is)");
    const dxtlt::EstimateSection s{d_ptr, len};
    if (int32_t rc = estimate_enqueue(&s, 1, st, 0))
        return rc;
    return estimate_read_back(1, st, out);
}

int32_t dxtlt_estimate_size(const uint8_t* host_ptr, size_t len, uint64_t* out)
{
    using namespace dxtlt_host;
    if (out == nullptr)
        return fail(kInvalidArgument, "NULL out");
    if (host_ptr == nullptr || len < 4) {
        *out = len;
        return kOk;
    }
    if (int32_t rc = need_device())
        return rc;
    HIP_TRY(g_upload.get(len), "estimator upload buffer / stream");
    hipStream_t st = g_upload.stream;
    hipError_t e = hipMemcpyAsync(g_upload.ptr, host_ptr, len, hipMemcpyHostToDevice, st);
    int32_t rc = kOk;
    if (e != hipSuccess) {
        rc = fail(kDevice, "H2D copy", e);
    } else {
        const dxtlt::EstimateSection s{g_upload.ptr, len};
        rc = estimate_enqueue(&s, 1, st, 0);
        if (rc == kOk)
            rc = estimate_read_back(1, st, out);
    }
    if (rc != kOk)
        (void)hipStreamSynchronize(st);   // the upload buffer belongs to this thread's next call
    return rc;
}

// ---- include/dxtlt_entropy_estimator.h ----------------------------------------------------------------------------------------
uint32_t dxtlt_entropy_estimator_version(void) { return dxtlt::kEntropyEstimatorVersion; }

const DltSizeEstimator* dxtlt_builtin_entropy_estimator(void) { return &kBuiltinEntropy; }

uint32_t dxtlt_debug_entropy_table(uint32_t k) { return dxtlt::entropy_table_host(k); }

int32_t dxtlt_estimate_entropy_sizes_device(const DxtltEstimateSection* sections, size_t count, void* hip_stream, uint64_t* d_out)
{
    using namespace dxtlt_host;
    if (count == 0)
        return kOk;
    if (sections == nullptr || d_out == nullptr)
        return fail(kInvalidArgument, "NULL sections / d_out with count > 0");
    if (reinterpret_cast<uintptr_t>(d_out) % 8 != 0)
        return fail(kInvalidArgument, "d_out is not 8-byte aligned");
    if (int32_t rc = need_device())
        return rc;
    hipError_t e = dxtlt::launch_entropy(reinterpret_cast<const dxtlt::EstimateSection*>(sections), count, d_out,
                                         static_cast<hipStream_t>(hip_stream));
    if (e == hipErrorInvalidValue)
        return fail(kInvalidArgument, "a section of more than 2^31 - 1 windows");
    HIP_TRY(e, "entropy estimator launch");
    return kOk;
}

// the entropy estimates of `count` sections through launch_entropy_table: the table built here, staged in one slot of this
// thread's table ring and uploaded on the stream, ONE estimator launch whatever `count` is, one finishing launch
int32_t dxtlt_debug_estimate_entropy_table_counters_device(const DxtltEstimateSection* sections, const uint32_t* counters, size_t count,
                                                           size_t counter_count, void* hip_stream, uint64_t* d_out)
{
    using namespace dxtlt_host;
    if (count == 0 || counter_count == 0)
        return kOk;
    if (sections == nullptr || d_out == nullptr || reinterpret_cast<uintptr_t>(d_out) % 8 != 0)
        return fail(kInvalidArgument, "NULL sections / d_out with count > 0, or d_out not 8-byte aligned");
    if (counter_count > 0x7FFFFFFFu)
        return fail(kInvalidArgument, "more than 2^31 - 1 counters");
    std::vector<dxtlt::EstimateTableEntry> table;
    uint64_t wgs = 0;
    for (size_t i = 0; i < count; ++i) {
        const size_t counter = counters ? counters[i] : i;
        if (counter >= counter_count)
            return fail(kInvalidArgument, "a section's counter is out of range");
        if (sections[i].d_ptr == nullptr || sections[i].len == 0)
            continue;   // nothing to count: owns no workgroup, its counter stays as the others leave it
        wgs += (sections[i].len + dxtlt::kEntropyWindow - 1) / dxtlt::kEntropyWindow;
        if (wgs > 0x7FFFFFFFull)
            return fail(kInvalidArgument, "more than 2^31 - 1 windows in one launch");
        table.push_back({static_cast<const uint8_t*>(sections[i].d_ptr), sections[i].len, (uint32_t)wgs, (uint32_t)counter});
    }
    if (int32_t rc = need_device())
        return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument, "the table launch hook stages its table in a per-thread ring that later calls rewrite: not capturable");
    HIP_TRY(hipMemsetAsync(d_out, 0, counter_count * sizeof(uint64_t), st), "entropy counters clear");
    if (table.empty())
        return kOk;
    StagedTables staged;
    const size_t bytes = padded(table.size() * sizeof(dxtlt::EstimateTableEntry), 16);
    hipError_t e = staged.acquire(bytes);
    if (e != hipSuccess)
        return fail(kDevice, "entropy table staging", e);
    std::memset(staged.host(), 0, bytes);
    std::memcpy(staged.host(), table.data(), table.size() * sizeof(dxtlt::EstimateTableEntry));
    e = staged.upload(st);
    if (e == hipSuccess)
        e = dxtlt::launch_entropy_table(reinterpret_cast<const dxtlt::EstimateTableEntry*>(staged.dev()), (uint32_t)table.size(),
                                        (uint32_t)wgs, d_out, st);
    if (e == hipSuccess)
        e = dxtlt::launch_entropy_finish(d_out, counter_count, st);
    return staged.finish(e, st, "entropy table copy / launch", "entropy table event");
}

int32_t dxtlt_debug_estimate_entropy_table_device(const DxtltEstimateSection* sections, size_t count, void* hip_stream, uint64_t* d_out)
{
    return dxtlt_debug_estimate_entropy_table_counters_device(sections, nullptr, count, count, hip_stream, d_out);
}

int32_t dxtlt_estimate_entropy_size_device(const void* d_ptr, size_t len, void* hip_stream, uint64_t* out)
{
    using namespace dxtlt_host;
    if (out == nullptr)
        return fail(kInvalidArgument, "NULL out");
    if (d_ptr == nullptr || len == 0) {   // nothing to count (docs/ESTIMATOR.md): nothing to ask a device
        *out = 0;
        return kOk;
    }
    if (int32_t rc = need_device())
        return rc;
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (stream_is_capturing(st))
        return fail(kInvalidArgument,
                    "dxtlt_estimate_entropy_size_device waits for its stream: not capturable (dxtlt_estimate_entropy_sizes_device is)");
    const dxtlt::EstimateSection s{d_ptr, len};
    if (int32_t rc = entropy_enqueue(&s, 1, st, 0))
        return rc;
    return estimate_read_back(1, st, out);
}

int32_t dxtlt_estimate_entropy_size(const uint8_t* host_ptr, size_t len, uint64_t* out)
{
    using namespace dxtlt_host;
    if (out == nullptr)
        return fail(kInvalidArgument, "NULL out");
    if (host_ptr == nullptr || len == 0) {
        *out = 0;
        return kOk;
    }
    if (int32_t rc = need_device())
        return rc;
    HIP_TRY(g_upload.get(len), "estimator upload buffer / stream");
    hipStream_t st = g_upload.stream;
    hipError_t e = hipMemcpyAsync(g_upload.ptr, host_ptr, len, hipMemcpyHostToDevice, st);
    int32_t rc = kOk;
    if (e != hipSuccess) {
        rc = fail(kDevice, "H2D copy", e);
    } else {
        const dxtlt::EstimateSection s{g_upload.ptr, len};
        rc = entropy_enqueue(&s, 1, st, 0);
        if (rc == kOk)
            rc = estimate_read_back(1, st, out);
    }
    if (rc != kOk)
        (void)hipStreamSynchronize(st);   // the upload buffer belongs to this thread's next call
    return rc;
}

}  // extern "C"
