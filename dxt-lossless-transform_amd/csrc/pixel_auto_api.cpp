// pixel_auto_api.cpp -- the pixel auto transform (include/dxtlt_pixels.h, docs/PIXEL_FORMAT.md "The auto transform"): the six
// settings of the uncompressed-pixel transform tried in one fixed order, each candidate's WHOLE output shown to the estimator
// as one section, the first smallest kept (strict `<`).
//
// With the entropy estimator (include/dxtlt_entropy_estimator.h; the device call always, the host call when it is handed
// dxtlt_builtin_entropy_estimator()) nothing but six counters leaves the device:
//   arena route     one fused candidate kernel (pixel_auto_kernels.hip) reads the input once and writes the five candidates that
//                   are not the input itself side by side into this thread's candidate arena (5 x len, the arena of
//                   auto_transform.cpp), ONE entropy launch estimates the six sections where they lie;
//   fallback route  no arena, dxtlt_debug_auto_use_arena(0), or a d_input off a 16-byte boundary: one full transform per
//                   candidate into d_output, estimated there in stream order (the BC4 / BC5 no-arena shape).
// Either way one wait, for the counters, and then the winner's transform from d_input into d_output, enqueued and not waited
// for.  The same totals, choice and bytes on both routes.  With any other estimator the candidates are downloaded one after
// the other and the callbacks made in candidate order, as auto_transform.cpp does it.
#include <hip/hip_runtime_api.h>

#include "../../include/dxtlt_entropy_estimator.h"
#include "../../include/dxtlt_pixels.h"
#include "auto_call.h"
#include "pixel_launch.h"

namespace {

using namespace dxtlt_host;

constexpr int kCandidates = dxtlt::pixels::kAutoCandidates;   // in the order of kAutoOrder (pixel_launch.h)
constexpr auto& kOrder = dxtlt::pixels::kAutoOrder;
constexpr int kIdentity = 5;   // (false, INTERLEAVED): the input itself, never written for an estimate

thread_local uint64_t t_totals[kCandidates];
thread_local int t_total_count = 0;   // dxtlt_debug_pixels_auto_last_totals
thread_local bool t_time_phases = false;
thread_local double t_phase_ms[3] = {0, 0, 0};

int32_t check_arguments(int32_t pixel_bytes, size_t len)
{
    if (pixel_bytes != 3 && pixel_bytes != 4)
        return fail(kInvalidArgument, "pixel_bytes must be 4 (RGBA8888, BGRA8888) or 3 (BGR888)");
    if (len % (size_t)pixel_bytes != 0)
        return fail(kInvalidLength, "len is not a multiple of pixel_bytes");
    return kOk;
}

int32_t transform_candidate(int B, int i, const void* d_in, void* d_out, uint64_t pixels, hipStream_t st)
{
    return pixel_device_range(B, false, d_in, d_out, pixels, 0, pixels, kOrder[i].decorrelate, kOrder[i].layout, st);
}

// the bench hook's four events around the phases of one call (nothing without the switch)
struct PhaseEvents {
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool on = false;
    ~PhaseEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    bool begin(bool wanted)
    {
        on = wanted;
        for (int k = 0; k < 4 && on; ++k)
            on = hipEventCreate(&ev[k]) == hipSuccess;
        return on;
    }
    void mark(int k, hipStream_t st)
    {
        if (on) (void)hipEventRecord(ev[k], st);
    }
    void finish(hipStream_t st)
    {
        if (!on || hipStreamSynchronize(st) != hipSuccess)
            return;
        for (int k = 0; k < 3; ++k) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[k], ev[k + 1]) == hipSuccess)
                t_phase_ms[k] = ms;
        }
    }
};

// Chooses among the six candidates for the `len` > 0 bytes at d_in with the entropy estimator and leaves the winner's transform
// enqueued from d_in into d_out.  Waits for `st` once, for the counters: when it returns nothing in flight touches this thread's
// arena or counters (the pending transform reads d_in alone).
int32_t auto_on_device(int B, const void* d_in, void* d_out, size_t len, hipStream_t st, int* pick)
{
    const uint64_t pixels = len / (size_t)B;
    uint8_t* arena = nullptr;
    if (!auto_state().no_arena && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0 && len <= SIZE_MAX / 5)
        arena = static_cast<uint8_t*>(auto_state().arena.get(5 * len));
    t_phase_ms[0] = t_phase_ms[1] = t_phase_ms[2] = 0;
    PhaseEvents phases;
    phases.begin(t_time_phases);
    phases.mark(0, st);
    int last = -1;   // the candidate whose transform is in d_out
    if (arena != nullptr) {
        HIP_TRY(dxtlt::pixels::launch_auto_candidates(B, d_in, arena, pixels, st), "pixel candidate kernel launch");
        phases.mark(1, st);
        dxtlt::EstimateSection secs[kCandidates];
        for (int i = 0; i < kCandidates; ++i)
            secs[i] = {i == kIdentity ? d_in : arena + (size_t)i * len, len};
        if (int32_t rc = entropy_enqueue(secs, kCandidates, st, 0))
            return rc;
    } else {
        for (int i = 0; i < kCandidates; ++i) {
            if (i != kIdentity) {
                if (int32_t rc = transform_candidate(B, i, d_in, d_out, pixels, st))
                    return rc;
                last = i;
            }
            const dxtlt::EstimateSection sec{i == kIdentity ? d_in : d_out, len};
            if (int32_t rc = entropy_enqueue(&sec, 1, st, (size_t)i))
                return rc;
        }
        phases.mark(1, st);   // (candidates and estimates alternate on this route: all of it is phase 0)
    }
    phases.mark(2, st);
    uint64_t totals[kCandidates];
    if (int32_t rc = estimate_read_back(kCandidates, st, totals))
        return rc;
    *pick = dxtlt::pixels::auto_pick_of(totals);
    if (*pick != last)
        if (int32_t rc = transform_candidate(B, *pick, d_in, d_out, pixels, st))
            return rc;
    phases.mark(3, st);
    phases.finish(st);
    for (int i = 0; i < kCandidates; ++i)
        t_totals[i] = totals[i];
    t_total_count = kCandidates;
    return kOk;
}

// any estimator but the entropy one: MaxCompressedSize once for `len`, then per candidate in order one full transform, its
// download into `out` and EstimateCompressedSize on it (the last candidate is `in` itself); the winner is transformed and
// downloaded again unless it was the last one written
int32_t auto_with_callbacks(int B, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* est, int* pick)
{
    const uint64_t pixels = len / (size_t)B;
    AutoThreadState& state = auto_state();
    size_t max_comp = 0;
    ++state.estimator_callbacks;
    if (est->MaxCompressedSize(est->Context, len, &max_comp) != 0)
        return fail(kEstimator, "size estimator: max_compressed_size failed");
    EstimatorScratch scratch;
    if (!scratch.allocate(max_comp))
        return fail(kAllocation, "estimator scratch allocation failed");
    void *d_in = nullptr, *d_out = nullptr;
    StreamDrain drain;
    if (int32_t rc = acquire_staging(len, &d_in, &d_out, &drain.stream))
        return rc;
    hipStream_t st = drain.stream;
    drain.armed = true;
    HIP_TRY(hipMemcpyAsync(d_in, in, len, hipMemcpyHostToDevice, st), "H2D copy");
    int best = 0, last = -1;
    size_t best_size = SIZE_MAX;
    for (int i = 0; i < kCandidates; ++i) {
        const uint8_t* seen = in;
        if (i != kIdentity) {
            if (int32_t rc = transform_candidate(B, i, d_in, d_out, pixels, st))
                return rc;
            last = i;
            state.section_bytes_downloaded += len;
            HIP_TRY(hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, st), "D2H candidate");
            HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
            seen = out;
        }
        size_t size = 0;
        ++state.estimator_callbacks;
        if (est->EstimateCompressedSize(est->Context, seen, len, scratch.ptr, max_comp, &size) != 0)
            return fail(kEstimator, "size estimator: estimate_compressed_size failed");
        if (size < best_size) {
            best_size = size;
            best = i;
        }
    }
    if (best != last) {
        if (int32_t rc = transform_candidate(B, best, d_in, d_out, pixels, st))
            return rc;
        HIP_TRY(hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, st), "D2H result");
        HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    }
    drain.armed = false;   // everything enqueued has been waited for
    *pick = best;
    return kOk;
}

int32_t report(int32_t rc, int pick, bool* out_decorrelate, uint8_t* out_layout)
{
    if (rc == kOk) {
        store_if(out_decorrelate, kOrder[pick].decorrelate);
        store_if(out_layout, kOrder[pick].layout);
    }
    return rc;
}

}  // namespace

extern "C" {

int32_t dxtlt_transform_pixels_auto_device(const void* d_input, void* d_output, size_t len, int32_t pixel_bytes, void* hip_stream,
                                           bool* out_decorrelate, uint8_t* out_layout)
{
    t_total_count = 0;
    if (int32_t rc = check_arguments(pixel_bytes, len))
        return rc;
    if (len > 0 && (d_input == nullptr || d_output == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    auto_state().begin_call();
    int pick = 0;   // every estimate of an empty buffer is 0: the first candidate stays
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (len > 0)
        if (int32_t rc = auto_device_call(st, [&] { return auto_on_device(pixel_bytes, d_input, d_output, len, st, &pick); }))
            return rc;
    return report(kOk, pick, out_decorrelate, out_layout);
}

int32_t dxtlt_transform_pixels_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, int32_t pixel_bytes,
                                    const DltSizeEstimator* estimator, bool* out_decorrelate, uint8_t* out_layout)
{
    t_total_count = 0;
    if (int32_t rc = check_arguments(pixel_bytes, len))
        return rc;
    if (estimator == nullptr || estimator->MaxCompressedSize == nullptr || estimator->EstimateCompressedSize == nullptr)
        return fail(kInvalidArgument, "NULL estimator");
    if (len > 0 && (input_ptr == nullptr || output_ptr == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    auto_state().begin_call();
    int pick = 0;
    if (len == 0)
        return report(kOk, pick, out_decorrelate, out_layout);
    if (!is_builtin_entropy_estimator(estimator))
        return report(auto_with_callbacks(pixel_bytes, input_ptr, output_ptr, len, estimator, &pick), pick, out_decorrelate, out_layout);

    // one upload, everything on the device, one download
    const int32_t rc = auto_staged_call(input_ptr, output_ptr, len, [&](const void* d_in, void* d_out, hipStream_t st) {
        return auto_on_device(pixel_bytes, d_in, d_out, len, st, &pick);
    });
    if (rc != kOk)
        t_total_count = 0;
    return report(rc, pick, out_decorrelate, out_layout);
}

int32_t dxtlt_debug_pixels_auto_last_totals(uint64_t* out, int32_t cap)
{
    for (int i = 0; out != nullptr && i < t_total_count && i < cap; ++i)
        out[i] = t_totals[i];
    return t_total_count;
}

void dxtlt_debug_pixels_auto_time_phases(int32_t on) { t_time_phases = on != 0; }

void dxtlt_debug_pixels_auto_last_phase_ms(double out[3])
{
    for (int k = 0; k < 3; ++k)
        out[k] = t_phase_ms[k];
}

int32_t dxtlt_debug_pixels_auto_candidates_device(const void* d_input, size_t len, int32_t pixel_bytes, void* hip_stream)
{
    if (int32_t rc = check_arguments(pixel_bytes, len))
        return rc;
    if (d_input == nullptr || len == 0 || (reinterpret_cast<uintptr_t>(d_input) & 15) != 0 || len > SIZE_MAX / 5)
        return fail(kInvalidArgument, "a non-empty buffer on a 16-byte boundary");
    void* arena = auto_state().arena.get(5 * len);
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    HIP_TRY(dxtlt::pixels::launch_auto_candidates(pixel_bytes, d_input, arena, len / (size_t)pixel_bytes,
                                                  static_cast<hipStream_t>(hip_stream)),
            "pixel candidate kernel launch");
    return kOk;
}

int32_t dxtlt_debug_pixels_auto_candidates_into_device(const void* d_input, size_t len, int32_t pixel_bytes, void* d_arena, void* hip_stream)
{
    if (int32_t rc = check_arguments(pixel_bytes, len))
        return rc;
    if (d_input == nullptr || len == 0 || (reinterpret_cast<uintptr_t>(d_input) & 15) != 0 || len > SIZE_MAX / 5)
        return fail(kInvalidArgument, "a non-empty buffer on a 16-byte boundary");
    if (d_arena == nullptr)
        return fail(kInvalidArgument, "NULL arena");
    HIP_TRY(dxtlt::pixels::launch_auto_candidates(pixel_bytes, d_input, d_arena, len / (size_t)pixel_bytes,
                                                  static_cast<hipStream_t>(hip_stream)),
            "pixel candidate kernel launch");
    return kOk;
}

}  // extern "C"
