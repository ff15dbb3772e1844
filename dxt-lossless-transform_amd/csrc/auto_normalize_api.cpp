// auto_normalize_api.cpp -- transform_bcN_auto_with_normalization on the device, BC1 and BC2 (include/dxtlt_auto_normalize.h;
// the definition: docs/ESTIMATOR.md, "Auto transform with block normalisation").
//
// The flow, all on the caller's stream: a read-only classification launch into this thread's flag word and a wait for it; with
// the flag 0 the plain transform_auto_device path; otherwise ONE candidate kernel (auto_normalize_kernels.hip) that reads the input
// once and writes the colour section of all 12 / 24 (normalisation, variant, split) candidates into the per-thread arena, the
// built-in estimator over them where they lie, one readback of 12 / 24 counters, the pick (auto_normalize_pick, pure), and the
// winner's fused normalise + transform launch, which is not waited for.  Without the arena -- an input off a 16-byte boundary,
// dxtlt_debug_auto_use_arena(0), a failed allocation -- every candidate is one fused normalise + transform into d_out, estimated
// there in stream order into the counter of its section: the same sizes, the same pick.  The host-pointer calls with the built-in
// estimator (normalize_api.cpp) stage their buffer and run this flow.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dxtlt_auto_normalize.h"
#include "../../include/dxtlt_bc1_normalize.h"
#include "../../include/dxtlt_gfx950.h"
#include "auto_launch.h"
#include "bcn_launch.h"
#include "host_common.h"

using namespace dxtlt_host;

namespace {

// dxtlt_debug_auto_normalization_last: waits, candidate launches, estimator launches, the flag
thread_local uint64_t t_last[4] = {0, 0, 0, 0};

struct NormOrder {
    AutoChoice order[16];
    int count;   // 4 or 8: also the sections of one normalisation mode
};

NormOrder order_of(int32_t format, bool use_all)
{
    NormOrder o{};
    o.count = auto_candidate_order(format, use_all, o.order);
    return o;
}

int section_of(const NormOrder& o, int norm, int i) { return norm * o.count + 2 * o.order[i].mode + (o.order[i].split_colour ? 1 : 0); }

// THE pick of every route.  sizes: 3 * count estimates in section order; totals: the same in candidate order (norm * count +
// position in the test order).  Strict `<` in candidate order against (None, Variant1, split) with the maximum size.
AutoNormalizeChoice auto_normalize_pick(int32_t format, bool use_all, const uint64_t* sizes, uint64_t* totals)
{
    const NormOrder o = order_of(format, use_all);
    AutoNormalizeChoice best{DXTLT_NORMALIZE_NONE, 1, true};
    uint64_t best_size = UINT64_MAX;
    for (int norm = 0; norm < 3; ++norm)
        for (int i = 0; i < o.count; ++i) {
            const uint64_t size = sizes[section_of(o, norm, i)];
            totals[norm * o.count + i] = size;
            if (size < best_size) {
                best_size = size;
                best = AutoNormalizeChoice{(uint8_t)norm, o.order[i].mode, o.order[i].split_colour};
            }
        }
    return best;
}

// waits for the stream on every exit but the one that disarms it: the flag word, the arena and the counters belong to this
// thread's next call
struct Drain {
    hipStream_t stream;
    bool armed = true;
    ~Drain()
    {
        if (armed) (void)hipStreamSynchronize(stream);
    }
};

int32_t device_call(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all, void* hip_stream, uint8_t* out_norm,
                    uint8_t* out_mode, bool* out_split)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (len % (format == 1 ? 8 : 16) != 0)
        return fail(kInvalidLength, format == 1 ? "len is not a multiple of 8" : "len is not a multiple of 16");
    if (len > 0 && (d_in == nullptr || d_out == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with len > 0");
    AutoNormalizeChoice choice{DXTLT_NORMALIZE_NONE, 0, false};
    if (len == 0) {
        t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
        AutoChoice c{};
        if (int32_t rc = transform_auto_device(format, d_in, d_out, 0, use_all, st, &c))
            return rc;
        choice = AutoNormalizeChoice{DXTLT_NORMALIZE_NONE, c.mode, c.split_colour};
    } else {
        int count = 0;
        hipError_t e = hipGetDeviceCount(&count);
        if (e != hipSuccess || count <= 0)
            return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
        if (stream_is_capturing(st))
            return fail(kInvalidArgument, "the auto transforms read their estimates back and wait for the stream: not capturable");
        if (int32_t rc = auto_normalize_on_device(format, d_in, d_out, len, use_all, st, &choice))
            return rc;
    }
    if (out_norm) *out_norm = choice.norm;
    if (out_mode) *out_mode = choice.mode;
    if (out_split) *out_split = choice.split_colour;
    return kOk;
}

}  // namespace

int32_t dxtlt_host::auto_normalize_on_device(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all, hipStream_t st,
                                             AutoNormalizeChoice* choice)
{
    t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
    const uint64_t blocks = len / (format == 1 ? 8 : 16);
    Drain drain{st};

    // 1. would any block change?
    uint32_t* d_flag = nullptr;
    uint32_t any = 0;
    if (int32_t rc = normalize_thread_flag(&d_flag, st))
        return rc;
    HIP_TRY(format == 1 ? dxtlt::launch_bc1_any_normalizable(d_in, blocks, d_flag, st) : dxtlt::launch_bc2_any_normalizable(d_in, blocks, d_flag, st),
            "classification launch");
    HIP_TRY(hipMemcpyAsync(&any, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H flag");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    t_last[0] = 1;
    t_last[3] = any;

    // 2. nothing to normalise: the plain auto transform, mode None
    if (any == 0) {
        drain.armed = false;   // nothing of this flow is in flight; the plain path keeps its own invariant
        AutoChoice c{};
        const int32_t rc = transform_auto_device(format, d_in, d_out, len, use_all, st, &c);
        t_last[0] = 2;
        *choice = AutoNormalizeChoice{DXTLT_NORMALIZE_NONE, c.mode, c.split_colour};
        return rc;
    }

    // 3. every candidate's colour section and its estimate
    auto_begin_device_call();
    const NormOrder o = order_of(format, use_all);
    const dxtlt::AutoNormalizeSections secs = dxtlt::auto_normalize_sections(use_all, blocks);
    uint8_t* arena = nullptr;
    if (!auto_arena_disabled() && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0)
        arena = static_cast<uint8_t*>(auto_thread_arena((size_t)secs.bytes));
    if (arena != nullptr) {
        int launches = 0;
        HIP_TRY(dxtlt::launch_auto_normalize_candidates((dxtlt::Format)format, use_all, d_in, arena, blocks, st, &launches),
                "candidate kernel launch");
        t_last[1] = (uint64_t)launches;
        dxtlt::EstimateSection shown[24];
        for (int k = 0; k < secs.count; ++k)
            shown[k] = {arena + secs.off[k], secs.len[k]};
        if (int32_t rc = estimate_enqueue(shown, (size_t)secs.count, st, 0))
            return rc;
        t_last[2] = (uint64_t)(secs.count + 15) / 16;
    } else {
        // one fused normalise + transform per candidate into d_out, estimated there before the next one overwrites it (stream order).
        // BC1's `None` candidates are estimated with their transparent blocks rewritten: internal fused mode 3.
        uint8_t* out8 = static_cast<uint8_t*>(d_out);
        const dxtlt::EstimateSection shown = format == 1 ? dxtlt::EstimateSection{out8, len / 2} : dxtlt::EstimateSection{out8 + len / 2, len / 4};
        for (int norm = 0; norm < 3; ++norm) {
            const int fused = dxtlt::norm_estimation_mode(format, norm);
            for (int i = 0; i < o.count; ++i) {
                if (int32_t rc = enqueue(format, false, d_in, d_out, blocks, dxtlt::Settings{o.order[i].mode, false, o.order[i].split_colour, fused}, st))
                    return rc;
                ++t_last[1];
                if (int32_t rc = estimate_enqueue(&shown, 1, st, (size_t)section_of(o, norm, i)))
                    return rc;
                ++t_last[2];
            }
        }
    }
    uint64_t sizes[kMaxCounters], totals[24];
    if (int32_t rc = estimate_read_back((size_t)secs.count, st, sizes))
        return rc;
    t_last[0] = 2;
    drain.armed = false;   // the stream is idle: what follows reads d_in and writes d_out alone

    // 4., 5. the pick, and the winner as transform_bcN_with_normalize_blocks defines it (a `None` winner without the rewrite)
    *choice = auto_normalize_pick(format, use_all, sizes, totals);
    if (int32_t rc = enqueue(format, false, d_in, d_out, blocks, dxtlt::Settings{choice->mode, false, choice->split_colour, choice->norm}, st))
        return rc;
    auto_set_last_totals(totals, secs.count);
    return kOk;
}

extern "C" {

int32_t dxtlt_transform_bc1_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(1, d_input, d_output, len, use_all, hip_stream, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints);
}

int32_t dxtlt_transform_bc2_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(2, d_input, d_output, len, use_all, hip_stream, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints);
}

int32_t dxtlt_debug_auto_normalization_sections(int32_t format, bool use_all, uint64_t blocks, uint64_t out_off[24], uint64_t out_len[24])
{
    if (format != 1 && format != 2)
        return -1;
    const dxtlt::AutoNormalizeSections s = dxtlt::auto_normalize_sections(use_all, blocks);
    for (int k = 0; k < s.count; ++k) {
        if (out_off) out_off[k] = s.off[k];
        if (out_len) out_len[k] = s.len[k];
    }
    return s.count;
}

int32_t dxtlt_debug_auto_normalization_pick(int32_t format, bool use_all, const uint64_t* sizes, int32_t n, uint64_t* out_totals, int32_t cap,
                                            uint8_t* out_color_mode, uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints)
{
    if ((format != 1 && format != 2) || sizes == nullptr || n != (use_all ? 24 : 12))
        return fail(kInvalidArgument, "auto normalisation pick: format 1 or 2 and 12 (fast) or 24 (all modes) sizes");
    uint64_t totals[24];
    const AutoNormalizeChoice c = auto_normalize_pick(format, use_all, sizes, totals);
    for (int i = 0; out_totals != nullptr && i < n && i < cap; ++i)
        out_totals[i] = totals[i];
    if (out_color_mode) *out_color_mode = c.norm;
    if (out_decorrelation_mode) *out_decorrelation_mode = c.mode;
    if (out_split_colour_endpoints) *out_split_colour_endpoints = c.split_colour;
    return kOk;
}

int32_t dxtlt_debug_auto_normalization_candidates_into_device(int32_t format, bool use_all, const void* d_input, size_t len, void* d_arena,
                                                              uint64_t arena_bytes, void* hip_stream)
{
    if ((format != 1 && format != 2) || len % (format == 1 ? 8 : 16) != 0)
        return fail(kInvalidArgument, "auto normalisation candidates: format 1 or 2, a whole number of blocks");
    if (len == 0)
        return kOk;
    if (d_input == nullptr || d_arena == nullptr || ((reinterpret_cast<uintptr_t>(d_input) | reinterpret_cast<uintptr_t>(d_arena)) & 15) != 0)
        return fail(kInvalidArgument, "auto normalisation candidates: input and arena on a 16-byte boundary");
    const uint64_t blocks = len / (format == 1 ? 8 : 16);
    if (arena_bytes < dxtlt::auto_normalize_sections(use_all, blocks).bytes)
        return fail(kInvalidArgument, "auto normalisation candidates: an arena smaller than auto_normalize_sections' bytes");
    HIP_TRY(dxtlt::launch_auto_normalize_candidates((dxtlt::Format)format, use_all, d_input, d_arena, blocks, static_cast<hipStream_t>(hip_stream),
                                                    nullptr),
            "candidate kernel launch");
    return kOk;
}

void dxtlt_debug_auto_normalization_last(uint64_t out[4])
{
    for (int i = 0; out != nullptr && i < 4; ++i)
        out[i] = t_last[i];
}

}  // extern "C"
