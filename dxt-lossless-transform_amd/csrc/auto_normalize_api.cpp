// auto_normalize_api.cpp -- transform_bcN_auto_with_normalization, BC1 and BC2 (include/dxtlt_bc1_normalize.h,
// include/dxtlt_auto_normalize.h; the definition: docs/ESTIMATOR.md, "Auto transform with block normalisation").
//
// transform_bc1_auto_with_normalization (the reference's dxt-lossless-transform-bc1/src/experimental/normalize_blocks/
// transform.rs:222-333) as the reference runs it:
//   * one max_compressed_size(len / 2) query up front (its failure is the only estimator error that propagates);
//   * all blocks are classified once; if no block would change, the call IS transform_bc1_auto;
//   * otherwise for mode in {None, Color0Only, ReplicateColor}, for (decorrelation, split) in the BC1 test order:
//     the estimator sees the first len / 2 bytes (the colour section) of transform(normalize(input, mode));
//     a failing estimate skips that candidate; strict `<` against the running best, which starts at
//     {None, Variant1, split} with size usize::MAX;
//   * the data is transformed once more with the winner.
// BC2 has the same call (this build's extension: the colour section is [len / 2, + len / 4), the `None` candidates are the input's
// own colours).  Stated once below and used by every flow: the section shown (shown_section), the candidate walk (candidate_of),
// the classification step (classify) and the fold (auto_normalize_pick).
//
// The device flow (auto_normalize_on_device), all on the caller's stream: the read-only classification launch into this thread's flag
// word and a wait for it; with the flag 0 the plain transform_auto_device path; otherwise ONE candidate kernel
// (auto_normalize_kernels.hip) that reads the input once and writes the colour section of all 12 / 24 (normalisation, variant,
// split) candidates into the per-thread arena, the built-in estimator over them where they lie, one readback of 12 / 24 counters,
// the pick, and the winner's fused normalise + transform launch, which is not waited for.  Without the arena -- an input off a
// 16-byte boundary, dxtlt_debug_auto_use_arena(0), a failed allocation -- every candidate is one fused normalise + transform into
// d_out, estimated there in stream order into the counter of its section: the same sizes, the same pick.  The host-pointer calls
// given the built-in estimator stage their buffer and run this flow: no section travels and no callback is made.
//
// The callback flow (auto_with_callbacks), any other estimator on host pointers: the input is uploaded once and classified; every
// candidate is one fused normalise + transform launch on the resident copy and only its colour section travels back.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/dxtlt_auto_normalize.h"
#include "../../include/dxtlt_bc1_normalize.h"
#include "../../include/dxtlt_estimator.h"
#include "../../include/dxtlt_gfx950.h"
#include "auto_call.h"
#include "auto_launch.h"
#include "bcn_launch.h"

using namespace dxtlt_host;

namespace {

constexpr int kMaxCandidates = 24;   // 3 normalisation modes x 8 (variant, split) with every decorrelation mode
static_assert(kMaxCandidates <= kAutoTotalsCap, "dxtlt_debug_auto_last_totals holds every candidate's total");
static_assert(kMaxCandidates <= (int)kMaxCounters, "one estimate counter per candidate");

// dxtlt_debug_auto_normalization_last: waits, candidate launches, estimator launches, the flag
thread_local uint64_t t_last[4] = {0, 0, 0, 0};

struct AutoNormalizeChoice {
    uint8_t norm;   // ColorNormalizationMode
    uint8_t mode;   // core numbering
    bool split_colour;
};

AutoNormalizeChoice without_normalization(const AutoChoice& c) { return {DXTLT_NORMALIZE_NONE, c.mode, c.split_colour}; }

// the choice of a successful call through the out-parameters of a C entry point, every one of which may be NULL
int32_t store_choice(int32_t rc, const AutoNormalizeChoice& c, uint8_t* out_norm, uint8_t* out_mode, bool* out_split)
{
    if (rc == kOk) {
        store_if(out_norm, c.norm);
        store_if(out_mode, c.mode);
        store_if(out_split, c.split_colour);
    }
    return rc;
}

// The section of a transformed buffer of `len` bytes the estimator is shown, its colour endpoints: BC1 [0, len / 2), BC2
// [len / 2, + len / 4).
struct Span {
    size_t off, len;
};
Span shown_section(const NormFormat& F, size_t len) { return F.fmt == 1 ? Span{0, len / 2} : Span{len / 2, len / 4}; }

struct NormOrder {
    AutoChoice order[16];
    int count;   // 4 or 8: also the sections of one normalisation mode
};

NormOrder order_of(const NormFormat& F, bool use_all)
{
    NormOrder o{};
    o.count = auto_candidate_order(F.fmt, use_all, o.order);
    return o;
}

// Candidate k of the walk every flow makes, k = norm * count + position in the format's test order: what it is, the settings its
// ESTIMATE is made with -- BC1's `None` candidates with their fully transparent blocks rewritten, internal fused mode 3
// (dxtlt::norm_estimation_mode) -- and the section of the candidate arena, which is also the counter, that holds its estimate.
struct NormCandidate {
    AutoNormalizeChoice is;
    dxtlt::Settings estimated;
    int section;
};

NormCandidate candidate_of(const NormFormat& F, const NormOrder& o, int k)
{
    const int norm = k / o.count;
    const AutoChoice& c = o.order[k % o.count];
    return {{(uint8_t)norm, c.mode, c.split_colour},
            dxtlt::Settings{c.mode, false, c.split_colour, dxtlt::norm_estimation_mode(F.fmt, norm)},
            norm * o.count + 2 * c.mode + (c.split_colour ? 1 : 0)};
}

// the winner as transform_bcN_with_normalize_blocks defines it (transform.rs:307-313): a `None` winner without the rewrite its
// candidates were estimated with
dxtlt::Settings winner_settings(const AutoNormalizeChoice& c) { return dxtlt::Settings{c.mode, false, c.split_colour, c.norm}; }

// THE fold of every flow.  sizes: 3 * count estimates in section order, of which the ones whose bit of `valid` is set count (a
// failing estimate skips its candidate, transform.rs:403); totals: the same in candidate order.  Strict `<` in candidate order
// against (None, Variant1, split) with the maximum size.
AutoNormalizeChoice auto_normalize_pick(const NormFormat& F, bool use_all, const uint64_t* sizes, uint32_t valid, uint64_t* totals)
{
    const NormOrder o = order_of(F, use_all);
    AutoNormalizeChoice best{DXTLT_NORMALIZE_NONE, 1, true};
    uint64_t best_size = UINT64_MAX;
    for (int k = 0; k < 3 * o.count; ++k) {
        const NormCandidate c = candidate_of(F, o, k);
        totals[k] = sizes[c.section];
        if ((valid >> c.section & 1) != 0 && totals[k] < best_size) {
            best_size = totals[k];
            best = c.is;
        }
    }
    return best;
}
constexpr uint32_t kEveryEstimate = (1u << kMaxCandidates) - 1;

// Step 1 of both flows: would any block of the `len` bytes at d_in change?  Zeroes this thread's flag word, launches the read-only
// classification, reads the flag back and waits for `st`.
int32_t classify(const NormFormat& F, const void* d_in, size_t len, hipStream_t st, const char* launch_text, uint32_t* any)
{
    uint32_t* d_flag = nullptr;
    if (int32_t rc = normalize_thread_flag(&d_flag, st))
        return rc;
    const uint64_t blocks = len / F.block_bytes;
    HIP_TRY(F.fmt == 1 ? dxtlt::launch_bc1_any_normalizable(d_in, blocks, d_flag, st) : dxtlt::launch_bc2_any_normalizable(d_in, blocks, d_flag, st),
            launch_text);
    HIP_TRY(hipMemcpyAsync(any, d_flag, sizeof(uint32_t), hipMemcpyDeviceToHost, st), "D2H flag");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    return kOk;
}

// Device pointers, the built-in estimator; the arguments are valid and len > 0.  Two waits for `st` (the flag, the counters); the
// winner's fused normalise + transform launch is left enqueued.  When it returns, successful or not, nothing in flight uses this
// thread's flag word, arena or counters.
int32_t auto_normalize_on_device(const NormFormat& F, const void* d_in, void* d_out, size_t len, bool use_all, hipStream_t st,
                                 AutoNormalizeChoice* choice)
{
    t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
    const uint64_t blocks = len / F.block_bytes;
    StreamDrain drain{st, true};

    // 1. would any block change?
    uint32_t any = 0;
    if (int32_t rc = classify(F, d_in, len, st, "classification launch", &any))
        return rc;
    t_last[0] = 1;
    t_last[3] = any;

    // 2. nothing to normalise: the plain auto transform, mode None
    if (any == 0) {
        drain.armed = false;   // nothing of this flow is in flight; the plain path keeps its own invariant
        AutoChoice c{};
        const int32_t rc = transform_auto_device(F.fmt, d_in, d_out, len, use_all, st, &c);
        t_last[0] = 2;
        *choice = without_normalization(c);
        return rc;
    }

    // 3. every candidate's colour section and its estimate
    AutoThreadState& state = auto_state();
    state.begin_call();
    const NormOrder o = order_of(F, use_all);
    const dxtlt::AutoNormalizeSections secs = dxtlt::auto_normalize_sections(use_all, blocks);
    uint8_t* arena = nullptr;
    if (!state.no_arena && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0)
        arena = static_cast<uint8_t*>(state.arena.get((size_t)secs.bytes));
    if (arena != nullptr) {
        int launches = 0;
        HIP_TRY(dxtlt::launch_auto_normalize_candidates((dxtlt::Format)F.fmt, use_all, d_in, arena, blocks, st, &launches),
                "candidate kernel launch");
        t_last[1] = (uint64_t)launches;
        dxtlt::EstimateSection shown[kMaxCandidates];
        for (int k = 0; k < secs.count; ++k)
            shown[k] = {arena + secs.off[k], secs.len[k]};
        if (int32_t rc = estimate_enqueue(shown, (size_t)secs.count, st, 0))
            return rc;
        t_last[2] = (uint64_t)(secs.count + 15) / 16;
    } else {
        // one fused normalise + transform per candidate into d_out, estimated there before the next one overwrites it (stream order)
        const Span span = shown_section(F, len);
        const dxtlt::EstimateSection shown{static_cast<uint8_t*>(d_out) + span.off, span.len};
        for (int k = 0; k < 3 * o.count; ++k) {
            const NormCandidate c = candidate_of(F, o, k);
            if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, c.estimated, st))
                return rc;
            ++t_last[1];
            if (int32_t rc = estimate_enqueue(&shown, 1, st, (size_t)c.section))
                return rc;
            ++t_last[2];
        }
    }
    uint64_t sizes[kMaxCounters], totals[kMaxCandidates];
    if (int32_t rc = estimate_read_back((size_t)secs.count, st, sizes))
        return rc;
    t_last[0] = 2;
    drain.armed = false;   // the stream is idle: what follows reads d_in and writes d_out alone

    // 4., 5. the pick and the winner
    *choice = auto_normalize_pick(F, use_all, sizes, kEveryEstimate, totals);
    if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, winner_settings(*choice), st))
        return rc;
    state.set_last_totals(totals, secs.count);
    return kOk;
}

int32_t device_call(const NormFormat& F, const void* d_in, void* d_out, size_t len, bool use_all, void* hip_stream, uint8_t* out_norm,
                    uint8_t* out_mode, bool* out_split)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (len > 0 && (d_in == nullptr || d_out == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with len > 0");
    AutoNormalizeChoice choice{DXTLT_NORMALIZE_NONE, 0, false};
    int32_t rc;
    if (len == 0) {
        t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
        AutoChoice c{};
        rc = transform_auto_device(F.fmt, d_in, d_out, 0, use_all, st, &c);
        choice = without_normalization(c);
    } else {
        rc = auto_device_call(st, [&] { return auto_normalize_on_device(F, d_in, d_out, len, use_all, st, &choice); });
    }
    return store_choice(rc, choice, out_norm, out_mode, out_split);
}

// Any estimator but the built-in one, on host pointers: one MaxCompressedSize(shown length), the classification, then per candidate
// in order one full fused transform on the resident copy, the download of its colour section into `out` where the reference
// estimates it, and one EstimateCompressedSize; the winner is transformed again unless it is what the last candidate left in d_out.
// This flow does not count its downloads and callbacks for dxtlt_debug_auto_last_estimation, leaves the totals of
// dxtlt_debug_auto_last_totals alone and records nothing for dxtlt_debug_auto_last_estimator_error: those figures are the plain
// auto call's when no block is normalisable, and an earlier call's otherwise.
int32_t auto_with_callbacks(const NormFormat& F, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* est, bool use_all,
                            AutoNormalizeChoice* choice, uint32_t* estimator_error)
{
    const Span shown = shown_section(F, len);
    size_t max_comp = 0;
    if (uint32_t bad = est->MaxCompressedSize(est->Context, shown.len, &max_comp)) {
        *estimator_error = bad;
        return fail(kEstimator, "size estimator: max_compressed_size failed");
    }
    void *d_in = nullptr, *d_out = nullptr;
    StreamDrain drain;
    hipStream_t& st = drain.stream;
    uint32_t any = 0;
    if (len > 0) {
        if (int32_t rc = acquire_staging(len, &d_in, &d_out, &st))
            return rc;
        drain.armed = true;
        HIP_TRY(hipMemcpyAsync(d_in, in, len, hipMemcpyHostToDevice, st), "H2D copy");
        if (int32_t rc = classify(F, d_in, len, st, "kernel launch", &any))
            return rc;
    }
    if (any == 0) {
        // transform.rs:321-331: nothing to normalise -> the regular brute force, mode None
        drain.armed = false;   // the stream is idle; the plain call keeps its own invariant
        AutoChoice c{};
        const int32_t rc = transform_auto(F.fmt, in, out, len, est, use_all, &c);
        *estimator_error = c.estimator_error;
        *choice = without_normalization(c);
        return rc;
    }

    EstimatorScratch scratch;
    if (!scratch.allocate(max_comp))
        return fail(kAllocation, "estimator scratch allocation failed");
    const NormOrder o = order_of(F, use_all);
    const uint64_t blocks = len / F.block_bytes;
    uint64_t sizes[kMaxCandidates] = {}, totals[kMaxCandidates];
    uint32_t valid = 0;
    NormCandidate last{};   // the candidate whose transform is in d_out
    for (int k = 0; k < 3 * o.count; ++k) {
        last = candidate_of(F, o, k);
        if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, last.estimated, st))
            return rc;
        hipError_t herr = hipMemcpyAsync(out + shown.off, static_cast<const uint8_t*>(d_out) + shown.off, shown.len, hipMemcpyDeviceToHost, st);
        if (herr == hipSuccess)
            herr = hipStreamSynchronize(st);
        if (herr != hipSuccess)
            return fail(kDevice, "candidate transform / download", herr);
        size_t size = 0;
        if (est->EstimateCompressedSize(est->Context, out + shown.off, shown.len, scratch.ptr, max_comp, &size) != 0)
            continue;   // skipped: its bit of `valid` stays clear
        sizes[last.section] = size;
        valid |= 1u << last.section;
    }
    *choice = auto_normalize_pick(F, use_all, sizes, valid, totals);

    const bool resident = last.is.norm == choice->norm && last.is.mode == choice->mode && last.is.split_colour == choice->split_colour &&
                          last.estimated.normalize == choice->norm;
    if (!resident)
        if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, winner_settings(*choice), st))
            return rc;
    HIP_TRY(hipMemcpyAsync(out, d_out, len, hipMemcpyDeviceToHost, st), "D2H result");
    HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
    drain.armed = false;
    return kOk;
}

// transform_bcN_auto_with_normalization on host pointers.  The built-in estimator is recognised and never called: one upload, the
// device flow, one download.
int32_t host_call(const NormFormat& F, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* est, bool use_all,
                  uint8_t* out_norm, uint8_t* out_mode, bool* out_split, uint32_t* out_estimator_error)
{
    store_if(out_estimator_error, 0u);
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (est == nullptr || est->MaxCompressedSize == nullptr || est->EstimateCompressedSize == nullptr)
        return fail(kInvalidArgument, "NULL estimator");
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");

    AutoNormalizeChoice choice{DXTLT_NORMALIZE_NONE, 0, false};
    uint32_t estimator_error = 0;
    int32_t rc;
    if (!is_builtin_estimator(est)) {
        rc = auto_with_callbacks(F, in, out, len, est, use_all, &choice, &estimator_error);
    } else if (len == 0) {
        AutoChoice c{};
        rc = transform_auto(F.fmt, in, out, 0, est, use_all, &c);
        choice = without_normalization(c);
    } else {
        rc = auto_staged_call(in, out, len, [&](const void* d_in, void* d_out, hipStream_t st) {
            return auto_normalize_on_device(F, d_in, d_out, len, use_all, st, &choice);
        });
    }
    store_if(out_estimator_error, estimator_error);
    return store_choice(rc, choice, out_norm, out_mode, out_split);
}

}  // namespace

extern "C" {

int32_t dxtlt_transform_bc1_auto_with_normalization(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                                    const DltSizeEstimator* est, bool use_all, uint8_t* out_color_mode,
                                                    uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                                    uint32_t* out_estimator_error)
{
    return host_call(kNormBc1, input_ptr, output_ptr, len, est, use_all, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints,
                     out_estimator_error);
}

int32_t dxtlt_transform_bc2_auto_with_normalization(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                                    const DltSizeEstimator* est, bool use_all, uint8_t* out_color_mode,
                                                    uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                                    uint32_t* out_estimator_error)
{
    return host_call(kNormBc2, input_ptr, output_ptr, len, est, use_all, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints,
                     out_estimator_error);
}

int32_t dxtlt_transform_bc1_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(kNormBc1, d_input, d_output, len, use_all, hip_stream, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints);
}

int32_t dxtlt_transform_bc2_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(kNormBc2, d_input, d_output, len, use_all, hip_stream, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints);
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
    uint64_t totals[kMaxCandidates];
    const AutoNormalizeChoice c = auto_normalize_pick(format == 1 ? kNormBc1 : kNormBc2, use_all, sizes, kEveryEstimate, totals);
    for (int i = 0; out_totals != nullptr && i < n && i < cap; ++i)
        out_totals[i] = totals[i];
    return store_choice(kOk, c, out_color_mode, out_decorrelation_mode, out_split_colour_endpoints);
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
