// auto_normalize_api.cpp -- transform_bcN_auto_with_normalization, BC1, BC2 and BC3 (include/dxtlt_bc1_normalize.h,
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
// BC3 (this build's extension) adds an alpha part: alpha_mode over 0..3 outside the colour modes, the test order is BC3's 8 / 16
// (variant, split alpha, split colour), and a candidate's total is est(alpha endpoints [0, 2N)) + est(colour endpoints
// [len / 2, + 4N)).  The two halves of a block are normalised independently, so the 96 / 192 totals are sums over 8 alpha sections
// (alpha mode, split alpha) and BC2's 12 / 24 colour sections: a format's plan (plan_of) says how many sections of each kind there
// are, candidate_of which two a candidate adds, and fused_launch which full transforms show every section once.
//
// The device flow (auto_normalize_on_device), all on the caller's stream: the read-only classification launch into this thread's flag
// word and a wait for it; with the flag 0 the plain transform_auto_device path; otherwise ONE candidate kernel
// (auto_normalize_kernels.hip) that reads the input once and writes the colour section of all 12 / 24 (normalisation, variant,
// split) candidates into the per-thread arena, the built-in estimator over them where they lie, one readback of 12 / 24 counters,
// the pick, and the winner's fused normalise + transform launch, which is not waited for.  Without the arena -- an input off a
// 16-byte boundary, dxtlt_debug_auto_use_arena(0), a failed allocation -- every candidate is one fused normalise + transform into
// d_out, estimated there in stream order into the counter of its section: the same sizes, the same pick.  The host-pointer calls
// given the built-in estimator stage their buffer and run this flow: no section travels and no callback is made.
// BC3: the candidate kernel writes 8 alpha + 12 / 24 colour sections (20 / 32 counters, kMaxCounters), the pick is the literal
// 96 / 192-entry walk over their sums, and without the arena 12 / 24 fused launches show every section once (fused_launch).
//
// The callback flow (auto_with_callbacks), any other estimator on host pointers: the input is uploaded once and classified; every
// candidate is one fused normalise + transform launch on the resident copy and only its colour section travels back.
#include <hip/hip_runtime.h>

#include <algorithm>
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

constexpr int kMaxCandidates = 192;  // BC3: 4 alpha modes x 3 colour modes x 16 (variant, split alpha, split colour)
constexpr int kMaxSections = 32;     // BC3: 8 alpha sections + 24 colour sections with every decorrelation mode
static_assert(kMaxCandidates <= kAutoTotalsCap, "dxtlt_debug_auto_last_totals holds every candidate's total");
static_assert(kMaxSections <= (int)kMaxCounters, "one estimate counter per section");

// dxtlt_debug_auto_normalization_last: waits, candidate launches, estimator launches, the flag
thread_local uint64_t t_last[4] = {0, 0, 0, 0};

struct AutoNormalizeChoice {
    uint8_t alpha_norm;   // AlphaNormalizationMode, BC3; 0 otherwise
    uint8_t norm;         // ColorNormalizationMode
    uint8_t mode;         // core numbering
    bool split_alpha;     // BC3
    bool split_colour;
};

AutoNormalizeChoice without_normalization(const AutoChoice& c) { return {0, DXTLT_NORMALIZE_NONE, c.mode, c.split_alpha, c.split_colour}; }

// where a C entry point wants the choice: every pointer may be NULL, the alpha ones are BC3's
struct ChoiceOuts {
    uint8_t* alpha_norm;
    uint8_t* norm;
    uint8_t* mode;
    bool* split_alpha;
    bool* split_colour;
};

// the choice of a successful call through the out-parameters of a C entry point
int32_t store_choice(int32_t rc, const AutoNormalizeChoice& c, const ChoiceOuts& out)
{
    if (rc == kOk) {
        store_if(out.alpha_norm, c.alpha_norm);
        store_if(out.norm, c.norm);
        store_if(out.mode, c.mode);
        store_if(out.split_alpha, c.split_alpha);
        store_if(out.split_colour, c.split_colour);
    }
    return rc;
}

// The sections of a transformed buffer of `len` bytes the estimator is shown: the colour endpoints -- BC1 [0, len / 2), BC2 and BC3
// [len / 2, + len / 4) -- and, BC3, the alpha endpoints [0, len / 8) (a format without an alpha part: no bytes).
struct Span {
    size_t off, len;
};
Span shown_section(const NormFormat& F, size_t len) { return F.fmt == 1 ? Span{0, len / 2} : Span{len / 2, len / 4}; }
Span shown_alpha_section(const NormFormat& F, size_t len) { return F.fmt == 3 ? Span{0, len / 8} : Span{0, 0}; }

// What the flows know about (format, search depth): the test order, and how the candidates and the sections are counted.
// Candidates: alpha_modes x 3 colour modes x count.  Sections, which are also the estimate counters: alpha_sections (0, or BC3's
// 8 = 4 alpha modes x split) in front of colour_sections (3 colour modes x variants x split).
struct NormPlan {
    AutoChoice order[16];
    int count;             // 4 or 8 (BC1 / BC2), 8 or 16 (BC3)
    int variants;          // 2 or 4
    int alpha_modes;       // 1, BC3: 4
    int alpha_sections;    // 0, BC3: 8
    int colour_sections;   // 12 or 24
    int candidates() const { return alpha_modes * 3 * count; }
    int sections() const { return alpha_sections + colour_sections; }
};

NormPlan plan_of(const NormFormat& F, bool use_all)
{
    NormPlan o{};
    o.count = auto_candidate_order(F.fmt, use_all, o.order);
    o.variants = use_all ? 4 : 2;
    o.alpha_modes = F.fmt == 3 ? 4 : 1;
    o.alpha_sections = F.fmt == 3 ? dxtlt::kBc3AlphaSections : 0;
    o.colour_sections = 3 * 2 * o.variants;
    return o;
}

// Candidate k of the walk every flow makes, k = (alpha_mode * 3 + norm) * count + position in the format's test order: what it
// is, the settings its ESTIMATE is made with -- BC1's `None` candidates with their fully transparent blocks rewritten, internal
// fused mode 3 (dxtlt::norm_estimation_mode) -- and the sections of the candidate arena, which are also the counters, whose
// estimates it is the sum of: its colour section and, BC3, its alpha section (-1 without an alpha part).
struct NormCandidate {
    AutoNormalizeChoice is;
    dxtlt::Settings estimated;
    int section;
    int alpha_section;
};

NormCandidate candidate_of(const NormFormat& F, const NormPlan& o, int k)
{
    const int alpha_norm = k / (3 * o.count), norm = k / o.count % 3;
    const AutoChoice& c = o.order[k % o.count];
    const bool split_alpha = o.alpha_sections != 0 && c.split_alpha;
    return {{(uint8_t)alpha_norm, (uint8_t)norm, c.mode, split_alpha, c.split_colour},
            dxtlt::Settings{c.mode, split_alpha, c.split_colour, dxtlt::norm_estimation_mode(F.fmt, norm), alpha_norm},
            o.alpha_sections + norm * 2 * o.variants + 2 * c.mode + (c.split_colour ? 1 : 0),
            o.alpha_sections != 0 ? 2 * alpha_norm + (split_alpha ? 1 : 0) : -1};
}

// The full fused transforms that, between them, show every section once -- what the flows without the arena launch, in this
// order.  BC1 / BC2: launch j is candidate j, one colour section each.  BC3: launch j shows colour section 8 + j (colour mode,
// variant and split in section order) and, for j < 8, alpha section j (alpha_mode = j / 2, split_alpha = j % 2); the later ones
// carry alpha mode None, unsplit.  12 / 24 launches either way; alpha_section = -1 where a launch's alpha part is not estimated.
NormCandidate fused_launch(const NormFormat& F, const NormPlan& o, int j)
{
    if (o.alpha_sections == 0)
        return candidate_of(F, o, j);
    const int norm = j / (2 * o.variants), variant = j / 2 % o.variants;
    const bool split_colour = (j & 1) != 0, shows_alpha = j < o.alpha_sections;
    const int alpha_norm = shows_alpha ? j / 2 : 0;
    const bool split_alpha = shows_alpha && (j & 1) != 0;
    return {{(uint8_t)alpha_norm, (uint8_t)norm, (uint8_t)variant, split_alpha, split_colour},
            dxtlt::Settings{variant, split_alpha, split_colour, dxtlt::norm_estimation_mode(F.fmt, norm), alpha_norm},
            o.alpha_sections + j, shows_alpha ? j : -1};
}

// the winner as transform_bcN_with_normalize_blocks defines it (transform.rs:307-313): a `None` winner without the rewrite its
// candidates were estimated with
dxtlt::Settings winner_settings(const AutoNormalizeChoice& c)
{
    return dxtlt::Settings{c.mode, c.split_alpha, c.split_colour, c.norm, c.alpha_norm};
}

bool same_settings(const dxtlt::Settings& a, const dxtlt::Settings& b)
{
    return a.variant == b.variant && a.split_alpha == b.split_alpha && a.split_colour == b.split_colour && a.normalize == b.normalize &&
           a.normalize_alpha == b.normalize_alpha;
}

// THE fold of every flow.  sizes: the estimates in section order, of which the ones whose bit of `valid` is set count (a failing
// estimate skips every candidate that uses its section, transform.rs:403); totals: the candidates' sums in candidate order -- the
// colour section's estimate plus, BC3, the alpha section's, wrapping as the plain BC3 call's sum does.  Strict `<` in candidate
// order against (None, None, Variant1, split [alpha and] colour) with the maximum size.
AutoNormalizeChoice auto_normalize_pick(const NormFormat& F, bool use_all, const uint64_t* sizes, uint32_t valid, uint64_t* totals)
{
    const NormPlan o = plan_of(F, use_all);
    AutoNormalizeChoice best{0, DXTLT_NORMALIZE_NONE, 1, o.alpha_sections != 0, true};
    uint64_t best_size = UINT64_MAX;
    for (int k = 0; k < o.candidates(); ++k) {
        const NormCandidate c = candidate_of(F, o, k);
        bool counts = (valid >> c.section & 1) != 0;
        totals[k] = sizes[c.section];
        if (c.alpha_section >= 0) {
            totals[k] += sizes[c.alpha_section];
            counts = counts && (valid >> c.alpha_section & 1) != 0;
        }
        if (counts && totals[k] < best_size) {
            best_size = totals[k];
            best = c.is;
        }
    }
    return best;
}
constexpr uint32_t kEveryEstimate = 0xFFFFFFFFu;
static_assert(kMaxSections <= 32, "one bit of `valid` per section");

// the candidate arena of `blocks` blocks (auto_launch.h)
dxtlt::AutoNormalizeSections arena_layout(const NormFormat& F, bool use_all, uint64_t blocks)
{
    return F.fmt == 3 ? dxtlt::auto_normalize_bc3_sections(use_all, blocks) : dxtlt::auto_normalize_sections(use_all, blocks);
}

// Step 1 of both flows: would any block of the `len` bytes at d_in change?  Zeroes this thread's flag word, launches the read-only
// classification, reads the flag back and waits for `st`.
int32_t classify(const NormFormat& F, const void* d_in, size_t len, hipStream_t st, const char* launch_text, uint32_t* any)
{
    uint32_t* d_flag = nullptr;
    if (int32_t rc = normalize_thread_flag(&d_flag, st))
        return rc;
    const uint64_t blocks = len / F.block_bytes;
    HIP_TRY(F.fmt == 1   ? dxtlt::launch_bc1_any_normalizable(d_in, blocks, d_flag, st)
            : F.fmt == 2 ? dxtlt::launch_bc2_any_normalizable(d_in, blocks, d_flag, st)
                         : dxtlt::launch_bc3_any_normalizable(d_in, blocks, d_flag, st),
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

    // 3. every section a candidate is the sum of, and its estimate
    AutoThreadState& state = auto_state();
    state.begin_call();
    const NormPlan o = plan_of(F, use_all);
    const dxtlt::AutoNormalizeSections secs = arena_layout(F, use_all, blocks);
    uint8_t* arena = nullptr;
    if (!state.no_arena && (reinterpret_cast<uintptr_t>(d_in) & 15) == 0)
        arena = static_cast<uint8_t*>(state.arena.get((size_t)secs.bytes));
    if (arena != nullptr) {
        int launches = 0;
        HIP_TRY(dxtlt::launch_auto_normalize_candidates((dxtlt::Format)F.fmt, use_all, d_in, arena, blocks, st, &launches),
                "candidate kernel launch");
        t_last[1] = (uint64_t)launches;
        dxtlt::EstimateSection shown[kMaxSections];
        for (int k = 0; k < secs.count; ++k)
            shown[k] = {arena + secs.off[k], secs.len[k]};
        if (int32_t rc = estimate_enqueue(shown, (size_t)secs.count, st, 0))
            return rc;
        t_last[2] = (uint64_t)(secs.count + 15) / 16;
    } else {
        // one fused normalise + transform per colour section into d_out, its section(s) estimated there before the next one
        // overwrites them (stream order)
        const Span span = shown_section(F, len), alpha_span = shown_alpha_section(F, len);
        const dxtlt::EstimateSection shown{static_cast<uint8_t*>(d_out) + span.off, span.len};
        const dxtlt::EstimateSection shown_alpha{static_cast<uint8_t*>(d_out) + alpha_span.off, alpha_span.len};
        for (int j = 0; j < o.colour_sections; ++j) {
            const NormCandidate c = fused_launch(F, o, j);
            if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, c.estimated, st))
                return rc;
            ++t_last[1];
            if (int32_t rc = estimate_enqueue(&shown, 1, st, (size_t)c.section))
                return rc;
            ++t_last[2];
            if (c.alpha_section >= 0) {
                if (int32_t rc = estimate_enqueue(&shown_alpha, 1, st, (size_t)c.alpha_section))
                    return rc;
                ++t_last[2];
            }
        }
    }
    uint64_t sizes[kMaxCounters], totals[kMaxCandidates];
    if (int32_t rc = estimate_read_back((size_t)o.sections(), st, sizes))
        return rc;
    t_last[0] = 2;
    drain.armed = false;   // the stream is idle: what follows reads d_in and writes d_out alone

    // 4., 5. the pick and the winner
    *choice = auto_normalize_pick(F, use_all, sizes, kEveryEstimate, totals);
    if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, winner_settings(*choice), st))
        return rc;
    state.set_last_totals(totals, o.candidates());
    return kOk;
}

int32_t device_call(const NormFormat& F, const void* d_in, void* d_out, size_t len, bool use_all, void* hip_stream, const ChoiceOuts& outs)
{
    hipStream_t st = static_cast<hipStream_t>(hip_stream);
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (len > 0 && (d_in == nullptr || d_out == nullptr))
        return fail(kInvalidArgument, "NULL device buffer with len > 0");
    AutoNormalizeChoice choice{0, DXTLT_NORMALIZE_NONE, 0, false, false};
    int32_t rc;
    if (len == 0) {
        t_last[0] = t_last[1] = t_last[2] = t_last[3] = 0;
        AutoChoice c{};
        rc = transform_auto_device(F.fmt, d_in, d_out, 0, use_all, st, &c);
        choice = without_normalization(c);
    } else {
        rc = auto_device_call(st, [&] { return auto_normalize_on_device(F, d_in, d_out, len, use_all, st, &choice); });
    }
    return store_choice(rc, choice, outs);
}

// Any estimator but the built-in one, on host pointers: one MaxCompressedSize per shown length (BC3: len / 8, then len / 4), the
// classification, then per fused launch (fused_launch: BC1 / BC2 the candidates in order) one full fused transform on the resident
// copy, the download of its shown section(s) into `out` where the reference estimates them, and one EstimateCompressedSize each
// (BC3: the alpha section of the first eight launches, then the colour section): every distinct section is estimated once.  The
// winner is transformed again unless it is what the last launch left in d_out.
// This flow does not count its downloads and callbacks for dxtlt_debug_auto_last_estimation, leaves the totals of
// dxtlt_debug_auto_last_totals alone and records nothing for dxtlt_debug_auto_last_estimator_error: those figures are the plain
// auto call's when no block is normalisable, and an earlier call's otherwise.
int32_t auto_with_callbacks(const NormFormat& F, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* est, bool use_all,
                            AutoNormalizeChoice* choice, uint32_t* estimator_error)
{
    const Span shown = shown_section(F, len), shown_alpha = shown_alpha_section(F, len);
    const bool has_alpha = F.fmt == 3;
    size_t max_comp = 0, max_comp_alpha = 0;
    if (uint32_t bad = has_alpha ? est->MaxCompressedSize(est->Context, shown_alpha.len, &max_comp_alpha) : 0) {
        *estimator_error = bad;
        return fail(kEstimator, "size estimator: max_compressed_size failed");
    }
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
    if (!scratch.allocate(std::max(max_comp, max_comp_alpha)))
        return fail(kAllocation, "estimator scratch allocation failed");
    const NormPlan o = plan_of(F, use_all);
    const uint64_t blocks = len / F.block_bytes;
    uint64_t sizes[kMaxSections] = {}, totals[kMaxCandidates];
    uint32_t valid = 0;
    NormCandidate last{};   // the launch whose transform is in d_out
    for (int j = 0; j < o.colour_sections; ++j) {
        last = fused_launch(F, o, j);
        if (int32_t rc = enqueue(F.fmt, false, d_in, d_out, blocks, last.estimated, st))
            return rc;
        hipError_t herr = hipMemcpyAsync(out + shown.off, static_cast<const uint8_t*>(d_out) + shown.off, shown.len, hipMemcpyDeviceToHost, st);
        if (herr == hipSuccess && last.alpha_section >= 0)
            herr = hipMemcpyAsync(out + shown_alpha.off, static_cast<const uint8_t*>(d_out) + shown_alpha.off, shown_alpha.len,
                                  hipMemcpyDeviceToHost, st);
        if (herr == hipSuccess)
            herr = hipStreamSynchronize(st);
        if (herr != hipSuccess)
            return fail(kDevice, "candidate transform / download", herr);
        // a failing estimate is skipped: its section's bit of `valid` stays clear
        size_t size = 0;
        if (last.alpha_section >= 0 &&
            est->EstimateCompressedSize(est->Context, out + shown_alpha.off, shown_alpha.len, scratch.ptr, max_comp_alpha, &size) == 0) {
            sizes[last.alpha_section] = size;
            valid |= 1u << last.alpha_section;
        }
        if (est->EstimateCompressedSize(est->Context, out + shown.off, shown.len, scratch.ptr, max_comp, &size) == 0) {
            sizes[last.section] = size;
            valid |= 1u << last.section;
        }
    }
    *choice = auto_normalize_pick(F, use_all, sizes, valid, totals);

    const bool resident = same_settings(last.estimated, winner_settings(*choice));
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
                  const ChoiceOuts& outs, uint32_t* out_estimator_error)
{
    store_if(out_estimator_error, 0u);
    if (len % F.block_bytes != 0)
        return fail(kInvalidLength, F.bad_len);
    if (est == nullptr || est->MaxCompressedSize == nullptr || est->EstimateCompressedSize == nullptr)
        return fail(kInvalidArgument, "NULL estimator");
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");

    AutoNormalizeChoice choice{0, DXTLT_NORMALIZE_NONE, 0, false, false};
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
    return store_choice(rc, choice, outs);
}

}  // namespace

extern "C" {

int32_t dxtlt_transform_bc1_auto_with_normalization(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                                    const DltSizeEstimator* est, bool use_all, uint8_t* out_color_mode,
                                                    uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                                    uint32_t* out_estimator_error)
{
    return host_call(kNormBc1, input_ptr, output_ptr, len, est, use_all,
                     {nullptr, out_color_mode, out_decorrelation_mode, nullptr, out_split_colour_endpoints}, out_estimator_error);
}

int32_t dxtlt_transform_bc2_auto_with_normalization(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                                    const DltSizeEstimator* est, bool use_all, uint8_t* out_color_mode,
                                                    uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                                    uint32_t* out_estimator_error)
{
    return host_call(kNormBc2, input_ptr, output_ptr, len, est, use_all,
                     {nullptr, out_color_mode, out_decorrelation_mode, nullptr, out_split_colour_endpoints}, out_estimator_error);
}

int32_t dxtlt_transform_bc3_auto_with_normalization(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                                    const DltSizeEstimator* est, bool use_all, uint8_t* out_alpha_mode,
                                                    uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                    bool* out_split_alpha_endpoints, bool* out_split_colour_endpoints,
                                                    uint32_t* out_estimator_error)
{
    return host_call(kNormBc3, input_ptr, output_ptr, len, est, use_all,
                     {out_alpha_mode, out_color_mode, out_decorrelation_mode, out_split_alpha_endpoints, out_split_colour_endpoints},
                     out_estimator_error);
}

int32_t dxtlt_transform_bc1_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(kNormBc1, d_input, d_output, len, use_all, hip_stream,
                       {nullptr, out_color_mode, out_decorrelation_mode, nullptr, out_split_colour_endpoints});
}

int32_t dxtlt_transform_bc2_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(kNormBc2, d_input, d_output, len, use_all, hip_stream,
                       {nullptr, out_color_mode, out_decorrelation_mode, nullptr, out_split_colour_endpoints});
}

int32_t dxtlt_transform_bc3_auto_with_normalization_device(const void* d_input, void* d_output, size_t len, bool use_all, void* hip_stream,
                                                           uint8_t* out_alpha_mode, uint8_t* out_color_mode,
                                                           uint8_t* out_decorrelation_mode, bool* out_split_alpha_endpoints,
                                                           bool* out_split_colour_endpoints)
{
    return device_call(kNormBc3, d_input, d_output, len, use_all, hip_stream,
                       {out_alpha_mode, out_color_mode, out_decorrelation_mode, out_split_alpha_endpoints, out_split_colour_endpoints});
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
    return store_choice(kOk, c, {nullptr, out_color_mode, out_decorrelation_mode, nullptr, out_split_colour_endpoints});
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

int32_t dxtlt_debug_bc3_auto_normalization_sections(bool use_all, uint64_t blocks, uint64_t out_off[32], uint64_t out_len[32])
{
    const dxtlt::AutoNormalizeSections s = dxtlt::auto_normalize_bc3_sections(use_all, blocks);
    for (int k = 0; k < s.count; ++k) {
        if (out_off) out_off[k] = s.off[k];
        if (out_len) out_len[k] = s.len[k];
    }
    return s.count;
}

int32_t dxtlt_debug_bc3_auto_normalization_pick(bool use_all, const uint64_t* sizes, int32_t n, uint64_t* out_totals, int32_t cap,
                                                uint8_t* out_alpha_mode, uint8_t* out_color_mode, uint8_t* out_decorrelation_mode,
                                                bool* out_split_alpha_endpoints, bool* out_split_colour_endpoints)
{
    const NormPlan o = plan_of(kNormBc3, use_all);
    if (sizes == nullptr || n != o.sections())
        return fail(kInvalidArgument, "BC3 auto normalisation pick: 20 (fast) or 32 (all modes) sizes");
    uint64_t totals[kMaxCandidates];
    const AutoNormalizeChoice c = auto_normalize_pick(kNormBc3, use_all, sizes, kEveryEstimate, totals);
    for (int i = 0; out_totals != nullptr && i < o.candidates() && i < cap; ++i)
        out_totals[i] = totals[i];
    return store_choice(kOk, c, {out_alpha_mode, out_color_mode, out_decorrelation_mode, out_split_alpha_endpoints, out_split_colour_endpoints});
}

int32_t dxtlt_debug_bc3_auto_normalization_candidates_into_device(bool use_all, const void* d_input, size_t len, void* d_arena,
                                                                  uint64_t arena_bytes, void* hip_stream)
{
    if (len % 16 != 0)
        return fail(kInvalidArgument, "BC3 auto normalisation candidates: a whole number of blocks");
    if (len == 0)
        return kOk;
    if (d_input == nullptr || d_arena == nullptr || ((reinterpret_cast<uintptr_t>(d_input) | reinterpret_cast<uintptr_t>(d_arena)) & 15) != 0)
        return fail(kInvalidArgument, "BC3 auto normalisation candidates: input and arena on a 16-byte boundary");
    if (arena_bytes < dxtlt::auto_normalize_bc3_sections(use_all, len / 16).bytes)
        return fail(kInvalidArgument, "BC3 auto normalisation candidates: an arena smaller than auto_normalize_bc3_sections' bytes");
    HIP_TRY(dxtlt::launch_auto_normalize_candidates(dxtlt::kBc3, use_all, d_input, d_arena, len / 16, static_cast<hipStream_t>(hip_stream), nullptr),
            "candidate kernel launch");
    return kOk;
}

void dxtlt_debug_auto_normalization_last(uint64_t out[4])
{
    for (int i = 0; out != nullptr && i < 4; ++i)
        out[i] = t_last[i];
}

}  // extern "C"
