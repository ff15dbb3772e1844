// auto_transform.cpp -- transform_bcN_auto behind the C ABI: brute-force choice of transform settings with a
// caller-supplied size estimator.
//
// Reference behaviour kept exactly (paths under /root/reference/src/core/):
//   BC1  dxt-lossless-transform-bc1/src/transform/transform_auto.rs:200-270, test orders settings.rs:81-98
//   BC2  dxt-lossless-transform-bc2/src/transform/transform_auto.rs:196-,   test orders settings.rs:81-98
//   BC3  dxt-lossless-transform-bc3/src/transform/transform_auto.rs:196-294, test orders settings.rs:91-121
//   * one max_compressed_size query up front (len/2 for BC1, len/4 for BC2 and BC3), scratch allocated once;
//   * candidates are tried in the reference's order; each is a FULL transform followed by the estimator on the
//     endpoint section(s) only: BC1 [0, len/2); BC2 [len/2, len/2+len/4); BC3 alpha endpoints [0, 2N) plus
//     colour endpoints [len/2, len/2+4N), sizes added;
//   * strict `<` against the running best (first best wins), defaults as the initial best;
//   * if the best candidate was not the last one tried, the data is transformed once more with it.
//
// GPU shape: the input is uploaded once.  ONE fused kernel (auto_kernels.hip) reads it once and writes every endpoint
// section any candidate can show the estimator into a device arena -- 4 / 8 colour sections (YCoCg-R variant x
// split) and, for BC3, 2 alpha-endpoint sections cover all 4 / 8 / 16 candidates; the index sections are the same for
// every candidate and are never produced here (transform_auto.rs:245-256).  Per candidate only its section(s) travel
// back (half or a quarter of the buffer), into the output buffer at the offsets the reference estimates at, and the
// estimator -- on the CPU behind the callback, as in the reference -- is called in the reference's order with the
// reference's bytes.  One transform launch with the winning settings and one download of the whole result finish the
// call.  If the arena (2-4 x len) cannot be allocated the candidates are produced one full transform at a time, as in
// round 1 (same results, len x 2 of traffic per candidate).
//
//
// BC4 / BC5 (include/dxtlt_bc45.h) go through the same flow with two candidates, split_endpoints = false then true: both full
// transforms side by side in the arena (2 x len; one upload, two launches), the estimator is shown BC4 [0, 2N), BC5 red [0, 2N)
// then green [8N, 10N), added, and the winner's arena copy is what is downloaded.
//
// The flow is written once, transform_auto(), over where a candidate's sections come from (Source): the fused arena, the full
// transforms side by side, or one full transform per candidate through d_out.  Stated once and used by every route: the candidate
// orders (candidates_of), the section(s) of a transformed buffer the estimator is shown (shown_sections), the distinct sections of
// a candidate arena (dxtlt::auto_sections) with the ones a candidate is the sum of (sections_of) and the pick over them
// (auto_pick), and the estimator thread count (estimator_threads).
// The frame around the flows -- the drain guard, the estimator scratch, the device-call guard, the staged host call and this thread's
// auto state, which the other single-buffer auto calls (auto_normalize_api.cpp, pixel_auto_api.cpp) use too -- is auto_call.h; its
// non-template definitions are below.
//
// The built-in estimator (include/dxtlt_estimator.h, estimate_kernels.hip) is recognised by the identity of its function
// pointers and never called: auto_on_device() estimates every distinct section where the candidate kernel left it, with one
// launch, reads back 4 - 10 counters and applies the same order, additions and strict `<`.  No section crosses PCIe.  The same
// function serves dxtlt_transform_bcN_auto_device, where the input and the result stay on the device as well.
#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <exception>
#include <thread>
#include <vector>

#include "../../include/dxtlt_bc45.h"
#include "../../include/dxtlt_estimator.h"
#include "../../include/dxtlt_gfx950.h"
#include "auto_call.h"
#include "auto_launch.h"
#include "bcn_launch.h"

namespace {

struct Candidate {
    uint8_t mode;
    bool split_alpha;
    bool split_colour;
};

// bc1/bc2 settings.rs:81-86 and :89-98
constexpr Candidate kFast12[] = {{0, false, false}, {0, false, true}, {1, false, false}, {1, false, true}};
constexpr Candidate kAll12[] = {{2, false, false}, {0, false, false}, {0, false, true}, {3, false, false},
                            {3, false, true},  {2, false, true},  {1, false, false}, {1, false, true}};
// bc3 settings.rs:91-100 and :104-121  (variant, split_alphas, split_colours)
constexpr Candidate kFast3[] = {{1, true, false}, {1, true, true},  {0, true, false},  {0, false, true},
                            {0, true, true},  {1, false, true}, {0, false, false}, {1, false, false}};
constexpr Candidate kAll3[] = {{2, true, false},  {2, true, true},  {3, true, true},   {3, true, false},
                           {1, true, false},  {3, false, true}, {1, true, true},   {2, false, true},
                           {2, false, false}, {3, false, false}, {0, true, false}, {0, false, true},
                           {0, true, true},   {1, false, true}, {0, false, false}, {1, false, false}};

struct Order {
    const Candidate* order;
    int count;
    int defaults;   // index of the format's default settings: Bc1 / Bc2 {Variant1, split}, Bc3 {Variant1, split alphas, split colours};
                    // BC4 / BC5: candidate 0.  The initial best of the callback flow, with size SIZE_MAX.
};

Order candidates_of(int32_t format, bool use_all)
{
    static const Candidate k45[] = {{0, false, false}, {0, true, false}};   // split_endpoints = false, then true
    if (format >= 4)
        return {k45, 2, 0};
    if (format == 3)
        return use_all ? Order{kAll3, 16, 6} : Order{kFast3, 8, 1};
    return use_all ? Order{kAll12, 8, 7} : Order{kFast12, 4, 3};
}

constexpr bool is_default(const Candidate& c, bool bc3) { return c.mode == 1 && c.split_alpha == bc3 && c.split_colour; }
static_assert(is_default(kFast12[3], false) && is_default(kAll12[7], false) && is_default(kFast3[1], true) && is_default(kAll3[6], true),
              "candidates_of: the index of the default settings");

// The section(s) of a transformed buffer of `len` bytes the estimator is shown, in the order their sizes are added: BC1 the colour
// endpoints [0, len/2); BC2 [len/2, + len/4); BC3 alpha endpoints [0, 2N) then colour endpoints [len/2, + 4N); BC4 [0, 2N); BC5
// red [0, 2N) then green [8N, + 2N).
struct Shown {
    int count;
    size_t off[2], len[2];
};

Shown shown_sections(int32_t format, size_t len)
{
    switch (format) {
    case 1: return {1, {0, 0}, {len / 2, 0}};
    case 2: return {1, {len / 2, 0}, {len / 4, 0}};
    case 3: return {2, {0, len / 2}, {len / 8, len / 4}};
    case 4: return {1, {0, 0}, {len / 4, 0}};
    default: return {2, {0, len / 2}, {len / 8, len / 8}};
    }
}

// The distinct sections (indices into dxtlt::auto_sections) candidate c of `format` is the sum of, in shown_sections' order.
void sections_of(int32_t format, const Candidate& c, int* idx)
{
    const int sa = c.split_alpha ? 1 : 0, colour = c.mode * 2 + (c.split_colour ? 1 : 0);
    switch (format) {
    case 3: idx[0] = sa; idx[1] = 2 + colour; break;
    case 4: idx[0] = sa; break;
    case 5: idx[0] = sa; idx[1] = 2 + sa; break;
    default: idx[0] = colour; break;
    }
}

using dxtlt_host::EstimatorScratch;
using dxtlt_host::StreamDrain;

thread_local dxtlt_host::AutoThreadState t_auto;
thread_local uint32_t t_last_estimator_error = 0;   // dxtlt_debug_auto_last_estimator_error

uint32_t call_max(const DltSizeEstimator* est, size_t len, size_t* out)
{
    ++t_auto.estimator_callbacks;
    return est->MaxCompressedSize(est->Context, len, out);
}

uint32_t call_estimate(const DltSizeEstimator* est, const uint8_t* in, size_t len, uint8_t* scratch, size_t max_comp, size_t* out)
{
    ++t_auto.estimator_callbacks;
    return est->EstimateCompressedSize(est->Context, in, len, scratch, max_comp, out);
}

hipError_t download_section(void* dst, const void* src, size_t len, hipStream_t st)
{
    t_auto.section_bytes_downloaded += len;
    return hipMemcpyAsync(dst, src, len, hipMemcpyDeviceToHost, st);
}

// ---------------------------------------------------------------------------------------------------------------
// Opt-in: the estimator on several host threads (dxtlt_set_auto_estimator_threads).  The reference evaluates its
// candidates one after the other because each is a transform into the one output buffer; here every section a
// candidate can show the estimator already sits in the arena, so the estimator -- the hot loop of this call
// (transform/mod.rs:32-34: 265 MiB/s with zstd level 1, 1 GiB/s with LTU, one thread) -- can run on all of them at
// once.  And every DISTINCT section is estimated once: BC3's 8 / 16 candidates are 2 alpha-endpoint sections x 4 / 8
// colour sections = 6 / 10 estimator calls instead of 16 / 32.  Same candidates, same sizes, same order of
// comparison and strict `<`: the same choice and the same bytes as the sequential flow -- what changes is the
// sequence of callback invocations (concurrent, once per distinct section), which is why the caller has to ask for it:
// the callbacks must be safe to call from several threads at once with the same Context.
// ---------------------------------------------------------------------------------------------------------------
std::atomic<int> g_estimator_threads{1};
// per-thread cap on top of it (dxtlt_set_auto_estimator_threads_for_this_thread): 0 = none.  A binding whose estimator type
// makes no thread-safety promise (the Rust glue: `T: SizeEstimationOperations` without `Sync`) sets 1 around its call, so that
// its soundness does not rest on nobody in the process having called the process-wide setter.
thread_local int t_estimator_threads_cap = 0;
constexpr size_t kStageCapBytes = size_t(512) << 20;   // pinned staging per wave of sections (one section at least)

int estimator_threads()
{
    const int threads = g_estimator_threads.load(std::memory_order_relaxed);
    return t_estimator_threads_cap > 0 ? std::min(threads, t_estimator_threads_cap) : threads;
}

struct Section {
    const uint8_t* d_src;   // in the arena
    size_t len;
    size_t size = 0;        // the estimator's answer
    uint32_t rc = 0;        // the estimator's status
    size_t slot = 0;        // byte offset in the staging buffer of its wave
};

// Estimates every section; false = a HIP call failed (*hip_error).  Estimator failures are recorded per section.
bool estimate_sections_parallel(std::vector<Section>& sections, const DltSizeEstimator* est, size_t max_comp, int threads,
                                hipStream_t st, hipError_t* hip_error)
{
    size_t largest = 0;
    for (const Section& s : sections)
        largest = std::max(largest, (s.len + 255) & ~size_t(255));
    const size_t cap = std::max(largest, kStageCapBytes);
    size_t want = 0, run = 0;
    for (const Section& s : sections) {   // the largest wave the cap allows, in order
        const size_t b = (s.len + 255) & ~size_t(255);
        if (run + b > cap)
            run = 0;
        run += b;
        want = std::max(want, run);
    }
    uint8_t* stage = static_cast<uint8_t*>(t_auto.stage.get(want));
    if (stage == nullptr) {
        *hip_error = hipErrorOutOfMemory;
        return false;
    }
    threads = std::max(1, std::min<int>(threads, (int)sections.size()));
    std::vector<EstimatorScratch> scratch((size_t)threads);
    bool ok = true;
    for (EstimatorScratch& p : scratch)
        ok = p.allocate(max_comp) && ok;
    *hip_error = ok ? hipSuccess : hipErrorOutOfMemory;
    size_t first = 0;
    while (ok && first < sections.size()) {
        size_t last = first, used = 0;
        while (last < sections.size() && (last == first || used + ((sections[last].len + 255) & ~size_t(255)) <= cap)) {
            sections[last].slot = used;
            used += (sections[last].len + 255) & ~size_t(255);
            ++last;
        }
        for (size_t i = first; i < last && ok; ++i)
            if (sections[i].len) {
                *hip_error = download_section(stage + sections[i].slot, sections[i].d_src, sections[i].len, st);
                ok = *hip_error == hipSuccess;
            }
        if (ok) {
            *hip_error = hipStreamSynchronize(st);
            ok = *hip_error == hipSuccess;
        }
        if (!ok)
            break;
        std::atomic<size_t> next{first};
        auto worker = [&](int tid) {
            for (;;) {
                const size_t i = next.fetch_add(1);
                if (i >= last)
                    return;
                Section& s = sections[i];
                s.rc = est->EstimateCompressedSize(est->Context, stage + s.slot, s.len, scratch[(size_t)tid].ptr, max_comp, &s.size);
            }
        };
        // a thread that cannot be started (EAGAIN under a process limit) is simply not part of the pool: the sections are
        // handed out through `next`, so the threads that did start -- this one at least -- take all of them
        std::vector<std::thread> pool;
        for (int t = 1; t < threads; ++t) {
            try {
                pool.emplace_back(worker, t);
            } catch (const std::exception&) {
                break;
            }
        }
        worker(0);
        for (auto& t : pool)
            t.join();
        t_auto.estimator_callbacks += last - first;   // (the workers have counters of their own)
        first = last;
    }
    return ok;
}


// ---------------------------------------------------------------------------------------------------------------
// The built-in estimator: everything on the device.
// ---------------------------------------------------------------------------------------------------------------
// Chooses among the candidates of `format` (1..5) for the `len` > 0 bytes at d_in with the built-in estimator and leaves the
// transform with *best enqueued from d_in into d_out.  Enqueues on `st` and waits for it once, for the counters: when it returns
// nothing in flight reads or writes this thread's arena or counters any more (the pending transform reads d_in alone), so the
// thread's next auto call may use them at once, on any stream.  The same candidates, the same order, the same sums and strict `<`
// as the callback flow below.
int32_t auto_on_device(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all, hipStream_t st, Candidate* best)
{
    using namespace dxtlt_host;
    const Order o = candidates_of(format, use_all);
    const uint64_t blocks = len / (format == 1 || format == 4 ? 8 : 16);
    uint8_t* out8 = static_cast<uint8_t*>(d_out);
    const Shown shown = shown_sections(format, len);
    uint64_t sizes[kMaxCounters];
    uint64_t total[16];
    int last = -1;   // the candidate whose transform is in d_out
    int pick = 0;

    // BC1-3: the candidate kernel reads the input as 16-byte vectors; an input off a 16-byte boundary takes the no-arena route,
    // whose transform kernels take any alignment (one full transform per candidate instead of one read)
    const bool vector_aligned = (reinterpret_cast<uintptr_t>(d_in) & 15) == 0;
    const dxtlt::AutoSections distinct = dxtlt::auto_sections((dxtlt::Format)format, use_all, blocks);
    uint8_t* arena = nullptr;
    if (!t_auto.no_arena && (format >= 4 || vector_aligned))
        arena = static_cast<uint8_t*>(t_auto.arena.get(format >= 4 ? 2 * len : (size_t)distinct.bytes));
    if (arena != nullptr && format <= 3) {
        // one read of the input -> every distinct section, estimated where it lies
        HIP_TRY(dxtlt::launch_auto_candidates((dxtlt::Format)format, use_all, d_in, arena, blocks, st), "candidate kernel launch");
        dxtlt::EstimateSection secs[10];
        for (int k = 0; k < distinct.count; ++k)
            secs[k] = {arena + distinct.off[k], distinct.len[k]};
        if (int32_t rc = estimate_enqueue(secs, (size_t)distinct.count, st, 0))
            return rc;
        if (int32_t rc = estimate_read_back((size_t)distinct.count, st, sizes))
            return rc;
        pick = auto_pick(format, use_all, false, sizes, total);
    } else {
        // BC4 / BC5 with the arena: both transforms side by side (the winner is transformed once more, into d_out: a copy out of
        // the arena would still be reading it when this thread's next call fills it).  Without it: one full transform per
        // candidate into d_out, estimated there before the next one overwrites it (stream order); the counters come back once.
        for (int i = 0; i < o.count; ++i) {
            const Candidate c = o.order[i];
            uint8_t* dst = arena != nullptr ? arena + (size_t)i * len : out8;
            if (int32_t rc = enqueue(format, false, d_in, dst, blocks, dxtlt::Settings{c.mode, c.split_alpha, c.split_colour}, st))
                return rc;
            if (arena == nullptr)
                last = i;
            const dxtlt::EstimateSection secs[2] = {{dst + shown.off[0], shown.len[0]}, {dst + shown.off[1], shown.len[1]}};
            if (int32_t rc = estimate_enqueue(secs, (size_t)shown.count, st, (size_t)(i * 2)))
                return rc;
        }
        if (int32_t rc = estimate_read_back((size_t)o.count * 2, st, sizes))
            return rc;
        pick = auto_pick(format, use_all, true, sizes, total);
    }

    *best = o.order[pick];
    if (pick != last) {
        if (int32_t rc = enqueue(format, false, d_in, d_out, blocks, dxtlt::Settings{best->mode, best->split_alpha, best->split_colour}, st))
            return rc;
    }
    t_auto.set_last_totals(total, o.count);
    return kOk;
}

void report(const Candidate& c, dxtlt_host::AutoChoice* choice)
{
    choice->mode = c.mode;
    choice->split_alpha = c.split_alpha;
    choice->split_colour = c.split_colour;
    choice->estimator_error = 0;
}
}  // namespace

extern "C" void dxtlt_set_auto_estimator_threads(int32_t threads)
{
    g_estimator_threads.store(threads < 1 ? 1 : threads > 64 ? 64 : threads, std::memory_order_relaxed);
}

extern "C" int32_t dxtlt_get_auto_estimator_threads(void) { return g_estimator_threads.load(std::memory_order_relaxed); }

extern "C" int32_t dxtlt_set_auto_estimator_threads_for_this_thread(int32_t cap)
{
    const int32_t before = t_estimator_threads_cap;
    t_estimator_threads_cap = cap < 0 ? 0 : cap > 64 ? 64 : cap;
    return before;
}

void dxtlt_host::release_auto_thread_arena()
{
    t_auto.arena.release();
    t_auto.stage.release();
    release_estimate_thread_counters();
    release_batch_auto_thread_buffers();
}

int dxtlt_host::auto_candidate_order(int32_t format, bool use_all, AutoChoice* out)
{
    const Order o = candidates_of(format, use_all);
    for (int i = 0; i < o.count; ++i)
        out[i] = AutoChoice{o.order[i].mode, o.order[i].split_alpha, o.order[i].split_colour, 0};
    return o.count;
}

int dxtlt_host::auto_pick(int32_t format, bool use_all, bool per_candidate, const uint64_t* sizes, uint64_t* total)
{
    const Order o = candidates_of(format, use_all);
    const bool two_shown = format == 3 || format == 5;
    for (int i = 0; i < o.count; ++i) {
        int idx[2] = {2 * i, 2 * i + 1};
        if (!per_candidate)
            sections_of(format, o.order[i], idx);
        total[i] = sizes[idx[0]] + (two_shown ? sizes[idx[1]] : 0);
    }
    int pick = 0;
    for (int i = 1; i < o.count; ++i)
        if (total[i] < total[pick])   // strict: the first best wins
            pick = i;
    return pick;
}

dxtlt_host::AutoThreadState& dxtlt_host::auto_state() { return t_auto; }

void dxtlt_host::AutoArena::release()
{
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
    device = -1;
}

void* dxtlt_host::AutoArena::get(size_t bytes)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess)
        return nullptr;
    if (dev != device || bytes > cap) {
        release();
        if (hipMalloc(&ptr, bytes) != hipSuccess) {
            (void)hipGetLastError();
            ptr = nullptr;
            return nullptr;
        }
        cap = bytes;
        device = dev;
    }
    return ptr;
}

void dxtlt_host::AutoHostStage::release()
{
    if (ptr) (void)hipHostFree(ptr);
    ptr = nullptr;
    cap = 0;
}

void* dxtlt_host::AutoHostStage::get(size_t bytes)
{
    if (bytes > cap) {
        release();
        if (hipHostMalloc(&ptr, bytes, hipHostMallocDefault) != hipSuccess) {
            (void)hipGetLastError();
            ptr = nullptr;
            return nullptr;
        }
        cap = bytes;
    }
    return ptr;
}

int32_t dxtlt_host::auto_device_preconditions(hipStream_t stream)
{
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0)
        return fail(kNoDevice, "no HIP device available (this library has no CPU fallback)", e);
    if (stream_is_capturing(stream))
        return fail(kInvalidArgument, "the auto transforms read their estimates back and wait for the stream: not capturable");
    return kOk;
}

// Where the sections of the callback flow's candidates come from, and with them how the winner reaches the output.
enum class Source {
    kFused,        // BC1-3: every distinct section in the arena from one read (launch_auto_candidates); the winner is transformed once
    kSideBySide,   // BC4 / BC5: both full transforms in the arena (2 x len); the winner's copy is downloaded
    kOneByOne,     // no arena, or nothing to transform: one full transform per candidate into d_out, again for the winner unless it
                   // was the last one tried
};

int32_t dxtlt_host::transform_auto(int32_t format, const uint8_t* in, uint8_t* out, size_t len,
                                   const DltSizeEstimator* est, bool use_all, AutoChoice* choice)
{
    t_auto.last_total_count = 0;   // whatever this call does next: no totals of an earlier one
    if (format < 1 || format > 5)
        return fail(kInvalidArgument, "format must be 1..5 (BC1..BC5)");
    const size_t block = format == 1 || format == 4 ? 8 : 16;
    if (len % block != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");
    if (est == nullptr || est->MaxCompressedSize == nullptr || est->EstimateCompressedSize == nullptr || choice == nullptr)
        return fail(kInvalidArgument, "NULL estimator / choice");
    if (len > 0 && (in == nullptr || out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    use_all = use_all && format <= 3;

    t_auto.section_bytes_downloaded = t_auto.estimator_callbacks = 0;
    if (is_builtin_estimator(est)) {   // never called: one upload, everything on the device, one download
        Candidate best = candidates_of(format, use_all).order[0];   // every estimate of an empty buffer is 0: the first candidate stays
        if (len > 0) {
            const int32_t rc = auto_staged_call(in, out, len, [&](const void* d_in, void* d_out, hipStream_t st) {
                return auto_on_device(format, d_in, d_out, len, use_all, st, &best);
            });
            if (rc != kOk) {
                t_auto.last_total_count = 0;
                return rc;
            }
        }
        report(best, choice);
        return kOk;
    }

    const uint64_t blocks = len / block;
    const Order o = candidates_of(format, use_all);
    const Shown shown = shown_sections(format, len);
    choice->estimator_error = 0;
    auto fail_estimate = [&](uint32_t bad, const char* what) {
        choice->estimator_error = bad;
        return fail(kEstimator, what);
    };

    size_t max_comp = 0;   // one query: len/2 for BC1, len/4 for BC2 / BC3, 2N for BC4 / BC5 -- the longest section shown
    if (uint32_t bad = call_max(est, std::max(shown.len[0], shown.len[1]), &max_comp))
        return fail_estimate(bad, "size estimator: max_compressed_size failed");
    EstimatorScratch scratch;
    if (!scratch.allocate(max_comp))
        return fail(kAllocation, "estimator scratch allocation failed");

    void *d_in = nullptr, *d_out = nullptr;
    StreamDrain drain;
    hipStream_t& st = drain.stream;
    uint8_t* arena = nullptr;
    dxtlt::AutoSections distinct{};
    if (len > 0) {
        if (int32_t rc = acquire_staging(len, &d_in, &d_out, &st))
            return rc;
        drain.armed = true;
        HIP_TRY(hipMemcpyAsync(d_in, in, len, hipMemcpyHostToDevice, st), "H2D copy");
        if (format >= 4 && !t_auto.no_arena) {
            arena = static_cast<uint8_t*>(t_auto.arena.get(2 * len));
            for (int i = 0; i < o.count && arena != nullptr; ++i)
                if (int32_t rc = enqueue(format, false, d_in, arena + (size_t)i * len, blocks, dxtlt::Settings{0, o.order[i].split_alpha, false}, st))
                    return rc;
        } else if (format <= 3 && !t_auto.no_arena) {
            distinct = dxtlt::auto_sections((dxtlt::Format)format, use_all, blocks);
            arena = static_cast<uint8_t*>(t_auto.arena.get((size_t)distinct.bytes));
            if (arena != nullptr)
                HIP_TRY(dxtlt::launch_auto_candidates((dxtlt::Format)format, use_all, d_in, arena, blocks, st), "candidate kernel launch");
        }
    }
    const Source source = arena == nullptr ? Source::kOneByOne : format >= 4 ? Source::kSideBySide : Source::kFused;
    // section h of candidate i where the source holds it on the device (kOneByOne: once its transform has been enqueued)
    auto device_section = [&](int i, int h) -> const uint8_t* {
        if (source == Source::kFused) {
            int idx[2];
            sections_of(format, o.order[i], idx);
            return arena + distinct.off[idx[h]];
        }
        return (source == Source::kSideBySide ? arena + (size_t)i * len : static_cast<const uint8_t*>(d_out)) + shown.off[h];
    };

    int best = o.defaults, last = -1;   // last: the candidate whose transform is in d_out (kOneByOne)
    size_t best_size = SIZE_MAX;
    const int est_threads = estimator_threads();
    if (est_threads > 1 && arena != nullptr) {
        // every distinct section (kFused) or every section of every candidate (kSideBySide) at once; combined in the sequential
        // order, so that the failure reported is the one the sequential flow meets first
        std::vector<Section> sections;
        for (int k = 0; k < distinct.count; ++k)
            sections.push_back(Section{arena + distinct.off[k], (size_t)distinct.len[k]});
        for (int i = 0; i < o.count && source == Source::kSideBySide; ++i)
            for (int h = 0; h < shown.count; ++h)
                sections.push_back(Section{device_section(i, h), shown.len[h]});
        hipError_t herr = hipSuccess;
        if (!estimate_sections_parallel(sections, est, max_comp, est_threads, st, &herr))
            return fail(kDevice, "parallel estimation (staging / download)", herr == hipSuccess ? hipErrorUnknown : herr);
        for (int i = 0; i < o.count; ++i) {
            int idx[2] = {i * shown.count, i * shown.count + 1};
            if (source == Source::kFused)
                sections_of(format, o.order[i], idx);
            size_t total = 0;
            for (int h = 0; h < shown.count; ++h) {
                const Section& sec = sections[(size_t)idx[h]];
                if (sec.rc != 0)
                    return fail_estimate(sec.rc, "size estimator: estimate_compressed_size failed");
                total += sec.size;
            }
            if (total < best_size) {
                best_size = total;
                best = i;
            }
        }
    } else {
        // kFused: the sections of candidate i + 1 travel into the other half of a pinned staging buffer while the estimator works on
        // candidate i -- the reference's sequence of calls and bytes, minus the wait for every download (and minus pageable-memory
        // copies); the estimator is shown the staged bytes.  Otherwise, or when a slot would pass 512 MiB or cannot be allocated, a
        // candidate's sections are downloaded into the output buffer at the offsets the reference estimates at, and waited for.
        const size_t second = shown.count == 2 ? (shown.len[0] + 255) & ~size_t(255) : 0;   // of a slot's second section
        const size_t slot_bytes = second + ((shown.len[shown.count - 1] + 255) & ~size_t(255));
        uint8_t* stage = nullptr;
        if (source == Source::kFused && slot_bytes <= kStageCapBytes)
            stage = static_cast<uint8_t*>(t_auto.stage.get(2 * slot_bytes));
        auto download = [&](int i, uint8_t* first_to, uint8_t* second_to) -> hipError_t {
            hipError_t e = download_section(first_to, device_section(i, 0), shown.len[0], st);
            if (e == hipSuccess && shown.count == 2)
                e = download_section(second_to, device_section(i, 1), shown.len[1], st);
            return e;
        };
        auto slot = [&](int i) { return stage + (size_t)(i & 1) * slot_bytes; };
        auto stage_candidate = [&](int i) { return download(i, slot(i), slot(i) + second); };
        if (stage != nullptr)
            HIP_TRY(stage_candidate(0), "D2H candidate sections");

        for (int i = 0; i < o.count; ++i) {
            const Candidate c = o.order[i];
            const uint8_t* seen[2] = {out + shown.off[0], out + shown.off[1]};
            if (stage != nullptr) {
                HIP_TRY(hipStreamSynchronize(st), "stream synchronize");   // candidate i has arrived
                if (i + 1 < o.count)
                    HIP_TRY(stage_candidate(i + 1), "D2H candidate sections");
                seen[0] = slot(i);
                seen[1] = slot(i) + second;
            } else if (len > 0) {
                if (source == Source::kOneByOne) {
                    if (int32_t rc = enqueue(format, false, d_in, d_out, blocks, dxtlt::Settings{c.mode, c.split_alpha, c.split_colour}, st))
                        return rc;
                    last = i;
                }
                HIP_TRY(download(i, out + shown.off[0], out + shown.off[1]), "D2H endpoint sections");
                HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
            }
            size_t total = 0;
            for (int h = 0; h < shown.count; ++h) {   // a candidate's second estimate is not asked for when its first fails
                size_t part = 0;
                if (uint32_t bad = call_estimate(est, seen[h], shown.len[h], scratch.ptr, max_comp, &part))
                    return fail_estimate(bad, "size estimator: estimate_compressed_size failed");
                total += part;
            }
            if (total < best_size) {
                best_size = total;
                best = i;
            }
        }
    }

    const Candidate won = o.order[best];
    if (len > 0) {
        if (source == Source::kFused || (source == Source::kOneByOne && best != last))
            if (int32_t rc = enqueue(format, false, d_in, d_out, blocks, dxtlt::Settings{won.mode, won.split_alpha, won.split_colour}, st))
                return rc;
        const void* result = source == Source::kSideBySide ? static_cast<const void*>(arena + (size_t)best * len) : d_out;
        HIP_TRY(hipMemcpyAsync(out, result, len, hipMemcpyDeviceToHost, st), "D2H result");
        HIP_TRY(hipStreamSynchronize(st), "stream synchronize");
        drain.armed = false;
    }
    choice->mode = won.mode;
    choice->split_alpha = won.split_alpha;
    choice->split_colour = won.split_colour;
    return kOk;
}

int32_t dxtlt_host::transform_auto_device(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all, hipStream_t st,
                                          AutoChoice* choice)
{
    t_auto.last_total_count = 0;   // whatever this call does next: no totals of an earlier one
    if (format < 1 || format > 5)
        return fail(kInvalidArgument, "format must be 1..5 (BC1..BC5)");
    if (len % (format == 1 || format == 4 ? 8 : 16) != 0)
        return fail(kInvalidLength, "len is not a multiple of the block size");
    if (choice == nullptr)
        return fail(kInvalidArgument, "NULL choice");
    if (len > 0 && (d_in == nullptr || d_out == nullptr))
        return fail(kInvalidArgument, "NULL buffer with len > 0");
    t_auto.section_bytes_downloaded = t_auto.estimator_callbacks = 0;
    use_all = use_all && format <= 3;
    Candidate best = candidates_of(format, use_all).order[0];
    if (len > 0)
        if (int32_t rc = auto_device_call(st, [&] { return auto_on_device(format, d_in, d_out, len, use_all, st, &best); }))
            return rc;
    report(best, choice);
    return kOk;
}

namespace {

// the choice of a successful call through the out-parameters of a C entry point, every one of which may be NULL
int32_t store_choice(int32_t rc, const dxtlt_host::AutoChoice& c, uint8_t* mode, bool* split_alpha, bool* split_colour)
{
    if (rc == DXTLT_OK) {
        dxtlt_host::store_if(mode, c.mode);
        dxtlt_host::store_if(split_alpha, c.split_alpha);
        dxtlt_host::store_if(split_colour, c.split_colour);
    }
    return rc;
}

int32_t auto_host(int32_t format, const uint8_t* in, uint8_t* out, size_t len, const DltSizeEstimator* estimator, bool use_all,
                  uint8_t* mode, bool* split_alpha, bool* split_colour, uint32_t* estimator_error)
{
    dxtlt_host::AutoChoice c{};
    const int32_t rc = dxtlt_host::transform_auto(format, in, out, len, estimator, use_all, &c);
    t_last_estimator_error = c.estimator_error;
    dxtlt_host::store_if(estimator_error, c.estimator_error);
    return store_choice(rc, c, mode, split_alpha, split_colour);
}

int32_t auto_device(int32_t format, const void* d_in, void* d_out, size_t len, bool use_all, void* hip_stream, uint8_t* mode,
                    bool* split_alpha, bool* split_colour)
{
    dxtlt_host::AutoChoice c{};
    const int32_t rc = dxtlt_host::transform_auto_device(format, d_in, d_out, len, use_all, static_cast<hipStream_t>(hip_stream), &c);
    return store_choice(rc, c, mode, split_alpha, split_colour);
}

}  // namespace

extern "C" {

// ---- include/dxtlt_gfx950.h, include/dxtlt_bc45.h: host pointers, the caller's estimator (split_endpoints travels as split_alpha) ----
int32_t dxtlt_transform_bc1_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                 const DltSizeEstimator* estimator, bool use_all_decorrelation_modes,
                                 uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                 uint32_t* out_estimator_error)
{
    return auto_host(1, input_ptr, output_ptr, len, estimator, use_all_decorrelation_modes, out_decorrelation_mode, nullptr,
                     out_split_colour_endpoints, out_estimator_error);
}

int32_t dxtlt_transform_bc2_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                 const DltSizeEstimator* estimator, bool use_all_decorrelation_modes,
                                 uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints,
                                 uint32_t* out_estimator_error)
{
    return auto_host(2, input_ptr, output_ptr, len, estimator, use_all_decorrelation_modes, out_decorrelation_mode, nullptr,
                     out_split_colour_endpoints, out_estimator_error);
}

int32_t dxtlt_transform_bc3_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len,
                                 const DltSizeEstimator* estimator, bool use_all_decorrelation_modes,
                                 uint8_t* out_decorrelation_mode, bool* out_split_alpha_endpoints,
                                 bool* out_split_colour_endpoints, uint32_t* out_estimator_error)
{
    return auto_host(3, input_ptr, output_ptr, len, estimator, use_all_decorrelation_modes, out_decorrelation_mode,
                     out_split_alpha_endpoints, out_split_colour_endpoints, out_estimator_error);
}

int32_t dxtlt_transform_bc4_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, const DltSizeEstimator* estimator,
                                 bool* out_split_endpoints)
{
    return auto_host(4, input_ptr, output_ptr, len, estimator, false, nullptr, out_split_endpoints, nullptr, nullptr);
}

int32_t dxtlt_transform_bc5_auto(const uint8_t* input_ptr, uint8_t* output_ptr, size_t len, const DltSizeEstimator* estimator,
                                 bool* out_split_endpoints)
{
    return auto_host(5, input_ptr, output_ptr, len, estimator, false, nullptr, out_split_endpoints, nullptr, nullptr);
}

// ---- include/dxtlt_estimator.h: device pointers, the built-in estimator ------------------------------------------------------
int32_t dxtlt_transform_bc1_auto_device(const void* d_input, void* d_output, size_t len, bool use_all_decorrelation_modes,
                                        void* hip_stream, uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints)
{
    return auto_device(1, d_input, d_output, len, use_all_decorrelation_modes, hip_stream, out_decorrelation_mode, nullptr,
                       out_split_colour_endpoints);
}

int32_t dxtlt_transform_bc2_auto_device(const void* d_input, void* d_output, size_t len, bool use_all_decorrelation_modes,
                                        void* hip_stream, uint8_t* out_decorrelation_mode, bool* out_split_colour_endpoints)
{
    return auto_device(2, d_input, d_output, len, use_all_decorrelation_modes, hip_stream, out_decorrelation_mode, nullptr,
                       out_split_colour_endpoints);
}

int32_t dxtlt_transform_bc3_auto_device(const void* d_input, void* d_output, size_t len, bool use_all_decorrelation_modes,
                                        void* hip_stream, uint8_t* out_decorrelation_mode, bool* out_split_alpha_endpoints,
                                        bool* out_split_colour_endpoints)
{
    return auto_device(3, d_input, d_output, len, use_all_decorrelation_modes, hip_stream, out_decorrelation_mode,
                       out_split_alpha_endpoints, out_split_colour_endpoints);
}

int32_t dxtlt_transform_bc4_auto_device(const void* d_input, void* d_output, size_t len, bool use_all_decorrelation_modes,
                                        void* hip_stream, bool* out_split_endpoints)
{
    return auto_device(4, d_input, d_output, len, use_all_decorrelation_modes, hip_stream, nullptr, out_split_endpoints, nullptr);
}

int32_t dxtlt_transform_bc5_auto_device(const void* d_input, void* d_output, size_t len, bool use_all_decorrelation_modes,
                                        void* hip_stream, bool* out_split_endpoints)
{
    return auto_device(5, d_input, d_output, len, use_all_decorrelation_modes, hip_stream, nullptr, out_split_endpoints, nullptr);
}

void dxtlt_debug_auto_last_estimation(uint64_t* out_section_bytes_downloaded, uint64_t* out_estimator_callbacks)
{
    dxtlt_host::store_if(out_section_bytes_downloaded, t_auto.section_bytes_downloaded);
    dxtlt_host::store_if(out_estimator_callbacks, t_auto.estimator_callbacks);
}

int32_t dxtlt_debug_auto_last_totals(uint64_t* out_totals, int32_t cap)
{
    for (int i = 0; out_totals != nullptr && i < t_auto.last_total_count && i < cap; ++i)
        out_totals[i] = t_auto.last_totals[i];
    return t_auto.last_total_count;
}

void dxtlt_debug_auto_use_arena(int32_t on) { t_auto.no_arena = on == 0; }

uint32_t dxtlt_debug_auto_last_estimator_error(void) { return t_last_estimator_error; }

int32_t dxtlt_debug_auto_candidates_device(int32_t format, bool use_all_decorrelation_modes, const void* d_input, size_t len,
                                           void* hip_stream)
{
    using namespace dxtlt_host;
    if (format < 1 || format > 3 || d_input == nullptr || len == 0 || len % (format == 1 ? 8 : 16) != 0)
        return fail(kInvalidArgument, "format 1..3, a non-empty whole number of blocks");
    const uint64_t blocks = len / (format == 1 ? 8 : 16);
    void* arena = t_auto.arena.get((size_t)dxtlt::auto_sections((dxtlt::Format)format, use_all_decorrelation_modes, blocks).bytes);
    if (arena == nullptr)
        return fail(kDevice, "candidate arena allocation failed", hipErrorOutOfMemory);
    HIP_TRY(dxtlt::launch_auto_candidates((dxtlt::Format)format, use_all_decorrelation_modes, d_input, arena, blocks,
                                          static_cast<hipStream_t>(hip_stream)),
            "candidate kernel launch");
    return kOk;
}

int32_t dxtlt_debug_auto_candidates_into_device(int32_t format, bool use_all_decorrelation_modes, const void* d_input, size_t len,
                                                void* d_arena, uint64_t arena_bytes, void* hip_stream)
{
    using namespace dxtlt_host;
    if (format < 1 || format > 3 || len % (format == 1 ? 8 : 16) != 0)
        return fail(kInvalidArgument, "auto candidates: format 1..3, a whole number of blocks");
    if (len == 0)
        return kOk;
    if (d_input == nullptr || d_arena == nullptr || ((reinterpret_cast<uintptr_t>(d_input) | reinterpret_cast<uintptr_t>(d_arena)) & 15) != 0)
        return fail(kInvalidArgument, "auto candidates: input and arena on a 16-byte boundary");
    const uint64_t blocks = len / (format == 1 ? 8 : 16);
    if (arena_bytes < dxtlt::auto_sections((dxtlt::Format)format, use_all_decorrelation_modes, blocks).bytes)
        return fail(kInvalidArgument, "auto candidates: an arena smaller than auto_sections' bytes");
    HIP_TRY(dxtlt::launch_auto_candidates((dxtlt::Format)format, use_all_decorrelation_modes, d_input, d_arena, blocks,
                                          static_cast<hipStream_t>(hip_stream)),
            "candidate kernel launch");
    return kOk;
}

}  // extern "C"
